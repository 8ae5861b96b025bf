"""FP8 (e4m3) projection weights without a GPU: the quantiser, Hugging Face FP8 checkpoint
directories through ``models.loader`` (synthetic ones, written here with safetensors), TP
sharding of codes and scales, and an fp8 ``LlamaModel`` served by ``LLMEngine`` on the CPU
through ``ops.reference.linear_w8``."""
from __future__ import annotations

import json
import os

import pytest
import torch
from safetensors.torch import save_file

from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaConfig, LlamaModel, PRESETS
from langstream_amd.models.loader import (checkpoint_weights_dtype, convert_hf_llama, llama_config_from_hf,
                                          load_packed, shard_llama)
from langstream_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn


# ------------------------------------------------------------------------------ quantiser
def _rows():
    g = torch.Generator().manual_seed(11)
    K = 512
    rows = [torch.randn(K, generator=g), torch.randn(K, generator=g) * 1e3, torch.randn(K, generator=g) * 1e-3]
    r = torch.randn(K, generator=g)
    r[7], r[300] = r.abs().max() * 2, -r.abs().max() * 2     # +amax and -amax in one row
    rows += [r, torch.zeros(K)]
    r = torch.randn(K, generator=g) * 1e-3                   # most of the row in the subnormal codes
    r[0] = 50.0
    rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_weight_fp8_bound_and_fixpoint(dtype):
    w = _rows().to(dtype)
    codes, s = ref.quantize_weight_fp8(w)
    assert codes.dtype == FP8 and codes.shape == w.shape and codes.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (w.shape[0],) and bool((s > 0).all())
    cf = codes.float()
    assert bool(torch.isfinite(cf).all()), "no NaN codes"
    wd = w.double()
    # s = amax / 448 in f32; 1 for the all-zero row
    amax = w.float().abs().amax(1)
    assert torch.equal(s, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)))
    assert float(s[4]) == 1.0 and not bool(cf[4].any())
    # half an e4m3 step (3 mantissa bits) relative, half a subnormal step (2^-9 code units) absolute
    err = (cf.double() * s.double()[:, None] - wd).abs()
    bound = 2.0 ** -4 * wd.abs() + 2.0 ** -10 * s.double()[:, None]
    assert bool((err <= bound).all()), (err / bound).max().item()
    # the row maximum lands on +-448
    assert bool((cf.abs().amax(1)[[0, 1, 2, 3, 5]] == 448.0).all())
    assert float(cf[3, 7]) == 448.0 and float(cf[3, 300]) == -448.0
    # a fixpoint: quantising code * s gives the same codes
    again, s2 = ref.quantize_weight_fp8(ref.dequantize_weight_fp8(codes, s))
    assert torch.equal(again.view(torch.uint8), codes.view(torch.uint8))
    assert bool(((s2 - s).abs() <= 2.0 ** -22 * s).all())


def test_linear_w8_reference_formula():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, 192, generator=g).to(torch.bfloat16)
    codes, s = ref.quantize_weight_fp8(torch.randn(64, 192, generator=g))
    want = (x.double() @ codes.double().t()) * s.double()
    got64 = ref.linear_w8(x, codes, s, dtype=torch.float64)
    assert got64.dtype == torch.float64 and torch.equal(got64, want)
    got = ref.linear_w8(x, codes, s)
    assert got.dtype == torch.bfloat16
    assert bool(((got.double() - want).abs() <= 2.0 ** -7 * want.abs() + 1e-6).all())
    assert torch.equal(ops.linear_w8(x, codes, s), got)             # CPU tensors dispatch to the reference
    xf = x.float()
    assert ref.linear_w8(xf, codes, s).dtype == torch.float32


# ------------------------------------------------------------------------------ checkpoints
SHAPE = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, max_position_embeddings=2048, tie_word_embeddings=False, model_type="llama",
             rms_norm_eps=1e-5, rope_theta=10000.0, bos_token_id=1, eos_token_id=2)
PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
        "mlp.up_proj", "mlp.down_proj")


def _hf_tensors(seed=0):
    """A random f32 Llama checkpoint in Hugging Face names (the shape of llama-tiny)."""
    g = torch.Generator().manual_seed(seed)
    H, F, V, D = 256, 512, 512, 64
    rn = lambda *sh: torch.randn(*sh, generator=g) * 0.05  # noqa: E731
    t = {"model.embed_tokens.weight": rn(V, H), "model.norm.weight": 1 + rn(H), "lm_head.weight": rn(V, H)}
    for i in range(2):
        p = f"model.layers.{i}."
        t[p + "self_attn.q_proj.weight"] = rn(4 * D, H)
        t[p + "self_attn.k_proj.weight"] = rn(2 * D, H) * 3.0      # different ranges: different per-tensor scales
        t[p + "self_attn.v_proj.weight"] = rn(2 * D, H) * 0.3
        t[p + "self_attn.o_proj.weight"] = rn(H, 4 * D)
        t[p + "mlp.gate_proj.weight"] = rn(F, H)
        t[p + "mlp.up_proj.weight"] = rn(F, H) * 2.0
        t[p + "mlp.down_proj.weight"] = rn(H, F)
        t[p + "input_layernorm.weight"] = 1 + rn(H)
        t[p + "post_attention_layernorm.weight"] = 1 + rn(H)
    return t


def _quantize_hf(t, mode, scale_dtype=torch.float32, input_scale=None):
    """Every ``*_proj.weight`` as float8_e4m3fn with a sibling ``weight_scale``: mode "tensor0"
    (0-d scalar), "tensor1" ([1]), "channel" ([N]) or "channel2" ([N, 1])."""
    out = {}
    for k, v in t.items():
        if not (k.endswith("_proj.weight")):
            out[k] = v
            continue
        if mode.startswith("tensor"):
            s = (v.abs().max() / 448.0).to(scale_dtype)
            codes = (v / s.float()).clamp(-448, 448).to(FP8)
            s = s.reshape(()) if mode == "tensor0" else s.reshape(1)
        else:
            s = (v.abs().amax(1) / 448.0).to(scale_dtype)
            codes = (v / s.float()[:, None]).clamp(-448, 448).to(FP8)
            s = s if mode == "channel" else s[:, None]
        out[k] = codes
        out[k + "_scale"] = s.contiguous()
        if input_scale:
            out[k[:-len("weight")] + input_scale] = torch.tensor([1200.0] if input_scale.endswith("ub") else 0.02)
    return out


def _write(path, tensors, quant_cfg=None, **cfg_over):
    os.makedirs(path, exist_ok=True)
    cfg = dict(SHAPE, **cfg_over)
    if quant_cfg is not None:
        cfg["quantization_config"] = quant_cfg
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in tensors.items()}, os.path.join(path, "model.safetensors"))
    return str(path)


def _dequant_hf(q):
    """The f32 checkpoint an fp8 one stands for: code * scale per projection."""
    out = {}
    for k, v in q.items():
        if k.endswith(("weight_scale", "input_scale", "input_scale_ub")):
            continue
        if v.dtype == FP8:
            s = q[k + "_scale"].float().reshape(-1)
            v = v.float() * (s[:, None] if s.numel() > 1 else s)
        out[k] = v
    return out


def _prefill_logits(model, ids):
    from langstream_amd.models.llama import AttnMeta
    T = len(ids)
    kv = [ops.new_kv_cache(4, model.hkv, model.cfg.head_dim, "cpu", torch.float32) for _ in model.layers]
    meta = AttnMeta(positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T, dtype=torch.int64),
                    num_decode=0, num_prefill_tokens=T, p_block_tables=torch.arange(4, dtype=torch.int32)[None],
                    q_start=torch.tensor([0], dtype=torch.int32), q_len=torch.tensor([T], dtype=torch.int32),
                    ctx_len=torch.tensor([T], dtype=torch.int32), tiles=ops.prefill_tiles([T], 1))
    return model.forward_logits(torch.tensor(ids, dtype=torch.int32), meta, kv)


IDS = [int(t) for t in torch.randint(3, 512, (37,), generator=torch.Generator().manual_seed(3))]

CT_CONFIG = {"quant_method": "compressed-tensors", "format": "float-quantized", "kv_cache_scheme": None,
             "ignore": ["lm_head"],
             "config_groups": {"group_0": {"targets": ["Linear"],
                                           "weights": {"num_bits": 8, "type": "float", "strategy": "channel",
                                                       "dynamic": False, "symmetric": True},
                                           "input_activations": {"num_bits": 8, "type": "float", "strategy": "token",
                                                                 "dynamic": True}}}}


@pytest.mark.parametrize("mode,scale_dtype,input_scale,qcfg", [
    ("tensor0", torch.float32, "input_scale", dict(CT_CONFIG)),
    ("tensor1", torch.bfloat16, None, None),
    ("channel", torch.float16, None, None),
    ("channel2", torch.float32, "input_scale_ub", {"quant_method": "fbgemm_fp8", "activation_scale_ub": 1200.0,
                                                  "modules_to_not_convert": ["lm_head"]}),
])
def test_fp8_checkpoint_directory_loads(tmp_path, mode, scale_dtype, input_scale, qcfg, caplog):
    """Scalar, [1], [N] and [N, 1] scales in f32 / bf16 / f16; q, k and v carry their own
    per-tensor scales in the rows of the fused qkv_s; activation scales are dropped with one
    log line; the loaded fp8 model computes what the f32 model of code * scale computes."""
    q = _quantize_hf(_hf_tensors(), mode, scale_dtype, input_scale)
    path = _write(tmp_path / "fp8", q, qcfg)
    cfg = llama_config_from_hf(path)
    with caplog.at_level("INFO", logger="langstream_amd.models.loader"):
        sd = load_packed(path)
    lines = [r for r in caplog.records if "activation-scale" in r.getMessage()]
    assert len(lines) == (1 if input_scale else 0)
    assert checkpoint_weights_dtype(sd) == "fp8"
    assert sd["lm_head"].dtype == torch.float32 and sd["embed"].dtype == torch.float32
    for i in range(2):
        p = f"model.layers.{i}.self_attn."
        qs = sd[f"layers.{i}.qkv_s"]
        assert qs.dtype == torch.float32 and qs.shape == (512,) and sd[f"layers.{i}.qkv_w"].dtype == FP8
        for nm, lo, hi in (("q", 0, 256), ("k", 256, 384), ("v", 384, 512)):
            want = q[p + nm + "_proj.weight_scale"].float().reshape(-1)
            assert torch.equal(qs[lo:hi], want.expand(hi - lo) if want.numel() == 1 else want), (i, nm)
            assert torch.equal(sd[f"layers.{i}.qkv_w"][lo:hi].view(torch.uint8),
                               q[p + nm + "_proj.weight"].view(torch.uint8))
        if mode.startswith("tensor"):
            assert len({float(qs[0]), float(qs[256]), float(qs[384])}) == 3
        assert sd[f"layers.{i}.gate_up_s"].shape == (1024,) and sd[f"layers.{i}.down_s"].shape == (256,)
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="fp8")
    model.load_state_dict(sd)
    wide = LlamaModel(cfg, device="cpu", dtype=torch.float32)
    wide.load_state_dict(convert_hf_llama(_dequant_hf(q), cfg))
    err = (_prefill_logits(model, IDS) - _prefill_logits(wide, IDS)).abs().max().item()
    assert err <= 1e-4, err
    # codes into a bf16 model: an error that names the tensor
    with pytest.raises(ValueError, match=r"layers\.0\.qkv_w"):
        LlamaModel(cfg, device="cpu", dtype=torch.float32).load_state_dict(sd)


def test_wide_checkpoint_into_fp8_model_is_quantised():
    """A bf16 / f32 state dict loaded into an fp8 model is quantised with quantize_weight_fp8."""
    cfg = PRESETS["llama-tiny"]
    src = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=3)
    dst = LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="fp8", seed=9)
    dst.load_state_dict(src.state_dict())
    for a, b in zip(src.layers, dst.layers):
        for n in ("qkv", "o", "gate_up", "down"):
            codes, s = ref.quantize_weight_fp8(getattr(a, n + "_w"))
            assert torch.equal(getattr(b, n + "_w").view(torch.uint8), codes.view(torch.uint8))
            assert torch.equal(getattr(b, n + "_s"), s)
    sd = dst.state_dict()
    assert {"layers.1.qkv_s", "layers.1.o_s", "layers.1.gate_up_s", "layers.1.down_s"} <= set(sd)
    # its own state dict round-trips, codes and scales
    again = LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="fp8", seed=1)
    again.load_state_dict(sd)
    assert torch.equal(again.layers[1].down_w.view(torch.uint8), dst.layers[1].down_w.view(torch.uint8))
    assert torch.equal(again.layers[1].down_s, dst.layers[1].down_s)
    del sd["layers.0.o_s"]
    with pytest.raises(ValueError, match=r"layers\.0\.o_s"):
        again.load_state_dict(sd)
    with pytest.raises(ValueError, match="weights_dtype"):
        LlamaModel(cfg, device="cpu", weights_dtype="int8")
    assert dst.weight_bytes < src.weight_bytes


@pytest.mark.parametrize("extra,match", [
    ("self_attn.q_proj.weight_scale_inv", "weight_scale_inv"),
    ("self_attn.k_proj.k_scale", "k_scale"),
    ("self_attn.v_scale", "v_scale"),
    ("mlp.down_proj.weight_zero_point", "weight_zero_point"),
    ("mlp.up_proj.weight_packed", "weight_packed"),
    ("mlp.up_proj.weight_shape", "weight_shape"),
])
def test_unsupported_quantisation_tensors_are_refused_by_name(extra, match):
    q = _quantize_hf(_hf_tensors(), "channel")
    q["model.layers.1." + extra] = torch.ones(1)
    with pytest.raises(ValueError, match=match + r".*not supported"):
        convert_hf_llama(q)


def test_malformed_fp8_checkpoints_are_refused():
    base = _hf_tensors()
    q = _quantize_hf(base, "channel")
    # one projection left wide: mixed
    mixed = dict(q)
    mixed["model.layers.1.mlp.down_proj.weight"] = base["model.layers.1.mlp.down_proj.weight"]
    del mixed["model.layers.1.mlp.down_proj.weight_scale"]
    with pytest.raises(ValueError, match="mixes fp8"):
        convert_hf_llama(mixed)
    mixed = dict(q)
    mixed["model.layers.0.self_attn.k_proj.weight"] = base["model.layers.0.self_attn.k_proj.weight"]
    del mixed["model.layers.0.self_attn.k_proj.weight_scale"]
    with pytest.raises(ValueError, match="mixes fp8"):
        convert_hf_llama(mixed)
    # codes without a scale
    lost = dict(q)
    del lost["model.layers.0.self_attn.o_proj.weight_scale"]
    with pytest.raises(ValueError, match=r"o_proj\.weight_scale.*missing"):
        convert_hf_llama(lost)
    # a scale of another length (a group or block scale)
    odd = dict(q)
    odd["model.layers.0.mlp.up_proj.weight_scale"] = torch.ones(512, 2)
    with pytest.raises(ValueError, match=r"up_proj\.weight_scale"):
        convert_hf_llama(odd)
    neg = dict(q)
    neg["model.layers.0.mlp.up_proj.weight_scale"] = -torch.ones(512)
    with pytest.raises(ValueError, match="positive"):
        convert_hf_llama(neg)
    # a scale beside a wide weight is not consumed
    stray = dict(base)
    stray["model.layers.0.mlp.up_proj.weight_scale"] = torch.ones(512)
    with pytest.raises(ValueError, match=r"weight_scale.*not supported"):
        convert_hf_llama(stray)
    head = dict(q)
    head["lm_head.weight"] = base["lm_head.weight"].to(FP8)
    with pytest.raises(ValueError, match="lm_head"):
        convert_hf_llama(head)


def _ct(**weights):
    c = json.loads(json.dumps(CT_CONFIG))
    c["config_groups"]["group_0"]["weights"].update(weights)
    return c


@pytest.mark.parametrize("qcfg,match", [
    ({"quant_method": "fp8", "weight_block_size": [128, 128]}, "weight_block_size"),
    (_ct(num_bits=4), "num_bits"),
    (_ct(type="int"), r"weights\.type"),
    (_ct(strategy="block"), "strategy"),
    (_ct(strategy="group"), "strategy"),
    (dict(CT_CONFIG, kv_cache_scheme={"num_bits": 8, "type": "float"}), "kv_cache_scheme"),
])
def test_quantization_config_refusals_name_the_field(tmp_path, qcfg, match):
    path = _write(tmp_path / "m", _quantize_hf(_hf_tensors(), "channel"), qcfg)
    with pytest.raises(ValueError, match=match):
        llama_config_from_hf(path)


def test_fp8_lm_head_is_refused(tmp_path):
    q = _quantize_hf(_hf_tensors(), "channel")
    q["lm_head.weight"] = q["lm_head.weight"].to(FP8)
    q["lm_head.weight_scale"] = torch.ones(512)
    path = _write(tmp_path / "m", q, dict(CT_CONFIG, ignore=[]))
    with pytest.raises(ValueError, match="lm_head"):
        llama_config_from_hf(path)


# ------------------------------------------------------------------------------ sharding
@pytest.mark.parametrize("world", [2, 8])
def test_shard_then_dequantise_equals_dequantise_then_shard(world):
    """qkv_s / gate_up_s follow their rows, o_s / down_s are replicated (world 8: the 2 KV heads
    are replicated on 4 ranks each)."""
    cfg = LlamaConfig(name="t", vocab_size=64, hidden_size=128, intermediate_size=256, num_layers=2, num_heads=8,
                      num_kv_heads=2, head_dim=16, max_position=128)
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="fp8", seed=4)
    sd = model.state_dict()

    def dequant(d):
        out = {}
        for k, v in d.items():
            if k.endswith("_s"):
                continue
            out[k] = ref.dequantize_weight_fp8(v, d[k[:-2] + "_s"]) if v.dtype == FP8 else v
        return out

    wide = dequant(sd)
    for rank in range(world):
        a = dequant(shard_llama(sd, cfg, rank, world))
        b = shard_llama(wide, cfg, rank, world)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (rank, k)
        sh = shard_llama(sd, cfg, rank, world)
        assert torch.equal(sh["layers.0.o_s"], sd["layers.0.o_s"]) and torch.equal(sh["layers.1.down_s"],
                                                                                  sd["layers.1.down_s"])
        assert sh["layers.0.qkv_s"].shape[0] == sh["layers.0.qkv_w"].shape[0] == (8 // world + 2 * max(1, 2 // world)) * 16
        assert sh["layers.0.qkv_w"].dtype == FP8 and sh["layers.0.o_w"].is_contiguous()


# ------------------------------------------------------------------------------ engine on the CPU
def _greedy(e, prompts, n):
    events = {}
    reqs = [e.submit(p, SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True, logprobs=5),
                     callback=lambda ev, i=i: events.setdefault(i, []).append(ev)) for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [(reqs[i].output_ids, events[i]) for i in range(len(prompts))]


def test_engine_serves_an_fp8_model_on_the_cpu():
    """PyStepExecutor over ref.linear_w8: greedy tokens and log-probs equal those of the f32 model
    whose projections hold code.float() * s."""
    cfg = PRESETS["llama-tiny"]
    m8 = LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="fp8")
    wide = LlamaModel(cfg, device="cpu", dtype=torch.float32)
    sd = {}
    for k, v in m8.state_dict().items():
        if k.endswith("_s"):
            continue
        sd[k] = v.float() * m8.state_dict()[k[:-2] + "_s"][:, None] if v.dtype == FP8 else v
    wide.load_state_dict(sd)
    kw = dict(num_blocks=32, max_model_len=256, max_batch=4, max_prefill_tokens=48)
    prompts = [list(range(3, 3 + n)) for n in (5, 33, 70)]
    e8, ew = LLMEngine(m8, None, **kw), LLMEngine(wide, None, **kw)
    assert e8.stats["weights_dtype"] == "fp8" and ew.stats["weights_dtype"] == "bf16"
    assert e8.stats["weight_bytes"] == m8.weight_bytes < ew.stats["weight_bytes"]
    for (ids8, ev8), (idsw, evw) in zip(_greedy(e8, prompts, 8), _greedy(ew, prompts, 8)):
        assert ids8 == idsw
        for a, b in zip(ev8, evw):
            assert [t for t, _ in a.top] == [t for t, _ in b.top]
            assert max(abs(x - y) for (_, x), (_, y) in zip(a.top, b.top)) <= 1e-4
    assert e8.stats["mixed_steps"] > 0      # chunked prefill with decode rows went through linear_w8 too


def test_weights_dtype_flows_from_configuration_and_environment(tmp_path, monkeypatch):
    from langstream_amd.services import ServiceRegistry
    base = {"device": "cpu", "num-blocks": 16, "use-graphs": "false", "max-model-len": 256, "chat-model": "llama-tiny"}

    def engine(**extra):
        reg = ServiceRegistry({**base, **extra})
        try:
            e = reg.llm_engine("llama-tiny")
            return e.stats["weights_dtype"], e.model.layers[0].qkv_w.dtype
        finally:
            reg.shutdown()

    monkeypatch.delenv("LS_WEIGHTS_DTYPE", raising=False)
    assert engine() == ("bf16", torch.float32)                       # auto on a preset
    assert engine(**{"weights-dtype": "fp8"}) == ("fp8", FP8)        # quantised at load
    monkeypatch.setenv("LS_WEIGHTS_DTYPE", "fp8")
    assert engine() == ("fp8", FP8)
    assert engine(**{"weights-dtype": "bf16"}) == ("bf16", torch.float32)   # the key wins over the environment
    monkeypatch.delenv("LS_WEIGHTS_DTYPE")
    with pytest.raises(ValueError, match="weights-dtype"):
        engine(**{"weights-dtype": "int4"})
    # checkpoints: auto follows the directory; fp8 quantises a wide one; bf16 refuses an fp8 one
    fp8_dir = _write(tmp_path / "fp8", _quantize_hf(_hf_tensors(), "channel2"), dict(CT_CONFIG))
    wide_dir = _write(tmp_path / "wide", _hf_tensors())
    assert engine(**{"model-path": fp8_dir}) == ("fp8", FP8)
    assert engine(**{"model-path": wide_dir}) == ("bf16", torch.float32)
    assert engine(**{"model-path": wide_dir, "weights-dtype": "fp8"}) == ("fp8", FP8)
    with pytest.raises(ValueError, match="weights-dtype bf16"):
        engine(**{"model-path": fp8_dir, "weights-dtype": "bf16"})
    from langstream_amd.core.config_model import docs_markdown
    assert "| `weights-dtype` | string |" in docs_markdown()
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "docs", "CONFIG_REFERENCE.md"), encoding="utf-8") as f:
        assert "| `weights-dtype` | string |" in f.read()
