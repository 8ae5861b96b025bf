"""Qwen3: the per-head RMSNorm of q and k between the QKV projection and RoPE
(``LlamaConfig.qk_norm``), on the CPU: logits against the installed ``transformers``, the
reference kernel's math, the loader, TP sharding, and the premise of the GPU runner test.
Nothing is fetched."""
from __future__ import annotations

import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import dataclasses  # noqa: E402
import functools  # noqa: E402
import json  # noqa: E402
import shutil  # noqa: E402
import socket  # noqa: E402

import pytest  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from langstream_amd import ops  # noqa: E402
from langstream_amd.models.llama import AttnMeta, LlamaModel, PRESETS, TPInfo  # noqa: E402
from langstream_amd.models.loader import (HF_MODEL_TYPES, convert_hf_llama, llama_config_from_hf,  # noqa: E402
                                          load_packed, shard_llama)
from langstream_amd.ops import reference as ref  # noqa: E402

# SHAPE and IDS of tests/test_hf_checkpoint_cpu.py
SHAPE = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, max_position_embeddings=2048, tie_word_embeddings=False)
IDS = [int(t) for t in torch.randint(3, 512, (37,), generator=torch.Generator().manual_seed(3))]
BOUND = 1e-4   # the bound of the three families of test_hf_checkpoint_cpu.py (fp32 on both sides)
BS = ops.KV_BLOCK


def _save_qwen3(path, head_dim: int, **extra) -> "torch.nn.Module":
    """A tiny random fp32 Qwen3 with every q_norm / k_norm weight drawn from U(0.5, 2) (the
    library's ones would hide a dropped weight) and any *_proj.bias from N(0, 0.5)."""
    import transformers as tf
    torch.manual_seed(0)
    cfg = tf.Qwen3Config(**SHAPE, head_dim=head_dim, rope_parameters={"rope_theta": 1e6, "rope_type": "default"},
                         **extra)
    model = tf.Qwen3ForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(("q_norm.weight", "k_norm.weight")):
                p.uniform_(0.5, 2.0)
            if n.endswith("_proj.bias"):
                p.normal_(0.0, 0.5)
    model.save_pretrained(str(path))
    return model


def _prefill_meta(T: int, nb: int) -> AttnMeta:
    return AttnMeta(positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T, dtype=torch.int64),
                    num_decode=0, num_prefill_tokens=T, p_block_tables=torch.arange(nb, dtype=torch.int32)[None],
                    q_start=torch.tensor([0], dtype=torch.int32), q_len=torch.tensor([T], dtype=torch.int32),
                    ctx_len=torch.tensor([T], dtype=torch.int32), tiles=ops.prefill_tiles([T], 1))


def _load(path) -> LlamaModel:
    cfg = llama_config_from_hf(str(path))
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32)
    model.load_state_dict(load_packed(str(path)))
    return model


def _our_logits(model: LlamaModel, ids) -> torch.Tensor:
    kv = [ops.new_kv_cache(4, model.hkv, model.cfg.head_dim, "cpu", torch.float32)
          for _ in range(model.cfg.num_layers)]
    return model.forward_logits(torch.tensor(ids, dtype=torch.int32), _prefill_meta(len(ids), 4), kv)


def _hf_logits(hf, ids) -> torch.Tensor:
    with torch.no_grad():
        return hf(torch.tensor([ids])).logits[0].float()


@pytest.fixture(scope="module")
def qwen3_dir(tmp_path_factory):
    path = tmp_path_factory.mktemp("qwen3")
    return _save_qwen3(path, 64), path


# ------------------------------------------------------------------------- logits against HF
@pytest.mark.parametrize("head_dim", [64, 128])   # 128: Hq * D = 512 is not the hidden size 256
def test_qwen3_logits_match_transformers(tmp_path, head_dim):
    """37-token prefill of a saved Qwen3ForCausalLM read back through models.loader, bound
    1e-4; and with the norm weights dropped (ones) our logits move by more than 1000 x that."""
    hf = _save_qwen3(tmp_path, head_dim)
    model = _load(tmp_path)
    cfg = model.cfg
    assert cfg.qk_norm and not cfg.qkv_bias and cfg.head_dim == head_dim and cfg.rms_eps == 1e-6
    assert cfg.rope_theta == 1e6 and cfg.num_heads * cfg.head_dim == 4 * head_dim
    w = torch.cat([t for l in model.layers for t in (l.q_norm, l.k_norm)])
    assert w.numel() == 4 * head_dim and float(w.min()) >= 0.5 and float(w.max()) <= 2.0 and float(w.std()) > 0.3
    ours = _our_logits(model, IDS)
    err = (ours - _hf_logits(hf, IDS)).abs().max().item()
    for l in model.layers:
        l.q_norm.fill_(1.0)
        l.k_norm.fill_(1.0)
    moved = (_our_logits(model, IDS) - ours).abs().max().item()
    print(f"qwen3 D={head_dim}: max |logits - transformers| {err:.3g}; ones for the norm weights move ours by "
          f"{moved:.3g}")
    assert err <= BOUND
    assert moved > 1000 * BOUND


def test_qwen3_attention_bias_follows_the_tensors(tmp_path):
    """attention_bias=True: the q/k/v biases are added before the norm (o_proj's is refused,
    so it is removed from the saved file and zeroed in the library's model)."""
    from safetensors.torch import load_file, save_file
    hf = _save_qwen3(tmp_path, 64, attention_bias=True)
    f = os.path.join(str(tmp_path), "model.safetensors")
    sd = load_file(f)
    with pytest.raises(ValueError, match=r"o_proj\.bias"):
        load_packed(str(tmp_path))
    save_file({k: v for k, v in sd.items() if not k.endswith("o_proj.bias")}, f)
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if n.endswith("o_proj.bias"):
                p.zero_()
    model = _load(tmp_path)
    assert model.cfg.qk_norm and model.cfg.qkv_bias and float(model.layers[0].qkv_b.abs().max()) > 0.5
    err = (_our_logits(model, IDS) - _hf_logits(hf, IDS)).abs().max().item()
    print(f"qwen3 with attention_bias: max |logits - transformers| {err:.3g}")
    assert err <= BOUND


# ----------------------------------------------------------------------- reference kernel math
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_reference_rope_and_cache_norm_math(with_bias):
    """ref.rope_and_cache(..., q_norm, k_norm, eps) against a few independent fp32 lines
    (bias -> per-head RMSNorm -> apply_rope); V rows and the V cache bit-identical to the call
    without the norm; and one (token, head) of std 1e-3, whose mean square is of the size of
    eps = 1e-6, so that a missing or a tenfold eps is a change of tens of percent there."""
    T, Hq, Hkv, D, eps = 7, 4, 2, 64, 1e-6
    H = Hq + 2 * Hkv
    g = torch.Generator().manual_seed(4)
    qkv0 = torch.randn(T, H, D, generator=g) * 2
    small = [(2, 1), (5, Hq)]   # a q head and a k head
    bias = torch.randn(H * D, generator=g) * 0.5 if with_bias else None
    for t, h in small:   # std 1e-3 is what the norm sees: after the bias
        qkv0[t, h] = torch.randn(D, generator=g) * 1e-3 - (bias.view(H, D)[h] if with_bias else 0.0)
    qn, kn = torch.rand(D, generator=g) * 1.5 + 0.5, torch.rand(D, generator=g) * 1.5 + 0.5
    pos = torch.randint(0, 2048, (T,), generator=g, dtype=torch.int32)
    cs = ref.rope_cos_sin(2048, D, 1e6)
    slots = torch.tensor([3, 64, -1, 5, 130, 131, 0], dtype=torch.int64)

    def run(**kw):
        q = qkv0.reshape(T, H * D).clone()
        kc, vc = ops.new_kv_cache(3, Hkv, D, "cpu", torch.float32)
        ref.rope_and_cache(q, pos, cs, slots, kc, vc, Hq, Hkv, True, 1.0, 1.0, bias, **kw)
        return q.view(T, H, D), kc, vc

    got, kc, vc = run(q_norm=qn, k_norm=kn, norm_eps=eps)
    plain, kc0, vc0 = run()

    def expect(e):
        x = qkv0.clone()
        if bias is not None:
            x = x + bias.view(H, D)
        qk = x[:, : Hq + Hkv]
        w = torch.stack([qn] * Hq + [kn] * Hkv)
        qk = qk / torch.sqrt((qk * qk).sum(-1, keepdim=True) / D + e) * w
        return torch.cat([ref.apply_rope(qk, pos, cs), x[:, Hq + Hkv:]], 1)

    exp = expect(eps)
    # per head, against the head's largest entry (the rotation subtracts, so single entries
    # can be small): about ten fp32 roundings of 6e-8 each per entry, bound 1e-5
    err = ((got - exp).abs().amax(-1) / exp.abs().amax(-1)).max().item()
    print(f"reference norm: max deviation from the independent computation, per head {err:.3g}")
    assert err < 1e-5
    assert torch.equal(got[:, Hq + Hkv:], plain[:, Hq + Hkv:]) and torch.equal(vc, vc0), "v is not normed"
    assert not torch.equal(got[:, : Hq + Hkv], plain[:, : Hq + Hkv]) and not torch.equal(kc, kc0)
    # the K cache holds the k heads of the rows
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            assert torch.equal(kc[s // BS, :, s % BS], got[t, Hq: Hq + Hkv])
    # the premise of the small heads: there eps is of the size of the mean square
    for t, h in small:
        for other in (0.0, 10 * eps):
            rel = ((expect(other)[t, h] - exp[t, h]).norm() / exp[t, h].norm()).item()
            assert rel > 0.2, (t, h, other, rel)
            assert ((got[t, h] - exp[t, h]).norm() / exp[t, h].norm()).item() < 1e-5
    with pytest.raises(AssertionError, match="together"):
        run(q_norm=qn)


# ------------------------------------------------------------------------------------- loader
def _write_config(path, cfg: dict) -> str:
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    return str(path)


def test_qwen3_config_reading(tmp_path, qwen3_dir):
    base = dict(model_type="qwen3", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=4,
                num_attention_heads=4, num_key_value_heads=2, head_dim=128, max_position_embeddings=2048,
                rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True)
    assert "qwen3" in HF_MODEL_TYPES
    c = llama_config_from_hf(_write_config(tmp_path / "a", base))
    assert c.qk_norm and not c.qkv_bias and c.head_dim == 128 and c.tie_embeddings and c.rope_theta == 1e6
    assert c.max_position == 2048 and c.sliding_window == 0
    # the window rules of qwen2: only with use_sliding_window; layer_types or max_window_layers
    w = {**base, "sliding_window": 128}
    assert llama_config_from_hf(_write_config(tmp_path / "w0", w)).max_position == 2048
    assert llama_config_from_hf(_write_config(tmp_path / "w1", {**w, "use_sliding_window": True})).max_position == 128
    cw = llama_config_from_hf(_write_config(tmp_path / "w2", {**w, "use_sliding_window": True,
                                                              "max_window_layers": 2}), sliding_window=True)
    assert cw.max_position == 2048 and cw.sliding_window == 128 and cw.window_layers == (2, 3)
    cl = llama_config_from_hf(_write_config(tmp_path / "w3", {
        **w, "use_sliding_window": True,
        "layer_types": ["full_attention", "sliding_attention", "full_attention", "sliding_attention"]}),
        sliding_window=True)
    assert cl.window_layers == (1, 3)
    with pytest.raises(ValueError, match="yarn"):
        llama_config_from_hf(_write_config(tmp_path / "y", {**base, "rope_parameters": {
            "rope_theta": 1e6, "rope_type": "yarn", "factor": 4.0}}))
    with pytest.raises(ValueError, match="qwen3_moe"):
        llama_config_from_hf(_write_config(tmp_path / "m", {**base, "model_type": "qwen3_moe"}))
    # a model of another type that carries the tensors loads with qk_norm set
    _, path = qwen3_dir
    other = tmp_path / "llama_with_norm"
    shutil.copytree(str(path), str(other))
    with open(os.path.join(str(other), "config.json")) as f:
        cj = json.load(f)
    _write_config(other, {**cj, "model_type": "llama"})
    lc = llama_config_from_hf(str(other))
    assert lc.qk_norm and not lc.qkv_bias
    m = LlamaModel(lc, device="cpu", dtype=torch.float32)
    m.load_state_dict(load_packed(str(other)))
    assert float((m.layers[1].k_norm - 1).abs().max()) > 0.3


def test_convert_takes_both_norm_weights_or_refuses(qwen3_dir, tmp_path):
    from safetensors.torch import load_file, save_file
    _, path = qwen3_dir
    sd = load_file(os.path.join(str(path), "model.safetensors"))
    out = convert_hf_llama(dict(sd))
    for i in range(2):
        assert torch.equal(out[f"layers.{i}.q_norm"], sd[f"model.layers.{i}.self_attn.q_norm.weight"])
        assert torch.equal(out[f"layers.{i}.k_norm"], sd[f"model.layers.{i}.self_attn.k_norm.weight"])
    assert "layers.0.qkv_b" not in out
    only_q = {k: v for k, v in sd.items() if k != "model.layers.1.self_attn.k_norm.weight"}
    with pytest.raises(ValueError, match=r"model\.layers\.1\.self_attn\.k_norm\.weight"):
        convert_hf_llama(only_q)
    only_k = {k: v for k, v in sd.items() if k != "model.layers.0.self_attn.q_norm.weight"}
    with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.q_norm\.weight"):
        convert_hf_llama(only_k)
    sd["model.layers.0.self_attn.o_proj.bias"] = torch.zeros(256)
    shutil.copy(os.path.join(str(path), "config.json"), tmp_path / "config.json")
    save_file(sd, str(tmp_path / "model.safetensors"))
    with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.o_proj\.bias"):
        load_packed(str(tmp_path))


def _normed(name: str, seed: int = 5) -> LlamaModel:
    """A preset model in fp32 on the CPU with U(0.5, 2) norm weights."""
    model = LlamaModel(PRESETS[name], device="cpu", dtype=torch.float32, seed=seed)
    g = torch.Generator().manual_seed(seed)
    for layer in model.layers:
        layer.q_norm.copy_(torch.rand(layer.q_norm.numel(), generator=g) * 1.5 + 0.5)
        layer.k_norm.copy_(torch.rand(layer.k_norm.numel(), generator=g) * 1.5 + 0.5)
    return model


def test_presets_state_dict_and_sharding():
    """The presets; q_norm / k_norm in tensors(), state_dict, load_state_dict and num_params;
    shard_llama at world 2 keeps both weights whole on every rank."""
    t, s = PRESETS["qwen3-tiny"], PRESETS["qwen3-small"]
    assert dataclasses.replace(t, name="qwen2-tiny", qk_norm=False, qkv_bias=True) == PRESETS["qwen2-tiny"]
    assert (s.hidden_size, s.intermediate_size, s.num_heads, s.num_kv_heads, s.head_dim, s.num_layers, s.vocab_size,
            s.rope_theta, s.rms_eps, s.tie_embeddings, s.qk_norm, s.qkv_bias) == (
        1024, 3072, 16, 8, 128, 4, 32000, 1e6, 1e-6, True, True, False)
    assert s.num_heads * s.head_dim == 2048 != s.hidden_size
    a, b = PRESETS["qwen3-0.6b"], PRESETS["qwen3-8b"]
    assert (a.hidden_size, a.intermediate_size, a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim, a.vocab_size,
            a.tie_embeddings, a.qk_norm) == (1024, 3072, 28, 16, 8, 128, 151936, True, True)
    assert (b.hidden_size, b.intermediate_size, b.num_layers, b.num_heads, b.num_kv_heads, b.head_dim, b.vocab_size,
            b.tie_embeddings, b.qk_norm) == (4096, 12288, 36, 32, 8, 128, 151936, False, True)
    assert 0.59e9 < a.num_params < 0.61e9 and 8.1e9 < b.num_params < 8.3e9   # 0.6B and 8.2B published
    assert not PRESETS["llama-tiny"].qk_norm
    assert LlamaModel(PRESETS["llama-tiny"], device="cpu").layers[0].q_norm is None
    fresh = LlamaModel(t, device="cpu", dtype=torch.float32)
    assert torch.equal(fresh.layers[0].q_norm, torch.ones(t.head_dim)) and fresh.layers[0].k_norm.shape == (t.head_dim,)
    model = _normed("qwen3-tiny")
    sd = model.state_dict()
    assert sd["layers.1.q_norm"] is model.layers[1].q_norm and "layers.0.k_norm" in sd
    assert t.num_params == sum(v.numel() for v in sd.values())
    assert sum(x.numel() for x in model.layers[0].tensors()) == sum(
        v.numel() for k, v in sd.items() if k.startswith("layers.0."))
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.layers[1].k_norm, model.layers[1].k_norm)
    for rank in range(2):
        part = shard_llama(sd, t, rank, 2)
        for i in range(t.num_layers):
            assert torch.equal(part[f"layers.{i}.q_norm"], sd[f"layers.{i}.q_norm"])
            assert torch.equal(part[f"layers.{i}.k_norm"], sd[f"layers.{i}.k_norm"])
        shard = LlamaModel(t, device="cpu", dtype=torch.float32, tp=TPInfo(rank, 2, None))
        shard.load_state_dict(part)


# --------------------------------------------------------------------- registry, end to end
_HEAD = r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|"
_TAIL = r"| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"
QWEN_SPLIT = _HEAD + r"\p{N}" + _TAIL


def _train_tokenizer(path, split: str, vocab_size: int = 512) -> "object":
    """tests/test_hf_checkpoint_cpu.py: a small byte-level BPE trained on the built-in corpus."""
    from tokenizers import Regex, Tokenizer, decoders, models, pre_tokenizers, trainers
    from langstream_amd.tokenizers import builtin_corpus
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.Sequence([
        pre_tokenizers.Split(Regex(split), behavior="isolated", invert=False),
        pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["<|endoftext|>", "<|im_start|>", "<|im_end|>"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(builtin_corpus(), trainer)
    tok.save(str(path))
    return tok


def test_registry_serves_a_qwen3_model_path(qwen3_dir):
    """local-gpu-configuration {model-path} on a Qwen3 directory: ChatML by default, and a
    greedy 8-token chat completion equal to the library's own greedy tokens."""
    from langstream_amd.agents.genai.services import ChatMessage, chatml_chat_prompt
    from langstream_amd.services import ServiceRegistry
    hf, path = qwen3_dir
    lib = _train_tokenizer(path / "tokenizer.json", QWEN_SPLIT)
    reg = ServiceRegistry({"model-path": str(path), "device": "cpu", "num-blocks": 16, "use-graphs": "false",
                           "max-model-len": 256})
    try:
        svc = reg.completions_service({"local": {}}, "qwen3-0.6b")
        eng = svc.engine
        assert eng.chat_template == "chatml"
        cfg = eng.model.cfg
        assert (cfg.hidden_size, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.num_layers, cfg.vocab_size,
                cfg.qkv_bias, cfg.qk_norm, cfg.rope_theta) == (256, 4, 2, 64, 2, 512, False, True, 1e6)
        msgs = [ChatMessage("system", "You are terse."), ChatMessage("user", "What is 12+30?")]
        ids = eng.tok.encode(chatml_chat_prompt(msgs))
        assert ids == lib.encode(chatml_chat_prompt(msgs), add_special_tokens=False).ids
        exp, cur = [], list(ids)
        for _ in range(8):
            exp.append(int(_hf_logits(hf, cur)[-1].argmax()))
            cur.append(exp[-1])
        res = svc.get_chat_completions(msgs, None, {"max-tokens": 8, "temperature": 0, "ignore-eos": True}).result(120)
        assert res.completion_tokens == 8 and res.prompt_tokens == len(ids)
        assert res.content == eng.tok.decode(exp)
    finally:
        reg.shutdown()


def test_docs_name_qwen3():
    from langstream_amd.core.config_model import docs_markdown
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "docs", "CONFIG_REFERENCE.md"), encoding="utf-8") as f:
        ref_md = f.read()
    for md in (docs_markdown(), ref_md):
        lines = [l for l in md.splitlines() if l.startswith(("| `model-path` |", "| `chat-template` |"))]
        assert len(lines) == 2 and all("qwen3" in l for l in lines), lines


# ---------------------------------------------------------- premise of the GPU runner test
def norm_w(D: int, k: bool, device="cpu") -> torch.Tensor:
    """_norm_w of tests/test_qk_norm_gpu.py: column c holds (-1)^(c + c // (D/2)) (0.5 + c / 256),
    times 1.5 for k_norm."""
    c = torch.arange(D)
    sign = 1.0 - 2.0 * ((c + c // (D // 2)) % 2)
    return (sign * (0.5 + c / 256.0) * (1.5 if k else 1.0)).to(device)


def step_inputs(model, nd, npre, seed, device="cpu"):
    """_step_inputs of tests/test_qk_norm_gpu.py (the same values on either device): nd decode
    rows (sequence i has ctx 20 + 3 i, blocks 2 i and 2 i + 1, over a cache of random earlier
    tokens) followed by one prefill chunk of npre tokens.  Checked rows: every decode row and
    the prefill rows at 1/4, 1/2 and the end of the chunk -- not the chunk's first row, which
    sees only its own key: its attention output is its v whatever q and k are."""
    cfg = model.cfg
    T = nd + npre
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, cfg.vocab_size, (T,), generator=g, dtype=torch.int32).to(device)
    pblocks = (npre + BS - 1) // BS
    nb = 2 * nd + pblocks + 1
    ctx = [20 + 3 * i for i in range(nd)]
    pos = torch.tensor([c - 1 for c in ctx] + list(range(npre)), dtype=torch.int32)
    d_bt = torch.tensor([[2 * i, 2 * i + 1] for i in range(nd)], dtype=torch.int32).reshape(nd, 2)
    p_bt = torch.arange(2 * nd, 2 * nd + pblocks, dtype=torch.int32).reshape(1, -1)
    slots = [int(d_bt[i, (c - 1) // BS]) * BS + (c - 1) % BS for i, c in enumerate(ctx)]
    slots += [int(p_bt[0, t // BS]) * BS + t % BS for t in range(npre)]
    meta = AttnMeta(positions=pos.to(device), slots=torch.tensor(slots, dtype=torch.int64, device=device),
                    num_decode=nd)
    if nd:
        meta.d_block_tables, meta.d_ctx_lens = d_bt.to(device), torch.tensor(ctx, dtype=torch.int32, device=device)
        meta.nsplit, meta.blocks_per_split = 1, 2
    if npre:
        meta.num_prefill_tokens = npre
        meta.p_block_tables = p_bt.to(device)
        meta.q_start = torch.tensor([nd], dtype=torch.int32, device=device)
        meta.q_len = torch.tensor([npre], dtype=torch.int32, device=device)
        meta.ctx_len = torch.tensor([npre], dtype=torch.int32, device=device)
        meta.tiles = ops.prefill_tiles([npre], model.hq // model.hkv).to(device)

    def caches():
        gk = torch.Generator().manual_seed(seed + 1)
        kv = [ops.new_kv_cache(nb, model.hkv, cfg.head_dim, device, model.dtype) for _ in range(cfg.num_layers)]
        for kc, vc in kv:
            kc.copy_(torch.randn(kc.shape, generator=gk) * 0.5)
            vc.copy_(torch.randn(vc.shape, generator=gk) * 0.5)
        return kv

    rows = set(range(nd))
    if npre:
        rows |= {nd + npre // 4, nd + npre // 2, T - 1}
    return ids, meta, caches, torch.tensor(sorted(rows), dtype=torch.long, device=device)


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-12))


CASES = [("qwen3-small", 3, 0), ("qwen3-small", 8, 0), ("qwen3-small", 8, 70), ("qwen3-small", 0, 1100),
         ("qwen3-tiny", 8, 0)]


@functools.lru_cache(maxsize=None)
def _premise_model(name):
    """The model of the GPU tests (_normed_model there) in fp32: the CPU's seeded init with
    every weight rounded to bf16, the values the GPU model holds, and the weights of _norm_w."""
    model = LlamaModel(PRESETS[name], device="cpu", dtype=torch.float32)
    for l in model.layers:
        l.q_norm.copy_(norm_w(model.cfg.head_dim, False))
        l.k_norm.copy_(norm_w(model.cfg.head_dim, True))
    for t in {id(v): v for v in model.state_dict().values()}.values():
        t.copy_(t.to(torch.bfloat16).float())
    return model


@pytest.mark.parametrize("name,nd,npre", CASES, ids=["gemv3", "dgemm8", "mixed8+70", "prefill1100", "tiny-d64-8"])
def test_norm_weights_move_every_checked_row(name, nd, npre):
    """The margin the GPU test test_runner_routes_apply_the_norm relies on, established on
    the fp32 Python forward alone: with the weights of _norm_w every checked row's logits
    have 1 - cos > 0.01 against (a) the same model with both norm weights set to ones and
    (b) the same weights with qk_norm off."""
    model = _premise_model(name)
    ids, meta, caches, rows = step_inputs(model, nd, npre, 100 + nd + npre)

    def logits(m):
        return m.logits(m.forward(ids, meta, caches()).index_select(0, rows)).float()

    a = logits(model)
    saved = [(l.q_norm.clone(), l.k_norm.clone()) for l in model.layers]
    try:
        for l in model.layers:
            l.q_norm.fill_(1.0)
            l.k_norm.fill_(1.0)
        ones = logits(model)
    finally:
        for l, (q, k) in zip(model.layers, saved):
            l.q_norm.copy_(q)
            l.k_norm.copy_(k)
    off = LlamaModel(dataclasses.replace(model.cfg, qk_norm=False), device="cpu", dtype=torch.float32)
    off.load_state_dict({k: v for k, v in model.state_dict().items() if not k.endswith(("q_norm", "k_norm"))})
    noff = logits(off)
    d1 = [1 - _cos(a[i], ones[i]) for i in range(len(rows))]
    d2 = [1 - _cos(a[i], noff[i]) for i in range(len(rows))]
    print(f"premise {name} nd={nd} npre={npre}: min 1 - cos against ones {min(d1):.4f}, against no norm {min(d2):.4f}")
    assert min(d1) > 0.01, d1
    assert min(d2) > 0.01, d2


ENGINE_LENS = (33, 40, 64, 65, 100, 130, 160, 200)
ENGINE_SEEDS = (14, 5, 36, 38, 16, 26, 28, 4)   # prompt k: the k-th prompt of the stream seeded ENGINE_SEEDS[k]


def engine_prompts(vocab: int):
    """_engine_prompts of tests/test_qk_norm_gpu.py: eight prompts of random ids."""
    out = []
    for k, seed in enumerate(ENGINE_SEEDS):
        g = torch.Generator().manual_seed(seed)
        out.append([torch.randint(5, vocab, (n,), generator=g).tolist() for n in ENGINE_LENS][k])
    return out


def test_norm_weights_move_every_engine_prompt():
    """The premise of the GPU engine test ('the ones-weight model generates other tokens for
    every prompt'), on the fp32 forward alone.  The logits of a randomly initialised model are
    nearly flat (top-2 gaps of 0.01 to 0.1 nats), and for short prompts, or prompts of
    consecutive ids, the first generated token is often the same with either weights.  For
    these prompts, picked on this forward from seeded streams, it is not, with a margin: in
    each model the log-probability of its own first token exceeds that of the other model's
    first token by more than 0.5 nats, 25 times the 0.02 nats within which two bf16 runs of one
    model may split (the near-tie rule of the engine tests)."""
    model = _premise_model("qwen3-small")
    prompts = engine_prompts(model.cfg.vocab_size)

    def first_logprobs():
        out = []
        for p in prompts:
            kv = [ops.new_kv_cache(4, model.hkv, model.cfg.head_dim, "cpu", torch.float32)
                  for _ in range(model.cfg.num_layers)]
            lg = model.forward_logits(torch.tensor(p, dtype=torch.int32), _prefill_meta(len(p), 4), kv,
                                      rows=torch.tensor([len(p) - 1]))
            out.append(torch.log_softmax(lg[0].double(), -1))
        return out

    a = first_logprobs()
    saved = [(l.q_norm.clone(), l.k_norm.clone()) for l in model.layers]
    try:
        for l in model.layers:
            l.q_norm.fill_(1.0)
            l.k_norm.fill_(1.0)
        z = first_logprobs()
    finally:
        for l, (q, k) in zip(model.layers, saved):
            l.q_norm.copy_(q)
            l.k_norm.copy_(k)
    gaps = [min(float(x.max() - x[y.argmax()]), float(y.max() - y[x.argmax()])) for x, y in zip(a, z)]
    print("first-token gaps between the two models, nats:", [round(g, 3) for g in gaps])
    assert min(gaps) > 0.5, gaps


# ----------------------------------------------------------------------------------- TP = 2
PROMPTS = [list(range(3, 3 + n)) for n in (5, 64, 97)]


def _port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
        cfg = PRESETS["qwen3-tiny"]
        m = LlamaModel(cfg, device="cpu", dtype=torch.float32, tp=TPInfo(rank, world, None))
        m.load_state_dict(shard_llama(_normed("qwen3-tiny").state_dict(), cfg, rank, world))
        eng = LLMEngine(m, None, num_blocks=64, max_model_len=512)
        if rank == 0:
            out = [r.output_ids for r in eng.generate(PROMPTS, SamplingParams(max_tokens=6, temperature=0.0,
                                                                             ignore_eos=True))]
            eng.stop()
            q.put(out)
        else:
            eng.worker_loop()
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_normed_model_matches_single():
    """gloo, 2 ranks (test_tensor_parallel_biased_model_matches_single): greedy tokens of the
    sharded qwen3-tiny equal TP = 1, and the norm weights matter for them."""
    from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
    sp = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    single = [r.output_ids for r in LLMEngine(_normed("qwen3-tiny"), None, num_blocks=64, max_model_len=512).generate(
        PROMPTS, sp)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        out = q.get(timeout=240)
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert out == single
    plain = LlamaModel(PRESETS["qwen3-tiny"], device="cpu", dtype=torch.float32, seed=5)
    assert [r.output_ids for r in LLMEngine(plain, None, num_blocks=64, max_model_len=512).generate(
        PROMPTS, sp)] != single
