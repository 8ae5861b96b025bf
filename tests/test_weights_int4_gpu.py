"""Int4 projection weights on the GPU: gemm_w4.hip against ops.reference.linear_w4 in float64, and the engine.  EXACT operands (x = +-1,
<= 16 codes per row off their zero point by <= 4, scales in {0.5, 1, 2}): sums are multiples of 0.5 below 128, so out EQUALS bf16(ref)."""
import dataclasses

import pytest
import torch

import gemm_probe as gp
from test_weights_fp8_gpu import (PROMPTS, _auto_splits, _bm, _close_tops, _first_token_tops, _run_tops,
                                  _same_or_near_tie, _step_tops)
from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaModel, PRESETS, W8_NAMES
from langstream_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV, SENTINEL = "cuda", gp.SENTINEL


def _exact(M, N, K, G, S=1):
    g = torch.Generator().manual_seed(M + K)
    x = (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).to(torch.bfloat16)
    zero = torch.randint(0, 16, (N, K // G), generator=g)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, K // G), generator=g)]
    cols = set(gp.probe_columns(K, 64 if K <= 4096 else 1024)) | set(gp.probe_columns(K, G))
    cols = torch.tensor(sorted(cols | {k for lo, hi in gp.split_ranges(K, S, 64) for k in (lo, hi - 1)}))
    q = zero.repeat_interleave(G, 1)
    for n in range(N):
        pick = cols[torch.randperm(len(cols), generator=g)[:16]]
        d = torch.randint(1, 5, (len(pick),), generator=g) * (torch.randint(0, 2, (len(pick),), generator=g) * 2 - 1)
        q[n, pick] = (q[n, pick] + d).clamp(0, 15)
    w = (ref.pack_weight_int4(q), scale, zero.to(torch.uint8))
    want = ref.linear_w4(x, *w, dtype=torch.float64)
    # the reference alone notices an x zeroed at a probed column
    x0 = x.clone()
    x0[:, int(cols[(q[:, cols] != zero[:, cols // G]).any(0).nonzero()[0, 0]])] = 0
    assert not torch.equal(ref.linear_w4(x0, *w, dtype=torch.float64), want)
    return (x, *w, want)


def _run(x, codes, scale, zero, splits=0, out=None):
    ops.w8_launch_counts(reset=True)
    got = ops.linear_w4(x.to(DEV), codes.to(DEV), scale.to(DEV), zero.to(DEV), out=out, splits=splits)
    torch.cuda.synchronize()
    return got, ops.w8_launch_counts(reset=True)


def _key(M, N, K, splits=0):
    return "w4_gemv" if M <= 4 and K % 1024 == 0 and not splits else f"w4_bm{_bm(M)}_s{splits or _auto_splits(M, N, K)}"


CASES = ([(M, 128, 2816, 64, 0) for M in (1, 5, 63, 64, 65, 128, 129, 300)]
         + [(5, 64, 64, 64, 0), (65, 192, 128, 128, 0), (5, 64, 2048, 128, 0), (130, 64, 2048, 256, 0), (5, 64, 512, 512, 0)]
         # forced splits: uneven slices; at G = 128, K = 2560 slices 1 and 2 start inside a group
         + [(129, 128, 2816, 64, 3), (5, 192, 2816, 64, 7), (5, 64, 2560, 128, 3)]
         # the GEMV's shape rule: inside it, one row past it, a K off it
         + [(M, 64, K, 128, 0) for M in (1, 2, 3, 4) for K in (1024, 5120, 14336, 28672)]
         + [(2, 64, 5120, 1024, 0), (5, 64, 1024, 128, 0), (4, 64, 1088, 64, 0)])


@pytest.mark.parametrize("M,N,K,G,splits", CASES)
def test_w4_exact(M, N, K, G, splits):
    x, codes, scale, zero, want = _exact(M, N, K, G, splits or _auto_splits(M, N, K))
    got, census = _run(x, codes, scale, zero, splits)
    assert census == {_key(M, N, K, splits): 1}, census
    assert torch.equal(got.cpu(), want.to(torch.bfloat16)), (got.cpu().double() - want).abs().max().item()


@pytest.mark.parametrize("key,splits,ks", [("w4_gemv", 0, (3, 70, 525, 1016)), ("w4_gemv", 0, (1, 66, 516, 1023)),
                                           ("w4_bm64_s1", 1, range(0, 1024, 67)), ("w4_bm64_s4", 4, range(0, 1024, 67))])
def test_w4_every_code_every_zero_point(key, splits, ks):
    """One-hot x, scale 1: out = q - zero, all 256 pairs per column; both GEMV sets together and each GEMM set cover the 8 nibble slots."""
    N, K, G, ks = 256, 1024, 64, list(ks)
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    q, zero = (n // 16 + k) % 16, (n + torch.arange(K // G)[None, :]) % 16
    assert len(set(zip(q[:, ks[0]].tolist(), zero[:, ks[0] // G].tolist()))) == 256
    x = torch.zeros(len(ks), K, dtype=torch.bfloat16)
    x[torch.arange(len(ks)), ks] = 1.0
    got, census = _run(x, ref.pack_weight_int4(q), torch.ones(N, K // G), zero.to(torch.uint8), splits)
    assert census == {key: 1}, census
    assert torch.equal(got.cpu().double(), torch.stack([q[:, c] - zero[:, c // G] for c in ks]).double())


@pytest.mark.parametrize("M,N,K,G,splits", [(5, 128, 2816, 64, 0), (129, 128, 2816, 128, 3), (4, 128, 14336, 128, 0)])
def test_w4_rounded(M, N, K, G, splits):
    g = torch.Generator().manual_seed(K + G)
    x = (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).to(torch.bfloat16)
    w = (ref.pack_weight_int4(torch.randint(0, 16, (N, K), generator=g)), 10.0 ** (torch.rand(N, K // G, generator=g) * 3 - 3),
         torch.randint(0, 16, (N, K // G), generator=g).to(torch.uint8))
    got, census = _run(x, *w, splits)
    assert list(census) == [_key(M, N, K, splits)], census
    want = ref.linear_w4(x, *w, dtype=torch.float64)
    assert bool(((got.cpu().double() - want).abs() <= gp.RTOL * want.abs() + gp.FLOOR).all())


def test_w4_views_and_sentinels():
    M, N, K, G = 5, 128, 512, 128
    x, codes, scale, zero, want = _exact(M, N, K, G, 2)
    wide = torch.full((M + 2, K + 64), 3.0, dtype=torch.bfloat16, device=DEV)
    wide[1:M + 1, 8:K + 8] = x.to(DEV)
    frame = torch.full((M + 2, N + 16), SENTINEL, dtype=torch.bfloat16, device=DEV)
    got, census = _run(wide[1:M + 1, 8:K + 8], codes, scale, zero, out=frame[1:M + 1, 8:N + 8])
    assert census == {"w4_bm64_s2": 1}, census
    f = frame.cpu()
    assert torch.equal(f[1:M + 1, 8:N + 8], want.to(torch.bfloat16))
    f[1:M + 1, 8:N + 8] = SENTINEL
    assert bool((f.float() == SENTINEL).all())


def test_w4_guards_refuse_and_write_nothing():
    h = ops.hip()
    M, N, K, G = 5, 128, 1024, 128
    x, codes, scale, zero = (t.to(DEV) for t in _exact(M, N, K, G)[:4])
    ws = torch.zeros(8 * M * N, dtype=torch.float32, device=DEV)
    out = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    bad = [("x must be bf16", dict(x=x.float())), ("zero must be uint8", dict(z=zero.to(torch.int32))),
           ("w must be uint8", dict(w=codes.view(torch.float8_e4m3fn))),
           ("scale must be float32", dict(s=scale.to(torch.bfloat16))),
           ("contiguous", dict(w=codes.t().contiguous().t())),
           ("group size", dict(s=torch.ones(N, K // 32, device=DEV), z=torch.zeros(N, K // 32, dtype=torch.uint8, device=DEV))),
           ("shape of scale", dict(z=zero[:, :-1].contiguous())),
           ("16-byte aligned", dict(w=torch.zeros(N * K // 2 + 16, dtype=torch.uint8, device=DEV)[8:8 + N * K // 2].view(N, K // 2))),
           ("unit inner stride", dict(x=torch.zeros(M, 2 * K, dtype=torch.bfloat16, device=DEV)[:, ::2])),
           ("multiples of 64", dict(w=codes[:96].contiguous(), s=scale[:96].contiguous(), z=zero[:96].contiguous())),
           ("out must be", dict(out=torch.full((M + 1, N), SENTINEL, dtype=torch.bfloat16, device=DEV))),
           ("workspace", dict(workspace=ws[: 4 * M * N - 1], splits=4))]
    for msg, kw in bad:
        a = dict(dict(out=out, x=x, w=codes, s=scale, z=zero, workspace=ws, splits=0), **kw)
        with pytest.raises(RuntimeError, match=msg):
            h.w4_gemm(a["out"], a["x"], a["w"], a["s"], a["z"], a["workspace"], a["splits"])
        torch.cuda.synchronize()
        assert bool((a["out"].float().cpu() == SENTINEL).all()) and not bool(ws.any()), msg
    with pytest.raises(RuntimeError, match="M <= 4"):
        h.w4_gemv(out, x, codes, scale, zero)
    for call in (lambda: h.w8_gemm(out, x, codes.repeat(1, 2), scale[:, 0].contiguous(), ws, 0), lambda: h.decode_gemm(out, x, codes, ws)):
        with pytest.raises(RuntimeError):    # the fp8 and bf16 entry points never take packed nibbles
            call()
    assert bool((out.float().cpu() == SENTINEL).all())
    assert h.w4_supported(codes) and not h.w4_supported(codes[:96]) and not h.w8_supported(codes)


# ------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def small_pair():
    gpu = LlamaModel(PRESETS["llama-small"], device=DEV, weights_dtype="int4")
    sd = {k: v.cpu() for k, v in gpu.state_dict().items()}
    cpu = LlamaModel(gpu.cfg, device="cpu", dtype=torch.float32)
    cpu.load_state_dict({k: (ref.dequantize_weight_int4(v, sd[k[:-2] + "_s"], sd[k[:-2] + "_z"]) if v.dtype == torch.uint8
                             else v.float()) for k, v in sd.items() if not k.endswith(("_s", "_z"))})
    return gpu, cpu


@pytest.mark.parametrize("M", [1, 4, 5, 129])
def test_runner_w4_at_m_rows_matches_fp32(small_pair, M):
    """A prefill of M tokens and a decode step of M rows against the f32 CPU model; only W4 projection launches."""
    gpu, cpu = small_pair
    torch.manual_seed(M)
    prompt = [[int(t) for t in torch.randint(5, 30000, (M,))]]
    prompts = [[int(t) for t in torch.randint(5, 30000, (3,))] for _ in range(M)]
    kw = dict(num_blocks=1024, max_model_len=1024, max_batch=512, max_prefill_tokens=4096)
    ops.w8_launch_counts(reset=True)
    ops.hip().decode_gemm_launch_counts(True)
    _close_tops(_first_token_tops(LLMEngine(gpu, None, **kw), prompt)[0], _first_token_tops(LLMEngine(cpu, None, **kw), prompt)[0])
    eg, ec = (_step_tops(LLMEngine(m, None, use_graphs=False, **kw), prompts, 2) for m in (gpu, cpu))
    for a, b in zip(eg, ec):
        _close_tops(a[0], b[0])
        if a[0].token_id == b[0].token_id:
            _close_tops(a[1], b[1])
    assert sum(a[0].token_id == b[0].token_id for a, b in zip(eg, ec)) >= 0.8 * M
    census, dg = ops.w8_launch_counts(reset=True), ops.hip().decode_gemm_launch_counts(True)
    assert all(k.startswith("w4_") for k in census) and sum(census.values()) >= 3 * 4 * gpu.cfg.num_layers, census
    assert ("w4_gemv" in census) == (M <= 4), census   # K = 1024 takes the GEMV at M <= 4, K = 2816 (down) never
    assert all("_partial_" in k and k.endswith("_s1") for k in dg), dg    # only the LM head's f32 launches


@pytest.mark.parametrize("name,bias,kw", [("llama-small", False, {}), ("qwen3-small", True, dict(
    kv_cache_dtype="fp8", kv_k_scale=0.5, kv_v_scale=2.0))])
def test_engine_w4_graphs_match_eager_and_python(name, bias, kw):
    """Graphs against the eager native runner and the Python executor; qwen3-small adds a QKV bias, q / k norms, an fp8 KV cache."""
    from langstream_amd.engine.arena import PyStepExecutor
    from langstream_amd.engine.llm_engine import NSLOTS
    cfg = dataclasses.replace(PRESETS[name], qkv_bias=bias)
    model = LlamaModel(cfg, device=DEV, weights_dtype="int4")
    for layer in model.layers if bias else ():
        layer.qkv_b.normal_(0.0, 0.5)
        layer.q_norm.uniform_(0.5, 1.5)
        layer.k_norm.uniform_(0.5, 1.5)
    kw = dict(num_blocks=128, max_model_len=1024, max_batch=8, **kw)
    eng = [LLMEngine(model, None, **kw)] + [LLMEngine(model, None, use_graphs=False, **kw) for _ in range(2)]
    eng[2].exec = PyStepExecutor(model, eng[2].kv_caches, eng[2].layout, NSLOTS, eng[2].nsplit, eng[2].bps, eng[2].device)
    outs = [_run_tops(e, PROMPTS[:4], SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True, logprobs=2 if i else 0))
            for i, e in enumerate(eng)]
    assert eng[0].stats["graph_steps"] > 0 and eng[0].stats["weights_dtype"] == "int4"
    assert eng[0].kv_cache_dtype == kw.get("kv_cache_dtype", "bf16") and all(len(ids) == 12 for ids, _ in outs[0])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            _same_or_near_tie(a, b)
    elems = sum(2 * getattr(l, n + "_w").numel() for l in model.layers for n in W8_NAMES)
    groups = sum(getattr(l, n + "_z").numel() for l in model.layers for n in W8_NAMES)
    assert eng[0].stats["weight_bytes"] == LlamaModel(cfg, device=DEV).weight_bytes - (3 * elems) // 2 + 5 * groups
