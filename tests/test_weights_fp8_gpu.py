"""FP8 (e4m3) projection weights on the GPU: the W8A16 kernels of ops/csrc/gemm_w8.hip against
ops.reference.linear_w8 in float64, and the engine serving ``weights_dtype="fp8"`` models
through the native runner (eager and under HIP graphs).

Kernel tests use the operand sets of w8_operands.py: EXACT inputs (small integers, code values
that are multiples of 0.5, scales in {0.5, 1, 2}) for which the output must EQUAL
bf16(reference) under any accumulation order and any K split, the same inputs with arbitrary
scales under the project's rounded rule, and all 254 finite codes through an identity x.  The
launch census (ops.w8_launch_counts) proves which kernel variant served each shape.
"""
import pytest
import torch

import gemm_probe as gp
import w8_operands as w8
from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaConfig, LlamaModel, PRESETS
from langstream_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
SENTINEL = 77.0

# M: one below, at and one above both row-tile heights (64, 128), 1 / 3 / 4 / 5 and one above two tiles
MS = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300)


def _bm(M):
    return 64 if M <= 64 else 128


def _auto_splits(M, N, K):
    """The launcher's rule (gemm_w8.hip pick_split), restated: a power of two <= 8, at least
    4 K steps per slice, only while tiles * splits <= 512."""
    tiles = -(-M // _bm(M)) * (N // 64)
    want, cap, s = 512 // tiles, min(8, K // 64 // 4), 1
    while s * 2 <= want and s * 2 <= cap:
        s *= 2
    return s


def _run(x, codes, s, splits=0, out=None):
    ops.w8_launch_counts(reset=True)
    got = ops.linear_w8(x, codes, s, out=out, splits=splits)
    torch.cuda.synchronize()
    return got, ops.w8_launch_counts(reset=True)


def _dev(M, N, K, rounded=False):
    s = w8.rounded_scales(N) if rounded else w8.exact_scales(N)
    return w8.make_x(M, K).to(DEV), w8.make_codes(N, K).to(DEV), s.to(DEV)


def _check_exact(got, M, N, K):
    want = w8.oracle(M, N, K).to(torch.bfloat16)
    assert torch.equal(got.cpu(), want), (M, N, K, (got.cpu().double() - want.double()).abs().max().item())


def _check_rounded(got, M, N, K):
    want = w8.oracle(M, N, K, rounded=True)
    err = (got.cpu().double() - want).abs()
    tol = gp.RTOL * want.abs() + gp.FLOOR
    assert bool((err <= tol).all()), (M, N, K, (err / tol).max().item())


# ------------------------------------------------------------------------------ w8_gemm
GEMM_CASES = (
    # every M at K = 2816 (44 K steps, llama-small's odd K; not a GEMV shape), two column tiles
    [(M, 128, 2816, 0) for M in MS]
    # one and three column tiles, one K step
    + [(M, N, 64, 0) for M in (5, 65, 129) for N in (64, 192)]
    # a K at which each automatic split count occurs (one column tile, one row tile)
    + [(5, 64, 64, 0), (5, 64, 512, 0), (5, 64, 1024, 0), (5, 64, 2048, 0), (130, 64, 2048, 0)]
    # forced split counts the launcher never picks, uneven slices (44 steps in 3 / 5 / 7 / 16), more than K steps
    + [(129, 128, 2816, 3), (64, 128, 2816, 5), (5, 192, 2816, 7), (300, 64, 2816, 16), (5, 64, 128, 6)]
    # M <= 4 where the GEMV's shape rule does not hold: K % 1024 != 0
    + [(4, 64, 1088, 0), (1, 128, 960, 0)]
)


@pytest.mark.parametrize("M,N,K,splits", GEMM_CASES)
def test_w8_gemm_exact(M, N, K, splits):
    assert w8.probes_seen(M, N, K)
    x, codes, s = _dev(M, N, K)
    got, census = _run(x, codes, s, splits)
    S = min(splits, K // 64) if splits else _auto_splits(M, N, K)
    assert census == {f"gemm_bm{_bm(M)}_s{S}": 1}, census
    _check_exact(got, M, N, K)


def test_w8_gemm_auto_splits_cover_every_count():
    """The cases above reach every split count the launcher can choose, on both tile heights."""
    seen = {(_bm(M), _auto_splits(M, N, K)) for M, N, K, sp in GEMM_CASES if sp == 0}
    assert {(64, 1), (64, 2), (64, 4), (64, 8), (128, 1), (128, 8)} <= seen, seen


@pytest.mark.parametrize("M,N,K,splits", [(5, 128, 2816, 0), (65, 192, 64, 0), (129, 128, 2816, 3), (300, 128, 2816, 0)])
def test_w8_gemm_rounded(M, N, K, splits):
    x, codes, s = _dev(M, N, K, rounded=True)
    got, census = _run(x, codes, s, splits)
    assert list(census) == [f"gemm_bm{_bm(M)}_s{splits or _auto_splits(M, N, K)}"], census
    _check_rounded(got, M, N, K)


# ------------------------------------------------------------------------------ w8_gemv
# K / 1024 chunks over 4 waves: 1 chunk (three idle waves), every chunks-per-wave count 1..7,
# and counts that leave the last round partial (14 = 3 rounds + 2, 5 = 1 round + 1)
GEMV_KS = (1024, 4096, 5120, 8192, 12288, 14336, 20480, 24576, 28672)


@pytest.mark.parametrize("K", GEMV_KS)
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_w8_gemv_exact(M, K):
    N = 64
    assert w8.probes_seen(M, N, K)
    x, codes, s = _dev(M, N, K)
    got, census = _run(x, codes, s)
    assert census == {"gemv": 1}, census
    _check_exact(got, M, N, K)


@pytest.mark.parametrize("M,K", [(1, 4096), (4, 14336)])
def test_w8_gemv_rounded(M, K):
    x, codes, s = _dev(M, 128, K, rounded=True)
    got, census = _run(x, codes, s)
    assert census == {"gemv": 1}, census
    _check_rounded(got, M, 128, K)


def test_w8_gemv_shape_rule_both_sides():
    """M <= 4 and K % 1024 == 0 -> the GEMV; one row more, or a K off the rule, -> the tiled kernel."""
    h = ops.hip()
    for M, K, key in [(4, 1024, "gemv"), (5, 1024, "gemm_bm64_s4"), (4, 1088, "gemm_bm64_s4"),
                      (4, 2816, "gemm_bm64_s8")]:
        x, codes, s = _dev(M, 64, K)
        got, census = _run(x, codes, s)
        assert census == {key: 1}, (M, K, census)
        _check_exact(got, M, 64, K)
        assert h.w8_gemv_supported(codes) == (K % 1024 == 0)
    assert h.w8_supported(w8.make_codes(64, 1024).to(DEV))
    assert not h.w8_supported(torch.zeros(64, 1024, dtype=torch.bfloat16, device=DEV))
    assert not h.w8_supported(torch.zeros(96, 1024, device=DEV).to(FP8))
    assert not h.w8_supported(torch.zeros(64, 1056, device=DEV).to(FP8))
    # forcing splits sends an M <= 4 GEMV shape to the tiled kernel
    x, codes, s = _dev(2, 64, 1024)
    got, census = _run(x, codes, s, splits=2)
    assert census == {"gemm_bm64_s2": 1}, census
    _check_exact(got, 2, 64, 1024)


# ------------------------------------------------------------------------------ all codes
@pytest.mark.parametrize("route", ["gemm", "gemm_split", "gemv"])
def test_w8_decodes_every_code_exactly(route):
    """Identity x: out[m, n] is the decoded value of code (n + m) mod 256 times s[n], for all 254
    finite codes (subnormals and +-448 included), in both kernels."""
    x, codes, s, expect = w8.all_codes_case()
    assert int(torch.isfinite(codes.float()).sum()) == codes.numel()
    assert len(set(codes.view(torch.uint8).flatten().tolist())) == 254
    if route == "gemv":
        # the GEMV needs K % 1024 == 0: the 256 columns repeated 4 times along K against an x that
        # is the identity on one repetition per row block, 4 rows at a time
        K = 1024
        cw = codes.view(torch.uint8).repeat(1, 4).contiguous().view(FP8).to(DEV)
        sd = s.to(DEV)
        for m0 in (0, 124, 252):
            xs = torch.zeros(4, K, dtype=torch.bfloat16)
            for i in range(4):
                xs[i, ((m0 + i) // 64) * 256 + m0 + i] = 1.0
            got, census = _run(xs.to(DEV), cw, sd)
            assert census == {"gemv": 1}
            assert torch.equal(got.cpu().double(), expect[m0:m0 + 4].to(torch.bfloat16).double()), m0
        return
    got, census = _run(x.to(DEV), codes.to(DEV), s.to(DEV), splits=4 if route == "gemm_split" else 1)
    assert census == {"gemm_bm128_s4" if route == "gemm_split" else "gemm_bm128_s1": 1}, census
    # value * s is a 4-bit significand times a power of two: bf16 holds it exactly
    assert torch.equal(got.cpu().double(), expect)


# ------------------------------------------------------------------------------ views and guards
@pytest.mark.parametrize("M,K,key", [(3, 1024, "gemv"), (70, 2816, "gemm_bm128_s8"), (5, 512, "gemm_bm64_s2")])
def test_w8_views_and_sentinels(M, K, key):
    """x as a row slice of a wider tensor, out as an interior block of a sentinel-filled one."""
    N = 128
    x, codes, s = _dev(M, N, K)
    wide = torch.full((M + 2, K + 64), 3.0, dtype=torch.bfloat16, device=DEV)
    wide[1:M + 1, 8:K + 8] = x
    xv = wide[1:M + 1, 8:K + 8]
    assert not xv.is_contiguous() and xv.data_ptr() % 16 == 0
    frame = torch.full((M + 2, N + 16), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ov = frame[1:M + 1, 8:N + 8]
    got, census = _run(xv, codes, s, out=ov)
    assert census == {key: 1}, census
    _check_exact(frame[1:M + 1, 8:N + 8], M, N, K)
    f = frame.cpu().float()
    assert bool((f[0] == SENTINEL).all() and (f[-1] == SENTINEL).all())
    assert bool((f[:, :8] == SENTINEL).all() and (f[:, N + 8:] == SENTINEL).all())


def test_w8_guards_refuse_and_write_nothing():
    h = ops.hip()
    M, N, K = 5, 128, 1024
    x, codes, s = _dev(M, N, K)
    ws = torch.zeros(8 * M * N, dtype=torch.float32, device=DEV)
    out = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    bf = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    bad = [
        ("x must be bf16", dict(x=x.float())),
        ("float8_e4m3fn", dict(w=bf)),
        ("s must be float32", dict(s=s.to(torch.bfloat16))),
        ("out must be bf16", dict(out=out.float())),
        ("contiguous", dict(w=codes.view(torch.uint8).t().contiguous().t().view(FP8))),
        ("N = 128", dict(s=torch.ones(N + 1, device=DEV)[:N + 1])),
        ("N = 128", dict(s=torch.ones(N - 1, device=DEV))),
        ("16-byte aligned", dict(s=torch.ones(N + 1, device=DEV)[1:])),
        ("16-byte aligned", dict(w=torch.zeros(N * K + 16, dtype=torch.uint8, device=DEV)[8:8 + N * K].view(N, K).view(FP8))),
        ("unit inner stride", dict(x=torch.zeros(M, 2 * K, dtype=torch.bfloat16, device=DEV)[:, ::2])),
        ("multiples of 64", dict(w=codes[:96].contiguous(), s=s[:96].contiguous(),
                                 out=torch.full((M, 96), SENTINEL, dtype=torch.bfloat16, device=DEV))),
        ("GPU tensors", dict(s=s.cpu())),
        ("GPU tensors", dict(x=x.cpu(), w=codes.cpu(), s=s.cpu(), out=out.cpu())),
        ("out must be", dict(out=torch.full((M + 1, N), SENTINEL, dtype=torch.bfloat16, device=DEV))),
        ("workspace", dict(workspace=ws[: 4 * M * N - 1], splits=4)),
        ("workspace", dict(workspace=ws.double(), splits=4)),
    ]
    for msg, kw in bad:
        a = dict(out=out, x=x, w=codes, s=s, workspace=ws, splits=0)
        a.update(kw)
        ws.zero_()
        with pytest.raises(RuntimeError, match=msg):
            h.w8_gemm(a["out"], a["x"], a["w"], a["s"], a["workspace"], a["splits"])
        torch.cuda.synchronize()
        assert bool((a["out"].float().cpu() == SENTINEL).all()), msg
        assert not bool(ws.any()), msg
    # the GEMV's own limits
    with pytest.raises(RuntimeError, match="M <= 4"):
        h.w8_gemv(out, x, codes, s)
    x4, c4, s4 = _dev(4, N, 1088)
    o4 = torch.full((4, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 1024"):
        h.w8_gemv(o4, x4, c4, s4)
    torch.cuda.synchronize()
    assert bool((out.float().cpu() == SENTINEL).all()) and bool((o4.float().cpu() == SENTINEL).all())
    # the bf16 projection kernels never take fp8 bytes
    for call in (lambda: h.gemv(o4, x4[:, :1024].contiguous(), codes),
                 lambda: h.decode_gemm(out, x, codes, ws),
                 lambda: h.skinny_gemm(out, x, codes),
                 lambda: h.gemm_prefill(out, x, codes, False)):
        with pytest.raises(RuntimeError):
            call()
    assert not h.gemm_prefill_supported(codes, False) and not h.decode_gemm_supported(codes, False)
    # the workspace bound holds for every row count below the one asked for
    for (n, k) in ((64, 2048), (6144, 4096), (1280, 1024)):
        top = h.w8_gemm_workspace(4096, n, k)
        for m in (1, 5, 64, 65, 128, 129, 256, 300, 1000, 4096):
            assert _auto_splits(m, n, k) * m * n * 4 * (_auto_splits(m, n, k) > 1) <= top, (m, n, k)
    with pytest.raises(RuntimeError, match="layers.0.qkv_w"):
        m = LlamaModel(PRESETS["llama-tiny"], device=DEV)
        caches = [ops.new_kv_cache(4, m.hkv, m.cfg.head_dim, DEV, torch.bfloat16) for _ in m.layers]
        m.layers[0].qkv_w = m.layers[0].qkv_w.to(FP8)
        m._native_runner(caches)


# ------------------------------------------------------------------------------ engine
def _w8_cpu_copy(model: LlamaModel) -> LlamaModel:
    """An f32 CPU model whose projections hold code * s."""
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    wide = {}
    for k, v in sd.items():
        if k.endswith("_s"):
            continue
        if v.dtype == FP8:
            v = ref.dequantize_weight_fp8(v, sd[k[:-2] + "_s"])
        wide[k] = v.float()
    cpu = LlamaModel(model.cfg, device="cpu", dtype=torch.float32)
    cpu.load_state_dict(wide)
    return cpu


def _first_token_tops(e, prompts, n_top=20):
    events = {}
    reqs = [e.submit(p, SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True, logprobs=n_top),
                     callback=lambda ev, i=i: events.setdefault(i, ev)) for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [events[i] for i in range(len(prompts))]


def _step_tops(e, prompts, n_gen, n_top=10):
    events = {}
    reqs = [e.submit(p, SamplingParams(max_tokens=n_gen, temperature=0.0, ignore_eos=True, logprobs=n_top),
                     callback=lambda ev, i=i: events.setdefault(i, []).append(ev)) for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [events[i] for i in range(len(prompts))]


def _close_tops(g, c, tol=0.05):
    cmap = dict(c.top)
    assert g.token_id in cmap and cmap[g.token_id] >= c.top[0][1] - tol
    assert abs(g.top[0][1] - c.top[0][1]) < tol


@pytest.fixture(scope="module")
def small_pair():
    gpu = LlamaModel(PRESETS["llama-small"], device=DEV, weights_dtype="fp8")
    assert gpu.layers[0].qkv_w.dtype == FP8 and gpu.layers[0].qkv_s.dtype == torch.float32
    return gpu, _w8_cpu_copy(gpu)


@pytest.mark.parametrize("M", [1, 4, 5, 64, 129, 300])
def test_runner_w8_at_m_rows_matches_fp32(small_pair, M):
    """The rule of test_runner_projection_routing_at_m_rows_matches_fp32 for an fp8 model: a
    prefill step of M tokens and a decode-only step of M rows against the f32 CPU model that
    holds code * s; the census shows W8 launches and not one bf16 projection kernel."""
    gpu, cpu = small_pair
    torch.manual_seed(M)
    prompt = [[int(t) for t in torch.randint(5, 30000, (M,))]]
    kw = dict(num_blocks=1024, max_model_len=1024, max_batch=512, max_prefill_tokens=4096)
    ops.w8_launch_counts(reset=True)
    ops.hip().decode_gemm_launch_counts(True)
    g = _first_token_tops(LLMEngine(gpu, None, **kw), prompt)[0]
    c = _first_token_tops(LLMEngine(cpu, None, **kw), prompt)[0]
    _close_tops(g, c)
    prompts = [[int(t) for t in torch.randint(5, 30000, (3,))] for _ in range(M)]
    eg = _step_tops(LLMEngine(gpu, None, use_graphs=False, **kw), prompts, 2)
    ec = _step_tops(LLMEngine(cpu, None, **kw), prompts, 2)
    same = 0
    for a, b in zip(eg, ec):
        _close_tops(a[0], b[0])
        if a[0].token_id == b[0].token_id:
            _close_tops(a[1], b[1])
            same += 1
    assert same >= 0.8 * M
    census = ops.w8_launch_counts(reset=True)
    L = gpu.cfg.num_layers
    assert sum(census.values()) >= 3 * 4 * L, census
    # llama-small: K = 1024 (qkv, o, gate_up) takes the GEMV at M <= 4, K = 2816 (down) never does
    assert ("gemv" in census) == (M <= 4), census
    # the only decode-GEMM launches are the LM head's (f32 output: the partial epilogue at one
    # split); a bf16 projection would show as store, silu or a split count above 1 -- and the
    # bf16 kernels refuse fp8 bytes anyway (test_w8_guards_refuse_and_write_nothing)
    dg = ops.hip().decode_gemm_launch_counts(True)
    assert all("_partial_" in k and k.endswith("_s1") for k in dg), dg


def _run_tops(e, prompts, sp):
    tops = {}
    reqs = [e.submit(p, sp, callback=lambda ev, i=i: tops.setdefault(i, []).append(ev.top))
            for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [(r.output_ids, tops.get(i)) for i, r in enumerate(reqs)]


def _same_or_near_tie(a, b, gap: float = 0.1) -> None:
    """The project's rule for greedy sequences of two bf16 paths (test_kv_fp8_gpu.py)."""
    (ids_a, _), (ids_b, tops_b) = a, b
    assert len(ids_a) == len(ids_b)
    for t, (x, y) in enumerate(zip(ids_a, ids_b)):
        if x == y:
            continue
        alt = dict(tops_b[t])
        assert x in alt and y in alt and abs(alt[x] - alt[y]) < gap, (t, x, y, tops_b[t])
        return


def _graphs_vs_eager(model, prompts, n_gen, python=False, **kw):
    """The native executor under HIP graphs against the eager native runner (python=True: the
    Python executor, whose forward calls ops.linear_w8 op by op)."""
    from langstream_amd.engine.arena import PyStepExecutor
    from langstream_amd.engine.llm_engine import NSLOTS
    kw = dict(dict(num_blocks=128, max_model_len=1024, max_batch=8), **kw)
    sp = SamplingParams(max_tokens=n_gen, temperature=0.0, ignore_eos=True)
    sp_ref = SamplingParams(max_tokens=n_gen, temperature=0.0, ignore_eos=True, logprobs=2)
    e1 = LLMEngine(model, None, **kw)
    assert e1.stats["weights_dtype"] == "fp8" and e1.stats["weight_bytes"] == model.weight_bytes
    ops.hip().decode_gemm_launch_counts(True)
    out1 = _run_tops(e1, prompts, sp)
    assert e1.stats["graph_steps"] > 0
    assert all(len(ids) == n_gen for ids, _ in out1)
    e2 = LLMEngine(model, None, use_graphs=False, **kw)
    if python:
        e2.exec = PyStepExecutor(model, e2.kv_caches, e2.layout, NSLOTS, e2.nsplit, e2.bps, e2.device)
    out2 = _run_tops(e2, prompts, sp_ref)
    for a, b in zip(out1, out2):
        _same_or_near_tie(a, b)
    return e1, e2


PROMPTS = [list(range(3, 3 + n)) for n in (5, 33, 64, 65, 200)]


def test_engine_w8_graphs_match_eager_and_python(small_pair):
    gpu, _ = small_pair
    _graphs_vs_eager(gpu, PROMPTS, 16)
    _graphs_vs_eager(gpu, PROMPTS, 16, python=True)
    bf = LlamaModel(PRESETS["llama-small"], device=DEV)
    # one byte less per projection element, four more per output row; embed, lm_head and norms stay bf16
    codes = sum(getattr(l, n + "_w").numel() for l in gpu.layers for n in ("qkv", "o", "gate_up", "down"))
    rows = sum(getattr(l, n + "_s").numel() for l in gpu.layers for n in ("qkv", "o", "gate_up", "down"))
    assert gpu.weight_bytes == bf.weight_bytes - codes + 4 * rows


@pytest.mark.parametrize("name,kw", [("qwen2-small", {}), ("qwen3-small", {}),
                                     ("llama-small", dict(kv_cache_dtype="fp8", kv_k_scale=0.5, kv_v_scale=2.0))])
def test_engine_w8_bias_qk_norm_and_fp8_kv(name, kw):
    model = LlamaModel(PRESETS[name], device=DEV, weights_dtype="fp8")
    for layer in model.layers:
        if layer.qkv_b is not None:
            layer.qkv_b.normal_(0.0, 0.5)
        if layer.q_norm is not None:
            layer.q_norm.uniform_(0.5, 1.5)
            layer.k_norm.uniform_(0.5, 1.5)
    e1, _ = _graphs_vs_eager(model, PROMPTS[:4], 12, python=True, **kw)
    if kw:
        assert e1.kv_cache_dtype == "fp8"


def test_engine_w8_batch_le4_gemv_graphs():
    """Decode batches of 1-4 rows on a model whose every K is a multiple of 1024: all four
    projections of a decode step run on w8_gemv, under graphs."""
    cfg = LlamaConfig(name="llama-gemv", vocab_size=32000, hidden_size=1024, intermediate_size=3072, num_layers=4,
                      num_heads=8, num_kv_heads=2, head_dim=128, max_position=4096, bos_token_id=1, eos_token_ids=(2,))
    model = LlamaModel(cfg, device=DEV, weights_dtype="fp8")
    for n in (1, 4):
        prompts = [list(range(3 + 7 * i, 3 + 7 * i + n_tok)) for i, n_tok in enumerate((5, 70, 129, 300)[:n])]
        ops.w8_launch_counts(reset=True)
        _graphs_vs_eager(model, prompts, 12)
        census = ops.w8_launch_counts(reset=True)
        assert census.get("gemv", 0) >= 4 * cfg.num_layers * 11, census   # the eager engine's decode steps alone


def test_engine_w8_chunked_prefill_mixed_steps(small_pair):
    gpu, _ = small_pair
    e1, e2 = _graphs_vs_eager(gpu, PROMPTS, 16, max_prefill_tokens=96)
    assert e1.stats["mixed_steps"] > 0 and e2.stats["mixed_steps"] > 0
