"""MXFP4 projection weights on the GPU: mx4_skinny (<= 16 rows) and the tiled mx4_gemm of
ops/csrc/gemm_mx4.hip against a float64 product over the dequantised weight, and the engine.

EXACT operands: x in {+-1, +-2}, e2m1 weight values (<= 64 non-zeros per row), block scale bytes in
{126, 127, 128}, row scales in {0.5, 1, 2}: sums of <= 64 multiples of 0.25 below 24, exact in f32.

ENGINE tolerance: the reference alone (CPU mxfp4 model in f32 against bf16, the test's prompts;
top-1 log-prob gap / deficit of the chosen token): M = 3: 0.0455 / 0, M = 16: 0.1121 / 0.0855,
M = 129: 0.1927 / 0.1191.  TOL is twice the largest.
"""
import pytest
import torch

import gemm_probe as gp
import w8_operands as w8
from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaModel, PRESETS
from langstream_amd.ops import reference as ref
from test_weights_fp8_gpu import PROMPTS, _close_tops, _first_token_tops, _run_tops, _same_or_near_tie, _step_tops

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
SENTINEL = 77.0
TOL = 0.39
MAGS = torch.tensor(ref.E2M1_VALUES)


def _pack(values):   # e2m1 values [N, K] -> packed codes, low nibble first
    q = (values.abs()[:, :, None] == MAGS).int().argmax(2) | ((values < 0).int() << 3)
    q = q.to(torch.uint8).view(values.shape[0], -1, 2)
    return (q[:, :, 0] | (q[:, :, 1] << 4)).contiguous()


def _operands(M, N, K, rounded=False):
    values = w8.make_codes(N, K).float()
    assert bool((values.view(N, K // 32, 32) != 0).any(2).any(0).all())       # every block counts in some row
    g = torch.Generator().manual_seed(3 + N + K)
    scales = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
    codes = _pack(values)
    wd = ref.dequantize_weight_mxfp4(codes, scales, torch.float64)
    assert torch.equal(ref.dequantize_weight_mxfp4(codes, torch.full_like(scales, 127)), values)
    xq = w8.make_x(M, K).to(FP8)
    xs = (w8.rounded_scales(M) if rounded else w8.exact_scales(M)).clone()
    return xq, xs, codes, scales, xq.double() @ wd.t()


def _form(M):
    return "skinny" if M <= 16 else f"bm{64 if M <= 64 else (128 if M < 512 else 256)}"


def _auto_splits(M, N, K):   # pick_split of gemm_mx4.hip, restated
    if M <= 16:
        want = 1024 // (N // 16)
    else:
        bm = int(_form(M)[2:])
        want = (256 if bm == 256 else 512) // (-(-M // bm) * (N // 128))
    return max(1, min(want, K // 128 // 4, 16))


def _run(xq, xs, codes, scales, splits=0):
    ops.w8_launch_counts(reset=True)
    got = ops.mx4_gemm(xq.to(DEV), xs.to(DEV), codes.to(DEV), scales.to(DEV), splits=splits)
    torch.cuda.synchronize()
    return got.cpu(), ops.w8_launch_counts(reset=True)


EXACT_CASES = (
    # both forms and every tile: one below, at and one above each threshold; K = 2816 is 22 K steps
    [(M, 128, 2816, 0) for M in (1, 4, 16, 17, 64, 65, 128, 129, 511, 512, 513)]
    # one and three column tiles, one and two K steps
    + [(M, N, K, 0) for M in (5, 65, 513) for N in (128, 384) for K in (128, 256)]
    # forced uneven slices of the 22 steps on the skinny form and on each tile; more slices than K steps
    + [(16, 128, 2816, 3), (5, 128, 2816, 7), (64, 128, 2816, 5), (129, 128, 2816, 3), (513, 128, 2816, 7),
       (5, 128, 256, 6), (65, 128, 256, 6)]
)


# arbitrary row scales on the exact accumulator: unsplit on each form and tile, and split
ROUNDED_CASES = [(M, 128, 2816, sp) for M, sp in ((5, 1), (65, 1), (513, 1), (16, 3), (129, 3))]


@pytest.mark.parametrize("M,N,K,splits,rounded", [c + (False,) for c in EXACT_CASES] + [c + (True,) for c in ROUNDED_CASES])
def test_mx4_gemm_exact_and_rounded(M, N, K, splits, rounded):
    xq, xs, codes, scales, acc = _operands(M, N, K, rounded)
    got, census = _run(xq, xs, codes, scales, splits)
    S = min(splits, K // 128) if splits else _auto_splits(M, N, K)
    assert census == {f"mx4_{_form(M)}_s{S}": 1}, census
    want = acc * xs.double()[:, None]
    if rounded and S > 1:       # the project's rounded rule
        assert bool(((got.double() - want).abs() <= gp.RTOL * want.abs() + gp.FLOOR).all())
    else:                       # exact scales: acc * xs is exact; arbitrary ones: one f32 rounding, then bf16
        assert torch.equal(got, (acc.float() * xs[:, None]).to(torch.bfloat16))


@pytest.mark.parametrize("route", ["tile", "skinny"])
@pytest.mark.parametrize("splits", [1, 2])
def test_mx4_every_code_every_position(route, splits):
    """x the identity: out[m, n] = value(q[n, m]) * 2^(s[n, m // 32] - 127).  A wrong nibble order, K
    order inside a lane's group, or a scale of the wrong row or block changes an output."""
    n, k = torch.arange(128)[:, None], torch.arange(256)[None, :]
    q = ((n + k) % 16).to(torch.uint8).view(128, 128, 2)
    codes = (q[:, :, 0] | (q[:, :, 1] << 4)).contiguous()
    scales = (125 + (3 * n + torch.arange(8)[None, :]) % 5).to(torch.uint8)
    want = ref.dequantize_weight_mxfp4(codes, scales).t().to(torch.bfloat16)       # [m = k, n], exact in bf16
    xq = torch.eye(256).to(FP8)
    for r0, rows in ([(0, 256)] if route == "tile" else [(r, 16) for r in range(0, 256, 16)]):
        got, census = _run(xq[r0:r0 + rows].contiguous(), torch.ones(rows), codes, scales, splits)
        assert census == {f"mx4_{'bm128' if route == 'tile' else 'skinny'}_s{splits}": 1}, census
        assert torch.equal(got, want[r0:r0 + rows]), r0


BAD = {
    "ok": (None, {}),
    "w dtype": ("uint8", dict(w=lambda a: a["w"].view(torch.int8))),
    "N = 96": ("multiples of 128|N % 128", dict(w=lambda a: a["w"][:96].contiguous(), s=lambda a: a["s"][:96].contiguous(),
                                                out=lambda a: a["out"][:, :96])),
    "scale shape": (r"\[N, K / 32\]", dict(s=lambda a: a["s"][:, :-1].contiguous())),
    "misaligned x": ("16-byte aligned", dict(x=lambda a: a["wide"][1:8, 9:265])),
    "short workspace": ("workspace", dict(workspace=lambda a: a["workspace"][: 2 * 7 * 128 - 1], splits=lambda a: 2)),
}


@pytest.mark.parametrize("case", list(BAD))
def test_linear_mxfp4_views_and_guards(case):
    """x a window of a wider tensor, out inside a sentinel frame; a bad argument raises and writes
    nothing.  x in {+-1, +-2} quantises exactly, so only the product with xs rounds, as in f32."""
    M, N, K = 7, 128, 256
    _, _, codes, scales, _ = _operands(M, N, K)
    x = w8.make_x(M, K)
    wide = torch.full((M + 2, K + 64), 3.0, dtype=torch.bfloat16, device=DEV)
    wide[1:M + 1, 8:K + 8] = x.to(DEV)
    frame = torch.full((M + 2, N + 16), SENTINEL, dtype=torch.bfloat16, device=DEV)
    a = dict(out=frame[1:M + 1, 8:N + 8], x=wide[1:M + 1, 8:K + 8], w=codes.to(DEV), s=scales.to(DEV), wide=wide,
             workspace=torch.zeros(2 * M * N, device=DEV), splits=0)
    msg, kw = BAD[case]
    a.update({k: f(a) for k, f in kw.items()})
    call = lambda: ops.hip().linear_mxfp4(a["out"], a["x"], a["w"], a["s"], a["workspace"], a["splits"])  # noqa: E731
    if msg is None:
        call()
        assert torch.equal(frame[1:M + 1, 8:N + 8].cpu(), ref.linear_mxfp4(x, codes, scales))
        frame[1:M + 1, 8:N + 8] = SENTINEL
    else:
        with pytest.raises(RuntimeError, match=msg):
            call()
    torch.cuda.synchronize()
    assert bool((frame == SENTINEL).all()) and not bool(a["workspace"].any())


# ------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def small_pair():
    gpu = LlamaModel(PRESETS["llama-small"], device=DEV, weights_dtype="mxfp4")
    cpu = LlamaModel(gpu.cfg, device="cpu", dtype=torch.float32, weights_dtype="mxfp4")
    cpu.load_state_dict({k: v.cpu() for k, v in gpu.state_dict().items()})
    return gpu, cpu


def test_engine_mx4_graphs_match_eager_and_python(small_pair):
    """test_weights_fp8_gpu._graphs_vs_eager pins weights_dtype == "fp8": the same steps, composed here."""
    from langstream_amd.engine.arena import PyStepExecutor
    from langstream_amd.engine.llm_engine import NSLOTS
    gpu, _ = small_pair
    kw = dict(num_blocks=128, max_model_len=1024, max_batch=8)
    eng = [LLMEngine(gpu, None, **kw)] + [LLMEngine(gpu, None, use_graphs=False, **kw) for _ in range(2)]
    eng[2].exec = PyStepExecutor(gpu, eng[2].kv_caches, eng[2].layout, NSLOTS, eng[2].nsplit, eng[2].bps, eng[2].device)
    ops.w8_launch_counts(reset=True)
    outs = [_run_tops(e, PROMPTS, SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True, logprobs=2 if i else 0))
            for i, e in enumerate(eng)]
    assert eng[0].stats["graph_steps"] > 0 and eng[0].stats["weights_dtype"] == "mxfp4"
    assert eng[0].stats["weight_bytes"] == gpu.weight_bytes and all(len(ids) == 16 for ids, _ in outs[0])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            _same_or_near_tie(a, b)
    census = ops.w8_launch_counts(reset=True)
    assert census.get("quant", 0) > 0 and census.get("quant_silu", 0) > 0, census
    assert any(k.startswith("mx4_skinny") for k in census) and any(k.startswith("mx4_bm") for k in census), census
    assert not any(k.startswith(("gemm_", "gemv", "a8_", "w4_")) for k in census), census


@pytest.mark.parametrize("M", [3, 16, 129])
def test_runner_mx4_at_m_rows_matches_fp32(small_pair, M):
    """A prefill step and a decode step of M rows against the f32 CPU model with the same quantisation."""
    gpu, cpu = small_pair
    torch.manual_seed(M)
    prompt = [[int(t) for t in torch.randint(5, 30000, (M,))]]
    kw = dict(num_blocks=1024, max_model_len=1024, max_batch=512, max_prefill_tokens=4096)
    g = _first_token_tops(LLMEngine(gpu, None, **kw), prompt)[0]
    c = _first_token_tops(LLMEngine(cpu, None, **kw), prompt)[0]
    _close_tops(g, c, TOL)
    prompts = [[int(t) for t in torch.randint(5, 30000, (3,))] for _ in range(M)]
    eg = _step_tops(LLMEngine(gpu, None, use_graphs=False, **kw), prompts, 2)
    ec = _step_tops(LLMEngine(cpu, None, **kw), prompts, 2)
    same = 0
    for a, b in zip(eg, ec):
        _close_tops(a[0], b[0], TOL)
        if a[0].token_id == b[0].token_id:
            _close_tops(a[1], b[1], TOL)
            same += 1
    assert same >= 0.8 * M
