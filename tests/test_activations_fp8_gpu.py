"""FP8 activations on the GPU: the kernels of ops/csrc/gemm_w8a8.hip against ops.reference, and the engine."""
import pytest
import torch

import w8_operands as w8
from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine
from langstream_amd.models.llama import LlamaModel, PRESETS
from langstream_amd.ops import reference as ref
from test_weights_fp8_gpu import PROMPTS, _close_tops, _first_token_tops, _graphs_vs_eager, _step_tops

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
SENTINEL = 77.0
# The project's 0.05 is too tight once rows are re-quantised per projection: an e4m3 rounding
# flip moves a logit by more.  Measured on the reference alone -- the CPU a8 model in f32 against
# the same CPU model in bf16, on the prompts of test_runner_a8_at_m_rows_matches_fp32 -- the
# largest _close_tops gap is 0.0783 (M = 5), 0.1506 (64), 0.1625 (129), 0.1771 (300); the
# tolerance is twice the largest.
TOPS_TOL = 2 * 0.1771


def _rows(M, K, seed):
    """Normal rows; from 5 rows on a zero row, one with amax = 448 * 2^-3, one with a single huge element."""
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed))
    if M >= 5:
        x[1] = 0.0
        x[2] = x[2].clamp(-40.0, 40.0)
        x[2, K // 3] = -56.0
        x[3] *= 0.01
        x[3, K - 1] = 3.0e4
    return x.to(torch.bfloat16)


def _same_quant(got, want):
    assert torch.equal(got[1].cpu(), want[1]) and torch.equal(got[0].cpu().view(torch.uint8), want[0].view(torch.uint8))


@pytest.mark.parametrize("M,K,silu", [(M, K, False) for M in (1, 5, 65) for K in (128, 2816, 14336)]
                         + [(M, F, True) for M in (3, 65) for F in (128, 2816)])
def test_quantize_rows_equals_reference(M, K, silu):
    """silu: equal to the reference quantisation of the existing silu_and_mul kernel's output."""
    x = _rows(M, 2 * K if silu else K, M + K).to(DEV)
    ops.w8_launch_counts(reset=True)
    got = ops.quantize_rows_fp8(x, silu_mul=silu)
    assert ops.w8_launch_counts(reset=True) == {"quant_silu" if silu else "quant": 1}
    _same_quant(got, ref.quantize_rows_fp8((ops.silu_and_mul(x) if silu else x).cpu()))


# ------------------------------------------------------------------------------- GEMM, exact
def _bm(M):
    return 64 if M <= 64 else (128 if M < 512 else 256)


def _auto_splits(M, N, K):
    """The launcher's rule (gemm_w8a8.hip pick_split), restated."""
    tiles = -(-M // _bm(M)) * (N // 128)
    return max(1, min((256 if _bm(M) == 256 else 512) // tiles, K // 128 // 4, 16))


def _exact(M, N, K):
    return w8.make_x(M, K).to(FP8), w8.exact_scales(M, seed=1), w8.make_codes(N, K), w8.exact_scales(N)


GEMM_CASES = (
    # 5, 300, one below / at / above the tile heights 64, 128, 256 and the 512-row switch to the 256-row tile
    [(M, 128, 2816, 0) for M in (5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513)]
    + [(M, N, K, 0) for M in (5, 65, 513) for N in (128, 384) for K in (128, 256)]
    # 22 K steps in 3 / 5 / 7 uneven slices, on each tile
    + [(129, 128, 2816, 3), (64, 384, 2816, 5), (600, 128, 2816, 7), (5, 128, 256, 6)]
)


@pytest.mark.parametrize("M,N,K,splits", GEMM_CASES)
def test_w8a8_gemm_exact(M, N, K, splits):
    assert w8.probes_seen(M, N, K)
    xq, xs, codes, ws = _exact(M, N, K)
    ops.w8_launch_counts(reset=True)
    got = ops.w8a8_gemm(xq.to(DEV), xs.to(DEV), codes.to(DEV), ws.to(DEV), splits=splits)
    torch.cuda.synchronize()
    S = min(splits, K // 128, 16) if splits else _auto_splits(M, N, K)
    assert ops.w8_launch_counts(reset=True) == {f"a8_bm{_bm(M)}_s{S}": 1}
    want = ref.w8a8_gemm(xq, xs, codes, ws, dtype=torch.float64).to(torch.bfloat16)
    assert torch.equal(got.cpu(), want), (got.cpu().double() - want.double()).abs().max().item()


@pytest.mark.parametrize("side", ["weights", "activations"])
@pytest.mark.parametrize("splits", [1, 2])
def test_w8a8_every_code_exact(side, splits):
    """All 254 finite codes against an identity on the other side: a code decoded wrongly, or an
    A / B fragment pairing that differs inside a K step, changes an output."""
    x, codes, s, expect = w8.all_codes_case()
    eye, one = x.to(FP8).to(DEV), torch.ones(256, device=DEV)
    if side == "weights":
        got = ops.w8a8_gemm(eye, one, codes.to(DEV), s.to(DEV), splits=splits)
    else:
        got = ops.w8a8_gemm(codes.to(DEV), s.to(DEV), eye, one, splits=splits).t()
    assert torch.equal(got.cpu().double(), expect)


# ------------------------------------------------------------------------------- views and guards
BAD = {
    "ok": (None, {}),
    "x_f32": ("x must be bf16", dict(x=lambda a: a["x"].float())),
    "n_96": ("N % 128", dict(w=lambda a: a["w"][:96].contiguous())),
    "out_rows": ("out must be", dict(out=lambda a: torch.full((8, 128), SENTINEL, dtype=torch.bfloat16, device=DEV))),
    "x_misaligned": ("aligned", dict(x=lambda a: torch.zeros(7, 264, dtype=torch.bfloat16, device=DEV)[:, 4:260])),
    "workspace": ("workspace", dict(splits=lambda a: 2, workspace=lambda a: a["workspace"][:10])),
}


@pytest.mark.parametrize("case", list(BAD))
def test_linear_w8a8_views_and_guards(case):
    """x a row slice of a wider tensor, out inside a sentinel frame; a bad argument raises and
    leaves out untouched.  x in {+-1, +-2} quantises to +-224 / +-448 with xs = 2 / 448: the
    accumulator is exact and only the two scale products round, as in the f32 reference."""
    M, N, K = 7, 128, 256
    x = w8.make_x(M, K)
    wide = torch.full((M + 2, K + 64), 3.0, dtype=torch.bfloat16, device=DEV)
    wide[1:M + 1, 8:K + 8] = x.to(DEV)
    frame = torch.full((M + 2, N + 16), SENTINEL, dtype=torch.bfloat16, device=DEV)
    a = dict(out=frame[1:M + 1, 8:N + 8], x=wide[1:M + 1, 8:K + 8], w=w8.make_codes(N, K).to(DEV),
             ws=w8.rounded_scales(N).to(DEV), workspace=torch.zeros(2 * M * N, device=DEV), splits=0)
    msg, kw = BAD[case]
    a.update({k: f(a) for k, f in kw.items()})
    call = lambda: ops.hip().linear_w8a8(a["out"], a["x"], a["w"], a["ws"], a["workspace"], a["splits"])  # noqa: E731
    if msg is None:
        call()
        want = ref.linear_w8a8(x, w8.make_codes(N, K), w8.rounded_scales(N))
        assert torch.equal(frame[1:M + 1, 8:N + 8].cpu(), want)
        frame[1:M + 1, 8:N + 8] = SENTINEL
    else:
        with pytest.raises(RuntimeError, match=msg):
            call()
    torch.cuda.synchronize()
    assert bool((frame == SENTINEL).all()) and bool((a["out"] == SENTINEL).all())


# ------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def small_pair():
    gpu = LlamaModel(PRESETS["llama-small"], device=DEV, weights_dtype="fp8", activations_dtype="fp8")
    cpu = LlamaModel(gpu.cfg, device="cpu", dtype=torch.float32, weights_dtype="fp8", activations_dtype="fp8")
    cpu.load_state_dict({k: v.cpu() for k, v in gpu.state_dict().items()})
    return gpu, cpu


def test_engine_a8_graphs_match_eager_and_python(small_pair):
    gpu, _ = small_pair
    ops.w8_launch_counts(reset=True)
    e1, _ = _graphs_vs_eager(gpu, PROMPTS, 16)
    assert e1.stats["activations_dtype"] == "fp8"
    census = ops.w8_launch_counts(reset=True)
    assert census.get("quant", 0) > 0 and census.get("quant_silu", 0) > 0 and any(k.startswith("a8_") for k in census)
    assert not any(k.startswith("gemm_") for k in census), census
    _graphs_vs_eager(gpu, PROMPTS, 16, python=True)
    e1, e2 = _graphs_vs_eager(gpu, PROMPTS, 16, max_prefill_tokens=96)
    assert e1.stats["mixed_steps"] > 0 and e2.stats["mixed_steps"] > 0
    # decode batches of up to 4 rows: the W8A16 GEMV, no quantiser (llama-small's down, K = 2816, is no GEMV shape)
    _graphs_vs_eager(gpu, PROMPTS[:1], 2)
    ops.w8_launch_counts(reset=True)
    _graphs_vs_eager(gpu, [[3, 4, 5]], 8)
    census = ops.w8_launch_counts(reset=True)
    assert census.get("gemv", 0) > 0 and not any(k.startswith(("quant", "a8_")) for k in census), census


@pytest.mark.parametrize("M", [5, 64, 129, 300])
def test_runner_a8_at_m_rows_matches_fp32(small_pair, M):
    """A prefill step of M tokens and a decode step of M rows against the f32 CPU model with the
    same activation quantisation (test_runner_w8_at_m_rows_matches_fp32's rule)."""
    gpu, cpu = small_pair
    torch.manual_seed(M)
    prompt = [[int(t) for t in torch.randint(5, 30000, (M,))]]
    kw = dict(num_blocks=1024, max_model_len=1024, max_batch=512, max_prefill_tokens=4096)
    ops.w8_launch_counts(reset=True)
    g = _first_token_tops(LLMEngine(gpu, None, **kw), prompt)[0]
    c = _first_token_tops(LLMEngine(cpu, None, **kw), prompt)[0]
    print("prefill", M, g.top[0], c.top[0])
    _close_tops(g, c, TOPS_TOL)
    prompts = [[int(t) for t in torch.randint(5, 30000, (5,))] for _ in range(M)]
    eg = _step_tops(LLMEngine(gpu, None, use_graphs=False, **kw), prompts, 2)
    ec = _step_tops(LLMEngine(cpu, None, **kw), prompts, 2)
    same = 0
    for a, b in zip(eg, ec):
        _close_tops(a[0], b[0], TOPS_TOL)
        if a[0].token_id == b[0].token_id:
            _close_tops(a[1], b[1], TOPS_TOL)
            same += 1
    # the share of equal first tokens is not bounded: on these random-init logits e4m3 rounding
    # flips near ties (75 - 80 % agreed on an MI355X) and _close_tops bounds each flip; the second
    # step is compared where the first agrees, which must happen
    assert same > 0
    census = ops.w8_launch_counts(reset=True)
    assert any(k.startswith(f"a8_bm{_bm(M)}_") for k in census) and "gemv" not in census, census
