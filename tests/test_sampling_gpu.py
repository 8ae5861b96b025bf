"""sampling.hip against its CPU model (sampling_oracle.py): the kernel has to return the
token the oracle says, not one that roughly follows the softmax.

Every replayed token must lie in the oracle's kept set and its f64 oracle score must be
within DELTA of the oracle's best score.  DELTA covers the device's fast log / exp (and the
FMA the compiler may form of ``z - log2(..) * ln 2``) and nothing else: the noise, the bins
and the cut are replayed exactly.  Measured on an MI355X, the largest deficit over all the
replay rows (and over the key, masked and vocab-parallel rows as well) is 0.0 nat: every
row returned the oracle's own token.  DELTA = max(4 x measured, 1e-3) = 1e-3 nat.  0.25 nat is
the hard ceiling; where the oracle's margin exceeds DELTA the token must be the oracle's.
test_sampling_oracle_cpu.py asserts the input conditions of every fixture used here.

Which branch of sweep() each layout and size reaches (N = 16 / sizeof(T), nt = 1024):

  odd_pitch, offset (any size)            scalar loop only
  aligned / tail, V = 3                   tail only
  tail, V = N*nt - 1, N*nt + 1            one vector round + tail
  aligned, V = N*3*nt                     three single vector rounds, unrolled loop not entered
  aligned, V = N*3*nt + N                 unrolled round (thread 0 only) + single rounds
  tail, V = N*5*nt + 5                    unrolled round + single round(s) + tail
  aligned, V = 128256 (f32)               seven / eight unrolled rounds + single rounds

for f32 and bf16 alike.  The tp_* kernels (f32) run 16032-column slices (aligned, unrolled),
4008-column slices (aligned, single rounds) and 10669 / 3-column slices (scalar).
"""
import math

import numpy as np
import pytest
import torch

import sampling_oracle as so
from langstream_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
MEASURED_DEFICIT = 0.0        # nat, largest over all replayed rows on an MI355X (all picks equal the oracle's)
DELTA = max(4 * MEASURED_DEFICIT, 1e-3)
FILL = 60.0                   # what surrounds a view: larger than any logit, so a stray read shows


# ------------------------------------------------------------------------------ helpers
def place(x, layout, dtype):
    """The rows [B, V] (numpy f32 or a torch tensor) as a GPU view laid out as ``layout`` says."""
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    B, V = x.shape
    width, col = so.buffer_of(layout, V, dtype)
    buf = torch.full((B, width), FILL, dtype=TD[dtype], device=DEV)
    view = buf[:, col:col + V]
    view.copy_(x.to(DEV))
    esz = buf.element_size()
    aligned = view.data_ptr() % 16 == 0 and (view.stride(0) * esz) % 16 == 0
    assert aligned == (layout in ("aligned", "tail")), (layout, V, dtype)
    if layout == "tail":
        assert V % so.vec(dtype) != 0
    same = torch.allclose(view.float().cpu(), x.float(), rtol=0, atol=0, equal_nan=True)
    assert same, "fixture is not representable in " + dtype
    return view


def sample(view, T, k, p, seed, step, n_top):
    B = view.shape[0]
    out = ops.sample(view,
                     torch.tensor(T, dtype=torch.float32, device=DEV).expand(B).contiguous(),
                     torch.tensor(k, dtype=torch.int32, device=DEV).expand(B).contiguous(),
                     torch.tensor(p, dtype=torch.float32, device=DEV).expand(B).contiguous(),
                     torch.tensor(seed, dtype=torch.int64, device=DEV).expand(B).contiguous(),
                     torch.tensor(step, dtype=torch.int64, device=DEV).expand(B).contiguous(), n_top)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def lp_close(got, exp, what):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert np.isfinite(got).all(), f"{what}: {got}"
    err = np.abs(got - exp)
    assert (err <= 1e-3 + 1e-4 * np.abs(exp)).all(), f"{what}: max err {err.max():.3g}"


def check(case, out, rows=None):
    """Tokens, log-probs and top-n of a Case against the oracle; returns the largest deficit."""
    tok, lp, ti, tl = out
    worst = 0.0
    for r in (range(case.x.shape[0]) if rows is None else rows):
        x, t = case.x[r], int(tok[r])
        where = f"{case.name} row {r} (T={case.T[r]} k={case.k[r]} p={case.p[r]})"
        assert 0 <= t < x.size, where
        if case.T[r] <= 0:
            assert t == so.greedy(x), where
        else:
            o = so.replay(x, case.T[r], case.k[r], case.p[r], case.seed[r], case.step[r])
            assert o.loose[t], f"{where}: token {t} is outside the kept set (oracle picks {o.token})"
            d = o.best - o.score(t)
            worst = max(worst, d)
            assert d <= DELTA, f"{where}: token {t} scores {d:.4g} nat under the oracle's {o.token}"
            if o.margin > DELTA:
                assert t == o.token, where
        lz = so.log_z(x)
        lp_close(lp[r], float(x[t]) - lz, where + " logprob")
        if ti is not None:
            ids = so.top_n(x, ti.shape[1])
            assert ti[r].tolist() == ids.tolist(), where + " top ids"
            lp_close(tl[r], x[ids].astype(np.float64) - lz, where + " top logprobs")
    print(f"deficit {case.name} {worst:.3e}")
    return worst


def run_case(case):
    view = place(case.x, case.layout, case.dtype)
    return sample(view, case.T, case.k, case.p, case.seed, case.step, case.n_top)


# ---------------------------------------------------------------------- planted positions
PLANTED = [(d, l, V) for d in so.DTYPES for l in so.LAYOUTS for V in so.sizes(d) if so.layout_ok(l, V, d)]
PLANTED.append(("f32", "aligned", 128256))


@pytest.mark.parametrize("dtype,layout,V", PLANTED)
def test_planted_positions(dtype, layout, V):
    """A constant -30 row with one (then two) elements at 0, at every boundary of the sweep: a
    vector, round or tail that is skipped loses the plant, one visited twice or mis-indexed
    moves the token, and either moves the log-prob by log 2."""
    pos = so.planted_positions(layout, V, dtype)
    B = len(pos)
    assert B >= 2
    one = torch.full((B, V), -30.0)
    two = torch.full((B, V), -30.0)
    pairs = [tuple(sorted((pos[r], pos[(r + 1) % B]))) for r in range(B)]
    for r in range(B):
        one[r, pos[r]] = 0.0
        two[r, list(pairs[r])] = 0.0
    v1, v2 = place(one, layout, dtype), place(two, layout, dtype)
    seeds, steps = list(range(11, 11 + B)), list(range(B))
    for T, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 0, 0.5)):
        what = f"T={T} k={k} p={p}"
        tok, lp, ti, tl = sample(v1, T, k, p, seeds, steps, 2)
        assert tok.tolist() == pos, what
        assert ti[:, 0].tolist() == pos, what
        assert ti[:, 1].tolist() == [1 if q == 0 else 0 for q in pos], what     # all equal: the lowest index
        lp_close(lp, np.zeros(B), what + " logprob")
        lp_close(tl[:, 0], np.zeros(B), what + " top logprob")
        tok, lp, ti, tl = sample(v2, T, k, p, seeds, steps, 2)
        for r in range(B):
            assert int(tok[r]) in pairs[r] and (T > 0 or int(tok[r]) == pairs[r][0]), (what, r, tok[r], pairs[r])
            assert tuple(ti[r].tolist()) == pairs[r], (what, r)
        lp_close(lp, np.full(B, -math.log(2)), what + " logprob, two plants")
        lp_close(tl, np.full((B, 2), -math.log(2)), what + " top logprobs, two plants")


# --------------------------------------------------------------------------------- replay
@pytest.mark.parametrize("case", so.replay_cases(), ids=lambda c: c.name)
def test_replay(case):
    check(case, run_case(case))


@pytest.mark.parametrize("case", so.key_cases(), ids=lambda c: c.name)
def test_determinism_and_keys(case):
    """One row under steps 0..63 gives the oracle's 64 tokens (and the same tokens wherever
    the rows sit in the batch); seeds above 2^32 and negative seeds / steps wrap as int64."""
    out = run_case(case)
    check(case, out)
    assert len(set(out[0].tolist())) > 1
    B = case.x.shape[0]
    perm = [(7 * r + 3) % B for r in range(B)]
    assert sorted(perm) == list(range(B))
    view = place(case.x, case.layout, case.dtype)
    tok2 = sample(view, case.T, case.k, case.p, [case.seed[q] for q in perm], [case.step[q] for q in perm], 0)[0]
    assert tok2.tolist() == [int(out[0][q]) for q in perm]


@pytest.mark.parametrize("case", so.top_draw_case(), ids=lambda c: c.name)
def test_largest_draw_is_below_one(case):
    """The element that draws 24 one-bits sits 20 nats down and must lose: (float)0xffffff +
    0.5f rounds to 2^24, and an unclamped u = 1 gives it infinite noise."""
    out = run_case(case)
    assert int(out[0][0]) != so.TOP_DRAW_INDEX
    check(case, out)


# ----------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("layout", ["tail", "odd_pitch"])
@pytest.mark.parametrize("dtype", so.DTYPES)
def test_ties_lowest_index_first(dtype, layout):
    N, nt = so.vec(dtype), so.NT
    V = N * 5 * nt + 5
    nvec = V // N
    groups = [(0, N), (3 * N, 70 * N), ((nt - 1) * N, nt * N), (5 * N, (4 * nt + 5) * N), (9 * N + 1, nvec * N),
              (V - 2, V - 1), (2 * N + 1, 2 * N + 2, (2 * nt + 2) * N), (1, nt + 1, 64), ()]
    rng = np.random.default_rng(77)
    x = np.minimum(rng.standard_normal((len(groups), V)) * 3, 10.0).astype(np.float32)
    for r, g in enumerate(groups):
        x[r, list(g)] = 20.0
    x[-1] = 1.5                                   # a constant row: 0, 1, 2, ... in order
    if dtype == "bf16":
        x = so.round_bf16(x)
    view = place(x, layout, dtype)
    for n_top in (1, 32):
        tok, lp, ti, tl = sample(view, 0.0, 0, 1.0, 1, 2, n_top)
        for r, g in enumerate(groups):
            ids = so.top_n(x[r], n_top)
            assert int(tok[r]) == so.greedy(x[r]) == (min(g) if g else 0)
            assert ti[r].tolist() == ids.tolist(), (r, n_top)
            assert ids[:len(g)].tolist() == sorted(g)[:n_top]
            lz = so.log_z(x[r])
            lp_close(tl[r], x[r][ids].astype(np.float64) - lz, f"row {r} top logprobs")
            lp_close(lp[r], float(x[r][int(tok[r])]) - lz, f"row {r} logprob")


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("dtype", so.DTYPES)
def test_top_n_equals_vocab(dtype, layout):
    x = np.array([[1, 3, 3, 2, 3, -1, 2, 0], [2, 2, 2, 2, 2, 2, 2, 2], [0, 1, 2, 3, 4, 5, 6, 7],
                  [7, 6, 5, 4, 4, 5, 6, 7]], dtype=np.float32)
    view = place(x, layout, dtype)
    for n_top in (1, 8):
        tok, lp, ti, tl = sample(view, 0.0, 0, 1.0, 0, 0, n_top)
        for r in range(x.shape[0]):
            ids = so.top_n(x[r], n_top)
            assert int(tok[r]) == so.greedy(x[r]) and ti[r].tolist() == ids.tolist(), (r, n_top)
            lp_close(tl[r], x[r][ids].astype(np.float64) - so.log_z(x[r]), f"row {r}")


# -------------------------------------------------------------------------- masked logits
@pytest.mark.parametrize("case", so.masked_cases(), ids=lambda c: c.name)
def test_masked_logits(case):
    """-inf at index 0, at every lane's first element, over a whole vector and over all but two
    entries; greedy and sampled, restricted and not: never a masked token, finite log-probs."""
    out = run_case(case)
    tok, lp, ti, tl = out
    for r in range(case.x.shape[0]):
        assert np.isfinite(case.x[r][int(tok[r])]), (case.name, r)
        assert np.isfinite(case.x[r][ti[r]]).all(), (case.name, r)
    assert np.isfinite(lp).all() and np.isfinite(tl).all()
    check(case, out)


@pytest.mark.parametrize("bad", [float("-inf"), float("nan")])
@pytest.mark.parametrize("layout", ["aligned", "odd_pitch"])
@pytest.mark.parametrize("dtype", so.DTYPES)
def test_row_without_a_finite_entry(dtype, layout, bad):
    """Between two ordinary rows, a row with no finite entry returns a token in [0, V) (its
    log-prob is unspecified) and leaves its neighbours' results as they are without it."""
    N = so.vec(dtype)
    V = N * so.NT + (N if layout == "aligned" else 1)
    g = torch.Generator().manual_seed(5)
    rows = (torch.randn(3, V, generator=g) * 3).to(TD[dtype]).float()
    pair = rows[[0, 2]].clone()
    rows[1] = bad
    for T, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 5, 0.9)):
        a = sample(place(rows, layout, dtype), T, k, p, [3, 4, 5], [6, 7, 8], 3)
        b = sample(place(pair, layout, dtype), T, k, p, [3, 5], [6, 8], 3)
        assert 0 <= int(a[0][1]) < V and ((0 <= a[2][1]) & (a[2][1] < V)).all()
        for got, exp in zip(a, b):
            assert np.array_equal(got[[0, 2]], exp), (T, k, p)


# -------------------------------------------------------------------------- vocab-parallel
def tp_sample(logits, W, T, k, p, seed, step, n_top):
    """The four tp_sample_* phases over W vocabulary slices of f32 ``logits`` [R, V], the
    exchanges done in torch (all-gather = concatenation, all-reduce = sum)."""
    h = ops.hip()
    R, V = logits.shape
    per = (V + W - 1) // W
    sl = [(min(V, w * per), min(V, (w + 1) * per)) for w in range(W)]
    parts = [logits[:, a:b].contiguous() for a, b in sl]
    stats = []
    for (a, _), part in zip(sl, parts):
        st = torch.empty(R * 4, device=DEV)
        h.tp_sample_stats(part, a, st)
        stats.append(st)
    stats_all = torch.cat(stats)
    hist = torch.zeros(R * 2 * 1024, dtype=torch.int64, device=DEV)
    for part in parts:
        hh = torch.empty_like(hist)
        h.tp_sample_hist(part, V, T, k, p, stats_all, W, hh)
        hist += hh
    cands = []
    for (a, _), part in zip(sl, parts):
        c = torch.empty(R * (3 + 2 * n_top), device=DEV)
        h.tp_sample_pick(part, a, V, T, k, p, seed, step, stats_all, W, hist, n_top, c)
        cands.append(c)
    tok = torch.empty(R, dtype=torch.int32, device=DEV)
    lp = torch.empty(R, device=DEV)
    ti = torch.empty(R * n_top, dtype=torch.int32, device=DEV)
    tl = torch.empty(R * n_top, device=DEV)
    h.tp_sample_final(stats_all, torch.cat(cands), W, R, T, n_top, tok, lp, ti, tl)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy(), ti.view(R, n_top).cpu().numpy(), tl.view(R, n_top).cpu().numpy(), parts


@pytest.mark.parametrize("tc", so.tp_cases(), ids=lambda t: t.name)
def test_vocab_parallel(tc):
    """Slices that are aligned and cross the unrolled threshold (16032 columns: the engine's
    shard), masked rows with one rank's whole slice banned, the maximum on two ranks, slices
    shorter than n_top: equal to the single-GPU kernel, and right by the oracle."""
    c = tc.case
    R, V = c.x.shape
    logits = torch.from_numpy(c.x).to(DEV)
    T = torch.tensor(c.T, dtype=torch.float32, device=DEV)
    k = torch.tensor(c.k, dtype=torch.int32, device=DEV)
    p = torch.tensor(c.p, dtype=torch.float32, device=DEV)
    seed = torch.tensor(c.seed, dtype=torch.int64, device=DEV)
    step = torch.tensor(c.step, dtype=torch.int64, device=DEV)
    one = ops.sample(logits, T, k, p, seed, step, n_top=tc.n_top)
    tok, lp, ti, tl, parts = tp_sample(logits, tc.W, T, k, p, seed, step, tc.n_top)
    if (V, tc.W) in ((128256, 8), (32064, 2), (32064, 8)):
        assert all(q.data_ptr() % 16 == 0 and q.stride(0) % 4 == 0 for q in parts)
        assert (parts[0].shape[1] // 4 > 3 * so.NT) == (parts[0].shape[1] == 16032)
    if V == 20:
        assert max(q.shape[1] for q in parts) < tc.n_top
    assert np.array_equal(one[0].cpu().numpy(), tok)
    assert np.abs(one[1].cpu().numpy() - lp).max() < 1e-4
    assert np.array_equal(one[2].cpu().numpy(), ti)
    assert np.abs(one[3].cpu().numpy() - tl).max() < 1e-4
    check(c, (tok, lp, ti, tl))
    if V > 1000:                                  # rows 0 and 6: the maximum sits on ranks 0 and W - 1
        per = (V + tc.W - 1) // tc.W
        assert tok[0] == per - 3 and ti[0][:2].tolist() == [per - 3, (tc.W - 1) * per + 17]
        assert ti[6][:2].tolist() == [per - 3, (tc.W - 1) * per + 17] and tok[6] in ti[6][:2]


# ---------------------------------------------------------------------- apply_logit_deltas
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dtype", so.DTYPES)
def test_apply_logit_deltas(dtype, strided):
    """Against the CPU branch of the same function (sequential adds).  Logits and deltas are
    multiples of 1/8 small enough that every partial sum is exact in bf16, so any order of
    the atomic adds gives the same bits and the comparison is exact.  (row, tok) pairs repeat
    two and three times, within one wave and across blocks; tokens -1 and V are skipped."""
    B, V, n = 5, 301, 700
    g = torch.Generator().manual_seed(9)
    base = (torch.randint(-32, 33, (B, V), generator=g).float() / 8).to(TD[dtype])
    rows = torch.randint(0, B, (n,), generator=g, dtype=torch.int32)
    toks = torch.randint(0, V, (n,), generator=g, dtype=torch.int32)
    delta = torch.randint(-16, 17, (n,), generator=g).float() / 8
    for (r, t), where in (((1, 7), (3, 4)), ((2, 11), (10, 11, 40)), ((3, 5), (20, 600)), ((0, V - 1), (100, 300, 650)),
                          ((4, 0), (255, 256))):
        for i in where:
            rows[i], toks[i], delta[i] = r, t, 0.625 + i / 8 % 1
    toks[[50, 290, 699]] = -1
    toks[[51, 513]] = V
    keys = (rows.long() * (V + 2) + toks.long()).tolist()
    assert max(keys.count(q) for q in set(keys)) >= 3
    exp = base.clone()
    ops.apply_logit_deltas(exp, rows, toks, delta)            # CPU tensors: the sequential branch
    if strided:
        buf = torch.full((B, V + 27), FILL, dtype=TD[dtype], device=DEV)
        view = buf[:, 1:1 + V]
        view.copy_(base)
    else:
        buf = view = base.to(DEV)
    ops.apply_logit_deltas(view, rows.to(DEV), toks.to(DEV), delta.to(DEV))
    assert torch.equal(view.cpu(), exp)
    assert not torch.equal(exp, base)
    if strided:
        assert (buf[:, 0] == FILL).all() and (buf[:, 1 + V:] == FILL).all()
    e = torch.empty(0, dtype=torch.int32, device=DEV)
    ops.apply_logit_deltas(view, e, e, torch.empty(0, device=DEV))      # n = 0
    assert torch.equal(view.cpu(), exp)
