"""The CPU model of the sampler (sampling_oracle.py) checked on its own, and the input
conditions of the GPU tests asserted on the very fixtures those tests use.

* noise: fixed vectors worked out from the C++ of sampling.hip with Python integers;
* kept set: against the exact top-k / top-p rule of ops.reference.sample.  With ONE
  restriction and one element in the cut bin the two sets are equal; otherwise the oracle
  keeps the cut bin whole, so its set is a superset of the exact one and reaches at most
  1/32 scaled nat below the last exact element.  With BOTH restrictions the kernel (and the
  oracle) intersect top-k with top-p of the whole row, while the reference renormalises
  inside the top-k set first: the exact set compared against is that intersection, and
  the reference's own set is checked to lie inside it;
* input conditions (sampling_oracle.conditions_ok) on every sampled fixture, the share of
  replay rows whose pick is clear by more than 0.25 nat, and the coverage the fixtures
  promise: every top_k x top_p x T combination, every branch of sweep() for both dtypes.
"""
import math

import numpy as np
import torch

import sampling_oracle as so
from langstream_amd.ops import reference as ref


# ------------------------------------------------------------------------------ noise
def test_row_key_vectors():
    assert so.row_key(0, 0) == 0x0
    assert so.row_key(1, 0) == 0x7DF2D060
    assert so.row_key(0, 1) == 0x469913F8
    assert so.row_key(1234, 56) == 0x496F765B
    assert so.row_key((1 << 32) + 5, 0) == 0x4F4B38D8            # seed above 2^32
    assert so.row_key(-1, 1) == 0xB0840F9A                       # int64 -1 = 2^64 - 1
    assert so.row_key(-(1 << 63), 2) == 0xCFE6F112
    assert so.row_key(-1, 1) == so.row_key((1 << 64) - 1, 1)


def test_uniform01_vectors():
    key = 0x496F765B
    idx = np.array([0, 1, 128255, 0xFFFFFFFF], dtype=np.uint32)
    h = so.hash32(idx.astype(np.uint64) * np.uint64(0x9E3779B9) + np.uint64(key))
    assert [int(v) for v in h] == [0xB794BBBD, 0xBC81DDAF, 0x42CE9672, 0x15B09E2D]
    # top 24 bits 12031163, 12354013 (odd and >= 2^23: the f32 sum x + 0.5 ties to even, x + 1),
    # 4378262, 1421470 (< 2^23: x + 0.5 is exact)
    exp = [12031164 / 2 ** 24, 12354014 / 2 ** 24, 4378262.5 / 2 ** 24, 1421470.5 / 2 ** 24]
    assert so.uniform01(key, idx).tolist() == exp


def test_uniform01_stays_below_one():
    # hash32 is a bijection: invert it for a value whose 24 top bits are ones.  (float)0xffffff
    # + 0.5f rounds to 2^24, i.e. u = 1 and Gumbel noise +inf, unless the draw is clamped.
    for h in (0, 1, 0xDEADBEEF, 0xFFFFFFFF):
        assert int(so.hash32(np.array([so.hash32_inv(h)]))[0]) == h
    key = so.row_key(so.TOP_DRAW_SEED, so.TOP_DRAW_STEP)
    i = so.index_with_top_draw(key, so.TOP_DRAW_V)
    assert i == so.TOP_DRAW_INDEX
    h = int(so.hash32(np.array([i * 0x9E3779B9 + key], dtype=np.uint64))[0])
    assert h >> 8 == 0xFFFFFF
    assert np.float32(h >> 8) + np.float32(0.5) == np.float32(2 ** 24)
    u = so.uniform01(key, np.arange(so.TOP_DRAW_V, dtype=np.uint32))
    assert u.max() == u[i] == 1.0 - 2.0 ** -24 and u.min() > 0.0


# --------------------------------------------------------------------- bins and the cut
def test_bins_scalar_model():
    """bins() against the kernel's expression evaluated element by element."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(300) * 3).astype(np.float32)
    x[7] = -np.inf
    for T in (0.25, 0.7, 1.3, 100.0):
        z, b, _ = so.bins(x, T)
        gm, invT = np.float32(x.max()), np.float32(1.0) / np.float32(T)
        for i in range(x.size):
            zi = np.float32(np.float32(x[i] - gm) * invT)
            bi = min(1023, int(np.float32(np.float32(zi + np.float32(32.0)) * np.float32(32.0)))) if zi >= -32 else -1
            assert (b[i], z[i]) == (bi, zi)
    assert so.bins(x, 1.0)[1][7] == -1 and so.bins(x, 1.0)[1][int(x.argmax())] == 1023


def test_cut_rules_by_hand():
    # z = 0, -1/32, -2/32, -3/32 -> bins 1023, 1023 (boundary of the clamp), 1022, 1021 ...
    x = np.array([0.0, -0.5, -0.5, -1.0, -8.0, -40.0], dtype=np.float32)
    z, b, _ = so.bins(x, 1.0)
    assert b.tolist() == [1023, 1008, 1008, 992, 768, -1]
    assert so.cut(z, b, 6, 1, 1.0)[0] == 1023
    assert so.cut(z, b, 6, 2, 1.0)[0] == 1008          # the cut bin is kept whole: 3 elements
    assert so.cut(z, b, 6, 3, 1.0)[0] == 1008
    assert so.cut(z, b, 6, 4, 1.0)[0] == 992
    assert so.cut(z, b, 6, 5, 1.0)[0] == 768
    assert so.cut(z, b, 6, 6, 1.0) == (-1, math.inf) and so.cut(z, b, 6, 0, 1.0)[0] == -1
    tot = 1 + 2 * math.exp(-0.5) + math.exp(-1) + math.exp(-8)
    c, m = so.cut(z, b, 6, 0, 0.5)
    assert c == 1008 and abs(m - min(abs(1 / tot - 0.5), abs((1 + 2 * math.exp(-0.5)) / tot - 0.5))) < 1e-6
    assert so.cut(z, b, 6, 1, 0.9)[0] == 1023          # both on: the higher bin wins
    assert so.cut(z, b, 6, 5, 1e-6)[0] == 1023
    r = so.cut_row(x, 1.0, 0, 1.0)
    assert r.cut == -1 and r.strict.all()              # unrestricted: everything finite, z < -32 included


def _exact_sets(x, T, k, p):
    """The exact kept sets by the rules of ops.reference.sample, in f64: (kernel semantics =
    top-k intersected with top-p of the whole row, the reference's own nested set)."""
    z = (x.astype(np.float64) - float(x.max())) / float(np.float32(T))
    pr = np.exp(z)
    V = x.size
    topk = np.ones(V, dtype=bool)
    if 0 < k < V:
        topk = pr >= np.sort(pr)[::-1][k - 1]

    def nucleus(q):
        order = np.argsort(-q, kind="stable")
        c = np.cumsum(q[order])
        keep = np.zeros(V, dtype=bool)
        keep[order[(c - q[order]) < float(np.float32(p)) * c[-1]]] = True
        return keep & (q > 0)
    if not 0 < p < 1:
        return topk, topk
    return topk & nucleus(pr), nucleus(np.where(topk, pr, 0.0))


def test_kept_set_against_the_exact_rule():
    seen_equal = seen_wider = 0
    for c in so.replay_cases():
        for r in range(c.x.shape[0]):
            x, T, k, p = c.x[r], c.T[r], c.k[r], c.p[r]
            o = so.cut_row(x, T, k, p)
            if o.cut < 0:
                assert o.strict.all()
                continue
            exact, nested = _exact_sets(x, T, k, p)
            assert not (nested & ~exact).any()
            assert not (exact & ~o.strict).any(), (c.name, r)
            if int((o.bin == o.cut).sum()) == 1:
                assert np.array_equal(o.strict, exact), (c.name, r)
                seen_equal += 1
            else:
                zmin = o.z[exact].min()
                assert (o.z[o.strict] >= zmin - 1.0 / 32 - 1e-6).all(), (c.name, r)
                seen_wider += 1
    assert seen_equal >= 20 and seen_wider >= 20, (seen_equal, seen_wider)


def test_reference_sampler_draws_lie_in_the_kept_set():
    c = so.replay_cases()[0]
    g = torch.Generator().manual_seed(1)
    for r in range(c.x.shape[0]):
        if so.cut_row(c.x[r], c.T[r], c.k[r], c.p[r]).cut < 0:
            continue
        o = so.cut_row(c.x[r], c.T[r], c.k[r], c.p[r])
        row = torch.from_numpy(c.x[r])[None].repeat(64, 1)
        tok, _ = ref.sample(row, [c.T[r]] * 64, [c.k[r]] * 64, [c.p[r]] * 64, [g] * 64)
        assert o.strict[tok.numpy()].all()


def test_pick_greedy_topn_logz():
    x = np.array([1.0, 3.0, -np.inf, 3.0, 0.5, 3.0, -1.0], dtype=np.float32)
    assert so.greedy(x) == 1 and so.top_n(x, 5).tolist() == [1, 3, 5, 0, 4]
    ref_lz = float(torch.logsumexp(torch.from_numpy(x).double(), 0))
    assert abs(so.log_z(x) - ref_lz) < 1e-12
    o = so.replay(x, 1.0, 0, 1.0, 3, 4)
    u = so.uniform01(so.row_key(3, 4), np.arange(7, dtype=np.uint32))
    gz = x.astype(np.float64) - 3.0 - np.log(-np.log(u))
    assert o.token == int(np.argmax(gz)) and o.token != 2 and not o.loose[2]
    srt = np.sort(gz[np.isfinite(gz)])
    assert abs(o.margin - (srt[-1] - srt[-2])) < 1e-12 and o.score(o.token) == o.best and o.score(2) == -np.inf
    assert so.replay(x, 1.0, 1, 1.0, 3, 4).token in (1, 3, 5)     # the cut bin holds the three maxima
    assert so.round_bf16(np.array([1.00390625, 1.01171875, -np.inf], np.float32)).tolist() == [1.0, 1.015625, -np.inf]
    t = torch.randn(1000) * 50
    assert np.array_equal(so.round_bf16(t.numpy()), t.bfloat16().float().numpy())


# ------------------------------------------------------------------- input conditions
def test_input_conditions_hold_on_every_gpu_fixture():
    rows = 0
    for c in so.sampled_cases():
        assert c.x.dtype == np.float32
        if c.dtype == "bf16":
            assert np.array_equal(so.round_bf16(c.x), c.x), c.name
        for r in range(c.x.shape[0]):
            if c.T[r] <= 0:
                continue
            o = so.cut_row(c.x[r], c.T[r], c.k[r], c.p[r])
            assert o.edges_at_cut == 0, (c.name, r)
            assert np.array_equal(o.loose, o.strict)
            if 0 < c.p[r] < 1:
                assert o.p_margin >= so.P_MARGIN, (c.name, r, o.p_margin)
            rows += 1
    assert rows > 300


def test_most_replay_rows_have_a_clear_pick():
    m = [so.replay(c.x[r], c.T[r], c.k[r], c.p[r], c.seed[r], c.step[r]).margin
         for c in so.replay_cases() for r in range(c.x.shape[0])]
    assert np.mean(np.array(m) > 0.25) >= 0.6, np.mean(np.array(m) > 0.25)


def test_replay_fixtures_cover_what_they_promise():
    cases = so.replay_cases()
    combos, keys = set(), set()
    for c in cases:
        V = c.V
        for r in range(c.x.shape[0]):
            combos.add((c.T[r], so.ks(V).index(c.k[r]) if V != 128256 else -1, c.p[r]))
            keys.add((c.seed[r], c.step[r]))
    assert len({q for q in combos if q[1] >= 0}) == len(so.TS) * 6 * len(so.PS)
    assert len(keys) == sum(c.x.shape[0] for c in cases)           # distinct seeds and steps
    assert sum(c.V == 128256 for c in cases) == 1
    for dtype in so.DTYPES:
        N, paths, lays = so.vec(dtype), set(), set()
        for c in cases:
            if c.dtype != dtype:
                continue
            lays.add(c.layout)
            paths |= set(so.sweep_path(c.layout, c.V, dtype).split("+"))
            width, col = so.buffer_of(c.layout, c.V, dtype)
            esz = 16 // N
            aligned = (width * esz) % 16 == 0 and (col * esz) % 16 == 0
            assert aligned == (c.layout in ("aligned", "tail")), c.name
            assert (c.V % N != 0) == (c.layout == "tail") or c.layout in ("offset", "odd_pitch")
        assert lays == set(so.LAYOUTS) and paths == {"scalar", "single", "unrolled", "tail"}
        assert {c.V for c in cases if c.dtype == dtype} >= set(so.sizes(dtype))


def test_planted_positions_cover_the_sweep_boundaries():
    N, V = 4, 4 * 5 * 1024 + 5
    pos = so.planted_positions("tail", V, "f32")
    nvec = V // N
    for q in (0, N - 1, N, nvec * N - 1, nvec * N, V - 1, 1023 * N, 1024 * N, 2 * 1024 * N, 3 * 1024 * N,
              (1023 + 3 * 1024) * N, 4 * 1024 * N, 5 * 1024 * N):
        assert q in pos, q
    big = so.planted_positions("aligned", 128256, "f32")
    assert 4 * 1024 * 4 in big and 128255 in big and (28672 + 320) * 4 in big    # remainder loop starts at thread 320
    assert so.planted_positions("odd_pitch", 3, "bf16") == [0, 2]
