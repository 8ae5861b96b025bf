"""Integer operands for the GEMM tests (a plain module, shared by test_gemm_probe_cpu.py and
test_gemm_probe_gpu.py; torch only, everything here is built on the CPU).

With Gaussian operands one product of a K = 4096 row is ~0.016 and a whole 16-byte chunk
~0.044, below the 0.02-0.03 absolute tolerance of test_kernels_gpu.py: a GEMM that drops a
chunk, reads a ring slot one step early or mis-assigns a stage at a split boundary passes.
Here every operand is a small integer (exact in bf16) and the inputs are built so that

    sum_k |x[m, k]| |w[n, k]|  (+ |bias| + |residual|)  <=  BOUND

for every output, so every partial sum of ANY subset of the K products, in any order and
under any K split, is an integer of magnitude <= BOUND: f32 accumulation is exact, the bf16
(BOUND <= 256) or f32 result is exact, and the kernel must EQUAL the int64 reference.

    WIDE    x in {-2, -1, 1, 2}, min(K, 128) non-zeros (+-1) per w row         BOUND 256
    NARROW  x in {-1, 1}, 15 non-zeros per w row: every sum is odd, |sum| <= 15  BOUND 16
            (the epilogues that round: SwiGLU, RMSNorm; no gate / up sum is ever 0, so a
            unit error in either always shows)
    FP8     x in {-1, 1}, 7 non-zeros per w row: |sum| <= 7, exact in e4m3 at scales 1, 2, 0.5

The non-zeros of w are placed so that every probed column -- 0, K - 1, every multiple of
the kernel's K step and the column before it (which include every split boundary) -- is
non-zero in some row: zeroing one x element there changes an output.

Epilogues that round are compared with |got - ref| <= 2^-7 |ref| + 1e-6 against a float64
epilogue of the exact integer sums (the kernels compute in f32 and round once to bf16:
at most half a bf16 spacing, under 2^-8 |ref|; the allowance is twice that and covers
the f32 __expf / rsqrt; the floor is for silu of large negative sums).

A Case carries x, w, the epilogue (row-wise: epi(sums[R, N], rows[R]) -> {name: (f64
tensor, EXACT | ROUNDED)}), the K ranges of its splits and the column step of the kernel;
check_inputs asserts the conditions above, mutants() yields wrong results a faulty kernel
would produce and rejected() is the comparator the GPU test uses.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

EXACT, ROUNDED = "exact", "rounded"
RTOL, FLOOR = 2.0 ** -7, 1e-6
WIDE, NARROW, FP8 = "wide", "narrow", "fp8"
# operand set -> (x values, non-zeros per w row, bound on sum |x||w|)
SETS = {WIDE: ((-2, -1, 1, 2), 128, 256), NARROW: ((-1, 1), 15, 16), FP8: ((-1, 1), 7, 8)}
HALF = "half"      # gemv prologue forms: x = +-norm weight in {0.5, 1, 2}, 32 non-zeros: |sum| <= 64
SETS[HALF] = ((-1, 1), 32, 64)
NORM_W = (0.5, 1.0, 2.0)
EPS = 1e-5
BS = 64            # KV block size of the paged caches
SENTINEL = 77.0    # what guard rows, guard columns and untouched bf16 cache slots hold


# ------------------------------------------------------------------------------ operands
def probe_columns(K, step):
    ks = {0, K - 1}
    for k in range(step, K, step):
        ks |= {k - 1, k}
    return sorted(ks)


def _choice(vals, shape, g):
    v = torch.tensor(vals, dtype=torch.float32)
    return v[torch.randint(0, len(vals), shape, generator=g)]


@functools.lru_cache(maxsize=16)
def make_w(N, K, nz, step, seed):
    """[N, K] f32 in {-1, 0, 1}: exactly min(nz, K) non-zeros per row, every probe column
    non-zero in REP rows (spread over the rows, so gate and up halves both get some)."""
    g = torch.Generator().manual_seed(seed)
    nz = min(nz, K)
    cols = probe_columns(K, step)
    rep = max(1, min(3, (N * nz) // (2 * len(cols))))
    score = torch.rand(N, K, generator=g)
    per_row = [0] * N
    stride = 37 if N % 37 else 41
    for i, k in enumerate(cols):
        for j in range(rep):
            r = ((i * rep + j) * stride) % N
            score[r, k] = -1.0
            per_row[r] += 1
    assert max(per_row) <= nz, (N, K, nz, max(per_row))
    idx = score.topk(nz, dim=1, largest=False).indices
    w = torch.zeros(N, K)
    w.scatter_(1, idx, _choice((-1, 1), (N, nz), g))
    assert bool((w[:, cols] != 0).any(0).all())
    return w


@functools.lru_cache(maxsize=16)
def make_x(M, K, vals, seed):
    return _choice(vals, (M, K), torch.Generator().manual_seed(seed))


def operands(M, N, K, oset, step=64, seed=0, nz=None):
    """x [M, K] and w [N, K] of an operand set; nz: fewer non-zeros per w row, where a bias
    or a residual needs its share of the bound."""
    vals, nz0, _ = SETS[oset]
    nz = nz0 if nz is None else nz
    mmax = 4 if M <= 4 else 257 if M <= 257 else 2305
    assert M <= mmax
    x = make_x(mmax, K, vals, 1000 + seed)[:M]
    return x, make_w(N, K, nz, step, seed + K + 7 * N)


def ints(lo, hi, shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def norm_weights(n, seed):
    return _choice(NORM_W, (n,), torch.Generator().manual_seed(seed))


def quarter_turns(npos, D, seed=5):
    """cos_sin [npos, D] f32 with (cos, sin) in {(1,0), (0,1), (-1,0), (0,-1)} varying by
    position and by dimension."""
    q = torch.randint(0, 4, (npos, D // 2), generator=torch.Generator().manual_seed(seed))
    co = torch.tensor([1.0, 0.0, -1.0, 0.0])[q]
    si = torch.tensor([0.0, 1.0, 0.0, -1.0])[q]
    return torch.cat([co, si], 1).contiguous()


def sumsq_parts(M, K, npart, seed):
    """f32 [M, npart] partial sums of squares whose 1/rms spans 0.5 .. 2 over the rows."""
    r = torch.linspace(0.5, 2.0, M, dtype=torch.float64)
    r = r[torch.randperm(M, generator=torch.Generator().manual_seed(seed))]
    total = K * (1.0 / r ** 2 - EPS)
    frac = torch.rand(M, npart, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64) + 0.5
    return (total[:, None] * frac / frac.sum(1, keepdim=True)).float().contiguous()


def row_scale(parts, K):
    return torch.rsqrt(parts.double().sum(1) / K + EPS)


# ------------------------------------------------------------------------------ epilogues
def epi_plain(bias=None):
    def epi(s, rows):
        return {"out": (s if bias is None else s + bias.double(), EXACT)}
    return epi


def _rms(h, g):
    return h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS) * g.double()


def epi_res_norm(res, g):
    """residual += sums (exact); out = rmsnorm(residual) * g (rounds once)."""
    def epi(s, rows):
        h = res.double()[rows] + s
        return {"residual": (h, EXACT), "out": (_rms(h, g), ROUNDED)}
    return epi


def epi_cmb_res(res, g):
    """decode_gemm_res: residual += sums; y = residual * g; sumsq per 128-column tile."""
    def epi(s, rows):
        h = res.double()[rows] + s
        return {"residual": (h, EXACT), "y": (h * g.double(), EXACT),
                "sumsq": (h.pow(2).view(h.shape[0], -1, 128).sum(-1), EXACT)}
    return epi


def epi_silu(F, r=None, swap=False):
    def epi(s, rows):
        sc = 1.0 if r is None else r[rows][:, None]
        g, u = s[:, :F] * sc, s[:, F:] * sc
        if swap:
            g, u = u, g
        return {"out": (g * torch.sigmoid(g) * u, ROUNDED)}
    return epi


def epi_qkv(Hq, Hkv, D, cos_sin, pos, bias=None, r=None, scales=(1.0, 1.0), fault=None):
    """RoPE on q and k heads (pairs d, d + D/2), v heads pass; 'k' / 'v': the cache values
    of the row (the qkv values over the cache scale).  fault: 'pair' rotates d with the
    partner d + D/2 + 1, 'sign' flips the sine."""
    def epi(s, rows):
        y = s if bias is None else s + bias.double()
        if r is not None:
            y = y * r[rows][:, None]
        y = y.view(y.shape[0], Hq + 2 * Hkv, D)
        cs = cos_sin.double()[pos[rows].long()]
        co, si = cs[:, None, : D // 2], cs[:, None, D // 2:]
        if fault == "sign":
            si = -si
        a, b = y[:, : Hq + Hkv, : D // 2], y[:, : Hq + Hkv, D // 2:]
        if fault == "pair":
            b2 = b.roll(-1, -1)
            rot = torch.cat([a * co - b2 * si, b * co + a.roll(-1, -1) * si], -1)
        else:
            rot = torch.cat([a * co - b * si, b * co + a * si], -1)
        out = torch.cat([rot, y[:, Hq + Hkv:]], 1)
        kind = EXACT if r is None else ROUNDED
        return {"qkv": (out.reshape(out.shape[0], -1), kind),
                "k": (out[:, Hq: Hq + Hkv].reshape(out.shape[0], -1) / scales[0], kind),
                "v": (out[:, Hq + Hkv:].reshape(out.shape[0], -1) / scales[1], kind)}
    return epi


def epi_fused(bias=None, res=None, stats=False):
    def epi(s, rows):
        v = s
        if bias is not None:
            v = v + bias.double()
        if res is not None:
            v = v + res.double()[rows]
        o = {"out": (v, EXACT)}
        if stats:
            t = v.view(v.shape[0], -1, 64)
            o["stats"] = (torch.stack([t.sum(-1), t.pow(2).sum(-1)], -1), EXACT)
        return o
    return epi


# ------------------------------------------------------------------------------ cases
def split_ranges(K, S, unit):
    """K ranges of S splits of whole `unit`-deep stages: split s = stages [s nk / S, (s+1) nk / S)."""
    nk = K // unit
    return [((s * nk) // S * unit, ((s + 1) * nk) // S * unit) for s in range(S)]


def make_case(name, x, w, epi, oset, S=1, unit=64, step=64, extra_abs=0.0, xs=None, **kw):
    """xs: the x of each call of a stale-data case (x is xs[0])."""
    M, K = x.shape
    c = SimpleNamespace(name=name, x=x, w=w, M=M, K=K, N=w.shape[0], epi=epi, oset=oset, S=S, unit=unit,
                        ranges=split_ranges(K, S, unit), step=step, extra_abs=extra_abs, xs=xs, **kw)
    c.sums = sums(x, w)
    return c


def sums(x, w):
    return x.double() @ w.double().t()


def expect(c, x=None):
    """{name: (f64 reference, kind)} of the whole case (of call input x for stale cases)."""
    s = c.sums if x is None else sums(x, c.w)
    return c.epi(s, torch.arange(c.M))


def exact_in(t, dtype):
    return torch.equal(t.to(dtype).to(t.dtype), t)


def check_inputs(c):
    """The conditions on the inputs that make the reference exact (asserted for every case)."""
    bound = SETS[c.oset][2]
    for t in [c.w] + list(c.xs or [c.x]):
        assert exact_in(t, torch.bfloat16), c.name
    for x in (c.xs or [c.x]):
        assert bool((x != 0).all()), c.name
        worst = (x.abs().double() @ c.w.abs().double().t()).max().item() + c.extra_abs
        assert worst <= bound, (c.name, worst, bound)
    for v in getattr(c, "bf16_inputs", []):
        assert exact_in(v, torch.bfloat16), c.name
    if c.oset == NARROW and c.extra_abs == 0:
        assert bool((c.sums.abs() >= 1).all()), c.name   # odd sums: no gate / up is ever 0
    if getattr(c, "parts", None) is not None:
        r = row_scale(c.parts, c.K)
        assert 0.45 <= r.min().item() and r.max().item() <= 2.05 and r.max() / r.min() > 3, c.name
    if getattr(c, "fp8_scales", None) is not None:
        e = expect(c)
        assert e["qkv"][0].abs().max().item() <= 8, c.name
        for nm in ("k", "v"):     # the codes: value / scale
            assert exact_in(e[nm][0].float(), torch.float8_e4m3fn), (c.name, nm)
    for nm, (v, kind) in expect(c).items():
        if kind == EXACT:
            lim = 2 ** 24 if nm in ("sumsq", "stats") or getattr(c, "f32_out", False) else 256
            assert v.abs().max().item() <= lim, (c.name, nm)
            if lim == 256:
                assert exact_in(v.float(), torch.bfloat16), (c.name, nm)


# ------------------------------------------------------------------------------ comparator
def excess(got, ref):
    """Largest error of a rounded output in units of 2^-8 |ref| (+ the floor)."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return ((got - ref).abs() / (2.0 ** -8 * ref.abs() + FLOOR / 2)).max().item()


def rejected(kind, got, ref, rtol=RTOL):
    """True when the comparator of the GPU test refuses `got`: torch.equal for exact
    outputs, |got - ref| <= rtol |ref| + 1e-6 elementwise otherwise (NaN never passes)."""
    got, ref = got.double(), ref.double()
    if kind == EXACT:
        return not torch.equal(got, ref)
    return not bool(((got - ref).abs() <= rtol * ref.abs() + FLOOR).all())


def as_stored(v, name, c):
    """What a kernel that computed v would leave in memory (the output's number format)."""
    if name in ("sumsq", "stats") or getattr(c, "f32_out", False):
        return v.float().double()
    return v.to(torch.bfloat16).double()


# ------------------------------------------------------------------------------ mutants
def _rows(c):
    return sorted({0, c.M - 1})


def sum_mutants(c, x=None):
    """(label, rows, wrong sums [len(rows), N], per_row): the sums a faulty kernel would
    have accumulated.  per_row: each row is a mutant of its own (one x element)."""
    x = c.x if x is None else x
    w, K = c.w, c.K
    xd, wd = x.double(), w.double()
    ks = probe_columns(K, c.step)
    for b in {kb for kb, _ in c.ranges if kb > 0}:
        assert b in ks and b - 1 in ks, (c.name, b)       # every split boundary is probed
    kt = torch.tensor(ks)
    for m in _rows(c):
        rows = torch.full((len(ks),), m)
        yield f"x[{m},k]=0", rows, c.sums[m][None, :] - xd[m, kt][:, None] * wd[:, kt].t(), True
    rows = torch.arange(c.M)
    for k in [0, K - 1] + ([c.step] if c.step < K else []):
        # one row of w: the first row the fault shows in (a row whose chunk is all zeros, or
        # whose products cancel for every x row, would hide it)
        ch = k // 8 * 8
        nx = ch + 8 if ch + 16 <= K else ch - 8
        d = xd[:, ch: ch + 8] @ wd[:, ch: ch + 8].t()                 # [M, N]
        n = int((d != 0).any(0).nonzero()[0])
        s = c.sums.clone()
        s[:, n] -= d[:, n]
        yield f"w[{n}] chunk {ch // 8} zeroed", rows, s, False
        if nx >= 0:
            e = xd[:, ch: ch + 8] @ wd[:, nx: nx + 8].t() - d
            n = int((e != 0).any(0).nonzero()[0])
            s = c.sums.clone()
            s[:, n] += e[:, n]
            yield f"w[{n}] chunk {ch // 8} read from {nx // 8}", rows, s, False
    if K >= 16:
        # two adjacent chunks of x swapped under an unswapped w: at the first chunk pairs
        # next to a probe column where it changes a sum (sparse w rows leave most pairs idle)
        found = 0
        for ch in sorted({min(k // 8 * 8, K - 16) for k in ks}):
            xs = xd.clone()
            xs[:, ch: ch + 8], xs[:, ch + 8: ch + 16] = xd[:, ch + 8: ch + 16], xd[:, ch: ch + 8]
            s = xs @ wd.t()
            if not torch.equal(s, c.sums):
                yield f"x chunks {ch // 8},{ch // 8 + 1} swapped", rows, s, False
                found += 1
                if found == 3:
                    break
        assert found, (c.name, "no chunk swap changes a sum")
    u = c.unit          # the depth of one K stage of the kernel (gemv: a wave's 512-element chunk)
    for t in sorted({0, (K // u) // 2, K // u - 1}):
        d = xd[:, u * t: u * t + u] @ wd[:, u * t: u * t + u].t()
        yield f"stage {t} twice", rows, c.sums + d, False
        yield f"stage {t} skipped", rows, c.sums - d, False
    for s_, (kb, ke) in enumerate(c.ranges):
        yield f"split {s_} dropped", rows, c.sums - xd[:, kb:ke] @ wd[:, kb:ke].t(), False


def out_mutants(c, ref):
    """(label, {name: wrong f64 output}): faults of the store side."""
    M = c.M
    if M >= 2:
        for m in sorted({0, (M - 1) & ~1}):
            if (m ^ 1) < M:
                idx = torch.arange(M)
                idx[m], idx[m ^ 1] = m ^ 1, m
                yield f"rows {m},{m ^ 1} exchanged", {k: v[idx] for k, (v, _) in ref.items()}
    o = {k: v.clone() for k, (v, _) in ref.items()}
    main = "qkv" if "qkv" in o else "out" if "out" in o else "residual"
    n = o[main].shape[1]
    if n > 16:
        idx = torch.arange(n) ^ 16
        idx = torch.where(idx < n, idx, torch.arange(n))
        yield "columns n, n^16 exchanged", {**o, main: o[main][:, idx]}
    last = {k: v.clone() for k, v in o.items()}
    last[main][M - 1] = float("nan")     # the GPU test pre-fills the outputs with NaN
    yield "row M-1 unwritten", last


def stale_mutants(c):
    """Call i (i >= 1) computed from call i-1's x on one split."""
    wd = c.w.double()
    for i in range(1, len(c.xs)):
        cur, prev = c.xs[i].double(), c.xs[i - 1].double()
        s = sums(c.xs[i], c.w)
        for s_, (kb, ke) in enumerate(c.ranges):
            yield i, f"call {i} split {s_} from call {i - 1}", s + (prev[:, kb:ke] - cur[:, kb:ke]) @ wd[:, kb:ke].t()


def _any_rejected(c, got, ref, rows=None):
    for nm, (r, kind) in ref.items():
        r = r if rows is None else r[rows]
        if rejected(kind, as_stored(got[nm], nm, c), r):
            return True
    return False


def check_mutants(c):
    """Asserts that the comparator refuses every mutant of the case; returns how many."""
    ref = expect(c)
    n = 0
    for label, rows, s, per_row in sum_mutants(c):
        got = {k: v for k, (v, _) in c.epi(s, rows).items()}
        if per_row:
            for i in range(len(rows)):
                ok = any(rejected(kind, as_stored(got[nm][i: i + 1], nm, c), r[rows[i: i + 1]])
                         for nm, (r, kind) in ref.items())
                assert ok, (c.name, label, i)
                n += 1
            if c.oset in (NARROW, FP8) and any(kind == ROUNDED for _, kind in ref.values()):
                # a unit error in one sum is >= 8x the allowance (or breaks an exact output)
                for i in range(len(rows)):
                    big = any(excess(got[nm][i: i + 1], r[rows[i: i + 1]]) >= 16 if kind == ROUNDED
                              else rejected(kind, as_stored(got[nm][i: i + 1], nm, c), r[rows[i: i + 1]])
                              for nm, (r, kind) in ref.items())
                    assert big, (c.name, label, i, "unit error under 8x the allowance")
        else:
            assert _any_rejected(c, got, ref, rows), (c.name, label)
            n += 1
    for label, got in out_mutants(c, ref):
        assert _any_rejected(c, got, ref), (c.name, label)
        n += 1
    if getattr(c, "silu_F", None):
        got = {k: v for k, (v, _) in epi_silu(c.silu_F, getattr(c, "r", None), swap=True)(c.sums, torch.arange(c.M)).items()}
        assert _any_rejected(c, got, ref), (c.name, "gate / up exchanged")
        n += 1
    if getattr(c, "rope", None):
        for fault in ("pair", "sign"):
            got = {k: v for k, (v, _) in epi_qkv(**c.rope, fault=fault)(c.sums, torch.arange(c.M)).items()}
            assert _any_rejected(c, got, ref), (c.name, "rope " + fault)
            n += 1
    if c.xs is not None:
        for i, label, s in stale_mutants(c):
            refi = expect(c, c.xs[i])
            got = {k: v for k, (v, _) in c.epi(s, torch.arange(c.M)).items()}
            assert _any_rejected(c, got, refi), (c.name, label)
            n += 1
    return n


# ------------------------------------------------------------------------------ shapes
DG_K = [64, 128, 192, 320, 576, 1088]          # 1, 2, 3, 5, 9, 17 stages of 64
DG_M = [1, 63, 64, 65, 127, 128, 129, 255, 256]
DG_N = [128, 256, 384]
DG_FORCE = [(0, 0), (64, 1), (128, 1), (256, 1), (128, 2), (64, 3), (256, 2), (128, -1)]   # -1: K / 64 splits
CMB_M = [129, 255, 256]
PF_M = [1, 255, 256, 257, 513, 2305]
PF_N = [256, 768]
PF_K = [128, 256, 384, 1056]
SK_M = [1, 63, 64, 65, 128, 129, 257]
SK_NK = [(128, 64), (128, 320), (256, 1024), (128, 2048)]
GV_T = [1, 2, 3, 4]
GV_K = [512, 2048, 2560, 4608, 14336]
FU_M = [1, 255, 257]
FU_NK = [(128, 32), (128, 96), (384, 384)]
CUS = 256                                       # MI355X compute units (decode_gemm_cmb_splits)


def dg_pick_split(tiles, K, min_steps=4):
    """gemm_decode.hip pick_split."""
    best = 1
    for s in range(1, 65):
        if tiles * s > 264 or (K // 64) // s < min_steps:
            break
        best = s
    return best


def dg_route(M, N, K, bn, splits, norm=False):
    """(bn, S) decode_gemm runs for the forced (bn, splits), 0 = automatic."""
    b = bn if bn in (64, 128, 256) and N % bn == 0 else 128
    if bn == 0 and norm and K <= 4096 and M > 128:
        b = 64
    S = min(splits, K // 64) if splits > 0 else dg_pick_split(N // b, K)
    return b, S


def dg_bm(M, bn, epi):
    if bn == 128 and epi in ("store", "partial", "silu"):
        return 64 if M <= 64 else 128 if M <= 128 else 256
    return 256


def dg_key(M, bn, epi, S):
    return f"bn{bn}_{epi}_bm{dg_bm(M, bn, epi)}_s{min(S, 16)}"


def cmb_splits(N, K, cus=CUS):
    """gemm_decode.hip decode_gemm_cmb_splits."""
    tiles, best = N // 128, 0
    for s in range(1, 17):
        if tiles * s > cus or (K // 64) // s < 4:
            break
        best = s
    return best


def skinny_splits(M, N, K):
    """gemm_skinny.hip pick_bm / pick_splitk."""
    bm = 64 if M <= 64 else 128 if M <= 128 else 256
    tiles, target, s = -(-M // bm) * (N // 128), 256 if bm == 256 else 512, 1
    while tiles * s < target and (K // 64) % (2 * s) == 0 and K // (2 * s) >= 512:
        s *= 2
    return s


def prefill_splits(M, N, K, variant):
    """gemm_prefill.hip: split-K of the ping-pong kernel."""
    tiles = -(-M // 256) * (N // 256)
    if variant == 1 and K % 128 == 0 and K >= 4096 and tiles < 200:
        return max(1, min(4, 256 // tiles, (K // 128) // 8))
    return 1


# ---- builders: one Case per (spec, M); the operands of a (N, K) are shared through the caches
def plain_case(M, N, K, S=1, unit=64, oset=WIDE, name="", f32=False, step=64, seed=0):
    x, w = operands(M, N, K, oset, step, seed)
    return make_case(f"{name} M{M} N{N} K{K} S{S}", x, w, epi_plain(), oset, S, unit, step, f32_out=f32)


def res_norm_case(M, N, K, S=1, unit=64, oset=WIDE, name="", step=64):
    """residual + RMSNorm forms.  WIDE checks the exact residual stream at full density,
    NARROW (|residual + sum| <= 16) gives the normed output teeth."""
    lim = 64 if oset == WIDE else 1
    x, w = operands(M, N, K, oset, step, nz=96 if oset == WIDE else None)
    res = ints(-lim, lim, (M, N), 11 + M)
    g = norm_weights(N, 13)
    return make_case(f"{name} M{M} N{N} K{K} S{S}", x, w, epi_res_norm(res, g), oset, S, unit, step,
                     extra_abs=float(lim), res=res, g=g, bf16_inputs=[res, g])


def silu_case(M, F, K, S=1, unit=64, name="", parts=None, step=64):
    x, w = operands(M, 2 * F, K, NARROW, step)
    r = None if parts is None else row_scale(parts, K)
    return make_case(f"{name} M{M} F{F} K{K} S{S}", x, w, epi_silu(F, r), NARROW, S, unit, step, silu_F=F, r=r,
                     parts=parts)


def qkv_case(M, K, S=1, name="", bias=False, fp8=None, parts=None, Hq=2, Hkv=1, D=128, step=64, oset=None, x=None,
             **kw):
    N = (Hq + 2 * Hkv) * D
    oset = oset or (FP8 if fp8 else NARROW if parts is not None else WIDE)
    lim = 1 if oset != WIDE else 32
    x0, w = operands(M, N, K, oset, step, nz=(112 if oset == WIDE else SETS[oset][1] - 1) if bias else None)
    x = x0 if x is None else x
    b = None
    extra = 0.0
    if bias:
        b = ints(-lim, lim, (N,), 17)
        extra = float(lim)
    npos = 16
    pos = torch.randint(0, npos, (M,), generator=torch.Generator().manual_seed(19), dtype=torch.int32)
    cs = quarter_turns(npos, D)
    NB = 2 * M // BS + 3
    slots = torch.randperm(NB * BS, generator=torch.Generator().manual_seed(23))[:M].long()
    if M > 1:
        slots[M // 2] = -1
    if M > 2:
        slots[M - 1] = -1
    r = None if parts is None else row_scale(parts, K)
    rope = dict(Hq=Hq, Hkv=Hkv, D=D, cos_sin=cs, pos=pos, bias=b, r=r, scales=fp8 or (1.0, 1.0))
    return make_case(f"{name} M{M} K{K} S{S} bias{int(bias)} fp8{fp8}", x, w, epi_qkv(**rope), oset, S, 64, step,
                     extra_abs=extra, rope=rope, bias=b, pos=pos, cos_sin=cs, slots=slots, NB=NB, Hq=Hq, Hkv=Hkv, D=D,
                     fp8_scales=fp8, parts=parts, bf16_inputs=([b] if bias else []) + kw.pop("bf16_inputs", []), **kw)


def cmb_res_case(M, N, K, xs=None):
    S = cmb_splits(N, K)
    x, w = operands(M, N, K, WIDE, nz=96)       # |sum| <= 192, |residual| <= 64
    res = ints(-64, 64, (M, N), 29 + M)
    g = norm_weights(N, 31)
    return make_case(f"cmb_res M{M} N{N} K{K} S{S}", x, w, epi_cmb_res(res, g), WIDE, S, extra_abs=64.0, res=res, g=g,
                     bf16_inputs=[res, g], xs=xs)


def fused_case(M, N, K, mode):
    bias = res = None
    extra = 0.0
    if mode != "plain":
        bias = ints(-16, 16, (N,), 37)
        extra += 16
    if mode == "res_stats":
        res = ints(-48, 48, (M, N), 41)
        extra += 48
    x, w = operands(M, N, K, WIDE, step=32, nz=int(256 - extra) // 2)
    return make_case(f"fused {mode} M{M} N{N} K{K}", x, w, epi_fused(bias, res, mode == "res_stats"), WIDE, 1, 32, 32,
                     extra_abs=extra, bias=bias, res=res, bf16_inputs=[t for t in (bias, res) if t is not None])


def gemv_case(T, N, K, kind, seed=0):
    """kind: plain | silu | addnorm | norm | silu_norm | qkv | qkv_pro.  The K step of the
    GEMV is the 512-element chunk a wave owns (there are no 64-deep stages)."""
    pro = kind in ("norm", "silu_norm", "qkv_pro")
    oset = HALF if pro and kind != "silu_norm" else NARROW if kind in ("silu", "silu_norm", "addnorm") else WIDE
    vals, nz, _ = SETS[oset]
    w = make_w(N, K, nz, 512, seed + K + 7 * N)
    kw = {}
    if pro:
        # o + res = +-c_t (c_t = 0.5, 1, 2, 4 by row): rmsnorm(o + res) = +-(1 - O(eps)), which
        # rounds to +-1 in bf16, so the GEMV input is exactly +-norm_w whatever the row scale
        g = torch.Generator().manual_seed(43 + seed)
        sign = _choice((-1, 1), (T, K), g)
        c = torch.tensor([0.5, 1.0, 2.0, 4.0])[:T, None]
        h = sign * c
        o = ints(-3, 3, (T, K), 47 + seed)
        nw = norm_weights(K, 53) if kind != "silu_norm" else torch.ones(K)
        x = sign * nw
        kw = dict(o=o, res=h - o, h=h, nw=nw, bf16_inputs=[o, h - o, nw])
    else:
        x = make_x(4, K, vals, 2000 + seed)[:T]
    name = f"gemv_{kind} T{T} N{N} K{K}"
    if kind in ("qkv", "qkv_pro"):
        assert N == 512
        return qkv_case(T, K, name=name, step=512, oset=oset, x=x, **kw)
    if kind in ("silu", "silu_norm"):
        return make_case(name, x, w, epi_silu(N // 2), oset, 1, 512, 512, silu_F=N // 2, **kw)
    if kind == "addnorm":
        res = ints(-1, 1, (T, N), 59)
        g = norm_weights(N, 61)
        return make_case(name, x, w, epi_res_norm(res, g), oset, 1, 512, 512, extra_abs=1.0, res=res, g=g,
                         bf16_inputs=[res, g], **kw)
    return make_case(name, x, w, epi_plain(), oset, 1, 512, 512, **kw)


# ------------------------------------------------------------------------------ families
# SPECS[family]: the parametrisation both test files share; cases(family, spec) yields the
# Cases of one spec (one per M / T, which the tests loop over).
def stale_xs(M, K, vals, n=3):
    """The x of the calls of a stale-data check: a draw, a fresh draw, its negation."""
    a = make_x(257 if M > 4 else 4, K, vals, 3000)[:M]
    b = make_x(257 if M > 4 else 4, K, vals, 3001)[:M]
    return [a, b, -b][:n]


def _with_xs(c, vals):
    c.xs = stale_xs(c.M, c.K, vals)
    c.x, c.sums = c.xs[0], sums(c.xs[0], c.w)
    return c


SPECS = {
    "decode": [(K, N, bn, sp) for K in DG_K for N in DG_N for bn, sp in DG_FORCE if bn != 256 or N % 256 == 0],
    "decode_norm": [(K, N, bn, sp, o) for K in DG_K for N in (128, 384)
                    for bn, sp, o in [(0, 0, WIDE), (64, 3, WIDE), (128, 2, WIDE), (0, 0, NARROW)]],
    "decode_f32": [(K, bn) for K in DG_K for bn in (128, 256)],
    "decode_qkv": [(K, bias, fp8) for K in DG_K
                   for bias, fp8 in [(False, None), (True, None), (False, (1.0, 1.0)), (True, (2.0, 0.5))]],
    "decode_silu": [(K, F, sp) for K in DG_K for F in (128, 384) for sp in (1, 2)],
    "cmb_res": [(128, 512), (256, 576), (128, 1088)],
    "cmb_qkv": [(512, 4), (576, 5)],                 # (K, npart): float4 and scalar partial loads
    "silu_r": [(128, 512, 4), (384, 320, 5)],        # (F, K, npart)
    "prefill": [(v, N, K) for v in (0, 1, 2) for N in PF_N for K in PF_K],
    "prefill_f32": [(N, K) for N in PF_N for K in PF_K if K % 128 == 0],
    "prefill_big": [(2, 2304, 8192, 128)],
    "prefill_splitk": [(1, 256, 4096), (255, 256, 4224), (257, 256, 4096)],
    "prefill_silu": [(v, F, K) for v in (0, 1, 2) for F in (128, 384) for K in (128, 384, 1056)],
    "skinny": [(kind, N, K) for kind in ("plain", "silu", "addnorm") for N, K in SK_NK],
    "gemv": [(kind, N, K) for kind in ("plain", "silu", "addnorm", "norm", "silu_norm") for K in GV_K
             for N in (8, 264)] + [(kind, 512, K) for kind in ("qkv", "qkv_pro") for K in GV_K],
    "fused": [(mode, N, K) for mode in ("plain", "bias", "res_stats") for N, K in FU_NK],
}
STALE = {"cmb_res", "cmb_qkv"}      # families whose every case is a three-call stale-data check


def cases(family, spec):
    if family == "decode":
        K, N, bn, sp = spec
        for M in DG_M:
            b, S = dg_route(M, N, K, bn, sp if sp >= 0 else K // 64)
            c = plain_case(M, N, K, S, name="decode")
            c.key = dg_key(M, b, "store" if S == 1 else "partial", S)
            yield c
    elif family == "decode_norm":
        K, N, bn, sp, o = spec
        for M in DG_M:
            b, S = dg_route(M, N, K, bn, sp, norm=True)
            c = res_norm_case(M, N, K, S, oset=o, name="decode_norm " + o)
            c.key = dg_key(M, b, "partial", S)
            yield c
    elif family == "decode_f32":
        K, bn = spec
        for M in DG_M:
            c = plain_case(M, bn, K, name="decode_f32", f32=True)
            c.key = dg_key(M, bn, "partial", 1)
            yield c
    elif family == "decode_qkv":
        K, bias, fp8 = spec
        S = min(4, dg_pick_split(4, K))
        for M in DG_M:
            c = qkv_case(M, K, S, name="decode_qkv", bias=bias, fp8=fp8)
            c.key = dg_key(M, 128, "partial" if S > 1 else "store", S)
            yield c
    elif family == "decode_silu":
        K, F, sp = spec
        two = sp == 2 and K // 64 >= 8       # a 2-way split of fewer than 8 stages runs the single launch
        for M in DG_M:
            c = silu_case(M, F, K, 2 if two else 1, name="decode_silu")
            if two:
                _with_xs(c, SETS[NARROW][0])
            c.key = dg_key(M, 256, "silu2", 2) if two else dg_key(M, 128, "silu", 1)
            yield c
    elif family == "cmb_res":
        N, K = spec
        for M in CMB_M:
            yield cmb_res_case(M, N, K, xs=stale_xs(M, K, SETS[WIDE][0]))
    elif family == "cmb_qkv":
        K, npart = spec
        for M in CMB_M:
            c = qkv_case(M, K, cmb_splits(512, K), name="cmb_qkv", parts=sumsq_parts(M, K, npart, 67))
            yield _with_xs(c, SETS[NARROW][0])
    elif family == "silu_r":
        F, K, npart = spec
        for M in CMB_M:
            yield silu_case(M, F, K, name="silu_r", parts=sumsq_parts(M, K, npart, 71))
    elif family in ("prefill", "prefill_f32", "prefill_big", "prefill_splitk"):
        if family == "prefill":
            v, N, K = spec
            ms = PF_M
        elif family == "prefill_f32":
            (N, K), v, ms = spec, 1, PF_M
        elif family == "prefill_big":
            v, M, N, K = spec
            ms = [M]
        else:
            (M, N, K), v, ms = spec, 1, None
            ms = [M]
        pp = v != 0 and K % 128 == 0         # the ping-pong kernels walk 128-deep tile pairs
        for M in ms:
            S = prefill_splits(M, N, K, v) if family != "prefill_f32" else 1
            yield plain_case(M, N, K, S, unit=128 if pp else 32, name=f"{family} v{v}", f32=family == "prefill_f32",
                             step=32)
    elif family == "prefill_silu":
        v, F, K = spec
        for M in PF_M:
            yield silu_case(M, F, K, unit=128 if v != 0 and K % 128 == 0 else 32, name=f"prefill_silu v{v}", step=32)
    elif family == "skinny":
        kind, N, K = spec
        for M in SK_M:
            if kind == "silu":
                yield silu_case(M, N, K, name="skinny_silu")
            elif kind == "addnorm":
                for o in (WIDE, NARROW):
                    yield res_norm_case(M, N, K, skinny_splits(M, N, K), oset=o, name="skinny_addnorm " + o)
            else:
                yield plain_case(M, N, K, skinny_splits(M, N, K), name="skinny")
    elif family == "gemv":
        kind, N, K = spec
        for T in GV_T:
            c = gemv_case(T, N, K, kind)
            yield _with_xs(c, SETS[NARROW][0]) if kind == "addnorm" else c
    elif family == "fused":
        mode, N, K = spec
        for M in FU_M:
            yield fused_case(M, N, K, mode)
    else:
        raise KeyError(family)
