"""The GEMM kernels on integer operands (gemm_probe.py): every sum of every subset of the K
products is a small integer, so f32 accumulation is exact in any order and under any K
split, and the outputs that do not round -- plain, bias, f32, the in-place residual stream,
y / sumsq of decode_gemm_res, the LayerNorm statistics of gemm_fused, quarter-turn RoPE rows
and the paged K / V caches, bf16 and fp8 -- must EQUAL the int64 reference (torch.equal).
One dropped or doubled 16-byte chunk, a ring slot read a step early or a stage on the wrong
side of a split boundary changes an integer.  Outputs that round once (SwiGLU, RMSNorm, the
1/rms row scale) are held to |got - ref| <= 2^-7 |ref| + 1e-6 against a float64 epilogue of
the exact sums; test_gemm_probe_cpu.py proves that both comparators refuse every mutant.

Every call also runs on views: x as a window of a NaN buffer (row stride K + 24, 8 columns
in: 16-byte but not 128-byte aligned), out as a column window of a wider sentinel buffer
where the entry point takes a row stride, 8 sentinel rows after every output and in-place
residual (the M-tail stores of the 64-, 128- and 256-row tiles), NaN in every split-K and
exchange workspace the caller owns.  The in-launch combines (tickets, counters) run three
calls on one workspace with a fresh x and then its negation, each against its own reference.

Shapes: K below, at and across every ring depth (1, 2, 3, 5, 9, 17 stages of 64), M on both
sides of the 64 / 128 / 256 tile heights, one stage per split, uneven stages per split.

Largest observed error of the rounded outputs on an MI355X, in units of 2^-8 |ref| (the
allowance is 2 units):

    decode_gemm residual + norm  0.996      decode_gemm_qkv_cmb      0.996
    decode_gemm_silu, 1 split    0.990      decode_gemm_silu, 2 way  0.990
    decode_gemm_silu_r           0.987      rows_rms_scale           0.996
    gemm_prefill silu, v0 / 1 / 2  0.990    skinny_gemm_silu         0.990
    skinny_gemm_add_rmsnorm      0.996      gemv_add_rmsnorm         0.971
    gemv_silu                    0.765      gemv_silu_norm           0.800

i.e. one bf16 rounding and nothing else that shows; no entry point needs more than 2^-7.

Not reached from here: the split-K workspaces of skinny_gemm, skinny_gemm_add_rmsnorm and
gemm_prefill are allocated inside the entry points, so they cannot be pre-filled with NaN;
decode_gemm_ablate produces no result to compare; the
Qwen3 q_norm / k_norm form stays with test_qk_norm_gpu.py.
"""
import pytest
import torch

import gemm_probe as gp
from langstream_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
RTOL = {}            # entry point -> allowance where a kernel that is right by reading needs more than 2^-7
WORST = {}           # entry point -> largest observed error of a rounded output, units of 2^-8 |ref|


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nrounded outputs, largest error in units of 2^-8 |ref|:",
          {k: round(v, 3) for k, v in sorted(WORST.items())})


def H():
    return ops.hip()


def bf(t):
    return t.to(BF).to(DEV)


def w_dev(c, prev):
    """The case's w on the GPU; the cases of one spec mostly share one w, uploaded once."""
    if prev is not None and prev[0] is c.w:
        return prev
    return (c.w, bf(c.w))


def x_layouts(x):
    """The operand contiguous, and as a window of a NaN buffer: row stride K + 24, starting 8
    columns in."""
    M, K = x.shape
    buf = torch.full((M, K + 24), NAN, dtype=BF, device=DEV)
    v = buf[:, 8: 8 + K]
    v.copy_(x)
    return [bf(x), v]


class Out:
    """An output of [M, N] pre-filled with NaN inside a sentinel buffer: 8 guard rows after
    it and, with window, 8 guard columns on each side (a row stride of N + 16)."""

    def __init__(self, M, N, window=False, dtype=BF, fill=None):
        self.c0 = 8 if window else 0
        self.buf = torch.full((M + 8, N + 2 * self.c0), gp.SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[:M, self.c0: self.c0 + N]
        if fill is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(fill)

    def guards_intact(self, what):
        g = self.buf.clone()
        g[: self.t.shape[0], self.c0: self.c0 + self.t.shape[1]] = gp.SENTINEL
        assert bool((g == gp.SENTINEL).all()), f"{what}: a store outside the output"


def nan_ws(n):
    return torch.full((max(int(n), 1),), NAN, dtype=F32, device=DEV)


def compare(c, entry, got, x=None, rows=None):
    """got {name: GPU tensor} against the case's reference (of call input x)."""
    ref = gp.expect(c, x)
    for nm, g in got.items():
        r, kind = ref[nm]
        g = g.float().double().cpu().flatten(1)
        r = r.flatten(1)
        if rows is not None:
            r = r[rows]
        if kind == gp.EXACT:
            if not torch.equal(g, r):
                bad = (g != r).nonzero()
                raise AssertionError(f"{c.name} {entry} {nm}: {len(bad)} of {g.numel()} differ, first at "
                                     f"{bad[:4].tolist()}: got {g[tuple(bad[0])].item()} ref {r[tuple(bad[0])].item()}")
        else:
            e = gp.excess(g, r)
            WORST[entry] = max(WORST.get(entry, 0.0), e)
            assert not gp.rejected(kind, g, r, RTOL.get(entry, gp.RTOL)), f"{c.name} {entry} {nm}: {e:.3f} x 2^-8 |ref|"


def census_is(key):
    got = dict(H().decode_gemm_launch_counts(True))
    assert got == {key: 1}, (got, key)


# ------------------------------------------------------------------------------ paged caches
class Caches:
    """K / V caches holding a fill value (bf16 77, fp8 the code of 1.5), the slot rows read
    back as [rows, Hkv * D] and the check that every other slot kept its fill."""

    def __init__(self, c, fp8=False):
        self.c, self.fp8 = c, fp8
        dt = torch.float8_e4m3fn if fp8 else BF
        self.fill = 1.5 if fp8 else gp.SENTINEL
        mk = lambda *s: torch.full(s, self.fill, dtype=torch.float32).to(dt).to(DEV)   # noqa: E731
        self.kc = mk(c.NB, c.Hkv, gp.BS, c.D)
        self.vc = mk(c.NB, c.Hkv, gp.BS // 8, c.D, 8)
        self.valid = (c.slots >= 0).nonzero()[:, 0]

    def slot_rows(self):
        c = self.c
        k = self.kc.float().permute(0, 2, 1, 3).reshape(c.NB * gp.BS, c.Hkv * c.D)
        v = self.vc.float().permute(0, 2, 4, 1, 3).reshape(c.NB * gp.BS, c.Hkv * c.D)
        return k, v

    def rows_and_rest(self):
        k, v = self.slot_rows()
        sl = self.c.slots[self.valid].to(DEV)
        keep = torch.ones(k.shape[0], dtype=torch.bool, device=DEV)
        keep[sl] = False
        assert bool((k[keep] == self.fill).all()) and bool((v[keep] == self.fill).all()), "a cache slot lost its fill"
        return k[sl], v[sl]


def qkv_args(c):
    return c.pos.to(DEV), c.cos_sin.to(DEV), c.slots.to(DEV)


# ------------------------------------------------------------------------------ gemm_decode.hip
@pytest.mark.parametrize("spec", gp.SPECS["decode"], ids=str)
def test_decode_gemm(spec):
    K, N, bn, sp = spec
    wc = None
    for c in gp.cases("decode", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        assert H().decode_gemm_supported(w, False)
        if (bn, sp) == (0, 0):
            assert H().decode_gemm_workspace(c.M, N, K, False) == (4 * c.S * c.M * N if c.S > 1 else 0)
        for lay, x in enumerate(x_layouts(c.x)):
            out = Out(c.M, N, window=bool(lay))
            H().decode_gemm_launch_counts(True)
            H().decode_gemm(out.t, x, w, nan_ws(c.S * c.M * N), None, None, gp.EPS, bn, sp if sp >= 0 else K // 64)
            census_is(c.key)
            compare(c, "decode_gemm", {"out": out.t})
            out.guards_intact(c.name)


@pytest.mark.parametrize("spec", gp.SPECS["decode_norm"], ids=str)
def test_decode_gemm_residual_norm(spec):
    K, N, bn, sp, _ = spec
    wc = None
    for c in gp.cases("decode_norm", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        for x in x_layouts(c.x):
            out, res = Out(c.M, N), Out(c.M, N, fill=c.res)
            H().decode_gemm_launch_counts(True)
            H().decode_gemm(out.t, x, w, nan_ws(c.S * c.M * N), res.t, bf(c.g), gp.EPS, bn, sp)
            census_is(c.key)
            compare(c, "decode_gemm+norm", {"residual": res.t, "out": out.t})
            out.guards_intact(c.name)
            res.guards_intact(c.name + " residual")


@pytest.mark.parametrize("spec", gp.SPECS["decode_f32"], ids=str)
def test_decode_gemm_f32(spec):
    K, bn = spec
    wc = None
    for c in gp.cases("decode_f32", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        assert H().decode_gemm_f32_supported(w, c.M)
        for x in x_layouts(c.x):
            out = Out(c.M, c.N, dtype=F32)
            H().decode_gemm_launch_counts(True)
            H().decode_gemm_f32(out.t, x, w, bn)
            census_is(c.key)
            compare(c, "decode_gemm_f32", {"out": out.t})
            out.guards_intact(c.name)


@pytest.mark.parametrize("spec", gp.SPECS["decode_qkv"], ids=str)
def test_decode_gemm_qkv_rope(spec):
    K, bias, fp8 = spec
    wc = None
    for c in gp.cases("decode_qkv", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        for x in x_layouts(c.x):
            out, kv = Out(c.M, c.N), Caches(c, fp8 is not None)
            H().decode_gemm_launch_counts(True)
            H().decode_gemm_qkv_rope(out.t, x, w, nan_ws(4 * c.M * c.N), *qkv_args(c), kv.kc, kv.vc, c.Hq, c.Hkv,
                                     *(fp8 or (1.0, 1.0)), bf(c.bias) if bias else None)
            census_is(c.key)
            compare(c, "decode_gemm_qkv_rope", {"qkv": out.t})
            k, v = kv.rows_and_rest()
            compare(c, "decode_gemm_qkv_rope", {"k": k, "v": v}, rows=kv.valid)
            out.guards_intact(c.name)


def test_decode_gemm_qkv_rope_rejects_a_strided_qkv():
    """With one K split the entry point goes through rope_and_cache, which takes no row
    stride, and its one caller allocates qkv itself: a column window is refused up front."""
    c = gp.qkv_case(5, 64)
    out, kv = Out(c.M, c.N, window=True), Caches(c)
    with pytest.raises(RuntimeError, match="contiguous"):
        H().decode_gemm_qkv_rope(out.t, bf(c.x), bf(c.w), nan_ws(1), *qkv_args(c), kv.kc, kv.vc, c.Hq, c.Hkv)
    assert bool(out.t.isnan().all()), "refused before anything ran"


@pytest.mark.parametrize("spec", gp.SPECS["decode_silu"], ids=str)
def test_decode_gemm_silu(spec):
    """splits = 2 below 8 stages runs the single launch (the census says so); with the
    exchange: three calls on one workspace and ticket array, a fresh x and its negation."""
    K, F, sp = spec
    wc = None
    tiles = F // 128
    for c in gp.cases("decode_silu", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        assert H().decode_gemm_supported(w, True)
        tickets = torch.zeros(2 * tiles, dtype=torch.int32, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = nan_ws(tiles * 256 * 256)
        assert H().decode_gemm_workspace(c.M, 2 * F, K, True) == 4 * ws.numel()
        calls = 0
        for lay in range(2):
            for xc in (c.xs or [c.x]):
                x = x_layouts(xc)[lay]
                out = Out(c.M, F, window=bool(lay))
                H().decode_gemm_launch_counts(True)
                H().decode_gemm_silu(out.t, x, w, ws, tickets, err, sp)
                census_is(c.key)
                compare(c, f"decode_gemm_silu s{c.S}", {"out": out.t}, x=xc)
                out.guards_intact(c.name)
                calls += 1
        assert int(err.item()) == 0
        want = [2 * calls, calls] * tiles if c.S == 2 else [0, 0] * tiles    # arrivals, generation per tile
        assert tickets.tolist() == want, (tickets.tolist(), want)


@pytest.mark.parametrize("spec", gp.SPECS["cmb_res"], ids=str)
def test_decode_gemm_res_combine(spec):
    N, K = spec
    S = H().decode_gemm_cmb_splits(N, K)
    wc = None
    for c in gp.cases("cmb_res", spec):
        assert S == c.S > 1
        wc = w_dev(c, wc)
        w = wc[1]
        cnt = torch.zeros(N // 128, dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = nan_ws(S * c.M * N)
        calls = 0
        for lay in range(2):
            for xc in c.xs:
                x = x_layouts(xc)[lay]
                y, res, ss = Out(c.M, N), Out(c.M, N, fill=c.res), Out(c.M, N // 128, dtype=F32)
                H().decode_gemm_launch_counts(True)
                H().decode_gemm_res(y.t, x, w, ws, cnt, res.t, bf(c.g), ss.t, err)
                census_is(gp.dg_key(c.M, 128, "cmb_res", S))
                compare(c, "decode_gemm_res", {"residual": res.t, "y": y.t, "sumsq": ss.t}, x=xc)
                for o in (y, res, ss):
                    o.guards_intact(c.name)
                calls += 1
                assert cnt.tolist() == [calls * S] * (N // 128)
        assert int(err.item()) == 0


@pytest.mark.parametrize("spec", gp.SPECS["cmb_qkv"], ids=str)
def test_decode_gemm_qkv_combine(spec):
    K, _ = spec
    wc = None
    for c in gp.cases("cmb_qkv", spec):
        S = H().decode_gemm_cmb_splits(c.N, K)
        assert S == c.S > 1
        wc = w_dev(c, wc)
        w = wc[1]
        cnt = torch.zeros(c.N // 128, dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws, parts = nan_ws(S * c.M * c.N), c.parts.to(DEV)
        calls = 0
        for lay in range(2):
            for xc in c.xs:
                x = x_layouts(xc)[lay]
                out, kv = Out(c.M, c.N, window=bool(lay)), Caches(c)
                H().decode_gemm_launch_counts(True)
                H().decode_gemm_qkv_cmb(out.t, x, w, ws, cnt, parts, gp.EPS, *qkv_args(c), kv.kc, kv.vc, c.Hq, c.Hkv,
                                        err)
                census_is(gp.dg_key(c.M, 128, "cmb_qkv", S))
                compare(c, "decode_gemm_qkv_cmb", {"qkv": out.t}, x=xc)
                k, v = kv.rows_and_rest()
                rows = out.t[kv.valid.to(DEV)].float()
                d0 = c.Hq * c.D
                assert torch.equal(k, rows[:, d0: d0 + c.Hkv * c.D]) and torch.equal(v, rows[:, d0 + c.Hkv * c.D:]), \
                    "the caches hold the written rows"
                out.guards_intact(c.name)
                calls += 1
                assert cnt.tolist() == [calls * S] * (c.N // 128)
        assert int(err.item()) == 0


@pytest.mark.parametrize("spec", gp.SPECS["silu_r"], ids=str)
def test_decode_gemm_silu_r(spec):
    F, K, _ = spec
    wc = None
    for c in gp.cases("silu_r", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        for lay, x in enumerate(x_layouts(c.x)):
            out = Out(c.M, F, window=bool(lay))
            H().decode_gemm_launch_counts(True)
            H().decode_gemm_silu_r(out.t, x, w, c.parts.to(DEV), gp.EPS)
            census_is(gp.dg_key(c.M, 128, "silu_r", 1))
            compare(c, "decode_gemm_silu_r", {"out": out.t})
            out.guards_intact(c.name)


@pytest.mark.parametrize("N", [128, 2056])      # 2056 = 8 x 257: one column group past the 256-thread stride
def test_rms_prep_and_rows_rms_scale(N):
    """The row helpers of the norm-deferred layer: y = h * g and sum h^2 are exact on integer
    rows; out = y / rms rounds once."""
    for M in (1, 129, 256):
        h = gp.ints(-64, 64, (M, N), 73 + M)
        g = gp.norm_weights(N, 79)
        y, ss = Out(M, N), Out(M, 1, dtype=F32)
        H().rms_prep(y.t, ss.t, bf(h), bf(g))
        assert torch.equal(y.t.float().cpu(), h * g) and torch.equal(ss.t.cpu()[:, 0], h.pow(2).sum(1))
        parts = gp.sumsq_parts(M, N, 5, 83) if M > 1 else torch.full((1, 5), 0.3 * N)
        out = Out(M, N)
        H().rows_rms_scale(out.t, y.t, parts.to(DEV), gp.EPS)
        ref = (h * g).double() * gp.row_scale(parts, N)[:, None]
        e = gp.excess(out.t.float().cpu(), ref)
        WORST["rows_rms_scale"] = max(WORST.get("rows_rms_scale", 0.0), e)
        assert not gp.rejected(gp.ROUNDED, out.t.float().cpu(), ref), e
        for o in (y, ss, out):
            o.guards_intact(f"rms helpers M{M} N{N}")


# ------------------------------------------------------------------------------ gemm_prefill.hip
def _prefill(family, spec, entry, silu=False):
    v = spec[0] if family not in ("prefill_f32", "prefill_splitk") else 1
    wc = None
    for c in gp.cases(family, spec):
        wc = w_dev(c, wc)
        w = wc[1]
        assert H().gemm_prefill_supported(w, silu)
        for lay, x in enumerate(x_layouts(c.x)):
            if family == "prefill_f32":
                assert H().gemm_prefill_f32_supported(w)
                out = Out(c.M, c.N, dtype=F32)
                H().gemm_prefill_f32(out.t, x, w)
            else:
                out = Out(c.M, c.N // 2 if silu else c.N, window=bool(lay))
                H().gemm_prefill(out.t, x, w, silu, v)
            compare(c, entry, {"out": out.t})
            out.guards_intact(c.name)


@pytest.mark.parametrize("spec", gp.SPECS["prefill"], ids=str)
def test_gemm_prefill(spec):
    _prefill("prefill", spec, "gemm_prefill")


@pytest.mark.parametrize("spec", gp.SPECS["prefill_f32"], ids=str)
def test_gemm_prefill_f32(spec):
    _prefill("prefill_f32", spec, "gemm_prefill_f32")


@pytest.mark.parametrize("spec", gp.SPECS["prefill_big"], ids=str)
def test_gemm_prefill_persistent_walks_tiles(spec):
    """More tiles than CUs at one tile pair of K: a persistent workgroup walks two tiles."""
    _prefill("prefill_big", spec, "gemm_prefill")


@pytest.mark.parametrize("spec", gp.SPECS["prefill_splitk"], ids=str)
def test_gemm_prefill_splitk(spec):
    _prefill("prefill_splitk", spec, "gemm_prefill")


@pytest.mark.parametrize("spec", gp.SPECS["prefill_silu"], ids=str)
def test_gemm_prefill_silu(spec):
    _prefill("prefill_silu", spec, f"gemm_prefill silu v{spec[0]}", silu=True)


# ------------------------------------------------------------------------------ gemm_skinny.hip
@pytest.mark.parametrize("spec", gp.SPECS["skinny"], ids=str)
def test_skinny_gemm(spec):
    kind, N, K = spec
    wc = None
    for c in gp.cases("skinny", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        for lay, x in enumerate(x_layouts(c.x)):
            if kind == "plain":
                out = Out(c.M, N, window=bool(lay))
                H().skinny_gemm(out.t, x, w)
                compare(c, "skinny_gemm", {"out": out.t})
            elif kind == "silu":
                out = Out(c.M, N)
                H().skinny_gemm_silu(out.t, x, w)
                compare(c, "skinny_gemm_silu", {"out": out.t})
            else:
                out, res = Out(c.M, N), Out(c.M, N, fill=c.res)
                H().skinny_gemm_add_rmsnorm(out.t, x, w, res.t, bf(c.g), gp.EPS)
                compare(c, "skinny_gemm_add_rmsnorm", {"residual": res.t, "out": out.t})
                res.guards_intact(c.name + " residual")
            out.guards_intact(c.name)


# ------------------------------------------------------------------------------ gemm_gemv.hip
@pytest.mark.parametrize("spec", gp.SPECS["gemv"], ids=str)
def test_gemv(spec):
    kind, N, K = spec
    wc = None
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for c in gp.cases("gemv", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        assert H().gemv_supported(w, kind in ("silu", "silu_norm"))
        T = c.M
        for lay in range(2):
            win = bool(lay)
            if kind in ("norm", "silu_norm", "qkv_pro"):
                pro = [bf(c.o), bf(c.res), Out(T, K), bf(c.nw)]
            if kind == "plain":
                out = Out(T, N, window=win)
                H().gemv(out.t, bf(c.x), w)
                compare(c, "gemv", {"out": out.t})
            elif kind == "silu":
                out = Out(T, N // 2, window=win)
                H().gemv_silu(out.t, bf(c.x), w)
                compare(c, "gemv_silu", {"out": out.t})
            elif kind == "addnorm":
                for xc in c.xs:
                    out, res = Out(T, N), Out(T, N, fill=c.res)
                    H().gemv_add_rmsnorm(out.t, bf(xc), w, res.t, bf(c.g), gp.EPS, ticket)
                    compare(c, "gemv_add_rmsnorm", {"residual": res.t, "out": out.t}, x=xc)
                    res.guards_intact(c.name + " residual")
                    out.guards_intact(c.name)
                    assert int(ticket.item()) == 0
            elif kind in ("norm", "silu_norm"):
                out = Out(T, N // 2 if kind == "silu_norm" else N, window=win)
                (H().gemv_silu_norm if kind == "silu_norm" else H().gemv_norm)(out.t, pro[0], pro[1], pro[2].t, pro[3],
                                                                              gp.EPS, w)
                compare(c, "gemv_" + kind, {"out": out.t})
            else:
                out, kv = Out(T, N, window=win), Caches(c)
                extra = [pro[0], pro[1], pro[2].t, pro[3]] if kind == "qkv_pro" else [None] * 4
                H().gemv_qkv(out.t, pro[0] if kind == "qkv_pro" else bf(c.x), w, *qkv_args(c), kv.kc, kv.vc, c.Hq,
                             c.Hkv, True, *extra, gp.EPS)
                compare(c, "gemv_qkv", {"qkv": out.t})
                k, v = kv.rows_and_rest()
                compare(c, "gemv_qkv", {"k": k, "v": v}, rows=kv.valid)
            if kind in ("norm", "silu_norm", "qkv_pro"):
                assert torch.equal(pro[2].t.float().cpu(), c.h), "res_out = o + res"
                pro[2].guards_intact(c.name + " res_out")
            out.guards_intact(c.name)


def test_gemv_rejects_a_strided_x():
    """No caller passes the GEMVs a strided x and the kernel indexes rows by K: the check
    refuses it."""
    c = gp.gemv_case(2, 8, 512, "plain")
    out = torch.empty(2, 8, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous x"):
        H().gemv(out, x_layouts(c.x)[1], bf(c.w))


# ------------------------------------------------------------------------------ gemm_fused.hip
@pytest.mark.parametrize("spec", gp.SPECS["fused"], ids=str)
def test_gemm_fused(spec):
    mode, N, K = spec
    wc = None
    for c in gp.cases("fused", spec):
        wc = w_dev(c, wc)
        w = wc[1]
        for lay, x in enumerate(x_layouts(c.x)):
            out = Out(c.M, N, window=bool(lay))
            kw, got = {}, {"out": out.t}
            if c.bias is not None:
                kw["bias"] = bf(c.bias)
            if c.res is not None:
                res = Out(c.M, N, window=bool(lay), fill=c.res)
                st = Out(c.M, (N // 64) * 2, dtype=F32)
                kw.update(residual=res.t, stats_out=st.t.view(c.M, N // 64, 2))
                got["stats"] = st.t
            ops.gemm_fused(x, w, out=out.t, **kw)
            compare(c, "gemm_fused " + mode, got)
            out.guards_intact(c.name)
            if c.res is not None:
                st.guards_intact(c.name + " stats")
                assert torch.equal(res.t.float().cpu(), c.res), "the residual operand is read only"
