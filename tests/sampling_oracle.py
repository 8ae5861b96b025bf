"""A CPU model of the sampler in sampling.hip (a plain numpy module, shared by
test_sampling_oracle_cpu.py and test_sampling_gpu.py).

The kernel's noise is a pure function of (seed, step, token index) and its top-k / top-p
cut is an integer histogram rule, so a row can be replayed here and the kernel asked for
*the* token, not for a token that roughly follows the softmax:

* noise   row_key / uniform01: the kernel's integer hashes, and the f32 value it makes of
          the top 24 bits ((float)(h >> 8) + 0.5f rounds to even above 2^23; the one value
          that would round to u = 1 is clamped to 1 - 2^-24, as in the kernel);
* bins    z = (x - max) * (1/T), bin = min(1023, int((z + 32) * 32)) in f32, in the
          kernel's operation order (a subtract feeding a multiply and an add feeding a
          multiply cannot contract to an FMA, so the bins are the kernel's bit for bit),
          bin = -1 below -32.  The maximum is exact and the subtract, multiply and add are
          IEEE on both sides, so 1/T is the one value of the chain that a device could
          round differently: *edge* elements are those whose bin changes when 1/T moves by
          up to EDGE_ULPS = 2 f32 ulps, i.e. whose scaled value sits within 2 ulps of an
          integer in the only way that can matter (the distance of the scaled value
          itself would flag the row maximum, which is exactly 1024, and every bf16 logit
          at T = 1, which sit on integers by construction and cannot move).  Where 1/T
          is exact (T a power of two) there is nothing to round and no element is an edge;
* cut     the highest bin whose suffix count is >= k or whose suffix mass is >= p * total
          (mass = floor(exp(z) * 2^24), summed in f64: the kernel's fixed point), the
          higher bin when both rules are on, bin 0 when neither hits; the top-p margin is
          min over bins |suffix / total - p|;
* kept    strict = bin >= cut (every finite element when the row is unrestricted),
          loose = strict + the edge elements of bin cut - 1;
* pick    gz = z - log(-log(u)) in f64 over the kept set, argmax with the lower index
          winning ties, the margin to the runner-up, and score(token) for any token;
* greedy / log Z / top-n in f64, lower index first among equals, -inf entries ignored.

The fixtures of the GPU tests are built here too (``replay_cases`` and friends), so that
the CPU test can assert the input conditions on exactly the rows the kernel will see:
no edge element in bins cut - 1 or cut, and no top-p margin under P_MARGIN.  Generator
seeds are advanced per row until both hold; no row is dropped afterwards.
"""
from __future__ import annotations

import functools
from fractions import Fraction
from dataclasses import dataclass, field

import numpy as np

NT = 1024                    # threads per row (== bins)
NBINS = 1024
RANGE = 32.0
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
EDGE_ULPS = 2                # how far 1/T may move before an element counts as an edge
P_MARGIN = 1e-4              # f32 epsilon x the 1024-term scan (~6e-5) + the __expf error
U_MAX = np.float32(1.0 - 2.0 ** -24)
DTYPES = ("f32", "bf16")
LAYOUTS = ("aligned", "odd_pitch", "offset", "tail")


# ------------------------------------------------------------------------------ noise
def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def row_key(seed: int, step: int) -> int:
    """32-bit row key of the int64 (seed, step); negative values wrap as two's complement."""
    z = mix64((int(seed) * 0x2545F4914F6CDD1D + int(step)) & M64)
    return (z & M32) ^ (z >> 32)


def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def hash32_inv(h: int) -> int:
    """Inverse of hash32 on one Python int (hash32 is a bijection of uint32)."""
    x = h & M32
    x ^= x >> 16
    x = (x * pow(0x846CA68B, -1, 1 << 32)) & M32
    x ^= (x >> 15) ^ (x >> 30)
    x = (x * pow(0x7FEB352D, -1, 1 << 32)) & M32
    x ^= x >> 16
    return x


def uniform01(key: int, idx):
    """The kernel's f32 draw for each uint32 index, returned as f64."""
    idx = np.asarray(idx, dtype=np.uint32)
    h = hash32(idx.astype(np.uint64) * np.uint64(0x9E3779B9) + np.uint64(key))
    t = (h >> np.uint32(8)).astype(np.float32) + np.float32(0.5)
    u = np.minimum(t * np.float32(2.0 ** -24), U_MAX)
    return u.astype(np.float64)


def index_with_top_draw(key: int, limit: int):
    """An index < limit whose 24 hash bits are all ones under ``key`` (the draw that the f32
    sum rounds up to 2^24), or None."""
    inv = pow(0x9E3779B9, -1, 1 << 32)
    for low in range(256):
        i = ((hash32_inv(0xFFFFFF00 | low) - key) * inv) & M32
        if i < limit:
            return i
    return None


# ------------------------------------------------------------------------------- bins
def round_bf16(a):
    """f32 array rounded to the nearest bf16 (ties to even), kept as f32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def row_max(x):
    f = x[~np.isnan(x)]
    return np.float32(f.max()) if f.size else np.float32(-np.inf)


def _bin_of(x, gm, invT):
    with np.errstate(invalid="ignore", over="ignore"):
        z = (x - gm) * invT
        s = (z + np.float32(RANGE)) * np.float32(NBINS / RANGE)
        s = np.nan_to_num(s, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)
        return z, np.where(z >= np.float32(-RANGE), np.minimum(NBINS - 1, s), -1)


def bins(x, T):
    """(z f32, bin int, edge bool) of one f32 row at temperature T > 0."""
    x = np.asarray(x, dtype=np.float32)
    gm = row_max(x)
    invT = np.float32(1.0) / np.float32(T)
    z, b = _bin_of(x, gm, invT)
    edge = np.zeros(x.shape, dtype=bool)
    if Fraction(float(invT)) * Fraction(float(np.float32(T))) == 1:
        return z, b, edge                     # 1/T is exact (a power of two): nothing can move
    lo = hi = invT
    for _ in range(EDGE_ULPS):
        lo, hi = np.nextafter(lo, np.float32(0.0)), np.nextafter(hi, np.float32(np.inf))
        edge |= (_bin_of(x, gm, lo)[1] != b) | (_bin_of(x, gm, hi)[1] != b)
    return z, b, edge


def cut(z, b, V, k, p):
    """(cut bin, top-p margin) for top_k = k, top_p = p; (-1, inf) for an unrestricted row."""
    need_cnt = 0 < k < V
    p = float(np.float32(p))
    need_mass = 0.0 < p < 1.0
    if not (need_cnt or need_mass):
        return -1, np.inf
    ok = b >= 0
    cnt = np.bincount(b[ok], minlength=NBINS)
    mass = np.bincount(b[ok], weights=np.floor(np.exp(z[ok].astype(np.float64)) * 2.0 ** 24), minlength=NBINS)
    sc = np.cumsum(cnt[::-1])[::-1]
    sm = np.cumsum(mass[::-1])[::-1]
    tot = sm[0]
    hit = np.zeros(NBINS, dtype=bool)
    if need_cnt:
        hit |= sc >= k
    margin = np.inf
    if need_mass:
        hit |= sm >= p * tot
        if tot > 0:
            margin = float(np.min(np.abs(sm / tot - p)))
    c = int(np.nonzero(hit)[0].max()) if hit.any() else 0
    return c, margin


@dataclass
class Replay:
    x: np.ndarray
    z: np.ndarray
    bin: np.ndarray
    edge: np.ndarray
    cut: int
    p_margin: float
    strict: np.ndarray
    loose: np.ndarray
    gz: np.ndarray = field(default=None)        # f64 scores, -inf outside the loose set
    token: int = -1
    margin: float = np.inf

    def score(self, tok: int) -> float:
        return float(self.gz[tok]) if 0 <= tok < self.gz.size else -np.inf

    @property
    def best(self) -> float:
        return float(self.gz[self.token])

    @property
    def edges_at_cut(self) -> int:
        if self.cut < 0:
            return 0
        return int((self.edge & ((self.bin == self.cut) | (self.bin == self.cut - 1))).sum())


def cut_row(x, T, k, p) -> Replay:
    """Everything about a row that does not depend on the noise."""
    x = np.asarray(x, dtype=np.float32)
    z, b, edge = bins(x, T)
    c, pm = cut(z, b, x.size, int(k), p)
    strict = (b >= c) if c >= 0 else np.isfinite(x)
    loose = strict | (edge & (b == c - 1)) if c >= 0 else strict
    return Replay(x, z, b, edge, c, pm, strict, loose)


def pick(r: Replay, seed: int, step: int) -> Replay:
    """The Gumbel-max pick of a cut row for one (seed, step)."""
    u = uniform01(row_key(seed, step), np.arange(r.x.size, dtype=np.uint32))
    with np.errstate(invalid="ignore"):
        gz = r.z.astype(np.float64) - np.log(-np.log(u))
    gz = np.where(r.loose & ~np.isnan(gz), gz, -np.inf)
    own = np.where(r.strict, gz, -np.inf)
    tok = int(np.argmax(own))                      # first occurrence = lower index
    rest = own.copy()
    rest[tok] = -np.inf
    margin = float(own[tok] - rest.max()) if np.isfinite(rest.max()) else np.inf
    return Replay(r.x, r.z, r.bin, r.edge, r.cut, r.p_margin, r.strict, r.loose, gz, tok, margin)


def replay(x, T, k, p, seed, step) -> Replay:
    return pick(cut_row(x, T, k, p), seed, step)


# ----------------------------------------------------------------------- greedy / top-n
def greedy(x) -> int:
    x = np.asarray(x, dtype=np.float64)
    return int(np.argmax(np.where(np.isnan(x), -np.inf, x)))


def log_z(x) -> float:
    x = np.asarray(x, dtype=np.float64)
    f = x[x > -np.inf]
    m = f.max()
    return float(m + np.log(np.exp(f - m).sum()))


def top_n(x, n: int):
    """Ids of the n largest entries, lower index first among equal values."""
    x = np.asarray(x, dtype=np.float64)
    return np.argsort(-x, kind="stable")[:n]


# ------------------------------------------------------------------- layouts and sizes
def vec(dtype: str) -> int:
    return 4 if dtype == "f32" else 8


def sizes(dtype: str):
    N = vec(dtype)
    return [3, N * NT - 1, N * NT + 1, N * 3 * NT, N * 3 * NT + N, N * 5 * NT + 5]


def layout_ok(layout: str, V: int, dtype: str) -> bool:
    """Whether a row length can be laid out this way (B >= 2 rows)."""
    N = vec(dtype)
    if layout == "aligned":
        return V % N == 0
    if layout == "odd_pitch":
        return V % N != 0
    if layout == "tail":
        return V % N != 0
    return True


def buffer_of(layout: str, V: int, dtype: str):
    """(buffer width, first column) of the [B, width] buffer whose view [:, c:c+V] is the input."""
    N = vec(dtype)
    if layout in ("aligned", "odd_pitch"):
        return V, 0
    up = (V + N - 1) // N * N
    if layout == "offset":
        return up + N, 1
    return up + N, 0


def sweep_path(layout: str, V: int, dtype: str) -> str:
    """Which branches of sweep() a layout / size reaches (for the record in the tests)."""
    N = vec(dtype)
    if layout in ("odd_pitch", "offset"):
        return "scalar"
    nvec = V // N
    unrolled = single = False
    for tid in range(NT):
        v = tid
        while v + 3 * NT < nvec:
            unrolled = True
            v += 4 * NT
        single |= v < nvec
    parts = ["unrolled"] * unrolled + ["single"] * single + ["tail"] * (V % N != 0)
    return "+".join(parts)


def planted_positions(layout: str, V: int, dtype: str):
    """Every boundary of the sweep that exists in a row of V elements."""
    N = vec(dtype)
    nvec = V // N
    pos = {0, N - 1, N, nvec * N - 1, nvec * N, V - 1}
    for t in (0, NT - 1):
        for u in range(4):
            pos.add((t + u * NT) * N)            # the four unrolled vectors of thread 0 / 1023
    pos.add(4 * NT * N)                          # second unrolled round (or the remainder loop)
    rem = []
    for t in range(NT):                          # where each thread enters the remainder loop
        v = t
        while v + 3 * NT < nvec:
            v += 4 * NT
        if v < nvec:
            rem.append(v)
        if t == 0 and v >= 4 * NT:
            pos.add((v - 4 * NT) * N)            # thread 0's last unrolled round
        if t == 0:
            pos |= {w * N for w in range(v, nvec, NT)}   # each of thread 0's remainder rounds
    if rem:
        pos |= {min(rem) * N, rem[0] * N, rem[-1] * N, max(rem) * N}
    return sorted(q for q in pos if 0 <= q < V)


# ---------------------------------------------------------------------------- fixtures
@dataclass
class Case:
    name: str
    dtype: str
    layout: str
    x: np.ndarray            # [B, V] f32 (bf16-representable for dtype == "bf16")
    T: list
    k: list
    p: list
    seed: list
    step: list
    n_top: int = 3

    @property
    def V(self):
        return self.x.shape[1]


TS = (0.25, 0.7, 1.0, 1.3, 100.0)
PS = (1.0, 0.9, 0.5, 1e-6)


def ks(V):
    return (0, 1, 5, 40, V, V + 1)


def conditions_ok(x, T, k, p) -> bool:
    r = cut_row(x, T, k, p)
    return r.edges_at_cut == 0 and r.p_margin >= P_MARGIN


def make_row(tag, V, dtype, T, k, p, mutate=None):
    """randn * 3 row; the generator seed advances until the input conditions hold."""
    for attempt in range(400):
        rng = np.random.default_rng([0x5A3D, *tag, attempt])
        x = (rng.standard_normal(V) * 3.0).astype(np.float32)
        if mutate is not None:
            x = mutate(x, rng)
        if dtype == "bf16":
            x = round_bf16(x)
        if T <= 0 or conditions_ok(x, T, k, p):
            return x
    raise AssertionError(f"no admissible row for {tag} V={V} {dtype} T={T} k={k} p={p}")


def rotation(i, V):
    """Mixed-radix walk over top_k x top_p x T: 120 rows visit every combination."""
    kk = ks(V)[i % 6]
    return TS[(i // 24) % 5], kk, PS[(i // 6) % 4]


def _key_of(i):
    seed = (0x1234567 * (i + 1)) % (1 << 31)
    return seed, (i * 7 + 3) % 1000


@functools.lru_cache(maxsize=None)
def replay_cases():
    cases, i = [], 0
    for dtype in DTYPES:
        for layout in LAYOUTS:
            for V in sizes(dtype):
                if not layout_ok(layout, V, dtype):
                    continue
                B = 6
                rows, T, K, P, S, ST = [], [], [], [], [], []
                for b in range(B):
                    t, k, p = rotation(i, V)
                    rows.append(make_row((1, i), V, dtype, t, k, p))
                    s, st = _key_of(i)
                    T.append(t), K.append(k), P.append(p), S.append(s), ST.append(st)
                    i += 1
                cases.append(Case(f"{dtype}-{layout}-{V}", dtype, layout, np.stack(rows), T, K, P, S, ST))
    V = 128256
    rows, T, K, P, S, ST = [], [], [], [], [], []
    for b, (t, k, p) in enumerate([(1.0, 0, 1.0), (0.7, 40, 0.9), (1.3, 0, 0.5), (100.0, 5, 1.0)]):
        rows.append(make_row((2, b), V, "f32", t, k, p))
        s, st = _key_of(1000 + b)
        T.append(t), K.append(k), P.append(p), S.append(s), ST.append(st)
    cases.append(Case(f"f32-aligned-{V}", "f32", "aligned", np.stack(rows), T, K, P, S, ST))
    return tuple(cases)


STEP_PARAMS = (0.8, 40, 0.95)         # (T, top_k, top_p) of the 64-step row
WIDE_KEYS = [((1 << 32) + 5, 0), ((1 << 40) + 123, 7), (-1, 1), (-(1 << 63), 2), ((1 << 63) - 1, (1 << 33) + 1),
             (-987654321987, -3), (77, -1), (1 << 62, 1 << 62)]


@functools.lru_cache(maxsize=None)
def key_cases():
    """Determinism and key fixtures: one row under 64 steps; wide and negative seeds / steps."""
    out = []
    T, k, p = STEP_PARAMS
    for dtype, V in (("f32", 4 * NT + 1), ("bf16", 8 * NT - 1)):
        x = make_row((3, V), V, dtype, T, k, p)
        n = 64
        out.append(Case(f"steps-{dtype}", dtype, "tail", np.tile(x, (n, 1)), [T] * n, [k] * n, [p] * n, [4242] * n,
                        list(range(n)), n_top=0))
        n = len(WIDE_KEYS)
        out.append(Case(f"wide-{dtype}", dtype, "odd_pitch", np.tile(x, (n, 1)), [1.0] * n, [0] * n, [1.0] * n,
                        [s for s, _ in WIDE_KEYS], [t for _, t in WIDE_KEYS], n_top=0))
    return tuple(out)


def mask_patterns(V, N):
    """name -> indices set to -inf."""
    first = sorted(set(range(min(NT, V))) | {t * N for t in range(NT) if t * N < V})
    keep = {V // 3, V - 2}
    return {
        "index0": [0],
        "lane_first": first,
        "whole_vector": list(range(5 * N, 6 * N)),
        "all_but_two": [i for i in range(V) if i not in keep],
    }


MASK_PARAMS = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 5, 1.0), (1.3, 0, 0.5), (1.0, 40, 0.9)]


@functools.lru_cache(maxsize=None)
def masked_cases():
    out = []
    for dtype in DTYPES:
        N = vec(dtype)
        for layout, V in (("tail", N * NT + 1), ("odd_pitch", N * NT + 1), ("aligned", N * 3 * NT + N)):
            rows, T, K, P, S, ST, j = [], [], [], [], [], [], 0
            for name, idx in mask_patterns(V, N).items():
                ii = np.asarray(idx)

                def mutate(x, rng, ii=ii):
                    x = x.copy()
                    x[ii] = -np.inf
                    return x
                for (t, k, p) in MASK_PARAMS:
                    rows.append(make_row((4, V, j), V, dtype, t, k, p, mutate))
                    s, st = _key_of(5000 + j)
                    T.append(t), K.append(k), P.append(p), S.append(s), ST.append(st)
                    j += 1
            out.append(Case(f"masked-{dtype}-{layout}-{V}", dtype, layout, np.stack(rows), T, K, P, S, ST, n_top=2))
    return tuple(out)


@dataclass
class TPCase:
    name: str
    W: int
    n_top: int
    case: Case


@functools.lru_cache(maxsize=None)
def tp_cases():
    """Vocab-parallel fixtures (f32): aligned slices past the unrolled threshold, masked rows
    (one rank's whole slice banned), a maximum duplicated across two ranks, slices shorter
    than n_top."""
    out = []
    params = [(0.0, 0, 1.0), (0.7, 40, 0.9), (1.0, 0, 0.5), (1.3, 1, 1.0), (1.0, 7, 1.0), (100.0, 0, 1.0),
              (0.25, 5, 0.9), (1.0, 0, 1.0)]
    for V, W, n_top in ((128256, 8, 5), (32064, 2, 5), (32064, 8, 5), (32005, 3, 5), (20, 8, 5)):
        per = (V + W - 1) // W
        rows, T, K, P, S, ST = [], [], [], [], [], []
        muts = [None] * len(params)
        if V > 1000:
            def ban_rank(x, rng, per=per):           # rank 1's whole slice, and index 0
                x = x.copy()
                x[per:2 * per] = -np.inf
                x[0] = -np.inf
                return x

            def ban_some(x, rng):
                x = x.copy()
                x[rng.integers(0, x.size, x.size // 2)] = -np.inf
                return x

            def dup_max(x, rng, per=per, W=W):       # the maximum on two ranks: the lower index must win
                x = x.copy()
                x[(W - 1) * per + 17] = 30.0
                x[per - 3] = 30.0
                return x
            muts = [dup_max, ban_rank, ban_some, None, ban_rank, None, dup_max, ban_some]
        for j, ((t, k, p), mu) in enumerate(zip(params, muts)):
            rows.append(make_row((6, V, W, j), V, "f32", t, k, p, mu))
            s, st = _key_of(7000 + 10 * W + j)
            T.append(t), K.append(k), P.append(p), S.append(s), ST.append(st)
        out.append(TPCase(f"tp-{V}-{W}", W, n_top,
                          Case(f"tp-{V}-{W}", "f32", "aligned", np.stack(rows), T, K, P, S, ST, n_top=n_top)))
    return tuple(out)


# the draw whose 24 hash bits are all ones: (seed, step) and the index that receives it
TOP_DRAW_SEED, TOP_DRAW_STEP, TOP_DRAW_V, TOP_DRAW_INDEX = 99, 757, 4097, 3858


@functools.lru_cache(maxsize=None)
def top_draw_case():
    """A flat row whose element TOP_DRAW_INDEX is 20 nats down and draws the largest u: it must
    lose (its noise is -log(-log(1 - 2^-24)) = 16.6), and wins only if u rounds up to 1."""
    rows = []
    for dtype in DTYPES:
        x = np.zeros((2, TOP_DRAW_V), dtype=np.float32)
        x[:, TOP_DRAW_INDEX] = -20.0
        rows.append(Case(f"topdraw-{dtype}", dtype, "odd_pitch", x, [1.0, 1.0], [0, 0], [1.0, 1.0],
                         [TOP_DRAW_SEED, TOP_DRAW_SEED + 1], [TOP_DRAW_STEP, TOP_DRAW_STEP], n_top=0))
    return tuple(rows)


def sampled_cases():
    """Every fixture whose tokens the GPU tests replay."""
    return replay_cases() + key_cases() + masked_cases() + top_draw_case() + tuple(t.case for t in tp_cases())
