"""Pointer-query inputs for the attention tests (a plain module, shared by
test_attention_probe_cpu.py and test_attention_probe_gpu.py).

With randn q / K / V the softmax is nearly flat: one key of a 777-key context carries
weight ~1/777, and an attention kernel that drops, leaks or mis-pairs ONE key stays inside
the project's 0.03 + 0.03|ref| tolerance.  Here the caches stay the project's random paged
caches (random K and V everywhere, tails of last blocks and spare blocks included; permuted
block tables with at least one spare column that names a real random block), but every
query head *points* at one key t of its kv head:

    q = K[t] * (SCORE * sqrt(D) / |K[t]|^2),   SCORE = sqrt(128)

so with scale = 1/sqrt(D) the target's score is SCORE (~11.3, what q = K[t] gives on
average at D = 128) and every other key scores ~N(0, (SCORE/|K[t]|)^2).  The rescaling
(instead of the bare q = K[t]) is what lets the weight condition below hold for every one
of the thousands of targets of a prefill / wave-per-pair case and at D = 64 and 32, where
|K|^2/sqrt(D) is only ~8 and ~5.7.  The output of the head is then ~V[t], of order 1 to 4:

* IN targets lie inside the context: losing the key moves the output by ~|V[t]|;
* PAST targets lie just outside it (key n, n + 1, the next 8-key V group, the last slot of
  the last block, key 0 of the spare block, a neighbouring sequence's token, the stale
  slot a fused write is about to overwrite): the reference ignores them, so the expected
  output is small, and a kernel that lets one in is off by ~|V[t]|;
* TWO heads point at two keys (first / last block) with equal scores: the LDS merge and
  the KV-split merge have to weight two partial softmaxes correctly.

Weight condition (asserted here in fp64, a condition on the inputs): every IN target has
softmax weight >= MIN_WEIGHT, every PAST target would have it if it were visible, the two
keys of a TWO head share >= MIN_WEIGHT with >= 0.35 each.

Every builder returns a Probe: the operator's inputs (CPU tensors) plus one View per
sequence -- the same problem as dense f32 q / K / V with per-head target bookkeeping, which
the CPU test uses to mutate the reference.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from langstream_amd import ops
from langstream_amd.ops import reference as ref

BS = ops.KV_BLOCK
SCORE = math.sqrt(128.0)
MIN_WEIGHT = 0.9
MIN_HALF = 0.35
IN, PAST, TWO = 0, 1, 2
DECOY = -2      # View.pos of the stale key a fused-RoPE step overwrites
PREV = -1       # View.pos of the previous sequence's last token (encoder)


# ------------------------------------------------------------------------------ pieces
def point(k):
    """The pointer query of key rows k [..., D] (f32)."""
    D = k.shape[-1]
    return k * (SCORE * math.sqrt(D) / k.pow(2).sum(-1, keepdim=True))


def point2(k1, k2):
    """a k1 + b k2 with q.k1 == q.k2 == SCORE * sqrt(D)."""
    D = k1.shape[-1]
    n1, n2, c = k1.pow(2).sum(-1, keepdim=True), k2.pow(2).sum(-1, keepdim=True), (k1 * k2).sum(-1, keepdim=True)
    s = SCORE * math.sqrt(D) / (n1 * n2 - c * c)
    return k1 * (s * (n2 - c)) + k2 * (s * (n1 - c))


def paged_cache(nblk, Hkv, D, seed, kv=None):
    """_random_paged of test_kernels_gpu.py on the CPU with spare columns: table s owns nblk[s]
    blocks; every later column (at least one) names one of three spare random blocks.
    kv = (k_scale, v_scale): fp8 codes of the same randn values."""
    g = torch.Generator().manual_seed(seed)
    NB, ncols = sum(nblk) + 3, max(nblk) + 1
    kc = torch.randn(NB, Hkv, BS, D, generator=g)
    vc = torch.randn(NB, Hkv, BS // 8, D, 8, generator=g)
    if kv is None:
        kc, vc = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    else:
        kc, vc = ref.quantize_kv(kc, kv[0]), ref.quantize_kv(vc, kv[1])
    perm = torch.randperm(NB, generator=g)
    bt = torch.zeros(len(nblk), ncols, dtype=torch.int32)
    used = 0
    for s, nb in enumerate(nblk):
        for i in range(ncols):
            if i < nb:
                bt[s, i] = perm[used]
                used += 1
            else:
                bt[s, i] = perm[NB - 3 + (s + i) % 3]
    return kc, vc, bt


def stream(kc, vc, bt_row, kv=None):
    """Every key / value a block-table row names, spare columns included, dequantised:
    f32 K, V [ncols * 64, Hkv, D]."""
    K, V = ref.gather_kv(kc, vc, bt_row, bt_row.numel() * BS)
    K, V = ref.dequant_kv(K, V, *(kv or (1.0, 1.0)))
    return K.float().contiguous(), V.float().contiguous()


def make_view(q, K, V, pos, n, kind, t, t2):
    v = SimpleNamespace(q=q, K=K, V=V, pos=pos, n=n, kind=kind, t=t, t2=t2)
    v.Hq, v.Hkv = q.shape[1], K.shape[1]
    return v


def base_visible(v):
    """[Tq, Tk]: key positions 0 .. n - 1 of each query row."""
    return (v.pos[None, :] >= 0) & (v.pos[None, :] < v.n[:, None])


def target_weights(v, scale):
    """fp64 softmax weight of each head's target(s): [Tq, Hq] for t and for t2 (0 where
    there is none).  PAST targets are weighed as if they were visible."""
    Tq, Hq, D = v.q.shape
    G = Hq // v.Hkv
    s = torch.einsum("qvgd,kvd->qvgk", v.q.double().reshape(Tq, v.Hkv, G, D), v.K.double()).reshape(Tq, Hq, -1) * scale
    lse = torch.logsumexp(s.masked_fill(~base_visible(v)[:, None, :], float("-inf")), -1)
    st = s.gather(-1, v.t[..., None])[..., 0]
    st2 = s.gather(-1, v.t2.clamp(min=0)[..., None])[..., 0]
    w_in = (st - lse).exp()
    w_past = 1.0 / (1.0 + (lse - st).exp())
    w = torch.where(v.kind == PAST, w_past, w_in)
    w2 = torch.where(v.kind == TWO, (st2 - lse).exp(), torch.zeros_like(w))
    return w, w2


def check_weights(views, scale):
    """The weight condition; returns the smallest single-pointer weight."""
    lo = 1.0
    for v in views:
        w, w2 = target_weights(v, scale)
        v.weight = w
        single = v.kind != TWO
        if single.any():
            m = float(w[single].min())
            assert m >= MIN_WEIGHT, f"single-pointer target weight {m:.3f} < {MIN_WEIGHT}"
            lo = min(lo, m)
        two = v.kind == TWO
        if two.any():
            assert float((w + w2)[two].min()) >= MIN_WEIGHT and float(torch.minimum(w, w2)[two].min()) >= MIN_HALF, \
                "two-pointer head does not split its weight over both keys"
    return lo


def _assign(entries, nslots):
    """Entries cycled over nslots head slots -> (kind, t, t2) lists."""
    e = [entries[i % len(entries)] for i in range(nslots)]
    return [x[0] for x in e], [x[1] for x in e], [x[2] if len(x) > 2 else -1 for x in e]


def _fill(qf, K, kvh_of_head, kind, t, t2):
    """qf [Hq, D] <- pointer queries at K [Tk, Hkv, D] rows t (and t2 for TWO heads)."""
    for j in range(qf.shape[0]):
        k1 = K[t[j], kvh_of_head[j]]
        qf[j] = point2(k1, K[t2[j], kvh_of_head[j]]) if kind[j] == TWO else point(k1)


# ------------------------------------------------------------------------------ decode
def decode_targets(n, nblk_every=0):
    """(kind, t[, t2]) entries of a decode context of n keys; nblk_every > 0 adds one key in
    each of that many blocks."""
    ins = {t for t in (0, n - 1, n - 2, 8 * ((n - 1) // 8), 64 * ((n - 1) // 64), 63, 64) if 0 <= t < n}
    ins |= {min(64 * b + (11 * b + 5) % 64, n - 1) for b in range(nblk_every)}
    up8, up64 = 8 * -(-n // 8), 64 * -(-n // 64)
    past = {t for t in (n, n + 1, up8, up64 - 1, up64) if t >= n}
    e = [(IN, t) for t in sorted(ins)] + [(PAST, t) for t in sorted(past)]
    if n >= 2:
        t1 = min(37, n - 2)
        e.append((TWO, t1, max(64 * ((n - 1) // 64) + ((n - 1) % 64) // 2, t1 + 1)))
    return e


def decode_probe(ctx, Hkv, G, D, seed, kv=None, ntables=None):
    """ops.paged_decode_attention inputs.  ntables None: each context length gets its own
    block table and as many batch rows (Hkv * G targets each, sharing the table) as its
    targets need; the longest also points into every one of its blocks.  ntables = N: one
    row per entry of ctx, row r on table r % N (rows share tables at different ctx_len)."""
    Hq = Hkv * G
    nb = lambda n: (n + BS - 1) // BS
    if ntables is None:
        tab_ctx = list(ctx)
        rows = []
        for s, n in enumerate(ctx):
            e = decode_targets(n, nb(n) if n == max(ctx) else 0)
            for r in range(-(-len(e) // Hq)):
                rows.append((s, n, e[r * Hq:] + e[: r * Hq]))
    else:
        tab_ctx = [max(ctx[s::ntables]) for s in range(ntables)]
        rows = [(r % ntables, n, decode_targets(n)) for r, n in enumerate(ctx)]
    kc, vc, bt = paged_cache([nb(n) for n in tab_ctx], Hkv, D, seed, kv)
    streams = [stream(kc, vc, bt[s], kv) for s in range(len(tab_ctx))]
    B = len(rows)
    kvh_of = [j // G for j in range(Hq)]
    qf = torch.zeros(B, Hq, D)
    meta = []
    for r, (s, n, e) in enumerate(rows):
        kind, t, t2 = _assign(e, Hq)
        _fill(qf[r], streams[s][0], kvh_of, kind, t, t2)
        meta.append((kind, t, t2))
    q = qf.to(torch.bfloat16)
    views = []
    for r, (s, n, _) in enumerate(rows):
        K, V = streams[s]
        kind, t, t2 = (torch.tensor(x)[None] for x in meta[r])
        views.append(make_view(q[r: r + 1].float(), K, V, torch.arange(K.shape[0]), torch.tensor([n]), kind, t, t2))
    p = SimpleNamespace(q=q.reshape(B, Hq * D), kc=kc, vc=vc, bt=bt[[s for s, _, _ in rows]].contiguous(),
                        ctx=torch.tensor([n for _, n, _ in rows], dtype=torch.int32), scale=1 / math.sqrt(D),
                        kv=kv or (1.0, 1.0), Hkv=Hkv, G=G, Hq=Hq, D=D, B=B, views=views)
    p.min_weight = check_weights(views, p.scale)
    return p


def decode_reference(p):
    return ref.paged_decode_attention(p.q.reshape(p.B, p.Hq, p.D), p.kc, p.vc, p.bt, p.ctx, p.scale,
                                      *p.kv).reshape(p.B, p.Hq * p.D)


# ------------------------------------------------------------------- decode, fused RoPE
def rope_probe(ctx, Hkv, G, D, seed):
    """ops.paged_decode_attention_rope inputs: un-rotated projection rows whose q heads,
    once rotated to the new token's position, point at the new token itself (q row = its k
    row), at cached keys (the cached key counter-rotated: apply_rope with the sin half
    negated), and -- as PAST targets -- at the stale key in the slot the step overwrites
    (a pointed decoy) and at keys n, n + 1.  Every row owns its blocks (it writes one)."""
    Hq = Hkv * G
    nb = lambda n: (n + BS - 1) // BS
    rows = []
    for n in ctx:
        e = [(IN, n - 1), (PAST, DECOY), (PAST, n), (PAST, n + 1)]
        if n >= 2:
            ins = {0, n - 2, 64 * ((n - 2) // 64)}
            if n == max(ctx):
                ins |= {min(64 * b + (11 * b + 5) % 64, n - 2) for b in range(nb(n - 1))}
            e += [(IN, t) for t in sorted(ins)] + [(TWO, min(37, n - 2), n - 1), (TWO, n - 2, n - 1)]
        for r in range(-(-len(e) // Hq)):
            rows.append((n, e[r * Hq:] + e[: r * Hq]))
    B = len(rows)
    kc, vc, bt = paged_cache([nb(n) for n, _ in rows], Hkv, D, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    qkv = torch.randn(B, Hq + 2 * Hkv, D, generator=g).to(torch.bfloat16)
    ctx_t = torch.tensor([n for n, _ in rows], dtype=torch.int32)
    pos = (ctx_t - 1).clamp(min=0)
    slots = torch.tensor([int(bt[b, (n - 1) // BS]) * BS + (n - 1) % BS for b, (n, _) in enumerate(rows)],
                         dtype=torch.int64)
    cs = ref.rope_cos_sin(4096, D, 500000.0)
    cs_inv = torch.cat([cs[:, : D // 2], -cs[:, D // 2:]], -1)
    k_new = ref.apply_rope(qkv[:, Hq: Hq + Hkv], pos, cs).float()          # as the cache will hold it
    v_new = qkv[:, Hq + Hkv:].float()
    kvh_of = [j // G for j in range(Hq)]
    want = torch.zeros(B, Hq, D)      # the rotated queries we are after
    parts = []
    for b, (n, e) in enumerate(rows):
        K, V = stream(kc, vc, bt[b])
        K = torch.cat([K, K[n - 1: n]])            # the stale key / value moves to the end ...
        V = torch.cat([V, V[n - 1: n]])
        K[n - 1], V[n - 1] = k_new[b], v_new[b]    # ... and the new token takes its slot
        kind, t, t2 = _assign([(x[0], K.shape[0] - 1 if x[1] == DECOY else x[1]) + tuple(x[2:]) for x in e], Hq)
        _fill(want[b], K, kvh_of, kind, t, t2)
        p_ = torch.arange(K.shape[0])
        p_[-1] = DECOY
        parts.append((K, V, p_, kind, t, t2))
    qkv[:, :Hq] = ref.apply_rope(want, pos, cs_inv).to(torch.bfloat16)
    q_rot = ref.apply_rope(qkv[:, :Hq], pos, cs).float()
    views = [make_view(q_rot[b: b + 1], K, V, p_, torch.tensor([rows[b][0]]), torch.tensor(kind)[None],
                       torch.tensor(t)[None], torch.tensor(t2)[None])
             for b, (K, V, p_, kind, t, t2) in enumerate(parts)]
    p = SimpleNamespace(qkv=qkv.reshape(B, -1), pos=pos, slots=slots, cos_sin=cs, kc=kc, vc=vc, bt=bt, ctx=ctx_t,
                        scale=1 / math.sqrt(D), Hkv=Hkv, G=G, Hq=Hq, D=D, B=B, views=views)
    p.min_weight = check_weights(views, p.scale)
    return p


def rope_reference(p):
    """(attention output, K cache, V cache, rotated rows) of rope_and_cache followed by
    paged_decode_attention, as test_paged_decode_attention_rope computes them."""
    kr, vr, rows = p.kc.clone(), p.vc.clone(), p.qkv.clone()
    ref.rope_and_cache(rows, p.pos, p.cos_sin, p.slots, kr, vr, p.Hq, p.Hkv)
    out = ref.paged_decode_attention(rows[:, : p.Hq * p.D].reshape(p.B, p.Hq, p.D), kr, vr, p.bt, p.ctx, p.scale)
    return out.reshape(p.B, p.Hq * p.D), kr, vr


# ----------------------------------------------------------------------------- prefill
def prefill_probe(q_lens, prefix, Hkv, G, D, seed, kv=None):
    """ops.paged_prefill_attention inputs.  Head j of query token i points at one of: its own
    position prefix + i (IN: the causal mask is `<=`), prefix + i + 1 (PAST; the key is in
    the cache: the next token's, or random data past the context), key 0, prefix - 1 and
    prefix.  The choice rotates with i + j, except on the first and last token and on the
    tokens next to a 128-row tile edge, whose heads start from (own, next) so that a tile's
    last row -- the one that decides kmax -- probes both sides of the mask at every G."""
    Hq = Hkv * G
    ctx = [a + b for a, b in zip(q_lens, prefix)]
    kc, vc, bt = paged_cache([(n + BS - 1) // BS for n in ctx], Hkv, D, seed, kv)
    T = sum(q_lens)
    g = torch.Generator().manual_seed(seed + 1000)
    qkv = torch.randn(T, Hq + 2 * Hkv, D, generator=g).to(torch.bfloat16)
    kvh_of = torch.tensor([j // G for j in range(Hq)])
    starts, views = [], []
    a = 0
    for s, (ql, pre) in enumerate(zip(q_lens, prefix)):
        starts.append(a)
        K, V = stream(kc, vc, bt[s], kv)
        i = torch.arange(ql)[:, None]
        j = torch.arange(Hq)[None, :]
        cand = torch.stack([pre + i, pre + i + 1, 0 * i, 0 * i + pre, 0 * i + max(pre - 1, 0)], -1)  # [ql, 1, 5]
        nk = 5 if pre >= 1 else 4
        edge = torch.zeros(ql, dtype=torch.bool)
        edge[0] = edge[-1] = True
        for r in range(ops.PREFILL_ROWS, ql * G, ops.PREFILL_ROWS):
            edge[(r - 1) // G] = edge[r // G] = True
        c = (j + torch.where(edge[:, None], 0 * i, i)) % nk                     # [ql, Hq]
        t = cand.expand(ql, Hq, 5).gather(-1, c[..., None])[..., 0]
        kind = torch.where(c == 1, PAST, IN)
        qf = point(K[t, kvh_of[None, :].expand(ql, Hq)])
        qkv[a: a + ql, :Hq] = qf.to(torch.bfloat16)
        views.append(make_view(qkv[a: a + ql, :Hq].float(), K, V, torch.arange(K.shape[0]), pre + i[:, 0] + 1, kind, t,
                               torch.full_like(t, -1)))
        a += ql
    p = SimpleNamespace(q=qkv.reshape(T, -1), kc=kc, vc=vc, bt=bt, q_start=torch.tensor(starts, dtype=torch.int32),
                        q_len=torch.tensor(q_lens, dtype=torch.int32), ctx=torch.tensor(ctx, dtype=torch.int32),
                        tiles=ops.prefill_tiles(q_lens, G, prefix), scale=1 / math.sqrt(D), kv=kv or (1.0, 1.0),
                        Hkv=Hkv, G=G, Hq=Hq, D=D, views=views)
    p.min_weight = check_weights(views, p.scale)
    return p


def prefill_reference(p):
    return ref.paged_prefill_attention(p.q, p.kc, p.vc, p.bt, p.q_start, p.q_len, p.ctx, p.Hq, p.scale, *p.kv)


# ----------------------------------------------------------------------------- encoder
def encoder_probe(lens, H, D, seed):
    """ops.varlen_encoder_attention inputs (packed randn qkv, Hq = Hkv = H).  Head h of token
    i points, rotating with i + h, at key n - 1 and key 0 of its sequence (IN) and at the
    next sequence's first token -- which is key n -- and the previous sequence's last
    token (PAST); the first / last sequence has only one neighbour."""
    T = sum(lens)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, 3 * H, D, generator=g).to(torch.bfloat16)
    starts, views = [], []
    a = 0
    for s, n in enumerate(lens):
        starts.append(a)
        lo, hi = (a - 1 if s > 0 else a), (a + n + 1 if s + 1 < len(lens) else a + n)
        K, V = qkv[lo:hi, H: 2 * H].float(), qkv[lo:hi, 2 * H:].float()
        pos = torch.arange(lo, hi) - a                                       # PREV, 0 .. n - 1, n
        idx = {int(x): k for k, x in enumerate(pos)}
        opts = [(IN, n - 1), (IN, 0)] + ([(PAST, n)] if n in idx else []) + ([(PAST, PREV)] if PREV in idx else [])
        c = (torch.arange(n)[:, None] + torch.arange(H)[None, :]) % len(opts)
        kind = torch.tensor([o[0] for o in opts])[c]
        t = torch.tensor([idx[o[1]] for o in opts])[c]
        qkv[a: a + n, :H] = point(K[t, torch.arange(H)[None, :].expand(n, H)]).to(torch.bfloat16)
        views.append(make_view(qkv[a: a + n, :H].float(), K, V, pos, torch.full((n,), n), kind, t,
                               torch.full_like(t, -1)))
        a += n
    p = SimpleNamespace(qkv=qkv.reshape(T, -1), q_start=torch.tensor(starts, dtype=torch.int32),
                        q_len=torch.tensor(lens, dtype=torch.int32), tiles=ops.prefill_tiles(lens, 1),
                        scale=1 / math.sqrt(D), H=H, Hq=H, D=D, views=views)
    p.min_weight = check_weights(views, p.scale)
    return p


def encoder_reference(p):
    return ref.varlen_encoder_attention(p.qkv, p.q_start, p.q_len, p.H, p.H, p.scale)


# ------------------------------------------------------------------- the cases, built once
DECODE_CTX = [0, 1, 2, 8, 9, 63, 64, 65, 128, 129, 300, 777]
DECODE_SHAPES = [(D, G) for D in (64, 128) for G in (1, 4, 16)]
SPLITS = [(1, 4), (3, 1), (16, 1)]
FP8_SCALES = [(1.0, 1.0), (0.25, 4.0)]
ROPE_CTX = [1, 2, 65, 129, 777]
PREFILL_LENS, PREFILL_PREFIX = [1, 17, 64, 130, 200], [0, 5, 64, 0, 300]
PREFILL_SHAPES = [(D, G) for D in (64, 128) for G in (1, 4, 8)]
ENCODER_SHAPES = [(32, 12), (64, 4)]
ENCODER_LENS = [3, 64, 65, 200]
_cache = {}


def _once(key, build, reference):
    if key not in _cache:
        p = build()
        p.expect = reference(p)
        _cache[key] = p
    return _cache[key]


def decode_case(D, G, kv=None):
    return _once(("decode", D, G, kv), lambda: decode_probe(DECODE_CTX, 2, G, D, seed=D + G, kv=kv), decode_reference)


def wave_per_pair_case():
    ctx = torch.randint(1, 300, (256,), generator=torch.Generator().manual_seed(7)).tolist()
    return _once("wpp", lambda: decode_probe(ctx, 8, 4, 128, seed=3, ntables=32), decode_reference)


def rope_case():
    return _once("rope", lambda: rope_probe(ROPE_CTX, 2, 4, 128, seed=5), rope_reference)


def prefill_case(D, G, kv=None):
    return _once(("prefill", D, G, kv),
                 lambda: prefill_probe(PREFILL_LENS, PREFILL_PREFIX, 2, G, D, seed=10 + D + G, kv=kv), prefill_reference)


def encoder_case(D, H):
    return _once(("encoder", D, H), lambda: encoder_probe(ENCODER_LENS, H, D, seed=20 + D), encoder_reference)
