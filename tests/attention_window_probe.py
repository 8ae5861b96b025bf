"""Pointer-query inputs for sliding-window attention (a plain module, shared by
test_attention_window_cpu.py and test_attention_window_gpu.py), built from the pieces of
attention_probe.py: the same random paged caches, pointer queries and Views.

A windowed query at position n - 1 sees the keys lo <= pos < n, lo = max(0, n - W).  The far
edge is probed as hard as the causal edge:

* IN targets: lo, lo + 1, n - 1 and one key in every VISITED block (lo // 64 onwards) of the
  longest context;
* PAST targets: lo - 1, the last key of the 8-key V group and of the block before lo's, key
  0 once it has left the window, and n, n + 1;
* TWO heads point at (lo, n - 1): the LDS merge and the KV-split merge weigh the first and
  the last visible key.

Prefill heads rotate over own position p (IN), p + 1 (PAST), p - W + 1 (IN) and p - W (PAST);
the first row of a 128-row tile (it decides the first KV tile the workgroup visits) starts
from the two far-side targets and its last row (it decides the last) from the two near-side
ones.

Weight condition (asserted in fp64, a condition on the inputs alone): attention_probe's
MIN_WEIGHT / MIN_HALF over the VISIBLE keys; a PAST target is weighed as if it were visible.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

import attention_probe as ap
from attention_probe import BS, DECOY, IN, PAST, TWO, _assign, _fill, make_view, paged_cache, point, stream
from langstream_amd import ops
from langstream_amd.ops import reference as ref


def visible(v):
    """[Tq, Tk]: lo <= pos < n for each query row."""
    return (v.pos[None, :] >= v.lo[:, None]) & (v.pos[None, :] < v.n[:, None])


def check_weights(views, scale):
    """attention_probe.check_weights over the windowed visibility; returns the smallest
    single-pointer weight."""
    low = 1.0
    for v in views:
        Tq, Hq, D = v.q.shape
        G = Hq // v.Hkv
        s = torch.einsum("qvgd,kvd->qvgk", v.q.double().reshape(Tq, v.Hkv, G, D),
                         v.K.double()).reshape(Tq, Hq, -1) * scale
        lse = torch.logsumexp(s.masked_fill(~visible(v)[:, None, :], float("-inf")), -1)
        st = s.gather(-1, v.t[..., None])[..., 0]
        st2 = s.gather(-1, v.t2.clamp(min=0)[..., None])[..., 0]
        w = torch.where(v.kind == PAST, 1.0 / (1.0 + (lse - st).exp()), (st - lse).exp())
        w2 = torch.where(v.kind == TWO, (st2 - lse).exp(), torch.zeros_like(w))
        v.weight = w
        single = v.kind != TWO
        if single.any():
            m = float(w[single].min())
            assert m >= ap.MIN_WEIGHT, f"single-pointer target weight {m:.3f} < {ap.MIN_WEIGHT}"
            low = min(low, m)
        two = v.kind == TWO
        if two.any():
            assert float((w + w2)[two].min()) >= ap.MIN_WEIGHT and \
                float(torch.minimum(w, w2)[two].min()) >= ap.MIN_HALF, \
                "two-pointer head does not split its weight over both keys"
    return low


def _view(q, K, V, pos, n, W, kind, t, t2):
    v = make_view(q, K, V, pos, n, kind, t, t2)
    v.lo = (n - W).clamp(min=0)
    v.W = W
    return v


def far_past(lo):
    """The PAST targets below the window: lo - 1, the last key of the previous 8-key group
    and of the previous block, key 0."""
    return {t for t in (lo - 1, 8 * (lo // 8) - 1, 64 * (lo // 64) - 1, 0) if 0 <= t < lo}


# ------------------------------------------------------------------------------ decode
def decode_targets(n, W, every=False):
    """(kind, t[, t2]) entries of a decode context of n keys under window W; every: one key
    in each visited block as well."""
    lo = max(0, n - W)
    ins = {t for t in (lo, lo + 1, n - 1) if lo <= t < n}
    if every:
        ins |= {min(max(64 * b + (11 * b + 5) % 64, lo), n - 1) for b in range(lo // 64, (n + 63) // 64)}
    past = far_past(lo) | {n, n + 1}
    e = [(IN, t) for t in sorted(ins)] + [(PAST, t) for t in sorted(past)]
    if n - lo >= 2:
        e.append((TWO, lo, n - 1))
    return e


def decode_probe(ctx, W, Hkv, G, D, seed, kv=None, ntables=None):
    """attention_probe.decode_probe with the targets of a window W (the same table layout:
    ntables None gives every context length its own table and as many rows as its targets
    need; ntables = N puts row r on table r % N)."""
    Hq = Hkv * G
    nb = lambda n: (n + BS - 1) // BS
    if ntables is None:
        tab_ctx = list(ctx)
        rows = []
        for s, n in enumerate(ctx):
            e = decode_targets(n, W, n == max(ctx))
            for r in range(-(-len(e) // Hq)):
                rows.append((s, n, e[r * Hq:] + e[: r * Hq]))
    else:
        tab_ctx = [max(ctx[s::ntables]) for s in range(ntables)]
        rows = [(r % ntables, n, decode_targets(n, W)) for r, n in enumerate(ctx)]
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
        views.append(_view(q[r: r + 1].float(), K, V, torch.arange(K.shape[0]), torch.tensor([n]), W, kind, t, t2))
    p = SimpleNamespace(q=q.reshape(B, Hq * D), kc=kc, vc=vc, bt=bt[[s for s, _, _ in rows]].contiguous(),
                        ctx=torch.tensor([n for _, n, _ in rows], dtype=torch.int32), scale=1 / math.sqrt(D),
                        kv=kv or (1.0, 1.0), Hkv=Hkv, G=G, Hq=Hq, D=D, B=B, W=W, views=views)
    p.min_weight = check_weights(views, p.scale)
    return p


def decode_reference(p):
    return ref.paged_decode_attention(p.q.reshape(p.B, p.Hq, p.D), p.kc, p.vc, p.bt, p.ctx, p.scale, *p.kv,
                                      window=p.W).reshape(p.B, p.Hq * p.D)


# ------------------------------------------------------------------- decode, fused RoPE
def rope_probe(ctx, W, Hkv, G, D, seed):
    """attention_probe.rope_probe under a window W: the new token n - 1 comes from registers
    and is always visible; the cached keys lo .. n - 2 are probed at lo, lo + 1, n - 2 and in
    every visited block of the longest context, the far side at far_past(lo).  At W = 1 no
    cached key is visible: a head that points at n - 2 is a PAST target."""
    Hq = Hkv * G
    nb = lambda n: (n + BS - 1) // BS
    rows = []
    for n in ctx:
        lo = max(0, n - W)
        e = [(IN, n - 1), (PAST, DECOY), (PAST, n), (PAST, n + 1)] + [(PAST, t) for t in sorted(far_past(lo))]
        ins = {t for t in (lo, lo + 1, n - 2) if lo <= t <= n - 2}
        if n == max(ctx):
            ins |= {min(max(64 * b + (11 * b + 5) % 64, lo), n - 2) for b in range(lo // 64, nb(n - 1)) if lo <= n - 2}
        e += [(IN, t) for t in sorted(ins)]
        if lo <= n - 2:
            e += [(TWO, lo, n - 1), (TWO, n - 2, n - 1)]
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
    views = [_view(q_rot[b: b + 1], K, V, p_, torch.tensor([rows[b][0]]), W, torch.tensor(kind)[None],
                   torch.tensor(t)[None], torch.tensor(t2)[None])
             for b, (K, V, p_, kind, t, t2) in enumerate(parts)]
    p = SimpleNamespace(qkv=qkv.reshape(B, -1), pos=pos, slots=slots, cos_sin=cs, kc=kc, vc=vc, bt=bt, ctx=ctx_t,
                        scale=1 / math.sqrt(D), Hkv=Hkv, G=G, Hq=Hq, D=D, B=B, W=W, views=views)
    p.min_weight = check_weights(views, p.scale)
    return p


def rope_reference(p):
    """(attention output, K cache, V cache) of rope_and_cache followed by the windowed
    paged_decode_attention."""
    kr, vr, rows = p.kc.clone(), p.vc.clone(), p.qkv.clone()
    ref.rope_and_cache(rows, p.pos, p.cos_sin, p.slots, kr, vr, p.Hq, p.Hkv)
    out = ref.paged_decode_attention(rows[:, : p.Hq * p.D].reshape(p.B, p.Hq, p.D), kr, vr, p.bt, p.ctx, p.scale,
                                     window=p.W)
    return out.reshape(p.B, p.Hq * p.D), kr, vr


# ----------------------------------------------------------------------------- prefill
def prefill_probe(q_lens, prefix, W, Hkv, G, D, seed, kv=None):
    """ops.paged_prefill_attention inputs under a window W.  Head j of the query token at
    position p points at candidate (j + shift) % 4 of: p (IN), p + 1 (PAST), p - W + 1 (IN;
    key 0 while the window still reaches it) and p - W (PAST; p + 1 while there is no such
    key).  shift rotates with the token, except that the first token of a sequence and of
    every 128-row tile starts from the far side (shift 2) and the last token of a tile and
    of the sequence from the near side (shift 0)."""
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
        p = pre + i
        far_in = (p - W + 1).clamp(min=0)
        far_out = torch.where(p - W >= 0, p - W, p + 1)
        cand = torch.stack([p, p + 1, far_in, far_out], -1)                       # [ql, 1, 4]
        shift = i.clone()
        shift[0] = 2
        for r in range(ops.PREFILL_ROWS, ql * G, ops.PREFILL_ROWS):
            shift[r // G] = 2
            shift[(r - 1) // G] = 0
        shift[-1] = 0
        c = (j + shift) % 4                                                       # [ql, Hq]
        t = cand.expand(ql, Hq, 4).gather(-1, c[..., None])[..., 0]
        kind = torch.where((c == 1) | (c == 3), PAST, IN)
        qf = point(K[t, kvh_of[None, :].expand(ql, Hq)])
        qkv[a: a + ql, :Hq] = qf.to(torch.bfloat16)
        views.append(_view(qkv[a: a + ql, :Hq].float(), K, V, torch.arange(K.shape[0]), pre + i[:, 0] + 1, W, kind, t,
                           torch.full_like(t, -1)))
        a += ql
    p = SimpleNamespace(q=qkv.reshape(T, -1), kc=kc, vc=vc, bt=bt, q_start=torch.tensor(starts, dtype=torch.int32),
                        q_len=torch.tensor(q_lens, dtype=torch.int32), ctx=torch.tensor(ctx, dtype=torch.int32),
                        tiles=ops.prefill_tiles(q_lens, G, prefix), scale=1 / math.sqrt(D), kv=kv or (1.0, 1.0),
                        Hkv=Hkv, G=G, Hq=Hq, D=D, W=W, views=views)
    p.min_weight = check_weights(views, p.scale)
    return p


def prefill_reference(p):
    return ref.paged_prefill_attention(p.q, p.kc, p.vc, p.bt, p.q_start, p.q_len, p.ctx, p.Hq, p.scale, *p.kv,
                                       window=p.W)


# ------------------------------------------------------------------- the cases, built once
DECODE_CTX = [0, 1, 2, 63, 64, 65, 129, 300, 777]
DECODE_W = [1, 5, 64, 65, 200]
DECODE_SHAPES = [(64, 1), (128, 4), (128, 16)]
SPLITS = [(1, 4), (3, 1), (16, 1)]
FP8_SCALES = (0.25, 4.0)
WPP_W = 70
ROPE_CTX = ap.ROPE_CTX
ROPE_W = [1, 2, 65, 200]
PREFILL_LENS, PREFILL_PREFIX = [1, 17, 64, 130, 200], [0, 5, 64, 0, 300]
PREFILL_W = [1, 5, 64, 100, 129]
PREFILL_SHAPES = [(D, G) for D in (64, 128) for G in (1, 4, 8)]
_cache = {}


def _once(key, build, reference):
    if key not in _cache:
        p = build()
        p.expect = reference(p)
        _cache[key] = p
    return _cache[key]


def decode_case(D, G, W, kv=None):
    return _once(("decode", D, G, W, kv), lambda: decode_probe(DECODE_CTX, W, 2, G, D, seed=D + G + W, kv=kv),
                 decode_reference)


def wave_per_pair_case():
    ctx = torch.randint(1, 300, (256,), generator=torch.Generator().manual_seed(7)).tolist()
    return _once("wpp", lambda: decode_probe(ctx, WPP_W, 8, 4, 128, seed=3, ntables=32), decode_reference)


def rope_case(W):
    return _once(("rope", W), lambda: rope_probe(ROPE_CTX, W, 2, 4, 128, seed=5 + W), rope_reference)


def prefill_case(D, G, W, kv=None):
    return _once(("prefill", D, G, W, kv),
                 lambda: prefill_probe(PREFILL_LENS, PREFILL_PREFIX, W, 2, G, D, seed=10 + D + G + W, kv=kv),
                 prefill_reference)
