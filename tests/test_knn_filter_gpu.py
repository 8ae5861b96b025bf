"""Filtered kNN on the GPU: per-query row masks in knn_exact_kernel, knn_filter_kernel and
knn_filter_q256_kernel, and the store's filtered search on top of them.

The reference everywhere is an fp32 top-k of the same bf16 operands with the rejected
rows' scores set to -inf.  The shapes are the smallest that reach each kernel:
``sample_chunks=2`` over 5000 rows is 5 chunks (the last one partial), so the exact sample,
the thresholded main pass and the tail all run; Q = 130 takes the 256-query main pass with
one partial block."""
import functools

import numpy as np
import pytest
import torch

from langstream_amd import ops
from langstream_amd.engine.vector_store import VectorStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-3   # the tolerance of the unfiltered kNN tests (bf16 operands, fp32 accumulation)

# (N, Q, dim, k, sample_chunks)
CASES = [
    (5000, 3, 384, 20, 2),      # knn_exact_kernel + knn_filter_kernel, one partial query group
    (5000, 20, 384, 5, 2),
    (5000, 70, 384, 64, 2),     # two 64-query blocks of knn_filter_kernel
    (5000, 130, 384, 20, 2),    # knn_filter_q256_kernel, one partial 256-block
    (70000, 130, 384, 20, None),  # where an unfiltered search takes the group-max route
    (5000, 130, 128, 5, 2),
    (5000, 20, 768, 64, 2),
]
IDS = [f"N{n}-Q{q}-D{d}-k{k}" for n, q, d, k, _ in CASES]


@functools.lru_cache(maxsize=None)
def _data(N, Qn, D, dup=0):
    """(X, Q, fp32 scores [Q, N]) -- built once per shape, never modified."""
    g = torch.Generator().manual_seed(1000 + N + Qn + D + dup)
    X = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    if dup:
        X = X[torch.arange(N) % dup]
    X = X.to(DEV, torch.bfloat16)
    Q = torch.nn.functional.normalize(torch.randn(Qn, D, generator=g), dim=-1).to(DEV, torch.bfloat16)
    return X, Q, Q.float() @ X.float().t()


def _pack(adm):
    """bool [M, N] -> device int32 [M, 32 * ceil(N / 1024)] (little-endian bits, zero padding)."""
    adm = adm.cpu().numpy()
    M, N = adm.shape
    bits = np.zeros((M, (N + 1023) // 1024 * 1024), dtype=bool)
    bits[:, :N] = adm
    return torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view(np.int32).copy()).to(DEV)


def _per_query(adm, qmask):
    """bool [Q, N]: what each query may return."""
    qm = torch.as_tensor(qmask, device=adm.device)
    out = adm[qm.clamp_min(0)]
    out[qm < 0] = True
    return out


def _check(s, i, full, allowed, k):
    """scores = the reference's; every index admitted, carrying its score, at most once."""
    es, _ = full.masked_fill(~allowed, float("-inf")).topk(k, dim=1)
    have = es > float("-inf")
    assert torch.equal(i >= 0, have), "an entry is missing or padding is not (-inf, -1)"
    assert torch.equal(s == float("-inf"), ~have)
    z = torch.zeros_like(s)
    err = (torch.where(have, s, z) - torch.where(have, es, z)).abs().max().item()
    print("max score error", err)
    assert err < TOL
    il = i.clamp_min(0).long()
    assert allowed.gather(1, il)[have].all(), "a rejected row was returned"
    assert ((full.gather(1, il) - s).abs()[have] < TOL).all(), "an index does not carry its score"
    srt = torch.where(have, i, -1 - torch.arange(k, device=i.device, dtype=i.dtype)[None]).sort(dim=1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a row appears twice"


def _random_masks(N, Qn, frac, seed):
    """A different mask per query, every fourth query unfiltered."""
    g = torch.Generator().manual_seed(seed)
    adm = (torch.rand(Qn, N, generator=g) < frac).to(DEV)
    qmask = [-1 if q % 4 == 3 else q for q in range(Qn)]
    return adm, qmask


@pytest.mark.parametrize("frac", [0.5, 1 / 97])
@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_random_masks(N, Qn, D, k, sc, frac):
    X, Q, full = _data(N, Qn, D)
    adm, qmask = _random_masks(N, Qn, frac, N + Qn)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(adm), qmask=qmask)
    _check(s, i, full, _per_query(adm, qmask), k)


@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_all_ones_equals_unfiltered(N, Qn, D, k, sc):
    X, Q, _ = _data(N, Qn, D)
    s0, i0 = ops.knn_topk(X, Q, k, sample_chunks=sc)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(torch.ones(1, N, dtype=torch.bool)), qmask=[0] * Qn)
    assert torch.equal(s, s0) and torch.equal(i, i0)


@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_all_zeros_is_padding(N, Qn, D, k, sc):
    X, Q, _ = _data(N, Qn, D)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(torch.zeros(1, N, dtype=torch.bool)), qmask=[0] * Qn)
    assert (s == float("-inf")).all() and (i == -1).all()


@pytest.mark.parametrize("frac", [0.5, 1 / 97])
@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_sampled_equals_all_exact(N, Qn, D, k, sc, frac):
    X, Q, _ = _data(N, Qn, D)
    adm, qmask = _random_masks(N, Qn, frac, 7 * N + Qn)
    m = _pack(adm)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=m, qmask=qmask)
    s0, i0 = ops.knn_topk(X, Q, k, sample_chunks=0, mask=m, qmask=qmask)
    assert torch.equal(s, s0) and torch.equal(i, i0)


def _plants(N, sc):
    sample = (32 if sc is None else sc) * 1024
    return [0, 31, 32, 1023, 1024, sample, N - 1]


@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_probe_rows(N, Qn, D, k, sc):
    """A copy of a query scores ~1.0 against ~0.25 for the best random row, so one wrong
    mask bit moves the answer: plant j (rows 0, 31, 32, 1023, 1024, the first row after the
    sample, N - 1) holds a copy of query j % Q."""
    X0, Q, _ = _data(N, Qn, D)
    P = _plants(N, sc)
    X = X0.clone()
    for j, p in enumerate(P):
        X[p] = Q[j % Qn]
    full = Q.float() @ X.float().t()
    base = torch.rand(Qn, N, generator=torch.Generator().manual_seed(N + 3)) < 0.5
    base[:, P] = False
    base = base.to(DEV)
    qmask = list(range(Qn))
    # every plant's bit clear: none comes back, and the best score is a random row's
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(base), qmask=qmask)
    _check(s, i, full, base, k)
    assert not torch.isin(i, torch.tensor(P, device=DEV, dtype=i.dtype)).any()
    assert s[:, 0].max().item() < 0.6
    # exactly one plant's bit set per query: it comes first
    for t in range((len(P) + Qn - 1) // Qn):
        adm = base.clone()
        mine = {q: P[t * Qn + q] for q in range(Qn) if t * Qn + q < len(P)}
        for q, p in mine.items():
            adm[q, p] = True
        s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(adm), qmask=qmask)
        _check(s, i, full, adm, k)
        for q, p in mine.items():
            assert i[q, 0].item() == p and s[q, 0].item() > 0.9, (q, p, i[q, :3].tolist(), s[q, :3].tolist())
    # the only admitted rows lie in the last, partial chunk / entirely outside the sample
    for first in ((N - 1) // 1024 * 1024, P[5]):
        adm = torch.zeros(1, N, dtype=torch.bool, device=DEV)
        adm[:, first:] = True
        s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(adm), qmask=[0] * Qn)
        _check(s, i, full, adm.expand(Qn, N), k)
        assert (i[:, 0] >= first).all()
        assert i[(len(P) - 1) % Qn, 0].item() == N - 1   # the plant at N - 1 is admitted by both


@pytest.mark.parametrize("admit", ["k-1", "1"])
@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_fewer_than_k_admitted(N, Qn, D, k, sc, admit):
    X, Q, full = _data(N, Qn, D)
    n_adm = k - 1 if admit == "k-1" else 1
    g = torch.Generator().manual_seed(N + Qn + n_adm)
    adm = torch.zeros(Qn, N, dtype=torch.bool)
    for q in range(Qn):
        adm[q, torch.randperm(N, generator=g)[:n_adm]] = True
    adm = adm.to(DEV)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(adm), qmask=list(range(Qn)))
    _check(s, i, full, adm, k)
    assert (i[:, n_adm:] == -1).all() and (s[:, n_adm:] == float("-inf")).all()
    got = torch.zeros_like(adm)
    got.scatter_(1, i[:, :n_adm].long(), True)
    assert torch.equal(got, adm), "exactly the admitted rows come back"


@pytest.mark.parametrize("Qn", [20, 130])
def test_ties_take_the_k_round_fallback(Qn):
    """7 distinct rows: every chunk holds hundreds of equal scores, so the wave-sort fast
    path gives way to the K-round argmax, with rejected rows at -inf among them."""
    N, D, k = 5000, 384, 20
    X, Q, full = _data(N, Qn, D, dup=7)
    adm, qmask = _random_masks(N, Qn, 0.5, 77)
    m = _pack(adm)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=2, mask=m, qmask=qmask)
    _check(s, i, full, _per_query(adm, qmask), k)
    s0, i0 = ops.knn_topk(X, Q, k, sample_chunks=0, mask=m, qmask=qmask)
    assert torch.equal(s, s0) and torch.equal(i, i0)


def test_weak_threshold_overflows_and_reruns_exactly():
    """The construction of test_knn_topk_threshold_overflow_and_exact at 20k rows: rows get
    more similar to the queries further in, and the mask admits only the second half, so
    the 4-chunk sample holds no admitted row, the threshold stays -inf, the 10000 admitted
    rows overflow the candidate lists (capacity chunks * k = 400) and the search reruns
    exactly."""
    torch.manual_seed(51)
    N, D, k = 20_000, 384, 20
    q = torch.nn.functional.normalize(torch.randn(3, D), dim=-1)
    alpha = torch.linspace(0, 1, N).unsqueeze(1)
    X = torch.nn.functional.normalize(alpha * q[torch.arange(N) % 3] + 0.5 * torch.randn(N, D), dim=-1)
    X, Q = X.to(DEV, torch.bfloat16), q.to(DEV, torch.bfloat16)
    adm = torch.zeros(1, N, dtype=torch.bool, device=DEV)
    adm[:, N // 2:] = True
    s, i = ops.knn_topk(X, Q, k, sample_chunks=4, mask=_pack(adm), qmask=[0, 0, 0])
    _check(s, i, Q.float() @ X.float().t(), adm.expand(3, N), k)


def test_rejections():
    X, Q, _ = _data(5000, 3, 384)
    ok = _pack(torch.ones(2, 5000, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, mask=ok[:, :-32].contiguous(), qmask=[0, 0, 0])      # too narrow
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, mask=ok, qmask=[0, 2, 0])                            # out of range
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, mask=ok, qmask=[0, -2, 0])
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, mask=ok, qmask=[0, 0])                               # wrong length
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, mask=ok.long(), qmask=[0, 0, 0])                     # wrong dtype
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, mask=ok, qmask=torch.tensor([0.0, 0.0, 0.0]))


# ---------------------------------------------------------------------------- the store
def _store_expect(st, queries, k, pred):
    """Brute force over the store's own rows: ids of the top-k rows whose metadata pass."""
    n = len(st)
    sc = st._to_device_query(st._normalize_host(queries)).float() @ st._vecs[:n].float().t()
    ok = torch.tensor([pred(st._ids[r], st._meta[r]) for r in range(n)], device=DEV)
    es, ei = sc.masked_fill(~ok[None], float("-inf")).topk(min(k, n), dim=1)
    return [[(st._ids[r], v) for r, v in zip(ir, vr) if v > float("-inf")]
            for ir, vr in zip(ei.tolist(), es.tolist())]


def _same(res, exp):
    assert [len(r) for r in res] == [len(e) for e in exp]
    for r, e in zip(res, exp):
        for hit, (_, v) in zip(r, e):
            assert abs(hit["similarity"] - v) < TOL
        # near-ties within the tolerance may swap: compare as sets of ids above the cut
        cut = e[-1][1] + TOL if e else 0.0
        assert {h["id"] for h in r if h["similarity"] > cut} == {i for i, v in e if v > cut}


@pytest.mark.parametrize("compact_max", [0, 1 << 30], ids=["masked", "compact"])
def test_store_filter_follows_upserts_and_deletes(compact_max):
    torch.manual_seed(9)
    N, D, k = 3000, 384, 10
    st = VectorStore(D, device=DEV)
    st.compact_max = compact_max
    vec = torch.randn(N, D)
    st.upsert(list(range(N)), vec, [{"tenant": "ab"[r % 2], "n": r % 5} for r in range(N)])
    qs = torch.randn(6, D)
    flt = {"tenant": "b", "n": {"$in": [1, 3]}}
    pred = lambda i, md: md.get("tenant") == "b" and md.get("n") in (1, 3)   # noqa: E731
    _same(st.search(qs, k, filter=flt), _store_expect(st, qs, k, pred))
    # overwrite some admitted rows out of the filter, add new admitted rows at the queries
    st.upsert([1, 3, 11], vec[[1, 3, 11]], [{"tenant": "a"}] * 3)
    st.upsert([f"new{j}" for j in range(6)], qs, [{"tenant": "b", "n": 1}] * 6)
    res = st.search(qs, k, filter=flt)
    _same(res, _store_expect(st, qs, k, pred))
    assert [r[0]["id"] for r in res] == [f"new{j}" for j in range(6)]
    # a delete that renumbers: tail rows (the new ones among them) move into the holes
    st.delete(list(range(0, 600, 3)))
    res = st.search(qs, k, filter=flt)
    _same(res, _store_expect(st, qs, k, pred))
    assert [r[0]["id"] for r in res] == [f"new{j}" for j in range(6)]
    assert all(h["tenant"] == "b" and h["n"] in (1, 3) for r in res for h in r)
    assert st.filter_stats["compact" if compact_max else "masked"] >= 3
    assert st.filter_stats["masked" if compact_max else "compact"] == 0


def test_store_routes_agree():
    """Both sides of compact_max: the gathered search and the masked kernels return the
    same rows with the same scores, per-query filters and an unfiltered query included."""
    torch.manual_seed(10)
    N, D, k = 6000, 384, 20
    st = VectorStore(D, device=DEV)
    st.upsert(list(range(N)), torch.randn(N, D), [{"lang": ["en", "de", "fr"][r % 3], "n": r % 50} for r in range(N)])
    qs = torch.randn(5, D)
    filters = [{"lang": "en"}, None, {"n": 7}, {"lang": {"$ne": "en"}}, {"$or": [{"n": 1}, {"lang": "fr"}]}]
    out = {}
    for cm in (0, 150, 1 << 30):   # all masked; n == 7 (120 rows) compact, the rest masked; all compact
        st.compact_max = cm
        out[cm] = [[(h["id"], h["similarity"]) for h in r] for r in st.search(qs, k, filter=filters)]
    assert out[0] == out[150] == out[1 << 30]
    assert all(len(r) == k for r in out[0])
