"""Dot-product and Euclidean metrics on the GPU: the per-row f32 bias in knn_exact_kernel,
knn_filter_kernel and knn_filter_q256_kernel (score = dot + bias[row]), and the store's
``dot-product`` / ``euclidean`` collections on top of it.

The reference everywhere is an fp32 top-k of the same bf16 operands with the same bias added
in fp32.  Rows and queries are unit vectors scaled by a factor from [0.5, 2] and rounded to
bf16: under ``q.x - |x|^2 / 2`` the top-k shares no row with the dot-product top-k and few
with the cosine top-k, so a kernel that drops, shifts or mis-indexes the bias cannot pass.

Tolerance: the unit-vector kNN tests allow 2e-3 on a score; here max|q| * max|x| = 4, so
scores compare within 8e-3 and the store's d^2 = |q|^2 - 2 * score within twice that.  The
shapes are those of test_knn_filter_gpu.py (the smallest that reach each kernel) plus
N = 4999, where the four-wide bias read meets the end of the bias."""
import functools

import numpy as np
import pytest
import torch

from langstream_amd import ops
from langstream_amd.engine.vector_store import VectorStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 8e-3      # 2e-3 of the unit-vector tests x max|q| * max|x| = 4
TOL_D2 = 2 * TOL

# (N, Q, dim, k, sample_chunks)
CASES = [
    (5000, 3, 384, 20, 2),      # knn_exact_kernel + knn_filter_kernel, one partial query group
    (5000, 20, 384, 5, 2),
    (5000, 70, 384, 64, 2),     # two 64-query blocks of knn_filter_kernel
    (5000, 130, 384, 20, 2),    # knn_filter_q256_kernel, one partial 256-block
    (70000, 130, 384, 20, None),  # the group-max route (MODE 2 + MODE 1)
    (5000, 130, 128, 5, 2),
    (5000, 20, 768, 64, 2),
    (4999, 20, 384, 20, 2),     # N not a multiple of 4: the four-wide bias read at the tail
]
IDS = [f"N{n}-Q{q}-D{d}-k{k}" for n, q, d, k, _ in CASES]


def _scaled(n, D, g):
    v = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=-1)
    return v * (0.5 + 1.5 * torch.rand(n, 1, generator=g))


def _bias(X):
    """-|x|^2 / 2 of the bf16 rows, in fp32."""
    return X.float().pow(2).sum(-1).mul(-0.5).contiguous()


@functools.lru_cache(maxsize=None)
def _data(N, Qn, D, dup=0):
    """(X, Q, bias, fp32 biased scores [Q, N]) -- built once per shape, never modified."""
    g = torch.Generator().manual_seed(2000 + N + Qn + D + dup)
    X = _scaled(N, D, g)
    if dup:
        X = X[torch.arange(N) % dup]
    X = X.to(DEV, torch.bfloat16)
    Q = _scaled(Qn, D, g).to(DEV, torch.bfloat16)
    b = _bias(X)
    return X, Q, b, Q.float() @ X.float().t() + b[None]


def _pack(adm):
    adm = adm.cpu().numpy()
    M, N = adm.shape
    bits = np.zeros((M, (N + 1023) // 1024 * 1024), dtype=bool)
    bits[:, :N] = adm
    return torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view(np.int32).copy()).to(DEV)


def _check(s, i, full, k, allowed=None):
    """scores = the reference's; every index admitted, carrying its score, at most once."""
    if allowed is None:
        allowed = torch.ones_like(full, dtype=torch.bool)
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


@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_bias_equals_reference(N, Qn, D, k, sc):
    X, Q, b, full = _data(N, Qn, D)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, bias=b)
    _check(s, i, full, k)


@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_zero_bias_equals_unbiased(N, Qn, D, k, sc):
    X, Q, _, _ = _data(N, Qn, D)
    s0, i0 = ops.knn_topk(X, Q, k, sample_chunks=sc)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, bias=torch.zeros(N, device=DEV))
    assert torch.equal(s, s0) and torch.equal(i, i0)


@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_sampled_equals_all_exact(N, Qn, D, k, sc):
    X, Q, b, _ = _data(N, Qn, D)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, bias=b)
    s0, i0 = ops.knn_topk(X, Q, k, sample_chunks=0, bias=b)
    assert torch.equal(s, s0) and torch.equal(i, i0)


def _random_masks(N, Qn, frac, seed):
    """A different mask per query, every fourth query unfiltered."""
    g = torch.Generator().manual_seed(seed)
    adm = (torch.rand(Qn, N, generator=g) < frac).to(DEV)
    qmask = [-1 if q % 4 == 3 else q for q in range(Qn)]
    return adm, qmask


def _per_query(adm, qmask):
    qm = torch.as_tensor(qmask, device=adm.device)
    out = adm[qm.clamp_min(0)]
    out[qm < 0] = True
    return out


@pytest.mark.parametrize("frac", [0.5, 1 / 97])
@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_bias_with_random_masks(N, Qn, D, k, sc, frac):
    X, Q, b, full = _data(N, Qn, D)
    adm, qmask = _random_masks(N, Qn, frac, N + Qn)
    m = _pack(adm)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=m, qmask=qmask, bias=b)
    _check(s, i, full, k, _per_query(adm, qmask))
    s0, i0 = ops.knn_topk(X, Q, k, sample_chunks=0, mask=m, qmask=qmask, bias=b)
    assert torch.equal(s, s0) and torch.equal(i, i0)


@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_bias_with_fewer_than_k_admitted(N, Qn, D, k, sc):
    X, Q, b, full = _data(N, Qn, D)
    n_adm = max(1, k - 1)
    g = torch.Generator().manual_seed(N + Qn + n_adm)
    adm = torch.zeros(Qn, N, dtype=torch.bool)
    for q in range(Qn):
        adm[q, torch.randperm(N, generator=g)[:n_adm]] = True
    adm = adm.to(DEV)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, mask=_pack(adm), qmask=list(range(Qn)), bias=b)
    _check(s, i, full, k, adm)
    if n_adm < k:
        assert (i[:, n_adm:] == -1).all() and (s[:, n_adm:] == float("-inf")).all()
    got = torch.zeros_like(adm)
    got.scatter_(1, i[:, :n_adm].long(), True)
    assert torch.equal(got, adm), "exactly the admitted rows come back"


def _plants(N, sc):
    sample = (32 if sc is None else sc) * 1024
    return [0, 31, 32, 1023, 1024, sample, N - 1]


@pytest.mark.parametrize("swap", [False, True], ids=["copy-at-plant", "double-at-plant"])
@pytest.mark.parametrize("N,Qn,D,k,sc", CASES, ids=IDS)
def test_probe_rows(N, Qn, D, k, sc, swap):
    """Plant j (rows 0, 31, 32, 1023, 1024, the first row after the sample, N - 1) holds a copy
    of query j % Q and the row two further (two before at N - 1) holds twice the query, or the
    other way round (``swap``); both are exact in bf16.  Under the Euclidean bias the copy is
    first with score |q|^2 / 2 (the doubled row scores 0); with no bias the doubled row is
    first; with normalised rows the two tie and the lower row wins.  One wrong bias slot at
    either position changes ``i[:, 0]``."""
    X0, Q, _, _ = _data(N, Qn, D)
    P = _plants(N, sc)
    qn2 = Q.float().pow(2).sum(-1)
    for t in range((len(P) + Qn - 1) // Qn):
        X = X0.clone()
        copy, dbl = {}, {}
        for q in range(Qn):
            if t * Qn + q >= len(P):
                break
            p = P[t * Qn + q]
            o = p + 2 if p + 2 < N else p - 2
            copy[q], dbl[q] = (o, p) if swap else (p, o)
            X[copy[q]] = Q[q]
            X[dbl[q]] = (2 * Q[q].float()).to(torch.bfloat16)
        b = _bias(X)
        full = Q.float() @ X.float().t()
        s, i = ops.knn_topk(X, Q, k, sample_chunks=sc, bias=b)
        _check(s, i, full + b[None], k)
        for q in copy:
            assert i[q, 0].item() == copy[q], (q, copy[q], dbl[q], i[q, :3].tolist(), s[q, :3].tolist())
            assert abs(s[q, 0].item() - 0.5 * qn2[q].item()) < TOL
        s, i = ops.knn_topk(X, Q, k, sample_chunks=sc)
        for q in copy:
            assert i[q, 0].item() == dbl[q] and abs(s[q, 0].item() - 2 * qn2[q].item()) < 2 * TOL
        Xn = torch.nn.functional.normalize(X.float(), dim=-1).to(torch.bfloat16)
        s, i = ops.knn_topk(Xn, Q, k, sample_chunks=sc)
        for q in copy:
            assert torch.equal(Xn[copy[q]], Xn[dbl[q]])
            assert i[q, :2].tolist() == sorted([copy[q], dbl[q]]) and s[q, 0].item() == s[q, 1].item()


@pytest.mark.parametrize("Qn", [20, 130])
def test_biased_ties_take_the_k_round_fallback(Qn):
    """7 distinct rows (and so 7 distinct biases): every chunk holds hundreds of equal biased
    scores, so the wave-sort fast path gives way to the K-round argmax."""
    N, D, k = 5000, 384, 20
    X, Q, b, full = _data(N, Qn, D, dup=7)
    s, i = ops.knn_topk(X, Q, k, sample_chunks=2, bias=b)
    _check(s, i, full, k)
    s0, i0 = ops.knn_topk(X, Q, k, sample_chunks=0, bias=b)
    assert torch.equal(s, s0) and torch.equal(i, i0)


def test_rejections():
    X, Q, b, _ = _data(5000, 3, 384)
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, bias=b[:-1].contiguous())            # wrong length
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, bias=b.double())                     # wrong dtype
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, bias=b.cpu())                        # wrong device
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, bias=torch.zeros(10000, device=DEV)[::2])   # non-contiguous
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 5, bias=b, _ablate=1)


def test_unaligned_bias_view():
    """A contiguous view that starts off a 16-byte boundary is accepted (and copied)."""
    X, Q, b, full = _data(5000, 3, 384)
    pad = torch.zeros(5001, device=DEV)
    pad[1:] = b
    s, i = ops.knn_topk(X, Q, 20, sample_chunks=2, bias=pad[1:])
    _check(s, i, full, 20)


# ---------------------------------------------------------------------------- the store
def _store_expect(st, queries, k, pred=None):
    """Brute force over the store's own rows: (id, kernel score, d^2) of the top-k."""
    n = len(st)
    X = st._vecs[:n].float()
    q = st._to_device_query(st._prepare_host(queries)).float()
    sc = q @ X.t()
    if st.metric == "euclidean":
        sc = sc - 0.5 * X.pow(2).sum(-1)[None]
    if pred is not None:
        ok = torch.tensor([pred(st._ids[r], st._meta[r]) for r in range(n)], device=DEV)
        sc = sc.masked_fill(~ok[None], float("-inf"))
    es, ei = sc.topk(min(k, n), dim=1)
    qn2 = q.pow(2).sum(-1).tolist()
    return [[(st._ids[r], v, max(0.0, n2 - 2 * v)) for r, v in zip(ir, vr) if v > float("-inf")]
            for ir, vr, n2 in zip(ei.tolist(), es.tolist(), qn2)]


def _same(st, res, exp):
    assert [len(r) for r in res] == [len(e) for e in exp]
    for r, e in zip(res, exp):
        if st.metric == "euclidean":
            worst = 0.0
            for hit, (_, _, d2) in zip(r, e):
                worst = max(worst, abs(hit["distance"] ** 2 - d2))
                assert abs(hit["distance"] ** 2 - d2) < TOL_D2
                assert abs(hit["similarity"] - 1.0 / (1.0 + hit["distance"] ** 2)) < 1e-6
            print("max d2 error", worst)
            assert [h["distance"] for h in r] == sorted(h["distance"] for h in r)
            # near-ties within the tolerance may swap: compare as sets of ids below the cut
            cut = e[-1][2] - TOL_D2 if e else 0.0
            assert {h["id"] for h in r if h["distance"] ** 2 < cut - TOL_D2} <= {i for i, _, d2 in e if d2 < cut}
            assert {i for i, _, d2 in e if d2 < cut - TOL_D2} <= {h["id"] for h in r if h["distance"] ** 2 < cut}
        else:
            for hit, (_, v, _) in zip(r, e):
                assert abs(hit["similarity"] - v) < TOL and "distance" not in hit
            cut = e[-1][1] + TOL if e else 0.0
            assert {h["id"] for h in r if h["similarity"] > cut + TOL} <= {i for i, v, _ in e if v > cut}
            assert {i for i, v, _ in e if v > cut + TOL} <= {h["id"] for h in r if h["similarity"] > cut}


@pytest.mark.parametrize("metric", ["euclidean", "dot-product"])
def test_store_metric_follows_upserts_deletes_and_growth(metric):
    g = torch.Generator().manual_seed(11)
    N, D, k = 3000, 384, 10
    st = VectorStore(D, device=DEV, metric=metric)
    assert st.metric == metric
    vec = _scaled(N, D, g)
    st.upsert(list(range(N)), vec, [{"tenant": "ab"[r % 2]} for r in range(N)])
    qs = _scaled(6, D, g)
    _same(st, st.search(qs, k), _store_expect(st, qs, k))
    # overwrite rows with vectors of other norms (a duplicate id in the batch: the last wins)
    ids = [5, 17, 5, 2999, 1024]
    st.upsert(ids, 3.0 * _scaled(len(ids), D, g), [{"tenant": "a"}] * len(ids))
    st.upsert(list(range(100, 400)), 0.25 * vec[100:400], [{"tenant": "b"}] * 300)
    _same(st, st.search(qs, k), _store_expect(st, qs, k))
    # stored copies of the queries come first, at distance ~0
    st.upsert([f"new{j}" for j in range(6)], qs, [{"tenant": "b"}] * 6)
    if metric == "euclidean":
        res = st.search(qs, k)
        assert [r[0]["id"] for r in res] == [f"new{j}" for j in range(6)]
        assert all(r[0]["distance"] < 0.05 for r in res)
    # a delete that renumbers: tail rows (the new ones among them) move into the holes
    st.delete(list(range(0, 600, 3)))
    res = st.search(qs, k)
    _same(st, res, _store_expect(st, qs, k))
    if metric == "euclidean":
        assert [r[0]["id"] for r in res] == [f"new{j}" for j in range(6)]
    # growth past the capacity the rows were written into
    cap = st._vecs.shape[0]
    more = cap - len(st) + 100
    st.upsert([f"g{j}" for j in range(more)], _scaled(more, D, g), [{"tenant": "a"}] * more)
    assert st._vecs.shape[0] > cap
    _same(st, st.search(qs, k), _store_expect(st, qs, k))
    # filtered: the masked kernels and the gathered rows return identical hits
    flt = {"tenant": "b"}
    out = {}
    for cm in (0, 150, 1 << 30):
        st.compact_max = cm
        res = st.search(qs, k, filter=[flt, None, {"id": {"$in": [f"g{j}" for j in range(120)]}}, flt, flt, None])
        out[cm] = [[(h["id"], h["similarity"], h.get("distance")) for h in r] for r in res]
    assert out[0] == out[150] == out[1 << 30]
    st.compact_max = 0
    _same(st, st.search(qs, k, filter=flt), _store_expect(st, qs, k, lambda i, md: md.get("tenant") == "b"))
    # vector() returns the stored, un-normalised row
    j = 3
    assert torch.allclose(torch.tensor(st.vector(f"new{j}")), qs[j].to(torch.bfloat16).float())
