"""Filtered vector search on the CPU: the filter compiler against a plain Python evaluation
of the same filter, the masked reference top-k, the store, the local JSON and SQL data
sources, and the sharded service over gloo."""
import json
import os
import socket
import sqlite3

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from langstream_amd.engine.vector_store import IdSet, VectorStore, VectorStoreRegistry, check_filter, pack_mask
from langstream_amd.ops import reference as ref


def _spawn(fn, world=2):
    """Run ``fn(rank, world, port, queue)`` in ``world`` fresh processes; rank 0's answer."""
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=fn, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = q.get(timeout=240)
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return out


# ---------------------------------------------------------------- the filter compiler
def _py_eval(flt, row_id, md) -> bool:
    """The grammar, evaluated the slow way on one row."""
    def field(name):
        if name == "id":
            return True, row_id
        return name in md, md.get(name)

    for key, val in flt.items():
        if key == "$and":
            ok = all(_py_eval(f, row_id, md) for f in val)
        elif key == "$or":
            ok = any(_py_eval(f, row_id, md) for f in val)
        elif isinstance(val, dict) and any(str(o).startswith("$") for o in val):
            ok = True
            for op, arg in val.items():
                present, v = field(key)
                if op == "$eq":
                    ok &= present and v == arg
                elif op == "$ne":
                    ok &= not (present and v == arg)
                elif op == "$in":
                    ok &= present and any(v == a for a in arg)
                else:
                    assert op == "$nin"
                    ok &= not (present and any(v == a for a in arg))
        else:
            present, v = field(key)
            ok = present and v == val
        if not ok:
            return False
    return True


FILTERS = [
    {"tenant": "b"},
    {"tenant": "b", "n": 3},
    {"n": {"$eq": 2}},
    {"n": {"$ne": 2}},
    {"lang": {"$ne": "en"}},                 # lang is missing on some rows: they match
    {"lang": {"$in": ["en", "fr"]}},
    {"lang": {"$nin": ["en", "fr"]}},
    {"lang": None},                          # an explicit null, not a missing key
    {"n": {"$in": []}},
    {"n": {"$in": [1, 2], "$ne": 2}},
    {"tags": ["x", "y"]},                    # unhashable values compare row by row
    {"tags": {"$ne": ["x", "y"]}},
    {"id": "r7"},
    {"id": {"$in": ["r1", "r2", "gone", 5]}},
    {"id": {"$nin": ["r1"]}, "tenant": "a"},
    {"$or": [{"tenant": "a", "n": 0}, {"lang": "de"}]},
    {"$and": [{"n": {"$in": [0, 1, 2]}}, {"$or": [{"lang": "en"}, {"tenant": "b"}]}]},
    {"$or": []},
    {"nosuchfield": 1},
    {"nosuchfield": {"$ne": 1}},
    {"flag": True},                          # True == 1 in Python and in the codes alike
]


def _meta(r):
    md = {"tenant": "ab"[r % 2], "n": r % 5}
    if r % 3:
        md["lang"] = ["en", "de", "fr", None][r % 4]
    if r % 7 == 0:
        md["tags"] = ["x", "y"] if r % 2 else ["z"]
    if r % 11 == 0:
        md["flag"] = [True, 1, 2][r % 3]
    return md


def _compare(st):
    for flt in FILTERS:
        check_filter(flt)
        with st.lock:
            got = st._admitted(flt)
        want = np.array([_py_eval(flt, st._ids[r], st._meta[r]) for r in range(len(st))], dtype=bool)
        assert np.array_equal(got, want), flt


def test_filter_compiler_matches_python_evaluation():
    st = VectorStore(8, device="cpu")
    g = torch.Generator().manual_seed(1)
    N = 400
    st.upsert([f"r{r}" for r in range(N)] + [5], torch.randn(N + 1, 8, generator=g), [_meta(r) for r in range(N + 1)])
    _compare(st)                              # builds every code column
    # overwrites change values, add and drop keys; new rows append
    st.upsert([f"r{r}" for r in range(0, 60, 2)], torch.randn(30, 8, generator=g), [_meta(r + 1) for r in range(0, 60, 2)])
    st.upsert([f"s{r}" for r in range(50)], torch.randn(50, 8, generator=g),
              [{"tenant": "c", "lang": "it", "tags": {"k": r}} for r in range(50)])
    _compare(st)
    # deletes move tail rows into the holes: the columns move with them
    st.delete([f"r{r}" for r in range(3, 200, 3)] + ["s49", 5])
    _compare(st)
    st.upsert(["r3", "late"], torch.randn(2, 8, generator=g), [{"n": 2}, {"lang": "fr", "n": 2}])
    _compare(st)


@pytest.mark.parametrize("flt,op", [({"n": {"$gt": 3}}, "$gt"), ({"n": {"$lte": 3}}, "$lte"),
                                    ({"$not": {"n": 1}}, "$not"), ({"$and": [{"n": {"$regex": "x"}}]}, "$regex"),
                                    ({"n": {"$in": 3}}, "$in"), ({"$or": {"n": 1}}, "$or")])
def test_unknown_operators_raise(flt, op):
    st = VectorStore(8, device="cpu")
    st.upsert([1], [[1.0] * 8], [{"n": 1}])
    with pytest.raises(ValueError, match=r"\%s" % op):
        st.search([[1.0] * 8], 1, filter=flt)


# ---------------------------------------------------------------- reference and store
def test_reference_topk_masked():
    g = torch.Generator().manual_seed(2)
    N, Qn, k = 2500, 5, 6
    X, Q = torch.randn(N, 16, generator=g), torch.randn(Qn, 16, generator=g)
    adm = torch.rand(3, N, generator=g) < 0.3
    adm[2] = False
    adm[2, [5, 2499]] = True                 # fewer than k admitted
    mask = torch.from_numpy(np.stack([pack_mask(a.numpy()) for a in adm]))
    assert mask.shape == (3, 32 * 3) and mask.dtype == torch.int32
    qmask = [0, 1, -1, 2, 0]
    s, i = ref.knn_topk(X, Q, k, mask, qmask)
    full = Q @ X.t()
    for q, m in enumerate(qmask):
        ok = adm[m] if m >= 0 else torch.ones(N, dtype=torch.bool)
        es, ei = full[q].masked_fill(~ok, float("-inf")).topk(k)
        n = int(min(k, ok.sum()))
        assert torch.equal(s[q, :n], es[:n]) and torch.equal(i[q, :n].long(), ei[:n])
        assert (s[q, n:] == float("-inf")).all() and (i[q, n:] == -1).all()
    assert i[3, :2].tolist() in ([5, 2499], [2499, 5])
    s0, i0 = ref.knn_topk(X, Q, k)
    assert torch.equal(s[2], s0[2]) and torch.equal(i[2], i0[2])


def _brute(st, queries, k, flt):
    qn = st._to_device_query(st._normalize_host(queries)).float()
    sc = qn @ st._vecs[: len(st)].float().t()
    out = []
    for q in range(sc.shape[0]):
        f = flt[q] if isinstance(flt, list) else flt
        ok = torch.tensor([f is None or _py_eval(f, st._ids[r], st._meta[r]) for r in range(len(st))])
        es, ei = sc[q].masked_fill(~ok, float("-inf")).topk(min(k, len(st)))
        out.append([st._ids[r] for r, v in zip(ei.tolist(), es.tolist()) if v > float("-inf")])
    return out


@pytest.mark.parametrize("compact_max", [0, 1 << 30], ids=["masked", "compact"])
def test_cpu_store_filters_single_and_per_query(compact_max):
    st = VectorStore(24, device="cpu")
    st.compact_max = compact_max
    g = torch.Generator().manual_seed(3)
    N = 1500
    st.upsert([f"r{r}" for r in range(N)], torch.randn(N, 24, generator=g), [_meta(r) for r in range(N)])
    qs = torch.randn(4, 24, generator=g)
    one = {"tenant": "b", "lang": {"$in": ["en", "de"]}}
    assert [[h["id"] for h in r] for r in st.search(qs, 7, filter=one)] == _brute(st, qs, 7, one)
    per = [None, {"n": 4}, {"id": {"$in": ["r3", "r9", "r12"]}}, {"$or": [{"tags": ["z"]}, {"flag": 2}]}]
    res = st.search(qs, 7, filter=per, with_vectors=True)
    assert [[h["id"] for h in r] for r in res] == _brute(st, qs, 7, per)
    assert len(res[2]) == 3 and all(len(h["vector"]) == 24 for r in res for h in r)
    # an IdSet resolves ids under the same lock as the search, unknown ids admit nothing
    res = st.search(qs[:1], 7, filter=IdSet(["r5", "r1400", "nope"]))
    assert sorted(h["id"] for h in res[0]) == ["r1400", "r5"]
    # the cached mask does not outlive a mutation
    st.delete(["r3"])
    st.upsert(["fresh"], qs[2:3], [{"n": 4}])
    res = st.search(qs, 7, filter=per)
    assert [[h["id"] for h in r] for r in res] == _brute(st, qs, 7, per)
    assert sorted(h["id"] for h in res[2]) == ["r12", "r9"]
    with pytest.raises(ValueError):
        st.search(qs, 7, filter=[one])       # one filter per query, or one for all


def test_mask_cache_hits_until_a_mutation():
    st = VectorStore(8, device="cpu")
    st.upsert(list(range(50)), torch.randn(50, 8), [{"n": r % 2} for r in range(50)])
    for _ in range(3):
        st.search(torch.randn(2, 8), 3, filter=[{"n": 1}, {"n": 1}])
    assert st.filter_stats["mask_builds"] == 1
    st.upsert([7], torch.randn(1, 8), [{"n": 0}])
    st.search(torch.randn(2, 8), 3, filter={"n": 1})
    assert st.filter_stats["mask_builds"] == 2


# ---------------------------------------------------------------- the local data source
@pytest.fixture
def registry():
    VectorStoreRegistry.reset()
    yield VectorStoreRegistry
    VectorStoreRegistry.reset()


def _tenant_store(registry):
    """2000 rows; the 10 rows of tenant b are the 10 WORST matches of the query."""
    g = torch.Generator().manual_seed(4)
    N, D = 2000, 32
    query = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    vecs = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    order = (vecs @ query).argsort()          # ascending similarity
    meta = [{"tenant": "a", "lang": ["en", "de"][r % 2]} for r in range(N)]
    for r in order[:10].tolist():
        meta[r] = {"tenant": "b", "lang": "en"}
    st = registry.get("docs", D, device="cpu", persist=False)
    st.upsert([f"d{r}" for r in range(N)], vecs, meta)
    return st, query, [f"d{r}" for r in order[:10].tolist()]


def test_local_datasource_selective_filter_returns_k(registry):
    from langstream_amd.agents.vector.datasources import LocalVectorDataSource
    st, query, worst = _tenant_store(registry)
    ds = LocalVectorDataSource({"collection-name": "docs"})
    rows = ds.fetch_data({"vector": query.tolist(), "top-k": 5, "filter": {"tenant": "b"}}, [])
    assert [r["id"] for r in rows] == worst[::-1][:5]      # best of the ten worst, in order
    assert all(r["tenant"] == "b" for r in rows)


def test_local_datasource_batch_mixes_filters(registry):
    from langstream_amd.agents.vector.datasources import LocalVectorDataSource
    st, query, _ = _tenant_store(registry)
    ds = LocalVectorDataSource({"collection-name": "docs"})
    g = torch.Generator().manual_seed(5)
    qs = torch.randn(8, 32, generator=g).tolist()
    flts = [{"tenant": "b"}, {"lang": "de"}, None, {"tenant": "a", "lang": {"$ne": "de"}}] * 2
    text = '{"vector": ?, "top-k": 6, "filter": ?}'
    batch = ds.fetch_data_batch(text, [[v, f or {}] for v, f in zip(qs, flts)])
    calls0 = st.filter_stats["masked"] + st.filter_stats["compact"]
    single = [ds.fetch_data(text, [v, f or {}]) for v, f in zip(qs, flts)]
    assert [[r["id"] for r in rows] for rows in batch] == [[r["id"] for r in rows] for rows in single]
    assert all(len(rows) == 6 for rows in batch)
    assert all(r["tenant"] == "b" for r in batch[0]) and all(r["lang"] == "de" for r in batch[1])
    assert calls0 >= 1 and st.filter_stats["mask_builds"] == 3      # three filters, built once each


# ---------------------------------------------------------------- SQL with a WHERE clause
def test_sqlite_where_knn_equals_sqlite_order(registry, tmp_path):
    from langstream_amd.agents.vector.datasources import SqliteDataSource, _cosine
    path = str(tmp_path / "docs.db")
    ds = SqliteDataSource({"url": f"jdbc:sqlite:{path}"})
    ds.script(["CREATE TABLE docs (name TEXT, lang TEXT, n INTEGER, v TEXT)"])
    g = torch.Generator().manual_seed(6)
    D, N = 16, 300
    q = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    noise = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    # cosine to the query falls by ~0.006 per row: well separated at bf16 precision
    for r in range(N):
        c = 0.95 - 0.006 * r
        v = c * q + (1 - c * c) ** 0.5 * torch.nn.functional.normalize(noise[r] - (noise[r] @ q) * q, dim=0)
        ds.execute_statement("INSERT INTO docs (name, lang, n, v) VALUES (?, ?, ?, ?)", None,
                             [f"doc{r}", ["en", "de", "fr"][r % 3], r % 10, v.tolist()])
    plain = sqlite3.connect(path)                      # a connection without a mirror
    plain.create_function("cosine_similarity", 2, _cosine)
    for where, params in [("WHERE lang = ?", ["de"]), ("WHERE lang = ? AND n > ?", ["fr", 6]),
                          ("WHERE n = ?", [1234]), ("WHERE name IN (?, ?)", ["doc200", "doc7"])]:
        sql = f"SELECT rowid AS rid, name, lang FROM docs {where} ORDER BY cosine_similarity(v, ?) DESC LIMIT 8"
        want = plain.execute(sql, params + [json.dumps(q.tolist())]).fetchall()
        got = ds.fetch_data(sql, params + [q.tolist()])
        assert [(r["rid"], r["name"], r["lang"]) for r in got] == [tuple(r) for r in want], where
    st = VectorStoreRegistry.get(ds._store_name("docs", "v"), persist=False)
    assert st.filter_stats["mask_builds"] >= 3         # the WHERE queries ran on the mirror
    plain.close()


# ---------------------------------------------------------------- the sharded service
def _corpus():
    g = torch.Generator().manual_seed(12)
    vecs = torch.randn(600, 48, generator=g)
    queries = torch.randn(8, 48, generator=g)
    meta = [{"lang": ["en", "de", "fr"][i % 3], "n": i % 7, "half": int(i % 2)} for i in range(600)]
    return vecs, queries, meta


# "half": 1 lives on rank 1 only (rows i % 2 == rank)
SHARD_FILTERS = [{"lang": "de"}, {"half": 1}, None, {"$or": [{"n": 3}, {"lang": "fr"}]},
                 {"half": 1, "n": {"$in": [0, 6]}}, {"id": {"$in": ["d10", "d11", "d301"]}}, {"lang": "de"}, None]


def _sharded_filter_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from langstream_amd.engine import dist_knn
        vecs, queries, meta = _corpus()
        rows = [i for i in range(vecs.shape[0]) if i % world == rank]
        VectorStoreRegistry.get("docs", 48, device="cpu").upsert(
            [f"d{i}" for i in rows], vecs[rows].tolist(), [meta[i] for i in rows])
        svc = dist_knn.start(device="cpu")
        mine = list(range(rank, queries.shape[0], world))
        # one request with a filter per query, then single-filter requests
        batch = svc.search("docs", queries[mine].tolist(), 9, filter=[SHARD_FILTERS[i] for i in mine]).result(60)
        res = {i: r for i, r in zip(mine, batch)}
        solo = {i: svc.search("docs", queries[i:i + 1].tolist(), 9, filter=SHARD_FILTERS[i]).result(60)[0]
                for i in mine}
        bad = svc.search("docs", queries[:1].tolist(), 3, filter={"n": {"$gt": 1}})
        err = type(bad.exception(60)).__name__
        gathered = [None] * world
        dist.all_gather_object(gathered, (res, solo, err))
        dist_knn.stop()
        VectorStoreRegistry.reset()
        if rank == 0:
            q.put(gathered)
    finally:
        dist.destroy_process_group()


def test_sharded_filtered_search_equals_single_store():
    gathered = _spawn(_sharded_filter_worker, 2)
    vecs, queries, meta = _corpus()
    single = VectorStore(48, device="cpu")
    single.upsert([f"d{i}" for i in range(600)], vecs.tolist(), meta)
    res, solo = {}, {}
    for r, s, err in gathered:
        res.update(r)
        solo.update(s)
        assert err == "ValueError"
    for i in range(queries.shape[0]):
        want = single.search(queries[i:i + 1].tolist(), 9, filter=SHARD_FILTERS[i])[0]
        assert len(want) == (3 if i == 5 else 9)
        for got in (res[i], solo[i]):
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert abs(a["similarity"] - b["similarity"]) < 1e-4
                assert a["id"] == b["id"] or abs(a["similarity"] - b["similarity"]) < 1e-6
    assert all(int(d["id"][1:]) % 2 == 1 for d in res[1])      # rows of rank 1 only
