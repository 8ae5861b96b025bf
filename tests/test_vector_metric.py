"""Similarity metrics of the local vector store on the CPU: ``cosine`` / ``dot-product`` /
``euclidean`` collections on the exact top-k path, their persistence, the SQL datasource's
``dot_product`` / ``euclidean_distance`` orderings with one mirror per metric, the
``similarity`` key of the asset and the sink, and the sharded service over gloo.

Rows and queries are unit vectors scaled by a factor from [0.5, 2], so the three metrics rank
differently.  fp32 stores compare against fp64 brute force at 1e-4; bf16 stores compare
against brute force over the store's own rounded rows at 8e-3 on a score (2e-3 of the
unit-vector tests x max|q| * max|x| = 4) and twice that on d^2."""
import json
import os
import socket
import sqlite3
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from langstream_amd.engine.vector_store import (VectorStore, VectorStoreRegistry, _Persistence, canonical_metric)
from langstream_amd.ops import reference as ref

TOL = 8e-3


def _scaled(n, D, g):
    v = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=-1)
    return v * (0.5 + 1.5 * torch.rand(n, 1, generator=g))


@pytest.fixture()
def registry():
    VectorStoreRegistry.reset()
    old = VectorStoreRegistry.persist_dir
    VectorStoreRegistry.persist_dir = None
    yield VectorStoreRegistry
    VectorStoreRegistry.reset()
    VectorStoreRegistry.persist_dir = old


# ---------------------------------------------------------------- the reference op
def test_reference_adds_the_bias_in_fp32():
    g = torch.Generator().manual_seed(1)
    X, Q = _scaled(500, 24, g).bfloat16(), _scaled(4, 24, g).bfloat16()
    b = X.float().pow(2).sum(-1).mul(-0.5)
    s, i = ref.knn_topk(X, Q, 7, bias=b)
    d2 = torch.cdist(Q.double(), X.double()).pow(2)
    assert torch.equal(i.long(), d2.topk(7, largest=False).indices)
    qn2 = Q.double().pow(2).sum(-1, keepdim=True)
    assert (qn2 - 2 * s.double() - d2.gather(1, i.long())).abs().max() < 1e-5
    from langstream_amd import ops
    s2, i2 = ops.knn_topk(X, Q, 7, bias=b)             # the CPU path of the op
    assert torch.equal(s, s2) and torch.equal(i, i2)
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 7, bias=b[:-1])
    with pytest.raises(ValueError):
        ops.knn_topk(X, Q, 7, bias=b.double())


# ---------------------------------------------------------------- the store
def _expect(st, queries, k):
    """Brute force in fp64 over the store's own rows: [(id, score, d2)] best first."""
    X = st._vecs[: len(st)].double()
    q = st._to_device_query(st._prepare_host(queries)).double()
    dot = q @ X.t()
    if st.metric == "euclidean":
        key = -(q.pow(2).sum(-1, keepdim=True) - 2 * dot + X.pow(2).sum(-1)[None])
    else:
        key = dot
    v, i = key.topk(min(k, len(st)), dim=1)
    return [[(st._ids[r], s, -s) for r, s in zip(ir, vr)] for ir, vr in zip(i.tolist(), v.tolist())]


def _same(st, res, exp, tol):
    assert [len(r) for r in res] == [len(e) for e in exp]
    for r, e in zip(res, exp):
        for hit, (_, v, d2) in zip(r, e):
            if st.metric == "euclidean":
                assert abs(hit["distance"] ** 2 - d2) < 2 * tol
                assert abs(hit["similarity"] - 1 / (1 + hit["distance"] ** 2)) < 1e-9
            else:
                assert abs(hit["similarity"] - v) < tol and "distance" not in hit
        sims = [h["similarity"] for h in r]
        assert sims == sorted(sims, reverse=True)
        # near-ties within the tolerance may swap: ids as sets clear of the cut
        if st.metric == "euclidean":
            cut = e[-1][2]
            assert {i for i, _, d2 in e if d2 < cut - 4 * tol} <= {h["id"] for h in r}
        else:
            cut = e[-1][1]
            assert {i for i, v, _ in e if v > cut + 2 * tol} <= {h["id"] for h in r}


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, TOL)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("metric", ["euclidean", "dot-product"])
@pytest.mark.parametrize("D,k", [(24, 10), (100, 70)], ids=["D24-k10", "D100-k70"])   # no kernel dim; k > 64
def test_store_metric_semantics(metric, dtype, tol, D, k):
    g = torch.Generator().manual_seed(3)
    N = 700
    st = VectorStore(D, device="cpu", dtype=dtype, metric=metric, capacity=256)
    vec = _scaled(N, D, g)
    st.upsert(list(range(N)), vec, [{"tenant": "ab"[r % 2]} for r in range(N)])
    qs = _scaled(5, D, g)
    _same(st, st.search(qs, k), _expect(st, qs, k), tol)
    # rows are stored as given, rounded to the store dtype
    assert torch.equal(torch.tensor(st.vector(3)), vec[3].to(dtype).float())
    # overwrite with other norms (a duplicate id: the last wins), delete with renumbering, grow
    st.upsert([5, 17, 5], 3.0 * _scaled(3, D, g), [{"tenant": "a"}] * 3)
    st.upsert([f"new{j}" for j in range(5)], qs, [{"tenant": "b"}] * 5)
    st.delete(list(range(0, 300, 3)))
    res = st.search(qs, k)
    _same(st, res, _expect(st, qs, k), tol)
    if metric == "euclidean":
        assert [r[0]["id"] for r in res] == [f"new{j}" for j in range(5)]
        assert all(r[0]["distance"] < 0.05 for r in res)
        b = st._vecs[: len(st)].float().pow(2).sum(-1).mul(-0.5)
        assert torch.equal(st._bias[: len(st)], b), "the bias follows upserts, deletes and growth"
    cap = st._vecs.shape[0]
    st.upsert([f"g{j}" for j in range(cap)], _scaled(cap, D, g), [{"tenant": "a"}] * cap)
    assert st._vecs.shape[0] > cap
    _same(st, st.search(qs, k), _expect(st, qs, k), tol)
    # filtered: masked and compact routes agree
    out = {}
    for cm in (0, 1 << 30):
        st.compact_max = cm
        out[cm] = [[(h["id"], h["similarity"]) for h in r] for r in st.search(qs, 10, filter={"tenant": "b"})]
    assert out[0] == out[1 << 30] and all(len(r) == 10 for r in out[0])


def test_metric_spellings_and_cosine_is_unchanged():
    assert [canonical_metric(m) for m in ("dot", "dot_product", "l2", "Cosine")] == \
        ["dot-product", "dot-product", "euclidean", "cosine"]
    with pytest.raises(ValueError):
        VectorStore(8, device="cpu", metric="manhattan")
    g = torch.Generator().manual_seed(4)
    vec, qs = _scaled(300, 20, g), _scaled(4, 20, g)
    a = VectorStore(20, device="cpu")
    b = VectorStore(20, device="cpu", metric="cosine")
    for st in (a, b):
        st.upsert(list(range(300)), vec, [{"n": r} for r in range(300)])
    assert a.metric == "cosine" and a._bias is None
    assert a.search(qs, 9, with_vectors=True) == b.search(qs, 9, with_vectors=True)
    assert all("distance" not in h for r in a.search(qs, 9) for h in r)
    # the three metrics rank differently on this data
    tops = {}
    for m in ("cosine", "dot-product", "euclidean"):
        st = VectorStore(20, device="cpu", metric=m)
        st.upsert(list(range(300)), vec)
        tops[m] = [[h["id"] for h in r] for r in st.search(qs, 9)]
    assert tops["cosine"] != tops["dot-product"] != tops["euclidean"] != tops["cosine"]


# ---------------------------------------------------------------- persistence
def _hits(st, qs, k=6):
    return [[(h["id"], round(h["similarity"], 6), round(h.get("distance", 0.0), 6)) for h in r]
            for r in st.search(qs, k)]


def test_euclidean_collection_survives_wal_and_snapshot(registry, tmp_path):
    g = torch.Generator().manual_seed(5)
    vec, qs = _scaled(200, 16, g), _scaled(3, 16, g)
    registry.configure(persist_dir=str(tmp_path))
    try:
        st = registry.get("docs", 16, device="cpu", metric="l2")
        assert st.metric == "euclidean"
        st.upsert(list(range(200)), vec, [{"n": r} for r in range(200)])
        st.delete([3, 4])
        want = _hits(st, qs)
        assert registry.metric_of("docs") == "euclidean"
        d = registry._dir_of("docs")
        assert not os.path.exists(os.path.join(d, "snapshot.lsv"))     # WAL only
        registry.reset()
        assert registry.metric_of("docs") == "euclidean" and registry._persisted_dim("docs") == 16
        st = registry.get("docs", device="cpu")                         # no metric, no dim
        assert st.metric == "euclidean" and _hits(st, qs) == want
        st.snapshot()
        assert _Persistence.read_snapshot_header(os.path.join(d, "snapshot.lsv"))[0]["metric"] == "euclidean"
        os.remove(os.path.join(d, "collection.json"))                   # the header alone is enough
        registry.reset()
        st = registry.get("docs", device="cpu")
        assert st.metric == "euclidean" and _hits(st, qs) == want
        registry.reset()
        with pytest.raises(ValueError):
            registry.get("docs", device="cpu", metric="cosine")
        with pytest.raises(ValueError):
            VectorStore(16, device="cpu", persist_dir=d, metric="cosine")
        st = registry.get("docs", device="cpu", metric="euclidean")
        with pytest.raises(ValueError):
            registry.get("docs", metric="dot-product")                  # the open collection
    finally:
        registry.reset()
        registry.persist_dir = None


@pytest.mark.parametrize("snap", [False, True], ids=["wal", "snapshot"])
def test_directory_without_a_metric_opens_as_cosine(tmp_path, snap):
    g = torch.Generator().manual_seed(6)
    vec, qs = _scaled(50, 8, g), _scaled(2, 8, g)
    d = str(tmp_path / "c")
    st = VectorStore(8, device="cpu", persist_dir=d, name="c")
    st.upsert(list(range(50)), vec)
    want = _hits(st, qs)
    if snap:
        st.snapshot()
    st.close()
    # what the code before metrics wrote: no sidecar, no "metric" key in the header
    os.remove(os.path.join(d, "collection.json"))
    if snap:
        p = os.path.join(d, "snapshot.lsv")
        hdr, off = _Persistence.read_snapshot_header(p)
        with open(p, "rb") as f:
            body = f.read()[off:]
        hdr.pop("metric")
        h = json.dumps(hdr).encode()
        with open(p, "wb") as f:
            f.write(_Persistence.MAGIC + len(h).to_bytes(8, "little") + h + body)
    with pytest.raises(ValueError):
        VectorStore(8, device="cpu", persist_dir=d, name="c", metric="euclidean")
    st = VectorStore(8, device="cpu", persist_dir=d, name="c", metric=None)
    assert st.metric == "cosine" and _hits(st, qs) == want
    st.close()
    assert VectorStore(8, device="cpu", persist_dir=d, name="c").metric == "cosine"


# ---------------------------------------------------------------- SQL
def _sql_table(tmp_path, kind):
    """300 rows whose ranking under ``kind`` is well separated at bf16 precision (the mirror
    holds bf16 rows, SQLite ranks the unrounded ones), in an order unrelated to the rowid:
    euclidean   row r lies at distance 0.05 + 0.02 p(r) from the query (rounding moves a
                distance by < 0.01);
    dot-product row r = a q + noise orthogonal to q, a = 3 - 0.01 p(r): dot products 0.029
                apart (rounding moves one by < 0.01);
    cosine      the construction of test_sqlite_where_knn_equals_sqlite_order, all rows of
                the query's norm, so cosine and distance are both well separated."""
    from langstream_amd.agents.vector.datasources import SqliteDataSource, _cosine, _dot, _euclid
    path = str(tmp_path / "docs.db")
    ds = SqliteDataSource({"url": f"jdbc:sqlite:{path}"})
    ds.script(["CREATE TABLE docs (name TEXT PRIMARY KEY, lang TEXT, n INTEGER, v TEXT)"])
    g = torch.Generator().manual_seed(7)
    D, N = 16, 300
    q = 1.7 * torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    qh = q / q.norm()
    noise = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    for r in range(N):
        p = (r * 7) % N
        orth = torch.nn.functional.normalize(noise[r] - (noise[r] @ qh) * qh, dim=0)
        if kind == "euclidean":
            v = q + (0.05 + 0.02 * p) * noise[r]
        elif kind == "dot-product":
            v = (3 - 0.01 * p) * q + 0.5 * orth
        else:
            c = 0.95 - 0.006 * r
            v = q.norm() * (c * qh + (1 - c * c) ** 0.5 * orth)
        ds.execute_statement("INSERT INTO docs (name, lang, n, v) VALUES (?, ?, ?, ?)", None,
                             [f"doc{r}", ["en", "de", "fr"][r % 3], r % 10, v.tolist()])
    plain = sqlite3.connect(path)                      # a connection without a mirror
    for name, fn in (("cosine_similarity", _cosine), ("dot_product", _dot), ("euclidean_distance", _euclid)):
        plain.create_function(name, 2, fn)
    return ds, plain, q


ORDERS = {"euclidean": "euclidean_distance(v, ?) ASC", "dot-product": "dot_product(v, CAST(? AS FLOAT ARRAY)) DESC",
          "cosine": "cosine_similarity(v, ?) DESC"}


def _sql_check(ds, plain, q, metric, where="", params=(), k=8):
    order = ORDERS[metric]
    sql = f"SELECT rowid AS rid, name, lang FROM docs {where} ORDER BY {order} LIMIT {k}"
    want = plain.execute(sql.replace("CAST(? AS FLOAT ARRAY)", "?"), list(params) + [json.dumps(q.tolist())]).fetchall()
    got = ds.fetch_data(sql, list(params) + [q.tolist()])
    assert [(r["rid"], r["name"], r["lang"]) for r in got] == [tuple(r) for r in want], (metric, where)
    return got


@pytest.mark.parametrize("metric", ["euclidean", "dot-product"])
def test_sql_metric_knn_equals_sqlite_order(registry, tmp_path, metric):
    ds, plain, q = _sql_table(tmp_path, metric)
    for where, params in [("", []), ("WHERE lang = ?", ["de"]), ("WHERE lang = ? AND n > ?", ["fr", 6]),
                          ("WHERE n = ?", [1234]), ("WHERE name IN (?, ?)", ["doc200", "doc7"])]:
        _sql_check(ds, plain, q, metric, where, params)
    st = VectorStoreRegistry.get(ds._store_name("docs", "v", metric), persist=False)
    assert st.metric == metric and len(st) == 300 and st.filter_stats["mask_builds"] >= 3
    # the wrong direction is SQLite's to answer: no mirror is asked
    flipped = {"euclidean": "euclidean_distance(v, ?) DESC", "dot-product": "dot_product(v, ?) ASC"}[metric]
    builds = st.filter_stats["mask_builds"]
    sql = f"SELECT name FROM docs WHERE lang = ? ORDER BY {flipped} LIMIT 4"
    got = ds.fetch_data(sql, ["de", q.tolist()])
    want = plain.execute(sql, ["de", json.dumps(q.tolist())]).fetchall()
    assert [r["name"] for r in got] == [r[0] for r in want] and st.filter_stats["mask_builds"] == builds
    plain.close()


def test_sql_mirrors_per_metric_follow_writes(registry, tmp_path):
    from langstream_amd.agents.vector import _JdbcWriter
    from langstream_amd.agents.genai.mutable import MutableRecord
    from langstream_amd.api.record import SimpleRecord
    ds, plain, q = _sql_table(tmp_path, "cosine")
    # a long row almost along the query: second to none by cosine, far away by distance --
    # a euclidean query answered from the cosine mirror (normalised rows) would return it
    c = 0.99
    far = 3 * q.norm() * (c * q / q.norm() + (1 - c * c) ** 0.5 * torch.nn.functional.normalize(
        torch.tensor([1.0] + [0.0] * 15) - q[0] / q.norm() ** 2 * q, dim=0))
    ds.execute_statement("INSERT INTO docs (name, lang, n, v) VALUES (?, ?, ?, ?)", None, ["far", "en", 1, far.tolist()])
    assert _sql_check(ds, plain, q, "cosine")[0]["name"] == "far"
    assert all(r["name"] != "far" for r in _sql_check(ds, plain, q, "euclidean"))
    assert {k[2] for k in ds.vector_cols} == {"cosine", "euclidean"}
    # statements through the datasource drop both mirrors; they are rebuilt on the next query
    ds.execute_statement("INSERT INTO docs (name, lang, n, v) VALUES (?, ?, ?, ?)", None,
                         ["copy", "en", 1, q.tolist()])
    for m in ("cosine", "euclidean"):
        assert _sql_check(ds, plain, q, m)[0]["name"] == "copy"
    ds.execute_statement("DELETE FROM docs WHERE name = ?", None, ["copy"])
    for m in ("cosine", "euclidean"):
        assert all(r["name"] != "copy" for r in _sql_check(ds, plain, q, m))
    # the sink's writer updates every live mirror of the column in place
    w = _JdbcWriter.__new__(_JdbcWriter)
    w.ds, w.table = ds, "docs"
    w.fields = [{"name": "name", "expression": "key", "primary-key": True},
                {"name": "lang", "expression": "value.lang"}, {"name": "n", "expression": "value.n"},
                {"name": "v", "expression": "value.v"}]
    w.pk, w.cols = ["name"], ["lang", "n", "v"]
    stores = {m: VectorStoreRegistry.get(ds._store_name("docs", "v", m), persist=False) for m in ("cosine", "euclidean")}
    w.upsert(MutableRecord.from_record(SimpleRecord.of("copy2", {"lang": "de", "n": 2, "v": q.tolist()})))
    assert all(len(st) == 302 for st in stores.values())
    for m in ("cosine", "euclidean"):
        assert _sql_check(ds, plain, q, m)[0]["name"] == "copy2"
        assert VectorStoreRegistry.get(ds._store_name("docs", "v", m), persist=False) is stores[m]
    w.upsert(MutableRecord.from_record(SimpleRecord.of("copy2", None)))     # a tombstone
    assert all(len(st) == 301 for st in stores.values())
    for m in ("cosine", "euclidean"):
        assert all(r["name"] != "copy2" for r in _sql_check(ds, plain, q, m))
    plain.close()


# ---------------------------------------------------------------- asset, sink, datasource
def test_asset_similarity(registry):
    from langstream_amd.agents.assets import VectorCollectionManager
    from langstream_amd.core.config_model import validate_asset
    cfg = validate_asset("a", "vector-collection", {"collection-name": "euc", "dimension": 12, "similarity": "euclidean"})
    VectorCollectionManager(SimpleNamespace(config=cfg, asset_type="vector-collection")).deploy_asset()
    assert registry.get("euc").metric == "euclidean" and registry.get("euc").dim == 12
    cfg = validate_asset("a", "vector-collection", {"collection-name": "plain", "dimension": 12})
    VectorCollectionManager(SimpleNamespace(config=cfg, asset_type="vector-collection")).deploy_asset()
    assert registry.get("plain").metric == "cosine"
    with pytest.raises(ValueError):
        validate_asset("a", "vector-collection", {"collection-name": "x", "similarity": "manhattan"})


def test_sink_and_datasource_similarity(registry):
    from langstream_amd.agents.vector import VectorDBSinkAgent
    from langstream_amd.agents.vector.datasources import LocalVectorDataSource
    from langstream_amd.api.record import SimpleRecord
    from langstream_amd.core.config_model import validate_agent
    fields = [{"name": "id", "expression": "key"}, {"name": "vector", "expression": "value.vec"}]
    cfg = {"datasource": {"service": "local"}, "collection-name": "l2docs", "similarity": "euclidean", "fields": fields}
    validate_agent("s", "vector-db-sink", dict(cfg, datasource="ds"), "local")
    with pytest.raises(ValueError):
        validate_agent("s", "vector-db-sink", dict(cfg, datasource="ds", similarity="nearest"), "local")
    a = VectorDBSinkAgent()
    a.init(cfg)
    a.set_context(None)
    for i in range(4):
        a.write(SimpleRecord.of(f"k{i}", {"vec": [1.0 + i, 2.0, 0.0]})).result(10)
    a.close()
    st = registry.get("l2docs")
    assert st.metric == "euclidean" and len(st) == 4
    # the JSON query language needs no key: the collection decides, hits carry the distance
    ds = LocalVectorDataSource({"collection-name": "l2docs", "similarity": "l2"})
    rows = ds.fetch_data('{"vector": ?, "top-k": 2}', [[3.0, 2.0, 0.0]])
    assert [r["id"] for r in rows] == ["k2", "k1"] or [r["id"] for r in rows] == ["k2", "k3"]
    assert rows[0]["distance"] < 1e-3 and abs(rows[1]["distance"] - 1.0) < 1e-2
    # another metric than the existing collection's: an error at init, never an override
    b = VectorDBSinkAgent()
    with pytest.raises(ValueError):
        b.init(dict(cfg, similarity="cosine"))
    with pytest.raises(ValueError):
        LocalVectorDataSource({"collection-name": "l2docs", "similarity": "dot-product"})
    # a datasource creates its collections with its metric
    ds = LocalVectorDataSource({"collection-name": "mips", "similarity": "dot"})
    ds.execute_statement('{"id": "a", "vector": ?}', None, [[1.0, 0.0]])
    ds.execute_statement('{"id": "b", "vector": ?}', None, [[3.0, 0.0]])
    assert registry.get("mips").metric == "dot-product"
    assert [r["id"] for r in ds.fetch_data('{"vector": ?, "top-k": 2}', [[1.0, 0.0]])] == ["b", "a"]


# ---------------------------------------------------------------- the sharded service
def _spawn(fn, world=2):
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


def _corpus():
    g = torch.Generator().manual_seed(13)
    return _scaled(600, 48, g), _scaled(8, 48, g), [{"lang": ["en", "de", "fr"][i % 3]} for i in range(600)]


SHARD_FILTERS = [{"lang": "de"}, None, None, {"lang": "fr"}, None, {"id": {"$in": ["d10", "d11", "d301"]}}, None, None]


def _sharded_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from langstream_amd.engine import dist_knn
        vecs, queries, meta = _corpus()
        rows = [i for i in range(vecs.shape[0]) if i % world == rank]
        VectorStoreRegistry.get("docs", 48, device="cpu", metric="euclidean").upsert(
            [f"d{i}" for i in rows], vecs[rows].tolist(), [meta[i] for i in rows])
        # a collection whose shards disagree on the metric: rank 1's shard is cosine
        VectorStoreRegistry.get("mixed", 48, device="cpu", metric="euclidean" if rank == 0 else "cosine").upsert(
            [f"d{i}" for i in rows], vecs[rows].tolist())
        svc = dist_knn.start(device="cpu")
        mine = list(range(rank, queries.shape[0], world))
        batch = svc.search("docs", queries[mine].tolist(), 9, filter=[SHARD_FILTERS[i] for i in mine]).result(60)
        res = {i: r for i, r in zip(mine, batch)}
        bad = svc.search("mixed", queries[:1].tolist(), 3) if rank == 0 else None
        dist.barrier()
        errs = None
        if bad is not None:
            try:
                errs = ("ok", len(bad.result(60)[0]))
            except Exception as e:  # noqa: BLE001
                errs = (type(e).__name__, str(e))
        after = svc.search("docs", queries[mine[:1]].tolist(), 9).result(60)[0]   # the service still serves
        gathered = [None] * world
        dist.all_gather_object(gathered, (res, errs, len(after)))
        dist_knn.stop()
        VectorStoreRegistry.reset()
        if rank == 0:
            q.put(gathered)
    finally:
        dist.destroy_process_group()


def test_sharded_euclidean_search_equals_single_store():
    gathered = _spawn(_sharded_worker, 2)
    vecs, queries, meta = _corpus()
    single = VectorStore(48, device="cpu", metric="euclidean")
    single.upsert([f"d{i}" for i in range(600)], vecs.tolist(), meta)
    res = {}
    for r, errs, n_after in gathered:
        res.update(r)
        assert n_after == 9
    # rank 1's cosine shard of "mixed" refused the euclidean queries; the collectives went on
    assert gathered[1][1] is None and gathered[0][1][0] in ("ok", "ValueError")
    for i in range(queries.shape[0]):
        want = single.search(queries[i:i + 1].tolist(), 9, filter=SHARD_FILTERS[i])[0]
        got = res[i]
        assert len(got) == len(want) == (3 if i == 5 else 9)
        for a, b in zip(got, want):
            assert abs(a["distance"] - b["distance"]) < 1e-4 and abs(a["similarity"] - b["similarity"]) < 1e-4
            assert a["id"] == b["id"] or abs(a["distance"] - b["distance"]) < 1e-6
