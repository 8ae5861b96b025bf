"""Sliding-window attention through every LlamaRunner route and the engine's decode graphs.

The scheme of test_qkv_bias_gpu.py::test_runner_routes_add_the_bias: ``llama-small`` /
``llama-tiny`` with ``sliding_window=16`` (every decode context of a step is >= 20, every
checked prefill row sits at a position >= 2 * 16), the native runner against the Python
forward of the same model, and against the same weights with no window, which every row
must leave by more than ten times the agreement bound: a route that forgets the window
cannot pass."""
from __future__ import annotations

import dataclasses
import functools

import pytest
import torch

from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import AttnMeta, LlamaModel, PRESETS

pytestmark = pytest.mark.gpu
DEV = "cuda"
BS = ops.KV_BLOCK
W = 16
COS_BOUND = 0.999   # tests/test_engine_gpu.py test_native_runner_matches_python_forward


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-12))


@functools.lru_cache(maxsize=None)
def _model(name, window, layers=None):
    """Same seed, same weights for every (window, layers) of one preset."""
    cfg = dataclasses.replace(PRESETS[name], sliding_window=window, window_layers=layers)
    return LlamaModel(cfg, device=DEV)


def _step_inputs(model, nd, npre, seed):
    """One step of nd decode rows (sequence i has ctx 20 + 3 i in blocks of its own, over a
    cache of random earlier tokens) followed by one prefill chunk of npre tokens.  Logit rows:
    every decode row (at most 16, spread over the batch) and prefill tokens npre / 2 and
    npre - 1 (positions >= 2 W: at least half of their keys lie outside the window)."""
    cfg = model.cfg
    T = nd + npre
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, cfg.vocab_size, (T,), generator=g, dtype=torch.int32).to(DEV)
    ctx = [20 + 3 * i for i in range(nd)]
    nbs = [(c + BS - 1) // BS for c in ctx]
    cols = max(nbs + [1])
    d_bt = torch.zeros(nd, cols, dtype=torch.int32)
    used = 0
    for i, n in enumerate(nbs):
        d_bt[i, :n] = torch.arange(used, used + n, dtype=torch.int32)
        used += n
    pblocks = (npre + BS - 1) // BS
    p_bt = torch.arange(used, used + pblocks, dtype=torch.int32).reshape(1, -1)
    nb = used + pblocks + 1
    pos = torch.tensor([c - 1 for c in ctx] + list(range(npre)), dtype=torch.int32)
    slots = [int(d_bt[i, (c - 1) // BS]) * BS + (c - 1) % BS for i, c in enumerate(ctx)]
    slots += [int(p_bt[0, t // BS]) * BS + t % BS for t in range(npre)]
    meta = AttnMeta(positions=pos.to(DEV), slots=torch.tensor(slots, dtype=torch.int64, device=DEV), num_decode=nd)
    if nd:
        meta.d_block_tables, meta.d_ctx_lens = d_bt.to(DEV), torch.tensor(ctx, dtype=torch.int32, device=DEV)
        meta.nsplit, meta.blocks_per_split = 1, cols
    if npre:
        assert npre // 2 >= 2 * W
        meta.num_prefill_tokens = npre
        meta.p_block_tables = p_bt.to(DEV)
        meta.q_start = torch.tensor([nd], dtype=torch.int32, device=DEV)
        meta.q_len = torch.tensor([npre], dtype=torch.int32, device=DEV)
        meta.ctx_len = torch.tensor([npre], dtype=torch.int32, device=DEV)
        meta.tiles = ops.prefill_tiles([npre], model.hq // model.hkv).to(DEV)

    def caches():
        gk = torch.Generator(device=DEV).manual_seed(seed + 1)
        kv = [ops.new_kv_cache(nb, model.hkv, cfg.head_dim, DEV, model.dtype) for _ in range(cfg.num_layers)]
        for kc, vc in kv:
            kc.copy_(torch.randn(kc.shape, device=DEV, generator=gk) * 0.5)
            vc.copy_(torch.randn(vc.shape, device=DEV, generator=gk) * 0.5)
        return kv

    drows = set(range(nd)) if nd <= 16 else set(range(0, nd, nd // 8)) | {nd - 1}
    prows = {nd + npre // 2, T - 1} if npre else set()
    rows = torch.tensor(sorted(drows | prows), dtype=torch.long, device=DEV)
    return ids, meta, caches, rows


@pytest.mark.parametrize("name,nd,npre,layers", [
    ("llama-small", 3, 0, None),       # <= 4 rows: the GEMV layer, fused-RoPE attention or gemv_qkv + decode
    ("llama-small", 8, 0, None),       # decode GEMM with RoPE in its reduction, then decode attention
    ("llama-small", 8, 70, None),      # mixed step: decode + prefill attention in one attend()
    ("llama-small", 0, 1100, None),    # prefill: nine 128-row tiles per kv head, first KV tile > 0
    ("llama-tiny", 8, 0, None),        # D = 64
    ("llama-small", 8, 70, (1, 3)),    # the window is per layer
    ("llama-small", 130, 0, None),     # 129..256 rows: the 256-row decode GEMMs; in a process started
                                       # with LS_DGEMM_FUSED=1 the norm-deferred layer (forward_dgemm)
], ids=["gemv3", "dgemm8", "mixed8+70", "prefill1100", "tiny-d64-8", "layers13-mixed8+70", "dgemm130"])
def test_runner_routes_apply_the_window(name, nd, npre, layers):
    model = _model(name, W, layers)
    full = _model(name, 0)
    assert [model.cfg.layer_window(i) for i in range(model.cfg.num_layers)] == [
        W if layers is None or i in layers else 0 for i in range(model.cfg.num_layers)]
    assert all(torch.equal(a.qkv_w, b.qkv_w) for a, b in zip(model.layers, full.layers))
    ids, meta, caches, rows = _step_inputs(model, nd, npre, 100 + nd + npre)
    a = model.forward_logits(ids, meta, caches(), rows).float().cpu()
    b = model.logits(model.forward(ids, meta, caches()).index_select(0, rows)).float().cpu()
    z = full.forward_logits(ids, meta, caches(), rows).float().cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    same = [_cos(a[i], b[i]) for i in range(len(rows))]
    diff = [_cos(a[i], z[i]) for i in range(len(rows))]
    print(f"runner {name} nd={nd} npre={npre} layers={layers}: min cos(native, python) {min(same):.6f}, "
          f"max cos(window, no window) {max(diff):.4f}")
    assert min(same) > COS_BOUND, same
    assert max(diff) < 1 - 10 * (1 - COS_BOUND), diff


def _run_tops(e, prompts, sp):
    tops = {}
    reqs = [e.submit(p, sp, callback=lambda ev, i=i: tops.setdefault(i, []).append(ev.top))
            for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [(r.output_ids, tops.get(i)) for i, r in enumerate(reqs)]


def test_engine_graph_decode_matches_eager_with_window():
    """B = 8, 16 greedy tokens, W = 64: graph replay against eager (a split only at a
    near-tie of the eager run's top-2, 0.02 nats), on the prompts of
    test_engine_graph_decode_matches_eager_with_bias; the unwindowed engine generates other
    tokens for the prompts longer than the window."""
    model = _model("llama-small", 64)
    lens = (5, 9, 33, 40, 64, 65, 100, 130)
    prompts = [list(range(3 + 5 * i, 3 + 5 * i + n)) for i, n in enumerate(lens)]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    kw = dict(num_blocks=128, max_model_len=1024, max_batch=8)
    e1 = LLMEngine(model, None, use_graphs=True, **kw)
    assert e1.stats["sliding_window"] == 64
    out1 = _run_tops(e1, prompts, sp)
    assert e1.stats["graph_steps"] > 0
    e2 = LLMEngine(model, None, use_graphs=False, **kw)
    out2 = _run_tops(e2, prompts, SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True, logprobs=2))
    for (ia, _), (ib, tb) in zip(out1, out2):
        assert len(ia) == len(ib) == 16
        for t, (x, y) in enumerate(zip(ia, ib)):
            if x != y:
                alt = dict(tb[t])
                assert x in alt and y in alt and abs(alt[x] - alt[y]) < 0.02, (t, x, y, tb[t])
                break
    out0 = _run_tops(LLMEngine(_model("llama-small", 0), None, use_graphs=True, **kw), prompts, sp)
    assert all(a[0] != z[0] for n, a, z in zip(lens, out1, out0) if n > 64), \
        "the window did not change the tokens generated after a prompt longer than it"
