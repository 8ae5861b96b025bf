"""FP8 projection weights under tensor parallelism: two real ranks (two processes sharing
cuda:0 over a gloo group, as test_native_executor_tp2_two_ranks_one_gpu) serve the shards
``shard_llama`` cuts from one fp8 state dict -- codes and row scales -- and produce the TP = 1
fp8 engine's greedy tokens up to genuine near-ties."""
import pytest
import torch

from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaModel, PRESETS

pytestmark = pytest.mark.gpu

PROMPTS = [list(range(3, 3 + n)) for n in (5, 33, 64, 200)]


def _run_tops(e, prompts, sp):
    tops = {}
    reqs = [e.submit(p, sp, callback=lambda ev, i=i: tops.setdefault(i, []).append(ev.top))
            for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [(r.output_ids, tops.get(i)) for i, r in enumerate(reqs)]


def _same_or_near_tie(a, b, gap: float = 0.1) -> None:
    (ids_a, _), (ids_b, tops_b) = a, b
    assert len(ids_a) == len(ids_b)
    for t, (x, y) in enumerate(zip(ids_a, ids_b)):
        if x == y:
            continue
        alt = dict(tops_b[t])
        assert x in alt and y in alt and abs(alt[x] - alt[y]) < gap, (t, x, y, tops_b[t])
        return


def _full_model():
    return LlamaModel(PRESETS["llama-small"], device="cpu", dtype=torch.float32, seed=9, weights_dtype="fp8")


def _worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from langstream_amd import ops
        from langstream_amd.models.llama import TPInfo
        from langstream_amd.models.loader import shard_llama
        cfg = PRESETS["llama-small"]
        m = LlamaModel(cfg, device="cuda", tp=TPInfo(rank, world, None), weights_dtype="fp8")
        m.load_state_dict(shard_llama(_full_model().state_dict(), cfg, rank, world))
        eng = LLMEngine(m, None, num_blocks=128, max_model_len=1024, max_batch=8, use_graphs=False)
        if rank == 0:
            out = _run_tops(eng, PROMPTS, SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True, logprobs=2))
            stats = dict(eng.stats)
            eng.stop()
            q.put((out, stats, ops.w8_launch_counts()))
        else:
            eng.worker_loop()
    finally:
        dist.destroy_process_group()


def test_w8_native_executor_tp2_two_ranks_one_gpu():
    import multiprocessing as mp
    import socket
    cfg = PRESETS["llama-small"]
    m0 = LlamaModel(cfg, device="cuda", weights_dtype="fp8")
    m0.load_state_dict(_full_model().state_dict())
    e0 = LLMEngine(m0, None, num_blocks=128, max_model_len=1024, max_batch=8, use_graphs=False)
    ref = _run_tops(e0, PROMPTS, SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True, logprobs=2))
    e0.stop()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got, stats, census = q.get(timeout=100)
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert stats["decode_steps"] > 0 and stats["weights_dtype"] == "fp8"
    assert sum(census.values()) >= 4 * cfg.num_layers * stats["decode_steps"], census
    for a, b in zip(got, ref):
        _same_or_near_tie(a, b)
