"""The bias of a fused QKV projection (Qwen2) in the two kernels that finish one --
rope_and_cache and the split-K reduction of decode_gemm_qkv_rope -- and in every LlamaRunner
route of a model that has it.

Bias values (``_bias``): column c of head h holds (-1)^(c + c // (D/2)) (0.5 + c / 256)
(1 + h / 2), rounded to bf16.  The magnitudes of one head are distinct (steps of one bf16
ulp in [0.5, 1) before the head's factor), every |b| >= 0.5, and the neighbours a wrong
index would pick differ by far more than the bounds: the next column and the same column of
the other half have the opposite sign (> 1 apart), the same column of the next head is
>= 0.25 away.  Entries cannot all be distinct in bf16 at these magnitudes (1920 entries for
(Hq, Hkv, D) = (9, 3, 128), 128 bf16 values per binade)."""
from __future__ import annotations

import functools

import pytest
import torch

from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import AttnMeta, LlamaModel, PRESETS
from langstream_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
BS = ops.KV_BLOCK
KS, VS = 0.25, 4.0   # scales of the fp8 cases


def _err(a, b):
    return (a.float().cpu() - b.float().cpu()).abs()


def _close(a, b, atol, rtol=0.0, msg=""):
    """tests/test_kernels_gpu.py _close; returns the largest deviation."""
    err = _err(a, b)
    bad = err > atol + rtol * b.float().cpu().abs()
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"
    return err.max().item()


def _bias(H, D, device=DEV):
    c = torch.arange(D)
    sign = 1.0 - 2.0 * ((c + c // (D // 2)) % 2)
    row = sign * (0.5 + c / 256.0)
    b = row[None, :] * (1.0 + torch.arange(H)[:, None] / 2.0)
    return b.reshape(-1).to(torch.bfloat16).to(device)


@functools.lru_cache(maxsize=None)
def _cos_sin(D):
    return ref.rope_cos_sin(4096, D, 1e6, device=DEV)


def _caches(NB, Hkv, D, dtype):
    """Zeroed caches of NB + 1 blocks and the NB-block views the writers get: slot NB * BS,
    one past the views' end, still lies inside the allocation."""
    full = ops.new_kv_cache(NB + 1, Hkv, D, DEV, dtype)
    return full, tuple(c.narrow(0, 0, NB) for c in full)


def _slots(T, NB, seed):
    """Distinct valid slots, one NB * BS (one block past the views) and, from two tokens, one -1."""
    s = torch.randperm(NB * BS, generator=torch.Generator().manual_seed(seed))[:T].to(torch.int64)
    if T > 1:
        s[T // 2] = -1
    s[T - 1] = NB * BS
    return s.to(DEV)


def _bits(t):
    return t.view(torch.uint8) if t.dtype == FP8 else t.view(torch.int16)


def _check_caches_hold_rows(full, rows, slots, NB, Hq, Hkv, D, f8):
    """tests/test_kv_writers_gpu.py: every cached token's K row and V^T column hold the k / v
    heads of the writer's own qkv row bit for bit (fp8: their ops.reference codes); skipped
    slots (-1, NB * BS) and the block past the views are not written."""
    kfull, vfull = _bits(full[0]).cpu(), _bits(full[1]).cpu()
    assert not kfull[NB].any() and not vfull[NB].any(), "the block past the end was written"
    r = rows.cpu().view(-1, Hq + 2 * Hkv, D)
    k, v = r[:, Hq: Hq + Hkv], r[:, Hq + Hkv:]
    if f8:
        k, v = ref.quantize_kv(k, KS), ref.quantize_kv(v, VS)
    sl = slots.cpu()
    ok = (sl >= 0) & (sl < NB * BS)
    blk, off = sl[ok] // BS, sl[ok] % BS
    ek, ev = torch.zeros_like(kfull), torch.zeros_like(vfull)
    ek[blk, :, off] = _bits(k[ok].contiguous())
    ev[blk, :, off // 8, :, off % 8] = _bits(v[ok].contiguous())
    assert int(ok.sum()) == len(sl) - (2 if len(sl) > 1 else 1)
    assert torch.equal(kfull, ek), "k cache bits"
    assert torch.equal(vfull, ev), "v cache bits"


# --------------------------------------------------------------------------- rope_and_cache
@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (9, 3)])   # (9, 3): a one-head and a three-head rotate group
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 5, 2049])             # 2049: the 16-token tiles, a one-token last tile
def test_rope_and_cache_bias(T, D, Hq, Hkv, f8):
    """Against ref.rope_and_cache(..., bias=) on a CPU copy with the bounds of
    test_kernels_gpu.py::test_rope_and_cache (0.03 / 0.01 on qkv and the K cache, V exact),
    the cache contract of test_kv_writers_gpu.py, and: a zero bias is bit-identical to no bias."""
    H = Hq + 2 * Hkv
    NB = (T + BS - 1) // BS + 2
    torch.manual_seed(T + D + Hq)
    qkv0 = (torch.randn(T, H * D, device=DEV) * 2).to(torch.bfloat16)
    pos = torch.randint(0, 4096, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    slots = _slots(T, NB, T + D)
    bias = _bias(H, D)
    dt = FP8 if f8 else torch.bfloat16
    ks, vs = (KS, VS) if f8 else (1.0, 1.0)
    full, (kc, vc) = _caches(NB, Hkv, D, dt)
    qkv = qkv0.clone()
    ops.rope_and_cache(qkv, pos, _cos_sin(D), slots, kc, vc, Hq, Hkv, k_scale=ks, v_scale=vs, bias=bias)
    torch.cuda.synchronize()
    # reference on the CPU (it has no upper slot check: the slot past the views reads -1 there)
    qc = qkv0.cpu().clone()
    kr, vr = ops.new_kv_cache(NB + 1, Hkv, D, "cpu", dt)
    sc = slots.cpu().clone()
    sc[sc >= NB * BS] = -1
    ref.rope_and_cache(qc, pos.cpu(), _cos_sin(D).cpu(), sc, kr, vr, Hq, Hkv, True, ks, vs, bias.cpu())
    e_qkv = _close(qkv, qc, 0.03, 0.01, "qkv")
    v0 = (Hq + Hkv) * D
    assert torch.equal(qkv[:, v0:].cpu(), qc[:, v0:]), "v rows: bf16(v + b), one rounding"
    if f8:
        e_k = _err(full[0].float() * KS, kr.float() * KS).max().item()
    else:
        e_k = _close(full[0], kr, 0.03, 0.01, "k cache")
    assert torch.equal(_bits(full[1]).cpu(), _bits(vr)), "v cache"
    _check_caches_hold_rows(full, qkv, slots, NB, Hq, Hkv, D, f8)
    print(f"rope_and_cache bias T={T} D={D} H=({Hq},{Hkv}) {'fp8' if f8 else 'bf16'}: "
          f"max |qkv - ref| {e_qkv:.4g}, max |K cache - ref| {e_k:.4g}")
    # zero bias == no bias, bit for bit
    outs = []
    for b in (None, torch.zeros_like(bias)):
        f, (k2, v2) = _caches(NB, Hkv, D, dt)
        q2 = qkv0.clone()
        ops.rope_and_cache(q2, pos, _cos_sin(D), slots, k2, v2, Hq, Hkv, k_scale=ks, v_scale=vs, bias=b)
        outs.append((q2, f))
    (qa, fa), (qb, fb) = outs
    assert torch.equal(qa, qb) and torch.equal(_bits(fa[0]), _bits(fb[0])) and torch.equal(_bits(fa[1]), _bits(fb[1]))
    assert not torch.equal(qa, qkv), "the bias changed nothing"


# --------------------------------------------------------------------- decode_gemm_qkv_rope
def _dg_key(M, s):
    """The launch-census key of a 128-column partial-sum tile (test_kernels_gpu.py _dg_key)."""
    return f"bn128_partial_bm{64 if M <= 64 else 128 if M <= 128 else 256}_s{s}"


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("M,Hq,Hkv,D", [(5, 4, 2, 128), (64, 4, 2, 128), (129, 4, 2, 128), (256, 4, 2, 128),
                                        (5, 8, 4, 64)])   # D = 64: decode_gemm + rope_and_cache inside
def test_decode_gemm_qkv_rope_bias(M, Hq, Hkv, D, f8):
    """The reference and bounds of test_kernels_gpu.py::test_decode_gemm_qkv_rope with the
    bias: an fp32 projection + bias rotated in fp32 (0.03 / 0.03), the rows in the caches,
    rows with slot -1 (and the slot past the views) not cached."""
    K, H = 1024, Hq + 2 * Hkv
    N = H * D
    NB = 2 * M // BS + 2
    torch.manual_seed(M + D)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K ** 0.5).to(torch.bfloat16)
    pos = torch.randint(0, 4000, (M,), device=DEV, dtype=torch.int32)
    slots = _slots(M, NB, M)
    bias = _bias(H, D)
    full, (kc, vc) = _caches(NB, Hkv, D, FP8 if f8 else torch.bfloat16)
    qkv = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    wsp = torch.empty(64 * M * N + 4 * 256 * 256, device=DEV, dtype=torch.float32)
    ops.hip().decode_gemm_launch_counts(True)
    ops.hip().decode_gemm_qkv_rope(qkv, x, w, wsp, pos, _cos_sin(D), slots, kc, vc, Hq, Hkv, KS if f8 else 1.0,
                                   VS if f8 else 1.0, bias)
    # 8 tiles x 4 K slices: the split-K partial-sum GEMM whose reduction adds the bias
    assert dict(ops.hip().decode_gemm_launch_counts(True)) == {_dg_key(M, 4): 1}
    torch.cuda.synchronize()
    y = (x.float() @ w.float().t() + bias.float()).view(M, H, D)
    cs = _cos_sin(D)[pos.long()]
    co, si = cs[:, None, : D // 2], cs[:, None, D // 2:]
    a, b = y[:, : Hq + Hkv, : D // 2], y[:, : Hq + Hkv, D // 2:]
    exp = torch.cat([torch.cat([a * co - b * si, b * co + a * si], -1), y[:, Hq + Hkv:]], 1)
    e = _close(qkv.view(M, H, D), exp, 0.03, 0.03, "qkv")
    _check_caches_hold_rows(full, qkv, slots, NB, Hq, Hkv, D, f8)
    print(f"decode_gemm_qkv_rope bias M={M} D={D} {'fp8' if f8 else 'bf16'}: max |qkv - fp32| {e:.4g}")
    if D == 128:   # zero bias == no bias, bit for bit
        outs = []
        for bz in (None, torch.zeros_like(bias)):
            q2 = torch.empty_like(qkv)
            _, (k2, v2) = _caches(NB, Hkv, D, torch.bfloat16)
            ops.hip().decode_gemm_qkv_rope(q2, x, w, wsp, pos, _cos_sin(D), slots, k2, v2, Hq, Hkv, 1.0, 1.0, bz)
            outs.append(q2)
        assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], qkv)


# ------------------------------------------------------------------------------ host checks
@pytest.mark.parametrize("op", ["rope_and_cache", "decode_gemm_qkv_rope"])
def test_bias_host_checks(op):
    """Wrong dtype, wrong length, a CPU tensor and a misaligned view are refused with a
    message that names the op, and nothing is written."""
    Hq, Hkv, D, M, K, NB = 4, 2, 128, 5, 1024, 2
    N = (Hq + 2 * Hkv) * D
    full, (kc, vc) = _caches(NB, Hkv, D, torch.bfloat16)
    pos = torch.zeros(M, dtype=torch.int32, device=DEV)
    slots = torch.arange(M, dtype=torch.int64, device=DEV)
    qkv = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    good = _bias(Hq + 2 * Hkv, D)

    def call(bias):
        if op == "rope_and_cache":
            ops.hip().rope_and_cache(qkv, pos, _cos_sin(D), slots, kc, vc, Hq, Hkv, True, 1.0, 1.0, bias)
        else:
            x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
            w = torch.zeros(N, K, device=DEV, dtype=torch.bfloat16)
            ops.hip().decode_gemm_qkv_rope(qkv, x, w, torch.empty(4 * M * N, device=DEV), pos, _cos_sin(D), slots,
                                           kc, vc, Hq, Hkv, 1.0, 1.0, bias)

    bad = {"dtype": good.float(), "length": good[:-8].contiguous(), "cpu": good.cpu(),
           "misaligned": torch.cat([good, good])[1: N + 1], "strided": torch.cat([good, good])[::2]}
    for what, b in bad.items():
        with pytest.raises(RuntimeError, match=op):
            call(b)
    torch.cuda.synchronize()
    assert not full[0].view(torch.int16).any() and not full[1].view(torch.int16).any(), "a refused call must not write"
    call(good)


# ----------------------------------------------------------------------------------- runner
COS_BOUND = 0.999   # tests/test_engine_gpu.py test_native_runner_matches_python_forward


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-12))


@functools.lru_cache(maxsize=None)
def _biased_model(name):
    model = LlamaModel(PRESETS[name], device=DEV)
    g = torch.Generator().manual_seed(11)
    for l in model.layers:
        l.qkv_b.copy_((torch.randn(l.qkv_b.numel(), generator=g) * 0.5).to(DEV))
    return model


def _step_inputs(model, nd, npre, seed):
    """One step of nd decode rows (sequence i has ctx 20 + 3 i, blocks 2 i and 2 i + 1, over
    a cache of random earlier tokens) followed by one prefill chunk of npre tokens."""
    cfg = model.cfg
    T = nd + npre
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, cfg.vocab_size, (T,), generator=g, dtype=torch.int32).to(DEV)
    pblocks = (npre + BS - 1) // BS
    nb = 2 * nd + pblocks + 1
    ctx = [20 + 3 * i for i in range(nd)]
    pos = torch.tensor([c - 1 for c in ctx] + list(range(npre)), dtype=torch.int32)
    d_bt = torch.tensor([[2 * i, 2 * i + 1] for i in range(nd)], dtype=torch.int32).reshape(nd, 2)
    p_bt = torch.arange(2 * nd, 2 * nd + pblocks, dtype=torch.int32).reshape(1, -1)
    slots = [int(d_bt[i, (c - 1) // BS]) * BS + (c - 1) % BS for i, c in enumerate(ctx)]
    slots += [int(p_bt[0, t // BS]) * BS + t % BS for t in range(npre)]
    meta = AttnMeta(positions=pos.to(DEV), slots=torch.tensor(slots, dtype=torch.int64, device=DEV), num_decode=nd)
    if nd:
        meta.d_block_tables, meta.d_ctx_lens = d_bt.to(DEV), torch.tensor(ctx, dtype=torch.int32, device=DEV)
        meta.nsplit, meta.blocks_per_split = 1, 2
    if npre:
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

    rows = torch.tensor(sorted({0, T // 2, T - 1} | set(range(min(nd, T)))), dtype=torch.long, device=DEV)
    return ids, meta, caches, rows


@pytest.mark.parametrize("name,nd,npre", [
    ("qwen2-small", 3, 0),      # <= 4 rows: the plain GEMV, then rope_and_cache with the bias
    ("qwen2-small", 8, 0),      # decode_gemm_qkv_rope: the bias in the split-K reduction
    ("qwen2-small", 8, 70),     # mixed step: decode GEMM, then rope_and_cache
    ("qwen2-small", 0, 1100),   # prefill GEMM, then rope_and_cache (16-token tiles below 2049: 2-token)
    ("qwen2-tiny", 8, 0),       # D = 64
], ids=["gemv3", "dgemm8", "mixed8+70", "prefill1100", "tiny-d64-8"])
def test_runner_routes_add_the_bias(name, nd, npre):
    """forward_logits through the native runner against the Python forward of the same
    model (cosine per row above the 0.999 of test_native_runner_matches_python_forward),
    and against the same model with qkv_b zeroed: every row must differ by more than ten
    times that bound (1 - cos > 0.01), so a route that forgets the bias cannot pass."""
    model = _biased_model(name)
    ids, meta, caches, rows = _step_inputs(model, nd, npre, 100 + nd + npre)
    a = model.forward_logits(ids, meta, caches(), rows).float().cpu()
    b = model.logits(model.forward(ids, meta, caches()).index_select(0, rows)).float().cpu()
    saved = [l.qkv_b.clone() for l in model.layers]
    try:
        for l in model.layers:
            l.qkv_b.zero_()
        z = model.forward_logits(ids, meta, caches(), rows).float().cpu()
    finally:
        for l, s in zip(model.layers, saved):
            l.qkv_b.copy_(s)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    same = [_cos(a[i], b[i]) for i in range(len(rows))]
    diff = [_cos(a[i], z[i]) for i in range(len(rows))]
    print(f"runner {name} nd={nd} npre={npre}: min cos(native, python) {min(same):.6f}, "
          f"max cos(bias, zeroed bias) {max(diff):.4f}")
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


def test_engine_graph_decode_matches_eager_with_bias():
    """B = 8, 16 greedy tokens: graph replay against eager on the biased model, as
    test_engine_gpu.py::test_llama_graph_decode_matches_eager (a split only at a near-tie
    of the eager run's top-2, 0.02 nats); and the zeroed-bias model generates other tokens."""
    model = _biased_model("qwen2-small")
    prompts = [list(range(3 + 5 * i, 3 + 5 * i + n)) for i, n in enumerate((5, 9, 33, 40, 64, 65, 100, 130))]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    kw = dict(num_blocks=128, max_model_len=1024, max_batch=8)
    e1 = LLMEngine(model, None, use_graphs=True, **kw)
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
    saved = [l.qkv_b.clone() for l in model.layers]
    try:
        for l in model.layers:
            l.qkv_b.zero_()
        out0 = _run_tops(LLMEngine(model, None, use_graphs=True, **kw), prompts, sp)
    finally:
        for l, s in zip(model.layers, saved):
            l.qkv_b.copy_(s)
    assert all(a[0] != z[0] for a, z in zip(out1, out0)), "the bias did not change the generated tokens"
