"""FP8 (e4m3) paged KV cache on the GPU: the HIP writers against the reference quantiser
bit for bit, the fp8 decode / prefill attention kernels against the fp32 reference over
the dequantised cache, the entry points that must refuse an fp8 cache, and the engine
(native executor with graphs, small-batch GEMV route, chunked prefill, prefix cache)."""
import math

import numpy as np
import pytest
import torch

from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaConfig, LlamaModel, PRESETS
from langstream_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
BS = ops.KV_BLOCK


def _codes(t):
    return t.view(torch.uint8)


def _to_dev(t8):
    """An fp8 CPU tensor on the GPU, moved as bytes."""
    return _codes(t8).to(DEV).view(FP8)


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _cos_sin(D, n=4096):
    return ref.rope_cos_sin(n, D, 500000.0, device=DEV)


# ------------------------------------------------------------------------- write path
def _expected_caches(qkv_out, slots, nb, Hq, Hkv, D, ks, vs):
    """The reference quantiser applied to the kernel's own bf16 qkv rows (CPU)."""
    kr, vr = ops.new_kv_cache(nb, Hkv, D, "cpu", FP8)
    ref.rope_and_cache(qkv_out.cpu().clone(), None, None, slots.cpu(), kr, vr, Hq, Hkv, False, ks, vs)
    return kr, vr


@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.25, 4.0)])
@pytest.mark.parametrize("T,D", [(150, 128), (2600, 128), (37, 64)])
def test_rope_and_cache_fp8_bit_exact(T, D, ks, vs):
    # T <= 2048 takes the 2-token tiles, larger T the 16-token tiles
    torch.manual_seed(5)
    Hq, Hkv = 8, 2
    qkv = (torch.randn(T, (Hq + 2 * Hkv) * D, device=DEV) * 2).to(torch.bfloat16)
    pos = torch.arange(T, device=DEV, dtype=torch.int32) + 7
    cs = _cos_sin(D)
    nb = (T + BS - 1) // BS + 4
    slots = torch.randperm(nb * BS)[:T].to(DEV, torch.int64)
    slots[3] = -1
    kc, vc = ops.new_kv_cache(nb, Hkv, D, DEV, FP8)
    qkv_c = qkv.cpu().clone()
    ops.rope_and_cache(qkv, pos, cs, slots, kc, vc, Hq, Hkv, k_scale=ks, v_scale=vs)
    # the qkv rows are still rotated in place as bf16
    ref.rope_and_cache(qkv_c, pos.cpu(), cs.cpu(), slots.cpu(), *ops.new_kv_cache(nb, Hkv, D, "cpu", torch.bfloat16),
                       Hq, Hkv)
    _close(qkv, qkv_c, 0.03, 0.01, "qkv")
    kr, vr = _expected_caches(qkv, slots, nb, Hq, Hkv, D, ks, vs)
    assert torch.equal(_codes(kc).cpu(), _codes(kr)), "k cache bytes"
    assert torch.equal(_codes(vc).cpu(), _codes(vr)), "v cache bytes"
    assert int((_codes(kc) != 0).any(-1).sum()) == (T - 1) * Hkv


@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.25, 4.0)])
def test_rope_and_cache_fp8_every_bf16_pattern(ks, vs):
    """T = 64, Hkv = 8, D = 128, no RoPE: the V elements enumerate all 65 536 bf16 bit
    patterns.  Non-NaN patterns match the reference quantiser bit for bit; +-Inf store
    +-448; the K elements (randn, wide) are checked the same way."""
    T, Hq, Hkv, D = 64, 8, 8, 128
    torch.manual_seed(9)
    qkv = (torch.randn(T, Hq + 2 * Hkv, D) * 100).to(torch.bfloat16)
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    qkv[:, Hq + Hkv:] = bits[torch.randperm(65536)].view(T, Hkv, D)
    assert qkv[:, Hq + Hkv:].contiguous().view(torch.int16).unique().numel() == 65536
    qkv = qkv.view(T, -1).to(DEV)
    before = qkv.clone()
    pos = torch.zeros(T, device=DEV, dtype=torch.int32)
    nb = 3
    slots = torch.randperm(nb * BS)[:T].to(DEV, torch.int64)
    kc, vc = ops.new_kv_cache(nb, Hkv, D, DEV, FP8)
    ops.rope_and_cache(qkv, pos, _cos_sin(D, 8), slots, kc, vc, Hq, Hkv, apply_rope=False, k_scale=ks, v_scale=vs)
    assert torch.equal(qkv.view(torch.int16), before.view(torch.int16))
    rows = before.cpu().view(T, Hq + 2 * Hkv, D)
    kq = _codes(ref.quantize_kv(rows[:, Hq: Hq + Hkv], ks))
    vq = _codes(ref.quantize_kv(rows[:, Hq + Hkv:], vs))
    vin = rows[:, Hq + Hkv:]
    sl = slots.cpu()
    blk, off = sl // BS, sl % BS
    got_k = _codes(kc).cpu()[blk, :, off]                      # [T, Hkv, D]
    got_v = _codes(vc).cpu()[blk, :, off // 8, :, off % 8]     # [T, Hkv, D]
    assert torch.equal(got_k, kq)
    ok = ~vin.isnan()
    assert int(ok.sum()) == 65536 - 2 * 127
    assert torch.equal(got_v[ok], vq[ok])
    assert (got_v[vin == float("inf")] == 0x7E).all() and (got_v[vin == float("-inf")] == 0xFE).all()
    assert int((vin == float("inf")).sum()) == 1 and int((vin == float("-inf")).sum()) == 1


def _dg_split(tiles, K, min_steps=4):
    best = 1
    for s in range(1, 65):
        if tiles * s > 264 or (K // 64) // s < min_steps:
            break
        best = s
    return best


# (8, 1, 256): K / 64 = 4 k-steps leave no room to split, so S == 1 and the op falls back to
# decode_gemm + rope_and_cache; the other shapes reduce their K splits in the fused kernel.
@pytest.mark.parametrize("M,Hq,Hkv,K,ks,vs", [
    (5, 32, 8, 4096, 1.0, 1.0), (256, 32, 8, 4096, 0.25, 4.0), (100, 64, 8, 8192, 1.0, 1.0),
    (129, 8, 1, 8192, 0.25, 4.0), (17, 8, 1, 256, 0.25, 4.0), (200, 8, 1, 256, 1.0, 1.0)])
def test_decode_gemm_qkv_rope_fp8(M, Hq, Hkv, K, ks, vs):
    torch.manual_seed(M + Hq + K)
    D = 128
    N = (Hq + 2 * Hkv) * D
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K ** 0.5).to(torch.bfloat16)
    pos = torch.randint(0, 4000, (M,), device=DEV, dtype=torch.int32)
    cos_sin = _cos_sin(D)
    NB = 2 * M
    kc, vc = ops.new_kv_cache(NB, Hkv, D, DEV, FP8)
    slots = torch.randperm(NB * BS, device=DEV)[:M].long()
    slots[M // 2] = -1
    qkv = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    wsp = torch.empty(64 * M * N + 4 * 256 * 256, device=DEV, dtype=torch.float32)
    ops.hip().decode_gemm_launch_counts(True)
    ops.hip().decode_gemm_qkv_rope(qkv, x, w, wsp, pos, cos_sin, slots, kc, vc, Hq, Hkv, ks, vs)
    S = min(4, _dg_split(N // 128, K))
    assert (S == 1) == (K == 256)
    census = dict(ops.hip().decode_gemm_launch_counts(True))
    assert len(census) == 1 and ("_partial_" in next(iter(census))) == (S > 1), census
    y = (x.float() @ w.float().t()).view(M, Hq + 2 * Hkv, D)
    cs = cos_sin[pos.long()]
    co, si = cs[:, None, : D // 2], cs[:, None, D // 2:]
    a, b = y[:, : Hq + Hkv, : D // 2], y[:, : Hq + Hkv, D // 2:]
    exp = torch.cat([torch.cat([a * co - b * si, b * co + a * si], -1), y[:, Hq + Hkv:]], 1)
    _close(qkv.view(M, -1, D), exp, 0.03, 0.03, "qkv")
    kr, vr = _expected_caches(qkv, slots, NB, Hq, Hkv, D, ks, vs)
    assert torch.equal(_codes(kc).cpu(), _codes(kr)), "k cache bytes"
    assert torch.equal(_codes(vc).cpu(), _codes(vr)), "v cache bytes"


# -------------------------------------------------------------------------- attention
def _fp8_paged(B, ctx, Hkv, D, seed=0, kmul=1.0):
    """randn caches quantised to fp8 (scale 1 codes), scattered block tables."""
    torch.manual_seed(seed)
    nblk = [(c + BS - 1) // BS for c in ctx]
    NB = sum(nblk) + 3
    kc = ref.quantize_kv(torch.randn(NB, Hkv, BS, D) * kmul)
    vc = ref.quantize_kv(torch.randn(NB, Hkv, BS // 8, D, 8))
    perm = torch.randperm(NB)
    bt = torch.zeros(B, max(nblk), dtype=torch.int32)
    k = 0
    for b in range(B):
        for i in range(nblk[b]):
            bt[b, i] = perm[k]
            k += 1
    return kc, vc, bt


def _decode_case(ctx, Hkv, G, nsplit, min_bps, seed, ks=1.0, vs=1.0, kmul=1.0):
    D = 128
    Hq = Hkv * G
    B = len(ctx)
    kc, vc, bt = _fp8_paged(B, ctx, Hkv, D, seed, kmul)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    q = qkv[:, : Hq * D]
    cl = torch.tensor(ctx, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    ws = torch.empty(B * Hq * nsplit * (D + 2), device=DEV, dtype=torch.float32)
    got = ops.paged_decode_attention(q, _to_dev(kc), _to_dev(vc), bt.to(DEV), cl.to(DEV), scale, nsplit=nsplit,
                                     blocks_per_split=min_bps, workspace=ws, k_scale=ks, v_scale=vs)
    # the reference attends over the dequantised cache (codes.float() * scale)
    exp = ref.paged_decode_attention(q.cpu().reshape(B, Hq, D), kc, vc, bt, cl, scale, ks, vs)
    _close(got, exp.reshape(B, Hq * D), 0.03, 0.03)


@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("nsplit,min_bps", [(1, 4), (3, 4), (3, 1), (16, 1)])
def test_paged_decode_attention_fp8(G, nsplit, min_bps):
    _decode_case([1, 63, 64, 65, 300, 777], 2, G, nsplit, min_bps, seed=G)


@pytest.mark.parametrize("B,sort", [(256, False), (257, True)])
def test_paged_decode_attention_fp8_wave_per_pair(B, sort):
    """B*Hkv >= 2048: one wave per (seq, kv-head); ragged contexts exercise the masked
    tail-block loads through the halved descriptor ranges."""
    ctx = torch.randint(1, 300, (B,), generator=torch.Generator().manual_seed(7)).tolist()
    if sort:
        ctx.sort(reverse=True)
    _decode_case(ctx, 8, 4, 1, 1 << 30, seed=3)


def test_paged_decode_attention_fp8_subnormal_keys():
    # K = 0.02 * randn: most codes are e4m3 subnormals (|x| < 2^-6)
    _decode_case([1, 63, 64, 65, 300, 777], 2, 4, 3, 1, seed=21, kmul=0.02)


@pytest.mark.parametrize("ks,vs", [(0.5, 2.0), (0.3, 1.7)])
def test_paged_decode_attention_fp8_scales(ks, vs):
    _decode_case([1, 63, 64, 65, 300, 777], 2, 4, 3, 1, seed=31, ks=ks, vs=vs)
    _decode_case([1, 63, 64, 65, 300, 777], 2, 8, 1, 4, seed=32, ks=ks, vs=vs)


def _prefill_run(q_lens, prefix, Hkv, G, kc, vc, bt, q, ks=1.0, vs=1.0):
    D = 128
    Hq = Hkv * G
    ctx = [a + b for a, b in zip(q_lens, prefix)]
    starts = [0]
    for n in q_lens[:-1]:
        starts.append(starts[-1] + n)
    qs = torch.tensor(starts, dtype=torch.int32)
    ql = torch.tensor(q_lens, dtype=torch.int32)
    cl = torch.tensor(ctx, dtype=torch.int32)
    tiles = ops.prefill_tiles(q_lens, G, prefix)
    scale = 1 / math.sqrt(D)
    got = ops.paged_prefill_attention(q, _to_dev(kc), _to_dev(vc), bt.to(DEV), qs.to(DEV), ql.to(DEV), cl.to(DEV),
                                      tiles.to(DEV), Hq, scale, k_scale=ks, v_scale=vs)
    exp = ref.paged_prefill_attention(q.cpu(), kc, vc, bt, qs, ql, cl, Hq, scale, ks, vs)
    return got, exp


@pytest.mark.parametrize("G,ks,vs", [(1, 1.0, 1.0), (4, 1.0, 1.0), (8, 1.0, 1.0), (4, 0.5, 2.0), (4, 0.3, 1.7)])
def test_paged_prefill_attention_fp8(G, ks, vs):
    Hkv, D = 2, 128
    q_lens = [1, 17, 64, 130, 200]
    prefix = [0, 5, 64, 0, 300]
    ctx = [a + b for a, b in zip(q_lens, prefix)]
    kc, vc, bt = _fp8_paged(len(q_lens), ctx, Hkv, D, seed=10 + G)
    q = torch.randn(sum(q_lens), (Hkv * G + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    got, exp = _prefill_run(q_lens, prefix, Hkv, G, kc, vc, bt, q, ks, vs)
    _close(got, exp, 0.03, 0.03)


def _all_codes_case():
    """ctx = 1, B = 2, Hkv = 2, D = 128: the first key's V holds, over (b, kvh, d), every
    one of the 256 codes twice (the two NaN codes replaced by 0).  Softmax over one key is
    exactly 1, so the output of every query head is v.float(), exactly."""
    B, Hkv, G, D = 2, 2, 4, 128
    codes = (torch.arange(B * Hkv * D) % 256).to(torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0
    assert codes.unique().numel() == 254
    v = codes.view(B, Hkv, D)
    kc, vc, bt = _fp8_paged(B, [1, 1], Hkv, D, seed=77)
    vb = _codes(vc)
    vb.zero_()
    for b in range(B):
        vb[int(bt[b, 0]), :, 0, :, 0] = v[b]        # key 0 of the sequence's first block
    want = v.view(FP8).float()[:, :, None, :].expand(B, Hkv, G, D).reshape(B, Hkv * G * D)
    q = torch.randn(B, Hkv * G * D, device=DEV, dtype=torch.bfloat16)
    return Hkv, G, D, kc, vc, bt, q, want


@pytest.mark.parametrize("nsplit", [1, 3])
def test_decode_attention_decodes_every_code_exactly(nsplit):
    Hkv, G, D, kc, vc, bt, q, want = _all_codes_case()
    B = 2
    ws = torch.empty(B * Hkv * G * nsplit * (D + 2), device=DEV, dtype=torch.float32)
    got = ops.paged_decode_attention(q, _to_dev(kc), _to_dev(vc), bt.to(DEV),
                                     torch.ones(B, dtype=torch.int32, device=DEV), 1 / math.sqrt(D), nsplit=nsplit,
                                     blocks_per_split=1, workspace=ws, k_scale=1.0, v_scale=1.0)
    assert torch.equal(got.float().cpu(), want)


def test_prefill_attention_decodes_every_code_exactly():
    Hkv, G, D, kc, vc, bt, q, want = _all_codes_case()
    got, _ = _prefill_run([1, 1], [0, 0], Hkv, G, kc, vc, bt, q)
    assert torch.equal(got.float().cpu(), want)


# -------------------------------------------------------------------------- rejections
def test_bf16_only_writers_reject_fp8_caches():
    Hq, Hkv, D, NB = 4, 2, 128, 6
    kc, vc = ops.new_kv_cache(NB, Hkv, D, DEV, FP8)
    N = (Hq + 2 * Hkv) * D
    cos_sin = _cos_sin(D, 512)
    pos = torch.tensor([5, 77], dtype=torch.int32, device=DEV)
    slots = torch.tensor([3, 74], dtype=torch.int64, device=DEV)
    # gemv_qkv
    K = 2048
    w = (torch.randn(N, K, device=DEV) * 0.05).to(torch.bfloat16)
    x = torch.randn(2, K, device=DEV).to(torch.bfloat16)
    out = torch.empty(2, N, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="fp8"):
        ops.hip().gemv_qkv(out, x, w, pos, cos_sin, slots, kc, vc, Hq, Hkv, True, None, None, None, None, 1e-5)
    # paged_decode_attention_rope
    qkv = torch.randn(2, N, device=DEV, dtype=torch.bfloat16)
    bt = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=DEV)
    cl = torch.tensor([4, 11], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="fp8"):
        ops.paged_decode_attention_rope(qkv, pos, cos_sin, slots, kc, vc, bt, cl, 1 / math.sqrt(D), Hq)
    # decode_gemm_qkv_cmb (the LS_DGEMM_FUSED layer)
    M, K = 129, 1024
    S = max(1, ops.hip().decode_gemm_cmb_splits(N, K))
    with pytest.raises(RuntimeError, match="fp8"):
        ops.hip().decode_gemm_qkv_cmb(
            torch.empty(M, N, device=DEV, dtype=torch.bfloat16), torch.randn(M, K, device=DEV).to(torch.bfloat16),
            (torch.randn(N, K, device=DEV) * 0.03).to(torch.bfloat16),
            torch.empty(S * M * N, device=DEV, dtype=torch.float32), torch.zeros(N // 128, device=DEV, dtype=torch.int64),
            torch.ones(M, K // 128, device=DEV), 1e-5, torch.zeros(M, device=DEV, dtype=torch.int32), cos_sin,
            torch.arange(M, device=DEV), kc, vc, Hq, Hkv, torch.zeros(1, device=DEV, dtype=torch.int32))
    # mixed K / V dtypes are refused by the fp8-aware writer too
    with pytest.raises(RuntimeError):
        ops.rope_and_cache(qkv, pos, cos_sin, slots, kc, vc.view(torch.uint8).to(torch.bfloat16), Hq, Hkv)
    torch.cuda.synchronize()
    assert not _codes(kc).any() and not _codes(vc).any(), "a refused call must not write"


# ------------------------------------------------------------------------------ engine
def _run_tops(e, prompts, sp):
    tops = {}
    reqs = [e.submit(p, sp, callback=lambda ev, i=i: tops.setdefault(i, []).append(ev.top))
            for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [(r.output_ids, tops.get(i)) for i, r in enumerate(reqs)]


def _same_or_near_tie(a, b, gap: float = 0.1) -> None:
    """The project's rule for greedy sequences of two bf16 paths: equal over the whole
    length, except that they may part at a genuine near-tie (both tokens in b's top-2,
    within `gap` nats); after such a split they are not compared."""
    (ids_a, _), (ids_b, tops_b) = a, b
    assert len(ids_a) == len(ids_b)
    for t, (x, y) in enumerate(zip(ids_a, ids_b)):
        if x == y:
            continue
        alt = dict(tops_b[t])
        assert x in alt and y in alt and abs(alt[x] - alt[y]) < gap, (t, x, y, tops_b[t])
        return


def _native_vs_python(model, prompts, n_gen, **kw):
    """Native executor (graphs) against the Python executor, both over fp8 caches."""
    from langstream_amd.engine.arena import PyStepExecutor
    from langstream_amd.engine.llm_engine import NSLOTS
    kw = dict(dict(num_blocks=128, max_model_len=1024, max_batch=8, kv_cache_dtype="fp8", kv_k_scale=0.5,
                   kv_v_scale=2.0), **kw)
    sp = SamplingParams(max_tokens=n_gen, temperature=0.0, ignore_eos=True)
    sp_ref = SamplingParams(max_tokens=n_gen, temperature=0.0, ignore_eos=True, logprobs=2)
    e1 = LLMEngine(model, None, **kw)
    assert e1.kv_cache_dtype == "fp8" and all(k.dtype == FP8 and v.dtype == FP8 for k, v in e1.kv_caches)
    out1 = _run_tops(e1, prompts, sp)
    assert e1.stats["graph_steps"] > 0
    assert all(len(ids) == n_gen for ids, _ in out1)
    e2 = LLMEngine(model, None, use_graphs=False, **kw)
    e2.exec = PyStepExecutor(model, e2.kv_caches, e2.layout, NSLOTS, e2.nsplit, e2.bps, e2.device)
    out2 = _run_tops(e2, prompts, sp_ref)
    for a, b in zip(out1, out2):
        _same_or_near_tie(a, b)
    return e1, e2


def test_engine_fp8_native_matches_python_executor():
    model = LlamaModel(PRESETS["llama-small"], device="cuda")
    e1, _ = _native_vs_python(model, [list(range(3, 3 + n)) for n in (5, 33, 64, 65, 200)], 16)
    bf = LLMEngine(model, None, num_blocks=128, max_model_len=1024, max_batch=8)
    assert e1.kv_bytes_per_block * 2 == bf.kv_bytes_per_block


@pytest.mark.parametrize("n", [1, 4])
def test_engine_fp8_batch_le4_gemv_route(n):
    """Decode batches of 1-4 rows on the model of the bf16 batch <= 4 test (dimensions in
    multiples of 512): with fp8 caches the runner takes the un-fused GEMV qkv followed by
    rope_and_cache, not the GEMV whose epilogue writes bf16 K/V."""
    cfg = LlamaConfig(name="llama-gemv", vocab_size=32000, hidden_size=1024, intermediate_size=3072, num_layers=4,
                      num_heads=8, num_kv_heads=2, head_dim=128, max_position=4096, bos_token_id=1, eos_token_ids=(2,))
    model = LlamaModel(cfg, device="cuda")
    prompts = [list(range(3 + 7 * i, 3 + 7 * i + n_tok)) for i, n_tok in enumerate((5, 70, 129, 300)[:n])]
    _native_vs_python(model, prompts, 12)


def test_engine_fp8_chunked_prefill():
    """max_prefill_tokens below the longest prompt: prompts are prefilled in chunks over an
    fp8 prefix, in steps that also carry decode rows."""
    model = LlamaModel(PRESETS["llama-small"], device="cuda")
    e1, e2 = _native_vs_python(model, [list(range(3, 3 + n)) for n in (5, 33, 64, 65, 200)], 16,
                               max_prefill_tokens=96)
    assert e1.stats["mixed_steps"] > 0 and e2.stats["mixed_steps"] > 0


def test_engine_fp8_prefix_cache_matches_no_cache():
    """Prefix KV reuse over fp8 blocks (the byte-based block copy ahead of the forward),
    as test_prefix_cache_native_matches_no_cache does for bf16."""
    model = LlamaModel(PRESETS["llama-small"], device="cuda")
    rng = np.random.default_rng(7)
    head = rng.integers(3, 30000, 150).tolist()
    prompts = [head + rng.integers(3, 30000, int(rng.integers(10, 200))).tolist() for _ in range(12)]
    sp = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)
    sp_ref = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True, logprobs=2)
    kw = dict(num_blocks=256, max_model_len=1024, max_batch=16, max_prefill_tokens=256, kv_cache_dtype="fp8")
    on = LLMEngine(model, None, prefix_cache=True, **kw)
    out_on = _run_tops(on, prompts, sp)
    off = LLMEngine(model, None, prefix_cache=False, **kw)
    out_off = _run_tops(off, prompts, sp_ref)
    for a, b in zip(out_on, out_off):
        _same_or_near_tie(a, b)
    assert on.prefix.stats["hits"] >= 4 and on.stats["prefix_hit_tokens"] >= 4 * 128
    assert off.stats["prefill_tokens"] - on.stats["prefill_tokens"] == on.stats["prefix_hit_tokens"]
    held = sum(len(e.blocks) for e in on.prefix.entries)
    assert on.allocator.num_free() + held == 256
