"""The paged-KV write contract (ops/csrc/kv_write.h), checked the same way for every kernel
that files a new token's K and V: which slots are skipped, where a row lands and what it
holds; and the host check that the caches have the head count the caller names."""
from __future__ import annotations

import functools
import math

import pytest
import torch

from langstream_amd import ops
from langstream_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
BS = ops.KV_BLOCK
Hq, Hkv, D, NB = 4, 2, 128, 4
N = (Hq + 2 * Hkv) * D
KS, VS = 0.25, 4.0   # scales of the fp8 cases


@functools.lru_cache(maxsize=None)
def _cos_sin():
    return ref.rope_cos_sin(512, D, 500000.0, device=DEV)


def _caches(dtype, hkv=Hkv):
    """Zeroed caches of NB + 1 blocks and the NB-block views the writers get: slot NB * BS,
    one past the views' end, still lies inside the allocation."""
    full = ops.new_kv_cache(NB + 1, hkv, D, DEV, dtype)
    return full, tuple(c.narrow(0, 0, NB) for c in full)


def _slots(T, seed):
    """Distinct valid slots, one -1 and one NB * BS."""
    s = torch.randperm(NB * BS, generator=torch.Generator().manual_seed(seed))[:T].to(torch.int64)
    s[T // 2] = -1
    s[T - 1] = NB * BS
    return s.to(DEV)


def _pos(T, seed):
    return torch.randint(0, 512, (T,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(DEV)


def _xw(M, K, seed):
    torch.manual_seed(seed)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K ** 0.5).to(torch.bfloat16)
    return x, w


# Each writer fills the cache views and returns (its qkv output rows [T, N], slots).
def _rope_and_cache(kc, vc, f8):
    T = 5
    torch.manual_seed(1)
    qkv = (torch.randn(T, N, device=DEV) * 2).to(torch.bfloat16)
    slots = _slots(T, 1)
    ops.rope_and_cache(qkv, _pos(T, 1), _cos_sin(), slots, kc, vc, Hq, Hkv, k_scale=KS if f8 else 1.0,
                       v_scale=VS if f8 else 1.0)
    return qkv, slots


def _gemv_qkv(kc, vc, f8):
    T, K = 3, 1024
    x, w = _xw(T, K, 2)
    out = torch.empty(T, N, device=DEV, dtype=torch.bfloat16)
    slots = _slots(T, 2)
    ops.hip().gemv_qkv(out, x, w, _pos(T, 2), _cos_sin(), slots, kc, vc, Hq, Hkv, True, None, None, None, None, 1e-5)
    return out, slots


def _decode_gemm_qkv_rope(kc, vc, f8):
    M, K = 5, 1024   # 8 tiles x 4 K splits: the fused split-K reduce kernel runs
    x, w = _xw(M, K, 3)
    qkv = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    wsp = torch.empty(4 * M * N, device=DEV, dtype=torch.float32)
    slots = _slots(M, 3)
    ops.hip().decode_gemm_launch_counts(True)
    ops.hip().decode_gemm_qkv_rope(qkv, x, w, wsp, _pos(M, 3), _cos_sin(), slots, kc, vc, Hq, Hkv,
                                   KS if f8 else 1.0, VS if f8 else 1.0)
    assert dict(ops.hip().decode_gemm_launch_counts(True)) == {"bn128_partial_bm64_s4": 1}
    return qkv, slots


def _cmb_args(M, K, seed):
    x, w = _xw(M, K, seed)
    S = ops.hip().decode_gemm_cmb_splits(N, K)
    assert S >= 1
    parts = torch.full((M, K // 128), 128.0, device=DEV)
    return (x, w, torch.empty(S * M * N, device=DEV, dtype=torch.float32),
            torch.zeros(N // 128, device=DEV, dtype=torch.int64), parts)


def _decode_gemm_qkv_cmb(kc, vc, f8):
    M, K = 129, 1024
    x, w, ws, cnt, parts = _cmb_args(M, K, 4)
    qkv = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    slots = _slots(M, 4)
    ops.hip().decode_gemm_qkv_cmb(qkv, x, w, ws, cnt, parts, 1e-5, _pos(M, 4), _cos_sin(), slots, kc, vc, Hq, Hkv,
                                  err)
    assert err.item() == 0
    return qkv, slots


def _attention_rope(kc, vc, f8):
    """The fused attention leaves qkv alone: its rows are those rope_and_cache makes of a
    copy of the inputs."""
    ctx = [1, 65, 130]
    B = len(ctx)
    torch.manual_seed(5)
    qkv = torch.randn(B, N, device=DEV, dtype=torch.bfloat16)
    bt = torch.tensor([[0, 1, 2], [1, 2, 3], [3, 0, 1]], dtype=torch.int32, device=DEV)
    cl = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    pos = cl - 1
    slots = _slots(B, 5)
    ops.paged_decode_attention_rope(qkv, pos, _cos_sin(), slots, kc, vc, bt, cl, 1 / math.sqrt(D), Hq)
    rows = qkv.clone()
    _, (kc2, vc2) = _caches(torch.bfloat16)
    ops.rope_and_cache(rows, pos, _cos_sin(), slots, kc2, vc2, Hq, Hkv)
    return rows, slots


@pytest.mark.parametrize("writer,f8", [
    (_rope_and_cache, False), (_rope_and_cache, True), (_gemv_qkv, False), (_decode_gemm_qkv_rope, False),
    (_decode_gemm_qkv_rope, True), (_decode_gemm_qkv_cmb, False), (_attention_rope, False)],
    ids=["rope_and_cache-bf16", "rope_and_cache-fp8", "gemv_qkv", "decode_gemm_qkv_rope-bf16",
         "decode_gemm_qkv_rope-fp8", "decode_gemm_qkv_cmb", "paged_decode_attention_rope"])
def test_every_writer_skips_the_same_slots(writer, f8):
    """Slots -1 and NB * BS (one past the end) are skipped; every other token's K row and
    V^T column hold the k / v heads of the writer's own qkv row bit for bit (fp8: their
    ops.reference codes); nothing else is written, the block past the views included."""
    full, (kc, vc) = _caches(FP8 if f8 else torch.bfloat16)
    rows, slots = writer(kc, vc, f8)
    torch.cuda.synchronize()
    bits = (lambda t: t.view(torch.uint8)) if f8 else (lambda t: t.view(torch.int16))
    kfull, vfull = bits(full[0]).cpu(), bits(full[1]).cpu()
    assert not kfull[NB].any() and not vfull[NB].any(), "the block past the end was written"
    r = rows.cpu().view(-1, Hq + 2 * Hkv, D)
    k, v = r[:, Hq: Hq + Hkv], r[:, Hq + Hkv:]
    if f8:
        k, v = ref.quantize_kv(k, KS), ref.quantize_kv(v, VS)
    ek, ev = torch.zeros_like(kfull), torch.zeros_like(vfull)
    written = torch.zeros(NB + 1, Hkv, BS, dtype=torch.bool)
    nvalid = 0
    for t, s in enumerate(slots.tolist()):
        if 0 <= s < NB * BS:
            blk, off = divmod(s, BS)
            ek[blk, :, off] = bits(k[t].contiguous())
            ev[blk, :, off // 8, :, off % 8] = bits(v[t].contiguous())
            written[blk, :, off] = True
            nvalid += 1
    assert nvalid == len(slots) - 2
    assert torch.equal((kfull != 0).any(-1), written), "K rows written"
    assert torch.equal(kfull, ek), "k cache bits"
    assert torch.equal(vfull, ev), "v cache bits"


@pytest.mark.parametrize("op", ["decode_gemm_qkv_rope", "decode_gemm_qkv_cmb"])
def test_wrong_head_count_is_refused(op):
    """Caches built for Hkv + 1 heads with Hkv passed: refused, and nothing is written."""
    full, (kc, vc) = _caches(torch.bfloat16, Hkv + 1)
    if op == "decode_gemm_qkv_rope":
        M, K = 5, 1024
        x, w = _xw(M, K, 6)
        args = (torch.empty(M, N, device=DEV, dtype=torch.bfloat16), x, w,
                torch.empty(4 * M * N, device=DEV, dtype=torch.float32), _pos(M, 6), _cos_sin(), _slots(M, 6), kc, vc,
                Hq, Hkv, 1.0, 1.0)
    else:
        M, K = 129, 1024
        x, w, ws, cnt, parts = _cmb_args(M, K, 7)
        args = (torch.empty(M, N, device=DEV, dtype=torch.bfloat16), x, w, ws, cnt, parts, 1e-5, _pos(M, 7),
                _cos_sin(), _slots(M, 7), kc, vc, Hq, Hkv, torch.zeros(1, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        getattr(ops.hip(), op)(*args)
    torch.cuda.synchronize()
    assert not full[0].view(torch.int16).any() and not full[1].view(torch.int16).any(), "a refused call must not write"
