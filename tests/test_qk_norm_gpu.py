"""The per-head RMSNorm of q and k (Qwen3) in the two kernels that finish a QKV projection
-- rope_and_cache and the split-K reduction of decode_gemm_qkv_rope -- and in every
LlamaRunner route of a model that has it.

Norm weights (``_norm_w``): column c holds (-1)^(c + c // (D/2)) (0.5 + c / 256), times 1.5
for k_norm, rounded to bf16.  The next column and the same column of the other half have
the opposite sign, the magnitudes of one weight are distinct, and k's weight is 1.5 x q's: a
wrong column, the wrong half, or q's weight used on k is off by far more than the bounds.

Inputs: each (token, head) is scaled by a factor cycling through 0.25, 1, 4 (in the GEMM
test each head, on its rows of w), and two heads by 1e-3, where the mean square is of the
size of eps.  After the norm every head has the same scale, so a kernel that skips the
rsqrt, or reduces over the wrong lanes, misses by multiples."""
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
EPS = 1e-6
FACTORS = (0.25, 1.0, 4.0)


# ------------------------------------------------- helpers of tests/test_qkv_bias_gpu.py
def _err(a, b):
    return (a.float().cpu() - b.float().cpu()).abs()


def _close(a, b, atol, rtol=0.0, msg=""):
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


def _norm_w(D, k, device=DEV):
    c = torch.arange(D)
    sign = 1.0 - 2.0 * ((c + c // (D // 2)) % 2)
    return (sign * (0.5 + c / 256.0) * (1.5 if k else 1.0)).to(torch.bfloat16).to(device)


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
_ROPE_CASES = [pytest.param(T, D, Hq, Hkv, f8, False, id=f"{T}-{D}-{Hq}-{Hkv}-{'fp8' if f8 else 'bf16'}")
               for T in (1, 5, 2049)            # 2049: the 16-token tiles, a one-token last tile
               for D in (64, 128)
               for Hq, Hkv in ((4, 2), (9, 3))  # (9, 3): a one-head and a three-head rotate group
               for f8 in (False, True)]
_ROPE_CASES.append(pytest.param(5, 128, 9, 3, False, True, id="5-128-9-3-bf16-bias"))


@pytest.mark.parametrize("T,D,Hq,Hkv,f8,with_bias", _ROPE_CASES)
def test_rope_and_cache_qk_norm(T, D, Hq, Hkv, f8, with_bias):
    """Against ref.rope_and_cache(..., q_norm, k_norm, eps) on a CPU copy with the bounds of
    test_kernels_gpu.py::test_rope_and_cache (0.03 + 0.01 |ref| on qkv and the K cache, V
    exact), the cache contract of test_kv_writers_gpu.py, and against the call without the
    norm: V rows and the V cache bit-identical, q and k different."""
    H = Hq + 2 * Hkv
    NB = (T + BS - 1) // BS + 2
    torch.manual_seed(T + D + Hq)
    x = torch.randn(T, H, D, device=DEV) * 2
    fac = torch.tensor(FACTORS, device=DEV)[torch.arange(T * H, device=DEV) % 3].view(T, H, 1)
    x = x * fac
    x[0, Hq] *= 1e-3 / fac[0, Hq]        # a k head of a cached token
    x[T - 1, 1] *= 1e-3 / fac[T - 1, 1]  # a q head
    qkv0 = x.reshape(T, H * D).to(torch.bfloat16)
    pos = torch.randint(0, 4096, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    slots = _slots(T, NB, T + D)
    if T > 1:
        assert int(slots[0]) >= 0
    qn, kn = _norm_w(D, False), _norm_w(D, True)
    bias = _bias(H, D) if with_bias else None
    dt = FP8 if f8 else torch.bfloat16
    ks, vs = (KS, VS) if f8 else (1.0, 1.0)
    full, (kc, vc) = _caches(NB, Hkv, D, dt)
    qkv = qkv0.clone()
    ops.rope_and_cache(qkv, pos, _cos_sin(D), slots, kc, vc, Hq, Hkv, k_scale=ks, v_scale=vs, bias=bias,
                       q_norm=qn, k_norm=kn, norm_eps=EPS)
    torch.cuda.synchronize()
    # reference on the CPU (it has no upper slot check: the slot past the views reads -1 there)
    qc = qkv0.cpu().clone()
    kr, vr = ops.new_kv_cache(NB + 1, Hkv, D, "cpu", dt)
    sc = slots.cpu().clone()
    sc[sc >= NB * BS] = -1
    ref.rope_and_cache(qc, pos.cpu(), _cos_sin(D).cpu(), sc, kr, vr, Hq, Hkv, True, ks, vs,
                       None if bias is None else bias.cpu(), qn.cpu(), kn.cpu(), EPS)
    e_qkv = _close(qkv, qc, 0.03, 0.01, "qkv")
    v0 = (Hq + Hkv) * D
    assert torch.equal(qkv[:, v0:].cpu(), qc[:, v0:]), "v rows"
    if f8:
        e_k = _err(full[0].float() * KS, kr.float() * KS).max().item()
    else:
        e_k = _close(full[0], kr, 0.03, 0.01, "k cache")
    assert torch.equal(_bits(full[1]).cpu(), _bits(vr)), "v cache"
    _check_caches_hold_rows(full, qkv, slots, NB, Hq, Hkv, D, f8)
    print(f"rope_and_cache qk norm T={T} D={D} H=({Hq},{Hkv}) {'fp8' if f8 else 'bf16'}"
          f"{' bias' if with_bias else ''}: max |qkv - ref| {e_qkv:.4g}, max |K cache - ref| {e_k:.4g}")
    # without the norm: the same V, other q and k
    f2, (k2, v2) = _caches(NB, Hkv, D, dt)
    q2 = qkv0.clone()
    ops.rope_and_cache(q2, pos, _cos_sin(D), slots, k2, v2, Hq, Hkv, k_scale=ks, v_scale=vs, bias=bias)
    assert torch.equal(q2[:, v0:], qkv[:, v0:]) and torch.equal(_bits(f2[1]), _bits(full[1])), "v is not normed"
    a, b = qkv.view(T, H, D).float(), q2.view(T, H, D).float()
    moved = (a[:, : Hq + Hkv] - b[:, : Hq + Hkv]).abs().amax(-1)
    assert bool((moved > 0.1).all()), "a q or k head came out as without the norm"
    if T > 2:
        assert not torch.equal(_bits(f2[0]), _bits(full[0]))


# --------------------------------------------------------------------- decode_gemm_qkv_rope
def _dg_key(M, s):
    """The launch-census key of a 128-column partial-sum tile (test_kernels_gpu.py _dg_key)."""
    return f"bn128_partial_bm{64 if M <= 64 else 128 if M <= 128 else 256}_s{s}"


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("M,Hq,Hkv,D", [(5, 4, 2, 128), (64, 4, 2, 128), (129, 4, 2, 128), (256, 4, 2, 128),
                                        (5, 8, 4, 64)])   # D = 64: decode_gemm + rope_and_cache inside
def test_decode_gemm_qkv_rope_qk_norm(M, Hq, Hkv, D, f8):
    """Against an fp32 projection -> per-head RMSNorm -> rotation in fp32 (0.03 / 0.03, the
    bounds of test_kernels_gpu.py::test_decode_gemm_qkv_rope), the rows in the caches, rows
    with slot -1 (and the slot past the views) not cached, one split-K launch."""
    K, H = 1024, Hq + 2 * Hkv
    N = H * D
    NB = 2 * M // BS + 2
    torch.manual_seed(M + D)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = torch.randn(H, D, K, device=DEV) / K ** 0.5
    fac = torch.tensor(FACTORS, device=DEV)[torch.arange(H, device=DEV) % 3].view(H, 1, 1).clone()
    fac[1], fac[Hq] = 1e-3, 1e-3   # a q head and a k head with a mean square of the size of eps
    w = (w * fac).reshape(N, K).to(torch.bfloat16)
    pos = torch.randint(0, 4000, (M,), device=DEV, dtype=torch.int32)
    slots = _slots(M, NB, M)
    qn, kn = _norm_w(D, False), _norm_w(D, True)
    full, (kc, vc) = _caches(NB, Hkv, D, FP8 if f8 else torch.bfloat16)
    qkv = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    wsp = torch.empty(64 * M * N + 4 * 256 * 256, device=DEV, dtype=torch.float32)
    ops.hip().decode_gemm_launch_counts(True)
    ops.hip().decode_gemm_qkv_rope(qkv, x, w, wsp, pos, _cos_sin(D), slots, kc, vc, Hq, Hkv, KS if f8 else 1.0,
                                   VS if f8 else 1.0, None, qn, kn, EPS)
    # 8 tiles x 4 K slices: the split-K partial-sum GEMM whose reduction applies the norm
    assert dict(ops.hip().decode_gemm_launch_counts(True)) == {_dg_key(M, 4): 1}
    torch.cuda.synchronize()
    y = (x.float() @ w.float().t()).view(M, H, D)
    qk = y[:, : Hq + Hkv]
    wn = torch.stack([qn.float()] * Hq + [kn.float()] * Hkv)
    qk = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + EPS) * wn
    cs = _cos_sin(D)[pos.long()]
    co, si = cs[:, None, : D // 2], cs[:, None, D // 2:]
    a, b = qk[..., : D // 2], qk[..., D // 2:]
    exp = torch.cat([torch.cat([a * co - b * si, b * co + a * si], -1), y[:, Hq + Hkv:]], 1)
    e = _close(qkv.view(M, H, D), exp, 0.03, 0.03, "qkv")
    _check_caches_hold_rows(full, qkv, slots, NB, Hq, Hkv, D, f8)
    print(f"decode_gemm_qkv_rope qk norm M={M} D={D} {'fp8' if f8 else 'bf16'}: max |qkv - fp32| {e:.4g}")
    # without the norm: the same v heads, other q and k heads
    q2 = torch.empty_like(qkv)
    _, (k2, v2) = _caches(NB, Hkv, D, torch.bfloat16)
    ops.hip().decode_gemm_qkv_rope(q2, x, w, wsp, pos, _cos_sin(D), slots, k2, v2, Hq, Hkv, 1.0, 1.0, None)
    v0 = (Hq + Hkv) * D
    assert torch.equal(q2[:, v0:], qkv[:, v0:]), "v is not normed"
    moved = (qkv.view(M, H, D)[:, : Hq + Hkv].float() - q2.view(M, H, D)[:, : Hq + Hkv].float()).abs().amax(-1)
    assert bool((moved > 0.1).all()), "a q or k head came out as without the norm"


# ------------------------------------------------------------------------------ host checks
@pytest.mark.parametrize("op", ["rope_and_cache", "decode_gemm_qkv_rope"])
def test_qk_norm_host_checks(op):
    """Wrong dtype, wrong length, a CPU tensor, a misaligned or strided view, only one of the
    two weights and eps = 0 are refused with a message that names the op, and nothing is
    written; a good call then succeeds."""
    Hq, Hkv, D, M, K, NB = 4, 2, 128, 5, 1024, 2
    N = (Hq + 2 * Hkv) * D
    full, (kc, vc) = _caches(NB, Hkv, D, torch.bfloat16)
    pos = torch.zeros(M, dtype=torch.int32, device=DEV)
    slots = torch.arange(M, dtype=torch.int64, device=DEV)
    qkv = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    good = _norm_w(D, False)

    def call(qn, kn, eps=EPS):
        if op == "rope_and_cache":
            ops.hip().rope_and_cache(qkv, pos, _cos_sin(D), slots, kc, vc, Hq, Hkv, True, 1.0, 1.0, None, qn, kn, eps)
        else:
            x = torch.ones(M, K, device=DEV, dtype=torch.bfloat16)
            w = torch.ones(N, K, device=DEV, dtype=torch.bfloat16)
            ops.hip().decode_gemm_qkv_rope(qkv, x, w, torch.empty(4 * M * N, device=DEV), pos, _cos_sin(D), slots,
                                           kc, vc, Hq, Hkv, 1.0, 1.0, None, qn, kn, eps)

    bad = {"dtype": good.float(), "length": good[:-8].contiguous(), "cpu": good.cpu(),
           "misaligned": torch.cat([good, good])[1: D + 1], "strided": torch.cat([good, good])[::2]}
    for what, b in bad.items():
        with pytest.raises(RuntimeError, match=op):
            call(b, good)
        with pytest.raises(RuntimeError, match=op):
            call(good, b)
    with pytest.raises(RuntimeError, match=op):
        call(good, None)
    with pytest.raises(RuntimeError, match=op):
        call(None, good)
    for eps in (0.0, -1e-6):
        with pytest.raises(RuntimeError, match=op):
            call(good, good, eps)
    torch.cuda.synchronize()
    assert not full[0].view(torch.int16).any() and not full[1].view(torch.int16).any(), "a refused call must not write"
    assert not qkv.view(torch.int16).any(), "a refused call must not write"
    call(good, good)
    torch.cuda.synchronize()
    if op == "decode_gemm_qkv_rope":
        assert full[0].view(torch.int16).any() and full[1].view(torch.int16).any()


def test_runner_host_checks():
    """LlamaRunner refuses norm lists of the wrong length, one list without the other and a
    weight of the wrong size, before any step runs."""
    model = _normed_model("qwen3-tiny")
    L = model.layers
    kv = [ops.new_kv_cache(4, model.hkv, model.cfg.head_dim, DEV, model.dtype) for _ in L]

    def build(qn, kn):
        return ops.hip().LlamaRunner(
            model.embed, [l.qkv_w for l in L], [l.o_w for l in L], [l.gate_up_w for l in L], [l.down_w for l in L],
            [l.in_norm for l in L], [l.post_norm for l in L], model.final_norm, model.lm_head, [c[0] for c in kv],
            [c[1] for c in kv], model.cos_sin, model.hq, model.hkv, model.cfg.head_dim, model.cfg.rms_eps,
            model.scale, model.cfg.vocab_size, 0, None, 1.0, 1.0, None, None, qn, kn)

    qn, kn = [l.q_norm for l in L], [l.k_norm for l in L]
    build(qn, kn)
    build(None, None)
    for a, b in ((qn, None), (None, kn), (qn[:1], kn), (qn, [kn[0], kn[1][:32].contiguous()]),
                 (qn, [kn[0], kn[1].float()])):
        with pytest.raises(RuntimeError, match="LlamaRunner"):
            build(a, b)


# ----------------------------------------------------------------------------------- runner
COS_BOUND = 0.999   # tests/test_engine_gpu.py test_native_runner_matches_python_forward


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-12))


@functools.lru_cache(maxsize=None)
def _normed_model(name):
    """The preset with the CPU's seeded init (rounded to bf16 by the copy) and the weights of
    _norm_w: the model whose fp32 forward tests/test_qk_norm_cpu.py takes the margins from."""
    model = LlamaModel(PRESETS[name], device=DEV)
    model.load_state_dict(LlamaModel(PRESETS[name], device="cpu", dtype=torch.float32).state_dict())
    for l in model.layers:
        l.q_norm.copy_(_norm_w(model.cfg.head_dim, False))
        l.k_norm.copy_(_norm_w(model.cfg.head_dim, True))
    return model


class _ones:
    """The model's norm weights set to ones inside the block."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.saved = [(l.q_norm.clone(), l.k_norm.clone()) for l in self.model.layers]
        for l in self.model.layers:
            l.q_norm.fill_(1.0)
            l.k_norm.fill_(1.0)

    def __exit__(self, *exc):
        for l, (q, k) in zip(self.model.layers, self.saved):
            l.q_norm.copy_(q)
            l.k_norm.copy_(k)


def _step_inputs(model, nd, npre, seed):
    """One step of nd decode rows (sequence i has ctx 20 + 3 i, blocks 2 i and 2 i + 1, over
    a cache of random earlier tokens) followed by one prefill chunk of npre tokens; the
    values of step_inputs in tests/test_qk_norm_cpu.py, whose premise test establishes the
    margin on these rows.  Checked rows: every decode row and the prefill rows at 1/4, 1/2
    and the end of the chunk -- not the chunk's first row, which sees only its own key: its
    attention output is its v whatever q and k are."""
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
        gk = torch.Generator().manual_seed(seed + 1)
        kv = [ops.new_kv_cache(nb, model.hkv, cfg.head_dim, DEV, model.dtype) for _ in range(cfg.num_layers)]
        for kc, vc in kv:
            kc.copy_(torch.randn(kc.shape, generator=gk) * 0.5)
            vc.copy_(torch.randn(vc.shape, generator=gk) * 0.5)
        return kv

    rows = set(range(nd))
    if npre:
        rows |= {nd + npre // 4, nd + npre // 2, T - 1}
    return ids, meta, caches, torch.tensor(sorted(rows), dtype=torch.long, device=DEV)


@pytest.mark.parametrize("name,nd,npre", [
    ("qwen3-small", 3, 0),      # <= 4 rows: the plain GEMV, then rope_and_cache with the norm
    ("qwen3-small", 8, 0),      # decode_gemm_qkv_rope: the norm in the split-K reduction
    ("qwen3-small", 8, 70),     # mixed step: decode GEMM, then rope_and_cache
    ("qwen3-small", 0, 1100),   # prefill GEMM, then rope_and_cache
    ("qwen3-tiny", 8, 0),       # D = 64
], ids=["gemv3", "dgemm8", "mixed8+70", "prefill1100", "tiny-d64-8"])
def test_runner_routes_apply_the_norm(name, nd, npre):
    """forward_logits through the native runner against the Python forward of the same
    model (cosine per row above the 0.999 of test_native_runner_matches_python_forward),
    and against the same model with both norm weights set to ones: every row must have
    1 - cos > 0.01, so a route that forgets the weights cannot pass.  The margin is
    established on the fp32 forward alone by
    test_qk_norm_cpu.py::test_norm_weights_move_every_checked_row (there 0.08 to 0.35)."""
    model = _normed_model(name)
    ids, meta, caches, rows = _step_inputs(model, nd, npre, 100 + nd + npre)
    a = model.forward_logits(ids, meta, caches(), rows).float().cpu()
    b = model.logits(model.forward(ids, meta, caches()).index_select(0, rows)).float().cpu()
    with _ones(model):
        z = model.forward_logits(ids, meta, caches(), rows).float().cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    same = [_cos(a[i], b[i]) for i in range(len(rows))]
    diff = [_cos(a[i], z[i]) for i in range(len(rows))]
    print(f"runner {name} nd={nd} npre={npre}: min cos(native, python) {min(same):.6f}, "
          f"max cos(norm weights, ones) {max(diff):.4f}")
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


ENGINE_LENS = (33, 40, 64, 65, 100, 130, 160, 200)
ENGINE_SEEDS = (14, 5, 36, 38, 16, 26, 28, 4)   # prompt k: the k-th prompt of the stream seeded ENGINE_SEEDS[k]


def _engine_prompts(vocab):
    """Eight prompts of random ids (engine_prompts of tests/test_qk_norm_cpu.py)."""
    out = []
    for k, seed in enumerate(ENGINE_SEEDS):
        g = torch.Generator().manual_seed(seed)
        out.append([torch.randint(5, vocab, (n,), generator=g).tolist() for n in ENGINE_LENS][k])
    return out


def test_engine_graph_decode_matches_eager_with_qk_norm():
    """B = 8, 16 greedy tokens: graph replay against eager on qwen3-small, as
    test_engine_graph_decode_matches_eager_with_bias (a split only at a near-tie of the eager
    run's top-2, 0.02 nats); and the ones-weight model generates other tokens for every prompt.
    On the fp32 forward of the same weights the two models' first tokens for these prompts are
    more than 0.5 nats apart in either model
    (test_qk_norm_cpu.py::test_norm_weights_move_every_engine_prompt)."""
    model = _normed_model("qwen3-small")
    prompts = _engine_prompts(model.cfg.vocab_size)
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
    with _ones(model):
        out0 = _run_tops(LLMEngine(model, None, use_graphs=True, **kw), prompts, sp)
    print("first tokens, norm weights / ones:", [(a[0][0], z[0][0]) for a, z in zip(out1, out0)])
    assert all(a[0][0] != z[0][0] for a, z in zip(out1, out0)), "the norm weights did not change the generated tokens"
