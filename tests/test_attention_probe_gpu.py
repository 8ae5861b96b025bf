"""The attention kernels on pointer queries (attention_probe.py): every query head puts
>= 0.9 of its softmax weight on ONE key -- the first or last key of the context, of the last
8-key V group, of the last block, of every block of the longest context -- or on a key just
PAST the context that must not count, so one dropped, leaked or mis-paired key moves the
output by ~|V[t]|, 10x and more beyond the project's tolerance (test_attention_probe_cpu.py
proves that on the reference).  Tolerances are those of test_kernels_gpu.py and
test_kv_fp8_gpu.py: 0.03 + 0.03|ref| on attention outputs against the fp32 reference (over
the dequantised cache for fp8), 0.03 + 0.01|ref| / exact on the K / V caches the fused-RoPE
kernel writes.

Also the compiled variants no other test launches: D = 64 paged decode and prefill (bf16
and fp8), G = 1 and G = 16 decode, ctx_len = 0 rows, LS_ATTN_NT = 0 / 1 (the AUX 0 and
AUX 2 kernels).
"""
import pytest
import torch

import attention_probe as ap
from langstream_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _dev(t):
    """A CPU tensor on the GPU (fp8 moved as bytes)."""
    if t.dtype == ops.FP8_DTYPE:
        return t.view(torch.uint8).to(DEV).view(ops.FP8_DTYPE)
    return t.to(DEV)


def _run_decode(p, nsplit, min_bps):
    ws = torch.empty(p.B * p.Hq * nsplit * (p.D + 2), device=DEV, dtype=torch.float32)
    got = ops.paged_decode_attention(_dev(p.q), _dev(p.kc), _dev(p.vc), _dev(p.bt), _dev(p.ctx), p.scale,
                                     nsplit=nsplit, blocks_per_split=min_bps, workspace=ws, k_scale=p.kv[0],
                                     v_scale=p.kv[1])
    assert not got.isnan().any(), "NaN in the attention output"
    zero = got[_dev(p.ctx) == 0]
    assert zero.numel() == 0 or (zero.isfinite().all() and not zero.any()), "a ctx_len = 0 row must be all zeros"
    _close(got, p.expect, 0.03, 0.03)


@pytest.mark.parametrize("nsplit,min_bps", ap.SPLITS)
@pytest.mark.parametrize("D,G", ap.DECODE_SHAPES)
def test_decode_probe(D, G, nsplit, min_bps):
    p = ap.decode_case(D, G)
    assert int((p.ctx == 0).sum()) >= 1
    _run_decode(p, nsplit, min_bps)


@pytest.mark.parametrize("nt", ["0", "1"])
def test_decode_probe_cache_policies(nt, monkeypatch):
    """LS_ATTN_NT (read per launch) = 0 / 1: the all-cached and all-nt kernels; the default
    (nt except a sequence's first block) is what every other test runs."""
    monkeypatch.setenv("LS_ATTN_NT", nt)
    _run_decode(ap.decode_case(128, 4), 3, 1)
    _run_decode(ap.decode_case(64, 4), 1, 4)


def test_decode_probe_wave_per_pair():
    """B * Hkv >= 2048: one wave per (seq, kv-head); 256 ragged rows on 32 shared block
    tables, so the keys past each row's context are another row's live keys."""
    p = ap.wave_per_pair_case()
    assert p.B * p.Hkv >= 2048
    _run_decode(p, 1, 1 << 30)


@pytest.mark.parametrize("ks,vs", ap.FP8_SCALES)
@pytest.mark.parametrize("nsplit,min_bps", [(1, 4), (3, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_probe_fp8(D, nsplit, min_bps, ks, vs):
    _run_decode(ap.decode_case(D, 4, (ks, vs)), nsplit, min_bps)


@pytest.mark.parametrize("nsplit,min_bps", [(1, 4), (3, 1)])
def test_decode_rope_probe(nsplit, min_bps):
    """Heads point at the new token (seeded into the online softmax from registers), at the
    last cached key n - 2, into every cached block, at both (two-pointer), and at the stale
    key in the slot being overwritten, which must not be read before the write."""
    p = ap.rope_case()
    exp, kr, vr = p.expect
    kc, vc, qkv = _dev(p.kc.clone()), _dev(p.vc.clone()), _dev(p.qkv)
    qkv_before = qkv.clone()
    ws = torch.empty(p.B * p.Hq * nsplit * (p.D + 2), device=DEV, dtype=torch.float32)
    got = ops.paged_decode_attention_rope(qkv, _dev(p.pos), _dev(p.cos_sin), _dev(p.slots), kc, vc, _dev(p.bt),
                                          _dev(p.ctx), p.scale, p.Hq, nsplit=nsplit, blocks_per_split=min_bps,
                                          workspace=ws)
    assert not got.isnan().any()
    _close(got, exp, 0.03, 0.03, "attention")
    _close(kc, kr, 0.03, 0.01, "k cache")
    _close(vc, vr, 0.0, 0.0, "v cache")
    assert torch.equal(qkv, qkv_before), "the fused kernel must not modify the projection rows"


def _run_prefill(p):
    got = ops.paged_prefill_attention(_dev(p.q), _dev(p.kc), _dev(p.vc), _dev(p.bt), _dev(p.q_start), _dev(p.q_len),
                                      _dev(p.ctx), _dev(p.tiles), p.Hq, p.scale, k_scale=p.kv[0], v_scale=p.kv[1])
    assert not got.isnan().any()
    _close(got, p.expect, 0.03, 0.03)


@pytest.mark.parametrize("D,G", ap.PREFILL_SHAPES)
def test_prefill_probe(D, G):
    _run_prefill(ap.prefill_case(D, G))


@pytest.mark.parametrize("ks,vs", ap.FP8_SCALES)
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_probe_fp8(D, ks, vs):
    _run_prefill(ap.prefill_case(D, 4, (ks, vs)))


@pytest.mark.parametrize("D,H", ap.ENCODER_SHAPES)
def test_encoder_probe(D, H):
    p = ap.encoder_case(D, H)
    got = ops.varlen_encoder_attention(_dev(p.qkv), _dev(p.q_start), _dev(p.q_len), _dev(p.tiles), H, H, p.scale)
    assert not got.isnan().any()
    _close(got, p.expect, 0.03, 0.03)
