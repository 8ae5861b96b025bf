"""Sliding-window attention in the paged kernels, on the pointer queries of
attention_window_probe.py: every head puts >= 0.9 of its softmax weight on ONE key -- the
first key of the window (lo), lo + 1, the last key, a key of every visited block -- or on a
key that must not count: lo - 1, the last key of the 8-key group and of the block before the
window, key 0, keys n and n + 1.  One key leaked or dropped at either edge moves the output
by ~|V[t]|, 10x and more beyond the tolerance (test_attention_window_cpu.py proves that on the
reference).  Criterion: 0.03 + 0.03|ref| against the fp32 reference with the same window, as
in test_attention_probe_gpu.py; 0.03 + 0.01|ref| / exact on the K / V caches the fused-RoPE
kernel writes.  A window that covers the whole context must give the bits of window = 0.
"""
import pytest
import torch

import attention_probe as ap
import attention_window_probe as wp
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


def _decode(p, nsplit, min_bps, window):
    ws = torch.empty(p.B * p.Hq * nsplit * (p.D + 2), device=DEV, dtype=torch.float32)
    return ops.paged_decode_attention(_dev(p.q), _dev(p.kc), _dev(p.vc), _dev(p.bt), _dev(p.ctx), p.scale,
                                      nsplit=nsplit, blocks_per_split=min_bps, workspace=ws, k_scale=p.kv[0],
                                      v_scale=p.kv[1], window=window)


def _run_decode(p, nsplit, min_bps):
    got = _decode(p, nsplit, min_bps, p.W)
    assert not got.isnan().any(), "NaN in the attention output"
    zero = got[_dev(p.ctx) == 0]
    assert zero.numel() == 0 or (zero.isfinite().all() and not zero.any()), "a ctx_len = 0 row must be all zeros"
    _close(got, p.expect, 0.03, 0.03)


@pytest.mark.parametrize("nsplit,min_bps", wp.SPLITS)
@pytest.mark.parametrize("W", wp.DECODE_W)
@pytest.mark.parametrize("D,G", wp.DECODE_SHAPES)
def test_decode_window_probe(D, G, W, nsplit, min_bps):
    p = wp.decode_case(D, G, W)
    assert int((p.ctx == 0).sum()) >= 1
    _run_decode(p, nsplit, min_bps)


@pytest.mark.parametrize("nsplit,min_bps", [(1, 4), (3, 1)])
@pytest.mark.parametrize("W", [5, 65])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_window_probe_fp8(D, W, nsplit, min_bps):
    _run_decode(wp.decode_case(D, 4, W, wp.FP8_SCALES), nsplit, min_bps)


@pytest.mark.parametrize("nt", ["0", "1"])
def test_decode_window_probe_cache_policies(nt, monkeypatch):
    """LS_ATTN_NT (read per launch) = 0 / 1: the all-cached and all-nt kernels; the default
    (nt except block 0 of the table, which a window may never visit) is what the others run."""
    monkeypatch.setenv("LS_ATTN_NT", nt)
    _run_decode(wp.decode_case(128, 4, 65), 3, 1)
    _run_decode(wp.decode_case(64, 1, 200), 1, 4)


def test_decode_window_probe_wave_per_pair():
    """B * Hkv >= 2048: one wave per (seq, kv-head), 256 ragged rows on 32 shared tables."""
    p = wp.wave_per_pair_case()
    assert p.B * p.Hkv >= 2048 and p.W == 70
    _run_decode(p, 1, 1 << 30)


@pytest.mark.parametrize("nsplit,min_bps", [(1, 4), (3, 1)])
@pytest.mark.parametrize("W", wp.ROPE_W)
def test_decode_rope_window_probe(W, nsplit, min_bps):
    """The new token is key n - 1, seen from registers; the cached keys are lo .. n - 2.  At
    W = 1 no cached key is read and the owner wave still writes K / V (the cache checks)."""
    p = wp.rope_case(W)
    exp, kr, vr = p.expect
    kc, vc, qkv = _dev(p.kc.clone()), _dev(p.vc.clone()), _dev(p.qkv)
    qkv_before = qkv.clone()
    ws = torch.empty(p.B * p.Hq * nsplit * (p.D + 2), device=DEV, dtype=torch.float32)
    got = ops.paged_decode_attention_rope(qkv, _dev(p.pos), _dev(p.cos_sin), _dev(p.slots), kc, vc, _dev(p.bt),
                                          _dev(p.ctx), p.scale, p.Hq, nsplit=nsplit, blocks_per_split=min_bps,
                                          workspace=ws, window=W)
    assert not got.isnan().any()
    _close(got, exp, 0.03, 0.03, "attention")
    _close(kc, kr, 0.03, 0.01, "k cache")
    _close(vc, vr, 0.0, 0.0, "v cache")
    assert torch.equal(qkv, qkv_before), "the fused kernel must not modify the projection rows"


def _prefill(p, window):
    return ops.paged_prefill_attention(_dev(p.q), _dev(p.kc), _dev(p.vc), _dev(p.bt), _dev(p.q_start), _dev(p.q_len),
                                       _dev(p.ctx), _dev(p.tiles), p.Hq, p.scale, k_scale=p.kv[0], v_scale=p.kv[1],
                                       window=window)


@pytest.mark.parametrize("W", wp.PREFILL_W)
@pytest.mark.parametrize("D,G", wp.PREFILL_SHAPES)
def test_prefill_window_probe(D, G, W):
    """Prefix 300 under W = 5 starts at KV tile 4; W = 129 spans a 128-row tile."""
    p = wp.prefill_case(D, G, W)
    got = _prefill(p, W)
    assert not got.isnan().any()
    _close(got, p.expect, 0.03, 0.03)


def test_prefill_window_probe_fp8():
    p = wp.prefill_case(128, 4, 100, wp.FP8_SCALES)
    got = _prefill(p, 100)
    assert not got.isnan().any()
    _close(got, p.expect, 0.03, 0.03)


# ------------------------------------------------------- a window that covers the context
@pytest.mark.parametrize("nsplit,min_bps", wp.SPLITS)
def test_decode_covering_window_is_bit_equal_to_no_window(nsplit, min_bps):
    p = ap.decode_case(128, 4)                    # ctx up to 777
    full = _decode(p, nsplit, min_bps, 0)
    for W in (777, 778, 1 << 20):
        assert torch.equal(_decode(p, nsplit, min_bps, W), full), W
    f8 = ap.decode_case(64, 4, (0.25, 4.0))
    assert torch.equal(_decode(f8, nsplit, min_bps, 777), _decode(f8, nsplit, min_bps, 0))


def test_decode_rope_covering_window_is_bit_equal_to_no_window():
    p = ap.rope_case()
    outs = []
    for W in (0, 777, 1 << 20):
        kc, vc = _dev(p.kc.clone()), _dev(p.vc.clone())
        ws = torch.empty(p.B * p.Hq * 3 * (p.D + 2), device=DEV, dtype=torch.float32)
        got = ops.paged_decode_attention_rope(_dev(p.qkv), _dev(p.pos), _dev(p.cos_sin), _dev(p.slots), kc, vc,
                                              _dev(p.bt), _dev(p.ctx), p.scale, p.Hq, nsplit=3, blocks_per_split=1,
                                              workspace=ws, window=W)
        outs.append((got, kc, vc))
    for got, kc, vc in outs[1:]:
        assert torch.equal(got, outs[0][0]) and torch.equal(kc, outs[0][1]) and torch.equal(vc, outs[0][2])


@pytest.mark.parametrize("D,G", [(64, 1), (128, 8)])
def test_prefill_covering_window_is_bit_equal_to_no_window(D, G):
    p = ap.prefill_case(D, G)                     # contexts up to 500
    full = _prefill(p, 0)
    for W in (500, 501, 1 << 20):
        assert torch.equal(_prefill(p, W), full), W


# ------------------------------------------------------------------- arguments and bindings
def test_negative_windows_are_refused():
    p = ap.decode_case(128, 4)
    with pytest.raises(ValueError):
        _decode(p, 1, 4, -1)
    with pytest.raises(ValueError):
        _prefill(ap.prefill_case(128, 4), -1)
    r = ap.rope_case()
    with pytest.raises(ValueError):
        ops.paged_decode_attention_rope(_dev(r.qkv), _dev(r.pos), _dev(r.cos_sin), _dev(r.slots), _dev(r.kc.clone()),
                                        _dev(r.vc.clone()), _dev(r.bt), _dev(r.ctx), r.scale, r.Hq, window=-1)
    # the native entry points refuse them too, and take the window by keyword or position
    h = ops.hip()
    out = torch.empty(p.B, p.Hq * p.D, device=DEV, dtype=torch.bfloat16)
    ws = torch.empty(0, device=DEV, dtype=torch.float32)
    args = (out, _dev(p.q), _dev(p.kc), _dev(p.vc), _dev(p.bt), _dev(p.ctx), p.scale, 1, 4, ws)
    with pytest.raises(RuntimeError, match="window"):
        h.paged_decode_attention(*args, window=-1)
    h.paged_decode_attention(*args)                       # the old call, positional, still works
    a = out.clone()
    h.paged_decode_attention(*args, 1.0, 1.0, 0)
    assert torch.equal(out, a)
    w = wp.decode_case(128, 4, 5)
    out_w = torch.empty(w.B, w.Hq * w.D, device=DEV, dtype=torch.bfloat16)
    h.paged_decode_attention(out_w, _dev(w.q), _dev(w.kc), _dev(w.vc), _dev(w.bt), _dev(w.ctx), w.scale, 1, 4, ws,
                             1.0, 1.0, 5)
    _close(out_w, w.expect, 0.03, 0.03)
