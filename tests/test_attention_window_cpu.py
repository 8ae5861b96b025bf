"""The windowed pointer-query inputs of attention_window_probe.py have teeth (no GPU needed).

For every probe case of test_attention_window_gpu.py this file mutates the windowed
reference -- the window off by one in both directions (leak key lo - 1, drop key lo), drop the
first visited block, leak every PAST target (key 0, the last key of the 8-key group and of
the block before the window among them), plus the tail mutants of test_attention_probe_cpu.py
(drop the last key, leak key n, drop the pointed V group / block, attend the stale slot of a
fused-RoPE step) -- and asserts that the 0.03 + 0.03|ref| criterion rejects every mutant, by
at least 10x the tolerance, on every head whose target the mutant touches.  The unmutated
View reproduces ops.reference with the window argument.
"""
import pytest
import torch

import attention_probe as ap
import attention_window_probe as wp
from attention_probe import IN, PAST, TWO

MARGIN = 10.0


def _excess(a, b, atol=0.03, rtol=0.03):
    """err / tol per element: the GPU tests' _close(a, b, atol, rtol) passes iff max <= 1."""
    a, b = a.float(), b.float()
    return (a - b).abs() / (atol + rtol * b.abs())


def _attend(v, scale, vis):
    """Attention of a View under a per-(row, head) visibility mask [Tq, Hq, Tk]; a head that
    sees no key returns zeros, as the paged reference does."""
    Tq, Hq, D = v.q.shape
    G = Hq // v.Hkv
    s = torch.einsum("qvgd,kvd->qvgk", v.q.reshape(Tq, v.Hkv, G, D), v.K).reshape(Tq, Hq, -1) * scale
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1).nan_to_num(0.0)
    return torch.einsum("qvgk,kvd->qvgd", p.reshape(Tq, v.Hkv, G, -1), v.V).reshape(Tq, Hq, D)


def _mutants(v):
    """(name, visibility [Tq, Hq, Tk], heads whose target it touches [Tq, Hq])."""
    base = wp.visible(v)[:, None, :].expand(-1, v.Hq, -1)
    pos = v.pos[None, None, :]
    tpos = v.pos[v.t]                                    # [Tq, Hq]
    t2pos = torch.where(v.kind == TWO, v.pos[v.t2.clamp(min=0)], tpos)
    n, lo = v.n[:, None], v.lo[:, None]
    pointed = v.kind != PAST
    on = lambda x: (tpos == x) | (t2pos == x)
    # the far edge
    yield "leak_lo_minus_1", base | ((pos == (lo - 1)[..., None]) & (pos >= 0)), (v.kind == PAST) & (tpos == lo - 1)
    yield "drop_lo", base & (pos != lo[..., None]), pointed & on(lo)
    yield "drop_first_block", base & (pos // 64 != (lo // 64)[..., None]), pointed & ((tpos // 64 == lo // 64) |
                                                                                       (t2pos // 64 == lo // 64))
    # the near edge and the tail, as in test_attention_probe_cpu.py
    yield "drop_group", base & (pos // 8 != (tpos // 8)[..., None]), pointed
    yield "drop_block", base & (pos // 64 != (t2pos // 64)[..., None]), pointed
    yield "drop_last", base & (pos != (n - 1)[..., None]), pointed & on(n - 1)
    yield "leak_n", base | (pos == n[..., None]), (v.kind == PAST) & (tpos == n)
    leak = base.clone()
    leak.scatter_(-1, v.t[..., None], True)
    yield "leak_target", leak, v.kind == PAST
    if (v.pos == ap.DECOY).any():      # fused RoPE: the slot is read before it is written
        stale = base.clone()
        stale[..., (v.pos == ap.DECOY).nonzero()[0, 0]] = True
        yield "stale_slot", stale & (pos != (n - 1)[..., None]), (tpos == n - 1) | (tpos == ap.DECOY)


def _check(p, expect, need):
    hits = {}
    row = 0
    for v in p.views:
        Tq = v.q.shape[0]
        want = expect[row: row + Tq].reshape(Tq, v.Hq, -1)
        row += Tq
        base = _attend(v, p.scale, wp.visible(v)[:, None, :].expand(-1, v.Hq, -1))
        assert float(_excess(base, want, 0.01, 0.01).max()) <= 1.0, "the View is not the operator's problem"
        for name, vis, touched in _mutants(v):
            if not touched.any():
                continue
            ex = _excess(_attend(v, p.scale, vis), want).amax(-1)
            worst = float(ex[touched].min())
            assert worst >= MARGIN, f"mutant {name} moves a touched head by only {worst:.2f}x the tolerance"
            hits[name] = hits.get(name, 0) + int(touched.sum())
    assert row == expect.shape[0]
    assert set(need) <= set(hits), f"mutants never exercised: {set(need) - set(hits)}"
    assert p.min_weight >= ap.MIN_WEIGHT
    print(f"W = {p.W}: min single-pointer weight {p.min_weight:.4f}; touched heads per mutant {hits}")


FAR = ["leak_lo_minus_1", "drop_lo", "drop_first_block"]
TAIL = ["drop_group", "drop_block", "drop_last", "leak_n", "leak_target"]


@pytest.mark.parametrize("W", wp.DECODE_W)
@pytest.mark.parametrize("D,G", wp.DECODE_SHAPES)
def test_decode_window_probe_rejects_mutants(D, G, W):
    p = wp.decode_case(D, G, W)
    _check(p, p.expect, FAR + TAIL)
    ins, past = {}, {}
    for v in p.views:
        n = int(v.n[0])
        ins.setdefault(n, set()).update(v.t[v.kind == IN].tolist())
        past.setdefault(n, set()).update(v.t[v.kind == PAST].tolist())
    for n in wp.DECODE_CTX:
        lo = max(0, n - W)
        assert {t for t in (lo, lo + 1, n - 1) if lo <= t < n} <= ins.get(n, set()), n
        assert wp.far_past(lo) | {n, n + 1} <= past[n], n
        if n - lo >= 2:
            assert any(((v.kind == TWO) & (v.t == lo) & (v.t2 == n - 1)).any() for v in p.views if int(v.n[0]) == n)
    lo = max(0, 777 - W)
    assert {t // 64 for t in ins[777]} == set(range(lo // 64, 13))     # every visited block of the longest
    zero = p.expect[(p.ctx == 0).nonzero()[:, 0]]
    assert zero.numel() and not zero.any()


@pytest.mark.parametrize("W", [5, 65])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_window_probe_fp8_rejects_mutants(D, W):
    p = wp.decode_case(D, 4, W, wp.FP8_SCALES)
    _check(p, p.expect, FAR + TAIL)


def test_wave_per_pair_window_probe_rejects_mutants():
    p = wp.wave_per_pair_case()
    assert p.B * p.Hkv >= 2048
    _check(p, p.expect, FAR + TAIL)


@pytest.mark.parametrize("W", wp.ROPE_W)
def test_rope_window_probe_rejects_mutants(W):
    p = wp.rope_case(W)
    need = ["leak_lo_minus_1", "drop_last", "leak_n", "leak_target", "stale_slot"]
    _check(p, p.expect[0], need + (["drop_lo", "drop_first_block", "drop_group", "drop_block"] if W > 1 else []))
    if W == 1:      # no cached key is visible: the step's output is the new token's V
        assert all(int(v.lo[0]) == int(v.n[0]) - 1 for v in p.views)


@pytest.mark.parametrize("W", wp.PREFILL_W)
@pytest.mark.parametrize("D,G", wp.PREFILL_SHAPES)
def test_prefill_window_probe_rejects_mutants(D, G, W):
    # drop_lo / leak_lo_minus_1 of a row are the window mask off by one, `>=` / `> - 1`
    p = wp.prefill_case(D, G, W)
    _check(p, p.expect, ["leak_lo_minus_1", "drop_lo", "drop_last", "leak_n", "drop_group", "drop_block"])
    for v, ql, pre in zip(p.views, wp.PREFILL_LENS, wp.PREFILL_PREFIX):
        # the rows that decide a tile's last KV tile probe both sides of the causal edge ...
        for r in list(range(127, ql * G, 128)) + [ql * G - 1]:
            tp = v.t[r // G] - v.n[r // G]
            assert (tp == -1).any() and (tp == 0).any()
        # ... and the rows that decide its first KV tile both sides of the window's edge
        for r in range(0, ql * G, 128):
            i = r // G
            lo = int(v.lo[i])
            if pre + i - W >= 0:
                assert (v.t[i] == lo).any() and (v.t[i] == lo - 1).any(), (ql, r)
    # prefix 300 under W = 5: the first workgroup starts at KV tile 4
    if W == 5:
        assert max(0, 300 + 0 - W + 1) // 64 == 4


@pytest.mark.parametrize("D", [64, 128])
def test_prefill_window_probe_fp8_rejects_mutants(D):
    p = wp.prefill_case(D, 4, 100, wp.FP8_SCALES)
    _check(p, p.expect, ["leak_lo_minus_1", "drop_lo", "drop_last", "leak_n"])
