"""The pointer-query inputs of attention_probe.py have teeth (no GPU needed).

The attention tests with randn inputs cannot see one wrong key: on the exact inputs of
test_paged_decode_attention (G = 4, seed = G, ctx 777) a reference that drops the last
valid key is accepted by the project's 0.03 + 0.03|ref| criterion
(test_randn_inputs_accept_a_dropped_key keeps that on record).  For every probe case of
test_attention_probe_gpu.py this file mutates the reference -- drop the last key, leak key
n, drop the pointed 8-key V group, drop the pointed block, causal off-by-one in both
directions (drop_last / leak_n of a prefill row), leak a neighbouring sequence's token
(encoder), attend the stale slot instead of the new token (fused RoPE), leak each PAST
target -- and asserts that the same criterion rejects every mutant, by at least 10x the
tolerance, on every head whose target the mutant touches.
"""
import math

import pytest
import torch

import attention_probe as ap
from attention_probe import IN, PAST, TWO
from langstream_amd.ops import reference as ref

MARGIN = 10.0


def _excess(a, b, atol=0.03, rtol=0.03):
    """err / tol per element: _close(a, b, atol, rtol) of the GPU tests passes iff max <= 1."""
    a, b = a.float(), b.float()
    return (a - b).abs() / (atol + rtol * b.abs())


def _attend(v, scale, vis):
    """ops.reference.attention of a View with a per-(row, head) visibility mask
    [Tq, Hq, Tk]; a head that sees no key returns zeros, as the paged reference does."""
    Tq, Hq, D = v.q.shape
    G = Hq // v.Hkv
    s = torch.einsum("qvgd,kvd->qvgk", v.q.reshape(Tq, v.Hkv, G, D), v.K).reshape(Tq, Hq, -1) * scale
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1).nan_to_num(0.0)
    return torch.einsum("qvgk,kvd->qvgd", p.reshape(Tq, v.Hkv, G, -1), v.V).reshape(Tq, Hq, D)


def _mutants(v):
    """(name, visibility [Tq, Hq, Tk], heads whose target it touches [Tq, Hq])."""
    base = ap.base_visible(v)[:, None, :].expand(-1, v.Hq, -1)
    pos = v.pos[None, None, :]
    tpos = v.pos[v.t]                                    # [Tq, Hq]
    t_blk = torch.where(v.kind == TWO, v.pos[v.t2.clamp(min=0)], tpos)
    n = v.n[:, None]
    pointed = v.kind != PAST
    yield "drop_group", base & (pos // 8 != (tpos // 8)[..., None]), pointed
    yield "drop_block", base & (pos // 64 != (t_blk // 64)[..., None]), pointed
    yield "drop_last", base & (pos != (n - 1)[..., None]), pointed & ((tpos == n - 1) | (t_blk == n - 1))
    yield "leak_n", base | (pos == n[..., None]), (v.kind == PAST) & (tpos == n)
    leak = base.clone()
    leak.scatter_(-1, v.t[..., None], True)
    yield "leak_target", leak, v.kind == PAST
    if (v.pos == ap.DECOY).any():      # fused RoPE: the slot is read before it is written
        stale = base.clone()
        stale[..., (v.pos == ap.DECOY).nonzero()[0, 0]] = True
        yield "stale_slot", stale & (pos != (n - 1)[..., None]), (tpos == n - 1) | (tpos == ap.DECOY)


def _check_views(p, expect, hits):
    """Per View: the un-mutated mask reproduces ops.reference (`expect` rows in View order),
    every mutant is rejected on every head it touches."""
    row = 0
    for v in p.views:
        Tq = v.q.shape[0]
        want = expect[row: row + Tq].reshape(Tq, v.Hq, -1)
        row += Tq
        base = _attend(v, p.scale, ap.base_visible(v)[:, None, :].expand(-1, v.Hq, -1))
        assert float(_excess(base, want, 0.01, 0.01).max()) <= 1.0, "the View is not the operator's problem"
        for name, vis, touched in _mutants(v):
            if not touched.any():
                continue
            ex = _excess(_attend(v, p.scale, vis), want).amax(-1)
            worst = float(ex[touched].min())
            assert worst >= MARGIN, f"mutant {name} moves a touched head by only {worst:.2f}x the tolerance"
            hits[name] = hits.get(name, 0) + int(touched.sum())
    assert row == expect.shape[0]


def _check(p, expect, need):
    hits = {}
    _check_views(p, expect, hits)
    assert set(need) <= set(hits), f"mutants never exercised: {set(need) - set(hits)}"
    assert p.min_weight >= ap.MIN_WEIGHT
    print(f"min single-pointer weight {p.min_weight:.4f}; touched heads per mutant {hits}")


PAGED = ["drop_group", "drop_block", "drop_last", "leak_n", "leak_target"]


@pytest.mark.parametrize("D,G", ap.DECODE_SHAPES)
def test_decode_probe_rejects_mutants(D, G):
    p = ap.decode_case(D, G)
    _check(p, p.expect, PAGED)
    # every context length, and every block of the longest one, carries a pointed key
    ins = {}
    for v in p.views:
        ins.setdefault(int(v.n[0]), set()).update(v.t[v.kind == IN].tolist())
    for n in ap.DECODE_CTX:
        must = {t for t in (0, n - 1, n - 2, 8 * ((n - 1) // 8), 64 * ((n - 1) // 64), 63, 64) if 0 <= t < n}
        assert must <= ins.get(n, set()), (n, must - ins.get(n, set()))
    assert {t // 64 for t in ins[777]} == set(range(13))
    zero = p.expect[(p.ctx == 0).nonzero()[:, 0]]
    assert zero.numel() and not zero.any()


@pytest.mark.parametrize("ks,vs", ap.FP8_SCALES)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_probe_fp8_rejects_mutants(D, ks, vs):
    p = ap.decode_case(D, 4, (ks, vs))
    _check(p, p.expect, PAGED)


def test_wave_per_pair_probe_rejects_mutants():
    p = ap.wave_per_pair_case()
    assert p.B * p.Hkv >= 2048
    _check(p, p.expect, PAGED)


def test_rope_probe_rejects_mutants():
    p = ap.rope_case()
    _check(p, p.expect[0], ["drop_group", "drop_block", "drop_last", "leak_n", "leak_target", "stale_slot"])


@pytest.mark.parametrize("D,G", ap.PREFILL_SHAPES)
def test_prefill_probe_rejects_mutants(D, G):
    # drop_last / leak_n of a row are the causal mask off by one, `<` / `<= + 1`
    p = ap.prefill_case(D, G)
    _check(p, p.expect, ["drop_group", "drop_block", "drop_last", "leak_n"])
    for v, ql in zip(p.views, ap.PREFILL_LENS):      # the rows that decide a tile's kmax probe both sides
        for r in list(range(127, ql * G, 128)) + [ql * G - 1]:
            tp = v.t[r // G] - v.n[r // G]
            assert (tp == -1).any() and (tp == 0).any()


@pytest.mark.parametrize("ks,vs", ap.FP8_SCALES)
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_probe_fp8_rejects_mutants(D, ks, vs):
    p = ap.prefill_case(D, 4, (ks, vs))
    _check(p, p.expect, ["drop_group", "drop_block", "drop_last", "leak_n"])


@pytest.mark.parametrize("D,H", ap.ENCODER_SHAPES)
def test_encoder_probe_rejects_mutants(D, H):
    # leak_n: the next sequence's first token; leak_target also covers the previous one's last
    p = ap.encoder_case(D, H)
    _check(p, p.expect, ["drop_group", "drop_block", "drop_last", "leak_n", "leak_target"])
    assert any(((v.kind == PAST) & (v.pos[v.t] == ap.PREV)).any() for v in p.views)


def test_randn_inputs_accept_a_dropped_key():
    """Why this file exists: the inputs of test_paged_decode_attention (G = 4, seed = G),
    row ctx = 777, with the last valid key dropped from the reference -- the project's
    criterion accepts the mutant as if it were the reference."""
    Hkv, G, D, BS = 2, 4, 128, ap.BS
    Hq = Hkv * G
    ctx = [1, 63, 64, 65, 300, 777]
    B = len(ctx)
    torch.manual_seed(G)                               # _random_paged(B, ctx, Hkv, D, dev, seed=G)
    nblk = [(c + BS - 1) // BS for c in ctx]
    NB = sum(nblk) + 3
    kc = torch.randn(NB, Hkv, BS, D, dtype=torch.bfloat16)
    vc = torch.randn(NB, Hkv, BS // 8, D, 8, dtype=torch.bfloat16)
    perm = torch.randperm(NB)
    bt = torch.zeros(B, max(nblk), dtype=torch.int32)
    k = 0
    for b in range(B):
        for i in range(nblk[b]):
            bt[b, i] = perm[k]
            k += 1
    q = torch.randn(B, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16)[:, : Hq * D].reshape(B, Hq, D)
    scale = 1 / math.sqrt(D)
    cl = torch.tensor(ctx, dtype=torch.int32)
    good = ref.paged_decode_attention(q, kc, vc, bt, cl, scale)
    cl[-1] -= 1
    mutant = ref.paged_decode_attention(q, kc, vc, bt, cl, scale)
    ex = float(_excess(mutant[-1], good[-1]).max())
    assert 0.0 < ex <= 1.0, f"drop-last on randn inputs: {ex:.2f}x the tolerance"
