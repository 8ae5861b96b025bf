"""The GEMM probe cases without a GPU (gemm_probe.py): for EVERY case of every family the
conditions on the inputs hold -- operands exact in bf16, sum |x||w| (+ bias, residual) inside
the bound that makes f32 accumulation exact in any order, fp8 cache values that survive the
e4m3 round trip, 1/rms spread over 0.5 .. 2 -- and the comparator test_gemm_probe_gpu.py
uses (torch.equal for the exact outputs, |got - ref| <= 2^-7 |ref| + 1e-6 for the rounded
ones) refuses every mutant of the reference: one x element zeroed at every probe column
(0, K - 1, every multiple of the K step and the column before it, every split boundary) of
the first and last row; a 16-byte chunk of a w row zeroed or read from its neighbour; two x
chunks swapped; a K stage added twice or skipped; a split dropped; two output rows or the
columns n, n ^ 16 exchanged; the last row unwritten; gate and up exchanged; a RoPE pair at
the wrong distance or with the sine's sign flipped; a call that read one split of the
previous call's data.  For the operand sets of the rounding epilogues a unit error in one
sum is at least 8x the allowance.  (M = 1 has no row to exchange with; that mutant alone is
not applied there.)
"""
import pytest

import gemm_probe as gp

_seen = set()


@pytest.mark.parametrize("family", sorted(gp.SPECS))
def test_every_case_holds_and_rejects_its_mutants(family):
    n_cases = n_mut = 0
    for spec in gp.SPECS[family]:
        for c in gp.cases(family, spec):
            if c.name in _seen:      # the same operands under another tile width
                continue
            _seen.add(c.name)
            gp.check_inputs(c)
            n_mut += gp.check_mutants(c)
            n_cases += 1
    assert n_cases > 0 and n_mut >= 10 * n_cases


def test_routing_mirrors():
    """The split-K ranges the mutants use are the kernels': uneven stages over the splits."""
    assert gp.split_ranges(576, 2, 64) == [(0, 256), (256, 576)]
    assert gp.split_ranges(4224, 4, 128) == [(0, 1024), (1024, 2048), (2048, 3072), (3072, 4224)]
    assert gp.cmb_splits(128, 512) == 2 and gp.cmb_splits(256, 576) == 2 and gp.cmb_splits(128, 1088) == 4
    assert gp.dg_route(256, 384, 1088, 128, 17) == (128, 17) and gp.dg_route(129, 128, 576, 0, 0, norm=True) == (64, 2)
    assert gp.skinny_splits(64, 256, 1024) == 2 and gp.skinny_splits(257, 128, 2048) == 4
    assert gp.prefill_splits(255, 256, 4224, 1) == 4 and gp.prefill_splits(255, 256, 4224, 2) == 1


def test_comparator_allows_one_rounding_and_no_more():
    import torch
    ref = torch.tensor([1.0, -3.0, 100.0, 0.0], dtype=torch.float64)
    assert not gp.rejected(gp.ROUNDED, ref * (1 + 2.0 ** -8), ref)
    assert gp.rejected(gp.ROUNDED, ref * (1 + 2.0 ** -6), ref)
    assert gp.rejected(gp.ROUNDED, ref + torch.tensor([0, 0, 0, float("nan")]), ref)
    assert gp.rejected(gp.EXACT, ref + torch.tensor([0, 0, 2.0 ** -20, 0]), ref) and not gp.rejected(gp.EXACT, ref.clone(), ref)
