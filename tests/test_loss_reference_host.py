"""CPU: the condition on the inputs of tests/test_gpu_loss_reference.py (stated there), on every one of its cases: losses.py runs
in float64 with every term float64 and every figure finite, and its float32 run stays within 2e-2 of it on the plane-fit
pairs and within 1e-5 on every other (term, output) pair.  Needs no device; the GPU tests assert the same before they look
at a kernel."""
import pytest
import torch

import _loss_ref as L


@pytest.mark.parametrize("name", list(L.CASES))
def test_loss_reference_inputs_host(ref, name):
    gt, pred, kind, c64, c32 = L.reference(ref, name)
    assert set(c64[2].values()) == {torch.float64} and set(c32[2].values()) == {torch.float32}
    recs = L.pair_errors(c64, c32)
    bad = L.input_failures(recs)
    assert not bad, f"{name}: inadmissible input:\n" + "\n".join(map(L.show, bad[:20]))
    # a batch with all seven symmetry classes exercises every term: one that a case zeroed by accident would check nothing
    if gt["sym"].shape[0] >= 7:
        live = {r["term"] for r in recs if r["out"] is not None and r["m"] > 0.0}
        assert live == set(L.TERMS), set(L.TERMS) - live


def test_acos_case_is_clamped(ref):
    """the near-parallel / near-antiparallel axes lie beyond the clamp, in float32 and in float64"""
    gt, pred = L.acos_case(ref)
    for b, sign in ((2, 1.0), (4, -1.0)):
        for dt in (torch.float32, torch.float64):
            d = float((pred["p_green_R"][b].to(dt) * pred["p_red_R"][b].to(dt)).sum())
            assert sign * d > 1.0 - 1e-6, (b, dt, d)
