"""GPU: the fused loss kernels (csrc/losses.hip: prep, points, finish, cloud-bwd, points-bwd) against hs_pose_amd/losses.py in
float64 on the CPU, term by term: the value of each of the 19 terms and the gradient of EACH term w.r.t. each of the ten
network outputs (one backward per term hands the kernels a one-hot ``gw``), at the edges of the kernels' point and batch
passes and at the kinks of the formulas.  losses.py is the torch-op statement of the reference's loss modules, pinned on the
CPU by the reference-written fixtures tests/golden/losses_*.npz; it runs unchanged in float64.

Tolerance definition (stated once, used below; the code of it is tests/_loss_ref.py):
  * The unit of the check is a (term, output) pair; for the per-point outputs recon, face_normal, face_dis, face_f it is a
    (term, output, cloud) triple.  m = the largest absolute entry of the fp64 gradient of that unit.
  * m == 0 (a term that does not depend on an output, a red-axis term on a rotationally symmetric cloud, the reconstruction
    term on the 'skip' class): the kernel's gradient there is exactly zero, or None.
  * otherwise  e_kernel <= max(FLOOR, K * e_comp)  with  e_kernel = max |g_kernel - g64| / m  and e_comp the same figure of
    losses.py run in float32 on the CPU.  K = 4: the kernels and the fp32 composition are two fp32 evaluations of one formula
    that differ in sum order and fused multiply-adds.  FLOOR = 1e-5 for gradients: 4 x the largest e_comp measured on a pair
    that does not pass through the plane fits (2.6e-6, recon_p_f -> face_dis).
  * the same rule relative to |term64| for each term's value, with FLOOR = 2e-6 (plain-sum terms measure <= 4e-7).
  * the plane-fit pairs -- recon_point_vote / _r / _t / _s / _self against face_normal, face_dis, Pred_T -- go through the
    3x3 normal equations of a weighted plane fit, whose conditioning depends on the cloud: their e_comp measures 2e-4 ... 2e-2
    and the K * e_comp branch sets their bound.  No fixed number on purpose.
  * Condition on the inputs, asserted on the CPU quantities before the kernel is looked at: every fp64 figure finite,
    e_comp <= 2e-2 on the plane-fit pairs and <= 1e-5 on every other pair.  An ill-conditioned input fails as a bad input; it
    does not loosen the kernel's bound.  (tests/test_loss_reference_host.py asserts the same without a device.)  The seeds of
    the cases were chosen by this condition alone.  No pair is skipped.

Measured (1 x MI355X): DESIGN 2.0c."""
import pytest
import torch

import _loss_ref as L

pytestmark = pytest.mark.gpu


def _check(ref, dev, name):
    gt, pred, kind, c64, c32 = L.reference(ref, name)
    assert set(c64[2].values()) == {torch.float64} and set(c32[2].values()) == {torch.float32}
    bad = L.input_failures(L.pair_errors(c64, c32))
    assert not bad, f"{name}: inadmissible input (reference only):\n" + "\n".join(map(L.show, bad[:20]))
    got = L.kernels(gt, pred, dev, kind)
    recs = L.pair_errors(c64, c32, got)
    for plane in (True, False):                                  # the figures, before anything is asserted
        sel = [r for r in recs if r["plane"] == plane and r["m"] > 0.0 and r["out"] is not None]
        if sel:
            w = max(sel, key=lambda r: r["e_kernel"] / max(r["e_comp"], L.FLOOR_GRAD / L.K))
            print(f"{name}: {'plane-fit' if plane else 'other'} pairs, {len(sel)} units: largest e_comp "
                  f"{max(r['e_comp'] for r in sel):.2e}, largest e_kernel {max(r['e_kernel'] for r in sel):.2e}; "
                  f"nearest its bound: {L.show(w)}")
    bad = L.kernel_failures(recs)
    assert not bad, f"{name}: {len(bad)} of {len(recs)} units out of bound:\n" + "\n".join(map(L.show, bad[:30]))
    return gt, pred, c64, got


@pytest.mark.parametrize("name", [n for n in L.CASES if n.startswith("points-")])
def test_point_count_edges(dev, ref, name):
    """the seven symmetry classes at the edges of the two point passes (forward: 512 threads per cloud; backward: 256 points
    per block), L1 and smooth-L1"""
    _check(ref, dev, name)


@pytest.mark.parametrize("name", [n for n in L.CASES if n.startswith(("batch-", "rows-"))])
def test_batch_count_edges(dev, ref, name):
    """the edges of the per-cloud kernels (prep: 64 clouds per block; finish: stride 256, then a serial sum over B), and
    batches of a single symmetry class -- rows 0, 1, 3, 6 have no red axis, so B / #kept falls back to 1"""
    _check(ref, dev, name)


def test_sign_of_zero(dev, ref):
    """Pred_T == gt_t on cloud 1, Pred_s == gt_s on cloud 4, recon == PC on the cloud without symmetry: the L1 gradients on
    those entries are exactly 0 in the reference and on the device"""
    gt, pred, c64, got = _check(ref, dev, "sign-zero")
    for term, out, b in (("Tran", "Pred_T", 1), ("Size", "Pred_s", 4), ("Prop_sym_recon", "recon", 2)):
        assert float(c64[1][term][out][b].abs().max()) == 0.0, (term, out)
        assert float(got[1][term][out][b].abs().max()) == 0.0, (term, out)
        assert float(c64[1][term][out].abs().max()) > 0.0                    # (the other clouds do have a gradient)


def test_smooth_l1_knee(dev, ref):
    """translation and size residuals at exactly 0.5, 1 and 2 x beta: both branches of elem_loss and the tie |x| == beta"""
    gt, pred, c64, got = _check(ref, dev, "smoothl1-knee")
    for b, f in L.KNEE_CLOUDS:
        for p, g in (("Pred_T", "gt_t"), ("Pred_s", "gt_s")):
            assert torch.equal((pred[p][b] - gt[g][b]).abs(), torch.full((3,), f * L.KNEE_BETA)), (b, p)


def test_acos_clamp(dev, ref):
    """the red axis at L.ACOS_ANGLE from the green one on cloud 2 and at pi minus it on cloud 4: the clamp's zero gradient"""
    gt, pred, c64, got = _check(ref, dev, "acos-clamp")
    for b, sign in ((2, 1.0), (4, -1.0)):
        for dt in (torch.float32, torch.float64):
            d = float((pred["p_green_R"][b].to(dt) * pred["p_red_R"][b].to(dt)).sum())
            assert sign * d > 1.0 - 1e-6, (b, dt, d)


def test_unequal_confidences(dev, ref):
    """f_green_R / f_red_R = 0.02 / 0.98 and swapped: the confidence-weighted shares of vertical_axes, and R_con, the one term
    that differentiates them"""
    gt, pred, c64, got = _check(ref, dev, "confidences")
    for out in ("f_green_R", "f_red_R"):
        assert float(c64[1]["R_con"][out].abs().max()) > 0.0
        assert all(c64[1][t][out] is None for t in L.TERMS if t != "R_con")
