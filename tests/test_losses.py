"""The training losses and the on-device augmentation (hs_pose_amd/losses.py, augment.py, HSPose.forward(do_loss=True))
against the fixtures written by the reference's loss modules (oracle/gen_golden_losses.py).  They are torch-op
compositions, so the same assertions run on the CPU here and on the GPU (test_gpu_losses.py)."""
import numpy as np
import pytest
import torch

from _loss_ref import wire
from conftest import golden

LOSS_KEYS = {
    "fsnet_loss": ["Rot1", "Rot1_cos", "Rot2", "Rot2_cos", "Rot_r_a", "Tran", "Size", "R_con"],
    "recon_loss": ["recon_per_p", "recon_p_f", "recon_point_vote", "recon_point_r", "recon_point_t", "recon_point_s",
                   "recon_point_self"],
    "geo_loss": ["geo_point"],
    "prop_loss": ["Prop_pm", "Prop_sym_recon", "Prop_sym_rt"],
}


def run_losses(ref, device, flags, loss_type):
    """HSPose's loss wiring (its forward after the network call) on the closed-form batch"""
    flags.fsnet_loss_type = loss_type
    gt, pred = ref.loss_case()
    gt = {k: v.to(device) for k, v in gt.items()}
    pred = {k: v.detach().to(device).requires_grad_(True) for k, v in pred.items()}
    ld = wire(gt, pred)
    return ld, pred


def check_losses(ref, device, flags, name, loss_type):
    g = golden(name)
    ld, pred = run_losses(ref, device, flags, loss_type)
    assert {k: list(v) for k, v in ld.items()} == LOSS_KEYS                    # the 19 terms, in the reference's order
    for grp, d in ld.items():
        for k, v in d.items():
            want = g[f"{grp}.{k}"]
            got = v.detach().cpu().numpy().reshape(-1)
            assert got.shape == want.shape, (grp, k, got.shape, want.shape)   # (Rot2 keeps the reference's shape (1,))
            # the plane-fit ("voting") terms go through an ill-conditioned 3x3 inverse: on another device's BLAS /
            # libm their rounding moves by ~1e-4 relative; everything else is plain sums
            tol = 2e-6 * max(1.0, np.abs(want).max()) if device.type == "cpu" else 1e-3 * max(np.abs(want).max(), 1e-2)
            assert np.abs(got - want).max() <= tol, (grp, k, got, want)
    total = sum(sum(d.values()) for d in ld.values())
    assert abs(float(total.detach()) - float(g["total"][0])) <= (1e-5 if device.type == "cpu" else 1e-3)
    total.backward()
    for k, v in pred.items():
        want = g["grad." + k]
        err = np.abs(v.grad.cpu().numpy() - want).max()
        # face normals / distances also feed the weighted plane fits, whose 3x3 normal equations (points ~0.8 m from the
        # origin) amplify fp32 rounding ~1e3: any reordering of their sums moves these gradients by ~1e-4 of their scale
        tol = (5e-4 if device.type == "cpu" else 5e-3) if k in ("face_normal", "face_dis") else (2e-5 if device.type == "cpu" else 2e-4)
        assert err <= tol * max(1.0, np.abs(want).max()), (k, err)


@pytest.mark.parametrize("name,loss_type", [("losses_l1", "l1"), ("losses_smoothl1", "smoothl1")])
def test_losses_match_reference_cpu(ref, flags, name, loss_type):
    check_losses(ref, torch.device("cpu"), flags, name, loss_type)


def check_augment(ref, device, flags):
    from hs_pose_amd import HSPose as H
    from hs_pose_amd.augment import data_augment
    g = golden("losses_augment")
    gt = {k: v.to(device) for k, v in ref.augment_case().items()}
    green, red = H.get_gt_v(gt["gt_R"])
    assert np.abs(green.cpu().numpy() - g["green"]).max() < 1e-6 and np.abs(red.cpu().numpy() - g["red"]).max() < 1e-6
    assert torch.allclose(green, gt["gt_R"][:, :, 1]) and torch.allclose(red, gt["gt_R"][:, :, 0])
    for tag, pro in (("half", 0.6), ("all", 1.1), ("none", -1.0)):
        flags.aug_bb_pro = flags.aug_rt_pro = flags.aug_bc_pro = flags.aug_pc_pro = pro
        if device.type == "cpu":
            torch.manual_seed(5)                            # same generator, same consumption order as the reference
        elif tag == "half":
            continue                                        # device generator: only the draw-independent cases compare
        PC, R, t, s = data_augment(gt["PC"].clone(), gt["gt_R"].clone(), gt["gt_t"].clone(), gt["gt_s"].clone(), gt["mean_shape"],
                                   gt["sym"], gt["aug_bb"], gt["aug_rt_t"], gt["aug_rt_r"], gt["model_point"].clone(),
                                   gt["nocs_scale"], gt["obj_id"])
        if device.type != "cpu" and tag == "all":
            # the taper / jitter factors are random: compare what does not depend on them
            assert np.abs(R.cpu().numpy() - g["all.R"]).max() < 1e-5 and np.abs(t.cpu().numpy() - g["all.t"]).max() < 1e-5
            continue
        for k, v in (("PC", PC), ("R", R), ("t", t), ("s", s)):
            assert np.abs(v.cpu().numpy() - g[f"{tag}.{k}"]).max() < 2e-6, (tag, k)


def test_augment_matches_reference_cpu(ref, flags):
    check_augment(ref, torch.device("cpu"), flags)
