"""CPU: the Chamfer reconstruction term 'Prop_sym_cd' (config.FLAGS.prop_sym_cd_w) -- the switch and its
default, the readable statement in losses.py against the fp64 restatement of tests/_recon_chamfer_ref.py, the limits of the
ordered backward (hsp_chamfer_bwd_ordered_ok) and the new entry points' bad-argument codes (nothing is launched: the pointers
are never read)."""
import ctypes

import numpy as np
import pytest
import torch

import _recon_chamfer_ref as rc

U = 2.0 ** -24


def _lib():
    from hs_pose_amd import _lib
    return _lib.lib(), _lib.CONSTANTS                   # (a missing library is a hard error, not a skip)


def test_switch_defaults_to_off(flags):
    assert flags.prop_sym_cd_w == 0.0
    flags.prop_sym_cd_w = 2.0
    flags.reset()
    assert flags.prop_sym_cd_w == 0.0


def _prop_loss(batch, names=('Prop_pm', 'Prop_sym')):
    from hs_pose_amd.losses import prop_rot_loss
    B = batch["PC"].shape[0]
    green = torch.nn.functional.normalize(batch["gt_R"][..., 1] + 0.05, dim=-1)
    red = torch.nn.functional.normalize(batch["gt_R"][..., 0] - 0.05, dim=-1)
    pred = {'Rot1': green, 'Rot1_f': torch.full((B,), 0.7), 'Rot2': red, 'Rot2_f': torch.full((B,), 0.6),
            'Tran': batch["gt_t"] + 0.01, 'Recon': batch["recon"]}
    gt = {'Points': batch["PC"], 'R': batch["gt_R"], 'T': batch["gt_t"]}
    return prop_rot_loss()(list(names), pred, gt, batch["sym"])


def test_weight_zero_leaves_the_dict_as_it_was(ref, flags):
    batch = rc.batch(ref, 4, 7, rc.ALL_CLASSES)
    assert set(_prop_loss(batch)) == {"Prop_pm", "Prop_sym_recon", "Prop_sym_rt"}
    flags.prop_sym_cd_w = 0.5
    assert set(_prop_loss(batch)) == {"Prop_pm", "Prop_sym_recon", "Prop_sym_rt", "Prop_sym_cd"}
    assert set(_prop_loss(batch, names=('Prop_pm',))) == {"Prop_pm", "Prop_occ"}         # no 'Prop_sym' among the stage's names


@pytest.mark.parametrize("B,N,tiled", [(4, 7, None), (4, 64, 1)])
def test_readable_statement_against_fp64(ref, flags, B, N, tiled):
    """losses.py's term on batches that hold all four symmetry classes (cloud 3 is ``skip``; at N = 64 cloud 1 is tiled: exact
    duplicates in both sets).  Its target against the fp64 one within 2^-23 (4 sum_k |p_k - t_k| + |G|) per component (twice
    the roundings of two 3-term products, a subtraction and an add); the term and d term / d recon against the restatement
    run on that fp32 target, so the searches see the same inputs: the term within (2 B N + 8) 2^-24 of itself (five roundings
    per distance, the sums at their sequential worst), a gradient row within (c_i + 4) 2^-24 |s| sum |terms|, c_i its in-degree;
    rows that hang on a near tie (fp64 gap within 2^-18 of the runner-up, exact ties not among them) are excused, at most
    0.5 % of them; a skip cloud gets exactly zero."""
    from hs_pose_amd.losses import prop_rot_loss
    w = 0.75
    flags.prop_sym_cd_w = w
    batch = rc.batch(ref, B, N, rc.ALL_CLASSES, tiled=tiled)
    if tiled is not None:
        assert torch.equal(batch["recon"][tiled, 0], batch["recon"][tiled, (N + 2) // 3])
    G32, skip = prop_rot_loss._sym_target(batch["PC"], batch["gt_R"], batch["gt_t"], batch["sym"])
    G64, mag = rc.target64(batch["PC"], batch["gt_R"], batch["gt_t"], batch["sym"])
    assert skip.tolist() == [False, False, False, True]
    assert np.all(np.abs(G32.double().numpy() - G64) <= 2.0 ** -23 * (4 * mag[..., None] + np.abs(G64)))

    recon = batch["recon"].clone().requires_grad_(True)
    term = _prop_loss(dict(batch, recon=recon))["Prop_sym_cd"]
    term.backward()
    want, gwant, loose, gmag, deg = rc.term64(batch["PC"], batch["gt_R"], batch["gt_t"], batch["sym"], batch["recon"], w,
                                              G=G32.numpy())
    assert want > 0
    assert abs(float(term.detach()) - want) <= (2 * B * N + 8) * U * want, (float(term.detach()), want)
    got = recon.grad.double().numpy()
    assert np.all(got[3] == 0)
    assert loose.sum() <= 0.005 * B * N, int(loose.sum())
    bound = (deg[..., None] + 4) * U * (2 * w / (B * N)) * gmag
    ok = (np.abs(got - gwant) <= bound) | loose[..., None]
    assert ok.all(), float(np.abs(got - gwant).max())
    assert np.abs(gwant).max() > 0 and (tiled is None or deg.max() >= 2)        # duplicates: the first one is chosen by all


def test_ordered_backward_limits():
    """hsp_chamfer_bwd_ordered_ok(B, n, m): the last clouds taken and the first declined -- the reverse build's histogram
    (hsp_rev_build_takes: 35 839 source rows) on either side, 65 535 clouds"""
    L, _ = _lib()
    ok = L.hsp_chamfer_bwd_ordered_ok
    assert ok(1, 35839, 35839) == 1 and ok(1, 35840, 1) == 0 and ok(1, 1, 35840) == 0
    assert ok(65535, 1, 1) == 1 and ok(65536, 1, 1) == 0
    assert ok(0, 4, 4) == 0 and ok(1, 0, 4) == 0 and ok(1, 4, 0) == 0
    assert ok(1, 35839, 1) == L.hsp_rev_build_takes(35839) and ok(1, 35840, 1) == L.hsp_rev_build_takes(35840)
    assert L.hsp_chamfer_bwd_ordered_workspace_bytes(2, 5, 7) == 2 * (2 * 12 + 2) * 4
    assert L.hsp_recon_chamfer_fwd_workspace_bytes(2, 5) == 8 * 10 and L.hsp_recon_chamfer_bwd_workspace_bytes(2, 5) == 2 * 11 * 4
    assert L.hsp_chamfer_bwd_ordered_workspace_bytes(0, 5, 7) == 0 and L.hsp_recon_chamfer_fwd_workspace_bytes(2, 0) == 0


def test_bad_arguments_launch_nothing():
    L, K = _lib()
    bad, uns = K["ERR_BAD_ARG"], K["ERR_UNSUPPORTED"]
    one, null, big = ctypes.c_void_p(16), ctypes.c_void_p(0), 1 << 30
    # hsp_recon_chamfer_fwd(PC, gt_R, gt_t, sym, recon, B, N, w, term, G, idx1, idx2, ws, ws_bytes, stream)
    fwd = L.hsp_recon_chamfer_fwd
    good = [one, one, one, one, one, 2, 8, 1.0, one, one, one, one, one, big, null]
    for k in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12):
        assert fwd(*[null if i == k else a for i, a in enumerate(good)]) == bad, k
    for k, v in ((5, 0), (5, -1), (6, 0), (7, float("nan")), (7, float("inf")), (13, 8 * 16 - 1)):
        assert fwd(*[v if i == k else a for i, a in enumerate(good)]) == bad, (k, v)
    assert fwd(*[65536 if i == 5 else a for i, a in enumerate(good)]) == uns
    # hsp_recon_chamfer_bwd(recon, G, idx1, idx2, sym, g, B, N, w, gx, ws, ws_bytes, stream)
    bwd = L.hsp_recon_chamfer_bwd
    good = [one, one, one, one, one, one, 2, 8, 1.0, one, one, big, null]
    for k in (0, 1, 2, 3, 4, 5, 9, 10):
        assert bwd(*[null if i == k else a for i, a in enumerate(good)]) == bad, k
    for k, v in ((6, 0), (7, 0), (7, -3), (8, float("nan")), (8, float("-inf")), (11, 2 * 17 * 4 - 1)):
        assert bwd(*[v if i == k else a for i, a in enumerate(good)]) == bad, (k, v)
    assert bwd(*[35840 if i == 7 else a for i, a in enumerate(good)]) == uns
    # hsp_chamfer_bwd_ordered(xyz1, xyz2, idx1, idx2, gd1, gd2, B, n, m, gx1, gx2, ws, ws_bytes, stream)
    bo = L.hsp_chamfer_bwd_ordered
    good = [one, one, one, one, one, one, 2, 8, 5, one, one, one, big, null]
    for k in (0, 1, 2, 3, 4, 5, 11):
        assert bo(*[null if i == k else a for i, a in enumerate(good)]) == bad, k
    assert bo(*[null if i in (9, 10) else a for i, a in enumerate(good)]) == bad           # neither gradient wanted
    for k, v in ((6, 0), (7, 0), (8, -1), (12, 2 * (2 * 13 + 2) * 4 - 1)):
        assert bo(*[v if i == k else a for i, a in enumerate(good)]) == bad, (k, v)
    assert bo(*[35840 if i == 8 else a for i, a in enumerate(good)]) == uns
    assert bo(*[35840 if i == 7 else a for i, a in enumerate(good)]) == uns
