"""CPU: the numpy reference of the tracked front end (tests/_track_ref.py) against hand-worked cases, the margins of the
committed seeds, and the host half of the feature: header, ctypes table, wrappers, ``FrameTracker`` argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _track_ref as tr
import test_frame_host as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a pinhole camera with whole numbers: u = 100 X / Z + 32, v = 100 Y / Z + 24 on a 48 x 64 frame
K_HAND = np.array([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])
NEW = ["hsp_pose_windows", "hsp_roi_compact_box_f32", "hsp_roi_compact_box_u16", "hsp_track_update"]


def _axis_aligned(t):
    return tr.pose(np.eye(3, dtype=np.float32), t)


def test_axis_aligned_box_by_hand():
    """size (0.2, 0.1, 0.5), pad 1: half extents (0.1, 0.05, 0.25) about (0.05, 0.0125, 1): the near face at Z = 0.75 decides
    the extremes -- u = 100 * (-0.05 | 0.15) / 0.75 + 32 = 25.33 | 52, v = 100 * (-0.0375 | 0.0625) / 0.75 + 24 = 19 | 32.33"""
    RT, size = _axis_aligned([0.05, 0.0125, 1.0])[None], np.array([[0.2, 0.1, 0.5]], np.float32)
    u, v, Z = tr.corner_uv(RT[0], size[0], K_HAND.reshape(-1), 1.0)
    assert sorted(set(np.round(Z, 6))) == [0.75, 1.25]
    assert abs(u.min() - (32 - 5 / 0.75)) < 1e-5 and abs(u.max() - 52.0) < 1e-5          # (0.2 and 0.1 are not fp32 numbers)
    assert abs(v.min() - 19.0) < 1e-5 and abs(v.max() - (24 + 6.25 / 0.75)) < 1e-5
    win = tr.windows(RT, size, K_HAND, 48, 64, 32, 1.0)
    # u.max() and v.min() sit on integers up to fp32 noise in the size: take a pad that moves them off
    win = tr.windows(RT, size, K_HAND, 48, 64, 32, 1.01)
    assert win["wstatus"].tolist() == [0] and win["boxes"].tolist() == [[25, 18, 53, 33]]
    assert win["centers"].tolist() == [[39.0, 25.5]] and win["scales"].tolist() == [28.0]
    assert tuple(win["xf"][0].tolist()) == fh.ref_xf((39.0, 25.5), 28.0, 32)
    from hs_pose_amd.pc_sample import roi_transform
    assert np.array_equal(roi_transform(win["centers"], win["scales"], 32), win["xf"])


def test_inside_by_hand():
    """a frame of constant depth 1000 mm under the whole-number camera: pixel (u, v) is the point ((u - 32) / 100, (v - 24) /
    100, 1); the box of half extents (0.1, 0.05, 0.25) about (0.05, 0.0125, 1) holds -5 <= u - 32 <= 15, -3.75 <= v - 24 <= 6.25"""
    depth = np.full((48, 64), 1000.0, np.float32)
    depth[22, 30] = 0                                           # a hole inside the box
    depth[25, 40] = 1300.0                                      # a pixel behind the box: Z = 1.3 > 1.25
    RT, size = _axis_aligned([0.05, 0.0125, 1.0]), np.array([0.2, 0.1, 0.5], np.float32)
    m, margin = tr.inside(depth, RT, size, K_HAND.reshape(-1), 1.0)
    want = np.zeros((48, 64), bool)
    want[21:31, 28:47] = True              # v - 24 in [-3, 6], u - 32 in [-4, 14]: the edges u - 32 = -5, 15 lie ON the box up to
    want[22, 30] = want[25, 40] = False    # fp32 noise and are left to the margin
    inner = np.ones((48, 64), bool)
    inner[:, [27, 47]] = False
    assert np.array_equal(m[inner], want[inner])
    assert margin < 1e-6                                        # ... and the margin says so: this case would be redrawn
    # rotated a quarter turn about the optical axis, the box's first two extents swap
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    m2, _ = tr.inside(depth, tr.pose(Rz, [0.05, 0.0125, 1.0]), size[[1, 0, 2]], K_HAND.reshape(-1), 1.0)
    assert np.array_equal(m2[inner], want[inner])


def test_rejections_are_bit_4():
    size = np.array([[0.2, 0.2, 0.2]], np.float32)
    ok = tr.windows(_axis_aligned([0.0, 0.0, 1.0])[None], size, K_HAND, 48, 64, 32, 1.5)
    assert ok["wstatus"].tolist() == [0]
    behind = tr.windows(_axis_aligned([0.0, 0.0, 0.1])[None], size, K_HAND, 48, 64, 32, 1.5)       # near corners at Z = -0.05
    off = tr.windows(_axis_aligned([2.0, 0.0, 1.0])[None], size, K_HAND, 48, 64, 32, 1.5)          # u about 232: right of the frame
    above = tr.windows(_axis_aligned([0.0, -2.0, 1.0])[None], size, K_HAND, 48, 64, 32, 1.5)
    neg = tr.windows(_axis_aligned([0.0, 0.0, 1.0])[None], size * np.float32([1, -1, 1]), K_HAND, 48, 64, 32, 1.5)
    zero = tr.windows(_axis_aligned([0.0, 0.0, 1.0])[None], size * np.float32([1, 1, 0]), K_HAND, 48, 64, 32, 1.5)
    nan = tr.windows(_axis_aligned([0.0, np.nan, 1.0])[None], size, K_HAND, 48, 64, 32, 1.5)
    for w in (behind, off, above, neg, zero, nan):
        assert w["wstatus"].tolist() == [4] and not w["boxes"].any() and not w["xf"].any()
    # a flagged instance lists nothing, and the update keeps its state
    depth = np.full((48, 64), 1000.0, np.float32)
    assert tr.compact(depth, _axis_aligned([2.0, 0.0, 1.0])[None], size, K_HAND, 32, 1.5, off) == [(pytest.approx([]), [0, 0])]
    rt, sz, lost = tr.update(np.ones((2, 4, 4)), np.ones((2, 3)), [0, 5], np.zeros((2, 4, 4)), np.zeros((2, 3)), np.array([3, 3]))
    assert rt[0].all() and not rt[1].any() and sz[0].all() and not sz[1].any() and lost.tolist() == [0, 4]


def test_committed_seeds_hold_both_margins():
    names = []
    for name, case in tr.all_cases():
        assert case["uv_margin"] >= tr.UV_MARGIN and case["q_margin"] >= tr.Q_MARGIN, (name, case["uv_margin"], case["q_margin"])
        names.append(name)
    assert len(names) == 2 + len(tr.COMPACTION_CASES)
    w = tr.windows_case()["win"]
    assert w["wstatus"].tolist() == [0, 0, 0, 4, 4, 4, 4, 4]
    assert (w["boxes"][:3, 2] == 63).any()                      # one accepted window is cut by the frame's edge
    for args in tr.COMPACTION_CASES:
        c = tr.compaction_case(*args)
        O, s = args[0], c["win"]["scales"]
        counts = np.array([k[1] for k in c["want"]])
        assert c["win"]["wstatus"].tolist() == [0, 0, 0] and s.min() < O and s.max() == 63 and (O != 48 or s.max() > O)
        assert (counts[:, 0] > 0).all() and (counts[:, 1] > counts[:, 0]).all(), counts
        src0 = c["want"][0][0]
        assert len(np.unique(src0)) < len(src0)                 # the small window: source pixels repeat


def test_header_table_and_wrappers_agree():
    from hs_pose_amd import _lib, ops
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hsp.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    vp, i, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    want = {"hsp_pose_windows": [vp, vp, vp, i, i, i, i, i, d, vp, vp, vp, vp],
            "hsp_roi_compact_box_f32": [vp, vp, vp, d, vp, i, vp, vp, i, i, i, i, vp, vp, vp, sz, vp],
            "hsp_roi_compact_box_u16": [vp, vp, vp, d, vp, i, vp, vp, i, i, i, i, vp, vp, vp, sz, vp],
            "hsp_track_update": [vp, vp, vp, i, vp, vp, vp, vp]}
    for s in NEW:
        assert s in syms and hasattr(L, s) and _lib.SIGNATURES[s] == (i, want[s]), s
    null, one = vp(0), vp(64)
    pw = L.hsp_pose_windows
    assert pw(null, one, one, 1, 2, 48, 64, 16, 1.5, one, one, one, null) == -1                    # no pose
    assert pw(one, one, one, 1, 0, 48, 64, 16, 1.5, one, one, one, null) == -1                     # n = 0
    assert pw(one, one, one, 3, 2, 48, 64, 16, 1.5, one, one, one, null) == -1                     # camK rows neither 1 nor n
    assert pw(one, one, one, 1, 2, 48, 64, 16, 0.0, one, one, one, null) == -1                     # pad 0
    assert pw(one, one, one, 1, 2, 48, 64, 16, float("nan"), one, one, one, null) == -1
    assert pw(one, one, one, 1, 2, 48, 64, 16, float("inf"), one, one, one, null) == -1
    assert pw(one, one, one, 1, 2, 65536, 65536, 16, 1.5, one, one, one, null) == -1               # H*W >= 2^31
    assert pw(one, one, one, 1, 2, 48, 64, 50000, 1.5, one, one, one, null) == -1                  # O out of range
    assert pw(one, one, one, 1, 2, 48, 64, 16, 1.5, one, one, null, null) == -1                    # no wstatus
    for fn in (L.hsp_roi_compact_box_f32, L.hsp_roi_compact_box_u16):
        assert fn(null, one, one, 1.5, one, 1, null, one, 1, 48, 64, 16, one, one, one, 64, null) == -1       # no depth
        assert fn(one, null, one, 1.5, one, 1, null, one, 1, 48, 64, 16, one, one, one, 64, null) == -1       # no pose
        assert fn(one, one, one, -1.0, one, 1, null, one, 1, 48, 64, 16, one, one, one, 64, null) == -1       # pad < 0
        assert fn(one, one, one, 1.5, one, 2, null, one, 3, 48, 64, 16, one, one, one, 64, null) == -1        # camK rows
        assert fn(one, one, one, 1.5, one, 1, null, one, 1, 48, 64, 50000, one, one, one, 64, null) == -2     # O*O >= 2^31
        assert fn(one, one, one, 1.5, one, 1, null, one, 70000, 48, 64, 16, one, one, one, 1 << 30, null) == -2
        assert fn(one, one, one, 1.5, one, 1, null, one, 2, 48, 64, 96, one, one, null, 0, null) == -3        # no workspace
        assert fn(one, one, one, 1.5, one, 1, null, one, 2, 48, 64, 96, one, one, one, 47, null) == -3        # (roi_compact's size)
    tu = L.hsp_track_update
    assert tu(one, one, null, 2, vp(4096), vp(8192), one, null) == -1                              # no status
    assert tu(one, one, one, 0, vp(4096), vp(8192), one, null) == -1                               # n = 0
    assert tu(vp(4096), one, one, 2, vp(4096 + 64), vp(8192), one, null) == -1                     # new and state overlap
    # the wrappers refuse host tensors before anything is called
    from hs_pose_amd._lib import HspError
    RT, size, K = torch.eye(4).repeat(2, 1, 1), torch.ones(2, 3), torch.eye(3, dtype=torch.float64)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.pose_windows(RT, size, K, 48, 64, 16, 1.5)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.roi_compact_box(torch.zeros(48, 64), RT, size, 1.5, K, torch.zeros(2, 3, dtype=torch.float64), 16)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.track_update(RT, size, torch.zeros(2, dtype=torch.int32), RT.clone(), size.clone(), torch.zeros(2, dtype=torch.int32))


def test_frame_tracker_argument_errors():
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.frame import FrameTracker
    FLAGS.reset()
    try:
        tables = torch.zeros(6, 3), torch.zeros(6, 4)
        for sampler in (None, "host"):                           # (None follows FLAGS.pc_sampler = 'host')
            with pytest.raises(ValueError, match="need.* a device sampler .*the host draws wait for the counts"):
                FrameTracker(None, *tables, sampler=sampler)
        with pytest.raises(ValueError, match="pc sampler"):
            FrameTracker(None, *tables, sampler="nearest")
        for pad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="pad"):
                FrameTracker(None, *tables, sampler="fps", pad=pad)
        with pytest.raises(ValueError, match="min_pts"):
            FrameTracker(None, *tables, sampler="fps", min_pts=0)
        trk = FrameTracker(None, *tables, sampler="fps")
        assert trk.min_pts == 50 and trk.pad is None and pc_sample.track_pad(trk.pad) == FLAGS.DZI_PAD_SCALE == 1.5
        assert pc_sample.track_pad(2) == 2.0
        with pytest.raises(RuntimeError, match="start"):
            trk.step(torch.zeros(4, 4))
        with pytest.raises(RuntimeError, match="start"):
            trk.state()
        with pytest.raises(ValueError, match="on the device"):
            trk.start(torch.zeros(2, 4, 4), torch.zeros(2, 3), [1, 2])          # host tensors
        FLAGS.pc_sampler = "fps"
        assert FrameTracker(None, *tables)._sampler(torch.device("cpu")) is pc_sample.FPS
        with pytest.raises(ValueError, match="device sampler"):
            pc_sample.track_to_pcl_device(torch.zeros(4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 3), np.eye(3), sampler="host")
    finally:
        FLAGS.reset()
