"""CPU: the host half of the frame front end (hs_pose_amd/pc_sample.py::roi_window / roi_transform, ops.roi_compact /
ops.frame_to_pcl argument checks) and the numpy RESTATEMENT of the crop rule the kernels are held to on the GPU
(tests/test_gpu_frame.py imports it from here; tools/time_frame_frontend.py times it).

The restatement is written from the rule in include/hsp.h, independently of pc_sample.py: forward matrix a = O / s,
tx = O/2 - a*cx, ty = O/2 - a*cy; inverse in float64 D = 1/(a*a), m0 = a*D, b1 = -m0*tx, b2 = -m0*ty; crop pixel (u, v) reads
frame pixel X = (rint(b1*1024) + 512 + rint(m0*u*1024)) >> 10, Y likewise with b2 and v; outside the frame the border is 0.
cv2 is not installed here, so nothing in this file runs OpenCV: what is checked is that the rule equals the closed form
X = floor(cx - s/2 + 1/2 + u*s/O) on every window ``get_bbox`` can produce, in exact integer arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------------

def ref_xf(center, scale, O):
    """(m0, b1, b2) as Python floats (float64), one rounding per step, in the order the contract fixes"""
    cx, cy, s, O = float(center[0]), float(center[1]), float(scale), float(O)
    a = O / s
    tx = O / 2 - a * cx
    ty = O / 2 - a * cy
    D = 1.0 / (a * a)
    m0 = a * D
    return m0, -m0 * tx, -m0 * ty


def ref_map(xf, O):
    """(X (O,), Y (O,)) int64: the frame column crop column u reads and the frame row crop row v reads (the map is separable)"""
    m0, b1, b2 = xf
    t = np.arange(O, dtype=np.float64)
    delta = np.rint(m0 * t * 1024.0).astype(np.int64)
    X = (np.int64(np.rint(b1 * 1024.0)) + 512 + delta) >> 10
    Y = (np.int64(np.rint(b2 * 1024.0)) + 512 + delta) >> 10
    return X, Y


def ref_source(xf, O, H, W):
    """(O,O) int64: frame pixel id Y*W + X every crop pixel (v, u) reads, -1 outside the frame"""
    X, Y = ref_map(xf, O)
    inside = ((Y >= 0) & (Y < H))[:, None] & ((X >= 0) & (X < W))[None, :]
    return np.where(inside, Y[:, None] * W + X[None, :], -1)


def ref_crops(depth, mask, xf, O):
    """(roi_coord_2d (2,O,O) float32, roi_mask (O,O), roi_depth (O,O)): the three nearest-neighbour warps of
    load_data_eval.py:231-243 -- the coordinate grid of get_2d_coord_np, the mask and the depth, constant border 0"""
    H, W = depth.shape
    p = ref_source(xf, O, H, W)
    q = np.maximum(p, 0)
    inside = p >= 0
    coord = np.stack([np.where(inside, (q % W).astype(np.float32), np.float32(0)),
                      np.where(inside, (q // W).astype(np.float32), np.float32(0))]).astype(np.float32)
    roi_mask = np.where(inside, mask.reshape(-1)[q], 0).astype(mask.dtype)
    return coord, roi_mask, np.where(inside, depth.reshape(-1)[q], 0).astype(depth.dtype)


def ref_compact(depth, belongs, xf, O):
    """(src int64 (count,), [mask-and-depth valid, depth valid]): ``belongs`` (H,W) bool is the instance's mask"""
    H, W = depth.shape
    p = ref_source(xf, O, H, W).reshape(-1)
    q = np.maximum(p, 0)
    dvalid = (p >= 0) & (depth.reshape(-1)[q] > 0)
    valid = dvalid & belongs.reshape(-1)[q]
    return p[valid], [int(valid.sum()), int(dvalid.sum())]


def cpu_frame_to_pcl(depth, masks, centers, scales, K, n_pts, O, sample_ids):
    """the whole chain on the CPU (what tools/time_frame_frontend.py times beside the device path): crops, the loader's
    float64 back-projection (load_data_eval.py:309-320) / 1000, ``sample_ids`` = pc_sample.sample_point_ids"""
    K = np.asarray(K, dtype=np.float64).reshape(-1)
    out = []
    for j in range(len(scales)):
        coord, rm, rd = ref_crops(depth, masks[j], ref_xf(centers[j], scales[j], O), O)
        d = rd.reshape(-1).astype(np.float64)
        valid = ((d > 0) * rm.reshape(-1)) > 0
        d = d[valid]
        x = (coord[0].reshape(-1)[valid] - K[2]) * d / K[0]
        y = (coord[1].reshape(-1)[valid] - K[5]) * d / K[4]
        pcl = np.stack((x, y, d), axis=-1).astype(np.float32) / 1000.0
        out.append(pcl[sample_ids(pcl.shape[0], n_pts)])
    return np.stack(out)


# ---- roi_window against the reference's get_bbox --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def windows():
    return golden("frame_roi_windows")


def test_fixture_matches_its_manifest(windows):
    import json
    with open(os.path.join(ROOT, "tests", "golden", "frame_manifest.json")) as f:
        man = json.load(f)["files"]["frame_roi_windows"]
    assert {k: [list(windows[k].shape), str(windows[k].dtype)] for k in windows.files} == man


def test_fixture_covers_the_edges(windows):
    w, (H, W) = windows["windows"], windows["im_hw"]
    side = w[:, 1] - w[:, 0]
    assert len(w) >= 200 and set(side.tolist()) == set(range(40, 441, 40)) and (side == w[:, 3] - w[:, 2]).all()
    assert (w[:, 0] == 0).any() and (w[:, 1] == H).any() and (w[:, 2] == 0).any() and (w[:, 3] == W).any()
    b = windows["boxes"]
    assert ((b[:, 0] == b[:, 2]) & (b[:, 1] == b[:, 3])).any()            # degenerate boxes


def test_roi_window_matches_reference(windows):
    from hs_pose_amd.pc_sample import roi_window, roi_windows
    H, W = (int(v) for v in windows["im_hw"])
    for b, c, s in zip(windows["boxes"], windows["centers"], windows["scales"]):
        center, scale = roi_window(tuple(b.tolist()), H, W)
        assert center.dtype == np.float32 and center.shape == (2,) and isinstance(scale, float)
        assert np.array_equal(center.astype(np.float64), c) and scale == s, (b, center, scale, c, s)
    centers, scales = roi_windows(windows["boxes"], H, W)
    assert centers.dtype == np.float32 and np.array_equal(centers.astype(np.float64), windows["centers"])
    assert np.array_equal(scales, windows["scales"])
    centers, scales = roi_windows(np.zeros((0, 4), np.int32), H, W)
    assert centers.shape == (0, 2) and scales.shape == (0,)
    with pytest.raises(ValueError):
        roi_window((0.5, 1, 20, 30), H, W)


def test_fixed_point_rule_equals_closed_form(windows):
    """for every fixture window and all 256 x 256 crop pixels (the map is separable: 256 columns and 256 rows decide them
    all), the rule equals floor(c - s/2 + 1/2 + t*s/O), evaluated in exact integers; and roi_transform gives the
    restatement's bits"""
    from hs_pose_amd.pc_sample import roi_transform
    O = 256
    t = np.arange(O, dtype=np.int64)
    xfs = roi_transform(windows["centers"], windows["scales"], O)
    for k, (c, s) in enumerate(zip(windows["centers"], windows["scales"])):
        xf = ref_xf(c, s, O)
        assert tuple(xfs[k].tolist()) == xf
        # every term the rule rounds is an integer up to the last-bit noise of the float64 inverse (s = 280 gives
        # m0 * 1024 = 1120.0000000000002): far from rint's ties at .5, so that noise cannot move a pixel
        terms = np.concatenate([xf[0] * t.astype(np.float64) * 1024.0, [xf[1] * 1024.0, xf[2] * 1024.0]])
        assert np.abs(terms - np.rint(terms)).max() < 1e-6
        X, Y = ref_map(xf, O)
        c2, si = np.rint(2 * c).astype(np.int64), int(s)                   # centre in halves, integer side
        for got, cc in ((X, c2[0]), (Y, c2[1])):
            want = (cc * O - si * O + O + 2 * t * si) // (2 * O)
            assert np.array_equal(got, want), (c, s)


def test_roi_transform_rejects_bad_windows():
    from hs_pose_amd.pc_sample import roi_transform
    for c, s in (([[1.0, 2.0]], [0.0]), ([[1.0, 2.0]], [-3.0]), ([[np.nan, 2.0]], [40.0]), ([[1.0, 2.0]], [np.inf]),
                 ([[1.0, 2.0]], [40.0, 80.0])):
        with pytest.raises(ValueError):
            roi_transform(np.array(c), np.array(s), 256)


# ---- the wrappers refuse what they cannot run -------------------------------------------------------------------------------

def test_ops_reject_cpu_tensors_and_wrong_shapes():
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError
    H, W, n, O = 12, 16, 2, 8
    depth = torch.zeros(H, W)
    mask = torch.zeros(n, H, W, dtype=torch.uint8)
    xf = torch.zeros(n, 3, dtype=torch.float64)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.roi_compact(depth, mask, xf, O)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.roi_compact(depth.numpy(), mask, xf, O)
    src = torch.zeros(n, O * O, dtype=torch.int32)
    choose = torch.zeros(n, 5, dtype=torch.int32)
    K = torch.eye(3, dtype=torch.float64)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.frame_to_pcl(depth, K, src, choose)
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    depth, mask, xf, src, choose, K = (t.to(dev) for t in (depth, mask, xf, src, choose, K))
    for bad in (dict(depth=depth.double()), dict(depth=depth.reshape(1, H, W)), dict(mask=mask.float()),
                dict(mask=mask[:, :, :-1]), dict(mask=mask[:1]), dict(xf=xf.float()), dict(xf=xf[:, :2]), dict(xf=xf[:0]),
                dict(out_size=0), dict(inst_ids=torch.zeros(n + 1, dtype=torch.int32, device=dev)),
                dict(inst_ids=torch.zeros(n, dtype=torch.int64, device=dev)), dict(mask=mask.cpu()), dict(xf=xf.cpu())):
        args = dict(depth=depth, mask=mask, xf=xf, out_size=O, inst_ids=None)
        args.update(bad)
        with pytest.raises(HspError):
            ops.roi_compact(**args)
    for bad in (dict(depth=depth.double()), dict(camK64=K.float()), dict(camK64=torch.zeros(3, 3, 3, dtype=torch.float64, device=dev)),
                dict(src=src.long()), dict(src=src[:1]), dict(choose=choose.long()), dict(choose=choose[:, :0]),
                dict(choose=choose.cpu()), dict(src=src.reshape(-1))):
        args = dict(depth=depth, camK64=K, src=src, choose=choose)
        args.update(bad)
        with pytest.raises(HspError):
            ops.frame_to_pcl(**args)


def test_entry_points_validate_arguments_without_gpu():
    from hs_pose_amd._lib import lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    assert L.hsp_roi_compact_workspace_bytes(0, 256) == 0 and L.hsp_roi_compact_workspace_bytes(3, 0) == 0
    assert L.hsp_roi_compact_workspace_bytes(3, 16) == 3 * 1 * 8            # 256 pixels: one chunk, a pair of counts
    assert L.hsp_roi_compact_workspace_bytes(3, 64) == 3 * 1 * 8            # 4096: exactly one
    assert L.hsp_roi_compact_workspace_bytes(3, 96) == 3 * 3 * 8            # 9216: two chunks and a quarter
    assert L.hsp_roi_compact_workspace_bytes(4, 256) == 4 * 16 * 8
    for fn in (L.hsp_roi_compact_f32, L.hsp_roi_compact_u16):
        assert fn(null, one, 0, null, one, 1, 48, 64, 16, one, one, one, 64, null) == -1         # no depth
        assert fn(one, one, 0, null, one, 0, 48, 64, 16, one, one, one, 64, null) == -1          # n = 0
        assert fn(one, one, 5, null, one, 1, 48, 64, 16, one, one, one, 64, null) == -1          # mask stride neither 0 nor H*W
        assert fn(one, one, 0, null, one, 1, 65536, 65536, 16, one, one, one, 64, null) == -1    # H*W >= 2^31
        assert fn(one, one, 0, null, one, 1, 48, 64, 50000, one, one, one, 64, null) == -2       # O*O >= 2^31
        assert fn(one, one, 0, null, one, 70000, 48, 64, 16, one, one, one, 1 << 30, null) == -2  # n > 65535 (grid.y)
        assert fn(one, one, 0, null, one, 2, 48, 64, 96, one, one, null, 0, null) == -3          # no workspace
        assert fn(one, one, 0, null, one, 2, 48, 64, 96, one, one, one, 47, null) == -3          # workspace too small
    for fn in (L.hsp_frame_to_pcl_f32, L.hsp_frame_to_pcl_u16):
        assert fn(one, 48, 64, null, 1, one, 256, one, 2, 8, one, null) == -1                    # no camK
        assert fn(one, 48, 64, one, 3, one, 256, one, 2, 8, one, null) == -1                     # camK rows neither 1 nor n
        assert fn(one, 48, 64, one, 1, one, 0, one, 2, 8, one, null) == -1                       # src pitch 0
        assert fn(one, 48, 64, one, 1, one, 256, one, 2, 0, one, null) == -1                     # S = 0


def test_header_exports_and_table_agree():
    from hs_pose_amd import _lib
    txt = open(os.path.join(ROOT, "include", "hsp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", txt)))
    new = ["hsp_frame_to_pcl_f32", "hsp_frame_to_pcl_u16", "hsp_roi_compact_f32", "hsp_roi_compact_u16",
           "hsp_roi_compact_workspace_bytes"]
    assert all(s in syms for s in new)
    L = _lib.lib()
    assert all(hasattr(L, s) for s in syms) and sorted(_lib.SIGNATURES) == syms


# ---- the restatement against itself: compaction == boolean indexing of the three crops ---------------------------------------

def test_restatement_compaction_is_the_boolean_indexing_of_the_crops():
    """ref_compact (what the kernels are compared with) == the loader's own order of operations on the three crops"""
    rng = np.random.RandomState(3)
    H, W, O = 48, 64, 32
    depth = (rng.rand(H, W) * 900 * (rng.rand(H, W) > 0.2)).astype(np.float32)
    mask = (rng.rand(H, W) > 0.4).astype(np.uint8)
    for center, scale in (((30.5, 20.0), 24.0), ((5.0, 40.0), 40.0), ((31.7, 22.3), 17.9)):
        xf = ref_xf(center, scale, O)
        coord, rm, rd = ref_crops(depth, mask, xf, O)
        valid = ((rd.reshape(-1) > 0) * rm.reshape(-1)) > 0
        src, counts = ref_compact(depth, mask != 0, xf, O)
        assert counts == [int(valid.sum()), int((rd > 0).sum())]
        assert np.array_equal(src % W, coord[0].reshape(-1)[valid]) and np.array_equal(src // W, coord[1].reshape(-1)[valid])
