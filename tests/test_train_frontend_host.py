"""CPU: the host half of the training loader's front end -- ``pc_sample.dzi_windows`` against recorded runs of the reference's
``aug_bbox_DZI`` (tests/golden/train_dzi_windows.npz, tools/gen_golden_train_frontend.py), the mask rule of include/hsp.h
through its numpy restatement (tests/_roi_defor_ref.py): the triangle footprint is the iterated one-step rule, the gate and
the subset have the stated distributions --, and the argument checks of the new entry points, which launch nothing."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _roi_defor_ref as rr
import _sample_ids_ref as sr
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234


# ---- dzi_windows against the reference's aug_bbox_DZI ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dzi():
    return golden("train_dzi_windows")


def test_fixture_matches_its_manifest(dzi):
    with open(os.path.join(ROOT, "tests", "golden", "train_frontend_manifest.json")) as f:
        man = json.load(f)["files"]["train_dzi_windows"]
    assert {k: [list(dzi[k].shape), str(dzi[k].dtype)] for k in dzi.files} == man


def test_fixture_covers_the_edges(dzi):
    b, (H, W) = dzi["boxes"], dzi["im_hw"]
    assert len(b) == 64
    assert (b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == W).any() and (b[:, 3] == H).any()
    assert ((b[:, 2] - b[:, 0] > W) & (b[:, 3] - b[:, 1] > H)).any()                 # a box larger than the frame
    for kind in ("uniform", "none"):                                                  # the min(scale, max(H, W)) clamp fires
        assert (dzi["scales_" + kind] == max(H, W)).any() and (dzi["scales_" + kind] < max(H, W)).any()


@pytest.mark.parametrize("kind", ["uniform", "none"])
def test_dzi_windows_match_reference(dzi, flags, kind):
    from hs_pose_amd.pc_sample import dzi_windows
    H, W = (int(v) for v in dzi["im_hw"])
    flags.DZI_TYPE = kind
    np.random.seed(int(dzi["seed"][0]))
    centers, scales = dzi_windows(dzi["boxes"], H, W)
    state = np.random.get_state()
    assert centers.dtype == np.float64 and centers.shape == (64, 2) and scales.dtype == np.float64 and scales.shape == (64,)
    assert np.array_equal(centers, dzi["centers_" + kind]) and np.array_equal(scales, dzi["scales_" + kind])
    assert np.array_equal(state[1], dzi["state_keys_" + kind]) and state[2] == int(dzi["state_pos_" + kind][0])
    np.random.seed(int(dzi["seed"][0]))
    fresh = np.random.get_state()
    drew = not (np.array_equal(state[1], fresh[1]) and state[2] == fresh[2])
    assert drew == (kind == "uniform")                                                # three doubles per box, or none


def test_dzi_flags_and_unbuilt_types(flags):
    from hs_pose_amd.pc_sample import dzi_windows, mask_gate
    assert (flags.DZI_PAD_SCALE, flags.DZI_TYPE, flags.DZI_SCALE_RATIO, flags.DZI_SHIFT_RATIO) == (1.5, "uniform", 0.25, 0.25)
    assert (flags.roi_mask_pro, flags.roi_mask_r) == (0.5, 3)
    for kind in ("roi10d", "ROI10D", "truncnorm"):
        flags.DZI_TYPE = kind
        with pytest.raises(NotImplementedError):
            dzi_windows(np.array([[0, 0, 10, 10]]), 480, 640)
    flags.DZI_TYPE = "uniform"
    with pytest.raises(ValueError):
        dzi_windows(np.array([0, 0, 10, 10]), 480, 640)
    assert [mask_gate(p) for p in (-0.1, 0.0, 0.5, 1.0, 1.5)] == [0, 0, 2 ** 31, 2 ** 32, 2 ** 32]
    assert mask_gate(0.3) == int(np.floor(0.3 * 2.0 ** 32))


# ---- the morphology ---------------------------------------------------------------------------------------------------------

def _masks():
    O = 24
    yy, xx = np.mgrid[0:O, 0:O]
    disc = ((yy - 11) ** 2 + (xx - 13) ** 2 < 49).astype(np.uint8)
    pixel = np.zeros((O, O), np.uint8)
    pixel[9, 14] = 1
    out = {"disc": disc, "pixel": pixel, "full": np.ones((O, O), np.uint8), "empty": np.zeros((O, O), np.uint8)}
    for name, sl in (("top", np.s_[0:3, 5:15]), ("left", np.s_[6:16, 0:2]), ("bottom", np.s_[O - 2:O, 4:20]),
                     ("right", np.s_[3:9, O - 3:O]), ("corner", np.s_[0:1, 0:1])):
        m = np.zeros((O, O), np.uint8)
        m[sl] = 1
        out[name] = m
    return out


@pytest.mark.parametrize("r", [1, 2, 3])
def test_triangle_footprint_is_the_iterated_one_step_rule(r):
    for name, m in _masks().items():
        E, D = rr.erode_dilate(m, r)
        e, d = m.copy(), m.copy()
        for _ in range(r):
            e, d = rr.one_step_loops(e, min), rr.one_step_loops(d, max)
        assert np.array_equal(E, e) and np.array_equal(D, d), (name, r)
        assert (E <= m).all() and (m <= D).all()
    E, D = rr.erode_dilate(_masks()["full"], r)
    assert E.all() and D.all()                                # positions outside the crop are left out: a full crop has no band
    E, D = rr.erode_dilate(_masks()["pixel"], r)
    assert E.sum() == 0 and D.sum() == (r + 1) * (r + 2) // 2 and D[9:9 + r + 1, 14:14 + r + 1].sum() == D.sum()


@pytest.mark.parametrize("r", [1, 2, 3])
def test_morphology_equals_scipy_filters(r):
    """scipy.ndimage expresses footprint, anchor and borders: minimum_filter / maximum_filter with the 2 x 2 element (its
    default centre of an even size is the element's (1,1)) and a constant border of 1 / 0, iterated r times; and in one pass
    with the triangle as footprint and the origin moved to its corner.  grey_erosion is minimum_filter; grey_dilation REFLECTS
    the footprint (a dilation in the textbook sense, which cv2.dilate does not do), so it is not used."""
    ndi = pytest.importorskip("scipy.ndimage")
    fp = np.array([[0, 1], [1, 1]], bool)
    T = np.zeros((r + 1, r + 1), bool)
    for j in range(r + 1):
        T[r - j, j:] = True                         # row j up holds columns 0 .. r - j to the left
    o = r - (r + 1) // 2
    for name, m in _masks().items():
        E, D = rr.erode_dilate(m, r)
        e, d = m.copy(), m.copy()
        for _ in range(r):
            e = ndi.minimum_filter(e, footprint=fp, mode="constant", cval=1)
            d = ndi.maximum_filter(d, footprint=fp, mode="constant", cval=0)
        assert np.array_equal(E, e) and np.array_equal(D, d), (name, r)
        assert np.array_equal(E, ndi.minimum_filter(m, footprint=T, mode="constant", cval=1, origin=(o, o))), (name, r)
        assert np.array_equal(D, ndi.maximum_filter(m, footprint=T, mode="constant", cval=0, origin=(o, o))), (name, r)


def test_defor_leaves_everything_off_the_band_alone():
    m = _masks()["disc"]
    for r in (1, 3):
        E, D = rr.erode_dilate(m, r)
        band = E != D
        for gate in (0, 2 ** 32):
            cb, (l, deformed) = rr.defor(m, r, gate, SEED, 3, 2)
            assert l == band.sum() and deformed == (gate != 0)
            assert np.array_equal(cb >> 1, m) and np.array_equal((cb & 1)[~band], m[~band])
            if deformed:
                assert int(((cb & 1)[band] == 0).sum()) == l // 2
            else:
                assert np.array_equal(cb & 1, m)
    for name in ("full", "empty"):                            # l = 0: never deformed, whatever the gate
        cb, info = rr.defor(_masks()[name], 1, 2 ** 32, SEED, 0, 0)
        assert info == [0, 0] and np.array_equal(cb & 1, _masks()[name])


# ---- the distributions (seed 1234) -------------------------------------------------------------------------------------------

def test_gate_deforms_half_at_half():
    """gate = 2^31 over calls 0..63 x instances 0..7: a fair coin 512 times, sd = sqrt(128) = 11.3; within 256 +- 5 sd"""
    hits = sum(rr.gate_draw(SEED, call, j) < 2 ** 31 for call in range(64) for j in range(8))
    print(f"deformed {hits} of 512")
    assert abs(hits - 256) <= 5 * np.sqrt(128)
    assert all(rr.gate_draw(SEED, c, j) < 2 ** 32 for c in range(4) for j in range(4))        # gate 2^32 always, gate 0 never


@pytest.mark.parametrize("l", [7, 41, 300])
def test_subset_is_exact_in_size_and_uniform(l):
    """2000 calls: P is a permutation, exactly l // 2 ranks are zeroed every call, every rank's zero count lies within 5
    binomial sd of 2000 (l // 2) / l"""
    T = 2000
    zeros = np.zeros(l, dtype=np.int64)
    for call in range(T):
        kd = sr.absorb(sr.instance_key(SEED, call, 0), rr.SUBSET_DOMAIN)
        P = sr.permute(np.arange(l), l, kd)
        assert np.array_equal(np.sort(P), np.arange(l))
        z = rr.subset_zero(l, SEED, call, 0)
        assert np.array_equal(z, P < l // 2) and int(z.sum()) == l // 2
        zeros += z
    p = (l // 2) / l
    dev = np.abs(zeros - T * p) / np.sqrt(T * p * (1 - p))
    print(f"l {l}: max deviation {dev.max():.2f} sd")
    assert dev.max() <= 5.0


def test_domains_keep_the_draws_apart():
    kj = sr.instance_key(SEED, 0, 0)
    words = [int(sr.absorb(kj, w)[0]) for w in (0, 1, 2, 3, 0xffffffff, rr.GATE_DOMAIN, rr.SUBSET_DOMAIN)]
    assert len(set(words)) == len(words)


# ---- the wrappers and entry points refuse what they cannot run ---------------------------------------------------------------

def test_ops_reject_cpu_tensors():
    from hs_pose_amd import ops, pc_sample
    from hs_pose_amd._lib import HspError
    mask = torch.zeros(2, 12, 16, dtype=torch.uint8)
    xf = torch.zeros(2, 3, dtype=torch.float64)
    key = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.roi_defor(mask, xf, 8, key)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.crop_compact(torch.zeros(12, 16), torch.zeros(2, 64, dtype=torch.uint8), xf, 8)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.frames_to_pcl(torch.zeros(12, 16), torch.eye(3, dtype=torch.float64), torch.zeros(2, 64, dtype=torch.int32),
                          torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="device sampler"):
        pc_sample.train_batch_to_pcl(torch.zeros(12, 16), mask, None, np.zeros((2, 2)), np.ones(2), np.eye(3), sampler="host")


def test_entry_points_validate_arguments_without_gpu():
    """every case the header lists is HSP_ERR_BAD_ARG (-1) before any launch"""
    from hs_pose_amd._lib import lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    assert L.hsp_roi_defor_workspace_bytes(3, 16) == 3 * 4 and L.hsp_roi_defor_workspace_bytes(3, 64) == 3 * 4
    assert L.hsp_roi_defor_workspace_bytes(3, 96) == 3 * 3 * 4 and L.hsp_roi_defor_workspace_bytes(16, 256) == 16 * 16 * 4
    assert L.hsp_crop_compact_workspace_bytes(3, 96) == 3 * 3 * 12 and L.hsp_crop_compact_workspace_bytes(0, 96) == 0
    big = 1 << 30

    def defor(mask=one, stride=0, n=2, H=48, W=64, O=16, iters=1, gate=0, key=one, out=one, band=one, ws=one, wsb=big):
        return L.hsp_roi_defor(mask, stride, null, one, n, H, W, O, iters, gate, key, out, band, ws, wsb, null)
    for kw in (dict(iters=0), dict(iters=9), dict(iters=-1), dict(gate=2 ** 32 + 1), dict(gate=2 ** 64 - 1), dict(n=65536),
               dict(n=0), dict(O=46341), dict(O=0), dict(H=65536, W=32768), dict(stride=5), dict(stride=48 * 64 + 1),
               dict(mask=null), dict(key=null), dict(out=null), dict(band=null)):
        assert defor(**kw) == -1, kw
    assert defor(ws=null, wsb=0) == -3 and defor(n=2, O=96, wsb=23) == -3
    for fn in (L.hsp_crop_compact_f32, L.hsp_crop_compact_u16):
        def crop(depth=one, stride=0, n=2, H=48, W=64, O=16, pre=one, ws=one, wsb=big):
            return fn(depth, stride, one, one, n, H, W, O, one, one, pre, ws, wsb, null)
        for kw in (dict(n=65536), dict(O=46341), dict(H=65536, W=32768), dict(stride=7), dict(depth=null), dict(pre=null)):
            assert crop(**kw) == -1, kw
        assert crop(ws=null, wsb=0) == -3 and crop(O=96, wsb=71) == -3
    for fn in (L.hsp_frames_to_pcl_f32, L.hsp_frames_to_pcl_u16):
        def pcl(depth=one, stride=0, H=48, W=64, rows=1, pitch=256, n=2, S=8):
            return fn(depth, stride, H, W, one, rows, one, pitch, one, n, S, one, null)
        for kw in (dict(n=65536), dict(H=65536, W=32768), dict(stride=7), dict(depth=null), dict(rows=3), dict(pitch=0),
                   dict(S=0), dict(n=65535, S=40000)):
            assert pcl(**kw) == -1, kw
