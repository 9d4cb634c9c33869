"""The training loader's front end on the GPU (csrc/frontend.hip: hsp_roi_defor, hsp_crop_compact_*, hsp_frames_to_pcl_*;
pc_sample.train_batch_to_pcl) against the numpy restatement of the mask rule (tests/_roi_defor_ref.py, written from
include/hsp.h) and against the pinned ``pc_sample.depth_to_pcl`` path run on crops and deformed masks built by that
restatement.  Everything compared is integers or bits: equality is exact, no tolerance anywhere."""
import numpy as np
import pytest
import torch

import _roi_defor_ref as rr
import test_frame_host as fh

pytestmark = pytest.mark.gpu

K_REAL = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)   # REAL275 intrinsics
KEYS = ((1234, 0), (2 ** 64 - 5, 2 ** 33 + 7))                       # two key states: (seed, call counter)

# windows on the 48 x 64 frame, the first three those of tests/test_gpu_frame.py: scale < every O over the left and top edges
# (replicated source pixels); scale > every O over all four edges; a non-integer centre and scale over the right and bottom
# edges; a window inside the frame; a non-integer one near the left edge
CENTERS = np.array([[3.0, 5.0], [50.0, 30.0], [55.37, 40.81], [32.0, 24.0], [20.5, 30.25]])
SCALES = np.array([12.0, 120.0, 33.3, 40.0, 17.0])
H, W, B = 48, 64, 5


def _depth(rng, shape, dtype, zeros=0.25):
    d = rng.randint(1, 3000, size=shape).astype(np.float32)
    if dtype == "f32":
        d += rng.rand(*shape).astype(np.float32) - np.float32(0.999)
        d[rng.rand(*shape) < 0.05] = -3.0
    d[rng.rand(*shape) < zeros] = 0
    return d if dtype == "f32" else d.astype(np.uint16)


def _key(seed, call, dev):
    from hs_pose_amd.pc_sample import DeviceSampler
    s = DeviceSampler(seed, dev)
    s.set_state((seed, call))
    return s.advance()


def _xfs(O):
    from hs_pose_amd.pc_sample import roi_transform
    xf = roi_transform(CENTERS, SCALES, O)
    for j in range(B):
        assert tuple(xf[j].tolist()) == fh.ref_xf(CENTERS[j], SCALES[j], O)
    return xf


def _small_masks(mode, O, xf, rng):
    """-> (mask array for the kernel, inst ids or None, belongs (B,H,W) bool).  'masks': a blob under a 12 -> O zoom, a disc
    under a window over every frame edge, the frame pixels behind the crop's first row and first column, a full crop, one
    pixel.  'labels': one label image for all, one id absent (an empty mask).  'labels_each': a label image per instance."""
    yy, xx = np.mgrid[0:H, 0:W]
    if mode == "masks":
        m = np.zeros((B, H, W), np.uint8)
        m[0] = (rng.rand(H, W) < 0.6) * rng.randint(1, 256, size=(H, W))
        m[1] = ((yy - 26) ** 2 + (xx - 40) ** 2 < 330) * 200
        X, Y = fh.ref_map(tuple(xf[2].tolist()), O)
        assert 0 <= X[0] < W and 0 <= Y[0] < H
        m[2, Y[0], :] = 1
        m[2, :, X[0]] = 9
        m[3] = 1
        X, Y = fh.ref_map(tuple(xf[4].tolist()), O)
        m[4, Y[O // 2], X[O // 2]] = 77                       # one frame pixel, one the crop does sample
        return m, None, m != 0
    ids = np.array([2, 0, 3, 1, 7], dtype=np.int32)
    if mode == "labels":
        m = rng.randint(0, 4, size=(H, W)).astype(np.uint8)
        return m, ids, np.stack([m == i for i in ids])
    m = rng.randint(0, 4, size=(B, H, W)).astype(np.uint8)
    m[4, 10:30, 5:40] = 7
    return m, ids, np.stack([m[j] == ids[j] for j in range(B)])


@pytest.mark.parametrize("mode", ["masks", "labels", "labels_each"])
@pytest.mark.parametrize("O", [16, 64, 96])          # 256 crop pixels: under one chunk; 4096: exactly one; 9216: two and a quarter
def test_crop_mask_and_band_equal_restatement(dev, O, mode):
    from hs_pose_amd import ops
    rng = np.random.RandomState(200 + O)
    xf = _xfs(O)
    xf_d = torch.from_numpy(xf).to(dev)
    mask, ids, belongs = _small_masks(mode, O, xf, rng)
    mask_d = torch.from_numpy(mask).to(dev)
    ids_d = None if ids is None else torch.from_numpy(ids).to(dev)
    ms = [rr.crop_m(belongs[j], tuple(xf[j].tolist()), O) for j in range(B)]
    if mode == "masks":
        assert ms[3].all() and ms[2][0, :O // 2].all() and ms[2][:O // 2, 0].all() and 1 <= ms[4].sum() < 40   # (first row / column: up to the frame's edge)
    if mode == "labels":
        assert not ms[4].any()
    if O == 96:                                               # band ranks and offsets cross both chunk boundaries
        E, D = rr.erode_dilate(ms[0], 1)
        q = np.flatnonzero((E != D).reshape(-1))
        assert q.min() < 4096 and q.max() >= 8192 and ((q >= 4096) & (q < 8192)).any()
    seen = set()
    for seed, call in KEYS:
        key = _key(seed, call, dev)
        for iters in (1, 2, 3):
            for gate in (0, 2 ** 32, 2 ** 31):
                cm, band = ops.roi_defor(mask_d, xf_d, O, key, ids_d, iters, gate)
                cm, band = cm.cpu().numpy(), band.cpu().numpy()
                assert cm.shape == (B, O * O) and cm.dtype == np.uint8 and band.shape == (B, 2)
                for j in range(B):
                    want, info = rr.defor(ms[j], iters, gate, seed, call, j)
                    assert band[j].tolist() == info, (j, iters, gate, seed, band[j], info)
                    assert np.array_equal(cm[j].reshape(O, O), want), (j, iters, gate, seed)
                    seen.add((gate, info[1]))
                if gate == 0:
                    assert not band[:, 1].any() and np.array_equal(cm & 1, cm >> 1)
                if gate == 2 ** 32:
                    assert np.array_equal(band[:, 1], (band[:, 0] >= 1).astype(np.int32))
                if mode == "masks":
                    assert band[3].tolist() == [0, 0]                 # a full crop has no band
                if mode == "labels":
                    assert band[4].tolist() == [0, 0]                 # nor has an empty mask
    assert (2 ** 32, 1) in seen and (0, 0) in seen
    # bit 1 is the mask hsp_roi_compact uses: with depth everywhere its compaction lists exactly the crop pixels with bit 1
    cm, _ = ops.roi_defor(mask_d, xf_d, O, key, ids_d, 1, 0)
    src, count = ops.roi_compact(torch.ones(H, W, device=dev), mask_d, xf_d, O, ids_d)
    cm, src, count = cm.cpu().numpy(), src.cpu().numpy(), count.cpu().numpy()
    for j in range(B):
        p = fh.ref_source(tuple(xf[j].tolist()), O, H, W).reshape(-1)
        assert count[j, 0] == (cm[j] >> 1).sum() and np.array_equal(src[j, :count[j, 0]], p[(cm[j] >> 1) == 1])


def _check_compact(got, depth, cm, xf, O):
    src, count, pre = (t.cpu().numpy() for t in got)
    assert src.shape == (len(xf), O * O) and count.shape == (len(xf), 2) and pre.shape == (len(xf),)
    for j in range(len(xf)):
        want, counts, p = rr.crop_compact(depth[j] if depth.ndim == 3 else depth, cm[j], tuple(xf[j].tolist()), O)
        assert count[j].tolist() == counts and pre[j] == p, (j, count[j], counts, pre[j], p)
        assert np.array_equal(src[j, :counts[0]], want), j
    return src, count, pre


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("O", [16, 64, 96])
def test_compaction_equals_restatement(dev, O, dtype):
    from hs_pose_amd import ops
    rng = np.random.RandomState(300 + O)
    xf = _xfs(O)
    xf_d = torch.from_numpy(xf).to(dev)
    mask, _, belongs = _small_masks("masks", O, xf, rng)
    mask_d = torch.from_numpy(mask).to(dev)
    depth = _depth(rng, (B, H, W), dtype)
    depth_d = torch.from_numpy(depth).to(dev)
    seed, call = KEYS[0]
    key = _key(seed, call, dev)
    cm_d, band = ops.roi_defor(mask_d, xf_d, O, key, None, 2, 2 ** 32)
    cm = cm_d.cpu().numpy()
    for j in range(B):
        assert np.array_equal(cm[j].reshape(O, O), rr.defor(rr.crop_m(belongs[j], tuple(xf[j].tolist()), O), 2, 2 ** 32, seed, call, j)[0])
    src, count, pre = _check_compact(ops.crop_compact(depth_d, cm_d, xf_d, O), depth, cm, xf, O)
    assert (count[[0, 1, 3], 0] > 0).all() and (count[:, 1] >= count[:, 0]).all() and not np.array_equal(count[:, 0], pre)
    # one frame for all == B copies of it
    shared_d = torch.from_numpy(depth[1].copy()).to(dev)
    copies = np.stack([depth[1]] * B)
    one = _check_compact(ops.crop_compact(shared_d, cm_d, xf_d, O), depth[1], cm, xf, O)
    many = _check_compact(ops.crop_compact(torch.from_numpy(copies).to(dev), cm_d, xf_d, O), copies, cm, xf, O)
    assert np.array_equal(one[1], many[1]) and np.array_equal(one[2], many[2])
    assert all(np.array_equal(one[0][j, :one[1][j, 0]], many[0][j, :one[1][j, 0]]) for j in range(B))
    # gate 0 and one frame: hsp_roi_compact's src and count, and pre == count[:, 0]
    cm0, _ = ops.roi_defor(mask_d, xf_d, O, key, None, 2, 0)
    src0, count0, pre0 = (t.cpu().numpy() for t in ops.crop_compact(shared_d, cm0, xf_d, O))
    rsrc, rcount = (t.cpu().numpy() for t in ops.roi_compact(shared_d, mask_d, xf_d, O))
    assert np.array_equal(count0, rcount) and np.array_equal(pre0, rcount[:, 0])
    assert all(np.array_equal(src0[j, :rcount[j, 0]], rsrc[j, :rcount[j, 0]]) for j in range(B))


def test_real_size(dev):
    """480 x 640 uint16 frames, O = 256, B = 2, DZI-like windows: 16 chunks per instance, a frame and a label image each"""
    from hs_pose_amd import ops
    from hs_pose_amd.pc_sample import roi_transform
    Hr, Wr, O = 480, 640, 256
    rng = np.random.RandomState(17)
    depth = _depth(rng, (2, Hr, Wr), "u16", zeros=0.3)
    yy, xx = np.mgrid[0:Hr, 0:Wr]
    labels = np.zeros((2, Hr, Wr), np.uint8)
    labels[0][(yy - 200) ** 2 + (xx - 300) ** 2 < 70 ** 2] = 5
    labels[1][(np.abs(yy - 400) < 60) & (np.abs(xx - 80) < 90) & ((yy + xx) % 7 != 0)] = 2
    ids = np.array([5, 2], dtype=np.int32)
    centers, scales = np.array([[310.7, 190.2], [61.3, 420.9]]), np.array([233.4, 301.9])
    xf = roi_transform(centers, scales, O)
    xf_d = torch.from_numpy(xf).to(dev)
    seed, call = KEYS[1]
    cm_d, band = ops.roi_defor(torch.from_numpy(labels).to(dev), xf_d, O, _key(seed, call, dev), torch.from_numpy(ids).to(dev),
                               1, 2 ** 32)
    cm, band = cm_d.cpu().numpy(), band.cpu().numpy()
    for j in range(2):
        want, info = rr.defor(rr.crop_m(labels[j] == ids[j], tuple(xf[j].tolist()), O), 1, 2 ** 32, seed, call, j)
        assert band[j].tolist() == info and info[0] > 300 and np.array_equal(cm[j].reshape(O, O), want), (j, band[j], info)
    _check_compact(ops.crop_compact(torch.from_numpy(depth).to(dev), cm_d, xf_d, O), depth, cm, xf, O)


def test_past_256_chunks(dev):
    """one instance at O = 1040 on a 96 x 128 frame: 1 081 600 crop pixels in 265 chunks, so the write kernels' sums over the
    chunk counts (one count per thread, 256 threads) make a second trip, in all three forms that read a crop; and the
    back-projection of one frame by both of its entry points, bit for bit"""
    from hs_pose_amd import ops
    Hh, Ww, O = 96, 128, 1040
    OO, past = O * O, 256 * 4096
    xf = fh.ref_xf((64.0, 48.0), 90.0, O)
    assert (fh.ref_source(xf, O, Hh, Ww) >= 0).all()                             # the whole crop maps inside the frame
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    mask = ((yy // 3 + xx // 3) % 4 != 0).astype(np.uint8)
    rng = np.random.RandomState(1)
    depth32 = (rng.rand(Hh, Ww) * 2000).astype(np.float32)
    depth32[rng.rand(Hh, Ww) < 0.2] = 0
    xf_d = torch.tensor([xf], dtype=torch.float64, device=dev)
    mask_d = torch.from_numpy(mask[None]).to(dev)
    m = rr.crop_m(mask != 0, xf, O)
    seed, call = KEYS[0]
    key = _key(seed, call, dev)
    cms = {}
    for gate in (2 ** 32, 0):
        cm_d, band = ops.roi_defor(mask_d, xf_d, O, key, None, 1, gate)
        want, info = rr.defor(m, 1, gate, seed, call, 0)
        assert band.cpu().tolist() == [info] and info == [30775, int(gate != 0)]
        assert np.array_equal(cm_d.cpu().numpy().reshape(O, O), want), gate
        cms[gate] = cm_d, want
    E, D = rr.erode_dilate(m, 1)
    assert (np.flatnonzero((E != D).reshape(-1)) >= past).sum() == 961           # band ranks past the 256th chunk
    K_d = torch.from_numpy(K_REAL).to(dev)
    for depth in (depth32, depth32.astype(np.uint16)):
        depth_d = torch.from_numpy(depth).to(dev)
        want, counts = fh.ref_compact(depth, mask != 0, xf, O)
        p = fh.ref_source(xf, O, Hh, Ww).reshape(-1)
        per_chunk = np.bincount(np.flatnonzero((depth.reshape(-1)[p] > 0) & (mask.reshape(-1)[p] != 0)) // 4096, minlength=265)
        assert per_chunk.sum() == counts[0] > 600000 and per_chunk.min() >= 100 and per_chunk[256:].sum() > 10000
        src_d, count = ops.roi_compact(depth_d, mask_d, xf_d, O)
        assert src_d.shape == (1, OO) and count.cpu().tolist() == [counts]
        assert np.array_equal(src_d[0, :counts[0]].cpu().numpy(), want)
        for gate, (cm_d, cbytes) in cms.items():
            _check_compact(ops.crop_compact(depth_d[None], cm_d, xf_d, O), depth[None], cbytes.reshape(1, OO), [np.array(xf)], O)
        choose = torch.tensor([[0, counts[0] - 1, -1, counts[0] // 2, OO + 3, 1, OO]], dtype=torch.int32, device=dev)
        one = ops.frame_to_pcl(depth_d, K_d, src_d, choose)
        many = ops.frames_to_pcl(depth_d, K_d, src_d, choose)
        assert one.shape == many.shape == (1, 7, 3) and torch.equal(one.view(torch.int32), many.view(torch.int32))
        assert torch.isnan(one[0, [2, 4, 6]]).all() and torch.isfinite(one[0, [0, 1, 3, 5]]).all()


def _put_depth(frame, xf, O, crop_pixels, value):
    """give the frame pixels behind the listed crop pixels (flat ids) a depth"""
    p = fh.ref_source(xf, O, *frame.shape).reshape(-1)[crop_pixels]
    assert (p >= 0).all() and len(np.unique(p)) == len(p)
    frame.reshape(-1)[p] = value


def _tie_batch(dtype, n_pts, O):
    """three items on 96 x 128 frames of their own: short (a 15-pixel mask under a 20 -> 64 zoom), long (a disc), exactly n_pts
    (a 1:1 window inside the frame under a full mask -- no band, nothing to deform -- with depth on n_pts of its pixels)"""
    Hh, Ww = 96, 128
    rng = np.random.RandomState(11)
    depth = _depth(rng, (3, Hh, Ww), dtype, zeros=0.2)
    centers = np.array([[30.0, 40.0], [70.5, 50.5], [64.0, 48.0]])
    scales = np.array([20.0, 90.0, float(O)])
    mask = np.zeros((3, Hh, Ww), np.uint8)
    mask[0, 38:41, 26:31] = 1
    depth[0, 36:43, 24:33] = np.maximum(depth[0, 36:43, 24:33], 1)             # (no holes under the short one: it stays >= 50)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    mask[1] = (yy - 50) ** 2 + (xx - 70) ** 2 < 30 ** 2
    mask[2] = 1
    depth[2] = 0
    _put_depth(depth[2], fh.ref_xf(centers[2], scales[2], O), O, rng.permutation(O * O)[:n_pts], 900)
    return depth, mask, centers, scales


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_clouds_tie_to_the_pinned_path(dev, dtype):
    """crops and deformed masks built on the CPU by the restatement -> the existing pc_sample.depth_to_pcl; the frames ->
    train_batch_to_pcl; samplers in the same state: same j, count and short_mode, so the same rows and the same bits"""
    from hs_pose_amd.pc_sample import DeviceSampler, depth_to_pcl, train_batch_to_pcl
    n_pts, O = 256, 64
    depth, mask, centers, scales = _tie_batch(dtype, n_pts, O)
    seed, call = 77, 5
    crops, dmask, counts = [], [], []
    for j in range(3):
        xf = fh.ref_xf(centers[j], scales[j], O)
        crops.append(fh.ref_crops(depth[j], mask[j], xf, O))
        cb, info = rr.defor(rr.crop_m(mask[j] != 0, xf, O), 1, 2 ** 32, seed, call, j)
        assert info[1] == (j != 2)                                               # the full crop has no band
        dmask.append(cb & 1)
        counts.append(rr.crop_compact(depth[j], cb, xf, O)[1][0])
    assert 50 <= counts[0] < n_pts < counts[1] and counts[2] == n_pts, counts
    xymap = torch.from_numpy(np.stack([c[0] for c in crops])).to(dev)
    roi_mask = torch.from_numpy(np.stack(dmask).astype(np.float32)).reshape(3, 1, O, O).to(dev)
    roi_depth = torch.from_numpy(np.stack([c[2] for c in crops]).astype(np.float32)).reshape(3, 1, O, O).to(dev)
    pinned = DeviceSampler(seed, dev)
    pinned.set_state((seed, call))
    want = depth_to_pcl(roi_depth, K_REAL, xymap, roi_mask, n_pts=n_pts, min_pts=50, sampler=pinned)
    mine = DeviceSampler(seed, dev)
    mine.set_state((seed, call))
    before = np.random.get_state()[1].copy()
    got, status = train_batch_to_pcl(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), None, centers, scales,
                                     K_REAL, n_pts=n_pts, out_size=O, min_pts=50, mask_pro=1.0, sampler=mine)
    assert want is not None and got.shape == (3, n_pts, 3) and got.dtype == torch.float32 and status.dtype == torch.int32
    assert status.cpu().tolist() == [0, 0, 0] and mine.get_state() == pinned.get_state() == (seed, call + 1)
    assert torch.equal(got, want)
    assert np.array_equal(before, np.random.get_state()[1])
    # label images with ids and a camera per item: the same bits; the whole chain equals its restatement too
    mine.set_state((seed, call))
    again, _ = train_batch_to_pcl(torch.from_numpy(depth).to(dev), torch.from_numpy(mask * np.array([4, 5, 6], np.uint8)[:, None, None]).to(dev),
                                  [4, 5, 6], centers, scales, np.stack([K_REAL] * 3), n_pts=n_pts, out_size=O, mask_pro=1.0, sampler=mine)
    assert torch.equal(again, want)
    cpu_pc, cpu_status = rr.cpu_train_batch_to_pcl(depth, mask != 0, centers, scales, K_REAL, n_pts, O, 1, 2 ** 32, seed, call)
    assert cpu_status.tolist() == [0, 0, 0] and np.array_equal(got.cpu().numpy(), cpu_pc)


def test_status_bits_and_nan_rows(dev):
    """49 valid pixels: bit 0; one pixel with depth: bit 1 (and, being one, bits 0 and 2); a comb mask with depth only on its
    dilated rim -- nothing before the deformation, hundreds after: bit 2 alone; an ordinary item beside them is untouched"""
    from hs_pose_amd.pc_sample import DeviceSampler, mask_gate, train_batch_to_pcl
    Hh, Ww, O, n_pts = 96, 128, 64, 64
    rng = np.random.RandomState(23)
    centers = np.array([[64.0, 48.0]] * 3 + [[70.5, 50.5]])
    scales = np.array([float(O)] * 3 + [90.0])
    xf1 = fh.ref_xf(centers[0], scales[0], O)                                    # a 1:1 window inside the frame
    mask = np.ones((4, Hh, Ww), np.uint8)
    depth = np.zeros((4, Hh, Ww), np.float32)
    _put_depth(depth[0], xf1, O, rng.permutation(O * O)[:49], 800.0)
    _put_depth(depth[1], xf1, O, np.array([O * 20 + 33]), 800.0)
    comb = np.zeros((Hh, Ww), np.uint8)
    comb[20:76, 36:92:3] = 1                                                     # one-pixel columns, two apart
    m2 = rr.crop_m(comb != 0, xf1, O)
    E, D = rr.erode_dilate(m2, 1)
    rim = (D == 1) & (m2 == 0)
    assert rim.sum() > 1000 and not E.any()
    mask[2] = comb
    _put_depth(depth[2], xf1, O, np.flatnonzero(rim.reshape(-1)), 750.0)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    mask[3] = (yy - 50) ** 2 + (xx - 70) ** 2 < 30 ** 2
    depth[3] = _depth(rng, (Hh, Ww), "f32", zeros=0.2)
    seed, call = 4321, 9
    s = DeviceSampler(seed, dev)
    s.set_state((seed, call))
    before = np.random.get_state()
    PC, status = train_batch_to_pcl(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), None, centers, scales,
                                    K_REAL, n_pts=n_pts, out_size=O, min_pts=50, mask_pro=1.0, sampler=s)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    want_pc, want_status = rr.cpu_train_batch_to_pcl(depth, mask != 0, centers, scales, K_REAL, n_pts, O, 1, mask_gate(1.0),
                                                     seed, call)
    cb2, _ = rr.defor(m2, 1, 2 ** 32, seed, call, 2)
    _, counts2, pre2 = rr.crop_compact(depth[2], cb2, xf1, O)
    assert pre2 == 0 and counts2[0] >= 50, (pre2, counts2)
    status, PC = status.cpu().numpy(), PC.cpu().numpy()
    assert status.tolist() == [1, 7, 4, 0] == want_status.tolist()
    assert np.isnan(PC[:3]).all() and np.isfinite(PC[3]).all()
    assert np.array_equal(PC, want_pc, equal_nan=True)
    # min_pts 49 lets the first through, and the last comes out the same beside it
    s.set_state((seed, call))
    PC2, status2 = train_batch_to_pcl(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), None, centers, scales,
                                      K_REAL, n_pts=n_pts, out_size=O, min_pts=49, mask_pro=1.0, sampler=s)
    assert status2.cpu().tolist() == [0, 7, 4, 0] and np.array_equal(PC2[3].cpu().numpy(), PC[3])
    assert np.isfinite(PC2[0].cpu().numpy()).all()


def test_captured_call_equals_eager(dev):
    """train_batch_to_pcl inside torch.cuda.graph, every small array uploaded before the capture; replayed under two successive
    sampler states: each replay equals the eager call of a sampler in that state, bit for bit"""
    from hs_pose_amd.pc_sample import DeviceSampler, roi_transform, train_batch_to_pcl
    n_pts, O = 256, 64
    depth, mask, centers, scales = _tie_batch("u16", n_pts, O)
    depth_d, mask_d = torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev)
    xf_d = torch.from_numpy(roi_transform(centers, scales, O)).to(dev)
    K_d = torch.from_numpy(K_REAL).to(dev)
    args = dict(n_pts=n_pts, out_size=O, min_pts=50, mask_pro=0.5)
    s = DeviceSampler(99, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        train_batch_to_pcl(depth_d, mask_d, None, xf_d, None, K_d, sampler=s, **args)     # (warm-up: kernels loaded, pools grown)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    state = s.get_state()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        PC, status = train_batch_to_pcl(depth_d, mask_d, None, xf_d, None, K_d, sampler=s, **args)
    assert s.get_state() == state                                                # the captured call does not advance
    eager = DeviceSampler(99, dev)
    seen = []
    for _ in range(2):
        eager.set_state(s.get_state())
        s.advance()
        g.replay()
        want, want_status = train_batch_to_pcl(depth_d, mask_d, None, centers, scales, K_REAL, sampler=eager, **args)
        assert eager.get_state() == s.get_state()
        assert torch.equal(status, want_status) and torch.equal(PC.view(torch.int32), want.view(torch.int32))
        assert status.cpu().tolist() == [0, 0, 0]
        seen.append(PC.clone())
    assert not torch.equal(seen[0], seen[1])                                     # another key, other rows


def test_bad_arguments_touch_nothing(dev):
    """every case the header lists returns HSP_ERR_BAD_ARG and leaves the outputs as they were"""
    import ctypes
    from hs_pose_amd._lib import lib
    L = lib()
    O, n = 16, 2
    mask = torch.ones(n, H, W, dtype=torch.uint8, device=dev)
    depth = torch.ones(n, H, W, dtype=torch.float32, device=dev)
    xf = torch.from_numpy(_xfs(O)[:n].copy()).to(dev)
    key = _key(1, 0, dev)
    outs = dict(cm=torch.full((n, O * O), 0x55, dtype=torch.uint8, device=dev), band=torch.full((n, 2), -7, dtype=torch.int32, device=dev),
                src=torch.full((n, O * O), -7, dtype=torch.int32, device=dev), count=torch.full((n, 2), -7, dtype=torch.int32, device=dev),
                pre=torch.full((n,), -7, dtype=torch.int32, device=dev), pc=torch.full((n, 8, 3), 5.0, device=dev),
                ws=torch.zeros(1 << 16, dtype=torch.uint8, device=dev))
    keep = {k: v.clone() for k, v in outs.items()}
    choose = torch.zeros(n, 8, dtype=torch.int32, device=dev)
    K = torch.from_numpy(K_REAL).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    HW = H * W

    def defor(stride=HW, n=n, H=H, W=W, O=O, iters=1, gate=0):
        return L.hsp_roi_defor(p(mask), stride, None, p(xf), n, H, W, O, iters, gate, p(key), p(outs["cm"]), p(outs["band"]),
                               p(outs["ws"]), 1 << 16, None)

    def crop(stride=HW, n=n, H=H, W=W, O=O):
        return L.hsp_crop_compact_f32(p(depth), stride, p(outs["cm"]), p(xf), n, H, W, O, p(outs["src"]), p(outs["count"]),
                                      p(outs["pre"]), p(outs["ws"]), 1 << 16, None)

    def pcl(stride=HW, n=n, H=H, W=W):
        return L.hsp_frames_to_pcl_f32(p(depth), stride, H, W, p(K), 1, p(outs["src"]), O * O, p(choose), n, 8, p(outs["pc"]), None)

    for kw in (dict(iters=0), dict(iters=9), dict(gate=2 ** 32 + 1), dict(n=65536), dict(O=46341), dict(H=65536, W=32768),
               dict(stride=HW - 1), dict(stride=1)):
        assert defor(**kw) == -1, kw
    for kw in (dict(n=65536), dict(O=46341), dict(H=65536, W=32768), dict(stride=HW + 1)):
        assert crop(**kw) == -1, kw
    for kw in (dict(n=65536), dict(H=65536, W=32768), dict(stride=HW // 2)):
        assert pcl(**kw) == -1, kw
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, keep[k]), k
    assert defor() == 0 and crop() == 0 and pcl() == 0                           # (and the same calls in range do run)
    torch.cuda.synchronize()
    assert not torch.equal(outs["cm"], keep["cm"]) and (outs["count"] >= 0).all() and (outs["pre"] >= 0).all()
