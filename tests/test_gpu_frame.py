"""The frame front end on the GPU (csrc/frontend.hip: hsp_roi_compact_*, hsp_frame_to_pcl_*; pc_sample.frame_to_pcl;
frame.FramePipeline) against the numpy restatement of the crop rule in tests/test_frame_host.py and against the pinned
``pc_sample.depth_to_pcl`` path run on crops built by that restatement.  Everything compared is integers or bits: equality is
exact, no tolerance anywhere."""
import numpy as np
import pytest
import torch

import test_frame_host as fh

pytestmark = pytest.mark.gpu

K_REAL = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)   # REAL275 intrinsics


def _depth(rng, H, W, dtype, zeros=0.25):
    """a frame with holes; the fp32 one also holds fractions below 1 (valid) and negatives (not valid)"""
    d = rng.randint(1, 3000, size=(H, W)).astype(np.float32)
    if dtype == "f32":
        d += rng.rand(H, W).astype(np.float32) - np.float32(0.999)
        d[rng.rand(H, W) < 0.05] = -3.0
    d[rng.rand(H, W) < zeros] = 0
    return d if dtype == "f32" else d.astype(np.uint16)


def _xf_d(centers, scales, O, dev):
    from hs_pose_amd.pc_sample import roi_transform
    xf = roi_transform(centers, scales, O)
    for j in range(len(scales)):
        assert tuple(xf[j].tolist()) == fh.ref_xf(centers[j], scales[j], O)
    return xf, torch.from_numpy(xf).to(dev)


def _check_compaction(src, count, depth, belongs, xf, O):
    src, count = src.cpu().numpy(), count.cpu().numpy()
    assert src.shape == (len(xf), O * O) and count.shape == (len(xf), 2)
    for j in range(len(xf)):
        want, counts = fh.ref_compact(depth, belongs[j], tuple(xf[j].tolist()), O)
        assert count[j].tolist() == counts, (j, count[j], counts)
        assert np.array_equal(src[j, :counts[0]], want), j
    return count


# windows on the 48 x 64 frame: scale < every O and over the left and top edges (duplicated source pixels); scale > every O and
# over all four edges; a non-integer centre and scale (a DZI draw) over the right and bottom edges
SMALL_CENTERS = np.array([[3.0, 5.0], [50.0, 30.0], [55.37, 40.81]])
SMALL_SCALES = np.array([12.0, 120.0, 33.3])


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("mode", ["masks", "labels"])
@pytest.mark.parametrize("O", [16, 64, 96])          # 256 crop pixels: under one chunk; 4096: exactly one; 9216: two and a quarter
def test_compaction_equals_restatement(dev, O, mode, dtype):
    from hs_pose_amd import ops
    H, W, n = 48, 64, 3
    rng = np.random.RandomState(100 + O)
    depth = _depth(rng, H, W, dtype)
    xf, xf_d = _xf_d(SMALL_CENTERS, SMALL_SCALES, O, dev)
    assert SMALL_SCALES[0] < O < SMALL_SCALES[1]
    if mode == "masks":
        mask = (rng.rand(n, H, W) < 0.6).astype(np.uint8) * rng.randint(1, 256, size=(n, H, W)).astype(np.uint8)
        belongs, ids_d = mask != 0, None
    else:
        mask = rng.randint(0, 4, size=(H, W)).astype(np.uint8)
        ids = np.array([2, 0, 3], dtype=np.int32)
        belongs, ids_d = np.stack([mask == i for i in ids]), torch.from_numpy(ids).to(dev)
    src, count = ops.roi_compact(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), xf_d, O, ids_d)
    count = _check_compaction(src, count, depth, belongs, xf, O)
    assert (count[:, 0] > 0).all() and (count[:, 1] > count[:, 0]).all()
    # instance 0 (scale < O) reads source pixels more than once, instance 1's window leaves the frame on every side
    s0 = src[0, :count[0, 0]].cpu().numpy()
    assert len(np.unique(s0)) < len(s0)
    X, Y = fh.ref_map(tuple(xf[1].tolist()), O)
    assert X.min() < 0 and X.max() >= W and Y.min() < 0 and Y.max() >= H


def test_compaction_real_size(dev):
    """480 x 640, O = 256, windows from roi_window: an empty mask (count 0), a window that is valid everywhere (count 65536: src
    fills its row), and two ordinary ones -- 16 chunks per instance"""
    from hs_pose_amd import ops
    from hs_pose_amd.pc_sample import roi_windows
    H, W, O, n = 480, 640, 256, 4
    rng = np.random.RandomState(7)
    depth = _depth(rng, H, W, "u16", zeros=0.3)
    bboxes = np.array([[100, 200, 250, 330], [0, 0, 90, 70], [300, 500, 479, 639], [200, 50, 230, 300]], dtype=np.int32)
    centers, scales = roi_windows(bboxes, H, W)
    mask = (rng.rand(n, H, W) < 0.5).astype(np.uint8)
    mask[1] = 0                                                                 # instance 1: nothing set
    half = int(scales[0]) // 2                                                  # instance 0: its whole window valid
    r0, c0 = int(centers[0, 1]) - half, int(centers[0, 0]) - half
    assert r0 >= 0 and c0 >= 0 and r0 + 2 * half <= H and c0 + 2 * half <= W
    depth[r0:r0 + 2 * half, c0:c0 + 2 * half] = np.maximum(depth[r0:r0 + 2 * half, c0:c0 + 2 * half], 1)
    mask[0] = 1
    xf, xf_d = _xf_d(centers, scales, O, dev)
    src, count = ops.roi_compact(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), xf_d, O)
    count = _check_compaction(src, count, depth, mask != 0, xf, O)
    assert count[0].tolist() == [O * O, O * O] and count[1, 0] == 0 and count[1, 1] > 0
    assert 0 < count[2, 0] < count[2, 1] and 0 < count[3, 0] < count[3, 1]


def _tie_frame(dtype, n_pts, O):
    """96 x 128 frame, three instances: short (fewer than n_pts valid: tiling), long, exactly n_pts (a 1:1 window whose mask
    is cut to its first n_pts valid pixels)"""
    H, W = 96, 128
    rng = np.random.RandomState(11)
    depth = _depth(rng, H, W, dtype, zeros=0.2)
    centers = np.array([[30.0, 40.0], [70.5, 50.5], [64.0, 48.0]])
    scales = np.array([20.0, 90.0, float(O)])
    mask = np.zeros((3, H, W), np.uint8)
    mask[0, 38:41, 26:31] = 1                                                   # 15 frame pixels under a 20 -> 64 zoom
    full, _ = fh.ref_compact(depth, np.ones((H, W), bool), fh.ref_xf(centers[2], scales[2], O), O)
    mask[2].reshape(-1)[full[:n_pts]] = 1
    mask[1] = (rng.rand(H, W) < 0.7) & (mask[0] == 0) & (mask[2] == 0)         # disjoint: one label image can hold all three
    return depth, mask, centers, scales


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_clouds_tie_to_the_pinned_path(dev, dtype):
    """crops built on the CPU by the restatement -> the existing pc_sample.depth_to_pcl; the frame -> frame_to_pcl; same numpy
    seed: the clouds are equal bit for bit and so is the generator afterwards"""
    from hs_pose_amd.pc_sample import depth_to_pcl, frame_to_pcl
    n_pts, O = 256, 64
    depth, mask, centers, scales = _tie_frame(dtype, n_pts, O)
    crops = [fh.ref_crops(depth, mask[j], fh.ref_xf(centers[j], scales[j], O), O) for j in range(3)]
    counts = [fh.ref_compact(depth, mask[j] != 0, fh.ref_xf(centers[j], scales[j], O), O)[1][0] for j in range(3)]
    assert 50 <= counts[0] < n_pts < counts[1] and counts[2] == n_pts, counts
    xymap = torch.from_numpy(np.stack([c[0] for c in crops])).to(dev)
    roi_mask = torch.from_numpy(np.stack([c[1] for c in crops]).astype(np.float32)).reshape(3, 1, O, O).to(dev)
    roi_depth = torch.from_numpy(np.stack([c[2] for c in crops]).astype(np.float32)).reshape(3, 1, O, O).to(dev)
    np.random.seed(5)
    want = depth_to_pcl(roi_depth, K_REAL, xymap, roi_mask, n_pts=n_pts, min_pts=50)
    state_want = np.random.get_state()
    np.random.seed(5)
    got = frame_to_pcl(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), centers, scales, K_REAL, n_pts=n_pts,
                       out_size=O, min_pts=50)
    state_got = np.random.get_state()
    assert got.shape == (3, n_pts, 3) and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert state_got[0] == state_want[0] and np.array_equal(state_got[1], state_want[1]) and state_got[2:] == state_want[2:]
    np.random.seed(5)
    assert not np.array_equal(np.random.get_state()[1], state_got[1])           # (the long instance did draw)
    # a camera per instance, and the label-image form of the same masks, give the same bits
    labels = np.zeros(depth.shape, np.uint8)
    for j in (1, 0, 2):
        labels[mask[j] != 0] = j + 4
    assert all(np.array_equal(labels == j + 4, mask[j] != 0) for j in range(3))
    np.random.seed(5)
    again = frame_to_pcl(torch.from_numpy(depth).to(dev), torch.from_numpy(labels).to(dev), centers, scales,
                         np.stack([K_REAL] * 3), n_pts=n_pts, out_size=O, inst_ids=[4, 5, 6], min_pts=50)
    assert torch.equal(again, want)


def test_rejection_happens_before_any_draw(dev):
    from hs_pose_amd.pc_sample import frame_to_pcl
    H, W, O, n_pts = 96, 128, 64, 64
    depth = np.full((H, W), 700.0, np.float32)
    depth[:, :40] = 0
    depth[10, 10] = 650.0                                                       # the only pixel with depth on the left
    centers = np.array([[90.0, 48.0], [20.0, 20.0]])
    scales = np.array([40.0, 32.0])
    mask = np.zeros((2, H, W), np.uint8)
    mask[0, 40:56, 80:100] = 1                                                  # long: 320 frame pixels, zoomed 1.6 x
    mask[1] = 1

    def run(depth, mask, min_pts):
        np.random.seed(9)
        before = np.random.get_state()[1].copy()
        out = frame_to_pcl(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), centers, scales, K_REAL, n_pts=n_pts,
                           out_size=O, min_pts=min_pts)
        return out, np.array_equal(before, np.random.get_state()[1])

    # instance 1 sees a single pixel with depth, magnified 2 x: 4 crop pixels -- accepted, and the long instance draws
    out, untouched = run(depth, mask, 2)
    assert out is not None and out.shape == (2, n_pts, 3) and not untouched
    # ... a window over no depth but one crop pixel's worth: move it so that the lone pixel maps to exactly one crop pixel
    d1 = depth.copy()
    d1[10, 10] = 0
    d1[4, 4] = 650.0                                                            # the window's first row and column: sampled once
    X, Y = fh.ref_map(fh.ref_xf(centers[1], scales[1], O), O)
    assert (X == 4).sum() * (Y == 4).sum() == 1
    out, untouched = run(d1, mask, 2)                                           # depth-valid count 1 (<= 1)
    assert out is None and untouched
    # mask-and-depth count below min_pts with depth everywhere: 1 pixel for min_pts = 2, 30 for 50
    d2 = np.full((H, W), 700.0, np.float32)
    m2 = mask.copy()
    m2[1] = 0
    m2[1, 4, 4] = 1
    out, untouched = run(d2, m2, 2)
    assert out is None and untouched
    m2[1] = 0
    m2[1, 6, 4:19] = 1                                                          # 15 frame pixels in one row, 2 x wide, 2 rows: 60 > 50
    m3 = m2.copy()
    m3[1, 6, 11:19] = 0                                                         # 7 pixels: 28 crop pixels < 50
    for m, lo in ((m2, 50), (m3, 2)):
        out, untouched = run(d2, m, lo)
        assert out is not None and not untouched
    out, untouched = run(d2, m3, 50)
    assert out is None and untouched


def _pipeline_frame(n, seed):
    H, W = 480, 640
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (800 + 60 * np.sin(xx / 37) + 45 * np.cos(yy / 29)).astype(np.uint16)
    depth[rng.rand(H, W) < 0.1] = 0
    bboxes, masks = [], np.zeros((n, H, W), np.uint8)
    for j in range(n):
        cy, cx, r = rng.randint(80, H - 80), rng.randint(80, W - 80), rng.randint(25, 70)
        masks[j] = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        bboxes.append((cy - r, cx - r, cy + r, cx + r))
    return depth, masks, np.array(bboxes, dtype=np.int32), rng.randint(1, 7, size=n)


def test_frame_pipeline_equals_the_chain_by_hand(dev):
    """FramePipeline == roi_windows -> frame_to_pcl -> network -> generate_RT issued by hand under the same numpy seed and the
    same Pool_layer rows, bit for bit; a graph per instance count; zero rows for no detections"""
    from hs_pose_amd import gcn3d
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.frame import FramePipeline
    from hs_pose_amd.geom_utils import generate_RT
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.pc_sample import frame_to_pcl, roi_windows
    FLAGS.reset()
    FLAGS.train = 0
    try:
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():                       # non-trivial running statistics
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                    m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
        net.eval()
        mean_shapes = (torch.rand(6, 3, generator=g) * 0.2 + 0.1).to(dev)
        sym_infos = torch.zeros(6, 4)
        sym_infos[::2, 0] = 1
        sym_infos = sym_infos.to(dev)
        pipe = FramePipeline(net, mean_shapes, sym_infos)
        torch.manual_seed(21)
        for n, seed in ((2, 1), (3, 2), (2, 3)):                     # a graph for 2, a second one for 3, the first one again
            depth, masks, bboxes, cls = _pipeline_frame(n, seed)
            depth_d, masks_d = torch.from_numpy(depth).to(dev), torch.from_numpy(masks).to(dev)
            np.random.seed(40 + seed)
            got = pipe(depth_d, masks_d, bboxes, cls, K_REAL)
            assert got is not None and got[0].shape == (n, 4, 4) and got[1].shape == (n, 3)
            np.random.seed(40 + seed)
            PC = frame_to_pcl(depth_d, masks_d, *roi_windows(bboxes, 480, 640), K_REAL)
            obj = torch.from_numpy(cls.astype(np.int64) - 1).to(dev)
            with torch.no_grad(), gcn3d.pool_index_feed([p.clone() for p in pipe.graphs[n].pool_idx]):
                out = net(PC=PC, obj_id=obj, mean_shape=mean_shapes[obj], sym=sym_infos[obj])
                RT = generate_RT([out['p_green_R'], out['p_red_R']], [out['f_green_R'], out['f_red_R']], out['Pred_T'],
                                 mode='vec', sym=sym_infos[obj])
            assert torch.isfinite(RT).all()
            assert torch.equal(got[0], RT), (got[0] - RT).abs().max().item()
            assert torch.equal(got[1], out['Pred_s'] + mean_shapes[obj])
        assert sorted(pipe.graphs) == [2, 3]
        RT0, s0 = pipe(depth_d, masks_d[:0], np.zeros((0, 4), np.int32), np.zeros(0, np.int64), K_REAL)
        assert RT0.shape == (0, 4, 4) and s0.shape == (0, 3) and sorted(pipe.graphs) == [2, 3]
        masks_d[0] = 0                                               # an instance without a mask: the frame is rejected
        assert pipe(depth_d, masks_d, bboxes, cls, K_REAL) is None
    finally:
        FLAGS.reset()
