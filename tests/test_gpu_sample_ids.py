"""The device sampler on the GPU (csrc/frontend.hip: hsp_sample_ids; pc_sample.DeviceSampler, frame_to_pcl_device, the
``sampler=`` argument of the front ends; frame.FramePipeline's device and one-graph forms) against the numpy restatement of
include/hsp.h's text (tests/_sample_ids_ref.py).  Everything compared is integers or bits: equality is exact, no tolerance."""
import numpy as np
import pytest
import torch

import _sample_ids_ref as sr
import test_frame_host as fh
from conftest import golden
from test_gpu_frame import K_REAL, SMALL_CENTERS, SMALL_SCALES, _depth, _pipeline_frame

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 3, 15, 16, 17, 255, 256, 257, 1027, 1028, 1029, 4096, 4097, 65536, 307200]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _key_of(sampler):
    """(seed, call) of the launch that follows the next advance()"""
    return sampler.get_state()


@pytest.mark.parametrize("S", [1, 7, 256, 257, 1028])
def test_sample_ids_equals_restatement(dev, S):
    """every count x both strides (second counts 0, 1, 2) x both short modes x min_pts {1, 2, 50} x min_depth_pts {0, 2}: one
    launch per combination over mixed rows (rejected, tiled, identity, with replacement, permuted), bit for bit"""
    from hs_pose_amd import ops
    from hs_pose_amd.pc_sample import DeviceSampler
    single = np.array(COUNTS, dtype=np.int32)
    pairs = np.array([[c, d] for c in COUNTS for d in (0, 1, 2)], dtype=np.int32)
    sampler = DeviceSampler(0x9e3779b97f4a7c15 + S, dev)
    for counts in (single, pairs):
        counts_d = torch.from_numpy(counts).to(dev)
        for short_mode in (0, 1):
            for min_pts in (1, 2, 50):
                for min_depth_pts in ((0, 2) if counts.ndim == 2 else (0,)):
                    seed, call = _key_of(sampler)
                    choose, status = ops.sample_ids(counts_d, S, sampler.advance(), min_pts, min_depth_pts, short_mode)
                    want, want_status = sr.sample_ids(counts, S, seed, call, min_pts, min_depth_pts, short_mode)
                    what = (counts.ndim, short_mode, min_pts, min_depth_pts)
                    assert choose.shape == (len(counts), S) and choose.dtype == torch.int32 and status.dtype == torch.int32
                    assert np.array_equal(status.cpu().numpy(), want_status), what
                    got = choose.cpu().numpy()
                    rows = np.nonzero((got != want).any(axis=1))[0]
                    assert rows.size == 0, (what, [(int(r), counts[r].tolist()) for r in rows[:5]])
    # the next call differs on every permuted row (S >= 7: a one-row prefix of two orders may well coincide); a restored state
    # repeats the call
    state = sampler.get_state()
    counts_d = torch.from_numpy(single).to(dev)
    a, _ = ops.sample_ids(counts_d, S, sampler.advance(), 2, 0, 1)
    b, _ = ops.sample_ids(counts_d, S, sampler.advance(), 2, 0, 1)
    sampler.set_state(state)
    a2, _ = ops.sample_ids(counts_d, S, sampler.advance(), 2, 0, 1)
    assert torch.equal(a, a2)
    if S >= 7:
        for j, c in enumerate(COUNTS):
            if c >= S:
                assert not torch.equal(a[j], b[j]), c


def _small_frame(O, mode, dtype):
    """tests/test_gpu_frame.py's 48 x 64 frame and windows plus a fourth instance nothing belongs to"""
    H, W = 48, 64
    rng = np.random.RandomState(100 + O)
    depth = _depth(rng, H, W, dtype)
    centers = np.concatenate([SMALL_CENTERS, [[20.0, 20.0]]])
    scales = np.concatenate([SMALL_SCALES, [30.0]])
    if mode == "masks":
        mask = (rng.rand(4, H, W) < 0.6).astype(np.uint8) * rng.randint(1, 256, size=(4, H, W)).astype(np.uint8)
        mask[3] = 0
        belongs, ids = mask != 0, None
    else:
        mask = rng.randint(0, 4, size=(H, W)).astype(np.uint8)
        ids = np.array([2, 0, 3, 9], dtype=np.int32)
        belongs = np.stack([mask == i for i in ids])
    counts = [fh.ref_compact(depth, belongs[j], fh.ref_xf(centers[j], scales[j], O), O)[1] for j in range(4)]
    return depth, mask, ids, centers, scales, np.array(counts)


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("mode", ["masks", "labels"])
@pytest.mark.parametrize("O", [16, 64, 96])
def test_frame_to_pcl_device_equals_the_kernels_fed_the_restatement(dev, O, mode, dtype):
    from hs_pose_amd import ops
    from hs_pose_amd.pc_sample import DeviceSampler, frame_to_pcl, frame_to_pcl_device, roi_transform
    depth, mask, ids, centers, scales, counts = _small_frame(O, mode, dtype)
    assert counts[3, 0] == 0 and counts[3, 1] > 1 and len(set(counts[:3, 0].tolist())) == 3 and counts[:3, 0].min() >= 2
    n_pts = int(np.sort(counts[:3, 0])[1])                       # one instance short of it, one exactly at it, one long
    depth_d, mask_d = torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev)
    sampler = DeviceSampler(77 + O, dev)
    sampler.advance()                                            # (not the first call of its seed)

    def by_hand(keep, seed, call):
        xf_d = torch.from_numpy(roi_transform(centers[keep], scales[keep], O)).to(dev)
        ids_d = None if ids is None else torch.from_numpy(ids[keep]).to(dev)
        src, count = ops.roi_compact(depth_d, mask_d[keep] if mode == "masks" else mask_d, xf_d, O, ids_d)
        assert np.array_equal(count.cpu().numpy(), counts[keep])
        choose, status = sr.sample_ids(counts[keep], n_pts, seed, call, 2, 2, 0)
        K_d = torch.from_numpy(K_REAL).reshape(1, 9).to(dev)
        return ops.frame_to_pcl(depth_d, K_d, src, torch.from_numpy(choose).to(dev)), status

    for keep in (np.arange(4), np.arange(3)):
        args = (depth_d, mask_d[keep] if mode == "masks" else mask_d, centers[keep], scales[keep], K_REAL)
        kw = dict(n_pts=n_pts, out_size=O, inst_ids=None if ids is None else ids[keep])
        seed, call = state = _key_of(sampler)
        before = np.random.get_state()
        PC, status = frame_to_pcl_device(*args, sampler=sampler, **kw)
        after = np.random.get_state()
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
        want, want_status = by_hand(keep, seed, call)
        assert PC.shape == (len(keep), n_pts, 3) and PC.dtype == torch.float32 and PC.is_cuda and status.is_cuda
        assert np.array_equal(status.cpu().numpy(), want_status)
        assert torch.equal(_bits(PC), _bits(want))
        assert torch.isfinite(PC[:3]).all()
        # the wrapped form under the same state: the clouds, or None for the frame with the rejected instance
        sampler.set_state(state)
        wrapped = frame_to_pcl(*args, sampler=sampler, **kw)
        if len(keep) == 4:
            assert want_status.tolist() == [0, 0, 0, 1] and torch.isnan(PC[3]).all() and wrapped is None
        else:
            assert torch.equal(wrapped, PC)
    assert frame_to_pcl_device(depth_d, mask_d[:0], centers[:0], scales[:0], K_REAL, n_pts=n_pts, out_size=O,
                               sampler=sampler)[0].shape == (0, n_pts, 3)


def test_frame_rejection_status_bits(dev):
    """tests/test_gpu_frame.py::test_rejection_happens_before_any_draw's frames: bit 1 for <= 1 crop pixels with depth, bit 0 for
    fewer than min_pts with depth and mask; the flags follow FLAGS.pc_sampler when no sampler is named"""
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.pc_sample import DeviceSampler, frame_to_pcl, frame_to_pcl_device
    H, W, O, n_pts = 96, 128, 64, 64
    depth = np.full((H, W), 700.0, np.float32)
    depth[:, :40] = 0
    depth[4, 4] = 650.0                                          # the one pixel with depth on the left, sampled once
    centers, scales = np.array([[90.0, 48.0], [20.0, 20.0]]), np.array([40.0, 32.0])
    mask = np.zeros((2, H, W), np.uint8)
    mask[0, 40:56, 80:100] = 1
    mask[1] = 1
    sampler = DeviceSampler(3, dev)

    def run(depth, mask, min_pts):
        PC, status = frame_to_pcl_device(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), centers, scales,
                                         K_REAL, n_pts=n_pts, out_size=O, min_pts=min_pts, sampler=sampler)
        assert torch.isfinite(PC[0]).all() and torch.isnan(PC[1]).all() == bool(status[1] != 0)
        return status.cpu().tolist()

    assert run(depth, mask, 2) == [0, 3]                         # one pixel with depth: both tests fail
    d2 = np.full((H, W), 700.0, np.float32)
    m2 = mask.copy()
    m2[1] = 0
    m2[1, 6, 4:11] = 1                                           # 7 frame pixels, 28 crop pixels
    assert run(d2, m2, 50) == [0, 1] and run(d2, m2, 2) == [0, 0]
    FLAGS.reset()
    try:
        before = np.random.get_state()[1].copy()
        FLAGS.pc_sampler = "device"
        args = (torch.from_numpy(d2).to(dev), torch.from_numpy(m2).to(dev), centers, scales, K_REAL)
        out = frame_to_pcl(*args, n_pts=n_pts, out_size=O)
        assert out is not None and out.shape == (2, n_pts, 3) and np.array_equal(before, np.random.get_state()[1])
        assert frame_to_pcl(*args, n_pts=n_pts, out_size=O, min_pts=50) is None
        out = frame_to_pcl(*args, n_pts=n_pts, out_size=O, sampler="host")
        assert out is not None and not np.array_equal(before, np.random.get_state()[1])
    finally:
        FLAGS.reset()


def test_depth_to_pcl_and_pc_sample_with_a_device_sampler(dev, ref, flags):
    """the two crop-side front ends == their gather kernels fed the restatement's rows (short_mode 0 / 1), at the shapes of
    tests/test_gpu_frontend.py; rejection keeps each function's return contract; numpy's generator is left alone"""
    from hs_pose_amd import ops
    from hs_pose_amd.pc_sample import DeviceSampler, PC_sample, depth_to_pcl
    g = golden("frontend_pc_sample")
    mask, depth, camK, coor = ref.frontend_inputs(3, 64, 80, 900, [float(r) for r in g["radii"]])
    K64 = golden("frontend_depth_to_pcl")["K"]
    counts = np.array([int(c) for c in g["counts"]])
    assert len(set(counts.tolist())) == 3 and counts.min() >= 50
    S = int(np.sort(counts)[1])                                  # one image short of it, one exactly at it, one long
    flags.random_points = S
    mask_d, depth_d, camK_d, coor_d = (t.to(dev) for t in (mask, depth, camK, coor))
    HW = 64 * 80
    pix, count = ops.pc_compact(mask_d.reshape(3, HW), depth_d.reshape(3, HW))
    assert np.array_equal(count.cpu().numpy(), counts)
    sampler = DeviceSampler(2024, dev)
    before = np.random.get_state()[1].copy()

    seed, call = _key_of(sampler)
    got = PC_sample(mask_d, depth_d, camK_d, coor_d, sampler=sampler)
    choose, status = sr.sample_ids(counts, S, seed, call, 2, 0, 1)
    assert status.tolist() == [0, 0, 0] and sorted(choose[int(np.argsort(counts)[1])].tolist()) == list(range(S))
    want = ops.pc_gather(depth_d.reshape(3, HW), coor_d.reshape(3, 2, HW), camK_d, pix, torch.from_numpy(choose).to(dev))
    assert got.shape == (3, S, 3) and torch.equal(_bits(got), _bits(want))

    seed, call = _key_of(sampler)
    got = depth_to_pcl(depth_d, K64, coor_d, mask_d, n_pts=S, sampler=sampler)
    choose, status = sr.sample_ids(counts, S, seed, call, 50, 0, 0)
    assert status.tolist() == [0, 0, 0] and np.array_equal(choose[int(np.argsort(counts)[1])], np.arange(S))
    K_d = torch.from_numpy(np.asarray(K64, dtype=np.float64)).reshape(1, 9).expand(3, 9).contiguous().to(dev)
    want = ops.depth_to_pcl(depth_d.reshape(3, HW), coor_d.reshape(3, 2, HW), K_d, pix, torch.from_numpy(choose).to(dev))
    assert got.shape == (3, S, 3) and torch.equal(_bits(got), _bits(want))

    few = mask.clone()
    few[1] = 0                                                   # nothing valid: the compaction leaves this row undefined
    assert depth_to_pcl(depth_d, K64, coor_d, few.to(dev), n_pts=S, sampler=sampler) is None
    assert PC_sample(few.to(dev), depth_d, camK_d, coor_d, sampler=sampler) == (None, None)
    few[1, 0, 3, 4] = 1.0
    depth1 = depth.clone()
    depth1[1, 0, 3, 4] = 700.0                                   # one valid pixel: <= 1 rejects
    assert PC_sample(few.to(dev), depth1.to(dev), camK_d, coor_d, sampler=sampler) == (None, None)
    flags.pc_sampler = "device"
    assert PC_sample(mask_d, depth_d, camK_d, coor_d).shape == (3, S, 3)
    assert np.array_equal(before, np.random.get_state()[1])


@pytest.mark.parametrize("form", ["eager", "one_graph"])
def test_frame_pipeline_with_a_device_sampler_equals_the_chain_by_hand(dev, form):
    """FramePipeline(sampler=DeviceSampler) == frame_to_pcl_device under an equal-state sampler -> GraphedInference on the same
    Pool_layer rows, bit for bit: two instance counts and none, a second frame through an already captured graph (the replay
    reads the new frame and the new key), a rejected frame, and the unsynchronised form's three device tensors"""
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.frame import FramePipeline
    from hs_pose_amd.graph import GraphedInference
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.pc_sample import DeviceSampler, frame_to_pcl_device, roi_windows
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
        sampler, hand = DeviceSampler(5, dev), DeviceSampler(0, dev)
        pipe = FramePipeline(net, mean_shapes, sym_infos, sampler=sampler, one_graph=form == "one_graph")
        by_hand = {}
        torch.manual_seed(21)
        before = np.random.get_state()[1].copy()
        seen = []
        for n, seed in ((2, 1), (3, 2), (2, 3)):                     # a graph for 2, a second one for 3, the first one again
            depth, masks, bboxes, cls = _pipeline_frame(n, seed)
            depth_d, masks_d = torch.from_numpy(depth).to(dev), torch.from_numpy(masks).to(dev)
            hand.set_state(sampler.get_state())
            got = pipe(depth_d, masks_d, bboxes, cls, K_REAL)
            assert got is not None and got[0].shape == (n, 4, 4) and got[1].shape == (n, 3)
            assert sampler.get_state()[1] == len(seen) + 1           # one key per frame
            graphs = pipe.graphs if form == "eager" else {k[1]: fg.graphed for k, fg in pipe.frame_graphs.items()}
            PC, status = frame_to_pcl_device(depth_d, masks_d, *roi_windows(bboxes, 480, 640), K_REAL, sampler=hand)
            assert status.cpu().tolist() == [0] * n and hand.get_state() == sampler.get_state()
            obj = torch.from_numpy(cls.astype(np.int64) - 1).to(dev)
            gi = by_hand.get(n)
            if gi is None:
                rng = torch.get_rng_state()
                gi = by_hand[n] = GraphedInference(net, PC, obj, mean_shapes[obj], sym_infos[obj])
                torch.set_rng_state(rng)                             # (its warm-up draw is not the pipeline's)
            else:
                gi.load(PC, obj, mean_shapes[obj], sym_infos[obj])
            for mine, theirs in zip(gi.pool_idx, graphs[n].pool_idx):
                mine.copy_(theirs)                                   # the Pool_layer rows of the pipeline's replay
            gi.graph.replay()
            assert torch.isfinite(gi.pred_RT).all()
            assert torch.equal(got[0], gi.pred_RT), (got[0] - gi.pred_RT).abs().max().item()
            assert torch.equal(got[1], gi.pred_s)
            seen.append(got[0])
        assert not torch.equal(seen[0], seen[2])                     # the second frame of the 2-instance graph is another frame
        assert sorted(graphs) == [2, 3] and len(pipe.graphs) + len(pipe.frame_graphs) == 2
        assert np.array_equal(before, np.random.get_state()[1])
        # the same frame again: a new key, other rows, other poses
        again = pipe(depth_d, masks_d, bboxes, cls, K_REAL)
        assert again is not None and not torch.equal(again[0], seen[2])
        RT0, s0 = pipe(depth_d, masks_d[:0], np.zeros((0, 4), np.int32), np.zeros(0, np.int64), K_REAL)
        assert RT0.shape == (0, 4, 4) and s0.shape == (0, 3) and len(pipe.graphs) + len(pipe.frame_graphs) == 2
        pipe.sync = False
        out = pipe(depth_d, masks_d, bboxes, cls, K_REAL)
        assert len(out) == 3 and all(t.is_cuda for t in out) and out[0].shape == (2, 4, 4) and out[1].shape == (2, 3)
        assert out[2].dtype == torch.int32 and out[2].cpu().tolist() == [0, 0]
        masks_d[0] = 0                                               # an instance without a mask: the frame is rejected
        out = pipe(depth_d, masks_d, bboxes, cls, K_REAL)
        assert out[2].cpu().tolist() == [1, 0] and torch.isfinite(out[0]).all()
        pipe.sync = True
        assert pipe(depth_d, masks_d, bboxes, cls, K_REAL) is None
    finally:
        FLAGS.reset()
