"""The farthest-point instance sampler on the GPU (csrc/frontend.hip: hsp_fps_ids_*; ops.fps_ids; pc_sample's 'fps' sampler;
frame.FramePipeline(sampler='fps')) against the numpy restatement of its contract (tests/_fps_ids_ref.py) and, independently,
against ops.fps_levels run on the candidate cloud that ops.frame_to_pcl materialises.  Everything compared is integers or
bits: equality is exact, no tolerance anywhere."""
import numpy as np
import pytest
import torch

import _fps_ids_ref as fr
import test_frame_host as fh
from test_gpu_frame import K_REAL, _depth, _pipeline_frame

pytestmark = pytest.mark.gpu


def _run(dev, depth, mask, centers, scales, O, S, min_pts, K=K_REAL, inst_ids=None):
    """roi_compact -> fps_ids on the device, the model on what roi_compact listed -> everything a test looks at"""
    from hs_pose_amd import ops
    from hs_pose_amd.pc_sample import roi_transform
    depth_d = torch.from_numpy(depth).to(dev)
    xf_d = torch.from_numpy(roi_transform(centers, scales, O)).to(dev)
    ids_d = None if inst_ids is None else torch.tensor(inst_ids, dtype=torch.int32, device=dev)
    src, count = ops.roi_compact(depth_d, torch.from_numpy(mask).to(dev), xf_d, O, ids_d)
    K_d = torch.from_numpy(np.asarray(K, dtype=np.float64).reshape(-1, 9)).to(dev)
    choose, status = ops.fps_ids(depth_d, K_d, src, count, S, min_pts, 2)
    assert choose.shape == (len(scales), S) and choose.dtype == torch.int32 and status.dtype == torch.int32
    src_h, count_h = src.cpu().numpy(), count.cpu().numpy()
    want_choose, want_status = fr.fps_ids(depth, K, src_h, count_h, S, min_pts, 2)
    return dict(depth_d=depth_d, K_d=K_d, src=src, src_h=src_h, count=count_h, choose=choose.cpu().numpy(),
                status=status.cpu().numpy(), want_choose=want_choose, want_status=want_status)


def _check_against_fps_levels(r, j, S):
    """instance j's picks == ops.fps_levels on its candidates, back-projected by ops.frame_to_pcl"""
    from hs_pose_amd import ops
    c = int(r["count"][j, 0])
    g = fr.candidate_entries(c)
    assert len(g) <= fr.CAP and S <= len(g)
    g_d = torch.from_numpy(g.astype(np.int32)).to(r["src"].device)[None]
    cloud = ops.frame_to_pcl(r["depth_d"], r["K_d"][j:j + 1] if r["K_d"].shape[0] > 1 else r["K_d"], r["src"][j:j + 1], g_d)
    assert torch.isfinite(cloud).all()
    sel = ops.fps_levels(cloud, S, 0)[0][0].cpu().numpy()
    assert np.array_equal(g[sel], r["choose"][j]), j


def _branch_frame(dtype, S, O):
    """96 x 128 frame, five instances with disjoint masks: nothing valid; 3 valid (< min_pts = 5); 20 (< S); exactly S; and a
    60-pixel window over a random mask (S < c <= O * O).  Instances 1-3 share a 1:1 window and split its first valid pixels."""
    H, W = 96, 128
    rng = np.random.RandomState(23)
    depth = _depth(rng, H, W, dtype, zeros=0.2)
    centers = np.array([[100.0, 20.0], [64.0, 48.0], [64.0, 48.0], [64.0, 48.0], [50.5, 60.5]])
    scales = np.array([24.0, float(O), float(O), float(O), 60.0])
    full, _ = fh.ref_compact(depth, np.ones((H, W), bool), fh.ref_xf(centers[1], scales[1], O), O)
    mask = np.zeros((5, H, W), np.uint8)
    for j, (lo, hi) in ((1, (0, 3)), (2, (3, 23)), (3, (23, 23 + S))):
        mask[j].reshape(-1)[full[lo:hi]] = 1
    mask[4] = (rng.rand(H, W) < 0.8) & (mask[1:4].sum(0) == 0)
    return depth, mask, centers, scales


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_contract_on_every_branch(dev, dtype):
    S, O = 64, 32
    depth, mask, centers, scales = _branch_frame(dtype, S, O)
    r = _run(dev, depth, mask, centers, scales, O, S, 5)
    c = r["count"][:, 0]
    assert c[0] == 0 and c[1] == 3 and c[2] == 20 and c[3] == S and S < c[4] <= 1024 and (r["count"][:, 1] >= 2).all(), r["count"]
    assert np.array_equal(r["status"], r["want_status"]) and r["status"].tolist() == [1, 1, 0, 0, 0]
    assert np.array_equal(r["choose"], r["want_choose"])
    assert (r["choose"][:2] == -1).all() and np.array_equal(r["choose"][2], np.arange(S) % 20)
    assert np.array_equal(r["choose"][3], np.arange(S))
    assert r["choose"][4, 0] == 0 and len(set(r["choose"][4].tolist())) == S and r["choose"][4].max() < c[4]
    _check_against_fps_levels(r, 4, S)


@pytest.mark.parametrize("S", [64, 1028])
def test_several_points_per_thread_and_the_cap(dev, S):
    """O = 128 over the whole 128 x 128 frame: a half-set mask (1024 < c <= 12288: up to 12 points per lane, some waves with
    none) and a full one (c = 16384 > the cap: thinned)"""
    H = W = O = 128
    rng = np.random.RandomState(31)
    depth = _depth(rng, H, W, "u16", zeros=0.0)
    mask = np.ones((2, H, W), np.uint8)
    mask[0] = rng.rand(H, W) < 0.5
    centers, scales = np.array([[64.0, 64.0], [64.0, 64.0]]), np.array([128.0, 128.0])
    r = _run(dev, depth, mask, centers, scales, O, S, 2)
    c = r["count"][:, 0]
    assert 1024 < c[0] <= fr.CAP and c[1] == O * O > fr.CAP, c
    assert r["status"].tolist() == [0, 0]
    assert np.array_equal(r["choose"], r["want_choose"])
    g1 = set(fr.candidate_entries(int(c[1])).tolist())
    for j in (0, 1):
        assert len(set(r["choose"][j].tolist())) == S and r["choose"][j].min() == 0 and r["choose"][j].max() < c[j]
        _check_against_fps_levels(r, j, S)
    assert set(r["choose"][1].tolist()) <= g1 and max(g1) > fr.CAP             # the thinned row names entries past the cap


def test_up_sampled_crop(dev):
    """a 20-pixel window into O = 64: every source pixel about ten times, S above the number of distinct pixels"""
    H, W, O, S = 96, 128, 64, 512
    rng = np.random.RandomState(37)
    depth = _depth(rng, H, W, "u16", zeros=0.15)
    mask = np.ones((1, H, W), np.uint8)
    r = _run(dev, depth, mask, np.array([[40.0, 50.0]]), np.array([20.0]), O, S, 2)
    c = int(r["count"][0, 0])
    pixels = r["src_h"][0, :c]
    distinct = len(np.unique(pixels))
    assert distinct <= 21 * 21 < S < c and c > 5 * distinct, (distinct, c)
    assert np.array_equal(r["choose"], r["want_choose"]) and r["status"].tolist() == [0]
    picked = pixels[r["choose"][0]]
    assert len(np.unique(picked[:distinct])) == distinct                        # the distinct pixels first,
    assert len(set(r["choose"][0].tolist())) == S                               # then other entries, none twice,
    tail = r["choose"][0, distinct:]
    assert np.array_equal(tail, np.sort(tail))                                  # the lowest unpicked, in order
    _check_against_fps_levels(r, 0, S)


def test_a_camera_per_instance_and_a_label_image(dev):
    S, O = 64, 32
    depth, mask, centers, scales = _branch_frame("u16", S, O)
    one = _run(dev, depth, mask, centers, scales, O, S, 5)
    Ks = np.stack([K_REAL] * 5)
    for j in range(5):
        Ks[j, 0, 0] *= 1.0 + 0.4 * j                                            # another focal length and centre per instance
        Ks[j, 1, 2] += 3.0 * j
    per = _run(dev, depth, mask, centers, scales, O, S, 5, K=Ks)
    assert np.array_equal(per["choose"], per["want_choose"]) and np.array_equal(per["status"], per["want_status"])
    assert not np.array_equal(per["choose"][4], one["choose"][4])               # (instance 4 was ranked under its own K)
    _check_against_fps_levels(per, 4, S)
    labels = np.zeros(depth.shape, np.uint8)
    for j in range(5):
        labels[mask[j] != 0] = j + 3
    lab = _run(dev, depth, labels, centers, scales, O, S, 5, inst_ids=[3, 4, 5, 6, 7])
    assert np.array_equal(lab["count"], one["count"])
    assert np.array_equal(lab["choose"], lab["want_choose"]) and np.array_equal(lab["choose"], one["choose"])
    assert np.array_equal(lab["status"], one["status"])


def _network(dev):
    """an eval-mode HSPose as tests/test_gpu_frame.py builds it, and the two class tables"""
    from hs_pose_amd.HSPose import HSPose
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
    return net, mean_shapes, sym_infos.to(dev)


def _reseed(dev, k):
    from hs_pose_amd import pc_sample
    torch.manual_seed(k)
    np.random.seed(k)
    pc_sample.default_sampler(dev).manual_seed(k)


def test_frame_pipeline_is_a_function_of_the_frame(dev):
    """under FLAGS.pool_sampler = 'fps', FramePipeline(sampler='fps') gives the same bits whatever the generators hold -- eagerly
    and as one replay, which also reproduces a frame after another frame went through the graph --; a rejected frame is None
    with sync, its status without; and the control: under 'device' the same re-seeding changes the rows"""
    from hs_pose_amd import ops, pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.frame import FramePipeline
    FLAGS.reset()
    FLAGS.train = 0
    FLAGS.pool_sampler = "fps"
    try:
        net, mean_shapes, sym_infos = _network(dev)
        frames = []
        for seed in (1, 3):
            depth, masks, bboxes, cls = _pipeline_frame(2, seed)
            frames.append((torch.from_numpy(depth).to(dev), torch.from_numpy(masks).to(dev), bboxes, cls))
        np_before = None
        eager = FramePipeline(net, mean_shapes, sym_infos, sampler="fps")
        _reseed(dev, 11)
        np_before = np.random.get_state()[1].copy()
        torch_before = torch.get_rng_state().clone()
        first = eager(*frames[0], K_REAL)
        assert first is not None and first[0].shape == (2, 4, 4) and first[1].shape == (2, 3) and torch.isfinite(first[0]).all()
        assert np.array_equal(np_before, np.random.get_state()[1]) and torch.equal(torch_before, torch.get_rng_state())
        assert pc_sample.default_sampler(dev).get_state() == (11, 0)            # no generator, no key was touched
        _reseed(dev, 12)
        again = eager(*frames[0], K_REAL)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
        other = eager(*frames[1], K_REAL)
        assert not torch.equal(other[0], first[0])

        replay = FramePipeline(net, mean_shapes, sym_infos, sampler="fps", one_graph=True)
        for k, (frame, want) in enumerate(((frames[0], first), (frames[1], other), (frames[0], first))):
            _reseed(dev, 20 + k)
            got = replay(*frame, K_REAL)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), k
        assert len(replay.frame_graphs) == 1 and not replay.graphs and len(eager.graphs) == 1 and not eager.frame_graphs

        # the flag alone selects the sampler too
        FLAGS.pc_sampler = "fps"
        by_flag = FramePipeline(net, mean_shapes, sym_infos)(*frames[0], K_REAL)
        FLAGS.pc_sampler = "host"
        assert torch.equal(by_flag[0], first[0]) and torch.equal(by_flag[1], first[1])

        # a rejected frame: instance 0 without a mask
        depth_d, masks_d, bboxes, cls = frames[0]
        masks_d = masks_d.clone()
        masks_d[0] = 0
        for pipe in (eager, replay):
            assert pipe(depth_d, masks_d, bboxes, cls, K_REAL) is None
            pipe.sync = False
            out = pipe(depth_d, masks_d, bboxes, cls, K_REAL)
            assert len(out) == 3 and out[2].dtype == torch.int32 and out[2].cpu().tolist() == [1, 0]
            assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()     # (the network ran on the stand-in cloud)
            assert torch.equal(out[0][1], first[0][1])                               # the good instance's pose is its pose
            pipe.sync = True

        # the control: the keyed sampler's rows follow the seed, the farthest-point rows do not
        depth_d, masks_d, bboxes, cls = frames[0]
        centers, scales = pc_sample.roi_windows(bboxes, 480, 640)
        n_pts, O, xf, m8, _, K = pc_sample._frame_args(masks_d, centers, scales, K_REAL, None, None, None)
        src, count = ops.roi_compact(depth_d, m8, torch.from_numpy(xf).to(dev), O)
        K_d = torch.from_numpy(K).to(dev)
        rows = {}
        for how in ("device", "fps"):
            for k in (31, 32):
                _reseed(dev, k)
                sampler = pc_sample.resolve_sampler(how, dev)
                rows[how, k] = pc_sample.choose_rows(sampler, sampler.advance(), depth_d, K_d, src, count, n_pts, 2)[0].cpu()
        assert not torch.equal(rows["device", 31], rows["device", 32])
        assert torch.equal(rows["fps", 31], rows["fps", 32])
        assert (count[:, 0] > n_pts).all()                                           # (both instances were sampled, not tiled)
    finally:
        FLAGS.reset()
