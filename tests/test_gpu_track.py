"""The tracked front end on the GPU (csrc/frontend.hip: hsp_pose_windows, hsp_roi_compact_box_*, hsp_track_update;
pc_sample.track_to_pcl_device; frame.FrameTracker) against the numpy reference of tests/_track_ref.py and against the mask-fed
chain (ops.roi_compact, pc_sample.frame_to_pcl_device, graph.GraphedInference) fed that reference's masks and windows.
Everything compared is integers or bits: equality is exact, no tolerance anywhere (floats are compared as their int32 words, so
that the NaN rows of a rejected instance count as equal where they are)."""
import numpy as np
import pytest
import torch

import _track_ref as tr

pytestmark = pytest.mark.gpu


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- windows ----------------------------------------------------------------------------------------------------------------

def test_windows_equal_the_reference(dev):
    from hs_pose_amd import ops
    from hs_pose_amd.pc_sample import roi_transform
    c = tr.windows_case()
    win, n = c["win"], len(c["size"])
    assert win["wstatus"].tolist() == [0, 0, 0, 4, 4, 4, 4, 4]                  # three windows and one instance per cause
    want_xf = np.zeros((n, 3))
    want_xf[:3] = roi_transform(win["centers"][:3], win["scales"][:3], c["O"])
    assert np.array_equal(want_xf, win["xf"])                                  # (the restatement's bits, too)
    for K in (c["K"], np.stack([c["K"]] * n)):                                 # one camera for all, a camera per instance
        boxes, xf, ws = ops.pose_windows(_d(c["RT"], dev), _d(c["size"], dev), _d(K, dev), c["H"], c["W"], c["O"], c["pad"])
        assert boxes.dtype == torch.int32 and xf.dtype == torch.float64 and ws.dtype == torch.int32
        assert ws.cpu().tolist() == win["wstatus"].tolist()
        assert np.array_equal(boxes.cpu().numpy(), win["boxes"])
        assert np.array_equal(xf.cpu().numpy().view(np.int64), want_xf.view(np.int64))


# ---- compaction -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("O,dtype,k_rows", tr.COMPACTION_CASES)
def test_box_compaction_equals_the_reference(dev, O, dtype, k_rows):
    """(the frame bounds a window's scale by W - 1 = 63: the window "larger than O" exists for O = 48, for 64 and 80 the
    largest is the frame-filling one)"""
    from hs_pose_amd import ops
    c = tr.compaction_case(O, dtype, k_rows)
    n, win = 3, c["win"]
    assert win["scales"].min() < O and (O != 48 or win["scales"].max() > O)
    depth_d, RT_d, size_d, K_d = _d(c["depth"], dev), _d(c["RT"], dev), _d(c["size"], dev), _d(c["K"], dev)
    boxes, xf, ws = ops.pose_windows(RT_d, size_d, K_d, 48, 64, O, c["pad"])
    assert np.array_equal(xf.cpu().numpy().view(np.int64), win["xf"].view(np.int64)) and ws.cpu().tolist() == [0, 0, 0]
    src, count = ops.roi_compact_box(depth_d, RT_d, size_d, c["pad"], K_d, xf, O, ws)
    assert src.shape == (n, O * O) and count.shape == (n, 2) and src.dtype == count.dtype == torch.int32
    src_h, count_h = src.cpu().numpy(), count.cpu().numpy()
    for j, (want, counts) in enumerate(c["want"]):
        assert count_h[j].tolist() == counts, (j, count_h[j], counts)
        assert np.array_equal(src_h[j, :counts[0]], want), j
    assert (count_h[:, 0] > 0).all() and (count_h[:, 1] > count_h[:, 0]).all()
    # no flags at all is every flag 0
    src0, count0 = ops.roi_compact_box(depth_d, RT_d, size_d, c["pad"], K_d, xf, O, None)
    assert torch.equal(count0, count) and all(torch.equal(src0[j, :count_h[j, 0]], src[j, :count_h[j, 0]]) for j in range(n))
    # a flagged instance lists nothing; its neighbours are as before
    ws2 = ws.clone()
    ws2[1] = 4
    src2, count2 = ops.roi_compact_box(depth_d, RT_d, size_d, c["pad"], K_d, xf, O, ws2)
    assert count2.cpu().tolist() == [count_h[0].tolist(), [0, 0], count_h[2].tolist()]
    assert all(torch.equal(src2[j, :count_h[j, 0]], src[j, :count_h[j, 0]]) for j in (0, 2))
    # the pinned kernel fed the reference's own inside-mask and the same xf lists the same pixels
    m, _ = tr.masks(c["depth"], c["RT"], c["size"], c["K"], c["pad"], win["wstatus"])
    src3, count3 = ops.roi_compact(depth_d, _d(m, dev), xf, O)
    assert torch.equal(count3, count) and all(torch.equal(src3[j, :count_h[j, 0]], src[j, :count_h[j, 0]]) for j in range(n))


# ---- clouds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["fps", "device"])
def test_clouds_equal_the_mask_fed_chain(dev, how):
    from hs_pose_amd import pc_sample
    c = tr.clouds_case()
    assert 50 <= c["counts"][0] < c["n_pts"] < c["counts"][1] and c["counts"][2] < 50        # tiled, sampled, rejected
    depth_d = _d(c["depth"], dev)
    samplers = ("fps", "fps")
    if how == "device":                                                        # the same (seed, call) state on both sides
        samplers = pc_sample.DeviceSampler(77, dev), pc_sample.DeviceSampler(77, dev)
        for s in samplers:
            s.set_state((77, 5))
    PC, status = pc_sample.track_to_pcl_device(depth_d, _d(c["RT"], dev), _d(c["size"], dev), c["K"], c["n_pts"], c["O"],
                                               c["min_pts"], c["pad"], samplers[0])
    want_PC, want_status = pc_sample.frame_to_pcl_device(depth_d, _d(c["masks"], dev), c["centers"], c["scales"], c["K"],
                                                         c["n_pts"], c["O"], None, c["min_pts"], samplers[1])
    assert status.cpu().tolist() == [0, 0, 1] and torch.equal(status, want_status)
    assert PC.shape == (3, c["n_pts"], 3) and _same_bits(PC, want_PC)
    assert torch.isfinite(PC[:2]).all() and torch.isnan(PC[2]).all()
    if how == "device":
        assert samplers[0].get_state() == samplers[1].get_state() == (77, 6)


# ---- FrameTracker -----------------------------------------------------------------------------------------------------------

H, W, O_TRACK = 96, 128, 64
K_SCENE = tr.small_K(H, W)
SCENE_SEED = 0              # chosen on the GPU among 0 .. 7: both instances keep status 0 over the four frames
CLASSES = [2, 5]


def _scene(n_frames):
    """two slabs of constant depth (1000 and 1200 mm, 40 x 40 pixels) moving a few pixels per frame over a background at 2500 mm"""
    frames = []
    for f in range(n_frames):
        d = np.full((H, W), 2500, np.uint16)
        d[20 + 2 * f:60 + 2 * f, 15 + 3 * f:55 + 3 * f] = 1000
        d[40 - f:80 - f, 70 + 2 * f:110 + 2 * f] = 1200
        frames.append(d)
    return frames


def _seed_poses(seed):
    """poses at the two slabs' centres in frame 0 with random rotations, sizes of 0.2 m"""
    rng = np.random.RandomState(seed)
    RT = []
    for (u, v), z in (((35.0, 40.0), 1.0), ((90.0, 60.0), 1.2)):
        RT.append(tr.pose(tr.rotation(rng), [(u - K_SCENE[0, 2]) * z / K_SCENE[0, 0], (v - K_SCENE[1, 2]) * z / K_SCENE[1, 1], z]))
    return np.stack(RT), np.full((2, 3), 0.2, np.float32)


_net = {}


def _network(dev):
    from test_gpu_fps_ids import _network as make
    if dev not in _net:
        _net[dev] = make(dev)
    return _net[dev]


@pytest.fixture
def fps_flags():
    from hs_pose_amd.config import FLAGS
    FLAGS.reset()
    FLAGS.train = 0
    FLAGS.pool_sampler = "fps"
    yield FLAGS
    FLAGS.reset()


def _tracker(dev, sampler="fps", **kw):
    from hs_pose_amd.frame import FrameTracker
    net, mean_shapes, sym_infos = _network(dev)
    return FrameTracker(net, mean_shapes, sym_infos, out_size=O_TRACK, sampler=sampler, **kw)


class _HostLoop:
    """the loop a caller without the tracker runs: read the state back, make the reference's masks and windows on the host, feed
    the mask-fed chain, run the network's own graph, apply the update rule on the host"""

    def __init__(self, dev, RT, size, pad=tr.PAD):
        self.dev, self.RT, self.size, self.lost, self.pad = dev, RT.copy(), size.copy(), np.zeros(len(size), np.int32), pad
        self.graphed = None

    def step(self, depth):
        from hs_pose_amd import pc_sample
        from hs_pose_amd.graph import GraphedInference
        net, mean_shapes, sym_infos = _network(self.dev)
        m, centers, scales, ws, _ = tr.chain_inputs(depth, self.RT, self.size, K_SCENE, O_TRACK, self.pad)
        PC, status = pc_sample.frame_to_pcl_device(_d(depth, self.dev), _d(m, self.dev), centers, scales, K_SCENE, None, O_TRACK,
                                                   None, 50, "fps")
        status = status | _d(ws, self.dev)
        PC = torch.where((status != 0)[:, None, None], pc_sample.stand_in_cloud(PC.shape[1], self.dev), PC)
        obj = torch.tensor(CLASSES, device=self.dev) - 1
        if self.graphed is None:
            self.graphed = GraphedInference(net, PC, obj, mean_shapes[obj], sym_infos[obj])
        else:
            self.graphed.load(PC=PC)
        pred_RT, pred_s, _ = self.graphed.run()
        status_h = status.cpu().numpy()
        self.RT, self.size, self.lost = tr.update(pred_RT.cpu().numpy(), pred_s.cpu().numpy(), status_h, self.RT, self.size, self.lost)
        return pred_RT, pred_s, status, PC


def test_one_frame_equals_the_mask_fed_chain_and_the_eager_chain(dev, fps_flags):
    from hs_pose_amd import pc_sample
    from hs_pose_amd.geom_utils import generate_RT
    net, mean_shapes, sym_infos = _network(dev)
    depth = _scene(1)[0]
    RT0, size0 = _seed_poses(SCENE_SEED)
    trk = _tracker(dev)
    trk.start(_d(RT0, dev), _d(size0, dev), CLASSES)
    pred_RT, pred_s, status, lost = trk.step(_d(depth, dev), K_SCENE)
    assert pred_RT.shape == (2, 4, 4) and pred_s.shape == (2, 3) and status.dtype == lost.dtype == torch.int32
    assert status.cpu().tolist() == [0, 0] and lost.cpu().tolist() == [0, 0] and torch.isfinite(pred_RT).all()
    # GraphedInference on the clouds of the mask-fed chain
    want_RT, want_s, want_status, _ = _HostLoop(dev, RT0, size0).step(depth)
    assert torch.equal(status, want_status) and _same_bits(pred_RT, want_RT) and _same_bits(pred_s, want_s)
    # the same chain issued eagerly
    PC, st = pc_sample.track_to_pcl_device(_d(depth, dev), _d(RT0, dev), _d(size0, dev), K_SCENE, None, O_TRACK, 50, None, "fps")
    obj = torch.tensor(CLASSES, device=dev) - 1
    with torch.no_grad():
        out = net(PC=PC, obj_id=obj, mean_shape=mean_shapes[obj], sym=sym_infos[obj])
        RT = generate_RT([out['p_green_R'], out['p_red_R']], [out['f_green_R'], out['f_red_R']], out['Pred_T'], mode='vec',
                         sym=sym_infos[obj])
    assert st.cpu().tolist() == [0, 0] and _same_bits(pred_RT, RT) and _same_bits(pred_s, out['Pred_s'] + mean_shapes[obj])
    # the state took the poses
    s_RT, s_size, s_lost = trk.state()
    assert _same_bits(s_RT, pred_RT) and _same_bits(s_size, pred_s) and s_lost.cpu().tolist() == [0, 0]


def test_several_frames_equal_the_host_driven_loop(dev, fps_flags):
    frames = _scene(4)
    RT0, size0 = _seed_poses(SCENE_SEED)
    trk = _tracker(dev)
    trk.start(_d(RT0, dev), _d(size0, dev), CLASSES)
    loop, statuses = _HostLoop(dev, RT0, size0), []
    s_RT, s_size, s_lost = trk.state()
    assert _same_bits(s_RT, _d(RT0, dev)) and _same_bits(s_size, _d(size0, dev)) and s_lost.cpu().tolist() == [0, 0]
    for f, depth in enumerate(frames[1:]):                                     # the start, then three frames
        pred_RT, pred_s, status, lost = trk.step(_d(depth, dev), K_SCENE if f == 0 else None)
        want_RT, want_s, want_status, _ = loop.step(depth)
        print(f"frame {f + 1}: status {status.cpu().tolist()} lost {lost.cpu().tolist()}")
        assert torch.equal(status, want_status), f
        assert _same_bits(pred_RT, want_RT) and _same_bits(pred_s, want_s), f
        s_RT, s_size, s_lost = trk.state()
        assert _same_bits(s_RT, torch.from_numpy(loop.RT)) and _same_bits(s_size, torch.from_numpy(loop.size)), f
        assert s_lost.cpu().tolist() == loop.lost.tolist() == lost.cpu().tolist(), f
        statuses.append(status.cpu().tolist())
    assert len(trk.graphs) == 1
    # the feedback path, not only the lost path: some instance kept status 0 over two consecutive frames
    assert any(statuses[f][j] == 0 and statuses[f + 1][j] == 0 for f in range(2) for j in range(2)), statuses


def test_lost_and_found(dev, fps_flags):
    from hs_pose_amd import pc_sample
    from hs_pose_amd.graph import GraphedInference
    net, mean_shapes, sym_infos = _network(dev)
    frames = _scene(2)
    RT0, size0 = _seed_poses(SCENE_SEED)
    trk = _tracker(dev)
    trk.start(_d(RT0, dev), _d(size0, dev), CLASSES)
    good = trk.step(_d(frames[0], dev), K_SCENE)
    assert good[2].cpu().tolist() == [0, 0]
    before = trk.state()
    # nothing in the frame: every track is lost, the state stays bit for bit, the rows are the stand-in's
    pred_RT, pred_s, status, lost = trk.step(torch.zeros(H, W, dtype=torch.uint16, device=dev))
    assert (status != 0).all() and lost.cpu().tolist() == [1, 1]
    after = trk.state()
    assert _same_bits(after[0], before[0]) and _same_bits(after[1], before[1]) and after[2].cpu().tolist() == [1, 1]
    obj = torch.tensor(CLASSES, device=dev) - 1
    stand_in = pc_sample.stand_in_cloud(int(fps_flags.random_points), dev)
    gi = GraphedInference(net, stand_in[None].repeat(2, 1, 1), obj, mean_shapes[obj], sym_infos[obj])
    want_RT, want_s, _ = gi.run()
    assert _same_bits(pred_RT, want_RT) and _same_bits(pred_s, want_s)
    # the next good frame resumes from the kept state
    loop = _HostLoop(dev, before[0].cpu().numpy(), before[1].cpu().numpy())
    pred_RT, pred_s, status, lost = trk.step(_d(frames[1], dev))
    want_RT, want_s, want_status, _ = loop.step(frames[1])
    assert torch.equal(status, want_status) and _same_bits(pred_RT, want_RT) and _same_bits(pred_s, want_s)
    assert status.cpu().tolist() == [0, 0] and lost.cpu().tolist() == [0, 0] and trk.state()[2].cpu().tolist() == [0, 0]
    # start() with the same n re-seeds the tracks into the same buffers: nothing is captured again
    graphs = dict(trk.graphs)
    trk.start(_d(RT0, dev), _d(size0, dev), CLASSES)
    again = trk.step(_d(frames[0], dev))
    assert trk.graphs == graphs and len(graphs) == 1 and len(trk.tracks) == 1
    assert all(_same_bits(a, b) for a, b in zip(again, good))


def test_two_trackers_from_equal_states_agree(dev, fps_flags):
    """equal tracked states and equal sampler states give equal outputs, frame after frame; another seed draws other rows"""
    from hs_pose_amd import pc_sample
    frames = _scene(3)
    RT0, size0 = _seed_poses(SCENE_SEED)
    outs = []
    for seed in (5, 5, 6):
        trk = _tracker(dev, sampler=pc_sample.DeviceSampler(seed, dev))
        trk.start(_d(RT0, dev), _d(size0, dev), CLASSES)
        outs.append([trk.step(_d(d, dev), K_SCENE) for d in frames])
    for a, b in zip(outs[0], outs[1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))
    assert outs[0][0][2].cpu().tolist() == [0, 0]
    assert not _same_bits(outs[0][0][0], outs[2][0][0])
