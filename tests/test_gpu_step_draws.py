"""The keyed draws of a step on the GPU (csrc/frontend.hip: hsp_pool_rows_draw, hsp_dzi_windows; csrc/losses.hip:
hsp_pose_augment_keyed) against the numpy restatement of include/hsp.h's text (tests/_step_draws_ref.py), bit for bit, and the
captured objects under ``draws=`` (graph.GraphedTrainStep / GraphedInference, train.FrameTrainStep, frame.FramePipeline,
train.TrainDriver's checkpoint entry), each in a fresh child process (tests/_step_draws_check.py) like
tests/test_gpu_frame_train.py: a capture must precede the network's first eager backward."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _step_draws_ref as dr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x9e3779b97f4a7c15                                                        # (high bits set)
CALLS = (0, 2 ** 32 + 5)                                                         # sampler states: call < and >= 2^32


def _sampler(dev, call):
    from hs_pose_amd.pc_sample import DeviceSampler
    s = DeviceSampler(SEED, dev)
    s.set_state((SEED, call))
    return s


@pytest.mark.parametrize("n0", [16, 19, 64, 256, 1024, 257, 1025, 1028])
def test_pool_rows_equal_restatement(dev, n0):
    """16 -> 4 -> 1, sizes that are powers of four (no cycle walk) and sizes just above (walks), one and two levels, a seed with
    high bits set, call below and above 2^32"""
    from hs_pose_amd import ops
    for call in CALLS:
        for levels in (1, 2):
            if levels == 2 and n0 // 16 == 0:
                continue
            s = _sampler(dev, call)
            got = ops.pool_rows_draw(s.advance(), n0, 4, levels)
            want = dr.pool_rows(SEED, call, n0, 4, levels)
            assert len(got) == levels
            for g, w in zip(got, want):
                assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w), (n0, call, levels)
    # the layout of graph.alloc_pool_indices: both levels back to back in the caller's flat buffer
    if n0 >= 16:
        from hs_pose_amd.graph import alloc_pool_indices
        bufs = alloc_pool_indices(n0, dev)
        s = _sampler(dev, 7)
        ops.pool_rows_draw(s.advance(), n0, 4, 2, out=bufs[0]._hsp_flat)
        for b, w in zip(bufs, dr.pool_rows(SEED, 7, n0)):
            assert np.array_equal(b.cpu().numpy(), w)


def _augment_case(B, N, dev, M=32):
    g = torch.Generator().manual_seed(B * 10007 + N)
    r = lambda *shape: torch.rand(*shape, generator=g)
    q, _ = torch.linalg.qr(r(B, 3, 3) - 0.5)
    q2, _ = torch.linalg.qr(torch.eye(3) + 0.05 * (r(B, 3, 3) - 0.5))
    PC = (r(B, N, 3) - 0.5) * 0.1 + torch.tensor([0.0, 0.0, 0.8])
    obj = torch.arange(B).remainder(6).float()                                   # bowls (1) and mugs (5) among them
    sym = torch.zeros(B, 4)
    sym[::2, 0] = 1.0
    case = dict(PC=PC, gt_R=q, gt_t=PC.mean(1) + 0.01 * (r(B, 3) - 0.5), gt_s=0.02 * (r(B, 3) - 0.5), mean_shape=0.12 + 0.03 * r(B, 3),
                sym=sym, aug_bb=0.8 + 0.4 * r(B, 3), aug_rt_t=0.02 * (r(B, 3) - 0.5), aug_rt_r=q2, model_point=r(B, M, 3) - 0.5,
                nocs_scale=0.2 + 0.2 * r(B), obj_ids=obj)
    return {k: v.contiguous().to(dev) for k, v in case.items()}


@pytest.mark.parametrize("B,N,M", [pytest.param(B, N, 32, id=f"{B}-{N}") for N in (8, 256, 1028) for B in (1, 3, 16)] +
                         [pytest.param(3, 257, 1024, id="3-257-M1024")])    # (the loader's model size: four trips of the model loop)
def test_keyed_augmentation_equals_fed_augmentation(dev, flags, B, N, M):
    """hsp_pose_augment_keyed == hsp_pose_augment fed the restated uniforms and jitter factors, every output bit for bit, with
    every probability at 0, at 1 and at its default"""
    from hs_pose_amd import augment, ops
    case = _augment_case(B, N, dev, M)
    order = ("PC", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale", "obj_ids")
    default = (flags.aug_bb_pro, flags.aug_rt_pro, flags.aug_bc_pro, flags.aug_pc_pro)
    settings = [default, (0.0,) * 4, (1.0,) * 4] + [tuple(v if i == q else d for i, d in enumerate(default)) for q in range(4) for v in (0.0, 1.0)]
    for call in CALLS:
        draws, noise = dr.augment_draws(SEED, call, B, N, flags.aug_pc_r)
        draws_d, noise_d = torch.from_numpy(draws).to(dev), torch.from_numpy(noise).to(dev)
        for p_bb, p_rt, p_bc, p_pc in settings:
            s = _sampler(dev, call)
            got = ops.pose_augment_keyed(s.advance(), *[case[k] for k in order], flags.aug_pc_r, p_bb, p_rt, p_bc, p_pc)
            outs = [torch.empty_like(g) for g in got]
            ops._run("hsp_pose_augment", [ops._p(case[k]) for k in order] + [ops._p(draws_d), ops._p(noise_d), B, N, M, p_bb, p_rt,
                                                                             p_bc, p_pc] + [ops._p(o) for o in outs] + [ops._stream()])
            for name, g, w in zip(("PC", "R", "t", "s"), got, outs):
                assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (name, B, N, call, p_bb, p_rt, p_bc, p_pc)
    # the cases are not vacuous: at the defaults some items take each branch and some do not (B = 16), and the jitter moves points
    if B == 16:
        d = dr.augment_draws(SEED, 0, B, N, flags.aug_pc_r)[0]
        for q, p in ((0, default[0]), (1, default[1]), (2, default[2]), (5, default[3])):
            assert 0 < (d[q] < p).sum() < B, (q, d[q])
    # the public forward takes the keyed launch under a draw scope, and a jitter_noise_feed in scope still wins
    from hs_pose_amd import pc_sample
    s = _sampler(dev, 3)
    args = [case[k] for k in order]
    with pc_sample.draw_scope(s, dev) as scope:
        assert scope is not None and s.get_state() == (SEED, 4)
        got = augment.data_augment(*args)
        want = ops.pose_augment_keyed(s.key, *args, flags.aug_pc_r, *default)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        state = torch.cuda.get_rng_state()
        augment.data_augment(*args)
        assert torch.equal(state, torch.cuda.get_rng_state())
        with augment.jitter_noise_feed(torch.zeros(B, N, 3, device=dev)):
            augment.data_augment(*args)
        assert not torch.equal(state, torch.cuda.get_rng_state())                # (the fed form draws its six uniforms as before)


@pytest.mark.parametrize("M", [1, 5, 64])
def test_dzi_windows_equal_restatement(dev, flags, M):
    """boxes that reach the max(H, W) clip, ordinary ones and one-pixel boxes; xf == the header's operation list on the restated
    uniforms, which tests/test_step_draws_host.py holds equal to roi_transform(*dzi_windows(...)) on the host"""
    from hs_pose_amd import ops
    H, W, O = 96, 128, 64
    rng = np.random.RandomState(M)
    x1, y1 = rng.randint(0, W - 2, M), rng.randint(0, H - 2, M)
    boxes = np.stack([x1, y1, x1 + 1 + rng.randint(0, 40, M), y1 + 1 + rng.randint(0, 40, M)], axis=1).astype(np.int32)
    boxes[0] = (0, 0, W, H)                                                       # clipped at max(H, W) whatever the draw
    if M > 1:
        boxes[1] = (60, 40, 61, 41)                                               # one pixel
        boxes[2] = (5, 7, 120, 8)                                                 # one pixel high, wide
    dzi = (flags.DZI_PAD_SCALE, flags.DZI_SCALE_RATIO, flags.DZI_SHIFT_RATIO)
    for call in CALLS:
        s = _sampler(dev, call)
        got = ops.dzi_windows_device(torch.from_numpy(boxes).to(dev), s.advance(), H, W, O, *dzi).cpu().numpy()
        want = dr.dzi_xf(boxes, SEED, call, H, W, O, *dzi)
        assert np.isfinite(want).all() and want[0, 0] == 2.0                      # (scale 128 onto 64 pixels)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (M, call, np.abs(got - want).max())


@pytest.mark.parametrize("N", [256, 1028])
def test_eager_forward_draws_under_the_flag(dev, flags, N):
    """FLAGS.step_draws = 'device': an eager forward advances the module's sampler ONCE and takes both Pool_layers' rows -- in
    one launch with the levels' geometry at N = 1028, layer by layer at N = 256 -- and, in train mode, its augmentation from that
    key; torch's CPU generator does not move; the outputs are those of the forward fed the restated rows"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_cpu as oc
    from hs_pose_amd import gcn3d, ops, pc_sample
    from hs_pose_amd.HSPose import HSPose
    B = 2
    case = {k: v.contiguous().to(dev) for k, v in oc.hspose_train_case(B, N, 7).items()}
    flags.train = 0
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).eval()
    sampler = pc_sample.default_sampler(dev)
    saved = sampler.get_state()
    try:
        sampler.set_state((SEED, 9))
        flags.step_draws = "device"
        rng = torch.get_rng_state()
        with torch.no_grad():
            got = net(PC=case["PC"], obj_id=case["obj_id"], mean_shape=case["mean_shape"], sym=case["sym"])
        assert sampler.get_state() == (SEED, 10) and torch.equal(rng, torch.get_rng_state())
        flags.step_draws = "host"
        rows = [torch.from_numpy(r).to(dev) for r in dr.pool_rows(SEED, 9, N)]
        with torch.no_grad(), gcn3d.pool_index_feed(rows):
            want = net(PC=case["PC"], obj_id=case["obj_id"], mean_shape=case["mean_shape"], sym=case["sym"])
        assert sampler.get_state() == (SEED, 10)
        for k in ("p_green_R", "p_red_R", "f_green_R", "f_red_R", "Pred_T", "Pred_s"):
            assert torch.equal(got[k], want[k]), k
        with torch.no_grad(), gcn3d.pool_index_feed([torch.from_numpy(r).to(dev) for r in dr.pool_rows(SEED, 10, N)]):
            other = net(PC=case["PC"], obj_id=case["obj_id"], mean_shape=case["mean_shape"], sym=case["sym"])
        assert not torch.equal(other["Pred_T"], want["Pred_T"])                  # (the rows matter)
        # train mode: the augmentation under the same key as the rows, one advance for both
        flags.train = 1
        flags.step_draws = "device"
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).train()                             # (the train-mode module set)
        keys = ("PC", "obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")
        state, rng = torch.cuda.get_rng_state(), torch.get_rng_state()           # (after the new network's own initialisation draws)
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        with torch.no_grad():
            out = net(**{k: case[k] for k in keys})
        assert sampler.get_state() == (SEED, 11) and torch.equal(state, torch.cuda.get_rng_state()) and torch.equal(rng, torch.get_rng_state())
        draws, noise = dr.augment_draws(SEED, 10, B, N, flags.aug_pc_r)
        order = ("PC", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale", "obj_id")
        outs = [torch.empty(s_, device=dev) for s_ in ((B, N, 3), (B, 3, 3), (B, 3), (B, 3))]
        d, z = torch.from_numpy(draws).to(dev), torch.from_numpy(noise).to(dev)
        ops._run("hsp_pose_augment", [ops._p(case[k]) for k in order] + [ops._p(d), ops._p(z), B, N, 32, flags.aug_bb_pro, flags.aug_rt_pro,
                                                                         flags.aug_bc_pro, flags.aug_pc_pro] + [ops._p(o) for o in outs] + [ops._stream()])
        assert torch.equal(out["PC"], outs[0]) and torch.equal(out["gt_R"], outs[1]) and torch.equal(out["gt_s"], outs[3])
    finally:
        sampler.set_state(saved)


def test_wrappers_refuse_bad_arguments(dev):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError
    key = torch.zeros(2, dtype=torch.int64, device=dev)
    boxes = torch.zeros(3, 4, dtype=torch.int32, device=dev)
    for bad in (lambda: ops.pool_rows_draw(key, 3), lambda: ops.pool_rows_draw(key, 15, 4, 2), lambda: ops.pool_rows_draw(key[:1], 64),
                lambda: ops.pool_rows_draw(key.cpu(), 64), lambda: ops.pool_rows_draw(key, 64, 4, 3),
                lambda: ops.pool_rows_draw(key, 64, out=torch.zeros(19, dtype=torch.int32, device=dev)),
                lambda: ops.dzi_windows_device(boxes.long(), key, 96, 128, 64, 1.5, 0.25, 0.25),
                lambda: ops.dzi_windows_device(boxes[:, :3], key, 96, 128, 64, 1.5, 0.25, 0.25),
                lambda: ops.dzi_windows_device(boxes, key, 96, 128, 64, 1.5, 1.0, 0.25),
                lambda: ops.dzi_windows_device(boxes, key, 96, 128, 64, 1.5, 0.25, 0.25, out=torch.zeros(3, 3, device=dev))):
        with pytest.raises(HspError):
            bad()


@pytest.mark.parametrize("mode", ["train_f32", "train_bf16", "inference", "frame_train", "frame_pipeline", "checkpoint"])
def test_captured_objects_under_device_draws(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_step_draws_check.py"), mode], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
