"""Run by test_gpu_step_draws.py in a fresh process (a capture must precede the network's first eager backward):
usage: python tests/_step_draws_check.py mode        (B = 4, N = 256, 96 x 128 frames)

train_f32 / train_bf16: ``GraphedTrainStep(draws=sampler)``.  Building leaves the sampler's state alone; after ``advance()`` and a
  replay the static Pool index buffers and ``output_dict['PC']`` equal the restatement under that (seed, call)
  (tests/_step_draws_ref.py; the cloud through ``hsp_pose_augment`` fed the restated uniforms and jitter); a second replay after
  ``advance()`` differs; ``set_state`` back and replaying gives the first replay's bits; no host generator moves.  Losses,
  gradients and updated parameters against the eager step on a twin network fed the restated rows and noise through
  ``pool_index_feed`` / ``jitter_noise_feed``: fp32 within tests/_train_graph_check.py's bounds, bf16 EQUAL.  The box, rigid and
  jitter augmentations apply to every item and the taper to none (probabilities 1 and -1), so the twin's own six uniforms -- the
  feeds do not carry them -- decide nothing; every probability is covered at kernel level in tests/test_gpu_step_draws.py.
inference: ``GraphedInference(draws=sampler)``: the rows equal the restatement; pred_RT / pred_s against the eager eval forward
  under ``pool_index_feed`` of those rows within tests/test_gpu_graph.py's bounds (1e-5, 1e-6).
frame_train: ``FrameTrainStep(draws='device')``: after ``run()`` xf equals the restatement of the windows, the Pool rows theirs;
  numpy's, torch's CPU and torch's device generator states are unchanged across ``run()``; equal states give equal steps' draws.
frame_pipeline: ``FramePipeline(one_graph=True, draws='device')``: the same three generator states unchanged across
  ``__call__``, the Pool rows equal the restatement under the frame's key, equal states give equal poses.
checkpoint: ``TrainDriver(draws=sampler)``: the checkpoint carries 'draws'; after two steps, a checkpoint, a scrambled sampler
  and ``load_checkpoint`` the next replay draws what the uninterrupted run draws; without a sampler the keys are the reference's.
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _step_draws_ref as dr
from _frame_train_check import ITEM_KEYS, K, O, H, W, frames, items_of, make
from hs_pose_amd import augment, gcn3d, ops
from hs_pose_amd.config import FLAGS
from hs_pose_amd.graph import GraphedInference, GraphedTrainStep
from hs_pose_amd.pc_sample import DeviceSampler
import ref_cpu as oc

B, N = 4, 256
SEED, CALL = 0x9e3779b97f4a7c15, 2 ** 32 + 1
AUG_ORDER = ("PC", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale", "obj_id")


def rng_states():
    return np.random.get_state()[1].copy(), int(np.random.get_state()[2]), torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()


def same_rng(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def sampler_at(dev, call=CALL):
    s = DeviceSampler(SEED, dev)
    s.set_state((SEED, call))
    return s


def train_batch(dev):
    case = oc.hspose_train_case(B, N, 7)
    case["aug_bb"] = 1.0 + oc.hash_tensor((B, 3), 40, 0.2)                       # (the fixture's own are the identity)
    case["aug_rt_t"] = oc.hash_tensor((B, 3), 41, 0.02)
    q, _ = torch.linalg.qr(torch.eye(3) + oc.hash_tensor((B, 3, 3), 42, 0.05))
    case["aug_rt_r"] = (q * torch.sign(torch.linalg.det(q)).view(B, 1, 1)).contiguous()
    return {k: case[k].to(dev) for k in ("PC",) + ITEM_KEYS}


def fed_augment(batch, draws, noise):
    """hsp_pose_augment on the batch with the given uniforms (6,B) and jitter factors (B,N,3) -> the augmented cloud"""
    dev = batch["PC"].device
    args = [batch[k].detach().float().contiguous() for k in AUG_ORDER]
    n, npts, M = args[0].shape[0], args[0].shape[1], batch["model_point"].shape[1]
    d, z = torch.from_numpy(draws).to(dev), torch.from_numpy(noise).to(dev)
    outs = [torch.empty(s, device=dev) for s in ((n, npts, 3), (n, 3, 3), (n, 3), (n, 3))]
    ops._run("hsp_pose_augment", [ops._p(a) for a in args] + [ops._p(d), ops._p(z), n, npts, M, float(FLAGS.aug_bb_pro),
                                                              float(FLAGS.aug_rt_pro), float(FLAGS.aug_bc_pro), float(FLAGS.aug_pc_pro)]
             + [ops._p(o) for o in outs] + [ops._stream()])
    torch.cuda.synchronize()
    return outs[0]


def rows_differ(bad, what, bufs, seed, call, n=N):
    for level, (b, w) in enumerate(zip(bufs, dr.pool_rows(seed, call, n))):
        if not np.array_equal(b.cpu().numpy(), w):
            bad.append(f"{what}: Pool rows of level {level} differ from the restatement under call {call}")


def train(bf16, dev):
    FLAGS.train = 1
    FLAGS.aug_bb_pro = FLAGS.aug_rt_pro = FLAGS.aug_pc_pro = 1.0
    FLAGS.aug_bc_pro = -1.0
    batch = train_batch(dev)
    bad = []
    net_g, drv_g = make(dev, bf16)
    sampler = sampler_at(dev)
    rng0 = rng_states()
    graphed = GraphedTrainStep(net_g, drv_g.optimizer, batch, scheduler=drv_g.scheduler, warmup=2, draws=sampler)
    if sampler.get_state() != (SEED, CALL):
        bad.append(f"building moved the sampler to {sampler.get_state()}")
    if graphed.draws is not sampler or graphed.noise is not None:
        bad.append("the object did not resolve draws= to the sampler")

    def replay(apply=False):
        sampler.advance()
        graphed.run() if apply else graphed.replay()
        torch.cuda.synchronize()
        return [p.clone() for p in graphed.pool_idx], graphed.output_dict["PC"].clone()

    rows_a, pc_a = replay()
    rows_differ(bad, "first replay", rows_a, SEED, CALL)
    draws, noise = dr.augment_draws(SEED, CALL, B, N, FLAGS.aug_pc_r)
    want_pc = fed_augment(batch, draws, noise)
    if not torch.equal(pc_a.view(torch.int32), want_pc.view(torch.int32)):
        bad.append(f"output_dict['PC'] differs from the restatement: {(pc_a - want_pc).abs().max().item():.3e}")
    if torch.equal(pc_a, batch["PC"]):
        bad.append("the augmentation did nothing")
    rows_b, pc_b = replay()
    rows_differ(bad, "second replay", rows_b, SEED, CALL + 1)
    if torch.equal(pc_a, pc_b) or all(torch.equal(a, b) for a, b in zip(rows_a, rows_b)):
        bad.append("a replay after advance() drew the same")
    sampler.set_state((SEED, CALL))
    rows_c, pc_c = replay(apply=True)
    if not (torch.equal(pc_a.view(torch.int32), pc_c.view(torch.int32)) and all(torch.equal(a, c) for a, c in zip(rows_a, rows_c))):
        bad.append("set_state back and replaying did not give the same bits")
    if not same_rng(rng0, rng_states()):
        bad.append("a host generator moved")
    grads_g = {k: p.grad.detach().clone() for k, p in net_g.named_parameters()}
    loss_g = {f"{g}.{k}": float(v.detach()) for g, d in graphed.loss_dict.items() for k, v in d.items()}

    net_e, drv_e = make(dev, bf16)                                                # the eager twin, fed the RESTATED rows and noise
    rows = [torch.from_numpy(r).to(dev) for r in dr.pool_rows(SEED, CALL, N)]
    with gcn3d.pool_index_feed(rows), augment.jitter_noise_feed(torch.from_numpy(noise).to(dev)):
        _, ld = net_e(do_loss=True, **batch)
    total = net_e.total_loss(ld)
    drv_e.optimizer.zero_grad()
    total.backward()
    grads_e = {k: p.grad.detach().clone() for k, p in net_e.named_parameters() if p.grad is not None}
    drv_e.optimizer.clip_grad_norm_(5)
    drv_e.optimizer.step()
    torch.cuda.synchronize()
    worst = dict(loss=0.0, grad=0.0, param=0.0)
    for g, d in ld.items():
        for k, v in d.items():
            a, b = float(v.detach()), loss_g[f"{g}.{k}"]
            worst["loss"] = max(worst["loss"], abs(a - b) / max(1.0, abs(a)))
            if (a != b) if bf16 else (abs(a - b) > 1e-4 * max(1.0, abs(a))):
                bad.append(f"loss {g}.{k}: eager {a!r} graph {b!r}")
    gmax = max(v.abs().max().item() for v in grads_e.values())
    for k, v in grads_e.items():
        err = (v - grads_g[k]).abs().max().item()
        worst["grad"] = max(worst["grad"], err / gmax)
        if (not torch.equal(v, grads_g[k])) if bf16 else (err > 1e-4 * gmax):
            bad.append(f"grad {k}: |diff| {err:.3e} vs max|grad| {gmax:.3e}")
    pe = dict(net_e.named_parameters())
    for k, p in net_g.named_parameters():
        err = (p - pe[k]).abs().max().item()
        worst["param"] = max(worst["param"], err / max(1.0, p.abs().max().item()))
        if (not torch.equal(p, pe[k])) if bf16 else (err > 1e-5 * max(1.0, p.abs().max().item())):
            bad.append(f"param after step {k}: |diff| {err:.3e}")
    print(f"train {'bf16' if bf16 else 'f32'}: total loss eager {float(total.detach()):.6f} graph {float(graphed.total.detach()):.6f}; worst relative "
          f"differences {worst}; {len(bad)} mismatches")
    return bad


def eval_net(dev):
    FLAGS.train = 0
    torch.manual_seed(0)
    from hs_pose_amd.HSPose import HSPose
    net = HSPose("PoseNet_only").to(dev)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():                                                        # non-trivial running statistics
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    net.eval()
    mean_shapes = (torch.rand(6, 3, generator=g) * 0.2 + 0.1).to(dev)
    sym_infos = torch.zeros(6, 4)
    sym_infos[::2, 0] = 1
    return net, mean_shapes, sym_infos.to(dev), g


def inference(dev):
    from hs_pose_amd.geom_utils import generate_RT
    net, mean_shapes, sym_infos, g = eval_net(dev)
    PC = (torch.randn(B, N, 3, generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.8])).to(dev)
    obj = torch.randint(0, 6, (B,), generator=g).to(dev)
    mean_shape, sym = mean_shapes[obj], sym_infos[obj]
    bad = []
    sampler = sampler_at(dev)
    rng0 = rng_states()
    graphed = GraphedInference(net, PC, obj, mean_shape, sym, draws=sampler)
    if sampler.get_state() != (SEED, CALL):
        bad.append(f"building moved the sampler to {sampler.get_state()}")
    sampler.advance()
    RT_g, s_g, out_g = graphed.run()
    torch.cuda.synchronize()
    if not same_rng(rng0, rng_states()):
        bad.append("a host generator moved")
    rows_differ(bad, "replay", graphed.pool_idx, SEED, CALL)
    rows = [torch.from_numpy(r).to(dev) for r in dr.pool_rows(SEED, CALL, N)]
    with torch.no_grad(), gcn3d.pool_index_feed(rows):
        out = net(PC=PC, obj_id=obj, mean_shape=mean_shape, sym=sym)
        RT = generate_RT([out['p_green_R'], out['p_red_R']], [out['f_green_R'], out['f_red_R']], out['Pred_T'], mode='vec', sym=sym)
    errs = {k: (out_g[k] - out[k]).abs().max().item() for k in ('p_green_R', 'p_red_R', 'f_green_R', 'f_red_R', 'Pred_T', 'Pred_s')}
    errs["pred_RT"] = (RT_g - RT).abs().max().item()
    bad += [f"{k}: |diff| {v:.3e}" for k, v in errs.items() if not v <= 1e-5]
    e = (s_g - (out['Pred_s'] + mean_shape)).abs().max().item()
    if not e <= 1e-6:
        bad.append(f"pred_s: |diff| {e:.3e}")
    first = RT_g.clone()
    sampler.advance()
    graphed.run()
    rows_differ(bad, "second replay", graphed.pool_idx, SEED, CALL + 1)
    sampler.set_state((SEED, CALL))
    sampler.advance()
    if not torch.equal(graphed.run()[0], first):
        bad.append("set_state back and replaying did not give the same bits")
    print(f"inference: worst differences {errs}, pred_s {e:.3e}; {len(bad)} mismatches")
    return bad


def frame_train(dev):
    from hs_pose_amd.train import FrameTrainStep
    FLAGS.train = 1                                                              # (the augmentation at its default probabilities)
    M, keep = 6, 4
    fr, items = frames(M, dev), items_of(M, N, dev)
    net, drv = make(dev, False)
    sampler = sampler_at(dev)
    bad = []
    FLAGS.step_draws = "device"                                                  # the flag, read when the object is built
    rng0 = rng_states()
    step = FrameTrainStep(net, drv.optimizer, fr, items, keep, scheduler=drv.scheduler, sampler=sampler, n_pts=N, out_size=O, warmup=2)
    FLAGS.step_draws = "host"
    if step.draws is not sampler or step.graphed.draws is not sampler or sampler.get_state() != (SEED, CALL):
        bad.append(f"draws not resolved to the step's sampler, or the sampler moved: {sampler.get_state()}")
    ok = step.run()
    torch.cuda.synchronize()
    if ok is not True:
        bad.append(f"run() returned {ok!r}")
    if not same_rng(rng0, rng_states()):
        bad.append("a host generator moved across the build and run()")
    dzi = (FLAGS.DZI_PAD_SCALE, FLAGS.DZI_SCALE_RATIO, FLAGS.DZI_SHIFT_RATIO)
    want = dr.dzi_xf(fr["bboxes_xyxy"], SEED, CALL, H, W, O, *dzi)
    got = step.xf.cpu().numpy()
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        bad.append(f"xf differs from the restatement: {np.abs(got - want).max():.3e}")
    rows_differ(bad, "run", step.graphed.pool_idx, SEED, CALL)
    st = step.status.cpu().tolist()
    if st[1] == 0 or any(st[j] for j in (0, 2, 3)):
        bad.append(f"the frames do not make the intended case: status {st}")
    draws, noise = dr.augment_draws(SEED, CALL, keep, N, FLAGS.aug_pc_r)
    sel_batch = {k: (step.batch[k] if k in step.batch else None) for k in AUG_ORDER}
    want_pc = fed_augment(sel_batch, draws, noise)
    pc1 = step.graphed.output_dict["PC"].clone()
    if not torch.equal(pc1.view(torch.int32), want_pc.view(torch.int32)):
        bad.append("the augmented clouds differ from hsp_pose_augment fed the restated draws")
    xf1, sel1 = step.xf.clone(), step.sel.clone()
    rng1 = rng_states()
    step.run()
    torch.cuda.synchronize()
    if not same_rng(rng1, rng_states()):
        bad.append("a host generator moved across run()")
    if torch.equal(xf1, step.xf) or sampler.get_state() != (SEED, CALL + 2):
        bad.append("the second run() drew the same windows, or the sampler did not advance once per run()")
    sampler.set_state((SEED, CALL))
    step.run(check=False)
    torch.cuda.synchronize()
    if not (torch.equal(xf1, step.xf) and torch.equal(sel1, step.sel) and all(np.array_equal(b.cpu().numpy(), w) for b, w in
                                                                                   zip(step.graphed.pool_idx, dr.pool_rows(SEED, CALL, N)))):
        bad.append("equal sampler states did not give equal draws")
    print(f"frame_train: status {st}, xf[0] {got[0].tolist()}; {len(bad)} mismatches")
    return bad


def small_frame(n, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (800 + 25 * np.sin(xx / 9) + 20 * np.cos(yy / 7)).astype(np.uint16)
    depth[rng.rand(H, W) < 0.08] = 0
    bboxes, masks = [], np.zeros((n, H, W), np.uint8)
    for j in range(n):
        cy, cx, r = rng.randint(42, 54), rng.randint(44, 84), rng.randint(20, 28)
        masks[j] = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        bboxes.append((cy - r, cx - r, cy + r, cx + r))
    return depth, masks, np.array(bboxes, dtype=np.int32), rng.randint(1, 7, size=n)


def frame_pipeline(dev):
    from hs_pose_amd.frame import FramePipeline
    net, mean_shapes, sym_infos, _ = eval_net(dev)
    sampler = sampler_at(dev)
    pipe = FramePipeline(net, mean_shapes, sym_infos, n_pts=N, out_size=O, sampler=sampler, one_graph=True, draws="device")
    bad = []
    depth, masks, bboxes, cls = small_frame(3, 1)
    depth_d, masks_d = torch.from_numpy(depth).to(dev), torch.from_numpy(masks).to(dev)
    outs = []
    for k, call in enumerate((CALL, CALL + 1, CALL)):                            # builds the graph, replays it, replays the first key
        sampler.set_state((SEED, call))
        rng0 = rng_states()
        got = pipe(depth_d, masks_d, bboxes, cls, K)
        torch.cuda.synchronize()
        if not same_rng(rng0, rng_states()):
            bad.append(f"a host generator moved across call {k}")
        if got is None:
            bad.append(f"call {k}: the frame was rejected")
            continue
        outs.append(got)
        (fg,) = pipe.frame_graphs.values()
        if fg.graphed.draws is not sampler or sampler.get_state() != (SEED, call + 1):
            bad.append(f"call {k}: the graph's draws are not the pipeline's sampler, or not one advance per frame")
        rows_differ(bad, f"call {k}", fg.graphed.pool_idx, SEED, call)
    if len(outs) == 3:
        if not (torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])):
            bad.append("equal sampler states did not give equal poses")
        if torch.equal(outs[0][0], outs[1][0]):
            bad.append("another key gave the same poses")
    # the eager front end with the network's own graph: the same sampler keys both, one advance per frame
    pipe2 = FramePipeline(net, mean_shapes, sym_infos, n_pts=N, out_size=O, sampler=sampler, draws="device")
    for k, call in enumerate((CALL, CALL + 1)):
        sampler.set_state((SEED, call))
        got = pipe2(depth_d, masks_d, bboxes, cls, K)
        torch.cuda.synchronize()
        (gi,) = pipe2.graphs.values()
        if got is None or sampler.get_state() != (SEED, call + 1):
            bad.append(f"eager front end, call {k}: rejected, or not one advance per frame")
        rows_differ(bad, f"eager front end, call {k}", gi.pool_idx, SEED, call)
        if got is not None and len(outs) == 3 and not torch.equal(got[0], outs[k][0]):
            bad.append(f"eager front end, call {k}: poses differ from the one-graph form's")
    print(f"frame_pipeline: {len(outs)} frames; {len(bad)} mismatches")
    return bad


def checkpoint(dev):
    from hs_pose_amd.train import TrainDriver
    FLAGS.train = 1
    batch = train_batch(dev)
    bad = []
    plain = make(dev, False)[1].checkpoint(1, 0)
    if sorted(plain) != sorted(['seed', 'epoch', 'posenet_state_dict', 'scheduler', 'optimizer']):
        bad.append(f"without a sampler the checkpoint's keys are {sorted(plain)}")
    sampler = sampler_at(dev)
    torch.manual_seed(0)
    from hs_pose_amd.HSPose import HSPose
    net = HSPose("PoseNet_only").to(dev).train()
    drv = TrainDriver(net, total_iters=1000, check_nan=False, draws=sampler)
    graphed = GraphedTrainStep(net, drv.optimizer, batch, scheduler=drv.scheduler, warmup=2, draws=sampler)
    for _ in range(2):
        sampler.advance()
        graphed.run()
    ckpt = copy.deepcopy(drv.checkpoint(1, 0))
    if ckpt.get('draws') != (SEED, CALL + 2):
        bad.append(f"checkpoint['draws'] is {ckpt.get('draws')!r}")
    sampler.advance()
    graphed.replay()                                                             # the uninterrupted run's third step
    torch.cuda.synchronize()
    rows_u, pc_u = [p.clone() for p in graphed.pool_idx], graphed.output_dict["PC"].clone()
    sampler.manual_seed(999)                                                     # "a new process": the sampler starts elsewhere
    epoch = drv.load_checkpoint(ckpt)
    if sampler.get_state() != (SEED, CALL + 2) or epoch != 1:
        bad.append(f"load_checkpoint left the sampler at {sampler.get_state()}, epoch {epoch}")
    sampler.advance()
    graphed.replay()
    torch.cuda.synchronize()
    rows_differ(bad, "resumed replay", graphed.pool_idx, SEED, CALL + 2)
    if not (all(torch.equal(a, b) for a, b in zip(rows_u, graphed.pool_idx)) and torch.equal(pc_u, graphed.output_dict["PC"])):
        bad.append("the resumed replay did not draw what the uninterrupted run drew")
    print(f"checkpoint: draws {ckpt.get('draws')}; {len(bad)} mismatches")
    return bad


def main():
    mode = sys.argv[1]
    dev = torch.device("cuda:0")
    FLAGS.reset()
    run = {"train_f32": lambda: train(False, dev), "train_bf16": lambda: train(True, dev), "inference": lambda: inference(dev),
           "frame_train": lambda: frame_train(dev), "frame_pipeline": lambda: frame_pipeline(dev), "checkpoint": lambda: checkpoint(dev)}
    if mode not in run:
        raise SystemExit(f"unknown mode {mode}")
    bad = run[mode]()
    for line in bad[:20]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
