"""Run by test_gpu_frame_train.py in a fresh process (a capture must precede the network's first eager backward):
usage: python tests/_frame_train_check.py M keep N mode

mode f32 / bf16: ``train.FrameTrainStep.run()`` on one network against its twin on a second network with the same weights: the
  same numpy / sampler / torch seeds replayed in FrameTrainStep's order -- ``dzi_windows``, the eager ``train_batch_to_pcl``
  under a sampler in the same state, the items indexed by the restatement's sel (tests/_batch_select_ref.py), then
  ``GraphedTrainStep(batch).run()``.  Every loss term, every parameter gradient and every parameter after the Ranger step:
  fp32 within tests/_train_graph_check.py's bounds (1e-4 on losses, 1e-4 of the largest gradient, 1e-5 on parameters: the
  float LDS adds of the pooling backward are order-dependent), bf16 EQUAL as in tests/_train_graph_bf16_check.py.
mode rejected: every inst_id absent -- ``run(check=True)`` is False, parameters, optimizer step counts and the scheduler are
  bit-unchanged, info[0] == 0, the network ran on the finite stand-in cloud.
mode calls: ``GraphedTrainStep(prologue=None)`` issues the C-ABI calls recorded from the commit before the prologue existed
  (tests/golden/train_step_calls_B4_N256.json: construction with warmup = 2, then one run), by name and count.
"""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _batch_select_ref as br
from hs_pose_amd import ops
from hs_pose_amd.config import FLAGS
from hs_pose_amd.graph import GraphedTrainStep
from hs_pose_amd.HSPose import HSPose
from hs_pose_amd.train import TrainDriver
import ref_cpu as oc

ITEM_KEYS = ("obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")
H, W, O = 96, 128, 64
K = np.array([[500.0, 0.0, 64.0], [0.0, 500.0, 48.0], [0.0, 0.0, 1.0]])
CALLS_GOLDEN = os.path.join(ROOT, "tests", "golden", "train_step_calls_B4_N256.json")


def make(dev, bf16):
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).train()
    for m in net.modules():                      # dropout draws come from the device generator: not comparable
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    drv = TrainDriver(net, total_iters=1000, check_nan=False)
    if bf16:
        net.set_feature_dtype(torch.bfloat16)
    return net, drv


def frames(M, dev, all_absent=False):
    """M synthetic 96 x 128 uint16 frames at ~0.8 m with holes, a disc per label image; item 1's inst_id is absent from its
    label image (rejected, among the first four), or every item's with ``all_absent``"""
    rng = np.random.RandomState(4)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.empty((M, H, W), np.uint16)
    labels = np.zeros((M, H, W), np.uint8)
    ids, boxes = np.empty(M, np.int32), np.empty((M, 4), np.int64)
    for j in range(M):
        cy, cx, r = rng.randint(40, 56), rng.randint(50, 78), rng.randint(24, 30)
        depth[j] = 800 + 25 * np.sin((xx - cx) / 9.0) + 20 * np.cos((yy - cy) / 7.0) + rng.randint(0, 4, size=(H, W))
        depth[j][rng.rand(H, W) < 0.08] = 0
        ids[j] = 1 + j % 6
        labels[j][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = ids[j]
        boxes[j] = (cx - r, cy - r, cx + r, cy + r)
    ids[1] = 77
    if all_absent:
        ids[:] = 77
    return dict(depth=torch.from_numpy(depth).to(dev), labels=torch.from_numpy(labels).to(dev), inst_ids=ids, bboxes_xyxy=boxes, K=K)


def items_of(M, N, dev):
    case = oc.hspose_train_case(M, N, 7)
    return {k: case[k].to(dev) for k in ITEM_KEYS}


def setup():
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.aug_bb_pro = FLAGS.aug_rt_pro = FLAGS.aug_bc_pro = FLAGS.aug_pc_pro = -1.0   # device-generator draws off


def seed_all(samplers):
    np.random.seed(5)
    torch.manual_seed(3)
    for s in samplers:
        s.manual_seed(21)


def twin(M, keep, N, bf16, dev):
    from hs_pose_amd.pc_sample import DeviceSampler, dzi_windows, train_batch_to_pcl
    from hs_pose_amd.train import FrameTrainStep
    fr, items = frames(M, dev), items_of(M, N, dev)
    net_a, drv_a = make(dev, bf16)
    sa, sb = DeviceSampler(21, dev), DeviceSampler(21, dev)
    step = FrameTrainStep(net_a, drv_a.optimizer, fr, items, keep, scheduler=drv_a.scheduler, sampler=sa, n_pts=N, out_size=O,
                          warmup=2)
    net_b, drv_b = make(dev, bf16)
    case = oc.hspose_train_case(keep, N, 7)
    static = {k: case[k].to(dev) for k in ("PC",) + ITEM_KEYS}
    graphed = GraphedTrainStep(net_b, drv_b.optimizer, static, scheduler=drv_b.scheduler, warmup=2)

    seed_all([sa])
    ok = step.run()
    torch.cuda.synchronize()
    grads_a = {k: p.grad.detach().clone() for k, p in net_a.named_parameters()}
    loss_a = {f"{g}.{k}": float(v.detach()) for g, d in step.loss_dict.items() for k, v in d.items()}

    seed_all([sb])                                               # FrameTrainStep's order: windows, sampler, GraphedTrainStep's draws
    centers, scales = dzi_windows(fr["bboxes_xyxy"], H, W)
    PC, status = train_batch_to_pcl(fr["depth"], fr["labels"], fr["inst_ids"], centers, scales, K, n_pts=N, out_size=O, min_pts=50,
                                    sampler=sb)
    st = status.cpu().numpy()
    sel_ref, info_ref = br.select(st, keep)
    idx = torch.from_numpy(sel_ref.astype(np.int64)).to(dev)
    graphed.load_batch({"PC": PC[idx], **{k: v[idx] for k, v in items.items()}})
    graphed.run()
    torch.cuda.synchronize()
    grads_b = {k: p.grad.detach().clone() for k, p in net_b.named_parameters()}
    loss_b = {f"{g}.{k}": float(v.detach()) for g, d in graphed.loss_dict.items() for k, v in d.items()}

    bad = []
    if ok is not True:
        bad.append(f"run() returned {ok!r}")
    if st[1] == 0 or (st[[0, 2, 3]] != 0).any():
        bad.append(f"the frames do not make the intended case: status {st.tolist()}")
    if step.sel.cpu().tolist() != sel_ref.tolist() or step.info.cpu().tolist() != info_ref.tolist():
        bad.append(f"sel {step.sel.cpu().tolist()} info {step.info.cpu().tolist()}, restatement {sel_ref.tolist()} {info_ref.tolist()}")
    if not torch.equal(step.status, status):
        bad.append("status differs from the eager chain's")
    if not torch.equal(step.batch["PC"].view(torch.int32), PC[idx].view(torch.int32)):
        bad.append("the selected clouds differ from the eager chain's")
    worst = dict(loss=0.0, grad=0.0, param=0.0)
    if set(loss_a) != set(loss_b) or set(grads_a) != set(grads_b):
        bad.append("loss or gradient sets differ")
    finite = all(np.isfinite(v) for v in loss_a.values()) and all(torch.isfinite(v).all().item() for v in grads_a.values())
    if not finite:
        bad.append("non-finite loss or gradient")
    gmax = max(v.abs().max().item() for v in grads_b.values())
    pb = dict(net_b.named_parameters())
    for k, b in loss_b.items():
        a = loss_a[k]
        worst["loss"] = max(worst["loss"], abs(a - b) / max(1.0, abs(b)))
        if (a != b) if bf16 else (abs(a - b) > 1e-4 * max(1.0, abs(b))):
            bad.append(f"loss {k}: frame step {a!r} twin {b!r}")
    for k, v in grads_b.items():
        err = (v - grads_a[k]).abs().max().item()
        worst["grad"] = max(worst["grad"], err / gmax)
        if (not torch.equal(v, grads_a[k])) if bf16 else (err > 1e-4 * gmax):
            bad.append(f"grad {k}: |diff| {err:.3e} vs max|grad| {gmax:.3e}")
    for k, p in net_a.named_parameters():
        err = (p - pb[k]).abs().max().item()
        worst["param"] = max(worst["param"], err / max(1.0, p.abs().max().item()))
        if (not torch.equal(p, pb[k])) if bf16 else (err > 1e-5 * max(1.0, p.abs().max().item())):
            bad.append(f"param after step {k}: |diff| {err:.3e}")
    print(f"{'bf16' if bf16 else 'f32'} M={M} keep={keep} N={N}: status {st.tolist()} sel {sel_ref.tolist()}; total loss frame step "
          f"{float(step.total.detach()):.6f} twin {float(graphed.total.detach()):.6f}; worst relative differences {worst}; {len(bad)} mismatches")
    return bad


def rejected(M, keep, N, dev):
    from hs_pose_amd.pc_sample import DeviceSampler, stand_in_cloud
    from hs_pose_amd.train import FrameTrainStep
    net, drv = make(dev, False)
    step = FrameTrainStep(net, drv.optimizer, frames(M, dev, all_absent=True), items_of(M, N, dev), keep, scheduler=drv.scheduler,
                          sampler=DeviceSampler(21, dev), n_pts=N, out_size=O, warmup=2)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    steps = [int(drv.optimizer.state[p].get("step", 0)) for p in net.parameters() if p in drv.optimizer.state]
    sched = json.dumps(drv.scheduler.state_dict(), default=str, sort_keys=True)
    seed_all([step.sampler])
    ok = step.run(check=True)
    torch.cuda.synchronize()
    bad = []
    if ok is not False:
        bad.append(f"run(check=True) returned {ok!r} on an all-rejected batch")
    if step.info.cpu().tolist() != [0, 0] or step.sel.cpu().tolist() != list(range(keep)) or not bool((step.status != 0).all()):
        bad.append(f"info {step.info.cpu().tolist()} sel {step.sel.cpu().tolist()} status {step.status.cpu().tolist()}")
    for k, p in net.named_parameters():
        if not torch.equal(p, before[k]):
            bad.append(f"param {k} changed")
    if steps != [int(drv.optimizer.state[p].get("step", 0)) for p in net.parameters() if p in drv.optimizer.state]:
        bad.append("the optimizer's step count changed")
    if sched != json.dumps(drv.scheduler.state_dict(), default=str, sort_keys=True):
        bad.append("the scheduler stepped")
    want = stand_in_cloud(N, dev)
    if not all(torch.equal(step.batch["PC"][j], want) for j in range(keep)) or not bool(torch.isfinite(step.batch["PC"]).all()):
        bad.append("the network's clouds are not the stand-in")
    if not bool(torch.isfinite(step.total)) or not all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None):
        bad.append("a non-finite loss or gradient: something non-finite reached the network")
    print(f"rejected M={M} keep={keep} N={N}: run -> {ok}, info {step.info.cpu().tolist()}, total loss {float(step.total.detach()):.6f}; "
          f"{len(bad)} mismatches")
    return bad


def record_calls(cls, B, N, dev, **kw):
    """the C-ABI calls (name -> count) of building ``cls`` with warmup = 2 and of one run, through the recorder of
    tests/test_gpu_launch_diet.py"""
    names, real = [], ops._run

    def run(name, args, **k):
        names.append(name)
        return real(name, args, **k)
    case = oc.hspose_train_case(B, N, 7)
    batch = {k: case[k].to(dev) for k in ("PC",) + ITEM_KEYS}
    net, drv = make(dev, False)
    ops._run = run
    try:
        torch.manual_seed(3)
        graphed = cls(net, drv.optimizer, batch, scheduler=drv.scheduler, warmup=2, **kw)
        built = len(names)
        graphed.run()
        torch.cuda.synchronize()
    finally:
        ops._run = real
    return {"build": dict(collections.Counter(names[:built])), "run": dict(collections.Counter(names[built:]))}


def calls(B, N, dev):
    got = record_calls(GraphedTrainStep, B, N, dev, prologue=None)
    with open(CALLS_GOLDEN) as f:
        want = json.load(f)
    bad = []
    for part in ("build", "run"):
        if got[part] != want[part]:
            diff = {k: (want[part].get(k, 0), got[part].get(k, 0)) for k in set(got[part]) | set(want[part])
                    if want[part].get(k, 0) != got[part].get(k, 0)}
            bad.append(f"{part}: (recorded, now) {diff}")
    print(f"calls B={B} N={N}: build {sum(got['build'].values())} calls of {len(got['build'])} entry points, run {got['run']}; "
          f"{len(bad)} mismatches")
    return bad


def main():
    M, keep, N, mode = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dev = torch.device("cuda:0")
    setup()
    if mode in ("f32", "bf16"):
        bad = twin(M, keep, N, mode == "bf16", dev)
    elif mode == "rejected":
        bad = rejected(M, keep, N, dev)
    elif mode == "calls":
        bad = calls(keep, N, dev)
    else:
        raise SystemExit(f"unknown mode {mode}")
    for line in bad[:20]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
