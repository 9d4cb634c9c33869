"""Who makes a step's draws, host or device (config.FLAGS.step_draws), timed against each other in ONE process for the three
captured objects that draw:

  train        ``graph.GraphedTrainStep`` at B = 16, N = 1028: ``run()`` with the host draws (the jitter noise and two
               ``randperm`` on the CPU generator, uploaded through the pinned ring) against ``draws.advance()`` + ``run()`` with
               ``draws=sampler`` (the rows, the six uniforms and the jitter drawn inside the replay);
  frame_train  ``train.FrameTrainStep`` with keep = 16 of 20 items, 480 x 640 uint16 frames (the protocol of
               tools/time_frame_train_step.py), ``run(check=False)``: the host form also draws the 20 DZI windows on numpy's
               generator and uploads their transforms;
  inference    ``graph.GraphedInference`` with 4 instances, N = 1028: the host form draws two ``randperm`` per replay.

Every object is captured first, each on a network of its own, then the forms are timed ALTERNATELY in rounds like
tools/time_pool_sampler.py: every round a window of ``--steps`` steps between device events after a synchronise, wall clock
alongside (it holds the host work); the figures are the median over the rounds with the min - max spread.  Every host form is
listed twice (``*_host`` and ``*_host_again``): it is the code path from before the device draws existed, so it is the
yardstick, and the gap between its two interleaved runs is the noise floor the device form's gap is read against --
``verdict`` says, per object, whether the device form is slower than the host form by more than that gap.
Run on the GPU box:  python tools/time_step_draws.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
import numpy as np
import torch

from time_pool_sampler import alternate
from time_train_frontend import batch as synthetic_frames

ITEM_KEYS = ("obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--sent", type=int, default=20)
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="train,frame_train,inference", help="comma-separated subset of the three objects")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_step_draws.py measures the HIP path; it needs a GPU"
    import ref_cpu as oc
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.graph import GraphedInference, GraphedTrainStep
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.train import FrameTrainStep, TrainDriver

    dev = torch.device("cuda:0")
    B, M, N, O, H, W = args.batch, args.sent, args.points, 256, 480, 640
    K = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)
    FLAGS.reset()
    FLAGS.train = 1
    only = set(args.only.split(","))
    case = oc.hspose_train_case(M, N, 7)
    items = {k: case[k].to(dev) for k in ITEM_KEYS}

    def make():
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).train()
        return net, TrainDriver(net, total_iters=10 ** 6, check_nan=False)

    forms, groups = {}, {}

    def add(name, host, device):
        forms[f"{name}_host"], forms[f"{name}_device"], forms[f"{name}_host_again"] = host, device, host
        groups[name] = (f"{name}_host", f"{name}_device", f"{name}_host_again")

    if "train" in only:
        static = lambda: {"PC": case["PC"][:B].to(dev), **{k: v[:B].clone() for k, v in items.items()}}
        net_h, drv_h = make()
        train_h = GraphedTrainStep(net_h, drv_h.optimizer, static(), scheduler=drv_h.scheduler, draws="host")
        net_d, drv_d = make()
        s_train = pc_sample.DeviceSampler(1, dev)
        train_d = GraphedTrainStep(net_d, drv_d.optimizer, static(), scheduler=drv_d.scheduler, draws=s_train)

        def train_device():
            s_train.advance()
            train_d.run()
        add("train", train_h.run, train_device)

    if "frame_train" in only:
        depth, labels, ids, boxes = synthetic_frames(M, 0)
        ids = ids.copy()
        ids[[1, 7]] = 99                                         # two of the M items are rejected (ids absent from their images)
        frames = dict(depth=torch.from_numpy(depth).to(dev), labels=torch.from_numpy(labels).to(dev), inst_ids=ids,
                      bboxes_xyxy=np.asarray(boxes).astype(np.int64), K=K)
        steps = {}
        for how in ("host", "device"):
            net, drv = make()
            steps[how] = FrameTrainStep(net, drv.optimizer, frames, items, B, scheduler=drv.scheduler,
                                        sampler=pc_sample.DeviceSampler(1, dev), n_pts=N, out_size=O, draws=how)
        add("frame_train", lambda: steps["host"].run(check=False), lambda: steps["device"].run(check=False))

    if "inference" in only:
        FLAGS.train = 0
        n = args.instances
        g = torch.Generator().manual_seed(3)
        PC = (torch.randn(n, N, 3, generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.8])).to(dev)
        obj = torch.randint(0, 6, (n,), generator=g).to(dev)
        mean_shape = (torch.rand(n, 3, generator=g) * 0.2 + 0.1).to(dev)
        sym = torch.zeros(n, 4, device=dev)
        torch.manual_seed(0)
        net_i = HSPose("PoseNet_only").to(dev).eval()
        inf_h = GraphedInference(net_i, PC, obj, mean_shape, sym, draws="host")
        s_inf = pc_sample.DeviceSampler(1, dev)
        inf_d = GraphedInference(net_i, PC, obj, mean_shape, sym, draws=s_inf)
        FLAGS.train = 1

        def inf_device():
            s_inf.advance()
            inf_d.run()
        add("inference", inf_h.run, inf_device)

    timed = alternate(forms, args.rounds, args.steps, args.warmup)
    torch.cuda.synchronize()
    verdict = {}
    for name, (h, d, h2) in groups.items():
        v = {}
        for clock in ("wall_ms", "device_ms"):
            floor = abs(timed[h][clock] - timed[h2][clock])
            gap = timed[d][clock] - min(timed[h][clock], timed[h2][clock])
            v[clock] = {"host": timed[h][clock], "host_again": timed[h2][clock], "device": timed[d][clock],
                        "device_minus_faster_host": round(gap, 4), "host_spread": round(floor, 4),
                        "device_slower_beyond_spread": bool(gap > floor)}
        verdict[name] = v
    res = {"B": B, "M": M, "N": N, "instances": args.instances, "H": H, "W": W, "O": O, "rounds": args.rounds,
           "steps_per_round": args.steps, "forms": timed, "verdict": verdict}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
