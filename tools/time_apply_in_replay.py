"""Who applies the training step, the host behind the replay or the replay itself (``apply=`` on ``graph.GraphedTrainStep`` and
``train.FrameTrainStep``), timed against each other in ONE process, on the protocol of
tools/time_step_draws.py, all under device draws:

  train        ``GraphedTrainStep`` at B = 16, N = 1028
  frame_train  ``FrameTrainStep`` with keep = 16 of 20 items, 480 x 640 uint16 frames, two items rejected

  *_host_check    ``apply='host'``, ``run(check_nan=True)`` / ``run(check=True)``: the replay, a device->host copy of the loss's NaN
                  flag (and info) and a wait, then the Ranger launch and ``scheduler.step()`` from the host.  THE YARDSTICK: the safe
                  form as it was before the step could be applied inside the replay.  Listed twice (``*_host_check_again``): the gap
                  between its two interleaved runs is the noise floor.
  *_host_nocheck  ``apply='host'`` without the check: never waits, and trains on whatever the replay computed
  *_graph         ``apply='graph'``: ``sampler.advance()`` and one graph launch; gate, schedule and Ranger launch are in the graph

Every object is captured first, each on a network of its own, then the forms are timed ALTERNATELY in rounds: every round a window
of ``--steps`` steps between device events after a synchronise, wall clock alongside; the figures are the median over the rounds
with the min - max spread.  ``verdict`` says, per object and clock, whether the graph form is slower than the yardstick by more than
the noise floor.  Run on the GPU box:  python tools/time_apply_in_replay.py
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
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="train,frame_train", help="comma-separated subset of the two objects")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_apply_in_replay.py measures the HIP path; it needs a GPU"
    import ref_cpu as oc
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.graph import GraphedTrainStep
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.train import FrameTrainStep, TrainDriver

    dev = torch.device("cuda:0")
    B, M, N, O, H, W = args.batch, args.sent, args.points, 256, 480, 640
    K = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.step_draws = "device"
    only = set(args.only.split(","))
    case = oc.hspose_train_case(M, N, 7)
    items = {k: case[k].to(dev) for k in ITEM_KEYS}
    horizon = args.warmup + args.rounds * args.steps + 8            # the steps the graph form will be asked for, and a few

    def make():
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).train()
        return net, TrainDriver(net, total_iters=10 ** 6, check_nan=False)

    forms, groups = {}, {}

    def add(name, check, nocheck, graph):
        forms[f"{name}_host_check"], forms[f"{name}_host_nocheck"] = check, nocheck
        forms[f"{name}_graph"], forms[f"{name}_host_check_again"] = graph, check
        groups[name] = (f"{name}_host_check", f"{name}_graph", f"{name}_host_check_again")

    if "train" in only:
        static = lambda: {"PC": case["PC"][:B].to(dev), **{k: v[:B].clone() for k, v in items.items()}}

        def train_form(apply, **run_kw):
            net, drv = make()
            sampler = pc_sample.DeviceSampler(1, dev)
            step = GraphedTrainStep(net, drv.optimizer, static(), scheduler=drv.scheduler, draws=sampler, apply=apply,
                                    horizon=horizon if apply == "graph" else None)

            def run():
                sampler.advance()
                step.run(**run_kw)
            return run
        add("train", train_form("host", check_nan=True), train_form("host"), train_form("graph"))

    if "frame_train" in only:
        depth, labels, ids, boxes = synthetic_frames(M, 0)
        ids = ids.copy()
        ids[[1, 7]] = 99                                         # two of the M items are rejected (ids absent from their images)
        frames = dict(depth=torch.from_numpy(depth).to(dev), labels=torch.from_numpy(labels).to(dev), inst_ids=ids,
                      bboxes_xyxy=np.asarray(boxes).astype(np.int64), K=K)

        def frame_form(apply, check):
            net, drv = make()
            step = FrameTrainStep(net, drv.optimizer, frames, items, B, scheduler=drv.scheduler,
                                  sampler=pc_sample.DeviceSampler(1, dev), n_pts=N, out_size=O, draws="device", apply=apply,
                                  horizon=horizon if apply == "graph" else None)
            return lambda: step.run(check=check)
        add("frame_train", frame_form("host", True), frame_form("host", False), frame_form("graph", False))

    timed = alternate(forms, args.rounds, args.steps, args.warmup)
    torch.cuda.synchronize()
    verdict = {}
    for name, (h, g, h2) in groups.items():
        v = {}
        for clock in ("wall_ms", "device_ms"):
            floor = abs(timed[h][clock] - timed[h2][clock])
            gap = timed[g][clock] - min(timed[h][clock], timed[h2][clock])
            v[clock] = {"host_check": timed[h][clock], "host_check_again": timed[h2][clock],
                        "host_nocheck": timed[f"{name}_host_nocheck"][clock], "graph": timed[g][clock],
                        "graph_minus_faster_host_check": round(gap, 4), "host_check_spread": round(floor, 4),
                        "graph_slower_beyond_spread": bool(gap > floor)}
        verdict[name] = v
    res = {"B": B, "M": M, "N": N, "H": H, "W": W, "O": O, "rounds": args.rounds, "steps_per_round": args.steps, "forms": timed,
           "verdict": verdict}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
