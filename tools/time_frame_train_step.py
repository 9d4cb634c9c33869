"""A training step from raw frames, the two forms the package offers, timed against each other in ONE process at B = 16 kept
items of M = 20 sent (four spares), N = 1028 points, 480 x 640 uint16 frames and label images from a seed, O = 256:

  (a) ``status_readback``: what was possible before train.FrameTrainStep -- the eager ``pc_sample.train_batch_to_pcl`` on the M
      items, ``status`` read back on the host (a wait), the batch re-indexed there by the first B good items,
      ``GraphedTrainStep.load_batch`` and ``GraphedTrainStep.run()``;
  (b) ``frame_step_nocheck`` / ``frame_step_check``: ``FrameTrainStep.run(check=False)`` (never waits) and ``run(check=True)``
      (one small device->host copy behind the replay).

Both forms are captured first (each on a network of its own: a capture must precede a network's first eager backward), then
timed ALTERNATELY in rounds like tools/time_pool_sampler.py: every round a window of ``--steps`` steps between device events
after a synchronise, wall clock alongside (it holds the host work and the waits); the figures are the median over the rounds
with the min - max spread.  Form (a) is listed twice (``status_readback`` and ``status_readback_again``): the gap between two
runs of the same form is the noise floor the other gaps are read against.  Frames, label images and the per-item tensors are
on the device before the clock starts; every step draws its windows on the host and advances the sampler, as a loader would.
Run on the GPU box:  python tools/time_frame_train_step.py
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
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_frame_train_step.py measures the HIP path; it needs a GPU"
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
    depth, labels, ids, boxes = synthetic_frames(M, args.seed)
    ids = ids.copy()
    ids[[1, 7]] = 99                                             # two of the M items are rejected (ids absent from their images)
    depth_d, labels_d = torch.from_numpy(depth).to(dev), torch.from_numpy(labels).to(dev)
    case = oc.hspose_train_case(M, N, 7)
    items = {k: case[k].to(dev) for k in ITEM_KEYS}

    def make():
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).train()
        return net, TrainDriver(net, total_iters=10 ** 6, check_nan=False)

    # (b) the frame step
    net_b, drv_b = make()
    frames = dict(depth=depth_d, labels=labels_d, inst_ids=ids, bboxes_xyxy=boxes, K=K)
    step = FrameTrainStep(net_b, drv_b.optimizer, frames, items, B, scheduler=drv_b.scheduler,
                          sampler=pc_sample.DeviceSampler(1, dev), n_pts=N, out_size=O)
    # (a) the status read-back around GraphedTrainStep
    net_a, drv_a = make()
    sampler_a = pc_sample.DeviceSampler(1, dev)
    static = {"PC": case["PC"][:B].to(dev), **{k: v[:B].clone() for k, v in items.items()}}
    graphed = GraphedTrainStep(net_a, drv_a.optimizer, static, scheduler=drv_a.scheduler)
    rejected = []

    def status_readback():
        centers, scales = pc_sample.dzi_windows(boxes, H, W)
        PC, status = pc_sample.train_batch_to_pcl(depth_d, labels_d, ids, centers, scales, K, n_pts=N, out_size=O, sampler=sampler_a)
        good = np.flatnonzero(status.cpu().numpy() == 0)          # the wait
        rejected.append(M - len(good))
        if len(good) == 0:
            return
        idx = torch.from_numpy(np.resize(good, B)).to(dev)
        graphed.load_batch({"PC": PC[idx], **{k: v[idx] for k, v in items.items()}})
        graphed.run()

    forms = {"status_readback": status_readback, "frame_step_nocheck": lambda: step.run(check=False),
             "status_readback_again": status_readback, "frame_step_check": lambda: step.run(check=True)}
    res = {"B": B, "M": M, "N": N, "H": H, "W": W, "O": O, "rounds": args.rounds, "steps_per_round": args.steps,
           "forms": alternate(forms, args.rounds, args.steps, args.warmup)}
    torch.cuda.synchronize()
    res["rejected_per_step_readback_form"] = sorted(set(rejected))
    res["frame_step_last_info"] = step.info.cpu().tolist()
    res["frame_step_last_sel"] = step.sel.cpu().tolist()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
