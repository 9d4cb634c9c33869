"""The tracked frame (frame.FrameTracker: windows from the last pose, box compaction, rows, clouds, network, generate_RT, state
update, ONE replay) timed on the device beside its yardstick, the ``one_graph`` ``frame.FramePipeline`` replay fed masks and
boxes, in the protocol of tools/time_frame_frontend.py: 480 x 640 uint16 frame, O = 256, 1028 points, n = 1 and 4 instances,
the 'device' and the 'fps' sampler, a network with random weights.  Both graphs are warmed, then timed ALTERNATELY in rounds: a
window of ``--steps`` (20) bare replays between device events after a synchronise; the figures are the median over the rounds
with the min - max spread, in microseconds per replay.  What is timed is the captured graph alone (no upload, no host work).

The scene is the discs of time_frame_frontend.py; a track starts at its disc's centre, at the disc's depth, with the disc's
diameter as its size, so the padded box (``FLAGS.DZI_PAD_SCALE``) cuts a window like the detector's.  The network's weights
are random, so the tracked state wanders from replay to replay: every window starts from a fresh ``start()`` and the result
says how many tracks were still held at the end of the last one (``held``); a lost track's replay costs what a held one's does
but for the compaction (it lists nothing).  Run on the GPU box:  python tools/time_frame_tracker.py"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_frame_tracker.py measures the HIP path; it needs a GPU"
    from time_frame_frontend import frame
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.frame import FramePipeline, FrameTracker
    from hs_pose_amd.HSPose import HSPose

    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 0
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).eval()
    mean_shapes, sym_infos = torch.full((6, 3), 0.2, device=dev), torch.zeros(6, 4, device=dev)
    K = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)
    res = {"H": 480, "W": 640, "O": int(FLAGS.img_size), "n_pts": int(FLAGS.random_points), "pad": float(FLAGS.DZI_PAD_SCALE),
           "rounds": args.rounds, "replays_per_round": args.steps, "pool_sampler": FLAGS.pool_sampler, "unit": "us per replay"}

    def window(graph):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.steps

    def stat(v):
        return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}

    for how in ("device", "fps"):
        for n in (1, 4):
            depth, masks, bboxes = frame(n)
            depth_d, masks_d = torch.from_numpy(depth).to(dev), torch.from_numpy(masks).to(dev)
            cls = np.arange(n) % 6 + 1
            sampler = pc_sample.DeviceSampler(1, dev) if how == "device" else "fps"
            pipe = FramePipeline(net, mean_shapes, sym_infos, sampler=sampler, one_graph=True, sync=False)
            pipe(depth_d, masks_d, bboxes, cls, K)
            (fg,) = pipe.frame_graphs.values()
            # the tracks: at the discs' centres and depths, the discs' diameters as sizes
            RT, size = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), np.zeros((n, 3), np.float32)
            for j, (y1, x1, y2, x2) in enumerate(bboxes):
                cy, cx = (y1 + y2) // 2, (x1 + x2) // 2
                z = max(float(depth[cy, cx]), 800.0) / 1000.0
                RT[j, :3, 3] = (cx - K[0, 2]) * z / K[0, 0], (cy - K[1, 2]) * z / K[1, 1], z
                size[j] = (x2 - x1) * z / K[0, 0]
            RT_d, size_d = torch.from_numpy(RT).to(dev), torch.from_numpy(size).to(dev)
            trk = FrameTracker(net, mean_shapes, sym_infos, sampler=sampler)
            trk.start(RT_d, size_d, cls)
            first = trk.step(depth_d, K)
            (tg,) = trk.graphs.values()
            for _ in range(args.warmup):
                fg.graphed.graph.replay()
                tg.graphed.graph.replay()
            tracked, yard = [], []
            for _ in range(args.rounds):
                yard.append(window(fg.graphed.graph))
                trk.start(RT_d, size_d, cls)
                tracked.append(window(tg.graphed.graph))
            lost = trk.state()[2].cpu().numpy()
            res[f"{how}_n{n}"] = {"tracked_us": stat(tracked), "one_graph_pipeline_us": stat(yard),
                                  "first_status": first[2].cpu().tolist(), "held": int((lost == 0).sum())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
