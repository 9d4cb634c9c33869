"""The farthest-point instance sampler (hsp_fps_ids_*): device time of the launch from replaying a captured call, beside the dense
register kernel on the same candidates (hsp_fps_levels_f32, B = n: the same pick chain without the ragged set-up), beside the
keyed draw it stands in for (hsp_sample_ids), and the one-graph frame replay under 'fps' against 'device'.
Run on the GPU box:  python tools/time_fps_ids.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

from tools.time_chamfer_fps import gpu_us

K_REAL = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)


def surface(H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    return (800 + 60 * np.sin(xx / 37) + 45 * np.cos(yy / 29) + rng.randint(0, 4, size=(H, W))).astype(np.uint16)


def launches(dev, out):
    from hs_pose_amd import ops, pc_sample
    from hs_pose_amd._lib import lib
    H, W, O, S = 480, 640, 256, 1028
    cap = lib().hsp_fps_ids_cap()
    depth = torch.from_numpy(surface(H, W, 0)).to(dev)
    K = torch.from_numpy(K_REAL.reshape(1, 9)).to(dev)
    yy, xx = np.mgrid[112:112 + O, 192:192 + O]                     # a 1:1 window: crop raster order is frame raster order
    window = (yy * W + xx).reshape(-1).astype(np.int32)
    sampler = pc_sample.DeviceSampler(1, dev)
    key = sampler.advance()
    for n in (1, 8):
        src = torch.from_numpy(np.tile(window, (n, 1))).to(dev)
        for c in (2000, 8000, 12288, 40000):
            count = torch.full((n, 2), c, dtype=torch.int32, device=dev)
            t_ids = gpu_us(lambda: ops.fps_ids(depth, K, src, count, S, 2, 2))
            m = min(c, cap)
            g = torch.tensor([(t * c) // cap if c > cap else t for t in range(m)], dtype=torch.int32, device=dev)
            cloud = ops.frame_to_pcl(depth, K, src, g[None].expand(n, m).contiguous())
            t_dense = gpu_us(lambda: ops.fps_levels(cloud, S, 0))
            t_draw = gpu_us(lambda: ops.sample_ids(count, S, key, 2, 2, 0))
            sel = ops.fps_levels(cloud, S, 0)[0]
            same = bool(torch.equal(g[sel.long()], ops.fps_ids(depth, K, src, count, S, 2, 2)[0]))
            out.append({"op": "fps_ids", "n": n, "c": c, "candidates": m, "S": S, "us": round(t_ids, 1),
                        "us_per_pick": round(t_ids / S, 3), "fps_levels_dense_us": round(t_dense, 1),
                        "fps_levels_us_per_pick": round(t_dense / S, 3), "ratio_to_dense": round(t_ids / t_dense, 3),
                        "sample_ids_us": round(t_draw, 1), "picks_equal_dense": same})


def frame_replays(dev, out):
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.frame import FramePipeline
    from hs_pose_amd.HSPose import HSPose
    FLAGS.reset()
    FLAGS.train = 0
    FLAGS.pool_sampler = "fps"
    try:
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).eval()
        mean_shapes = torch.full((6, 3), 0.2, device=dev)
        sym_infos = torch.zeros(6, 4, device=dev)
        H, W = 480, 640
        depth = torch.from_numpy(surface(H, W, 1)).to(dev)
        yy, xx = np.mgrid[0:H, 0:W]
        for n in (1, 4):
            masks, boxes = np.zeros((n, H, W), np.uint8), []
            for j in range(n):
                cy, cx, r = 120 + 80 * j, 150 + 110 * j, 60
                masks[j] = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
                boxes.append((cy - r, cx - r, cy + r, cx + r))
            masks_d, boxes = torch.from_numpy(masks).to(dev), np.array(boxes, dtype=np.int32)
            row = {"op": "frame_replay", "n": n, "pool_sampler": "fps"}
            for how in ("fps", "device"):
                pipe = FramePipeline(net, mean_shapes, sym_infos, sampler=how, one_graph=True)
                assert pipe(depth, masks_d, boxes, np.ones(n, np.int64), K_REAL) is not None
                (fg,) = pipe.frame_graphs.values()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = 20
                e0.record()
                for _ in range(reps):
                    fg.graphed.graph.replay()
                e1.record()
                torch.cuda.synchronize()
                row[f"{how}_us"] = round(1e3 * e0.elapsed_time(e1) / reps, 1)
            out.append(row)
    finally:
        FLAGS.reset()


def main():
    dev = torch.device("cuda:0")
    out = []
    launches(dev, out)
    frame_replays(dev, out)
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
