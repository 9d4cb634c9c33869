"""The frame front end (pc_sample.frame_to_pcl: hsp_roi_compact + the count copy + the host draws + hsp_frame_to_pcl) timed per
480 x 640 frame for n = 1, 4, 8 detections, O = 256, 1028 points per instance, beside a numpy RESTATEMENT of the same chain on
the CPU (tests/test_frame_host.py::cpu_frame_to_pcl: the three nearest-neighbour crops, boolean compaction, float64
back-projection, the same draws).  The CPU figure is that restatement's, NOT the reference's cv2.warpAffine chain (cv2 is not
installed where this project is built); it does not include the upload of the crops the reference's chain ends with.

Device and CPU forms are timed ALTERNATELY in rounds like tools/time_pool_sampler.py: every round a window of ``--steps`` calls
between device events after a synchronise (the CPU form: wall clock only); the figures are the median over the rounds with the
min - max spread.  The frame, masks and K are on the device before the clock starts (a frame is uploaded once, whatever n).
The device kernels are also timed on their own (ops.KernelTimer).  Run on the GPU box:  python tools/time_frame_frontend.py

Beside the host-sampler front end (the default: the counts come to the host, numpy draws) the same rounds time the
device-sampler one (pc_sample.frame_to_pcl_device: hsp_sample_ids between the two kernels, nothing copied back), and -- frame to
poses, a network with random weights behind the front end -- frame.FramePipeline in its three forms: host sampler, device
sampler issued eagerly, device sampler with the whole frame captured as one graph (``pipeline_*_wall_ms``; each call ends by
reading the per-instance status, or, for the host form, waits for the counts in mid-frame).  ``--no-pipeline`` leaves those out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch


def frame(n, seed=0):
    """depth (480,640) uint16 with holes, n disc masks and their boxes"""
    H, W = 480, 640
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (800 + 60 * np.sin(xx / 37) + 45 * np.cos(yy / 29)).astype(np.uint16)
    depth[rng.rand(H, W) < 0.1] = 0
    masks, bboxes = np.zeros((n, H, W), np.uint8), []
    for j in range(n):
        cy, cx, r = rng.randint(80, H - 80), rng.randint(80, W - 80), rng.randint(25, 70)
        masks[j] = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        bboxes.append((cy - r, cx - r, cy + r, cx + r))
    return depth, masks, np.array(bboxes, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-pipeline", action="store_true", help="front end only: skip the frame-to-poses forms")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_frame_frontend.py measures the HIP path; it needs a GPU"
    import test_frame_host as fh
    from hs_pose_amd import ops, pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.frame import FramePipeline
    from hs_pose_amd.HSPose import HSPose

    dev = torch.device("cuda:0")
    sampler = pc_sample.DeviceSampler(1, dev)
    pipes = {}
    if not args.no_pipeline:
        FLAGS.reset()
        FLAGS.train = 0
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).eval()
        mean_shapes, sym_infos = torch.full((6, 3), 0.2, device=dev), torch.zeros(6, 4, device=dev)
        pipes = {"host": FramePipeline(net, mean_shapes, sym_infos, sampler="host"),
                 "device": FramePipeline(net, mean_shapes, sym_infos, sampler=sampler),
                 "one_graph": FramePipeline(net, mean_shapes, sym_infos, sampler=sampler, one_graph=True)}
    K = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)
    O, n_pts = 256, 1028
    res = {"H": 480, "W": 640, "O": O, "n_pts": n_pts, "rounds": args.rounds, "steps_per_round": args.steps,
           "cpu_steps_per_round": args.cpu_steps, "cpu_form": "numpy restatement (not the reference's cv2 chain)"}
    for n in (1, 4, 8):
        depth, masks, bboxes = frame(n)
        depth_d, masks_d = torch.from_numpy(depth).to(dev), torch.from_numpy(masks).to(dev)

        def device_form():
            centers, scales = pc_sample.roi_windows(bboxes, 480, 640)
            return pc_sample.frame_to_pcl(depth_d, masks_d, centers, scales, K, n_pts=n_pts, out_size=O, sampler="host")

        def sampler_form():
            centers, scales = pc_sample.roi_windows(bboxes, 480, 640)
            return pc_sample.frame_to_pcl_device(depth_d, masks_d, centers, scales, K, n_pts=n_pts, out_size=O, sampler=sampler)

        cls = np.arange(n) % 6 + 1
        forms = {"sampler": sampler_form}
        for name, pipe in pipes.items():
            forms["pipeline_" + name] = lambda pipe=pipe: pipe(depth_d, masks_d, bboxes, cls, K)

        def cpu_form():
            centers, scales = pc_sample.roi_windows(bboxes, 480, 640)
            return fh.cpu_frame_to_pcl(depth, masks, centers, scales, K, n_pts, O, pc_sample.sample_point_ids)

        np.random.seed(1)
        a = device_form()
        np.random.seed(1)
        b = cpu_form()
        assert a is not None and np.array_equal(a.cpu().numpy(), b), "device and restatement disagree"
        for _ in range(args.warmup):
            device_form()
            for f in forms.values():
                assert f() is not None
        dms, dwall, cwall = [], [], []
        fwall = {name: [] for name in forms}
        for _ in range(args.rounds):
            for name, f in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    f()
                torch.cuda.synchronize()
                fwall[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.steps):
                device_form()
            e1.record()
            torch.cuda.synchronize()
            dwall.append(1e3 * (time.perf_counter() - t0) / args.steps)
            dms.append(e0.elapsed_time(e1) / args.steps)
            t0 = time.perf_counter()
            for _ in range(args.cpu_steps):
                cpu_form()
            cwall.append(1e3 * (time.perf_counter() - t0) / args.cpu_steps)
        timer = ops.KernelTimer(only=("hsp_roi_compact_u16", "hsp_frame_to_pcl_u16", "hsp_sample_ids"))
        prev = ops.set_timer(timer)
        try:
            for _ in range(args.steps):
                device_form()
                sampler_form()
            torch.cuda.synchronize()
        finally:
            ops.set_timer(prev)

        def stat(v):
            return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res[f"n{n}"] = {"device_stream_ms": stat(dms), "device_wall_ms": stat(dwall), "cpu_restatement_wall_ms": stat(cwall),
                        "kernels_us": {name: round(d["avg_us"], 2) for (name, _), d in timer.summary().items()}}
        for name, v in fwall.items():
            res[f"n{n}"][("device_sampler" if name == "sampler" else name) + "_wall_ms"] = stat(v)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
