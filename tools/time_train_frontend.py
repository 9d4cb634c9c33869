"""The training loader's front end (pc_sample.train_batch_to_pcl: hsp_roi_defor + hsp_crop_compact + hsp_sample_ids +
hsp_frames_to_pcl, nothing copied back) timed per batch of B = 16 and B = 64 items, one 480 x 640 uint16 frame and label image
per item, O = 256, 1028 points per item, beside a numpy RESTATEMENT of the same chain on the CPU
(tests/_roi_defor_ref.py::cpu_train_batch_to_pcl: the nearest-neighbour crops, the mask rule, boolean compaction, float64
back-projection, the same keyed draws).  The CPU figure is that restatement's on ONE core, NOT the reference's
cv2.warpAffine / cv2.erode chain in its 20 loader workers (cv2 is not installed where this project is built); it includes
neither the file reads in front of the chain nor the upload of the clouds behind it.

Device and CPU forms are timed ALTERNATELY in rounds like tools/time_frame_frontend.py: every round a window of ``--steps``
calls between device events after a synchronise, and the wall clock around it (the CPU form: wall clock only); the figures are
the median over the rounds with the min - max spread.  Frames and label images are on the device before the clock starts;
the windows, ids and K are uploaded inside every call, as a loader would.  The kernels are also timed on their own
(ops.KernelTimer).  Run on the GPU box:  python tools/time_train_frontend.py
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


def batch(B, seed=0):
    """depth (B,480,640) uint16 with holes, label images with one disc each, its id and its box (x1, y1, x2, y2)"""
    H, W = 480, 640
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = (800 + 60 * np.sin(xx / 37) + 45 * np.cos(yy / 29)).astype(np.uint16)
    depth, labels, ids, boxes = np.empty((B, H, W), np.uint16), np.zeros((B, H, W), np.uint8), [], []
    for j in range(B):
        depth[j] = base
        depth[j][rng.rand(H, W) < 0.1] = 0
        cy, cx, r = rng.randint(80, H - 80), rng.randint(80, W - 80), rng.randint(25, 70)
        ids.append(rng.randint(1, 7))
        labels[j][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = ids[-1]
        boxes.append((cx - r, cy - r, cx + r, cy + r))
    return depth, labels, np.array(ids, dtype=np.int32), np.array(boxes, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_train_frontend.py measures the HIP path; it needs a GPU"
    import _roi_defor_ref as rr
    from hs_pose_amd import ops, pc_sample

    dev = torch.device("cuda:0")
    sampler = pc_sample.DeviceSampler(1, dev)
    K = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)
    O, n_pts, pro = 256, 1028, 0.5
    res = {"H": 480, "W": 640, "O": O, "n_pts": n_pts, "mask_pro": pro, "mask_iters": 1, "rounds": args.rounds,
           "steps_per_round": args.steps, "cpu_steps_per_round": args.cpu_steps,
           "cpu_form": "numpy restatement on one core (not the reference's cv2 chain)"}
    for B in (16, 64):
        depth, labels, ids, boxes = batch(B)
        depth_d, labels_d = torch.from_numpy(depth).to(dev), torch.from_numpy(labels).to(dev)
        np.random.seed(3)
        centers, scales = pc_sample.dzi_windows(boxes, 480, 640)

        def device_form():
            return pc_sample.train_batch_to_pcl(depth_d, labels_d, ids, centers, scales, K, n_pts=n_pts, out_size=O,
                                                mask_pro=pro, sampler=sampler)

        def cpu_form(call):
            belongs = labels == ids[:, None, None]
            return rr.cpu_train_batch_to_pcl(depth, belongs, centers, scales, K, n_pts, O, 1, pc_sample.mask_gate(pro),
                                             sampler.seed, call)

        call = sampler.get_state()[1]
        a, sa = device_form()
        b, sb = cpu_form(call)
        assert np.array_equal(sa.cpu().numpy(), sb) and np.array_equal(a.cpu().numpy(), b, equal_nan=True), \
            "device and restatement disagree"
        for _ in range(args.warmup):
            device_form()
        dms, dwall, cwall = [], [], []
        for _ in range(args.rounds):
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
                cpu_form(call)
            cwall.append(1e3 * (time.perf_counter() - t0) / args.cpu_steps)
        timer = ops.KernelTimer(only=("hsp_roi_defor", "hsp_crop_compact_u16", "hsp_frames_to_pcl_u16", "hsp_sample_ids"))
        prev = ops.set_timer(timer)
        try:
            for _ in range(args.steps):
                device_form()
            torch.cuda.synchronize()
        finally:
            ops.set_timer(prev)

        def stat(v):
            return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res[f"B{B}"] = {"device_stream_ms": stat(dms), "device_wall_ms": stat(dwall), "cpu_restatement_wall_ms": stat(cwall),
                        "rejected": int((sa != 0).sum()),
                        "kernels_us": {name: round(d["avg_us"], 2) for (name, _), d in timer.summary().items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
