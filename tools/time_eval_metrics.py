"""tools/time_eval_metrics.py -- how long scoring a REAL275-sized run takes: hs_pose_amd.evaluation.PoseEvaluator on the GPU, and
the same contract stated in numpy (tests/_eval_ref.py) on the same machine's CPU.

The run is synthetic (seeded): 2 754 images, the six NOCS classes, a handful of instances per image, the threshold lists of
evaluate.py:127-129 (101 IoU, 61 degree, 21 shift).  Timing: a host clock around ``compute()``, which ends in the copy of the two
AP arrays to the host (a device synchronise); every shape is warmed up first; the window is repeated and the median and the spread
are printed.  ``feed`` is ``add_results`` (packing on the host and the upload), timed apart.  Needs a GPU: there is no fallback.
Prints one JSON line; asserts no time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _eval_cases as cases  # noqa: E402
import _eval_ref  # noqa: E402

SYNSET = ["BG", "bottle", "bowl", "camera", "can", "laptop", "mug"]


def synthetic_run(n_images, seed):
    rng = np.random.default_rng(seed)
    scores = cases.score_pool(rng, 16 * n_images)
    real = list(range(1, len(SYNSET)))
    return [cases.random_image(rng, SYNSET, list(rng.choice(real, size=int(rng.integers(2, 6)), replace=False)), 2, scores)
            for _ in range(n_images)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2754)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-images", type=int, default=None, help="score only the first N images with the numpy statement (default: all)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    from hs_pose_amd.evaluation import PoseEvaluator
    if not torch.cuda.is_available():
        raise SystemExit("time_eval_metrics: no GPU; a CPU run gives no time")
    results = synthetic_run(a.images, a.seed)
    n_pred = sum(len(r["pred_class_ids"]) for r in results)
    n_gt = sum(len(r["gt_class_ids"]) for r in results)

    ev = PoseEvaluator(SYNSET, cases.DEG, cases.SHIFT, cases.IOU, 0.1, True)
    t0 = time.perf_counter()
    ev.add_results(results)
    torch.cuda.synchronize()
    feed_s = time.perf_counter() - t0
    times = []
    for k in range(a.warmup + a.repeats):
        ev._out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iou_aps, pose_aps = ev.compute()
        dt = time.perf_counter() - t0
        if k >= a.warmup:
            times.append(dt)
    times = np.array(times)

    sub = results if a.numpy_images is None else results[:a.numpy_images]
    t0 = time.perf_counter()
    flat = _eval_ref.evaluate(sub, SYNSET, cases.DEG, cases.SHIFT, cases.IOU, 0.1, True)
    numpy_s = time.perf_counter() - t0
    same = None
    if len(sub) == len(results):                                   # (no margins are drawn here: a flipped match would show as a difference)
        same = bool(np.array_equal(flat["iou_aps"], iou_aps, equal_nan=True) and np.array_equal(flat["pose_aps"], pose_aps, equal_nan=True))
    print(json.dumps(dict(images=a.images, predictions=n_pred, ground_truths=n_gt, groups=int(len(ev._out["layout"]["table"])),
                          gpu_compute_ms_median=float(np.median(times) * 1e3), gpu_compute_ms_min=float(times.min() * 1e3),
                          gpu_compute_ms_max=float(times.max() * 1e3), repeats=a.repeats, gpu_feed_ms=feed_s * 1e3,
                          numpy_images=len(sub), numpy_s=numpy_s, aps_equal_numpy=same,
                          mean_iou50=float(iou_aps[-1, 50]), mean_5deg5cm=float(pose_aps[-1, 5, 10]))))


if __name__ == "__main__":
    main()
