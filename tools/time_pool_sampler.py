"""The two pool samplers ('random': host randperm + upload before each replay; 'fps': per-cloud farthest-point sampling inside the
graph) timed against each other in ONE process:

  * the HS-stack training step bench.py times (B = 16, N = 1028, fp32 rows) as a hipGraph replay -- ``GraphedStep.run()``, i.e. with
    the host draw + upload the 'random' sampler needs;
  * the single-instance inference replay (``GraphedInference.run()``, eval mode);
  * the sampler's own launch (ops.fps_levels) and the coarse levels' geometry each sampler issues after it: the fused
    ops.geometry_all of the 'random' path against ops.knn_xyz x 3 + ops.nn1 x 2 of the 'fps' path, each as a graph replay.

Both samplers are captured first, then timed ALTERNATELY in rounds (random, fps, random, fps, ...), every round a window of
``--steps`` replays between device events after a synchronise; the figures are the median over the rounds with the min - max
spread, wall clock per step alongside (it holds the host work).  Run on the GPU box:  python tools/time_pool_sampler.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch
from hs_pose_amd.graph import capture_scope


def window(fn, steps):
    """(device ms, wall ms) per call over ``steps`` calls"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, 1e3 * (time.perf_counter() - t0) / steps


def alternate(forms, rounds, steps, warmup):
    """forms: name -> callable.  name -> dict(median / min / max of the per-round device and wall ms per call)"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    got = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            got[k].append(window(fn, steps))
    out = {}
    for k, v in got.items():
        d, w = [a for a, _ in v], [b for _, b in v]
        out[k] = {"device_ms": round(statistics.median(d), 4), "device_ms_min": round(min(d), 4), "device_ms_max": round(max(d), 4),
                  "wall_ms": round(statistics.median(w), 4), "wall_ms_min": round(min(w), 4), "wall_ms_max": round(max(w), 4)}
    return out


def graph_of(fn):
    """``fn`` captured once; returns the replay callable"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with capture_scope() as cap:
        cap.warm_up(fn)
        g = cap.capture(fn)
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_pool_sampler.py measures the HIP path; it needs a GPU"
    import ref_cpu as oc
    from hs_pose_amd import gcn3d, ops
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.FaceRecon import FaceRecon
    from hs_pose_amd.graph import GraphedInference, GraphedStep
    from hs_pose_amd.HSPose import HSPose

    dev = torch.device("cuda:0")
    B, N = args.batch, args.points
    n1 = N // 4
    n2 = n1 // 4
    res = {"B": B, "N": N, "rounds": args.rounds, "steps_per_round": args.steps}

    # ---- the HS-stack step ------------------------------------------------------------------------------------------------------
    pc = oc.hash_tensor((B, N, 3), 1, 0.05)
    centred = (pc - pc.mean(dim=1, keepdim=True)).to(dev)
    obj = (torch.arange(B) % 6).float().reshape(B, 1).to(dev)
    dfeat = oc.hash_tensor((B, N, 1286), 2, 1.0).to(dev)
    steps = {}
    for how in gcn3d.SAMPLERS:
        FLAGS.reset()
        FLAGS.train = 0
        FLAGS.pool_sampler = how
        torch.manual_seed(0)
        net = FaceRecon().to(dev).train()
        steps[how] = GraphedStep(net, centred, obj, dfeat).run       # (the sampler is fixed at capture)
    res["step"] = alternate(steps, args.rounds, args.steps, args.warmup)
    steps = None

    # ---- single-instance inference ----------------------------------------------------------------------------------------------
    PC = (oc.hash_tensor((1, N, 3), 3, 0.05) + torch.tensor([0.0, 0.0, 0.8])).to(dev)
    one = dict(obj_id=torch.tensor([2], device=dev), mean_shape=torch.tensor([[0.2, 0.15, 0.25]], device=dev),
               sym=torch.tensor([[1, 0, 0, 0]], dtype=torch.int32, device=dev))
    infer = {}
    for how in gcn3d.SAMPLERS:
        FLAGS.reset()
        FLAGS.train = 0
        FLAGS.pool_sampler = how
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).eval()
        infer[how] = GraphedInference(net, PC, one["obj_id"], one["mean_shape"], one["sym"]).run
    res["inference_1"] = alternate(infer, args.rounds, args.steps, args.warmup)
    infer = None
    FLAGS.reset()

    # ---- the sampler's launch and the coarse geometry of each path, on their own ---------------------------------------------------
    k, pk = 20, gcn3d.POOL_K
    k1, k2 = min(k, n1 // 8), min(k, n2 // 8)
    for tag, x in (("B%d" % B, centred), ("B1", PC)):
        sel1, v1, v2 = ops.fps_levels(x, n1, n2)
        s1, s2 = sel1[0].contiguous(), torch.arange(n2, dtype=torch.int32, device=dev)
        parts = {"fps_levels": graph_of(lambda: ops.fps_levels(x, n1, n2)),
                 "searches_fps_path": graph_of(lambda: (ops.knn_xyz(x, k, pk), ops.knn_xyz(v1, k1, pk), ops.knn_xyz(v2, k2, 0),
                                                        ops.nn1(x, v1), ops.nn1(x, v2)))}
        if ops.geometry_all(x, k, pk, s1, s2, k1, pk, k2) is not None:
            parts["geometry_all_random_path"] = graph_of(lambda: ops.geometry_all(x, k, pk, s1, s2, k1, pk, k2))
        res["parts_" + tag] = alternate(parts, args.rounds, args.steps, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
