"""Gradient accumulation inside the replay (``accumulate=`` on ``graph.GraphedTrainStep``, ``apply='graph'``),
timed per micro-step at B = 16, N = 1028 on fp32 and bf16 rows, all under device draws:

  parent        the ``apply='graph'`` step of ANOTHER TREE (``--parent-tree``: a built checkout of the parent commit), ``accumulate``
                not passed.  THE YARDSTICK.  Without ``--parent-tree`` it is absent and no verdict is given: this code's own
                ``accumulate=1`` is never the yardstick.
  acc1          this tree, ``accumulate=1`` (every slot steps; listed to show the default path has not moved)
  acc2, acc4    this tree, ``accumulate=2`` / ``4``: STEPPING slots (``micro % accumulate == 0``: accumulate + gated Ranger launch) and
                ACCUMULATE-ONLY slots (the accumulate pass alone; the Ranger launch leaves at its gate) reported apart

Every form lives in a worker process of its own (one captured object each), all started first; then the driver runs them
ALTERNATELY, one window at a time, ``--warmup`` windows unrecorded and ``--repeats`` recorded, in one lease.  A window is ``--steps``
replays, a device event between every two, so each replay is timed on its own and sorted by its slot kind; per window the median
per kind, over the windows median and min - max.  ``kernel``: ``hsp_grad_accumulate`` alone over the network's flat total (first = 0,
12 B per parameter) against its traffic floor at 6.3 TB/s.

Expectations the figures confirm or refute (nothing is asserted): an accumulate-only micro-step is no slower than the parent's step
beyond the +-2 % lease spread; a stepping micro-step costs at most the parent's step plus the accumulate pass's floor.
Run on the GPU box:  python tools/time_accumulate.py --parent-tree <checkout of the parent commit, built>
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.3e12            # the achievable HBM rate the floors of DESIGN.md are stated at
ITEM_KEYS = ("obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")


def worker(tree, accumulate, bf16, B, N, horizon):
    """one form: build, answer 'ready', then serve 'window <steps>' / 'kernel' / 'quit' lines from stdin with one JSON line each"""
    sys.path[:0] = [tree, os.path.join(tree, "oracle")]
    import torch
    import ref_cpu as oc
    from hs_pose_amd import ops, pc_sample
    from hs_pose_amd._lib import lib
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.graph import GraphedTrainStep
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.train import TrainDriver

    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.step_draws = "device"
    case = oc.hspose_train_case(B, N, 7)
    batch = {"PC": case["PC"].to(dev), **{k: case[k].to(dev) for k in ITEM_KEYS}}
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).train()
    drv = TrainDriver(net, total_iters=10 ** 6, check_nan=False)
    if bf16:
        net.set_feature_dtype(torch.bfloat16)
    sampler = pc_sample.DeviceSampler(1, dev)
    kw = dict(accumulate=accumulate) if accumulate is not None else {}              # (the parent's tree has no such argument)
    step = GraphedTrainStep(net, drv.optimizer, batch, scheduler=drv.scheduler, draws=sampler, apply="graph", horizon=horizon, **kw)
    acc, micro = accumulate or 1, 0
    torch.cuda.synchronize()
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "window":
            n = int(cmd[1])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                ev[i].record()
                sampler.advance()
                step.run()
            ev[n].record()
            torch.cuda.synchronize()
            wall = 1e3 * (time.perf_counter() - t0) / n
            slots = [((micro + i) % acc == 0, ev[i].elapsed_time(ev[i + 1])) for i in range(n)]
            micro += n
            out = {"wall_ms": wall, "stepping_ms": statistics.median(t for s, t in slots if s)}
            if acc > 1:
                out["accumulate_only_ms"] = statistics.median(t for s, t in slots if not s)
            print(json.dumps(out), flush=True)
        elif cmd[0] == "kernel":                                                    # the accumulate pass alone, this tree only
            fg = drv.optimizer._flat[0]
            a, f = torch.randn_like(fg.flat_g), torch.randn_like(fg.flat_g)
            nsq = torch.ones(1, dtype=torch.float32, device=dev)
            wsb = lib().hsp_sumsq_workspace_bytes(fg.total)
            ws = ops._ws(wsb, dev)
            args = (ops._p(a), ops._p(f), fg.total, ops._p(nsq), 1e30, 0, ops._p(None), ops._p(ws), wsb, ops._stream())
            times = []
            for rep in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(50):
                    ops._run("hsp_grad_accumulate", args)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times.append(1e3 * e0.elapsed_time(e1) / 50)
            us = statistics.median(times)
            floor_us = 1e6 * 12 * fg.total / HBM_BYTES_PER_S
            print(json.dumps({"elements": fg.total, "us": round(us, 2), "us_min": round(min(times), 2), "us_max": round(max(times), 2),
                              "floor_us_at_6.3TBps": round(floor_us, 2), "GBps": round(12 * fg.total / us / 1e3, 1),
                              "note": "both launches of the call (sweep + fold), back to back: the four 38.8 MB buffers fit the "
                                      "256 MiB Infinity Cache, so this is the cache-resident figure"}), flush=True)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=24, help="replays per window (a multiple of 4: whole rounds of every form)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: the yardstick")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--worker", nargs=3, metavar=("TREE", "ACCUMULATE", "DTYPE"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    windows = args.warmup + args.repeats
    horizon = windows * args.steps + 8
    if args.worker:
        tree, a, dtype = args.worker
        worker(tree, None if a == "none" else int(a), dtype == "bf16", args.batch, args.points, horizon)
        return
    if args.steps % 4:
        raise SystemExit("--steps expects a multiple of 4")
    forms = {}
    for dtype in args.dtypes.split(","):
        if args.parent_tree:
            forms[f"{dtype}/parent"] = (os.path.abspath(args.parent_tree), "none", dtype)
        for a in (1, 2, 4):
            forms[f"{dtype}/acc{a}"] = (ROOT, str(a), dtype)
    procs = {}
    try:
        for name, (tree, a, dtype) in forms.items():                                # all built first, one after the other
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--points", str(args.points),
                                  "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--steps", str(args.steps),
                                  "--worker", tree, a, dtype], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
            procs[name] = p
            line = p.stdout.readline().strip()
            if line != "ready":
                raise SystemExit(f"{name}: the worker answered {line!r} (exit {p.poll()})")

        def ask(name, cmd):
            p = procs[name]
            p.stdin.write(cmd + "\n")
            p.stdin.flush()
            line = p.stdout.readline()
            if not line:
                raise SystemExit(f"{name}: the worker ended (exit {p.poll()}) on {cmd!r}")
            return json.loads(line)

        got = {name: [] for name in forms}
        for w in range(windows):
            for name in forms:
                r = ask(name, f"window {args.steps}")
                if w >= args.warmup:
                    got[name].append(r)
            print(f"window {w + 1} of {windows}", file=sys.stderr, flush=True)
        kernel = ask(next(n for n in forms if n.endswith("/acc2")), "kernel")
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
            except OSError:
                pass
        for p in procs.values():
            try:
                p.wait(timeout=60)
            except subprocess.TimeoutExpired:
                p.kill()
    timed = {name: {k: spread([r[k] for r in rs]) for k in rs[0]} for name, rs in got.items()}
    verdict = {}
    floor_ms = kernel["floor_us_at_6.3TBps"] / 1e3
    for dtype in args.dtypes.split(","):
        if f"{dtype}/parent" not in timed:
            continue
        par = timed[f"{dtype}/parent"]["stepping_ms"]
        v = {"parent_step_ms": par["median"], "parent_spread_ms": round(par["max"] - par["min"], 4)}
        for a in (2, 4):
            t = timed[f"{dtype}/acc{a}"]
            only, stepping = t["accumulate_only_ms"]["median"], t["stepping_ms"]["median"]
            v[f"acc{a}"] = {"accumulate_only_ms": only, "accumulate_only_vs_parent": round(only / par["median"], 4),
                            "accumulate_only_within_2pct_of_parent": bool(only <= 1.02 * par["median"]),
                            "stepping_ms": stepping, "stepping_minus_parent_ms": round(stepping - par["median"], 4),
                            "stepping_within_parent_plus_floor_and_2pct": bool(stepping <= 1.02 * par["median"] + floor_ms)}
        v["acc1_vs_parent"] = round(timed[f"{dtype}/acc1"]["stepping_ms"]["median"] / par["median"], 4)
        verdict[dtype] = v
    res = {"B": args.batch, "N": args.points, "warmup_windows": args.warmup, "repeats": args.repeats, "steps_per_window": args.steps,
           "forms": timed, "kernel": kernel, "verdict": verdict}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
