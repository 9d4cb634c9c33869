"""What ``config.FLAGS.reproducible`` costs, timed in ONE process:

  step      ``graph.GraphedTrainStep.run()`` at B = 16, N = 1028 under device draws (``draws=sampler``), captured with the switch
            off and with it on, in fp32 rows and in bf16 rows: the ordered pooling backward (a reverse-index build and a gather
            per Pool_layer instead of one LDS scatter) and the keyed Dropout (one launch each way per head instead of torch's);
  pool_bwd  the per-call time of the two Pool_layers' backward launches at the step's shapes (1028 -> 257 rows of 128 columns,
            257 -> 64 rows of 256 columns, k = 4, lists from the coordinate search) in both forms and both storage types, with
            one kept-row list shared by the batch (the step's form) and with a list per cloud (the 'fps' sampler's form), from
            ``ops.KernelTimer`` over eager calls (HIP events around each entry point).

Every object is captured first, each on a network of its own, then the forms are timed ALTERNATELY in rounds like
tools/time_step_draws.py: every round a window of ``--steps`` steps between device events after a synchronise, wall clock
alongside; the figures are the median over the rounds with the min - max spread.  The switch-off form is listed twice
(``*_off`` and ``*_off_again``), interleaved: the gap between its two runs is the noise floor the switch's cost is read against.
Run on the GPU box:  python tools/time_reproducible_step.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
import torch

from time_pool_sampler import alternate

ITEM_KEYS = ("obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")
POOL_ENTRIES = ("hsp_gather_max_bwd", "hsp_gather_max_bwd_bf16", "hsp_gather_max_bwd_sel", "hsp_gather_max_bwd_sel_bf16",
                "hsp_gather_max_bwd_csr", "hsp_gather_max_bwd_csr_bf16", "hsp_rev_build_sel")


def pool_backward_times(dev, B, N, calls):
    """{dtype: {lists: {level: {form: {entry point: avg us}}}}} of the two Pool_layers' backward launches; ``lists``: "shared" --
    one kept-row list for the batch, what a Pool_layer draws ('random' sampler, host or device draws: the step's form) -- and
    "per_cloud" -- a (B,Nq) list, the form of the 'fps' sampler"""
    import ref_cpu as oc
    from hs_pose_amd import ops
    from hs_pose_amd.config import FLAGS
    out = {}
    xyz = oc.hash_tensor((B, N, 3), 7, 0.05).to(dev)
    for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        out[tag] = {}
        for lists in ("shared", "per_cloud"):
            out[tag][lists] = {}
            pts, n = xyz, N
            for level, C in enumerate((128, 256)):
                gen = torch.Generator().manual_seed(n)                 # the kept rows: a randperm prefix, one or one per cloud
                if lists == "shared":
                    qsel = torch.randperm(n, generator=gen)[: n // 4].to(torch.int32).to(dev)
                    kept = pts[:, qsel.long()]
                else:
                    qsel = torch.stack([torch.randperm(n, generator=gen)[: n // 4] for _ in range(B)]).to(torch.int32).to(dev)
                    kept = torch.gather(pts, 1, qsel.long().unsqueeze(-1).expand(-1, -1, 3))
                idx = ops.knn(pts, 4)
                feat = oc.hash_tensor((B, n, C), 11 + level, 1.0).to(dev).to(dtype)
                g = oc.hash_tensor((B, n // 4, C), 13 + level, 1.0).to(dev).to(dtype)
                res = {}
                for form, on in (("off", False), ("on", True)):
                    FLAGS.reproducible = on
                    timer = ops.KernelTimer(only=POOL_ENTRIES)
                    for i in range(calls + 3):
                        f = feat.clone().requires_grad_(True)
                        o = ops.gather_max(f, idx.clone(), 4, qsel=qsel)   # (a fresh idx: the reverse map is built every step)
                        prev = ops.set_timer(timer if i >= 3 else None)
                        try:
                            o.backward(g)
                        finally:
                            ops.set_timer(prev)
                    torch.cuda.synchronize()
                    res[form] = {name: round(d["avg_us"], 2) for (name, _), d in timer.summary().items()}
                FLAGS.reproducible = False
                out[tag][lists][f"pool_{level + 1}_Ns{n}_Nq{n // 4}_C{C}"] = res
                pts, n = kept.contiguous(), n // 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pool-calls", type=int, default=50)
    ap.add_argument("--only", default="f32,bf16", help="comma-separated subset of the row types whose step is timed ('none': pool_bwd alone)")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_reproducible_step.py measures the HIP path; it needs a GPU"
    import ref_cpu as oc
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.graph import GraphedTrainStep
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.train import TrainDriver

    dev = torch.device("cuda:0")
    B, N = args.batch, args.points
    FLAGS.reset()
    FLAGS.train = 1
    case = oc.hspose_train_case(B, N, 7)
    static = lambda: {"PC": case["PC"].to(dev), **{k: case[k].to(dev) for k in ITEM_KEYS}}

    forms, groups, keep = {}, {}, []
    for tag in ([] if args.only == "none" else args.only.split(",")):
        built = {}
        for form, on in (("off", False), ("on", True)):
            FLAGS.reproducible = on                                    # read when a call is issued: the capture keeps its form
            torch.manual_seed(0)
            net = HSPose("PoseNet_only").to(dev).train()
            drv = TrainDriver(net, total_iters=10 ** 6, check_nan=False)
            if tag == "bf16":
                net.set_feature_dtype(torch.bfloat16)
            sampler = pc_sample.DeviceSampler(1, dev)
            step = GraphedTrainStep(net, drv.optimizer, static(), scheduler=drv.scheduler, draws=sampler)
            keep.append((net, drv, step))

            def run(step=step, sampler=sampler):
                sampler.advance()
                step.run()
            built[form] = run
        FLAGS.reproducible = False
        forms[f"{tag}_off"], forms[f"{tag}_on"], forms[f"{tag}_off_again"] = built["off"], built["on"], built["off"]
        groups[tag] = (f"{tag}_off", f"{tag}_on", f"{tag}_off_again")

    timed = alternate(forms, args.rounds, args.steps, args.warmup) if forms else {}
    torch.cuda.synchronize()
    verdict = {}
    for tag, (a, b, a2) in groups.items():
        v = {}
        for clock in ("wall_ms", "device_ms"):
            floor = abs(timed[a][clock] - timed[a2][clock])
            gap = timed[b][clock] - min(timed[a][clock], timed[a2][clock])
            v[clock] = {"off": timed[a][clock], "off_again": timed[a2][clock], "on": timed[b][clock],
                        "on_minus_faster_off": round(gap, 4), "off_spread": round(floor, 4), "on_slower_beyond_spread": bool(gap > floor)}
        verdict[tag] = v
    res = {"B": B, "N": N, "rounds": args.rounds, "steps_per_round": args.steps, "forms": timed, "verdict": verdict,
           "pool_bwd_us": pool_backward_times(dev, B, N, args.pool_calls)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
