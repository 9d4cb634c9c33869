"""What the Chamfer reconstruction term (``config.FLAGS.prop_sym_cd_w``) costs, timed in ONE process:

  forward   at B = 16, N = 1028, device time by replaying a captured call (tools/time_chamfer_fps.py's ``gpu_us``):
            ``fused`` -- ``ops.recon_chamfer`` (hsp_recon_chamfer_fwd: the target made in the kernel, both directions in one
            launch, the ordered sum in a second); ``composed`` -- what the same term takes without it: the torch ops that build
            the target (losses.py's), ``ops.chamfer`` (hsp_chamfer_fwd's two launches) and the two sums -- listed twice, the gap
            between its two runs being the spread the fused figure is read against; ``pair`` -- hsp_chamfer_fwd's two launches
            alone on a ready target; and the same three with their backward (``*_fwd_bwd``: the ordered backward for the fused
            form, the atomic one for the others).
  step      ``graph.GraphedTrainStep.run()`` at B = 16, N = 1028 under device draws with ``FLAGS.reproducible`` on, captured with
            the weight at 0 and at 1, in fp32 rows and in bf16 rows, timed ALTERNATELY in rounds (tools/time_reproducible_step.py's
            protocol: the weight-0 form listed twice, interleaved; median and min - max over the rounds).

Run on the GPU box:  python tools/time_recon_chamfer.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch

from time_chamfer_fps import gpu_us
from time_pool_sampler import alternate

ITEM_KEYS = ("obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")


def forward_times(dev, B, N, reps):
    import ref_cpu as oc
    import _recon_chamfer_ref as rc
    from hs_pose_amd import ops
    from hs_pose_amd.losses import prop_rot_loss
    batch = {k: v.to(dev) for k, v in rc.batch(oc, B, N, (rc.SYM_Y, rc.SYM_YX, rc.SYM_NONE), seed=5).items()}
    PC, R, t, sym = batch["PC"], batch["gt_R"], batch["gt_t"], batch["sym"]
    recon = batch["recon"].requires_grad_(True)
    G = prop_rot_loss._sym_target(PC, R, t, sym)[0].contiguous()

    def composed(P):
        target, skip = prop_rot_loss._sym_target(PC, R, t, sym)
        d1, d2, _, _ = ops.chamfer(P, target.detach())
        keep = (~skip).view(-1, 1)
        return 1.0 * (torch.where(keep, d1, 0.0).sum() + torch.where(keep, d2, 0.0).sum()) / (B * N)

    def pair(P):
        d1, d2, _, _ = ops.chamfer(P, G)
        return d1, d2

    def with_backward(fn):
        def run():
            out = fn(recon)
            out = out if isinstance(out, torch.Tensor) else out[0].sum() + out[1].sum()
            return torch.autograd.grad(out, recon)[0]
        return run
    forms = {"fused": lambda: ops.recon_chamfer(recon.detach(), PC, R, t, sym, 1.0), "composed": lambda: composed(recon.detach()),
             "pair": lambda: pair(recon.detach()), "composed_again": lambda: composed(recon.detach()),
             "fused_fwd_bwd": with_backward(lambda P: ops.recon_chamfer(P, PC, R, t, sym, 1.0)),
             "composed_fwd_bwd": with_backward(composed), "pair_fwd_bwd": with_backward(pair)}
    out = {name: round(gpu_us(fn, reps), 2) for name, fn in forms.items()}
    out["fused_again"] = round(gpu_us(forms["fused"], reps), 2)
    out["composed_spread"] = round(abs(out["composed"] - out["composed_again"]), 2)
    out["fused_minus_faster_composed"] = round(min(out["fused"], out["fused_again"]) - min(out["composed"], out["composed_again"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="f32,bf16", help="comma-separated subset of the row types whose step is timed ('none': forward alone)")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_recon_chamfer.py measures the HIP path; it needs a GPU"
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
    FLAGS.reproducible = True
    case = oc.hspose_train_case(B, N, 7)
    static = lambda: {"PC": case["PC"].to(dev), **{k: case[k].to(dev) for k in ITEM_KEYS}}       # noqa: E731

    # the steps are captured first: a capture must precede a network's first eager backward, and the forward figures run eagerly
    forms, groups, keep = {}, {}, []
    for tag in ([] if args.only == "none" else args.only.split(",")):
        built = {}
        for form, w in (("off", 0.0), ("on", 1.0)):
            FLAGS.prop_sym_cd_w = w                                    # read when a call is issued: the capture keeps its form
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
        FLAGS.prop_sym_cd_w = 0.0
        forms[f"{tag}_off"], forms[f"{tag}_on"], forms[f"{tag}_off_again"] = built["off"], built["on"], built["off"]
        groups[tag] = (f"{tag}_off", f"{tag}_on", f"{tag}_off_again")

    timed = alternate(forms, args.rounds, args.steps, args.warmup) if forms else {}
    torch.cuda.synchronize()
    verdict = {}
    for tag, (a, b, a2) in groups.items():
        v = {}
        for clock in ("wall_ms", "device_ms"):
            v[clock] = {"off": timed[a][clock], "off_again": timed[a2][clock], "on": timed[b][clock],
                        "on_minus_faster_off": round(timed[b][clock] - min(timed[a][clock], timed[a2][clock]), 4),
                        "off_spread": round(abs(timed[a][clock] - timed[a2][clock]), 4)}
        verdict[tag] = v
    res = {"B": B, "N": N, "forward_us": forward_times(dev, B, N, args.reps), "rounds": args.rounds, "steps_per_round": args.steps,
           "forms": timed, "verdict": verdict}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
