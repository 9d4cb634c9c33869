"""Run by test_gpu_recon_chamfer.py in a fresh process (a capture must precede the network's first eager backward):
usage: python tests/_recon_chamfer_step_check.py mode        (B = 4, N = 256, Dropout at its default 0.2)

Whole training steps with the Chamfer reconstruction term, ``FLAGS.reproducible`` on, device draws under one ``DeviceSampler``
(the helpers are tests/_reproducible_step_check.py's).

train2x_f32 / train2x_bf16: ``FLAGS.prop_sym_cd_w = 1.0``.  A ``GraphedTrainStep(draws=sampler)``; three steps, the checkpoint loaded
  back, three steps again: every loss term (the 20th among them, positive), every gradient of the last step, every parameter and
  buffer ``torch.equal``; torch's device generator does not move across the build nor the steps; ``recon`` is an fp32 output; the
  graphed first step equals the eager step of a twin network under the same key bit for bit -- every loss term and gradient.
weight0: the flag at its default.  Three steps of a network as it is, and three of a twin whose ``pose_losses`` is the statement
  this repository had before the flag existed (19 terms, no question asked) and for which ``ops.recon_chamfer`` raises: the same
  loss keys -- today's -- and the same parameters and buffers, bit for bit.
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import torch

from hs_pose_amd import fused_losses, ops, pc_sample
from hs_pose_amd.config import FLAGS
from hs_pose_amd.graph import GraphedTrainStep
from _reproducible_step_check import CALL, SEED, compare, make, sampler_at, steps, train_batch

CD = "prop_loss.Prop_sym_cd"


def train2x(bf16, dev):
    FLAGS.prop_sym_cd_w = 1.0
    batch = train_batch(dev)
    bad = []
    sampler = sampler_at(dev)
    net, drv = make(dev, bf16, sampler)
    rng_build = torch.cuda.get_rng_state().clone()
    graphed = GraphedTrainStep(net, drv.optimizer, batch, scheduler=drv.scheduler, warmup=2, draws=sampler)
    rng0 = torch.cuda.get_rng_state().clone()
    if not torch.equal(rng_build, rng0):
        bad.append("torch's device generator moved across the build")
    if graphed.output_dict["recon"].dtype != torch.float32:
        bad.append(f"recon is {graphed.output_dict['recon'].dtype}")
    ckpt = copy.deepcopy(drv.checkpoint(1, 0))
    first = steps(graphed, sampler, 3)
    drv.load_checkpoint(ckpt)
    second = steps(graphed, sampler, 3)
    if not torch.equal(rng0, torch.cuda.get_rng_state()):
        bad.append("torch's device generator moved across the steps")
    compare(bad, "second run", first, second)
    for i, rec in enumerate(first["loss"]):
        if CD not in rec or not float(rec[CD]) > 0 or len(rec) != 20:
            bad.append(f"step {i + 1}: {len(rec)} terms, {CD} = {rec.get(CD)}")
    if all(torch.equal(first["loss"][0][k], first["loss"][1][k]) for k in first["loss"][0]):
        bad.append("steps 1 and 2 computed the same losses: the steps do not advance")
    # the eager step of a twin network under the same key
    sampler2 = sampler_at(dev)
    net2, drv2 = make(dev, bf16, sampler2)
    with pc_sample.draw_scope(sampler2, dev):
        _, ld = net2(do_loss=True, **batch)
    total = net2.total_loss(ld)
    drv2.optimizer.zero_grad()
    total.backward()
    torch.cuda.synchronize()
    eager_loss = {f"{g}.{k}": v.detach() for g, d in ld.items() for k, v in d.items()}
    for k, v in first["loss"][0].items():
        if not torch.equal(v, eager_loss[k]):
            bad.append(f"eager against graph: loss {k}: {float(eager_loss[k])!r} against {float(v)!r}")
    grads = {k: p.grad.detach() for k, p in net2.named_parameters() if p.grad is not None}
    if sorted(grads) != sorted(first["grads_first"]):
        bad.append("eager against graph: the gradients are not the same set")
    differ = [k for k in grads if k in first["grads_first"] and not torch.equal(grads[k], first["grads_first"][k])]
    if differ:
        bad.append(f"eager against graph: {len(differ)} of {len(grads)} gradients differ, e.g. {differ[:4]}")
    print(f"train2x {'bf16' if bf16 else 'f32'} with the term: step 3 total {float(graphed.total.detach()):.6f}, {CD} "
          f"{float(first['loss'][2][CD]):.6e}; eager against graph: {len(differ)} of {len(grads)} gradients differ; {len(bad)} mismatches")
    return bad


def _pose_losses_before_the_flag(net_out, PC, gt_R, gt_t, gt_s, mean_shape, sym, obj_id):
    """fused_losses.pose_losses as it stood before FLAGS.prop_sym_cd_w: the 19 terms of the loss kernels and their total"""
    N_TERMS, TERMS = fused_losses.N_TERMS, fused_losses.TERMS
    vals = fused_losses._PoseLosses.apply(*[net_out[k] for k in fused_losses._NET], PC, gt_R, gt_t, gt_s, mean_shape, sym,
                                          obj_id.reshape(-1).float())
    out, k = fused_losses.LossDict(), 0
    out.total = vals[N_TERMS]
    out.terms = tuple(vals[:N_TERMS])
    for group, keys in TERMS:
        out[group] = {}
        for key in keys:
            out[group][key] = vals[k]
            k += 1
    return out


def weight0(dev):
    batch = train_batch(dev)
    bad = []
    runs = []
    for before in (False, True):
        saved = fused_losses.pose_losses, ops.recon_chamfer
        if before:
            def never(*a, **k):
                raise AssertionError("ops.recon_chamfer was called with the weight at 0")
            fused_losses.pose_losses, ops.recon_chamfer = _pose_losses_before_the_flag, never
        try:
            sampler = sampler_at(dev)
            net, drv = make(dev, False, sampler)
            graphed = GraphedTrainStep(net, drv.optimizer, {k: v.clone() for k, v in batch.items()}, scheduler=drv.scheduler, warmup=2,
                                       draws=sampler)
            runs.append(steps(graphed, sampler, 3))
        finally:
            fused_losses.pose_losses, ops.recon_chamfer = saved
    today = sorted(f"{g}.{k}" for g, keys in fused_losses.TERMS for k in keys)
    for rec in runs[0]["loss"]:
        if sorted(rec) != today:
            bad.append(f"the loss keys with the weight at 0: {sorted(rec)}")
    compare(bad, "with the flag at 0 against before the flag", runs[1], runs[0])
    print(f"weight0: {len(runs[0]['params'])} parameters compared; {len(bad)} mismatches")
    return bad


def main():
    mode = sys.argv[1]
    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.reproducible = True
    run = {"train2x_f32": lambda: train2x(False, dev), "train2x_bf16": lambda: train2x(True, dev), "weight0": lambda: weight0(dev)}
    if mode not in run:
        raise SystemExit(f"unknown mode {mode}")
    bad = run[mode]()
    for line in bad[:30]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
