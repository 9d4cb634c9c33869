"""Run by test_gpu_reproducible_step.py in a fresh process (a capture must precede the network's first eager backward):
usage: python tests/_reproducible_step_check.py mode        (B = 4, N = 256, Dropout at its default 0.2)

``FLAGS.reproducible`` on, device draws under one ``DeviceSampler``; torch's generators are never reseeded between runs.

train2x_f32 / train2x_bf16: a ``GraphedTrainStep(draws=sampler)``; a checkpoint of everything the run depends on (parameters,
  BatchNorm buffers, optimizer, scheduler, sampler state), three steps, the checkpoint loaded back in place, three steps again.
  Every loss term of every step, every gradient of the last step, every parameter and every buffer must be ``torch.equal``,
  and torch's device generator state must not move across the build nor across the six steps.  fp32 also prints (never asserts) the largest
  difference between the graphed first step and the eager step of a twin network under the same key, per tensor.
resume: ``TrainDriver(draws=sampler)``: one step, ``checkpoint()``, two more steps; a fresh network, sampler and driver
  ``load_checkpoint()`` and run steps 2-3: the same losses, gradients, parameters and buffers, bit for bit.
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import torch

from hs_pose_amd import pc_sample
from hs_pose_amd.config import FLAGS
from hs_pose_amd.graph import GraphedTrainStep
from hs_pose_amd.HSPose import HSPose
from hs_pose_amd.pc_sample import DeviceSampler
from hs_pose_amd.train import TrainDriver
import ref_cpu as oc

B, N = 4, 256
SEED, CALL = 0x9e3779b97f4a7c15, 2 ** 32 + 1
BATCH_KEYS = ("PC", "obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")


def train_batch(dev):
    case = oc.hspose_train_case(B, N, 7)
    case["aug_bb"] = 1.0 + oc.hash_tensor((B, 3), 40, 0.2)
    case["aug_rt_t"] = oc.hash_tensor((B, 3), 41, 0.02)
    q, _ = torch.linalg.qr(torch.eye(3) + oc.hash_tensor((B, 3, 3), 42, 0.05))
    case["aug_rt_r"] = (q * torch.sign(torch.linalg.det(q)).view(B, 1, 1)).contiguous()
    return {k: case[k].to(dev) for k in BATCH_KEYS}


def make(dev, bf16, sampler, init_seed=0):
    """a training network with Dropout as the reference has it (p = 0.2) and its driver under ``sampler``"""
    cpu_rng = torch.get_rng_state()
    torch.manual_seed(init_seed)                                                 # the initialisation only ...
    net = HSPose("PoseNet_only").to(dev).train()
    torch.set_rng_state(cpu_rng)                                                 # ... the generators go on from where they were
    drv = TrainDriver(net, total_iters=1000, check_nan=False, draws=sampler)
    if bf16:
        net.set_feature_dtype(torch.bfloat16)
    assert all(m.p == 0.2 for m in net.modules() if isinstance(m, torch.nn.Dropout))
    return net, drv


def sampler_at(dev, call=CALL):
    s = DeviceSampler(SEED, dev)
    s.set_state((SEED, call))
    return s


def steps(graphed, sampler, n):
    """n steps -> the record of what they computed"""
    rec = dict(loss=[], grads_first=None)
    for i in range(n):
        sampler.advance()
        graphed.run()
        torch.cuda.synchronize()
        rec["loss"].append({f"{g}.{k}": v.detach().clone() for g, d in graphed.loss_dict.items() for k, v in d.items()})
        if i == 0:
            rec["grads_first"] = {k: p.grad.detach().clone() for k, p in graphed.net.named_parameters() if p.grad is not None}
    rec["grads"] = {k: p.grad.detach().clone() for k, p in graphed.net.named_parameters() if p.grad is not None}
    rec["params"] = {k: p.detach().clone() for k, p in graphed.net.named_parameters()}
    rec["buffers"] = {k: b.detach().clone() for k, b in graphed.net.named_buffers()}
    return rec


def compare(bad, what, a, b, first=0):
    """records a (steps first ..) and b (all its steps) of ``steps``: everything torch.equal"""
    la, lb = a["loss"][first:], b["loss"]
    if len(la) != len(lb):
        bad.append(f"{what}: {len(la)} steps against {len(lb)}")
    for i, (x, y) in enumerate(zip(la, lb)):
        for k in x:
            if not torch.equal(x[k], y[k]):
                bad.append(f"{what}: loss {k} of step {first + i + 1}: {float(x[k])!r} against {float(y[k])!r}")
    for group in ("grads", "params", "buffers"):
        if sorted(a[group]) != sorted(b[group]):
            bad.append(f"{what}: the {group} are not the same set")
        for k, x in a[group].items():
            y = b[group].get(k)
            if y is not None and not torch.equal(x, y):
                d = (x.double() - y.double()).abs().max().item()
                bad.append(f"{what}: {group} {k} differ, max |diff| {d:.3e} of max |value| {x.double().abs().max().item():.3e}")


def eager_figure(dev, batch, grads_graph):
    """the graphed first step against the eager step of a twin network under the same key: printed, never asserted"""
    sampler = sampler_at(dev)
    net, drv = make(dev, False, sampler)
    with pc_sample.draw_scope(sampler, dev):                                     # (advances once: the key of the graph's first step)
        _, ld = net(do_loss=True, **batch)
    total = net.total_loss(ld)
    drv.optimizer.zero_grad()
    total.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach() for k, p in net.named_parameters() if p.grad is not None}
    gmax = max(v.abs().max().item() for v in grads.values())
    diffs = sorted(((grads[k] - grads_graph[k]).abs().max().item() / gmax, k) for k in grads if k in grads_graph)
    worst = diffs[-1] if diffs else (0.0, "-")
    nonzero = [(d, k) for d, k in diffs if d > 0]
    print(f"eager against graph, fp32, same key: largest gradient difference {worst[0]:.3e} of the largest gradient ({worst[1]}); "
          f"{len(nonzero)} of {len(diffs)} tensors differ")
    for d, k in nonzero[-8:][::-1]:
        print(f"    {k}: {d:.3e}")
    for d, k in nonzero[:4]:
        print(f"    (smallest) {k}: {d:.3e}")


def train2x(bf16, dev):
    batch = train_batch(dev)
    bad = []
    sampler = sampler_at(dev)
    net, drv = make(dev, bf16, sampler)
    rng_build = torch.cuda.get_rng_state().clone()
    graphed = GraphedTrainStep(net, drv.optimizer, batch, scheduler=drv.scheduler, warmup=2, draws=sampler)
    if sampler.get_state() != (SEED, CALL):
        bad.append(f"building moved the sampler to {sampler.get_state()}")
    rng0 = torch.cuda.get_rng_state().clone()
    if not torch.equal(rng_build, rng0):
        bad.append("torch's device generator moved across the build (a draw in the warm-up or the capture that the key does not cover)")
    ckpt = copy.deepcopy(drv.checkpoint(1, 0))
    first = steps(graphed, sampler, 3)
    drv.load_checkpoint(ckpt)
    if sampler.get_state() != (SEED, CALL):
        bad.append(f"load_checkpoint left the sampler at {sampler.get_state()}")
    second = steps(graphed, sampler, 3)
    if not torch.equal(rng0, torch.cuda.get_rng_state()):
        bad.append("torch's device generator moved across the steps (a draw inside the replay that the key does not cover)")
    compare(bad, "second run", first, second)
    if all(torch.equal(first["loss"][0][k], first["loss"][1][k]) for k in first["loss"][0]):
        bad.append("steps 1 and 2 computed the same losses: the steps do not advance")
    if all(torch.equal(v, ckpt["posenet_state_dict"][k].to(dev)) for k, v in first["params"].items()):
        bad.append("three steps left the parameters where they were")
    print(f"train2x {'bf16' if bf16 else 'f32'}: total loss of step 3 {float(graphed.total.detach()):.6f}; {len(bad)} mismatches")
    if not bf16:
        eager_figure(dev, batch, first["grads_first"])
    return bad


def resume(dev):
    batch = train_batch(dev)
    bad = []
    sampler = sampler_at(dev)
    net, drv = make(dev, False, sampler)
    graphed = GraphedTrainStep(net, drv.optimizer, batch, scheduler=drv.scheduler, warmup=2, draws=sampler)
    steps(graphed, sampler, 1)
    ckpt = copy.deepcopy(drv.checkpoint(1, 0))
    if ckpt.get("draws") != (SEED, CALL + 1):
        bad.append(f"checkpoint['draws'] is {ckpt.get('draws')!r}")
    whole = steps(graphed, sampler, 2)                                           # steps 2-3 of the uninterrupted run

    sampler2 = DeviceSampler(999, dev)                                           # "a new process": everything starts elsewhere
    net2, drv2 = make(dev, False, sampler2, init_seed=1)
    drv2.load_checkpoint(ckpt)
    graphed2 = GraphedTrainStep(net2, drv2.optimizer, {k: v.clone() for k, v in batch.items()}, scheduler=drv2.scheduler, warmup=2,
                                draws=sampler2)
    if sampler2.get_state() != (SEED, CALL + 1):
        bad.append(f"the resumed sampler is at {sampler2.get_state()}")
    resumed = steps(graphed2, sampler2, 2)
    compare(bad, "resumed run", whole, resumed)
    print(f"resume: total loss of step 3 {float(graphed.total.detach()):.6f} / resumed {float(graphed2.total.detach()):.6f}; "
          f"{len(bad)} mismatches")
    return bad


def main():
    mode = sys.argv[1]
    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.reproducible = True
    run = {"train2x_f32": lambda: train2x(False, dev), "train2x_bf16": lambda: train2x(True, dev), "resume": lambda: resume(dev)}
    if mode not in run:
        raise SystemExit(f"unknown mode {mode}")
    bad = run[mode]()
    for line in bad[:30]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
