"""Run by test_gpu_scene.py in a fresh process (a capture must precede the network's first eager backward):
usage: python tests/_rendered_train_check.py mode        (tests/_frame_train_check.py's frame and network sizes, M = 6, keep = 4)

mode twin: three steps of ``train.RenderedTrainStep`` on one network, of a second one built from an equal sampler state on a
  second network, and of a ``FrameTrainStep(draws='device')`` on a third that is ``load``ed, before each run, with what
  ``SceneSource.draw`` returns eagerly under the key that run will use (its boxes from ``bboxes_d.cpu()``, none of them empty):
  ``batch``, ``sel``, ``info`` and ``status`` are equal bit for bit at every step -- the rendered step is the existing step fed
  the same scene, and nothing else.  numpy's and torch's CPU generator states are what they were before anything was built; the
  losses are finite and the parameters move.
mode occluded: every item inside a sphere that hides it, ``apply='graph'``: ``run(check=False)`` leaves the parameters and the
  optimizer state bit-unchanged, info == [0, 0] and ``skipped_no_item`` counts the batch.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _frame_train_check as fc
from hs_pose_amd.config import FLAGS
from hs_pose_amd.pc_sample import DeviceSampler
from hs_pose_amd.render import MeshSet, SceneSource, shapes
from hs_pose_amd.train import FrameTrainStep, RenderedTrainStep

M, KEEP, N, SEED = 6, 4, 256, 21


def source(dev, hidden=False):
    ms = MeshSet([shapes.box(), shapes.uv_sphere(8, 6)], device=dev)
    dist = [dict(mesh=0, size=(0.6, 0.02, 0.6), rest=True)]
    if hidden:                      # a sphere of 1 m around every item (largest side <= 0.2 m), the camera >= 1.3 m away, outside it
        dist.append(dict(mesh=1, size=(1.0, 1.0, 1.0)))
    return SceneSource(ms, [0, 3], [[0.1, 0.1, 0.1], [0.12, 0.12, 0.12]], np.zeros((2, 4)), fc.K, fc.H, fc.W,
                       distance=(1.3, 1.6) if hidden else (0.8, 1.2), size=(0.1, 0.2), n_model=128, distractors=dist)


def setup():
    fc.setup()
    FLAGS.reproducible = True
    FLAGS.step_draws = "device"


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def state_of(step):
    out = {f"batch.{k}": v.clone() for k, v in step.batch.items()}
    out.update(sel=step.sel.clone(), info=step.info.clone(), status=step.status.clone())
    return out


def twin(dev):
    kw = dict(n_pts=N, out_size=fc.O, warmup=2)
    nets = [fc.make(dev, False) for _ in range(3)]
    rng_before = (np.random.get_state(), torch.get_rng_state().clone())
    first = {k: p.detach().clone() for k, p in nets[0][0].named_parameters()}
    a, b = (RenderedTrainStep(net, drv.optimizer, source(dev), M, KEEP, scheduler=drv.scheduler, sampler=DeviceSampler(SEED, dev), **kw)
            for net, drv in nets[:2])
    eager = source(dev)
    key = torch.tensor([SEED, 0], dtype=torch.int64, device=dev)
    frames, items = eager.draw(M, key)
    host = lambda fr: dict(fr, bboxes_xyxy=fr["bboxes_d"].cpu().numpy())
    c = FrameTrainStep(nets[2][0], nets[2][1].optimizer, host(frames), items, KEEP, scheduler=nets[2][1].scheduler,
                       sampler=DeviceSampler(SEED, dev), draws="device", **kw)
    bad = []
    for step in range(3):
        key[1] = step
        frames, items = eager.draw(M, key)
        counts = eager.last["count"].cpu().tolist()
        if min(counts) <= 0:
            bad.append(f"step {step}: an empty box (counts {counts}): the seed does not make the intended case")
        c.load(frames=host(frames), items=items)
        answers = [s.run() for s in (a, b, c)]
        torch.cuda.synchronize()
        sa, sb, sc = state_of(a), state_of(b), state_of(c)
        for name, other in (("its twin", sb), ("the frame step fed the same scene", sc)):
            diff = [k for k in sa if k not in other or not same(sa[k], other[k])]
            if diff or set(sa) != set(other):
                bad.append(f"step {step}: differs from {name} in {diff}")
        if answers != [True] * 3 or not bool(torch.isfinite(a.total)):
            bad.append(f"step {step}: run() answered {answers}, total loss {float(a.total.detach())}")
        print(f"step {step}: counts {counts} status {a.status.cpu().tolist()} sel {a.sel.cpu().tolist()} info {a.info.cpu().tolist()} "
              f"total loss {float(a.total.detach()):.6f} / {float(b.total.detach()):.6f} / {float(c.total.detach()):.6f}")
        if a.info.cpu().tolist()[0] < 1:
            bad.append(f"step {step}: no good item")
    if not any(not torch.equal(p, first[k]) for k, p in nets[0][0].named_parameters()):
        bad.append("the parameters did not move")
    rng_after = (np.random.get_state(), torch.get_rng_state())
    if not (rng_before[0][0] == rng_after[0][0] and np.array_equal(rng_before[0][1], rng_after[0][1]) and
            rng_before[0][2:] == rng_after[0][2:] and torch.equal(rng_before[1], rng_after[1])):
        bad.append("a host generator moved")
    return bad


def occluded(dev):
    net, drv = fc.make(dev, False)
    step = RenderedTrainStep(net, drv.optimizer, source(dev, hidden=True), M, KEEP, scheduler=drv.scheduler,
                             sampler=DeviceSampler(SEED, dev), n_pts=N, out_size=fc.O, warmup=2, apply="graph")
    flat = drv.optimizer._flat[0]
    before = {k: getattr(flat, k).clone() for k in ("flat_p", "flat_m", "flat_v", "flat_s")}
    res = step.run(check=False)
    torch.cuda.synchronize()
    bad = [f"{k} changed across an all-occluded batch" for k, v in before.items() if not torch.equal(v, getattr(flat, k))]
    if res is not True:
        bad.append(f"run(check=False) answered {res!r}")
    if step.info.cpu().tolist() != [0, 0] or step.scene["count"].cpu().tolist() != [0] * M \
            or step.bboxes_d.cpu().tolist() != [[0, 0, 1, 1]] * M or not bool(torch.isfinite(step.xf).all()):
        bad.append(f"info {step.info.cpu().tolist()} counts {step.scene['count'].cpu().tolist()} boxes {step.bboxes_d.cpu().tolist()}")
    if not bool((step.status != 0).all()) or not bool(torch.isfinite(step.total)):
        bad.append(f"status {step.status.cpu().tolist()}, total loss {float(step.total.detach())}")
    c = drv.optimizer.sync_clock()
    want = dict(applied=0, replays=1, skipped_nan=0, skipped_no_item=1, exhausted=0)
    if {k: c[k] for k in want} != want:
        bad.append(f"counters {c}, expected {want}")
    print(f"occluded: info {step.info.cpu().tolist()} status {step.status.cpu().tolist()} counters {c}; {len(bad)} mismatches")
    return bad


def main():
    mode = sys.argv[1]
    dev = torch.device("cuda:0")
    setup()
    bad = {"twin": twin, "occluded": occluded}[mode](dev)
    for line in bad[:20]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
