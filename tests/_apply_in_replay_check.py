"""Run by test_gpu_apply_in_replay.py in a fresh process (a capture must precede the network's first eager backward):
usage: python tests/_apply_in_replay_check.py mode        (B = 4, N = 256; frames: M = 6, keep = 4, N = 256)

``apply='graph'``: the gate, the schedule and the Ranger launch inside the training step's replay.  ``FLAGS.reproducible`` on and
device draws under one ``DeviceSampler``, where two runs from one seed agree bit for bit: the runs compared below
differ only in WHO applies the step.

twin      two identically seeded networks and samplers, A ``apply='host'`` driven with ``run(check_nan=True)``, B
          ``apply='graph'`` driven with ``run()``; eight replays in the schedule's warm-up (another learning rate every step),
          replay 3 on a NaN ``gt_t``.  Parameters, exp_avg, exp_avg_sq and slow_buffer bit-equal; B's counters applied 7, replays
          8, skipped_nan 1; after ``sync_clock()`` B's step counts, ``scheduler.last_epoch`` and group lr are A's.
skip      one NaN replay on ``apply='graph'``: parameters and optimizer state bit-unchanged, a BatchNorm's
          ``num_batches_tracked`` has advanced.
rejected  ``FrameTrainStep(apply='graph')`` on the all-absent batch of tests/_frame_train_check.py with ``run(check=False)``:
          parameters bit-unchanged, info[0] == 0, skipped_no_item == 1.
unarmed   right after construction: parameters, optimizer state and BatchNorm buffers equal a twin on which nothing was built,
          every counter is 0.
resume    four replays, ``TrainDriver.checkpoint``, loaded into a fresh twin built with ``apply='graph'``, four more: bit-equal to
          eight uninterrupted replays.
calls     building the graph form issues ``hsp_step_gate`` and ``hsp_ranger_step_gated`` and never ``hsp_ranger_step``; a
          ``run()`` issues no C-ABI call from Python.
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import torch

import _reproducible_step_check as rs
from hs_pose_amd import _lib, ops
from hs_pose_amd.config import FLAGS
from hs_pose_amd.graph import GraphedTrainStep
from hs_pose_amd.pc_sample import DeviceSampler

STATE = (("params", "flat_p"), ("exp_avg", "flat_m"), ("exp_avg_sq", "flat_v"), ("slow_buffer", "flat_s"))


def build(dev, apply, init_seed=0, sampler=None, **kw):
    sampler = rs.sampler_at(dev) if sampler is None else sampler
    net, drv = rs.make(dev, False, sampler, init_seed)
    graphed = GraphedTrainStep(net, drv.optimizer, rs.train_batch(dev), scheduler=drv.scheduler, warmup=2, draws=sampler,
                               apply=apply, **kw)
    return net, drv, sampler, graphed


def snapshot(net, drv):
    out = {name: getattr(fg, attr).detach().clone() for name, attr in STATE for fg in drv.optimizer._flat[:1]}
    out.update({"buffer " + k: b.detach().clone() for k, b in net.named_buffers()})
    return out


def differences(what, a, b, keys=None):
    bad = []
    for k in (keys if keys is not None else a):
        same = torch.equal(a[k], b[k])
        if not same and k.startswith("buffer ") and a[k].is_floating_point():
            # a NaN replay leaves NaN running statistics behind in BOTH forms (the forward ran, as the reference's does before its
            # NaN test): NaN where the other has NaN is agreement.  Parameters and optimizer state are compared strictly.
            same = bool(((a[k] == b[k]) | (torch.isnan(a[k]) & torch.isnan(b[k]))).all())
        if not same:
            x, y = a[k].double(), b[k].double()
            bad.append(f"{what}: {k} differ in {int((a[k] != b[k]).sum())} of {a[k].numel()} elements, max |diff| "
                       f"{(x - y).abs().max().item():.3e}")
    return bad


def nan_batch(graphed):
    """a NaN gt_t into the static batch; returns the value to put back"""
    keep = graphed.batch["gt_t"].clone()
    graphed.load_batch({"gt_t": torch.full_like(keep, float("nan"))})
    return keep


def run_steps(graphed, sampler, n, nan_at=(), **run_kw):
    res = []
    for i in range(n):
        keep = nan_batch(graphed) if i in nan_at else None
        sampler.advance()
        res.append(graphed.run(**run_kw))
        if keep is not None:
            graphed.load_batch({"gt_t": keep})
    torch.cuda.synchronize()
    return res


def twin(dev):
    net_a, drv_a, sa, A = build(dev, "host")
    net_b, drv_b, sb, B = build(dev, "graph")
    bad = differences("before the first step", snapshot(net_a, drv_a), snapshot(net_b, drv_b))
    start = drv_b.optimizer._flat[0].flat_p.detach().clone()
    res_a =run_steps(A, sa, 8, nan_at=(2,), check_nan=True)
    res_b = run_steps(B, sb, 8, nan_at=(2,))
    if res_a != [True, True, False] + [True] * 5:
        bad.append(f"the host form's NaN check answered {res_a}: the NaN gt_t did not make the intended case")
    if res_b != [True] * 8:
        bad.append(f"the graph form's run() answered {res_b}")
    flags = B.clock.tables_host[0]["flags"][:7].tolist()
    if not (any(not f & _lib.STEP_ADAPTIVE for f in flags) and any(f & _lib.STEP_ADAPTIVE for f in flags)
            and any(f & _lib.STEP_LOOKAHEAD for f in flags) and flags[0] & _lib.STEP_FILL_SLOW):
        bad.append(f"the seven applied entries {flags} do not cross the plain->adaptive edge, a Lookahead step and the slow fill")
    lrs = B.clock.tables_host[0]["step_lr"][:7].tolist()
    if len(set(lrs)) != 7:
        bad.append(f"step_lr does not differ every step: {lrs}")
    bad += differences("after 8 replays", snapshot(net_a, drv_a), snapshot(net_b, drv_b))
    before = {k: drv_b.optimizer.state[p]["step"] for k, p in net_b.named_parameters()}
    if set(before.values()) != {0} or drv_b.scheduler.last_epoch != 0:
        bad.append("the graph form moved a host counter before sync_clock()")
    c = drv_b.optimizer.sync_clock()
    want = dict(armed=1, applied=7, replays=8, skipped_nan=1, skipped_no_item=0, exhausted=0)
    if {k: c[k] for k in want} != want:
        bad.append(f"counters {c}, expected {want}")
    steps_a = [drv_a.optimizer.state[p]["step"] for p in net_a.parameters()]
    steps_b = [drv_b.optimizer.state[p]["step"] for p in net_b.parameters()]
    if steps_a != steps_b or set(steps_a) != {7}:
        bad.append(f"step counts after sync_clock: host form {set(steps_a)}, graph form {set(steps_b)}")
    if drv_a.scheduler.last_epoch != drv_b.scheduler.last_epoch or drv_a.scheduler.last_epoch != 7:
        bad.append(f"last_epoch: host form {drv_a.scheduler.last_epoch}, graph form {drv_b.scheduler.last_epoch}")
    lr_a, lr_b = [g["lr"] for g in drv_a.optimizer.param_groups], [g["lr"] for g in drv_b.optimizer.param_groups]
    if lr_a != lr_b or drv_a.scheduler.get_last_lr() != drv_b.scheduler.get_last_lr():
        bad.append(f"group lr: host form {lr_a}, graph form {lr_b}")
    if not all(fg.slow_ready for fg in drv_b.optimizer._flat):
        bad.append("slow_ready is not set after sync_clock")
    if torch.equal(drv_b.optimizer._flat[0].flat_p, start):
        bad.append("seven applied steps left the parameters where they were")
    print(f"twin: host form answered {res_a}; counters {c}; lr {lr_b}; {len(bad)} mismatches")
    return bad


def skip(dev):
    net, drv, sampler, G = build(dev, "graph")
    before = snapshot(net, drv)
    tracked = {k: int(b) for k, b in net.named_buffers() if k.endswith("num_batches_tracked")}
    res = run_steps(G, sampler, 1, nan_at=(0,), check_nan=True)
    after = snapshot(net, drv)
    bad = differences("across a NaN replay", before, after, keys=[n for n, _ in STATE])
    if res != [False]:
        bad.append(f"run(check_nan=True) answered {res} on a NaN loss")
    if not bool(torch.isnan(G.total)):
        bad.append(f"the total loss is {float(G.total)!r}: the NaN gt_t did not make the intended case")
    now = {k: int(b) for k, b in net.named_buffers() if k.endswith("num_batches_tracked")}
    if not any(now[k] == v + 1 for k, v in tracked.items()) or not all(now[k] in (v, v + 1) for k, v in tracked.items()):
        bad.append(f"num_batches_tracked went {sorted(set(tracked.values()))} -> {sorted(set(now.values()))}: the forward did not run once")
    c = G.clock.read()
    want = dict(applied=0, replays=1, skipped_nan=1, skipped_no_item=0, exhausted=0, apply=0)
    if {k: c[k] for k in want} != want:
        bad.append(f"counters {c}, expected {want}")
    try:
        G.apply()
        bad.append("apply() did not raise on the graph form")
    except RuntimeError:
        pass
    try:
        drv.optimizer.step()
        bad.append("Ranger.step() did not raise with a device clock attached")
    except RuntimeError:
        pass
    # and the step that follows is applied: the skip left nothing behind
    res = run_steps(G, sampler, 1, check_nan=True)
    if res != [True] or torch.equal(before["params"], drv.optimizer._flat[0].flat_p):
        bad.append(f"the finite replay after the skip answered {res} or left the parameters where they were")
    print(f"skip: counters {c}; {len(bad)} mismatches")
    return bad


def rejected(dev):
    import _frame_train_check as fc
    from hs_pose_amd.train import FrameTrainStep
    M, keep, N = 6, 4, 256
    fc.setup()
    FLAGS.reproducible = True
    FLAGS.step_draws = "device"
    net, drv = fc.make(dev, False)
    step = FrameTrainStep(net, drv.optimizer, fc.frames(M, dev, all_absent=True), fc.items_of(M, N, dev), keep,
                          scheduler=drv.scheduler, sampler=DeviceSampler(21, dev), n_pts=N, out_size=fc.O, warmup=2, apply="graph")
    before = snapshot(net, drv)
    res = step.run(check=False)
    torch.cuda.synchronize()
    bad = differences("across an all-rejected batch", before, snapshot(net, drv), keys=[n for n, _ in STATE])
    if res is not True:
        bad.append(f"run(check=False) answered {res!r}")
    if step.info.cpu().tolist() != [0, 0]:
        bad.append(f"info {step.info.cpu().tolist()}")
    if not bool(torch.isfinite(step.total)):
        bad.append("the loss on the stand-in cloud is not finite: the skip would be the NaN rule's, not the item rule's")
    c = drv.optimizer.sync_clock()
    want = dict(applied=0, replays=1, skipped_nan=0, skipped_no_item=1, exhausted=0)
    if {k: c[k] for k in want} != want:
        bad.append(f"counters {c}, expected {want}")
    if step.run(check=True) is not False:
        bad.append("run(check=True) did not report the device's skip")
    print(f"rejected: info {step.info.cpu().tolist()}, total loss {float(step.total.detach()):.6f}, counters {c}; {len(bad)} mismatches")
    return bad


def unarmed(dev):
    net_a, drv_a, _, G = build(dev, "graph")
    net_b, drv_b = rs.make(dev, False, rs.sampler_at(dev))
    torch.cuda.synchronize()
    bad = differences("after construction", snapshot(net_a, drv_a), snapshot(net_b, drv_b))
    c = G.clock.ctl.cpu().tolist()
    if c != [1] + [0] * 15:
        bad.append(f"control block {c} after construction")
    print(f"unarmed: control block {c}; {len(bad)} mismatches")
    return bad


def resume(dev):
    net, drv, sampler, G = build(dev, "graph")
    run_steps(G, sampler, 4)
    ckpt = copy.deepcopy(drv.checkpoint(1, 0))
    bad = []
    st = ckpt["optimizer"]["state"]
    if ckpt["scheduler"]["last_epoch"] != 4 or {s["step"] for s in st.values()} != {4}:
        bad.append(f"the checkpoint holds last_epoch {ckpt['scheduler']['last_epoch']} and steps { {s['step'] for s in st.values()} }")
    run_steps(G, sampler, 4)
    whole = snapshot(net, drv)

    net2, drv2, sampler2, G2 = build(dev, "graph", init_seed=1, sampler=DeviceSampler(999, dev))
    drv2.load_checkpoint(ckpt)
    if G2.clock.step0 != [4] or G2.clock.epoch0 != 4 or G2.clock.ctl.cpu().tolist()[:4] != [1, 0, 0, 0]:
        bad.append(f"the resumed clock starts at step {G2.clock.step0}, epoch {G2.clock.epoch0}, block {G2.clock.ctl.cpu().tolist()[:8]}")
    run_steps(G2, sampler2, 4)
    bad += differences("resumed against uninterrupted", whole, snapshot(net2, drv2))
    c, c2 = drv.optimizer.sync_clock(), drv2.optimizer.sync_clock()
    if c["applied"] != 8 or c2["applied"] != 4 or drv.scheduler.last_epoch != 8 or drv2.scheduler.last_epoch != 8:
        bad.append(f"applied {c['applied']} / {c2['applied']}, last_epoch {drv.scheduler.last_epoch} / {drv2.scheduler.last_epoch}")
    print(f"resume: counters {c} / resumed {c2}; {len(bad)} mismatches")
    return bad


def calls(dev):
    names, real = [], ops._run

    def run(name, args, **k):
        names.append(name)
        return real(name, args, **k)
    ops._run = run
    try:
        net, drv, sampler, G = build(dev, "graph")
        built = list(names)
        del names[:]
        sampler.advance()
        G.run()
        torch.cuda.synchronize()
        ran = list(names)
    finally:
        ops._run = real
    bad = []
    if built.count("hsp_step_gate") != 3 or built.count("hsp_ranger_step_gated") != 3 or "hsp_ranger_step" in built:
        bad.append(f"build (2 warm-up runs + the capture): hsp_step_gate x{built.count('hsp_step_gate')}, hsp_ranger_step_gated "
                   f"x{built.count('hsp_ranger_step_gated')}, hsp_ranger_step x{built.count('hsp_ranger_step')}")
    if ran:
        bad.append(f"run() issued {ran}")
    if G.clock.read()["applied"] != 1:
        bad.append("the run applied no step")
    print(f"calls: build {len(built)} calls, run {ran}; {len(bad)} mismatches")
    return bad


def main():
    mode = sys.argv[1]
    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.reproducible = True
    FLAGS.step_draws = "device"
    run = dict(twin=twin, skip=skip, rejected=rejected, unarmed=unarmed, resume=resume, calls=calls)
    if mode not in run:
        raise SystemExit(f"unknown mode {mode}")
    bad = run[mode](dev)
    for line in bad[:30]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
