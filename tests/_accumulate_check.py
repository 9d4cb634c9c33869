"""Run by test_gpu_accumulate.py in a fresh process (a capture must precede the network's first eager backward):
usage: python tests/_accumulate_check.py mode        (B = 4, N = 256; frames: M = 6, keep = 4, N = 256)

Gradient accumulation in the graphed training step (``accumulate=``), on the harness of tests/_apply_in_replay_check.py:
``FLAGS.reproducible`` on and device draws under one ``DeviceSampler``, where two runs from one seed agree bit for bit.  Eight replays,
``accumulate = 3`` from ``global_step = 0``: slots 0, 3 and 6 step; replays 3 (a stepping slot) and 4 run on a NaN ``gt_t``.

manual    the independent oracle.  B is ``apply='graph', accumulate=3``.  The twin A is an ordinary ``accumulate=1, apply='host'``
          object on an identically seeded network, driven with ``replay()`` only; after each replay this file does the reference's
          arithmetic itself with pieces that existed before: A's ``flat_g`` added (torch fp32) into an accumulator of its own,
          ``clip_grad_norm_`` on it, then ``step()`` / ``scheduler.step()`` / zero on a stepping slot, ``scale_grads_by_clip_()`` on any
          other taken slot.  Run 1, ``max_norm = 1e30`` (every coefficient exactly 1): parameters, exp_avg, exp_avg_sq, slow_buffer,
          buffers and ``accumulated_grads()`` bit-equal after every replay.  Run 2, ``max_norm`` = half the twin's first
          accumulate-only norm of run 1: at least one accumulate-only coefficient is below 1; everything bit-equal before the first
          scaled slot, the optimizer state bit-equal up to the first stepping slot after it, and from the scaled slot to that
          stepping slot the accumulator within |diff| <= (accumulate - 1) * 2^-22 * max|acc| (torch's ``reciprocal() * max_norm``
          against the kernel's division: one ulp of c, plus one rounding per scaling); the measured figure is printed.
twin      A ``apply='host', accumulate=3`` with ``run(check_nan=True)``, B ``apply='graph', accumulate=3``: everything bit-equal; B's
          counters replays 8, skipped_nan 2, applied 2, micro 8, pending as ``_accum_ref`` says; after ``sync_clock()`` step counts,
          ``last_epoch`` and learning rates are A's.
k1        ``accumulate=1`` passed explicitly, in both forms: bit-equal to the default object over four replays, the same C-ABI call
          list, neither new entry in it.
resume    ``accumulate=3`` from ``global_step=1`` (from 0 four replays end on a stepping slot and nothing would be pending): four
          replays, ``TrainDriver.checkpoint`` (it has 'accum'), loaded into a fresh twin built with the same arguments, four more:
          bit-equal to eight uninterrupted replays.
frames    ``FrameTrainStep(apply='graph', accumulate=2)`` from ``global_step=1``: a good batch, the all-absent batch of
          tests/_frame_train_check.py, two good batches.  Across the all-absent slot accumulator, norm scalar and parameters are
          bit-unchanged, ``skipped_no_item == 1`` and ``micro`` advanced.
bf16      ``twin`` under ``set_feature_dtype(torch.bfloat16)``.
calls     building the graph form with ``accumulate=3`` issues ``hsp_step_gate_accum``, ``hsp_grad_accumulate`` and
          ``hsp_ranger_step_gated`` and never ``hsp_step_gate``, ``hsp_sumsq_f32`` or ``hsp_ranger_step``; a ``run()`` issues no C-ABI
          call from Python.
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _accum_ref as R
import _apply_in_replay_check as ar
import _reproducible_step_check as rs
from _apply_in_replay_check import STATE, differences, nan_batch, run_steps, snapshot
from hs_pose_amd import ops
from hs_pose_amd.config import FLAGS
from hs_pose_amd.graph import GraphedTrainStep
from hs_pose_amd.pc_sample import DeviceSampler

ACC, NAN_AT, REPLAYS = 3, (3, 4), 8
EVENTS = [R.NAN if i in NAN_AT else R.OK for i in range(REPLAYS)]


def build(dev, apply, bf16=False, init_seed=0, sampler=None, **kw):
    if not bf16:
        return ar.build(dev, apply, init_seed=init_seed, sampler=sampler, **kw)
    sampler = rs.sampler_at(dev) if sampler is None else sampler
    net, drv = rs.make(dev, True, sampler, init_seed)
    graphed = GraphedTrainStep(net, drv.optimizer, rs.train_batch(dev), scheduler=drv.scheduler, warmup=2, draws=sampler,
                               apply=apply, **kw)
    return net, drv, sampler, graphed


def with_grads(net, drv):
    """``snapshot`` and the accumulated gradients, one flat tensor"""
    out = snapshot(net, drv)
    out["accumulated_grads"] = torch.cat([g.reshape(-1) for g in drv.optimizer.accumulated_grads()])
    return out


def one_replay(graphed, sampler, i, fn):
    keep = nan_batch(graphed) if i in NAN_AT else None
    sampler.advance()
    res = fn()
    if keep is not None:
        graphed.load_batch({"gt_t": keep})
    return res


def manual_run(dev, max_norm, exact):
    net_a, drv_a, sa, A = build(dev, "host", max_norm=max_norm)
    net_b, drv_b, sb, B = build(dev, "graph", max_norm=max_norm, accumulate=ACC)
    opt, sched = drv_a.optimizer, drv_a.scheduler
    fg, fg_b = opt._flat[0], drv_b.optimizer._flat[0]
    acc = torch.zeros_like(fg.flat_g)
    bad, norms, coefs, figures = [], {}, {}, []
    scaled_at = None                                           # the first taken slot that left a coefficient < 1 pending
    bound_unit = (ACC - 1) * 2.0 ** -22
    for i in range(REPLAYS):
        one_replay(A, sa, i, A.replay)
        one_replay(B, sb, i, B.run)
        torch.cuda.synchronize()
        if bool(torch.isnan(A.total)) != (i in NAN_AT):
            bad.append(f"replay {i}: the twin's loss is {float(A.total)!r}: the NaN gt_t did not make the intended case")
        stepping = i % ACC == 0
        raw = None
        if i not in NAN_AT:                                    # engine/train.py:104-114 on the twin, by hand
            acc.add_(fg.flat_g)                                # (flat_g holds the replay's fresh gradient)
            fg.flat_g.copy_(acc)
            norm = float(opt.clip_grad_norm_(max_norm))
            norms[i], coefs[i] = norm, min(1.0, max_norm / (norm + 1e-6))
            if stepping:
                raw = acc.clone()
                opt.step()
                sched.step()
                acc.zero_()
            else:
                opt.scale_grads_by_clip_()
                acc.copy_(fg.flat_g)
                if coefs[i] < 1.0 and scaled_at is None:
                    scaled_at = i
        sa_, sb_ = snapshot(net_a, drv_a), snapshot(net_b, drv_b)
        got = torch.cat([g.reshape(-1) for g in drv_b.optimizer.accumulated_grads()])
        want = torch.cat([fg.view(acc, p, o).reshape(-1) for p, o in zip(fg.params, fg.offsets)])
        if exact or scaled_at is None:
            bad += differences(f"replay {i}", sa_, sb_)
            if not torch.equal(got, want):
                bad.append(f"replay {i}: accumulated_grads differ in {int((got != want).sum())} elements, max |diff| "
                           f"{(got.double() - want.double()).abs().max().item():.3e}")
            continue
        # from the first scaled slot on: the coefficient may differ by one ulp between torch and the kernel
        if stepping and raw is not None:                       # the first stepping slot after it: the accumulator the step consumed
            diff = (fg_b.flat_g.double() - raw.double()).abs().max().item()
            top = raw.abs().max().item()
            figures.append((i, diff, top))
            if not diff <= bound_unit * top:
                bad.append(f"replay {i} (stepping): |acc diff| {diff:.3e} exceeds {bound_unit:.3e} * max|acc| {top:.3e}")
            break
        bad += differences(f"replay {i}", sa_, sb_)            # (nothing was applied since: still bit-equal)
        diff, top = (got.double() - want.double()).abs().max().item(), want.abs().max().item()
        figures.append((i, diff, top))
        if not diff <= bound_unit * top:
            bad.append(f"replay {i}: |acc diff| {diff:.3e} exceeds {bound_unit:.3e} * max|acc| {top:.3e}")
    c = drv_b.optimizer.sync_clock()
    return bad, norms, coefs, figures, scaled_at, c


def manual(dev):
    bad, norms, coefs, _, _, c = manual_run(dev, 1e30, exact=True)
    if set(coefs.values()) != {1.0}:
        bad.append(f"max_norm 1e30: coefficients {coefs}")
    want = R.decisions(ACC, 0, EVENTS, 1000)[-1]
    if {k: c[k] for k in ("applied", "skipped_nan", "micro", "pending")} != {k: want[k] for k in ("applied", "skipped_nan", "micro", "pending")}:
        bad.append(f"counters {c}, expected {want}")
    print(f"manual, max_norm 1e30: twin norms {norms}; counters {c}; {len(bad)} mismatches")
    max_norm = 0.5 * norms[1]                                  # half the twin's first accumulate-only norm
    bad2, norms2, coefs2, figures, scaled_at, _ = manual_run(dev, max_norm, exact=False)
    only = {i: v for i, v in coefs2.items() if i % ACC}
    if not any(v < 1.0 for v in only.values()) or scaled_at is None:
        bad2.append(f"max_norm {max_norm}: no accumulate-only coefficient below 1 ({only}): the case was not made")
    if not figures or figures[-1][0] % ACC:
        bad2.append(f"max_norm {max_norm}: the run never reached the stepping slot after the scaled one ({figures})")
    print(f"manual, max_norm {max_norm:.6g}: twin norms {norms2}; coefficients {coefs2}; first scaled slot {scaled_at}; "
          f"{len(bad2)} mismatches")
    for i, diff, top in figures:
        print(f"    replay {i}: max |acc diff| {diff:.3e} = {diff / top / 2.0 ** -22 if top else 0.0:.3f} * 2^-22 * max|acc| "
              f"(max|acc| {top:.3e}; bound {ACC - 1} * 2^-22)")
    return bad + bad2


def twin(dev, bf16=False):
    net_a, drv_a, sa, A = build(dev, "host", bf16=bf16, accumulate=ACC)
    net_b, drv_b, sb, B = build(dev, "graph", bf16=bf16, accumulate=ACC)
    bad = differences("before the first step", snapshot(net_a, drv_a), snapshot(net_b, drv_b))
    start = drv_b.optimizer._flat[0].flat_p.detach().clone()
    res_a, res_b = [], []
    dec = R.decisions(ACC, 0, EVENTS, 1000)
    for i in range(REPLAYS):
        res_a.append(one_replay(A, sa, i, lambda: A.run(check_nan=True)))
        res_b.append(one_replay(B, sb, i, B.run))
        torch.cuda.synchronize()
        bad += differences(f"replay {i}", with_grads(net_a, drv_a), with_grads(net_b, drv_b))
        if drv_a.optimizer._accum.counts() != (dec[i]["micro"], dec[i]["pending"]):
            bad.append(f"replay {i}: the host form counts (micro, pending) = {drv_a.optimizer._accum.counts()}, expected {dec[i]}")
    if res_a != [i not in NAN_AT for i in range(REPLAYS)]:
        bad.append(f"the host form's NaN check answered {res_a}")
    if res_b != [True] * REPLAYS:
        bad.append(f"the graph form's run() answered {res_b}")
    if set(drv_b.optimizer.state[p]["step"] for p in net_b.parameters()) != {0} or drv_b.scheduler.last_epoch != 0:
        bad.append("the graph form moved a host counter before sync_clock()")
    c = drv_b.optimizer.sync_clock()
    want = dict(armed=1, replays=8, skipped_nan=2, skipped_no_item=0, applied=2, exhausted=0, micro=8, pending=dec[-1]["pending"],
                take=dec[-1]["take"], first=dec[-1]["first"], apply=dec[-1]["apply"])
    if {k: c[k] for k in want} != want or dec[-1]["pending"] != 1:
        bad.append(f"counters {c}, expected {want}")
    steps_a = {drv_a.optimizer.state[p]["step"] for p in net_a.parameters()}
    steps_b = {drv_b.optimizer.state[p]["step"] for p in net_b.parameters()}
    if steps_a != steps_b or steps_a != {2}:
        bad.append(f"step counts after sync_clock: host form {steps_a}, graph form {steps_b}")
    if drv_a.scheduler.last_epoch != drv_b.scheduler.last_epoch or drv_a.scheduler.last_epoch != 2:
        bad.append(f"last_epoch: host form {drv_a.scheduler.last_epoch}, graph form {drv_b.scheduler.last_epoch}")
    lr_a, lr_b = [g["lr"] for g in drv_a.optimizer.param_groups], [g["lr"] for g in drv_b.optimizer.param_groups]
    if lr_a != lr_b or drv_a.scheduler.get_last_lr() != drv_b.scheduler.get_last_lr():
        bad.append(f"group lr: host form {lr_a}, graph form {lr_b}")
    if torch.equal(drv_b.optimizer._flat[0].flat_p, start):
        bad.append("two applied steps left the parameters where they were")
    if not bool(drv_b.optimizer._flat[0].flat_g.abs().sum() > 0) or not bool(torch.isfinite(drv_b.optimizer._accum.norm_sq).all()):
        bad.append("the accumulator is empty or its norm is not finite after a taken slot")
    print(f"twin{' bf16' if bf16 else ''}: host form answered {res_a}; counters {c}; lr {lr_b}; {len(bad)} mismatches")
    return bad


def record(fn):
    """(fn's result, the C-ABI entry points Python called meanwhile)"""
    names, real = [], ops._run

    def run(name, args, **k):
        names.append(name)
        return real(name, args, **k)
    ops._run = run
    try:
        return fn(), names
    finally:
        ops._run = real


def k1(dev):
    bad = []
    for apply in ("graph", "host"):
        (net_a, drv_a, sa, A), built_a = record(lambda: build(dev, apply))
        (net_b, drv_b, sb, B), built_b = record(lambda: build(dev, apply, accumulate=1, global_step=0))
        _, ran_a = record(lambda: run_steps(A, sa, 4))
        _, ran_b = record(lambda: run_steps(B, sb, 4))
        bad += differences(f"apply={apply!r}, after 4 replays", snapshot(net_a, drv_a), snapshot(net_b, drv_b))
        if built_a != built_b or ran_a != ran_b:
            bad.append(f"apply={apply!r}: the call lists differ: build {len(built_a)} / {len(built_b)} calls, run {ran_a} / {ran_b}")
        new = [n for n in built_b + ran_b if n in ("hsp_grad_accumulate", "hsp_step_gate_accum")]
        if new:
            bad.append(f"apply={apply!r}: accumulate=1 issued {sorted(set(new))}")
        if B.accum is not None or drv_b.optimizer._accum is not None or drv_b.optimizer._flat[0].flat_f is not None:
            bad.append(f"apply={apply!r}: accumulate=1 attached accumulation state or made the second gradient buffer")
        if apply == "graph" and B.clock.ctl.cpu().tolist()[8:] != [0] * 8:
            bad.append(f"accumulate=1 wrote a slot above 7: {B.clock.ctl.cpu().tolist()}")
        print(f"k1 apply={apply!r}: build {len(built_b)} calls, run {len(ran_b)} calls")
    print(f"k1: {len(bad)} mismatches")
    return bad


def resume(dev):
    kw = dict(accumulate=ACC, global_step=1)
    net, drv, sampler, G = build(dev, "graph", **kw)
    run_steps(G, sampler, 4)
    ckpt = copy.deepcopy(drv.checkpoint(1, 0))
    bad = []
    want = R.decisions(ACC, 1, [R.OK] * 8, 1000)
    if "accum" not in ckpt:
        bad.append(f"the checkpoint has no 'accum' (keys {sorted(ckpt)})")
    elif (ckpt["accum"]["micro"], ckpt["accum"]["pending"]) != (want[3]["micro"], want[3]["pending"]) or want[3]["pending"] < 1:
        bad.append(f"the checkpoint's accum holds micro {ckpt['accum']['micro']}, pending {ckpt['accum']['pending']}, expected {want[3]}")
    if ckpt["scheduler"]["last_epoch"] != want[3]["applied"]:
        bad.append(f"the checkpoint holds last_epoch {ckpt['scheduler']['last_epoch']}, expected {want[3]['applied']}")
    run_steps(G, sampler, 4)
    whole = with_grads(net, drv)

    net2, drv2, sampler2, G2 = build(dev, "graph", init_seed=1, sampler=DeviceSampler(999, dev), **kw)
    drv2.load_checkpoint(ckpt)
    c0 = G2.clock.read()
    if (c0["micro"], c0["pending"], c0["applied"], c0["replays"]) != (want[3]["micro"], want[3]["pending"], 0, 0):
        bad.append(f"the resumed clock starts at {c0}")
    run_steps(G2, sampler2, 4)
    bad += differences("resumed against uninterrupted", whole, with_grads(net2, drv2))
    c, c2 = drv.optimizer.sync_clock(), drv2.optimizer.sync_clock()
    if (c["applied"], c["micro"], c["pending"]) != (want[7]["applied"], want[7]["micro"], want[7]["pending"]):
        bad.append(f"uninterrupted counters {c}, expected {want[7]}")
    if (c2["applied"], c2["micro"], c2["pending"]) != (want[7]["applied"] - want[3]["applied"], want[7]["micro"], want[7]["pending"]):
        bad.append(f"resumed counters {c2}")
    if drv.scheduler.last_epoch != drv2.scheduler.last_epoch or drv.scheduler.last_epoch != want[7]["applied"]:
        bad.append(f"last_epoch {drv.scheduler.last_epoch} / {drv2.scheduler.last_epoch}")
    # with nothing pending the checkpoint's keys are the ones it always had
    if "accum" in drv.checkpoint(1, 0) and c["pending"] == 0:
        bad.append("a checkpoint with nothing pending carries 'accum'")
    print(f"resume: counters {c} / resumed {c2}; {len(bad)} mismatches")
    return bad


def frames(dev):
    import _frame_train_check as fc
    from hs_pose_amd.train import FrameTrainStep
    M, keep, N = 6, 4, 256
    fc.setup()
    FLAGS.reproducible = True
    FLAGS.step_draws = "device"
    net, drv = fc.make(dev, False)
    good, absent = fc.frames(M, dev), fc.frames(M, dev, all_absent=True)
    step = FrameTrainStep(net, drv.optimizer, good, fc.items_of(M, N, dev), keep, scheduler=drv.scheduler,
                          sampler=DeviceSampler(21, dev), n_pts=N, out_size=fc.O, warmup=2, apply="graph", accumulate=2, global_step=1)
    opt = drv.optimizer
    bad, answers = [], []

    def state():
        torch.cuda.synchronize()
        out = {name: getattr(opt._flat[0], attr).detach().clone() for name, attr in STATE}
        out["accumulator"], out["norm scalar"] = opt._flat[0].flat_g.detach().clone(), opt._accum.norm_sq.detach().clone()
        return out
    start = state()
    answers.append(step.run(check=True))                       # micro 1: taken, accumulate-only
    before = state()
    if torch.equal(before["accumulator"], start["accumulator"]) or not bool(before["norm scalar"] > 0):
        bad.append("the first good batch left the accumulator or its norm where they were")
    step.load(frames=dict(inst_ids=absent["inst_ids"]))
    answers.append(step.run(check=True))                       # micro 2, a stepping slot: no good item -> skipped
    after = state()
    bad += differences("across the all-absent slot", before, after)
    info = step.info.cpu().tolist()
    c = step.graphed.clock.read()
    want = dict(replays=2, skipped_no_item=1, skipped_nan=0, applied=0, micro=3, pending=1, take=0, apply=0)
    if {k: c[k] for k in want} != want or info != [0, 0]:
        bad.append(f"after the all-absent slot: info {info}, counters {c}, expected {want}")
    if not bool(torch.isfinite(step.total)):
        bad.append("the loss on the stand-in cloud is not finite: the skip would be the NaN rule's")
    step.load(frames=dict(inst_ids=good["inst_ids"]))
    answers.append(step.run(check=True))                       # micro 3: taken, accumulate-only (two pending)
    bad += differences("across the accumulate-only slots", start, state(), keys=[n for n, _ in STATE])
    answers.append(step.run(check=False))                      # micro 4: taken and applied
    end = state()
    c = drv.optimizer.sync_clock()
    want = dict(replays=4, skipped_no_item=1, applied=1, micro=5, pending=0, take=1, first=0, apply=1)
    if {k: c[k] for k in want} != want:
        bad.append(f"after the stepping slot: counters {c}, expected {want}")
    if answers != [True, False, True, True]:
        bad.append(f"run() answered {answers}")
    if torch.equal(end["params"], start["params"]):
        bad.append("the stepping slot left the parameters where they were")
    print(f"frames: answers {answers}; counters {c}; {len(bad)} mismatches")
    return bad


def calls(dev):
    (net, drv, sampler, G), built = record(lambda: build(dev, "graph", accumulate=ACC))

    def go():
        sampler.advance()
        G.run()
        torch.cuda.synchronize()
    _, ran = record(go)
    bad = []
    for name in ("hsp_step_gate_accum", "hsp_grad_accumulate", "hsp_ranger_step_gated"):
        if built.count(name) != 3:
            bad.append(f"build (2 warm-up runs + the capture): {name} x{built.count(name)}")
    for name in ("hsp_step_gate", "hsp_sumsq_f32", "hsp_ranger_step"):
        if name in built:
            bad.append(f"build issued {name} x{built.count(name)}")
    if ran:
        bad.append(f"run() issued {ran}")
    c = G.clock.read()
    if (c["applied"], c["micro"], c["take"], c["first"]) != (1, 1, 1, 1):
        bad.append(f"the run's counters {c}")
    print(f"calls: build {len(built)} calls, run {ran}; {len(bad)} mismatches")
    return bad


def main():
    mode = sys.argv[1]
    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.reproducible = True
    FLAGS.step_draws = "device"
    run = dict(manual=manual, twin=twin, k1=k1, resume=resume, frames=frames, bf16=lambda d: twin(d, bf16=True), calls=calls)
    if mode not in run:
        raise SystemExit(f"unknown mode {mode}")
    bad = run[mode](dev)
    for line in bad[:30]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
