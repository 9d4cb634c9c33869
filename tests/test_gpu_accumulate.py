"""GPU: gradient accumulation in the graphed training step (``accumulate=`` on ``graph.GraphedTrainStep`` / ``train.FrameTrainStep``;
include/hsp.h: "gradient accumulation under the device's decision").

In process, through the C ABI:
  hsp_grad_accumulate   the accumulator against numpy fp32 from the header's formula (tests/_accum_ref.py), bit for bit, and the
                        norm scalar bit-equal to ``hsp_sumsq_f32`` run over the result, over sizes that reach the tail, a second
                        grid-stride trip and the network's own flat total, first = 1 / 0, and a previous norm far under max_norm (c
                        exactly 1), over it, and NaN; with ``ctl`` given, take = 0 and an unarmed block leave accumulator and scalar
                        bit-unchanged, and take / first come from the block, not from the argument
  hsp_step_gate_accum   every control slot after every launch against ``_accum_ref.decisions``, on the event lists of the host test

In child processes (tests/_accumulate_check.py, one mode each: a capture must precede the network's first eager backward): the
graphed step under accumulation against an independent oracle built from existing pieces, against its own host form, across a
checkpoint, from frames, on bf16 rows, and the calls it issues."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _accum_ref as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_NORM = 5.0
SENTINEL = np.float32(-1234.5)
PAD = 8
# 1 049 603 = 4 * 256 * 1024 + 4 * 256 + 3: a second grid-stride trip of some workgroups, then a tail
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 1049603)
PREV_NORMS = {"under": 1e-6, "over": 400.0, "nan": float("nan")}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _network_total():
    """one flat group's own ``total``: HSPose's trainable parameters, each start 16-byte aligned (solver._FlatGroup)"""
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.HSPose import HSPose
    FLAGS.reset()
    FLAGS.train = 1
    try:
        net = HSPose("PoseNet_only")
        return sum((p.numel() + 3) & ~3 for g in net.build_params(training_stage_freeze=[]) for p in g["params"])
    finally:
        FLAGS.reset()


@pytest.fixture(scope="module")
def data():
    """acc / fresh of the largest size, made once; every case reads a prefix"""
    n = max(max(SIZES), _network_total())
    rng = np.random.RandomState(11)
    return (rng.standard_normal(n).astype(np.float32) * np.float32(3.0),
            (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(np.float32), n)


def _accumulate(dev, acc, fresh, prev, first, ctl=None, first_arg=None):
    """the call on padded copies -> (acc after, padding after, norm scalar tensor, hsp_sumsq_f32 of the result)"""
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    n = acc.size
    a = torch.from_numpy(np.concatenate([acc, np.full(PAD, SENTINEL)])).to(dev)
    f = torch.from_numpy(np.concatenate([fresh, np.full(PAD, np.float32(7.0))])).to(dev)
    nsq = torch.tensor([prev], dtype=torch.float32, device=dev)
    wsb = lib().hsp_sumsq_workspace_bytes(n)
    ws = ops._ws(wsb, dev)
    ctl_d = None if ctl is None else torch.tensor(ctl, dtype=torch.int32, device=dev)
    ops._run("hsp_grad_accumulate", (ops._p(a), ops._p(f), n, ops._p(nsq), MAX_NORM, int(first if first_arg is None else first_arg),
                                     ops._p(ctl_d), ops._p(ws), wsb, ops._stream()))
    if ctl_d is not None:
        assert ctl_d.cpu().tolist() == ctl                                         # the block is read only
    assert np.array_equal(_bits(f.cpu().numpy()[:n]), _bits(fresh))                # so is the fresh gradient
    want = torch.empty(1, dtype=torch.float32, device=dev)
    ops._run("hsp_sumsq_f32", (ops._p(a), n, ops._p(want), ops._p(ws), wsb, ops._stream()))
    out = a.cpu().numpy()
    return out[:n], out[n:], nsq, want


@pytest.mark.parametrize("n", SIZES + ("network",))
def test_accumulate_formula_and_norm(dev, data, n):
    acc0, fresh0, nmax = data
    n = _network_total() if n == "network" else n
    assert 0 < n <= nmax
    acc, fresh = acc0[:n], fresh0[:n]
    bad = []
    for first in (1, 0):
        for name, prev in PREV_NORMS.items():
            got, pad, nsq, want_nsq = _accumulate(dev, acc, fresh, prev, first)
            want = A.accumulate(acc, fresh, first, prev, MAX_NORM)
            c = A.clip_coef(prev, MAX_NORM)
            assert (name == "under") == (c == 1.0) and (name == "nan") == bool(np.isnan(c)) and (name == "over") == bool(c < 1.0)
            if not np.array_equal(got, want, equal_nan=True):
                d = np.abs(got.astype(np.float64) - want.astype(np.float64))
                bad.append(f"n {n} first {first} norm {name}: {int((_bits(got) != _bits(want)).sum())} elements differ, "
                           f"worst |diff| {np.nanmax(d):.3e} (c = {c!r})")
            if not first and name == "nan" and not np.isnan(got).all():
                bad.append(f"n {n} first 0: a NaN norm did not reach every element")
            if first and np.isnan(got).any():
                bad.append(f"n {n} first 1 norm {name}: the stale accumulator or scalar was read")
            if not (_bits(pad) == _bits(SENTINEL)).all():
                bad.append(f"n {n} first {first} norm {name}: an element past the end was written")
            if not torch.equal(nsq.view(torch.int32), want_nsq.view(torch.int32)):
                bad.append(f"n {n} first {first} norm {name}: norm scalar {nsq.item()!r}, hsp_sumsq_f32 of the result {want_nsq.item()!r}")
            elif not np.isnan(want).any() and not torch.equal(nsq, want_nsq):
                bad.append(f"n {n} first {first} norm {name}: torch.equal fails on the norm scalar")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("ctl", [[1, 0, 0, 0, 3, 1, 0, 0, 5, 0, 1, 2, 0, 0, 0, 0], [0] * 8 + [5, 0, 1, 0] + [0] * 4,
                                 [1, 1, 0, 1, 3, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0]], ids=["skipped", "unarmed", "take0-apply1"])
def test_gated_accumulate_not_taken_touches_nothing(dev, data, ctl):
    for n in (5, 1025, 1049603):
        acc, fresh = data[0][:n], data[1][:n]
        for prev in (400.0, float("nan")):
            got, pad, nsq, _ = _accumulate(dev, acc, fresh, prev, 1, ctl=ctl)
            assert np.array_equal(_bits(got), _bits(acc)) and (_bits(pad) == _bits(SENTINEL)).all(), n
            assert np.array_equal(_bits(nsq.cpu().numpy()), _bits(np.float32([prev]))), n


@pytest.mark.parametrize("first", [0, 1])
def test_gated_accumulate_reads_take_and_first_from_the_block(dev, data, first):
    n = 1025
    acc, fresh = data[0][:n], data[1][:n]
    ctl = [1, 0, 0, 0, 1, 0, 0, 0, 2, 1, first, 1, 0, 0, 0, 0]
    got, pad, nsq, want_nsq = _accumulate(dev, acc, fresh, 400.0, first, ctl=ctl, first_arg=1 - first)     # (the argument says otherwise)
    assert np.array_equal(_bits(got), _bits(A.accumulate(acc, fresh, first, 400.0, MAX_NORM)))
    assert torch.equal(nsq, want_nsq) and (_bits(pad) == _bits(SENTINEL)).all()


@pytest.mark.parametrize("accumulate", [1, 2, 3, 4])
def test_gate_follows_the_statement(dev, accumulate):
    from hs_pose_amd import ops
    total = torch.zeros((), dtype=torch.float32, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    value = {A.OK: (float("inf"), 3), A.NAN: (float("nan"), 3), A.NOITEM: (1.0, 0)}     # (+inf is no skip)
    for name, g0, events, horizon in A.EVENT_CASES:
        for with_info in (True, False):
            if not with_info and A.NOITEM in events:
                continue
            ctl = torch.tensor([0] * 8 + [g0] + [0] * 3 + [41, 42, 43, 44], dtype=torch.int32, device=dev)
            total.fill_(float("nan"))
            # unarmed: take = apply = 0, nothing counted, micro stays
            ops._run("hsp_step_gate_accum", (ops._p(total), ops._p(info), ops._p(ctl), horizon, accumulate, ops._stream()))
            assert ctl.cpu().tolist() == [0] * 8 + [g0] + [0] * 3 + [41, 42, 43, 44], name
            ctl[0:1].fill_(1)
            for i, (ev, d) in enumerate(zip(events, A.decisions(accumulate, g0, events, horizon))):
                total.fill_(value[ev][0] if i % 2 else (-value[ev][0] if ev == A.OK else value[ev][0]))
                info.fill_(value[ev][1])
                ops._run("hsp_step_gate_accum", (ops._p(total), ops._p(info if with_info else None), ops._p(ctl), horizon,
                                                 accumulate, ops._stream()))
                want = [1, d["apply"], d["index"], d["applied"], d["replays"], d["skipped_nan"], d["skipped_no_item"],
                        d["exhausted"], d["micro"], d["take"], d["first"], d["pending"], 41, 42, 43, 44]
                assert ctl.cpu().tolist() == want, (name, accumulate, i, ev)


@pytest.mark.parametrize("mode", ["manual", "twin", "k1", "resume", "frames", "bf16", "calls"])
def test_accumulation_in_the_graphed_step(dev, mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_accumulate_check.py"), mode], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
