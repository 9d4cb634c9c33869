"""CPU: gradient accumulation of the graphed training step, the parts that need no device.

  (a) tests/_accum_ref.py::decisions -- the statement the gate kernel is held to -- against a LITERAL run of the reference's loop
      (engine/train.py:99-114: NaN test and ``continue`` before the backward, ``clip_grad_norm_`` after every backward, optimizer
      step and ``zero_grad`` when ``global_step % accumulate == 0``) on a 3-parameter torch model with SGD and injected NaN
      losses: the decisions, replayed on the same gradients, give the same final weights (``torch.equal``), the same stepping
      slots and the same skip count, over accumulate 1-4 and the event lists of ``_accum_ref.EVENT_CASES``.
  (b) the built library exports ``hsp_grad_accumulate`` and ``hsp_step_gate_accum``, ``_lib`` binds them from the header, the four
      new slot constants are the header's, and both entries decline bad arguments before any launch.
  (c) ``GraphedTrainStep`` and ``FrameTrainStep`` accept ``accumulate`` / ``global_step``; ``accumulate=0`` raises ``ValueError`` with
      no device present.
"""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import _accum_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM, LR = 0.75, 0.1


def _gradients(n):
    """the gradient of slot i (the loss is <w, g_i>): norms on both sides of MAX_NORM, so clips bite on some slots only"""
    gen = torch.Generator().manual_seed(5)
    return [torch.randn(3, generator=gen) * (0.2 if i % 3 == 1 else 0.7) for i in range(n)]


def reference_loop(accumulate, global_step0, events, horizon):
    """engine/train.py:99-114, line for line, until ``horizon`` optimizer steps were taken (the end of the schedule)"""
    w = torch.nn.Parameter(torch.tensor([0.3, -0.2, 0.5]))
    optimizer = torch.optim.SGD([w], lr=LR)
    global_step, steps, skipped, stepped_at = global_step0, 0, 0, []
    for i, (ev, g) in enumerate(zip(events, _gradients(len(events)))):
        total_loss = (w * g).sum() * (float("nan") if ev != A.OK else 1.0)      # ('noitem' skips like a NaN: FrameTrainStep's rule)
        if math.isnan(float(total_loss.detach())):
            skipped += 1
            global_step += 1
            continue
        if steps >= horizon:                                                    # the table is used up: training is over
            break
        if global_step % accumulate == 0:
            total_loss.backward()
            torch.nn.utils.clip_grad_norm_([w], MAX_NORM)
            optimizer.step()
            optimizer.zero_grad()
            steps += 1
            stepped_at.append(i)
        else:
            total_loss.backward()
            torch.nn.utils.clip_grad_norm_([w], MAX_NORM)
        global_step += 1
    return w.detach().clone(), stepped_at, skipped


def by_decisions(accumulate, global_step0, events, horizon):
    """the same gradients driven by ``decisions``: take (first: into a fresh accumulator), clip the accumulator, apply"""
    w = torch.nn.Parameter(torch.tensor([0.3, -0.2, 0.5]))
    optimizer = torch.optim.SGD([w], lr=LR)
    stepped_at = []
    for i, (d, g) in enumerate(zip(A.decisions(accumulate, global_step0, events, horizon), _gradients(len(events)))):
        if not d["take"]:
            assert not d["apply"]
            continue
        w.grad = g.clone() if d["first"] else w.grad + g
        torch.nn.utils.clip_grad_norm_([w], MAX_NORM)
        if d["apply"]:
            optimizer.step()
            stepped_at.append(i)
    return w.detach().clone(), stepped_at


@pytest.mark.parametrize("accumulate", [1, 2, 3, 4])
@pytest.mark.parametrize("case", A.EVENT_CASES, ids=[c[0] for c in A.EVENT_CASES])
def test_decisions_equal_the_reference_loop(accumulate, case):
    _, g0, events, horizon = case
    want_w, want_steps, want_skipped = reference_loop(accumulate, g0, events, horizon)
    got_w, got_steps = by_decisions(accumulate, g0, events, horizon)
    assert got_steps == want_steps
    assert torch.equal(got_w, want_w), (got_w, want_w)
    dec = A.decisions(accumulate, g0, events, horizon)
    last = dec[-1]
    assert last["skipped_nan"] + last["skipped_no_item"] == sum(e != A.OK for e in events)
    assert last["micro"] == g0 + len(events) and last["replays"] == len(events) and last["applied"] == len(want_steps)
    pending = applied = refused = 0
    for ev, d in zip(events, dec):                      # pending counts the takes since the last applied step
        refused |= int(ev == A.OK and applied >= horizon)
        assert d["take"] == int(ev == A.OK and applied < horizon) and d["exhausted"] == refused
        if d["take"]:
            assert d["first"] == int(pending == 0)
        pending = 0 if d["apply"] else pending + d["take"]
        applied += d["apply"]
        assert d["pending"] == pending and d["applied"] == applied
    if accumulate == 1:
        assert all(d["apply"] == d["take"] and d["pending"] == 0 for d in dec)


def test_the_event_lists_reach_the_cases():
    """a NaN on a stepping slot, on an accumulate-only slot, two in a row, a start that is no multiple of accumulate, exhaustion"""
    for accumulate in (2, 3, 4):
        kinds = set()
        for _, g0, events, horizon in A.EVENT_CASES:
            for i, ev in enumerate(events):
                if ev == A.NAN:
                    kinds.add("stepping" if (g0 + i) % accumulate == 0 else "accumulate-only")
                    if i and events[i - 1] == A.NAN:
                        kinds.add("row")
            if g0 % accumulate:
                kinds.add("offset")
            if A.decisions(accumulate, g0, events, horizon)[-1]["exhausted"]:
                kinds.add("exhausted")
            dec = A.decisions(accumulate, g0, events, horizon)
            if any(d["pending"] >= accumulate for d in dec):
                kinds.add("overgrown")                  # a skipped stepping slot: `accumulate` or more micro-batches pending
        assert kinds == {"stepping", "accumulate-only", "row", "offset", "exhausted", "overgrown"}, (accumulate, kinds)


def test_clip_coefficient_and_formula():
    import numpy as np
    assert A.clip_coef(1e-6, 5.0) == np.float32(1.0)                            # far under max_norm: exactly 1
    c = A.clip_coef(400.0, 5.0)
    assert c == np.float32(5.0) / (np.float32(20.0) + np.float32(1e-6)) and c < 1
    assert np.isnan(A.clip_coef(float("nan"), 5.0))
    acc, fresh = np.float32([1.5, -2.0, 0.0]), np.float32([0.25, 1.0, -0.0])
    assert np.array_equal(A.accumulate(acc, fresh, 1, float("nan"), 5.0), np.float32([0.25, 1.0, 0.0]))
    assert np.array_equal(A.accumulate(acc, fresh, 0, 1e-6, 5.0), acc + fresh)
    assert np.isnan(A.accumulate(acc, fresh, 0, float("nan"), 5.0)).all()


def test_library_exports_and_binds_the_new_entries():
    from hs_pose_amd import _lib
    L = _lib.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hsp.h")).read(), flags=re.S)
    for name in ("hsp_grad_accumulate", "hsp_step_gate_accum"):
        assert hasattr(L, name), f"libhsp.so lacks {name}"
        assert name in _lib.SIGNATURES and f"int {name}(" in txt
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["hsp_grad_accumulate"][1]) == 10 and len(_lib.SIGNATURES["hsp_step_gate_accum"][1]) == 6
    slots = dict(MICRO=8, TAKE=9, FIRST=10, PENDING=11)
    for name, slot in slots.items():
        assert getattr(_lib, f"STEP_CTL_{name}") == slot == int(re.search(rf"#define HSP_STEP_CTL_{name} (\d+)", txt).group(1))
    assert max(slots.values()) < _lib.STEP_CTL_SLOTS == 16
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    bad = _lib.ERR_BAD_ARG

    def gate(total=one, info=null, ctl=one, horizon=4, accumulate=3):
        return L.hsp_step_gate_accum(total, info, ctl, horizon, accumulate, null)
    assert gate(total=null) == bad and gate(ctl=null) == bad and gate(horizon=0) == bad and gate(accumulate=0) == bad

    def acc(a=one, f=one, n=1024, nsq=one, ws=one, ws_bytes=1 << 20):
        return L.hsp_grad_accumulate(a, f, n, nsq, 5.0, 0, null, ws, ws_bytes, null)
    assert acc(a=null) == bad and acc(f=null) == bad and acc(nsq=null) == bad and acc(n=0) == bad
    assert acc(a=ctypes.c_void_p(4100)) == _lib.ERR_UNSUPPORTED and acc(f=ctypes.c_void_p(4104)) == _lib.ERR_UNSUPPORTED
    assert acc(ws=null) == _lib.ERR_WORKSPACE and acc(ws_bytes=L.hsp_sumsq_workspace_bytes(1024) - 1) == _lib.ERR_WORKSPACE


def test_the_graphed_steps_take_the_arguments_and_validate_without_a_device():
    from hs_pose_amd.graph import GraphedTrainStep
    from hs_pose_amd.solver import DeviceClock, Ranger
    from hs_pose_amd.train import FrameTrainStep
    for cls in (GraphedTrainStep, FrameTrainStep):
        params = inspect.signature(cls.__init__).parameters
        assert params["accumulate"].default == 1 and params["global_step"].default == 0, cls
    for fn in (DeviceClock.__init__, Ranger.device_clock):
        params = inspect.signature(fn).parameters
        assert params["accumulate"].default == 1 and params["global_step"].default == 0, fn
    assert callable(Ranger.accumulated_grads)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="accumulate"):
            GraphedTrainStep(None, None, {}, accumulate=bad)
        with pytest.raises(ValueError, match="accumulate"):
            FrameTrainStep(None, None, {}, {}, 1, accumulate=bad)
