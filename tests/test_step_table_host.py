"""CPU: ``solver.step_table`` -- the host scalars of the applied steps to come, tabulated for ``hsp_ranger_step_gated`` -- against
the scalars the Ranger class is held to (tests/_optim_ref.class_scalars: ranger2020.py:192-213 in Python doubles, rounded to fp32
once) at the learning rate a real ``LambdaLR`` holds after as many scheduler steps, entry by entry and EXACTLY; the step at which
the table turns from the plain to the rectified update; a table built mid-run; and the argument checks and the struct of the two
entry points, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _optim_ref as R

BETAS, K, THRESH, BASE_LR = (0.95, 0.999), 6, 5, 1e-3
TOTAL, WARMUP, ANNEAL = 40, 5, 0.72


def _scheduler():
    """the project's flat-and-anneal schedule on a CPU stand-in optimizer: the learning rates come from torch's own LambdaLR"""
    from hs_pose_amd.solver import flat_and_anneal_lr_scheduler
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=BASE_LR)
    return opt, flat_and_anneal_lr_scheduler(opt, TOTAL, warmup_iters=WARMUP, anneal_point=ANNEAL)


def _lrs(n, skip=0):
    """group lr before scheduler step skip, skip + 1, ... skip + n - 1"""
    opt, sch = _scheduler()
    out = []
    for j in range(skip + n):
        if j >= skip:
            out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return out


def _table(step0, epoch0, horizon, fill_slow=False):
    from hs_pose_amd.solver import step_table
    _, sch = _scheduler()
    return step_table(step0, epoch0, horizon, sch.base_lrs[0], sch.lr_lambdas[0], BETAS, K, THRESH, fill_slow=fill_slow)


def _check_against_class_scalars(tab, step0, lrs):
    from hs_pose_amd import _lib
    assert tab.dtype.itemsize == 8 and tab["step_lr"].dtype == np.float32 and tab["flags"].dtype == np.int32
    assert len(tab) == len(lrs)
    for j, lr in enumerate(lrs):
        sc = R.class_scalars(step0 + j + 1, lr, betas=BETAS, k=K, n_sma_threshold=THRESH)
        got, flags = tab["step_lr"][j], int(tab["flags"][j])
        assert np.float32(got).view(np.uint32) == np.float32(sc.step_lr).view(np.uint32), (j, float(got), sc.step_lr)
        assert bool(flags & _lib.STEP_ADAPTIVE) == bool(sc.adaptive), j
        assert bool(flags & _lib.STEP_LOOKAHEAD) == bool(sc.lookahead), j
        assert flags & ~(_lib.STEP_ADAPTIVE | _lib.STEP_LOOKAHEAD | _lib.STEP_FILL_SLOW) == 0, j


def test_scheduler_records_its_length():
    _, sch = _scheduler()
    assert sch.total_iters == TOTAL and sch.last_epoch == 0


def test_entries_are_the_host_paths_scalars():
    """40 entries over warm-up, flat part and cosine anneal: step_lr bit for bit, both switches; the learning rate differs in the
    warm-up and in the anneal, so an entry one epoch off its step does not pass"""
    lrs = _lrs(TOTAL)
    assert len(set(lrs[:WARMUP + 1])) == WARMUP + 1 and len(set(lrs[int(ANNEAL * TOTAL):])) > 5 and lrs[WARMUP] == lrs[WARMUP + 1]
    _check_against_class_scalars(_table(0, 0, TOTAL), 0, lrs)


def test_epoch_and_step_are_aligned():
    """entry j is step j + 1 at the rate of epoch j: a table shifted by one on either count differs from the right one"""
    right = _table(0, 0, TOTAL)
    assert not np.array_equal(right["step_lr"], _table(0, 1, TOTAL)["step_lr"])
    assert not np.array_equal(right["step_lr"], _table(1, 0, TOTAL)["step_lr"])


def test_the_table_flips_to_the_adaptive_step_where_radam_does():
    from hs_pose_amd import _lib
    first = next(s for s in range(1, 100) if R.radam_scalars(s, *BETAS, THRESH)[0])
    assert first == 6                                        # N_sma first exceeds 5 at step 6 with betas (0.95, 0.999) ...
    assert first % K == 0 and all(s % K for s in range(1, first))       # ... which is also the first Lookahead step at k = 6
    flags = _table(0, 0, TOTAL)["flags"]
    adaptive = [bool(f & _lib.STEP_ADAPTIVE) for f in flags]
    assert adaptive == [j + 1 >= first for j in range(TOTAL)]
    look = [bool(f & _lib.STEP_LOOKAHEAD) for f in flags]
    assert look == [(j + 1) % K == 0 for j in range(TOTAL)]


def test_resumed_table_and_fill_bit():
    from hs_pose_amd import _lib
    lrs = _lrs(TOTAL - 7, skip=7)
    tab = _table(7, 7, TOTAL - 7)
    _check_against_class_scalars(tab, 7, lrs)
    whole = _table(0, 0, TOTAL)
    assert np.array_equal(tab["step_lr"].view(np.uint32), whole["step_lr"][7:].view(np.uint32))
    assert np.array_equal(tab["flags"], whole["flags"][7:])
    assert not (tab["flags"] & _lib.STEP_FILL_SLOW).any() and not (whole["flags"] & _lib.STEP_FILL_SLOW).any()
    for step0 in (0, 7):
        filled = _table(step0, step0, TOTAL - step0, fill_slow=True)
        assert filled["flags"][0] & _lib.STEP_FILL_SLOW and not (filled["flags"][1:] & _lib.STEP_FILL_SLOW).any()
        plain = _table(step0, step0, TOTAL - step0)
        assert np.array_equal(filled["flags"] & ~np.int32(_lib.STEP_FILL_SLOW), plain["flags"])
        assert np.array_equal(filled["step_lr"].view(np.uint32), plain["step_lr"].view(np.uint32))


def test_horizon_must_be_positive():
    with pytest.raises(ValueError):
        _table(0, 0, 0)


def test_abi_struct_constants_and_argument_checks_without_gpu():
    from hs_pose_amd import _lib
    from hs_pose_amd.solver import STEP_ENTRY
    assert ctypes.sizeof(_lib.HspStepEntry) == 8 == STEP_ENTRY.itemsize
    assert [(n, STEP_ENTRY.fields[n][1]) for n in STEP_ENTRY.names] == [(f, getattr(_lib.HspStepEntry, f).offset)
                                                                       for f, _ in _lib.HspStepEntry._fields_]
    assert (_lib.STEP_ADAPTIVE, _lib.STEP_LOOKAHEAD, _lib.STEP_FILL_SLOW, _lib.STEP_CTL_SLOTS) == (1, 2, 4, 16)
    assert [_lib.STEP_CTL_ARMED, _lib.STEP_CTL_APPLY, _lib.STEP_CTL_INDEX, _lib.STEP_CTL_APPLIED, _lib.STEP_CTL_REPLAYS,
            _lib.STEP_CTL_SKIPPED_NAN, _lib.STEP_CTL_SKIPPED_NO_ITEM, _lib.STEP_CTL_EXHAUSTED] == list(range(8))
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    bad = _lib.ERR_BAD_ARG
    assert bad == -1

    def gate(total=one, info=null, ctl=one, horizon=4):
        return L.hsp_step_gate(total, info, ctl, horizon, null)
    assert gate(total=null) == bad and gate(ctl=null) == bad and gate(horizon=0) == bad and gate(horizon=-3) == bad

    def step(p=one, g=one, m=one, v=one, s=one, rows=one, nrows=3, table=one, ctl=one, horizon=4):
        return L.hsp_ranger_step_gated(p, g, m, v, s, rows, nrows, 0.95, 0.999, 1e-5, 0.0, 0.5, 0, null, 0.0, table, ctl, horizon, null)
    for name in ("p", "g", "m", "v", "s", "rows", "table", "ctl"):
        assert step(**{name: null}) == bad, name
    assert step(nrows=0) == bad and step(horizon=0) == bad
