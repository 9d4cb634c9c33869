"""GPU: the two entry points that put the optimizer step under the device's own decision (include/hsp.h: "the step applied on
the device's own decision"), through the C ABI.

  hsp_step_gate          every one of the sixteen control slots after one launch against a restatement of the header's six rules,
                         over loss (finite, NaN, +inf, -inf) x info (NULL, [0,0], [1,1], [3,3]) x applied (horizon - 1,
                         horizon) x armed (0, 1), each from known, non-zero counters;
  hsp_ranger_step_gated  apply = 1: the cross/work and count cases of tests/_optim_ref.cases() with the scalars in a one-entry
                         table, within that module's bound |kernel - ref64| <= 2 e + 2^-149 AND bit-equal to hsp_ranger_step
                         handed the same scalars by value; apply = 0: all five buffers come back bit-identical; the fill bit:
                         slow is taken from the weights before the update."""
import numpy as np
import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

BUFS = ("p", "g", "m", "v", "slow")
HORIZON = 5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------------------

def gate_rules(ctl, total, info, horizon):
    """include/hsp.h, hsp_step_gate, rules 1-6 on a list of sixteen ints"""
    c = list(ctl)
    if c[0] == 0:
        c[1] = 0
        return c
    c[4] += 1
    c[1] = 0
    if np.isnan(total):
        c[5] += 1
    elif info is not None and info[0] == 0:
        c[6] += 1
    elif c[3] >= horizon:
        c[7] = 1
    else:
        c[1], c[2], c[3] = 1, c[3], c[3] + 1
    return c


def test_gate_truth_table(dev):
    from hs_pose_amd import ops
    bad, seen = [], set()
    for armed in (0, 1):
        for applied in (HORIZON - 1, HORIZON):
            for total in (1.5, float("nan"), float("inf"), float("-inf")):
                for info in (None, [0, 0], [1, 1], [3, 3]):
                    start = [armed, 7, 2, applied, 11, 3, 2, 0] + list(range(101, 109))
                    ctl = torch.tensor(start, dtype=torch.int32, device=dev)
                    t = torch.tensor(total, dtype=torch.float32, device=dev)
                    inf = None if info is None else torch.tensor(info, dtype=torch.int32, device=dev)
                    ops._run("hsp_step_gate", (ops._p(t), ops._p(inf), ops._p(ctl), HORIZON, ops._stream()))
                    got, want = ctl.cpu().tolist(), gate_rules(start, total, info, HORIZON)
                    if got != want:
                        bad.append(f"armed {armed} applied {applied} total {total} info {info}: got {got} want {want}")
                    if got[8:] != start[8:] or got[0] != armed:
                        bad.append(f"armed {armed} applied {applied} total {total} info {info}: a reserved slot or armed was written")
                    if armed == 0 and got[2:] != start[2:]:
                        bad.append(f"unarmed, total {total} info {info}: a counter moved")
                    seen.add((want[1], want[5] - start[5], want[6] - start[6], want[7]))
                    if inf is not None and inf.cpu().tolist() != info:
                        bad.append("info was written")
    assert not bad, "\n".join(bad[:20])
    # the cases reach every outcome: applied, skipped for NaN, for no item, refused at the end of the table, unarmed
    assert seen == {(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 0, 0)}


def test_gate_counts_over_a_sequence(dev):
    """one block through nine launches: infinities are applied, a NaN and an empty batch are not, and the table of three runs out"""
    from hs_pose_amd import ops
    ctl = torch.zeros(16, dtype=torch.int32, device=dev)
    t = torch.zeros((), dtype=torch.float32, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    seq = [(0, 1.0, 1), (1, float("inf"), 2), (1, float("nan"), 2), (1, 2.0, 0), (1, float("-inf"), 4), (1, 3.0, 1), (1, 4.0, 1),
           (1, float("nan"), 0), (1, 5.0, 1)]
    want, applies = [0] * 16, []
    for armed, total, good in seq:
        ctl[0:1].fill_(armed)
        want[0] = armed
        t.fill_(total)
        info.fill_(good)
        ops._run("hsp_step_gate", (ops._p(t), ops._p(info), ops._p(ctl), 3, ops._stream()))
        want = gate_rules(want, total, [good, good], 3)
        got = ctl.cpu().tolist()
        assert got == want, (armed, total, good, got, want)
        applies.append(got[1])
    assert applies == [0, 1, 0, 0, 1, 1, 0, 0, 0]
    assert want[:8] == [1, 0, 2, 3, 8, 2, 1, 1]


# ------------------------------------------------------------------------------------------------------------
# the gated step
# ------------------------------------------------------------------------------------------------------------

def _upload(dev, bufs, rows, gnorm_sq):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspRowDesc
    total = bufs["p"].size
    assert all(0 <= off and n > 0 and off + n <= total for off, n, _ in rows)          # no row leaves the buffers
    t = {k: torch.from_numpy(np.array(bufs[k], dtype=np.float32, copy=True)).to(dev) for k in BUFS}
    table = ops.upload_table((HspRowDesc * len(rows))(*[(int(o), int(n), int(gc)) for o, n, gc in rows]), dev)
    gn = None if gnorm_sq is None else torch.tensor([float(gnorm_sq)], dtype=torch.float32, device=dev)
    return t, table, gn


def _by_value(dev, bufs, rows, sc, gnorm_sq=None):
    from hs_pose_amd import ops
    t, table, gn = _upload(dev, bufs, rows, gnorm_sq)
    ops._run("hsp_ranger_step",
             (ops._p(t["p"]), ops._p(t["g"]), ops._p(t["m"]), ops._p(t["v"]), ops._p(t["slow"]), ops._p(table), len(rows),
              sc.beta1, sc.beta2, sc.eps, sc.weight_decay, sc.step_lr, sc.adaptive, sc.lookahead, sc.la_alpha, sc.gc_after,
              ops._p(gn), sc.max_norm, ops._stream()))
    return {k: t[k].cpu().numpy() for k in BUFS}


def _gated(dev, bufs, rows, sc, gnorm_sq=None, entries=None, ctl=None, fill=False):
    """hsp_ranger_step_gated on copies of the five host buffers.  Default: a one-entry table holding sc's step_lr and switches and
    a control block that says apply entry 0."""
    from hs_pose_amd import _lib, ops
    from hs_pose_amd.solver import STEP_ENTRY
    t, table, gn = _upload(dev, bufs, rows, gnorm_sq)
    if entries is None:
        flags = (_lib.STEP_ADAPTIVE if sc.adaptive else 0) | (_lib.STEP_LOOKAHEAD if sc.lookahead else 0) | (_lib.STEP_FILL_SLOW if fill else 0)
        entries = [(sc.step_lr, flags)]
    tab = np.array(entries, dtype=STEP_ENTRY)
    ctl = [1, 1, 0, 1] + [0] * 12 if ctl is None else ctl
    assert len(ctl) == 16 and (ctl[1] == 0 or 0 <= ctl[2] <= len(tab))     # the entry named exists (or is the first past the end)
    steps = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    ctl_d = torch.tensor(ctl, dtype=torch.int32, device=dev)
    ops._run("hsp_ranger_step_gated",
             (ops._p(t["p"]), ops._p(t["g"]), ops._p(t["m"]), ops._p(t["v"]), ops._p(t["slow"]), ops._p(table), len(rows),
              sc.beta1, sc.beta2, sc.eps, sc.weight_decay, sc.la_alpha, sc.gc_after, ops._p(gn), sc.max_norm,
              ops._p(steps), ops._p(ctl_d), len(tab), ops._stream()))
    assert ctl_d.cpu().tolist() == ctl and np.array_equal(steps.cpu().numpy(), tab.view(np.uint8))      # read only
    return {k: t[k].cpu().numpy() for k in BUFS}


def _case_bufs(c):
    return {k: getattr(c, k) for k in BUFS}


def _names(prefix):
    names = [n for n in R.cases() if n.startswith(prefix)]
    assert names
    return names


@pytest.mark.parametrize("prefix,count", [("cross/work/", 48), ("count/", 20)])
def test_gated_step_applies_the_table_entry(dev, prefix, count):
    """scalars from a one-entry table: within the float64 bound, bit-equal to the by-value entry point, gaps and gradients
    untouched"""
    names = _names(prefix)
    assert len(names) == count
    if prefix == "count/":
        assert {n.split("/")[1] for n in names} == {"rows1", "rows3", "rows4", "rows5", "rows9"}
    bad = []
    for name in names:
        c = R.cases()[name]
        got = _gated(dev, _case_bufs(c), c.rows, c.sc, c.gnorm_sq)
        bad += [f"{name}: {m}" for m in R.failures(got, R.reference(name))]
        ref = _by_value(dev, _case_bufs(c), c.rows, c.sc, c.gnorm_sq)
        for k in BUFS:
            if not np.array_equal(_bits(got[k]), _bits(ref[k])):
                bad.append(f"{name}: {k} differs from hsp_ranger_step's in {int((_bits(got[k]) != _bits(ref[k])).sum())} elements")
            if not (_bits(got[k])[c.gaps] == _bits(np.float32(R.SENTINEL[k]))).all():
                bad.append(f"{name}: a padding element of {k} was written")
        if not np.array_equal(_bits(got["g"]), _bits(c.g)):
            bad.append(f"{name}: the gradient buffer was written")
        if np.array_equal(_bits(got["m"]), _bits(c.m)):             # (the weights may stand still: a clipped, plain step of
            bad.append(f"{name}: the step did not run")             # 1e-4 * 1e-6 is below half an ulp of 0.1; the moment is not)
    assert not bad, "\n".join(bad[:40])


def test_gated_step_reads_the_entry_the_gate_named(dev):
    """three entries with different step_lr and switches: the control block's index picks"""
    from hs_pose_amd import _lib
    c = R.cases()["count/rows9/work/default"]
    entries = [(3e-4, 0), (7e-4, _lib.STEP_ADAPTIVE), (2e-3, _lib.STEP_ADAPTIVE | _lib.STEP_LOOKAHEAD)]
    outs = []
    for i, (lr, flags) in enumerate(entries):
        sc = c.sc._replace(step_lr=float(np.float32(lr)), adaptive=int(bool(flags & 1)), lookahead=int(bool(flags & 2)))
        got = _gated(dev, _case_bufs(c), c.rows, sc, c.gnorm_sq, entries=entries, ctl=[1, 1, i, i + 1] + [0] * 12)
        ref = _by_value(dev, _case_bufs(c), c.rows, sc, c.gnorm_sq)
        for k in BUFS:
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), (i, k)
        outs.append(got["p"])
    assert not np.array_equal(_bits(outs[0]), _bits(outs[1])) and not np.array_equal(_bits(outs[1]), _bits(outs[2]))


@pytest.mark.parametrize("ctl", [[1, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1], [1, 1, 1, 1]],
                         ids=["skip", "unarmed", "skip-stale-index", "index-at-horizon"])
def test_gated_step_not_applied_touches_nothing(dev, ctl):
    """apply = 0 (or an index outside the table, which the gate never writes): all five buffers, sentinel gaps included, come
    back bit-identical -- on the mixed table in both modes, fill bit set: nothing of it may run either"""
    for name in ("count/rows9/work/default", "count/rows9/update/second", "count/rows1/work/second"):
        c = R.cases()[name]
        got = _gated(dev, _case_bufs(c), c.rows, c.sc, c.gnorm_sq, ctl=ctl + [0] * 12, fill=True)
        for k in BUFS:
            assert np.array_equal(_bits(got[k]), _bits(getattr(c, k))), (name, k)


@pytest.mark.parametrize("name", ["count/rows9/work/default", "count/rows5/update/default", "count/rows9/work/second",
                                  "count/rows4/update/second", "cross/work/ad0-la1-gcafter0-wd0-noclip"])
def test_fill_bit_takes_slow_from_the_weights_before_the_step(dev, name):
    c = R.cases()[name]
    bufs = _case_bufs(c)
    bufs["slow"] = np.full_like(c.slow, np.float32(R.SENTINEL["slow"]))            # sentinels in the rows too
    got = _gated(dev, bufs, c.rows, c.sc, c.gnorm_sq, fill=True)
    inrow = ~c.gaps
    assert (_bits(got["slow"])[c.gaps] == _bits(np.float32(R.SENTINEL["slow"]))).all()
    if not c.sc.lookahead:
        assert np.array_equal(_bits(got["slow"])[inrow], _bits(c.p)[inrow])          # the weights from BEFORE the step
        want = R.step_ref64(c.p, c.g, c.m, c.v, bufs["slow"], c.rows, c.sc, c.gnorm_sq)
        want["slow"] = R.V(np.where(inrow, c.p, bufs["slow"]))
    else:
        slow0 = np.where(inrow, c.p, bufs["slow"]).astype(np.float32)               # step_ref64 run with slow := p
        want = R.step_ref64(c.p, c.g, c.m, c.v, slow0, c.rows, c.sc, c.gnorm_sq)
    assert not R.failures(got, want), R.failures(got, want)
    assert not np.array_equal(_bits(got["m"]), _bits(c.m))
    # and without the bit the same call leaves the sentinels where Lookahead does not write
    if not c.sc.lookahead:
        plain = _gated(dev, bufs, c.rows, c.sc, c.gnorm_sq)
        assert np.array_equal(_bits(plain["slow"]), _bits(bufs["slow"]))
