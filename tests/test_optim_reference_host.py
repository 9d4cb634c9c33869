"""CPU: the float64 Ranger step of tests/_optim_ref.py and its derived bound, before any kernel is looked at.

  * a correct fp32 evaluation of the formula (in the reference's operation order, not the kernel's) lies within 2 e + 2^-149 on
    every case of the table: the derivation admits what it must admit;
  * every one-line mutant of that evaluation is out of bound on at least one case, which is named: the table can see a kernel
    that is subtly wrong;
  * the float64 step, chained from the closed-form start, lands on what the reference optimizer itself wrote
    (tests/golden/solver_ranger_*.npz) at every step those fixtures hold -- the first is step 5, 7 and 6 -- and on their final
    moments, to the 1e-6 of tests/test_solver_oracle.py."""
import numpy as np
import pytest

import _optim_ref as R
from conftest import golden
from test_solver_oracle import CASES


def _fp32(c, mutant=None):
    return R.step_f32(c.p, c.g, c.m, c.v, c.slow, c.rows, c.sc, c.gnorm_sq, mutant=mutant)


def test_case_table_is_what_the_device_test_needs():
    cs = R.cases()
    lens = {(n, gc) for c in cs.values() for _, n, gc in c.rows}
    for n in R.ROW_LENGTHS + R.LONG_LENGTHS:
        assert (n, 1) in lens and (n, 0) in lens, n
    assert (5000, 1) in lens
    assert {len(c.rows) for c in cs.values()} >= {1, 3, 4, 5, 9}
    assert sum(k.startswith("cross/work/") for k in cs) == 48 and sum(k.startswith("cross/update/") for k in cs) == 48
    for c in cs.values():
        assert c.total < 20000 and c.gaps.any()
        assert all(off % 4 == 0 for off, _, _ in c.rows)
        end = 0
        for off, n, _ in c.rows:                               # a gap before every row, and one after the last
            assert off >= ((end + 3) & ~3) + 4
            end = off + n
        assert c.total >= ((end + 3) & ~3) + 4
        for k in ("p", "g", "m", "v", "slow"):
            assert (getattr(c, k)[c.gaps] == np.float32(R.SENTINEL[k])).all()
    coef = [float(R.clip_coefficient(c.gnorm_sq, c.sc.max_norm).x) for k, c in cs.items() if k.endswith("-small")]
    assert coef and all(0.9e-3 < x < 1.1e-3 for x in coef)
    assert all(float(R.clip_coefficient(c.gnorm_sq, c.sc.max_norm).x) == 1.0 for k, c in cs.items() if k.endswith("-cap"))
    big = cs["len/short/large/default"]
    assert np.abs(big.g[~big.gaps]).min() > 2e3 and float(R.clip_coefficient(big.gnorm_sq, big.sc.max_norm).x) < 1e-3
    tiny = cs["len/short/eps/default"]
    assert np.sqrt(tiny.v[~tiny.gaps]).max() < 1e-2 * tiny.sc.eps


def test_fp32_restatement_is_within_the_bound():
    worst = dict.fromkeys(R.NAMES, 0.0)
    for name, c in R.cases().items():
        got, want = _fp32(c), R.reference(name)
        assert not R.failures(got, want), (name, R.failures(got, want))
        for k in ("p", "g", "m", "v", "slow"):                 # and it leaves the gaps alone, like the reference
            if k != "g":
                assert (got[k][c.gaps] == np.float32(R.SENTINEL[k])).all()
        for k, r in R.ratios(got, want).items():
            worst[k] = max(worst[k], r)
    print("\nfp32 restatement, worst err / bound: " + "  ".join(f"{k} {worst[k]:.3f}" for k in R.NAMES))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_every_mutant_is_out_of_bound_somewhere(mutant):
    caught, worst = [], 0.0
    for name, c in R.cases().items():
        r = R.ratios(_fp32(c, mutant), R.reference(name))
        if max(r.values()) > 1.0:
            caught.append((name, r))
            worst = max(worst, max(r.values()))
    assert caught, f"{mutant} ({R.MUTANTS[mutant]}) stays within the bound on every case: the table is missing a case"
    name, r = caught[0]
    print(f"\n{mutant}: out of bound on {len(caught)} of {len(R.cases())} cases, first {name} "
          f"(" + " ".join(f"{k} x{r[k]:.3g}" for k in R.NAMES if r[k] > 1.0) + f"), worst x{worst:.3g}")


@pytest.mark.parametrize("name", list(CASES))
def test_fp64_step_reproduces_the_reference_fixtures(ref, name):
    g, c = golden(name), CASES[name]
    kw = dict(c["kw"])
    shapes = ref.OPT_SHAPES
    rows, total = R.expected_rows(shapes, use_gc=True, gc_conv_only=kw.pop("gc_conv_only", False))
    assert not R.row_table_problems(rows, shapes)[0]
    offs = np.cumsum([0] + [(int(np.prod(s)) + 3) & ~3 for s in shapes])

    def flat(tensors):
        a = np.zeros(total, np.float64)
        for t, o in zip(tensors, offs):
            a[o:o + t.numel()] = t.numpy().ravel()
        return a

    p = flat(ref.opt_case_tensors(0))
    m, v, slow = np.zeros(total), np.zeros(total), p.copy()
    seen = 0
    for step in range(1, c["nsteps"] + 1):
        gr = flat(ref.opt_case_tensors(step)).astype(np.float32)
        gsq = np.float32((np.float64(gr) ** 2).sum())
        sc = R.class_scalars(step, c["lr"], max_norm=c["max_norm"], **kw)
        out = R.step_ref64(p, gr, m, v, slow, rows, sc, gsq)
        p, m, v, slow = (out[k].x for k in R.NAMES)
        if f"s{step}.norm" in g.files:
            seen += 1
            assert abs(np.sqrt(float(gsq)) - float(g[f"s{step}.norm"][0])) <= 1e-5 * float(g[f"s{step}.norm"][0])
            for i, (s, o) in enumerate(zip(shapes, offs)):
                n = int(np.prod(s))
                assert np.abs(p[o:o + n] - g[f"s{step}.p{i}"].ravel()).max() <= 1e-6, (step, i)
    assert seen
    for i, (s, o) in enumerate(zip(shapes, offs)):
        n = int(np.prod(s))
        assert np.abs(m[o:o + n] - g[f"final.m{i}"].ravel()).max() <= 1e-6
        assert np.abs(v[o:o + n] - g[f"final.v{i}"].ravel()).max() <= 1e-6
        assert np.abs(slow[o:o + n] - g[f"final.slow{i}"].ravel()).max() <= 1e-6


def test_radam_scalars_follow_the_reference_formula():
    from hs_pose_amd.solver import _radam_step_size
    for step in (1, 5, 6, 7, 20, 1000):
        a, s = R.radam_scalars(step, 0.95, 0.999)
        b, t = _radam_step_size(step, 0.95, 0.999, 5)
        assert a == int(b) and s == t
    assert [R.radam_scalars(s, 0.95, 0.999)[0] for s in range(1, 9)] == [0] * 5 + [1] * 3


def test_sumsq_depth_and_sentinels():
    Q = R.SUMSQ_Q
    assert R.sumsq_blocks(Q) == 1024 and R.sumsq_blocks(Q - 4) == 1024 and R.sumsq_blocks(Q - 1024) == 1023
    assert R.sumsq_depth(Q) == 1 + 1 + 1 + 2 + 6 + 2 + 4 + 6 + 2 and R.sumsq_depth(Q + 4) == R.sumsq_depth(Q) + 1
    assert R.sumsq_depth(R.SUMSQ_SIZES[-1]) == R.sumsq_depth(Q) + 3           # some blocks make a fourth trip
    x, pos = R.sumsq_input(R.SUMSQ_SIZES[-1])
    n = x.size
    assert pos == sorted({0, 1024, 2047, Q, n - 4, n - 3, n - 1})
    small = np.delete(np.float64(x), pos)
    # one sentinel dropped or doubled moves the sum by 4096 of ~ 28672 + n 2^-24: far outside 2 D U sum
    assert 4096.0 > 50 * 2 * R.sumsq_depth(n) * R.U * float((np.float64(x) ** 2).sum())
    assert np.abs(small).max() <= 2.0 ** -12 and np.abs(small).min() >= 2.0 ** -13
