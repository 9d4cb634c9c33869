"""GPU: the three scoring entry points (hsp_eval_pairs / hsp_eval_match / hsp_eval_ap, csrc/eval.hip) called directly with
synthetic tables, at the sizes of a real run and on exact ties -- what the fixture and the random runs of test_gpu_eval_metrics.py
(at most 6 per group, about 25 per class, every value 1e-6 from every threshold) never reach.  Both sides read the same arrays, and
every output is an integer table or a sum in a stated order (tests/_eval_ref.py: contract_sum, which
test_eval_metrics_host.py pins to this numpy's np.sum), so every comparison is an equality.  The one exception is PAIR_BOUND, the
regime of test_gpu_eval_metrics.py, for the two pair cases whose degree is an arccos of rounded products."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_cases as cases  # noqa: E402
import _eval_ref  # noqa: E402

pytestmark = pytest.mark.gpu
PAIR_BOUND = 1e-7               # test_gpu_eval_metrics.py's: a tenth of the fixtures' margin; not a measurement


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ------------------------------------------------------------------------------------------------------------------------------
# hsp_eval_ap
# ------------------------------------------------------------------------------------------------------------------------------

def _hits(rng, n, kind):
    """one column of one class, in score order"""
    if kind == "all":                               # total == G: no sentinel term
        return np.ones(n, bool)
    if kind == "none":                              # the sentinel term alone
        return np.zeros(n, bool)
    if kind == "half":
        return rng.uniform(size=n) < 0.5
    if kind == "sparse":                            # most 256-thread chunks hold no hit: their envelope comes from later chunks
        return rng.uniform(size=n) < 0.02
    assert kind == "tail"                           # the envelope of every slot is set from the far right
    h = np.zeros(n, bool)
    k = min(n, 10)
    h[n - k:] = rng.uniform(size=k) < 0.7
    if n:
        h[n - 1 - int(rng.integers(0, k))] = True
    return h


FIVE = ("all", "none", "half", "sparse", "tail")


def ap_case(sizes, gts, columns, seed):
    """Classes of ``sizes`` slots with ``gts`` ground truths (None: as many as slots, so that an 'all' column has total == G; 0: no
    column holds a hit, as real matches cannot exceed G).  The slots lie class-interleaved in memory -- slot i of class c comes
    before slot i + 1 of every class --, so ``order`` is no identity and ``seg_off`` gathers.
    -> dict(match (slots, T) int8, order, seg_off, gt_count, want (C, T))"""
    rng = np.random.default_rng(seed)
    C, T = len(sizes), len(columns)
    gt_count = np.array([n if g is None else g for n, g in zip(sizes, gts)], np.int32)
    hit = [np.stack([_hits(rng, n, "none" if g == 0 else k) for k in columns], axis=1) if n else np.zeros((0, T), bool)
           for n, g in zip(sizes, gt_count)]                           # per class (n, T), rows in score order
    owner = np.concatenate([np.full(n, c) for c, n in enumerate(sizes)])
    rank = np.concatenate([np.arange(n) for n in sizes])
    by_memory = np.lexsort((owner, rank))                              # the (class, rank) pairs in memory order
    slot = np.empty(len(owner), np.int64)
    slot[by_memory] = np.arange(len(owner))                            # slot[k]: where pair k (class-major, by rank) lies
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    match = np.full((len(owner), T), -1, np.int8)
    values = (np.arange(len(owner)) % 3).astype(np.int8)[:, None]      # a match is any value > -1, 0 included
    match[slot] = np.where(np.concatenate(hit), values, np.int8(-1))
    for h, g in zip(hit, gt_count):
        assert np.all(h.sum(axis=0) <= g)
    want = np.stack([_eval_ref.average_precision(h.T, int(g), summer=_eval_ref.contract_sum) for h, g in zip(hit, gt_count)])
    return dict(match=match, order=slot.astype(np.int32), seg_off=seg_off, gt_count=gt_count, want=want, sizes=sizes)


def run_ap(case):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    slots, T = case["match"].shape
    C = len(case["gt_count"])
    match, order = _dev(case["match"]), _dev(case["order"])
    seg_off, gt_count = _dev(case["seg_off"]), _dev(case["gt_count"])
    aps = torch.full((C + 2, T), 7.0, dtype=torch.float64, device="cuda")                # every entry must be written
    nb = lib().hsp_eval_ap_workspace_bytes(slots, T, C)
    assert nb == 8 * T * (slots + C)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ops._run("hsp_eval_ap", (ops._p(match), slots, T, ops._p(order), ops._p(seg_off), ops._p(gt_count), C, ops._p(aps), ops._p(ws), nb,
                             ops._stream()))
    return aps.cpu().numpy()


def check_ap(case):
    got = run_ap(case)
    want, sizes, gt = case["want"], case["sizes"], case["gt_count"]
    for c in range(len(sizes)):
        assert np.array_equal(got[c + 1], want[c], equal_nan=True), \
            f"class {c} (n = {sizes[c]}, G = {gt[c]}): got {got[c + 1].tolist()}, want {want[c].tolist()}"
        if sizes[c] == 0:
            assert not got[c + 1].any()
        elif gt[c] == 0:
            assert np.isnan(got[c + 1]).all()
    assert not got[0].any() and not np.signbit(got[0]).any()
    with np.errstate(invalid="ignore"):
        mean = np.mean(got[1:-1], axis=0)
    assert np.array_equal(got[-1], mean, equal_nan=True), f"mean row: got {got[-1].tolist()}, np.mean {mean.tolist()}"
    return got


# every class length at which eval_ap_kernel or its sum changes path: one slot per thread up to 256 and chunks beyond, one block of
# the sum up to 128 terms and halves beyond, one piece up to 8192 terms and several beyond; an empty class; classes without ground truth
AP_CALLS = {
    "20000": ((20000, 1, 0, 257, 7, 1000), (None, None, 5, None, None, None), FIVE),
    "8192": ((8191, 8192, 8193, 8200, 128, 129), (None,) * 6, FIVE),
    "16385": ((16385, 8, 255, 256, 511, 513), (None,) * 6, FIVE),
    "no_gt": ((1000, 300, 0, 64, 2, 130), (None, 0, 0, None, None, None), FIVE),
    "nine_by_three": ((1000, 129, 0, 257, 8, 40, 513, 7, 300), (1003, 140, 2, 300, 8, 41, 600, 9, 301), ("half", "sparse", "tail")),
}


@pytest.mark.parametrize("name", list(AP_CALLS))
def test_ap_equals_the_contract_at_run_sizes(name):
    sizes, gts, columns = AP_CALLS[name]
    got = check_ap(ap_case(sizes, gts, columns, seed=sorted(AP_CALLS).index(name)))
    assert got.shape == (len(sizes) + 2, len(columns))


def test_ap_wide_rows():
    """the pose table's own width: 62 x 22 columns, the stride of ``order * T + t``; one class of 300 slots, hit rates from 0 to 1"""
    rng = np.random.default_rng(77)
    n, T = 300, 62 * 22
    hit = rng.uniform(size=(n, T)) < np.linspace(0.0, 1.0, T)[None, :]
    hit[:, 0], hit[:, -1] = False, True
    order = rng.permutation(n).astype(np.int32)
    match = np.full((n, T), -1, np.int8)
    match[order] = np.where(hit, np.int8(4), np.int8(-1))
    want = _eval_ref.average_precision(hit.T, n, summer=_eval_ref.contract_sum)[None, :]
    got = check_ap(dict(match=match, order=order, seg_off=np.array([0, n], np.int32), gt_count=np.array([n], np.int32), want=want,
                        sizes=(n,)))
    assert got[1, 0] == 0 and got[1, -1] > 0.99


@pytest.mark.parametrize("C", [6, 9, 20])
def test_ap_mean_row_of_a_single_column(C):
    """T == 1: np.mean along axis 0 of a (C, 1) array is a contiguous run, which numpy adds as np.sum does -- from 8 classes on that is
    not the running sum.  The seeds are chosen so that for C >= 8 the running sum of the class rows is NOT np.mean's value."""
    sizes = tuple(30 + 7 * c for c in range(C))
    case = ap_case(sizes, tuple(n + 1 + c for c, n in enumerate(sizes)), ("half",), seed={6: 0, 9: 7, 20: 7}[C])
    running = np.float64(0.0)
    for v in case["want"][:, 0]:
        running = running + v
    assert (running / C != np.mean(case["want"], axis=0)[0]) == (C >= 8), "the case does not tell the two orders apart"
    check_ap(case)


# ------------------------------------------------------------------------------------------------------------------------------
# hsp_eval_match
# ------------------------------------------------------------------------------------------------------------------------------

GROUP_SHAPES = [(1, 1), (1, 32), (32, 1), (32, 32), (31, 17), (5, 0), (0, 4), (7, 9), (12, 5), (20, 20), (3, 30), (9, 9)]
T_IOU = 300
IOU_THR = np.linspace(0.0, 0.9, T_IOU, dtype=np.float32)          # 300 thresholds: lanes 0 .. 43 make a second trip
DEG_THR = [float(x) for x in cases.DEG] + [360.0]                  # production's 62 x 22
SHIFT_THR = [float(x) for x in cases.SHIFT] + [100.0]


def make_match_tables():
    """One table of groups for all the match tests.  IoU entries come from fifteen values, five of them thresholds themselves (a
    third of the entries equal a threshold: neither < nor >, the walk goes on), plus a few NaN and 0: rows are full of ties.  Degree
    and shift lie on grids that hold the thresholds, so the sums tie and values equal thresholds; a few are NaN.  Scores come from
    eight values, so they repeat inside a group; one is NaN."""
    rng = np.random.default_rng(5)
    table = np.zeros((len(GROUP_SHAPES), 6), np.int32)
    n_p, n_g = np.array(GROUP_SHAPES).T
    table[:, 0], table[:, 1] = np.cumsum(n_p) - n_p, n_p
    table[:, 2], table[:, 3] = np.cumsum(n_g) - n_g, n_g
    table[:, 4] = np.cumsum(n_p * n_g) - n_p * n_g
    pairs = int((n_p * n_g).sum())
    on = IOU_THR[[10, 11, 50, 150, 299]]
    off = np.array([0.0351, 0.2, 0.31, 0.47, 0.6, 0.77, 0.85, 0.95, 1.0, 0.015], np.float32)
    assert not np.isin(off, IOU_THR).any()
    iou = rng.choice(np.concatenate([on, off]), size=pairs).astype(np.float32)
    iou[rng.uniform(size=pairs) < 0.02] = np.nan
    iou[rng.uniform(size=pairs) < 0.03] = 0.0
    degree = rng.integers(0, 70, size=pairs).astype(np.float64)
    shift = rng.integers(0, 26, size=pairs) / 2.0
    degree[rng.uniform(size=pairs) < 0.02] = np.nan
    shift[rng.uniform(size=pairs) < 0.02] = np.nan
    scores = rng.integers(1, 9, size=int(n_p.sum())) / 8.0
    scores[table[4, 0] + 3] = np.nan                                 # in the (31, 17) group
    assert np.isin(iou, IOU_THR).mean() > 0.3 and np.isin(degree, DEG_THR).mean() > 0.5 and np.isin(shift, SHIFT_THR).mean() > 0.5
    return dict(table=table, iou=iou, degree=degree, shift=shift, scores=scores)


@pytest.fixture(scope="module")
def match_tables():
    return make_match_tables()


def run_match(tb, deg_thr, shift_thr, pose_index):
    from hs_pose_amd import ops
    table = tb["table"]
    n_groups, P, G = len(table), int(table[:, 1].sum()), int(table[:, 3].sum())
    D1, S1 = len(deg_thr), len(shift_thr)
    TP = D1 * S1
    i8 = lambda *s: torch.full(s, 77, dtype=torch.int8, device="cuda")                    # every entry must be written
    f64 = lambda *s: torch.full(s, 77.0, dtype=torch.float64, device="cuda")
    groups, sc, iou, deg, shift = _dev(table), _dev(tb["scores"]), _dev(tb["iou"]), _dev(tb["degree"]), _dev(tb["shift"])
    it, dt, st = _dev(IOU_THR), _dev(deg_thr, np.float64), _dev(shift_thr, np.float64)
    order, ssort, pscore = i8(P), f64(P), f64(P)
    ipm, igm, ppm, pgm = i8(P, T_IOU), i8(G, T_IOU), i8(P, TP), i8(G, TP)
    kept = torch.full((n_groups, 2), 77, dtype=torch.int32, device="cuda")
    ops._run("hsp_eval_match", (ops._p(groups), n_groups, int(table[:, [1, 3]].max()), ops._p(sc), ops._p(iou), ops._p(deg), ops._p(shift),
                                ops._p(it), T_IOU, ops._p(dt), D1, ops._p(st), S1, pose_index, ops._p(order), ops._p(ssort), ops._p(ipm),
                                ops._p(igm), ops._p(ppm), ops._p(pgm), ops._p(pscore), ops._p(kept), ops._stream()))
    return {k: v.cpu().numpy() for k, v in dict(order=order, ssort=ssort, pscore=pscore, ipm=ipm, igm=igm, ppm=ppm, pgm=pgm, kept=kept).items()}


@pytest.mark.parametrize("pose_index,production", [(-1, True), (10, True), (299, True), (0, False), (10, False), (-1, False)])
def test_match_equals_the_contract_on_ties(match_tables, pose_index, production):
    """pose_index 299 belongs to a lane on its second trip; 62 x 22 is production's pose table, 1 x 1 the smallest.  What the ties
    decide: an IoU equal to its threshold must not match (the candidates after it, in descending order, cannot match either, so
    walking on and stopping there are the same function); among equal IoUs the higher index goes first, among equal degree +
    shift sums the lower; a degree or shift equal to its threshold passes."""
    tb = match_tables
    deg_thr, shift_thr = (DEG_THR, SHIFT_THR) if production else ([5.0], [2.0])
    TP = len(deg_thr) * len(shift_thr)
    got = run_match(tb, deg_thr, shift_thr, pose_index)
    kept_somewhere = 0
    for g, (p_off, n_p, g_off, n_g, pair_off, _) in enumerate(tb["table"].tolist()):
        pairs = slice(pair_off, pair_off + n_p * n_g)
        sc = tb["scores"][p_off:p_off + n_p]
        want = _eval_ref.match_group(sc, tb["iou"][pairs].reshape(n_p, n_g), tb["degree"][pairs].reshape(n_p, n_g),
                                     tb["shift"][pairs].reshape(n_p, n_g), IOU_THR, deg_thr, shift_thr, pose_index)
        where = f"group {g} ({n_p} x {n_g})"
        P, Q = slice(p_off, p_off + n_p), slice(g_off, g_off + n_g)
        kp, kg = len(want["kp"]), len(want["kg"])
        kept_somewhere += kp
        assert np.array_equal(got["order"][P], want["order"]), where
        assert np.array_equal(got["ssort"][P], sc[want["order"]], equal_nan=True), where
        assert np.array_equal(got["ipm"][P].T, want["iou_pred"]), where
        assert np.array_equal(got["igm"][Q].T, want["iou_gt"]), where
        assert got["kept"][g].tolist() == [kp, kg], where
        assert np.array_equal(got["ppm"][p_off:p_off + kp].T, want["pose_pred"].reshape(TP, kp)), where
        assert np.array_equal(got["pgm"][g_off:g_off + kg].T, want["pose_gt"].reshape(TP, kg)), where
        assert np.all(got["ppm"][p_off + kp:p_off + n_p] == -1) and np.all(got["pgm"][g_off + kg:g_off + n_g] == -1), where
        assert np.array_equal(got["pscore"][p_off:p_off + kp], sc[want["kp"]], equal_nan=True), where
        assert not got["pscore"][p_off + kp:p_off + n_p].any(), where
        if n_p * n_g == 0:                                             # no pair entries: nothing matches, everything is written
            assert np.all(got["ipm"][P] == -1) and np.all(got["igm"][Q] == -1) and np.all(got["ppm"][P] == -1) and np.all(got["pgm"][Q] == -1)
            assert got["kept"][g].tolist() == ([n_p, n_g] if pose_index < 0 else [0, 0]), where
    assert kept_somewhere > 0, "the case keeps nothing: the pose stage would be compared on empty tables"


# ------------------------------------------------------------------------------------------------------------------------------
# hsp_eval_pairs
# ------------------------------------------------------------------------------------------------------------------------------

def run_pairs(groups):
    """groups: [(kind, [(RT, scale)] predictions, [(RT, scale, handle)] ground truths)] -> per group (ours, the contract's), each
    (iou, degree, shift) of shape (np, ng)"""
    from hs_pose_amd import ops
    table, off = [], [0, 0, 0]
    for kind, preds, gts in groups:
        table.append([off[0], len(preds), off[1], len(gts), off[2], kind])
        off = [off[0] + len(preds), off[1] + len(gts), off[2] + len(preds) * len(gts)]
    pRT = np.array([p[0] for _, ps, _ in groups for p in ps], np.float64)
    psc = np.array([p[1] for _, ps, _ in groups for p in ps], np.float64)
    gRT = np.array([g[0] for _, _, gs in groups for g in gs], np.float64)
    gsc = np.array([g[1] for _, _, gs in groups for g in gs], np.float64)
    ghv = np.array([g[2] for _, _, gs in groups for g in gs], np.int32)
    d = [_dev(a) for a in (pRT, psc, gRT, gsc, ghv, np.array(table, np.int32))]
    iou = torch.full((off[2],), 7.0, dtype=torch.float32, device="cuda")
    deg, shift = (torch.full((off[2],), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    ops._run("hsp_eval_pairs", tuple(ops._p(t) for t in d) + (len(table), max(max(r[1], r[3]) for r in table), ops._p(iou), ops._p(deg),
                                                              ops._p(shift), ops._stream()))
    out = []
    for (kind, preds, gts), r in zip(groups, table):
        q = slice(r[4], r[4] + r[1] * r[3])
        ours = tuple(t.cpu().numpy()[q].reshape(r[1], r[3]) for t in (iou, deg, shift))
        want = _eval_ref.pair_values([p[0] for p in preds], [p[1] for p in preds], [g[0] for g in gts], [g[1] for g in gts],
                                     [g[2] for g in gts], kind)
        out.append((ours, want))
    return out


def test_pairs_whose_value_no_rounding_decides():
    """Identity rotations, extents and centres that are small dyadic numbers: every product and sum on the way is exact, in the
    kernel's order and in numpy's.  The eight intervals of the box (0, 0, 2) +- (0.5, 1, 2) are at least 1 long, two of them
    exactly 1: moved by (1, 1, 1) it touches the first, moved by (10, 10, 10) every interval lies apart."""
    size = [1.0, 2.0, 4.0]
    at = lambda *t: cases.rt(np.eye(3), t)
    base = at(0.0, 0.0, 2.0)
    gt = [(base, size, 1)]
    groups = [(0, [(base, size)], gt),                                 # the same box
              (0, [(at(10.0, 10.0, 12.0), size)], gt),                 # apart in every interval
              (0, [(at(1.0, 1.0, 3.0), size)], gt),                    # touching
              (0, [(at(0.375, 0.5, 2.0), [0.5, 0.25, 1.0])], gt),      # 3-4-5: the centres are 0.625 apart
              (3, [(at(0.375, 0.5, 2.0), size), (base, size)], [(base, size, 1), (at(1.0, 1.0, 3.0), size, 0)])]
    res = run_pairs(groups)
    for (ours, want), name in zip(res, ("same", "apart", "touching", "3-4-5", "2 x 2")):
        for a, b, k in zip(ours, want, ("iou", "degree", "shift")):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"{name}: {k}: {a.tolist()} != {b.tolist()}"
    value = lambda g: tuple(float(t[0, 0]) for t in res[g][0])
    assert value(0) == (1.0, 0.0, 0.0)
    assert value(1)[0] == 0.0 and value(1)[2] == math.sqrt(300.0) * 100
    assert value(2)[0] == 0.0
    assert value(3)[1:] == (0.0, 62.5)
    assert res[4][0][0][1].tolist() == [1.0, 0.0] and res[4][0][2][0, 0] == 62.5     # a half turn about y changes neither (kind 3)


def test_pairs_take_the_branch_of_their_kind():
    """a mug with and without a visible handle, and a phone seen from behind.  The predictions are tilted by 0.1 rad about x as well,
    which keeps every arccos argument away from +-1 (the margin rule of tests/_eval_cases.py): the degrees then differ between the
    branches by far more than PAIR_BOUND, and between the kernel and numpy by far less."""
    rng = np.random.default_rng(11)
    ry = lambda a: cases.rot([0, 1, 0], np.rad2deg(a))
    tilt = cases.rot([1, 0, 0], np.rad2deg(0.1))
    R = cases.rand_rot(rng)
    t = np.array([0.05, -0.1, 1.2])
    size = [0.8, 0.7, 0.6]
    mug = (cases.rt(R @ ry(0.3) @ tilt, t + [0.01, 0.0, 0.02]), [0.25, 0.2, 0.2])
    phone = (cases.rt(R @ ry(math.pi + 0.2) @ tilt, t + [0.0, 0.01, 0.0]), [0.25, 0.2, 0.2])
    g = lambda hv: [(cases.rt(R, t, 0.3), size, hv)]
    groups = [(2, [mug], g(0)), (2, [mug], g(1)), (3, [phone], g(1)), (0, [phone], g(1)), (1, [mug], g(1))]
    res = run_pairs(groups)
    for (ours, want), name in zip(res, ("mug, handle hidden", "mug, handle visible", "phone", "phone as camera", "mug as bottle")):
        for a, b, k in zip(ours, want, ("iou", "degree", "shift")):
            assert not np.isnan(a).any() and not np.isnan(b).any(), f"{name}: {k}"
            worst = float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))
            print(f"eval pairs, {name}: {k}: ours {a.tolist()}, |ours - contract| = {worst:.3e}")
            assert worst <= PAIR_BOUND, f"{name}: {k}"
    deg = [float(ours[1][0, 0]) for ours, _ in res]
    tilt_only = np.rad2deg(0.1)
    assert abs(deg[0] - tilt_only) < 0.5 and deg[1] > 15                  # hidden: the angle between the y axes; visible: the whole turn
    assert deg[4] == deg[0] and res[4][0][0][0, 0] == res[0][0][0][0, 0]    # the hidden-handle mug is a bottle, bit for bit
    assert res[0][0][0][0, 0] >= res[1][0][0][0, 0]                        # and its IoU is the best of twenty turns, the plain one among them
    assert deg[2] < 20 and deg[3] > 160                                   # the flipped branch; without it the same pair is a half turn
