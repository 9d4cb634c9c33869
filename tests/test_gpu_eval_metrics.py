"""GPU: hs_pose_amd.evaluation (hsp_eval_pairs / hsp_eval_match / hsp_eval_ap) against what the reference computed for the
fixture (tests/golden/eval_*, tools/gen_golden_eval.py) and against the contract in numpy (tests/_eval_ref.py) on random small
runs.  Match tables and the prediction order must be EQUAL: the fixture and the random runs keep every pair value 1e-6 from every
threshold (tests/_eval_cases.py: margins), so a pair value within 1e-7 of the reference's cannot change a match."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
TABLES = ("group_class", "group_image", "group_np", "group_ng", "kept_np", "kept_ng", "order", "iou_pred", "iou_gt", "pose_pred", "pose_gt")
PAIR_BOUND = 1e-7               # a tenth of the fixture's margin; not a measurement


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


@pytest.fixture(scope="module")
def ours(golden):
    """both settings of use_matches_for_pose run once: {use: (iou_aps, pose_aps, matches)}"""
    from hs_pose_amd.evaluation import PoseEvaluator
    results, _, _, man = golden
    out = {}
    for use in (True, False):
        ev = PoseEvaluator(man["synset_names"], man["degree_thresholds"], man["shift_thresholds"], man["iou_3d_thresholds"],
                           man["iou_pose_thres"], use)
        ev.add_results(results)
        out[use] = ev.compute() + (ev.matches(),)
    return out


def _same_tables(got, want):
    for k in TABLES:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), f"{k}: {int((got[k] != want[k]).sum())} entries differ"


def test_pair_values(golden, ours):
    det = golden[2]
    m = ours[False][2]
    for k in ("iou", "degree", "shift"):
        got, want = m[k].astype(np.float64), det[k].astype(np.float64)
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), k
        worst = float(np.nanmax(np.abs(got - want)))
        print(f"eval pair values: {k}: max |ours - reference| = {worst:.3e}")
        assert worst <= PAIR_BOUND, k
    assert np.array_equal(ours[True][2]["iou"], m["iou"])
    assert np.all(m["iou"][det["iou"] == 0] == 0)                      # a disjoint pair is exactly 0


@pytest.mark.parametrize("use_matches", [True, False])
def test_match_tables_equal_the_reference(golden, ours, use_matches):
    _same_tables(ours[use_matches][2], golden[1] if use_matches else golden[2])


@pytest.mark.parametrize("use_matches", [True, False])
def test_ap_arrays_equal_the_reference(golden, ours, use_matches):
    """the kernel adds the terms in np.sum's own order, so the arrays are the reference's bit for bit"""
    gold = golden[1] if use_matches else golden[2]
    iou_aps, pose_aps, _ = ours[use_matches]
    for got, want, k in ((iou_aps, gold["iou_aps"], "iou_aps"), (pose_aps, gold["pose_aps"], "pose_aps")):
        assert got.shape == want.shape and got.dtype == np.float64
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        print(f"eval {k}: max |ours - reference| = {float(np.nanmax(np.abs(got - want))):.3e}")
        assert np.array_equal(got, want, equal_nan=True), k


@pytest.fixture(scope="module")
def random_runs():
    """twenty small runs of 1 to 8 images under the margin conditions, with what tests/_eval_ref.py makes of them; group sizes
    include 1 and exactly the library's cap"""
    from hs_pose_amd.evaluation import group_cap
    L = group_cap()
    rng = np.random.default_rng(20)
    runs = []
    for k in range(20):
        synset = cases.SYNSET_FLIP if k % 2 else cases.SYNSET
        sizes = {0: [(1, L, L)], 1: [(2, L, 1), (4, 1, L)], 2: [(3, 1, 1), (1, 1, 1)], 3: [(2, L, 3)]}.get(k, [])
        n_images = int(rng.integers(1, 9)) - len(sizes)
        res, flat = cases.random_run_with_margins(100 + k, synset, max(n_images, 0), sizes)
        runs.append((synset, res, flat))
    return runs


def test_random_runs_equal_the_contract(random_runs):
    from hs_pose_amd.evaluation import PoseEvaluator
    for synset, res, flat in random_runs:
        ev = PoseEvaluator(synset, cases.DEG, cases.SHIFT, cases.IOU, 0.1, True)
        ev.add_results(res)
        iou_aps, pose_aps = ev.compute()
        _same_tables(ev.matches(), flat)
        assert np.array_equal(iou_aps, flat["iou_aps"], equal_nan=True) and np.array_equal(pose_aps, flat["pose_aps"], equal_nan=True)


def test_group_above_the_cap_is_refused_before_any_launch(monkeypatch):
    from hs_pose_amd import evaluation
    from hs_pose_amd._lib import HspError
    L = evaluation.group_cap()
    rng = np.random.default_rng(3)
    res = cases.random_run(rng, cases.SYNSET, 2) + cases.random_run(rng, cases.SYNSET, 0, [(3, L + 1, 2)])
    launched = []
    monkeypatch.setattr(evaluation, "_run", lambda name, *a, **k: launched.append(name))
    ev = evaluation.PoseEvaluator(cases.SYNSET, cases.DEG, cases.SHIFT, cases.IOU)
    ev.add_results(res)
    with pytest.raises(HspError, match=rf"image 2 holds {L + 1} predictions and 2 ground truths of class 'camera'"):
        ev.compute()
    assert launched == []


def test_one_image_at_a_time_with_device_tensors(golden, ours):
    from hs_pose_amd.evaluation import PoseEvaluator
    results, _, _, man = golden
    dev = torch.device("cuda")
    ev = PoseEvaluator(man["synset_names"], man["degree_thresholds"], man["shift_thresholds"], man["iou_3d_thresholds"], man["iou_pose_thres"], True)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    for r in results:
        n = len(r["pred_class_ids"])
        ev.add(t(r["pred_RTs"], torch.float64), t(np.asarray(r["pred_scales"]).reshape(n, -1)[:, :3] if n else np.zeros((0, 3)), torch.float64),
               t(r["pred_scores"], torch.float64), t(r["pred_class_ids"], torch.int64), r["gt_class_ids"], t(r["gt_RTs"], torch.float64),
               t(r["gt_scales"], torch.float64), t(r["gt_handle_visibility"], torch.int32))
    iou_aps, pose_aps = ev.compute()
    assert np.array_equal(iou_aps, ours[True][0], equal_nan=True) and np.array_equal(pose_aps, ours[True][1], equal_nan=True)
    m, w = ev.matches(), ours[True][2]
    assert all(np.array_equal(m[k], w[k], equal_nan=True) for k in w)


def test_drop_in_function_and_headline(golden, tmp_path):
    from hs_pose_amd.evaluation import compute_degree_cm_mAP, headline
    results, only, _, man = golden
    args = (man["synset_names"], str(tmp_path), man["degree_thresholds"], man["shift_thresholds"], man["iou_3d_thresholds"])
    iou_aps, pose_aps = compute_degree_cm_mAP(results, *args, iou_pose_thres=0.1, use_matches_for_pose=True)
    assert np.array_equal(iou_aps, only["iou_aps"], equal_nan=True) and np.array_equal(pose_aps, only["pose_aps"], equal_nan=True)
    saved = np.load(tmp_path / "mAP_data.npz")
    assert sorted(saved.files) == ["degree_thres_list", "iou_3d_aps", "iou_thres_list", "pose_aps", "shift_thres_list"]
    assert np.array_equal(saved["pose_aps"], pose_aps, equal_nan=True) and list(saved["degree_thres_list"]) == man["degree_thresholds"] + [360]
    # evaluate.py:143-169, written out: the mean row is NaN for the IoU figures here (a class without ground truth), so a class row too
    dl, sl, il = man["degree_thresholds"], man["shift_thresholds"], man["iou_3d_thresholds"]
    for idx in (-1, 2):
        want = [iou_aps[idx, il.index(0.25)], iou_aps[idx, il.index(0.5)], iou_aps[idx, il.index(0.75)],
                pose_aps[idx, dl.index(5), sl.index(2)], pose_aps[idx, dl.index(5), sl.index(5)], pose_aps[idx, dl.index(10), sl.index(2)],
                pose_aps[idx, dl.index(10), sl.index(5)], pose_aps[idx, dl.index(10), sl.index(10)], pose_aps[idx, dl.index(5), -1],
                pose_aps[idx, dl.index(10), -1], pose_aps[idx, -1, sl.index(2)], pose_aps[idx, -1, sl.index(5)], pose_aps[idx, -1, sl.index(10)]]
        got = headline(iou_aps, pose_aps, dl, sl, il, row=idx)
        assert len(got) == 13 and np.array_equal(list(got.values()), [v * 100 for v in want], equal_nan=True)
