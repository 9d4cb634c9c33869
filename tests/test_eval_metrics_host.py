"""CPU: the evaluation metrics' contract in numpy (tests/_eval_ref.py) equals what the reference computed for the fixture
(tests/golden/eval_*, tools/gen_golden_eval.py); pack_results round-trips the reference's dicts; the new entry points reject bad
arguments before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_cases as cases  # noqa: E402
import _eval_ref  # noqa: E402

TABLES = ("group_class", "group_image", "group_np", "group_ng", "kept_np", "kept_ng", "order", "iou_pred", "iou_gt", "pose_pred", "pose_gt")


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


@pytest.mark.parametrize("use_matches", [True, False])
def test_contract_in_numpy_equals_the_reference(golden, use_matches):
    results, only, det, man = golden
    gold = only if use_matches else det
    mine = _eval_ref.evaluate(results, man["synset_names"], man["degree_thresholds"], man["shift_thresholds"], man["iou_3d_thresholds"],
                              man["iou_pose_thres"], use_matches)
    for k in TABLES:
        assert mine[k].shape == gold[k].shape and np.array_equal(mine[k], gold[k]), k
    for k in ("iou_aps", "pose_aps"):
        assert np.array_equal(mine[k], gold[k], equal_nan=True), k
    for k in ("iou", "degree", "shift"):                              # (degree / shift of every pair: recorded with the False run)
        want = det[k].astype(np.float64)
        got = mine[k].astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        assert np.nanmax(np.abs(got - want)) <= 1e-12, k


def test_fixture_holds_its_cases_and_margins(golden):
    results, only, det, man = golden
    S = man["synset_names"]
    assert len(results) == 40 and max(only["group_np"].max(), only["group_ng"].max()) <= 6
    n = [(len(r["pred_class_ids"]), len(r["gt_class_ids"])) for r in results]
    assert (0, 0) in n and any(p and not g for p, g in n) and any(g and not p for p, g in n)                  # 1, 2, 3
    assert results[n.index((0, 0))]["pred_scales"].shape == (0, 4, 4)
    assert np.isnan(only["iou_aps"][S.index("laptop")]).all() and np.isnan(only["iou_aps"][-1]).all()           # 4
    assert not only["iou_aps"][S.index("cap")].any() and not only["pose_aps"][S.index("cap")].any()            # 5
    assert not only["iou_aps"][0].any() and only["iou_aps"].shape == (len(S) + 1, 101) and only["pose_aps"].shape == (len(S) + 1, 62, 22)
    for name in ("bottle", "bowl", "can"):                                                                        # 6
        assert np.any((only["group_class"] == S.index(name)) & (only["kept_np"] > 0)), name
    mugs = np.concatenate([r["gt_handle_visibility"][r["gt_class_ids"] == S.index("mug")] for r in results])
    assert {0, 1} <= set(mugs.tolist())                                                                          # 7
    assert all(abs(np.linalg.det(RT[:3, :3]) - 1) > 0.1 for r in results for RT in r["gt_RTs"])                 # 8
    m = cases.margins(det, results, S)
    assert cases.margins_ok(m, allow_above=1) and m["n_above"] == 1 and cases.scores_distinct_across_images(results)
    assert np.isnan(det["degree"]).sum() == 1                                                                    # 12
    # 9: in the two-bowl image the prediction that goes first (higher score) takes the ground truth the other one fits better
    po = np.cumsum(only["group_np"]) - only["group_np"]
    qo = np.cumsum(only["group_np"] * only["group_ng"]) - only["group_np"] * only["group_ng"]
    g = int(np.where((only["group_image"] == man["cases"]["case9_image"]) & (only["group_class"] == S.index("bowl")))[0][0])
    iou = only["iou"][qo[g]:qo[g] + 4].reshape(2, 2)
    first, second = only["order"][po[g]:po[g] + 2]
    took = only["iou_pred"][10, po[g]]
    assert iou[second, took] > iou[first, took] and only["iou_pred"][10, po[g] + 1] == 1 - took
    # 10: the duplicate prediction's two rows of the pair table are equal; 11: the group with equal scores lists the higher index first
    g = int(np.where((only["group_image"] == man["cases"]["case10_image"]) & (only["group_class"] == S.index("camera")))[0][0])
    assert only["iou"][qo[g]] == only["iou"][qo[g] + 1] and (only["iou_pred"][10, po[g]:po[g] + 2] > -1).sum() == 1
    g = int(np.where((only["group_image"] == man["cases"]["case11_image"]) & (only["group_class"] == S.index("mug")))[0][0])
    assert list(only["order"][po[g]:po[g] + 3]) in ([1, 2, 0], [2, 0, 1])


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1000, 8191, 8192, 8193, 8200, 16384, 16385, 20000])
def test_contract_sum_is_this_numpys_sum(n):
    """The GPU tests hold hsp_eval_ap to _eval_ref.contract_sum, the header's order in scalar additions; the golden arrays come from
    np.sum.  The two must be the same bits on the numpy that runs the suite: one that adds differently fails here, not on the GPU.
    Positive terms of mixed magnitude, so that nearly every order of additions rounds differently.  Likewise the mean row of a
    one-column table (hsp_eval_ap's T == 1) against np.mean along axis 0, which is a contiguous run from 8 classes on."""
    rng = np.random.default_rng(1000 + n)
    for _ in range(3):
        a = rng.uniform(size=n) * rng.uniform(size=n)
        got, want = _eval_ref.contract_sum(a), np.sum(a)
        assert got == want, f"n = {n}: contract_sum {float(got)!r}, np.sum {float(want)!r}"
        if n:
            table = np.zeros((n + 2, 1))
            table[1:-1, 0] = a
            assert got / n == np.mean(table[1:-1], axis=0)[0], n
    hit = rng.uniform(size=(3, n)) < 0.5
    G = int(hit.sum(axis=1).max()) + 3
    assert np.array_equal(_eval_ref.average_precision(hit, G, summer=_eval_ref.contract_sum), _eval_ref.average_precision(hit, G))


def test_pack_results_round_trip(golden):
    from hs_pose_amd.evaluation import pack_results, unpack_results
    results = golden[0]
    pk = pack_results(results)
    assert pk["pred_off"][-1] == sum(len(r["pred_class_ids"]) for r in results) == len(pk["pred_scores"])
    assert pk["pred_RTs"].dtype == np.float64 and pk["gt_class_ids"].dtype == np.int32 and pk["pred_scales"].shape[1:] == (3,)
    back = unpack_results(pk)
    assert len(back) == len(results)
    for a, b in zip(back, results):
        for k in a:
            if len(b["pred_class_ids"]) == 0 and k in ("pred_RTs", "pred_scales"):
                assert a[k].shape[0] == 0                              # the (0,4,4) placeholder comes back as an empty table
            else:
                assert np.array_equal(a[k], b[k]), k
    again = pack_results(back)
    assert all(np.array_equal(pk[k], again[k]) for k in pk)
    from hs_pose_amd._lib import HspError
    bad = dict(results[3], pred_scales=results[3]["pred_scales"][:1])
    with pytest.raises(HspError, match="image 0: pred_scales"):
        pack_results([bad])


def test_entry_points_validate_arguments_without_gpu():
    from hs_pose_amd._lib import lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    cap = L.hsp_eval_group_cap()
    assert cap == 32
    pairs = lambda *a: L.hsp_eval_pairs(*a)
    assert pairs(null, one, one, one, one, one, 1, 1, one, one, one, null) == -1               # NULL pointer
    assert pairs(one, one, one, one, one, one, 0, 1, one, one, one, null) == -1                # no group
    assert pairs(one, one, one, one, one, one, 1, cap + 1, one, one, one, null) == -2          # a group above the cap
    match = lambda **k: L.hsp_eval_match(*[k.get(n, d) for n, d in (
        ("groups", one), ("n_groups", 1), ("max_group", 1), ("scores", one), ("iou", one), ("degree", one), ("shift", one), ("iou_thres", one),
        ("T", 101), ("deg_thres", one), ("D1", 62), ("shift_thres", one), ("S1", 22), ("index", 10), ("order", one), ("ssort", one),
        ("ipm", one), ("igm", one), ("ppm", one), ("pgm", one), ("pscore", one), ("kept", one), ("stream", null))])
    assert match(kept=null) == -1 and match(scores=null) == -1
    assert match(T=0) == -1 and match(D1=0) == -1 and match(S1=-3) == -1 and match(n_groups=0) == -1
    assert match(index=101) == -1                                                              # not one of the T thresholds
    assert match(max_group=cap + 1) == -2
    ap = lambda **k: L.hsp_eval_ap(*[k.get(n, d) for n, d in (
        ("match", one), ("slots", 100), ("T", 101), ("order", one), ("seg_off", one), ("gt_count", one), ("C", 6), ("aps", one), ("ws", one),
        ("ws_bytes", 1 << 30), ("stream", null))])
    assert L.hsp_eval_ap_workspace_bytes(100, 101, 6) == 8 * 101 * 106 and L.hsp_eval_ap_workspace_bytes(100, 0, 6) == 0
    assert ap(match=null) == -1 and ap(slots=0) == -1 and ap(C=0) == -1 and ap(T=0) == -1
    assert ap(slots=1 << 23) == -2
    assert ap(ws=null) == -3 and ap(ws_bytes=8 * 101 * 106 - 1) == -3


def test_no_cpu_path_and_host_side_refusals(golden):
    import torch
    from hs_pose_amd._lib import HspError
    from hs_pose_amd.evaluation import PoseEvaluator, compute_degree_cm_mAP, headline
    with pytest.raises(HspError, match="iou_pose_thres"):
        PoseEvaluator(cases.SYNSET, cases.DEG, cases.SHIFT, [0.25, 0.5], iou_pose_thres=0.1)
    ev = PoseEvaluator(cases.SYNSET, cases.DEG, cases.SHIFT, cases.IOU)
    with pytest.raises(HspError, match="GPU tensor"):
        ev.add(torch.zeros(1, 4, 4), torch.zeros(1, 3), torch.zeros(1), [1], [1], np.zeros((1, 4, 4)), np.zeros((1, 3)), [1])
    if not torch.cuda.is_available():
        with pytest.raises(HspError, match="no GPU"):
            compute_degree_cm_mAP(golden[0], cases.SYNSET)
    # headline: evaluate.py:157-169's thirteen figures, from the golden arrays
    only = golden[1]
    h = headline(only["iou_aps"], only["pose_aps"], row=1)
    i, p = only["iou_aps"], only["pose_aps"]
    want = [i[1, 25], i[1, 50], i[1, 75], p[1, 5, 4], p[1, 5, 10], p[1, 10, 4], p[1, 10, 10], p[1, 10, 20], p[1, 5, -1], p[1, 10, -1],
            p[1, -1, 4], p[1, -1, 10], p[1, -1, 20]]
    assert len(h) == 13 and list(h.values()) == [float(v) * 100 for v in want]
    assert list(h)[:4] == ["3D IoU at 25", "3D IoU at 50", "3D IoU at 75", "5 degree, 2cm"]
