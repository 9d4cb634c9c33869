"""Synthetic evaluation runs (the reference's list of result dicts) for the evaluation-metric tests and tools/gen_golden_eval.py,
and the margin conditions under which exact equality of match tables is a fair demand."""
import numpy as np

SYNSET = ["BG", "bottle", "bowl", "camera", "can", "laptop", "mug", "cap"]       # the fixture's: laptop is only ever predicted, cap absent
SYNSET_FLIP = ["BG", "bottle", "phone", "camera", "mug"]                         # random runs: with a phone / eggbox / glue class
DEG = list(range(0, 61))
SHIFT = [i / 2 for i in range(21)]
IOU = [i / 100 for i in range(101)]
MARGIN = 1e-6
ARG_MARGIN = 1e-9


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rand_rot(rng, max_deg=180.0):
    return rot(rng.normal(size=3), rng.uniform(0, max_deg))


def rt(R, t, s=1.0):
    M = np.eye(4)
    M[:3, :3] = s * np.asarray(R)
    M[:3, 3] = t
    return M


def empty_image():
    """an image with nothing in it, with the (0,4,4) placeholders evaluate.py:86-87 stores"""
    return dict(gt_class_ids=np.zeros(0, np.int32), gt_RTs=np.zeros((0, 4, 4)), gt_scales=np.zeros((0, 3)),
                gt_handle_visibility=np.zeros(0, np.int32), pred_class_ids=np.zeros(0, np.int32), pred_scales=np.zeros((0, 4, 4)),
                pred_scores=np.zeros(0), pred_RTs=np.zeros((0, 4, 4)), pred_bboxes=np.zeros((0, 4)))


def image(gts, preds):
    """gts: [(cls, RT, scale, handle)], preds: [(cls, RT, scale, score)]"""
    if not gts and not preds:
        return empty_image()
    r = dict(gt_class_ids=np.array([g[0] for g in gts], np.int32), gt_RTs=np.array([g[1] for g in gts]).reshape(-1, 4, 4),
             gt_scales=np.array([g[2] for g in gts], np.float64).reshape(-1, 3), gt_handle_visibility=np.array([g[3] for g in gts], np.int32),
             pred_class_ids=np.array([p[0] for p in preds], np.int32), pred_RTs=np.array([p[1] for p in preds]).reshape(-1, 4, 4),
             pred_scales=np.array([p[2] for p in preds], np.float64).reshape(-1, 3), pred_scores=np.array([p[3] for p in preds], np.float64),
             pred_bboxes=np.ones((len(preds), 4)))
    return r


def _near(rng, g, synset, rot_deg, shift_m):
    """a prediction near ground truth g: rotation off by up to rot_deg (plus any turn about y for the symmetric classes), centre off
    by up to shift_m, extents off by a few percent; predicted RTs carry no scale"""
    cls, RT, scale, _ = g
    s = np.cbrt(np.linalg.det(RT[:3, :3]))
    R = RT[:3, :3] / s
    R = R @ rand_rot(rng, rot_deg)
    if synset[cls] in ("bottle", "bowl", "can", "mug"):
        R = R @ rot([0, 1, 0], rng.uniform(0, 360))
    t = RT[:3, 3] + rng.normal(size=3) * shift_m / np.sqrt(3)
    return cls, rt(R, t), np.asarray(scale) * s * rng.uniform(0.9, 1.1, 3)


def random_image(rng, synset, classes, max_per_class, scores):
    gts, preds = [], []
    for cls in classes:
        n = int(rng.integers(1, max_per_class + 1))
        for _ in range(n):
            s = rng.uniform(0.2, 0.6)
            gts.append((cls, rt(rand_rot(rng), rng.uniform(-0.15, 0.15, 3) + [0, 0, 1.0], s), rng.uniform(0.3, 1.0, 3), int(rng.integers(0, 2))))
            if rng.uniform() < 0.85:
                p = _near(rng, gts[-1], synset, rng.choice([3.0, 8.0, 25.0, 90.0]), rng.choice([0.01, 0.03, 0.08]))
                preds.append(p + (scores.pop(),))
        if rng.uniform() < 0.3:                                   # a detection with nothing behind it
            preds.append((cls, rt(rand_rot(rng), rng.uniform(-0.3, 0.3, 3) + [0, 0, 1.0]), rng.uniform(0.05, 0.3, 3), scores.pop()))
    o = rng.permutation(len(gts))
    q = rng.permutation(len(preds))
    return image([gts[k] for k in o], [preds[k] for k in q])


def score_pool(rng, n):
    """n distinct scores in (0.05, 1), in random order"""
    return list(0.05 + 0.95 * (rng.permutation(n) + rng.uniform(0.1, 0.9, n)) / n)


def random_run(rng, synset, n_images, group_sizes=()):
    """a small run; group_sizes: (cls, np, ng) groups of exactly that size, one image each, ahead of the random images"""
    scores = score_pool(rng, 64 * (n_images + len(group_sizes)) + 8)
    real = [c for c in range(1, len(synset))]
    out = []
    for cls, n_p, n_g in group_sizes:
        gts = [(cls, rt(rand_rot(rng), rng.uniform(-0.2, 0.2, 3) + [0, 0, 1.0], rng.uniform(0.2, 0.6)), rng.uniform(0.3, 1.0, 3),
                int(rng.integers(0, 2))) for _ in range(n_g)]
        preds = [_near(rng, gts[int(rng.integers(0, n_g))], synset, 30.0, 0.05) + (scores.pop(),) for _ in range(n_p)]
        out.append(image(gts, preds))
    for _ in range(n_images):
        k = int(rng.integers(0, len(real) + 1))
        out.append(random_image(rng, synset, list(rng.choice(real, size=k, replace=False)), 3, scores))
    return out


def golden_run(seed):
    """the fixture: 40 images holding the twelve cases of tools/gen_golden_eval.py's docstring.  -> (results, notes)"""
    rng = np.random.default_rng(seed)
    S = SYNSET
    c = {n: S.index(n) for n in S}
    scores = score_pool(rng, 600)
    tied = 0.5123456789                                          # the one score that appears twice (case 11); the pool avoids it
    out, notes = [], {}
    out.append(empty_image())                                    # 1
    out.append(image([], [(c["camera"], rt(rand_rot(rng), [0, 0, 1.0]), [0.2, 0.1, 0.1], scores.pop()),          # 2, 4
                          (c["laptop"], rt(rand_rot(rng), [0.1, 0, 1.0]), [0.3, 0.2, 0.3], scores.pop())]))
    out.append(image([(c["bottle"], rt(rand_rot(rng), [0, 0, 1.0], 0.3), [0.3, 1.0, 0.3], 1),                     # 3
                      (c["mug"], rt(rand_rot(rng), [0.2, 0, 1.0], 0.25), [0.8, 0.7, 0.6], 0)], []))
    # 9: two bowls 4 cm apart; the lower-scored prediction fits gt 0 better than the higher-scored one, which goes first
    R = rand_rot(rng)
    g0 = (c["bowl"], rt(R, [0, 0, 1.0], 0.4), [1.0, 0.5, 1.0], 1)
    g1 = (c["bowl"], rt(R, np.array([0, 0, 1.0]) + R @ [0.04, 0, 0], 0.4), [1.0, 0.5, 1.0], 1)
    hi = (c["bowl"], rt(R @ rot([1, 0, 0], 3.3), np.array([0, 0, 1.0]) + R @ [0.015, 0.002, 0.001]), [0.4, 0.2, 0.4], 0.97123)
    lo = (c["bowl"], rt(R @ rot([0, 0, 1], 2.2), np.array([0, 0, 1.0]) + R @ [0.003, 0.001, 0.002]), [0.4, 0.2, 0.4], 0.31357)
    notes["case9_image"] = len(out)
    out.append(image([g0, g1], [lo, hi]))
    # 10: the same prediction twice (scores differ)
    g = (c["camera"], rt(rand_rot(rng), [0.1, 0.1, 0.9], 0.35), [0.6, 0.5, 0.9], 1)
    p = _near(rng, g, S, 6.0, 0.02)
    notes["case10_image"] = len(out)
    out.append(image([g], [p + (scores.pop(),), p + (scores.pop(),)]))
    # 11: equal scores inside a group -- on two detections more than a metre from every ground truth, which no threshold matches,
    # so the order among equal scores moves the prediction order (recorded) and no average precision
    g = (c["mug"], rt(rand_rot(rng), [0, 0, 1.0], 0.3), [0.8, 0.7, 0.6], 1)
    far = lambda t: (c["mug"], rt(rand_rot(rng), t), [0.2, 0.2, 0.2], tied)
    notes["case11_image"] = len(out)
    out.append(image([g], [far([2.0, 2.0, 3.0]), _near(rng, g, S, 4.0, 0.01) + (scores.pop(),), far([-2.0, 2.5, 3.0])]))
    # 12: a prediction with exactly its ground truth's rotation, the rotation as a checkpoint printed to four decimals has it (so
    # not orthogonal to 1e-4): after the division by cbrt(det) the trace of R R^T is 3 + ~1e-8 and the arccos argument above 1
    R4 = np.round(rand_rot(rng), 4)
    notes["case12_image"] = len(out)
    out.append(image([(c["camera"], rt(R4, [0, 0.1, 1.1], 0.3), [0.5, 0.4, 0.8], 1)], [(c["camera"], rt(R4, [0.004, 0.1, 1.1031]), [0.15, 0.12, 0.24], scores.pop())]))
    real = [c[n] for n in ("bottle", "bowl", "camera", "can", "mug")]
    while len(out) < 40:
        k = int(rng.integers(1, 4))
        im = random_image(rng, S, list(rng.choice(real, size=k, replace=False)), 3, scores)
        if rng.uniform() < 0.25:                                  # laptops are detected now and then, never annotated (4)
            extra = (c["laptop"], rt(rand_rot(rng), [0, 0, 1.0]), [0.3, 0.2, 0.3], scores.pop())
            im = image([(int(a), b, d, int(e)) for a, b, d, e in zip(im["gt_class_ids"], im["gt_RTs"], im["gt_scales"], im["gt_handle_visibility"])],
                       [(int(a), b, d, float(e)) for a, b, d, e in zip(im["pred_class_ids"], im["pred_RTs"], im["pred_scales"], im["pred_scores"])] + [extra])
        out.append(im)
    return out, notes


def arccos_arguments(results, synset):
    """the argument of every arccos the degree computation takes, over all same-class pairs of every image"""
    from _eval_ref import kind_of
    args = []
    for r in results:
        for i, pc in enumerate(r["pred_class_ids"]):
            for j, gc in enumerate(r["gt_class_ids"]):
                if pc != gc or not 1 <= pc < len(synset):
                    continue
                A, B = np.asarray(r["pred_RTs"][i], np.float64), np.asarray(r["gt_RTs"][j], np.float64)
                R1 = A[:3, :3] / np.cbrt(np.linalg.det(A[:3, :3]))
                R2 = B[:3, :3] / np.cbrt(np.linalg.det(B[:3, :3]))
                kind = kind_of(synset[pc])
                if kind == 1 or (kind == 2 and r["gt_handle_visibility"][j] == 0):
                    y1, y2 = R1[:, 1], R2[:, 1]
                    args.append(y1.dot(y2) / (np.linalg.norm(y1) * np.linalg.norm(y2)))
                else:
                    args.append((np.trace(R1 @ R2.T) - 1) / 2)
                    if kind == 3:
                        args.append((np.trace(R1 @ np.diag([-1.0, 1.0, -1.0]) @ R2.T) - 1) / 2)
    return np.array(args)


def margins(flat, results, synset, deg_thr=DEG, shift_thr=SHIFT, iou_thr=IOU):
    """the smallest distances the conditions speak of: dict(iou, degree, shift, arccos_inside, arccos_above, n_above).  ``flat``: the
    output of ``_eval_ref.evaluate`` (or the golden) for ``results``"""
    dist = lambda v, thr: float(np.min(np.abs(v[:, None] - np.asarray(thr, np.float64)[None, :]))) if len(v) else np.inf
    iou = flat["iou"].astype(np.float64)
    deg, shift = flat["degree"], flat["shift"]
    a = arccos_arguments(results, synset)
    above = a[a > 1 - ARG_MARGIN]
    inside = a[a <= 1 - ARG_MARGIN]
    return dict(iou=dist(iou[iou != 0], iou_thr), degree=dist(deg[~np.isnan(deg)], list(deg_thr) + [360]),
                shift=dist(shift[~np.isnan(shift)], list(shift_thr) + [100]),
                arccos_inside=float(1 - np.max(np.abs(inside))) if len(inside) else np.inf,
                arccos_above=float(np.min(above) - 1) if len(above) else np.inf, n_above=int(len(above)))


def margins_ok(m, allow_above=0):
    """every value a match depends on is MARGIN from every threshold; every arccos argument is ARG_MARGIN inside [-1, 1], but for
    ``allow_above`` arguments that lie at least 1e-10 ABOVE 1 (NaN wherever it is computed)"""
    return (m["iou"] >= MARGIN and m["degree"] >= MARGIN and m["shift"] >= MARGIN and m["arccos_inside"] >= ARG_MARGIN
            and m["n_above"] <= allow_above and (m["n_above"] == 0 or m["arccos_above"] >= 1e-10))


def scores_distinct_across_images(results):
    seen = {}
    for im, r in enumerate(results):
        for s in np.asarray(r["pred_scores"]).reshape(-1):
            if seen.setdefault(float(s), im) != im:
                return False
    return True


def random_run_with_margins(seed, synset, n_images, group_sizes=()):
    """rejection: redraw until the conditions hold.  -> (results, flat reference result)"""
    import _eval_ref
    for k in range(200):
        rng = np.random.default_rng([seed, k])
        res = random_run(rng, synset, n_images, group_sizes)
        flat = _eval_ref.evaluate(res, synset, DEG, SHIFT, IOU, 0.1, True)
        if margins_ok(margins(flat, res, synset)) and scores_distinct_across_images(res):
            return res, flat
    raise AssertionError("no run under the margin conditions in 200 draws")


def load_golden():
    """(results, golden of use_matches_for_pose=True, golden of False, manifest) from tests/golden/eval_*: the run as the
    reference's list of dicts (empty images with the (0,4,4) placeholders) and what the reference computed for it"""
    import json
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    only = dict(np.load(os.path.join(gold, "eval_pose_only.npz")))
    det = dict(np.load(os.path.join(gold, "eval_pose_detection.npz")))
    with open(os.path.join(gold, "eval_manifest.json")) as f:
        manifest = json.load(f)
    results = []
    for im in range(len(only["in_pred_off"]) - 1):
        p = slice(only["in_pred_off"][im], only["in_pred_off"][im + 1])
        g = slice(only["in_gt_off"][im], only["in_gt_off"][im + 1])
        if p.start == p.stop and g.start == g.stop:
            results.append(empty_image())
            continue
        r = {k[3:]: only[k][p if k.startswith("in_pred") else g] for k in only if k.startswith("in_") and not k.endswith("_off")}
        r["pred_bboxes"] = np.ones((p.stop - p.start, 4))
        results.append(r)
    return results, only, det, manifest
