"""The evaluation metrics' contract (include/hsp.h, "evaluation metrics") stated in numpy, for the tests and the timing tool.
Plain loops over small arrays; fp64 except where the contract says fp32.  The result of ``evaluate`` has the layout of
``hs_pose_amd.evaluation.PoseEvaluator.matches()``: groups in (class, image) order, tables concatenated group after group."""
import math

import numpy as np

YSYM = ("bottle", "bowl", "can")
FLIP = ("phone", "eggbox", "glue")


def kind_of(name):
    return 1 if name in YSYM else 2 if name == "mug" else 3 if name in FLIP else 0


def _extremes(RT, scale):
    """The reference's np.amax / np.amin(bbox, axis=0) on its (3, 8) corner array: the extremes of each CORNER over its three
    coordinates (eval_utils_v1.py:47-50), eight intervals in get_3d_bbox's corner order -- not a box per axis.  Part of the contract."""
    h = np.asarray(scale, np.float64) / 2
    corners = np.array([[sx * h[0], sy * h[1], sz * h[2], 1.0] for sy in (1, -1) for sx in (1, -1) for sz in (1, -1)]).T
    out = RT @ corners
    out = out[:3] / out[3]
    return out.min(axis=0), out.max(axis=0)


def _iou_boxes(a, b):
    ext = np.minimum(a[1], b[1]) - np.maximum(a[0], b[0])
    inter = 0.0 if ext.min() < 0 else np.prod(ext)
    return inter / (np.prod(a[1] - a[0]) + np.prod(b[1] - b[0]) - inter)


def pair_values(pRT, ps, gRT, gs, ghv, kind):
    """(iou fp32, degree, shift), each (np, ng), rows and columns in the image's own order"""
    n_p, n_g = len(pRT), len(gRT)
    iou = np.zeros((n_p, n_g), np.float32)
    deg = np.zeros((n_p, n_g))
    shift = np.zeros((n_p, n_g))
    for i in range(n_p):
        for j in range(n_g):
            A, B = np.asarray(pRT[i], np.float64), np.asarray(gRT[j], np.float64)
            sym = kind == 1 or (kind == 2 and ghv[j] == 0)
            bb = _extremes(B, gs[j])
            if sym:
                best = 0.0
                for r in range(20):
                    th = 2 * math.pi * r / 20.0
                    c, s = np.cos(th), np.sin(th)
                    Ry = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
                    v = _iou_boxes(_extremes(A @ Ry, ps[i]), bb)
                    if v > best:
                        best = v
            else:
                best = _iou_boxes(_extremes(A, ps[i]), bb)
            iou[i, j] = best
            R1 = A[:3, :3] / np.cbrt(np.linalg.det(A[:3, :3]))
            R2 = B[:3, :3] / np.cbrt(np.linalg.det(B[:3, :3]))
            with np.errstate(invalid="ignore"):
                if sym:
                    y1, y2 = R1[:, 1], R2[:, 1]
                    th = np.arccos(y1.dot(y2) / (np.linalg.norm(y1) * np.linalg.norm(y2)))
                else:
                    th = np.arccos((np.trace(R1 @ R2.T) - 1) / 2)
                    if kind == 3:
                        t2 = np.arccos((np.trace(R1 @ np.diag([-1.0, 1.0, -1.0]) @ R2.T) - 1) / 2)
                        if t2 < th:
                            th = t2
            deg[i, j] = th * 180 / np.pi
            shift[i, j] = np.linalg.norm(A[:3, 3] - B[:3, 3]) * 100
    return iou, deg, shift


def _ascending(vals):
    """stable ascending order with NaN last"""
    vals = list(vals)
    return sorted(range(len(vals)), key=lambda k: (vals[k] != vals[k], 0.0 if vals[k] != vals[k] else vals[k], k))


def match_group(scores, iou, deg, shift, iou_thr, deg_thr, shift_thr, pose_index):
    """the two greedy stages of one group.  iou_thr: already fp32.  pose_index: the IoU threshold whose matches the pose stage keeps,
    or -1 for everything.  -> dict(order, iou_pred (T,np), iou_gt (T,ng), pose_pred (D1,S1,kp), pose_gt (D1,S1,kg), kp, kg)"""
    n_p, n_g = iou.shape
    order = _ascending(scores)[::-1]
    T = len(iou_thr)
    ipm = -np.ones((T, n_p), np.int8)
    igm = -np.ones((T, n_g), np.int8)
    rows = [_ascending(iou[i])[::-1] for i in range(n_p)]
    for t in range(T):
        thr = iou_thr[t]
        for pos, i in enumerate(order):
            for j in rows[i]:
                if igm[t, j] > -1:
                    continue
                if iou[i, j] < thr:
                    break
                if iou[i, j] > thr:
                    igm[t, j] = pos
                    ipm[t, pos] = j
                    break
    if pose_index < 0:
        kp, kg = list(order), list(range(n_g))
    else:
        kp = [order[pos] for pos in range(n_p) if ipm[pose_index, pos] > -1]
        kg = [j for j in range(n_g) if igm[pose_index, j] > -1]
    D1, S1 = len(deg_thr), len(shift_thr)
    ppm = -np.ones((D1, S1, len(kp)), np.int8)
    pgm = -np.ones((D1, S1, len(kg)), np.int8)
    prow = [_ascending([deg[i, j] + shift[i, j] for j in kg]) for i in kp]
    for d in range(D1):
        for s in range(S1):
            for pos, i in enumerate(kp):
                for jj in prow[pos]:
                    if pgm[d, s, jj] > -1:
                        continue
                    if deg[i, kg[jj]] > deg_thr[d] or shift[i, kg[jj]] > shift_thr[s]:
                        continue
                    pgm[d, s, jj] = pos
                    ppm[d, s, pos] = jj
                    break
    return dict(order=np.array(order, np.int8), iou_pred=ipm, iou_gt=igm, pose_pred=ppm, pose_gt=pgm, kp=kp, kg=kg)


def _sum_block(a):
    """at most 128 terms: below 8 in index order; otherwise eight interleaved partial sums, folded, then the tail in index order"""
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return res
    r = [a[j] for j in range(8)]
    full = n - n % 8
    for i in range(8, full, 8):
        for j in range(8):
            r[j] = r[j] + a[i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(full, n):
        res = res + a[i]
    return res


def _sum_halves(a):
    """above 128 terms: halves, the left one a multiple of 8 long"""
    n = len(a)
    if n <= 128:
        return _sum_block(a)
    n2 = n // 2
    n2 -= n2 % 8
    return _sum_halves(a[:n2]) + _sum_halves(a[n2:])


def contract_sum(terms):
    """The sum of a 1-D fp64 array in the order include/hsp.h promises for hsp_eval_ap (np.sum's, restated in scalar additions so
    that it does not depend on the numpy that runs it): pieces of at most 8192 elements, each summed pairwise, added up in order."""
    a = np.ascontiguousarray(terms, np.float64).reshape(-1)
    acc = np.float64(0.0)
    for k in range(0, len(a), 8192):
        acc = acc + _sum_halves(a[k:k + 8192])
    return acc


def average_precision(hit, n_gt, summer=np.sum):
    """hit (R, n) bool: per row (one threshold each), whether each prediction is matched, predictions in descending score order.
    ``summer``: what adds a row's terms up (np.sum, or contract_sum for the stated order).  -> (R,) average precisions"""
    R, n = hit.shape
    cnt = np.cumsum(hit, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        prec = cnt / (np.arange(n) + 1)
        rec = (cnt.astype(np.float32) / np.float32(n_gt)).astype(np.float64)
    z = np.zeros((R, 1))
    prec = np.concatenate([z, prec, z], axis=1)
    rec = np.concatenate([z, rec, z + 1], axis=1)
    env = np.maximum.accumulate(prec[:, ::-1], axis=1)[:, ::-1]       # the largest precision from here on
    moved = rec[:, :-1] != rec[:, 1:]
    terms = (rec[:, 1:] - rec[:, :-1]) * env[:, 1:]
    return np.array([summer(terms[r][moved[r]]) for r in range(R)])


def evaluate(results, synset_names, degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres=0.1,
             use_matches_for_pose=True):
    """results: the reference's list of dicts.  -> dict with iou_aps, pose_aps and the tables of every group"""
    ncls = len(synset_names)
    deg_thr = [float(x) for x in degree_thresholds] + [360.0]
    shift_thr = [float(x) for x in shift_thresholds] + [100.0]
    iou_list = list(iou_3d_thresholds)
    iou_thr = np.array(iou_list, np.float32)
    pose_index = iou_list.index(iou_pose_thres) if use_matches_for_pose else -1
    T, D1, S1 = len(iou_thr), len(deg_thr), len(shift_thr)
    groups = []
    for c in range(1, ncls):
        kind = kind_of(synset_names[c])
        for im, r in enumerate(results):
            gc = np.asarray(r["gt_class_ids"]).astype(np.int64).reshape(-1)
            pc = np.asarray(r["pred_class_ids"]).astype(np.int64).reshape(-1)
            gsel, psel = np.where(gc == c)[0], np.where(pc == c)[0]
            if len(gsel) == 0 and len(psel) == 0:
                continue
            pRT = np.asarray(r["pred_RTs"], np.float64)[psel] if len(psel) else np.zeros((0, 4, 4))
            ps = np.asarray(r["pred_scales"], np.float64)[psel] if len(psel) else np.zeros((0, 3))
            sc = np.asarray(r["pred_scores"], np.float64)[psel] if len(psel) else np.zeros(0)
            gRT = np.asarray(r["gt_RTs"], np.float64)[gsel] if len(gsel) else np.zeros((0, 4, 4))
            gs = np.asarray(r["gt_scales"], np.float64)[gsel] if len(gsel) else np.zeros((0, 3))
            ghv = np.asarray(r["gt_handle_visibility"])[gsel] if len(gsel) else np.zeros(0)
            iou, deg, shift = pair_values(pRT, ps, gRT, gs, ghv, kind)
            m = match_group(sc, iou, deg, shift, iou_thr, deg_thr, shift_thr, pose_index)
            m.update(cls=c, image=im, np=len(psel), ng=len(gsel), iou=iou, degree=deg, shift=shift, scores=sc)
            groups.append(m)
    iou_aps = np.zeros((ncls + 1, T))
    pose_aps = np.zeros((ncls + 1, D1, S1))
    for c in range(1, ncls):
        mine = [g for g in groups if g["cls"] == c]
        sc = np.concatenate([g["scores"][g["order"]] for g in mine] + [np.zeros(0)])
        idx = sorted(range(len(sc)), key=lambda k: (-sc[k], k))        # descending score, equal scores in concatenation order
        hit = np.concatenate([g["iou_pred"] > -1 for g in mine] + [np.zeros((T, 0), bool)], axis=1)
        iou_aps[c] = average_precision(hit[:, idx], sum(g["ng"] for g in mine))
        psc = np.concatenate([g["scores"][g["kp"]] for g in mine] + [np.zeros(0)])
        idx = sorted(range(len(psc)), key=lambda k: (-psc[k], k))
        hit = np.concatenate([g["pose_pred"].reshape(D1 * S1, -1) > -1 for g in mine] + [np.zeros((D1 * S1, 0), bool)], axis=1)
        pose_aps[c] = average_precision(hit[:, idx], sum(len(g["kg"]) for g in mine)).reshape(D1, S1)
    iou_aps[-1] = np.mean(iou_aps[1:-1], axis=0)
    pose_aps[-1] = np.mean(pose_aps[1:-1], axis=0)
    return flatten(groups, iou_aps, pose_aps, T, D1, S1)


def flatten(groups, iou_aps, pose_aps, T, D1, S1):
    cat = lambda parts, empty: np.concatenate(parts, axis=-1) if parts else empty
    return dict(
        iou_aps=iou_aps, pose_aps=pose_aps,
        group_class=np.array([g["cls"] for g in groups], np.int32), group_image=np.array([g["image"] for g in groups], np.int32),
        group_np=np.array([g["np"] for g in groups], np.int32), group_ng=np.array([g["ng"] for g in groups], np.int32),
        kept_np=np.array([len(g["kp"]) for g in groups], np.int32), kept_ng=np.array([len(g["kg"]) for g in groups], np.int32),
        order=cat([g["order"] for g in groups], np.zeros(0, np.int8)),
        iou_pred=cat([g["iou_pred"] for g in groups], np.zeros((T, 0), np.int8)),
        iou_gt=cat([g["iou_gt"] for g in groups], np.zeros((T, 0), np.int8)),
        pose_pred=cat([g["pose_pred"] for g in groups], np.zeros((D1, S1, 0), np.int8)),
        pose_gt=cat([g["pose_gt"] for g in groups], np.zeros((D1, S1, 0), np.int8)),
        iou=cat([g["iou"].reshape(-1) for g in groups], np.zeros(0, np.float32)),
        degree=cat([g["degree"].reshape(-1) for g in groups], np.zeros(0)),
        shift=cat([g["shift"].reshape(-1) for g in groups], np.zeros(0)))
