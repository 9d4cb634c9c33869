"""Scoring a run on the device: the reference's ``compute_degree_cm_mAP`` (evaluation/eval_utils_v1.py:430-621) over the three
entry points of include/hsp.h's "evaluation metrics" section -- pair values (3D IoU, degree, shift), the greedy matching per
threshold, average precision.  The host's part is bookkeeping: which instance belongs to which (class, image) group.  Class ids
are therefore read on the host (a few small integers per image); poses, scales and scores stay on the device.  torch's stable
sort orders the scores; everything else is libhsp's.  There is no CPU path."""
import os

import numpy as np
import torch

from ._lib import HspError, lib
from .ops import _p, _run, _stream, _ws

_YSYM = ("bottle", "bowl", "can")
_FLIP = ("phone", "eggbox", "glue")
_RESULT_KEYS = ("gt_class_ids", "gt_RTs", "gt_scales", "gt_handle_visibility", "pred_class_ids", "pred_scales", "pred_scores", "pred_RTs")


def _kind(name):
    """include/hsp.h: the `kind` column of a group row"""
    return 1 if name in _YSYM else 2 if name == "mug" else 3 if name in _FLIP else 0


def group_cap():
    """the most predictions, and the most ground truths, one (class, image) group may hold: the library's own statement"""
    return lib().hsp_eval_group_cap()


def pack_results(final_results):
    """The reference's list of result dicts as flat arrays plus per-image offsets (host only).  Returns a dict: ``pred_off`` /
    ``gt_off`` (n_images + 1) int64, ``pred_RTs`` (P,4,4) / ``pred_scales`` (P,3) / ``pred_scores`` (P) float64, ``pred_class_ids``
    (P) int32, ``gt_RTs`` (G,4,4) / ``gt_scales`` (G,3) float64, ``gt_class_ids`` / ``gt_handle_visibility`` (G) int32.  An image
    without predictions may carry the (0,4,4) placeholders evaluate.py:86-87 stores for both ``pred_RTs`` and ``pred_scales``."""
    cols = {k: [] for k in _RESULT_KEYS}
    pred_off, gt_off = [0], [0]
    for im, r in enumerate(final_results):
        n_p = len(r["pred_class_ids"])
        n_g = len(r["gt_class_ids"])
        shapes = dict(pred_RTs=(n_p, 4, 4), pred_scales=(n_p, 3), pred_scores=(n_p,), pred_class_ids=(n_p,), gt_RTs=(n_g, 4, 4),
                      gt_scales=(n_g, 3), gt_class_ids=(n_g,), gt_handle_visibility=(n_g,))
        for k, shp in shapes.items():
            a = np.asarray(r[k])
            if shp[0] == 0 and a.shape[:1] == (0,):
                a = np.zeros(shp)                                  # an empty image: whatever placeholder shape it was given
            if a.shape != shp:
                raise HspError(f"pack_results: image {im}: {k} has shape {a.shape}, expected {shp}")
            cols[k].append(a)
        pred_off.append(pred_off[-1] + n_p)
        gt_off.append(gt_off[-1] + n_g)
    f64 = lambda k, tail: np.concatenate(cols[k] + [np.zeros((0,) + tail)]).astype(np.float64)
    i32 = lambda k: np.concatenate(cols[k] + [np.zeros(0)]).astype(np.int32)
    return dict(pred_off=np.array(pred_off, np.int64), gt_off=np.array(gt_off, np.int64), pred_RTs=f64("pred_RTs", (4, 4)),
                pred_scales=f64("pred_scales", (3,)), pred_scores=f64("pred_scores", ()), pred_class_ids=i32("pred_class_ids"),
                gt_RTs=f64("gt_RTs", (4, 4)), gt_scales=f64("gt_scales", (3,)), gt_class_ids=i32("gt_class_ids"),
                gt_handle_visibility=i32("gt_handle_visibility"))


def unpack_results(packed):
    """the list of dicts ``pack_results`` was given (empty images come back with (0,4,4) / (0,3) arrays)"""
    out = []
    for im in range(len(packed["pred_off"]) - 1):
        p = slice(packed["pred_off"][im], packed["pred_off"][im + 1])
        g = slice(packed["gt_off"][im], packed["gt_off"][im + 1])
        out.append({k: packed[k][p if k.startswith("pred") else g] for k in _RESULT_KEYS})
    return out


def _ids(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(np.int64).reshape(-1)


def _nz(t):
    """a buffer the library accepts where a table is empty (it refuses NULL pointers): one zero row"""
    return t if t.numel() else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)


class PoseEvaluator:
    """``compute_degree_cm_mAP`` as an accumulator: ``add`` one image at a time (device tensors stay on the device) or
    ``add_results`` the reference's list of dicts, then ``compute()`` -> (iou_aps (C+1, T_iou), pose_aps (C+1, D+1, S+1)) as
    float64 numpy with C = len(synset_names), the reference's shapes: row 0 is 'BG' and stays 0, the last row is the mean.
    ``matches()`` -> the per-threshold match tables, the prediction order and the pair values of every (class, image) group."""

    def __init__(self, synset_names, degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres=0.1,
                 use_matches_for_pose=True, device=None):
        self.synset_names = list(synset_names)
        if len(self.synset_names) < 2:
            raise HspError("PoseEvaluator: synset_names must name 'BG' and at least one class")
        self.degree_thres_list = list(degree_thresholds) + [360]
        self.shift_thres_list = list(shift_thresholds) + [100]
        self.iou_thres_list = list(iou_3d_thresholds)
        if not self.iou_thres_list:
            raise HspError("PoseEvaluator: no IoU threshold")
        self.use_matches_for_pose = bool(use_matches_for_pose)
        if self.use_matches_for_pose and iou_pose_thres not in self.iou_thres_list:
            raise HspError(f"PoseEvaluator: iou_pose_thres {iou_pose_thres} is not one of the IoU thresholds")
        self.pose_index = self.iou_thres_list.index(iou_pose_thres) if self.use_matches_for_pose else -1
        self.device = torch.device(device) if device is not None else None
        self._images = []          # per image: (pred_cls, gt_cls) on the host
        self._dev = []             # per image: (pred_RT, pred_s, pred_score, gt_RT, gt_s, gt_hv) on the device, or None where empty
        self._out = None

    # ---- feeding ----
    def _to_dev(self, x, tail, dtype, what):
        if isinstance(x, torch.Tensor):
            if not x.is_cuda:
                raise HspError(f"PoseEvaluator.add: {what}: expected a GPU tensor or an array (hs_pose_amd has no CPU path), got a CPU tensor")
            if self.device is None:
                self.device = x.device
            t = x.detach().to(device=self.device, dtype=dtype)
        else:
            if self.device is None:
                self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
            if self.device is None:
                raise HspError("PoseEvaluator: no GPU (hs_pose_amd has no CPU path)")
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)).astype(np.float64 if dtype == torch.float64 else np.int32)).to(self.device)
        n = t.shape[0] if t.dim() else -1
        if n == 0:
            return t.new_zeros((0,) + tail)
        if tuple(t.shape[1:]) != tail:
            raise HspError(f"PoseEvaluator.add: {what} has shape {tuple(t.shape)}, expected (n,{','.join(map(str, tail))})")
        return t.contiguous()

    def add(self, pred_RT, pred_s, pred_scores, pred_class_ids, gt_class_ids, gt_RTs, gt_scales, gt_handle_visibility):
        """one image: pred_RT (n,4,4), pred_s (n,3), pred_scores (n), pred_class_ids (n); gt_class_ids (m), gt_RTs (m,4,4),
        gt_scales (m,3), gt_handle_visibility (m).  Device tensors of any float type or arrays; n or m may be 0."""
        pc, gc = _ids(pred_class_ids), _ids(gt_class_ids)
        d = (self._to_dev(pred_RT, (4, 4), torch.float64, "pred_RT"), self._to_dev(pred_s, (3,), torch.float64, "pred_s"),
             self._to_dev(pred_scores, (), torch.float64, "pred_scores"), self._to_dev(gt_RTs, (4, 4), torch.float64, "gt_RTs"),
             self._to_dev(gt_scales, (3,), torch.float64, "gt_scales"),
             self._to_dev(gt_handle_visibility, (), torch.int32, "gt_handle_visibility"))
        if not (d[0].shape[0] == d[1].shape[0] == d[2].shape[0] == len(pc)) or not (d[3].shape[0] == d[4].shape[0] == d[5].shape[0] == len(gc)):
            raise HspError(f"PoseEvaluator.add: image {len(self._images)}: the arrays disagree about the number of predictions or ground truths")
        self._images.append((pc, gc))
        self._dev.append(d)
        self._out = None

    def add_results(self, final_results):
        """the reference's list of result dicts (``pred_bboxes`` is not read)"""
        pk = pack_results(final_results)
        if self.device is None:
            if not torch.cuda.is_available():
                raise HspError("PoseEvaluator: no GPU (hs_pose_amd has no CPU path)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        up = {k: torch.from_numpy(pk[k]).to(self.device) for k in ("pred_RTs", "pred_scales", "pred_scores", "gt_RTs", "gt_scales",
                                                                  "gt_handle_visibility")}
        for im in range(len(final_results)):
            p = slice(int(pk["pred_off"][im]), int(pk["pred_off"][im + 1]))
            g = slice(int(pk["gt_off"][im]), int(pk["gt_off"][im + 1]))
            self._images.append((pk["pred_class_ids"][p].astype(np.int64), pk["gt_class_ids"][g].astype(np.int64)))
            self._dev.append((up["pred_RTs"][p], up["pred_scales"][p], up["pred_scores"][p], up["gt_RTs"][g], up["gt_scales"][g],
                              up["gt_handle_visibility"][g]))
        self._out = None

    # ---- the layout: instances by (class, image), one table row per group ----
    def _layout(self):
        ncls = len(self.synset_names)
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        pc = cat([p for p, _ in self._images])
        gc = cat([g for _, g in self._images])
        pim = cat([np.full(len(p), im, np.int64) for im, (p, _) in enumerate(self._images)])
        gim = cat([np.full(len(g), im, np.int64) for im, (_, g) in enumerate(self._images)])
        n_im = max(len(self._images), 1)

        def side(cls, img):
            keep = np.where((cls >= 1) & (cls < ncls))[0]              # the reference's loop sees classes 1 .. len - 1 only
            key = cls[keep] * n_im + img[keep]
            o = np.argsort(key, kind="stable")
            return keep[o], key[o]

        pperm, pkey = side(pc, pim)
        gperm, gkey = side(gc, gim)
        gkeys = np.unique(np.concatenate([pkey, gkey]))
        g_np = np.searchsorted(pkey, gkeys, "right") - np.searchsorted(pkey, gkeys, "left")
        g_ng = np.searchsorted(gkey, gkeys, "right") - np.searchsorted(gkey, gkeys, "left")
        cap = group_cap()
        big = np.where((g_np > cap) | (g_ng > cap))[0]
        if len(big):
            k = int(gkeys[big[0]])
            raise HspError(f"PoseEvaluator: image {k % n_im} holds {int(g_np[big[0]])} predictions and {int(g_ng[big[0]])} ground truths of "
                           f"class '{self.synset_names[k // n_im]}'; a group may hold at most {cap} of each")
        table = np.zeros((len(gkeys), 6), np.int32)
        table[:, 0] = np.cumsum(g_np) - g_np
        table[:, 1] = g_np
        table[:, 2] = np.cumsum(g_ng) - g_ng
        table[:, 3] = g_ng
        table[:, 4] = np.cumsum(g_np * g_ng) - g_np * g_ng
        table[:, 5] = [_kind(self.synset_names[int(k) // n_im]) for k in gkeys]
        return dict(table=table, pperm=pperm, gperm=gperm, g_cls=(gkeys // n_im).astype(np.int64), g_img=(gkeys % n_im).astype(np.int64),
                    n_pairs=int((g_np * g_ng).sum()))

    def _evaluate(self):
        if self._out is not None:
            return self._out
        ncls = len(self.synset_names)
        C = ncls - 1
        T, D1, S1 = len(self.iou_thres_list), len(self.degree_thres_list), len(self.shift_thres_list)
        TP = D1 * S1
        lay = self._layout()
        table = lay["table"]
        n_groups, P, G = len(table), len(lay["pperm"]), len(lay["gperm"])
        g_np, g_ng = table[:, 1].astype(np.int64), table[:, 3].astype(np.int64)
        out = dict(layout=lay, iou_aps=np.zeros((ncls + 1, T)), pose_aps=np.zeros((ncls + 1, D1, S1)))
        self._out = out
        if n_groups == 0:
            return out
        dev = self.device
        L = lib()                                                          # a missing library is an error here, not later
        i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        col = lambda k: torch.cat([d[k] for d in self._dev])
        pperm, gperm = i64(lay["pperm"]), i64(lay["gperm"])
        pRT, ps, sc = _nz(col(0)[pperm].contiguous()), _nz(col(1)[pperm].contiguous()), _nz(col(2)[pperm].contiguous())
        gRT, gs, ghv = _nz(col(3)[gperm].contiguous()), _nz(col(4)[gperm].contiguous()), _nz(col(5)[gperm].contiguous())
        groups = i32(table)
        max_group = int(max(g_np.max(), g_ng.max()))
        npairs = max(lay["n_pairs"], 1)
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
        i8 = lambda *s: torch.full(s, -1, dtype=torch.int8, device=dev)
        iou = torch.zeros(npairs, dtype=torch.float32, device=dev)
        deg, shift = f64(npairs), f64(npairs)
        st = _stream()
        _run("hsp_eval_pairs", (_p(pRT), _p(ps), _p(gRT), _p(gs), _p(ghv), _p(groups), n_groups, max_group, _p(iou), _p(deg), _p(shift), st),
             key=f"g{n_groups}", abytes=(P + G) * 160 + npairs * 20)
        iou_thr = torch.from_numpy(np.array(self.iou_thres_list, np.float32)).to(dev)     # fp32: how numpy >= 2 compares them
        deg_thr = torch.tensor([float(x) for x in self.degree_thres_list], dtype=torch.float64, device=dev)
        shift_thr = torch.tensor([float(x) for x in self.shift_thres_list], dtype=torch.float64, device=dev)
        Pn, Gn = max(P, 1), max(G, 1)
        order, ssort, pscore = i8(Pn), f64(Pn), f64(Pn)
        ipm, igm, ppm, pgm = i8(Pn, T), i8(Gn, T), i8(Pn, TP), i8(Gn, TP)
        kept = torch.zeros(n_groups, 2, dtype=torch.int32, device=dev)
        _run("hsp_eval_match", (_p(groups), n_groups, max_group, _p(sc), _p(iou), _p(deg), _p(shift), _p(iou_thr), T, _p(deg_thr), D1,
                                _p(shift_thr), S1, self.pose_index, _p(order), _p(ssort), _p(ipm), _p(igm), _p(ppm), _p(pgm), _p(pscore),
                                _p(kept), st), key=f"g{n_groups}T{T}+{TP}", abytes=npairs * 20 + (P + G) * (T + TP))
        out.update(order=order, iou_pred=ipm, iou_gt=igm, pose_pred=ppm, pose_gt=pgm, kept=kept, iou=iou, degree=deg, shift=shift, P=P, G=G)
        if P == 0:                                                         # no prediction anywhere: every AP is 0
            return out

        # ---- average precision: slots are class-major, so a class's slots are its concatenation across images ----
        g_cls0 = lay["g_cls"] - 1                                          # class index 0 .. C - 1 of each group
        slot_cls = i64(np.repeat(g_cls0, g_np))
        slot_group = i64(np.repeat(np.arange(n_groups), g_np))
        slot_pos = i64(np.concatenate([np.arange(n) for n in g_np]))
        cls_edges = np.searchsorted(g_cls0, np.arange(C + 1), "left")      # groups of class c: [cls_edges[c], cls_edges[c + 1])
        edges = torch.arange(C + 1, device=dev)

        def ap(match, Tn, scores, cls_key, gt_count):
            o1 = torch.sort(scores, descending=True, stable=True).indices
            o2 = torch.sort(cls_key[o1], stable=True)
            seg_off = torch.searchsorted(o2.values, edges).to(torch.int32)
            aps = torch.zeros(C + 2, Tn, dtype=torch.float64, device=dev)
            nb = L.hsp_eval_ap_workspace_bytes(P, Tn, C)
            ws = _ws(nb, dev)
            order32 = o1[o2.indices].to(torch.int32)
            _run("hsp_eval_ap", (_p(match), P, Tn, _p(order32), _p(seg_off), _p(gt_count), C, _p(aps), _p(ws), nb, st),
                 key=f"P{P}T{Tn}C{C}", abytes=P * Tn * 2 + P * 4 + (C + 2) * Tn * 8)
            return aps

        gt_all = i32(np.bincount(g_cls0, weights=g_ng, minlength=C))
        iou_aps = ap(ipm, T, ssort, slot_cls, gt_all)
        valid = slot_pos < kept[:, 0].to(torch.int64)[slot_group]
        csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(kept[:, 1].to(torch.int64), 0)])
        gt_kept = (csum[i64(cls_edges[1:])] - csum[i64(cls_edges[:-1])]).to(torch.int32)
        pose_aps = ap(ppm, TP, pscore, torch.where(valid, slot_cls, torch.full_like(slot_cls, C)), gt_kept)
        out["iou_aps"] = iou_aps.cpu().numpy()
        out["pose_aps"] = pose_aps.cpu().numpy().reshape(C + 2, D1, S1)
        return out

    def compute(self):
        """(iou_aps (C+1, T_iou), pose_aps (C+1, D+1, S+1)), float64 numpy"""
        out = self._evaluate()
        return out["iou_aps"], out["pose_aps"]

    def matches(self):
        """The tables behind the result, for tests and debugging, as numpy.  Groups are in (class, image) order; per-group tables are
        concatenated group after group along the last axis.  ``group_class`` / ``group_image`` / ``group_np`` / ``group_ng`` /
        ``kept_np`` / ``kept_ng`` (n_groups); ``order``: per group, the original (in-class) index of the prediction at each position
        of ``argsort(scores)[::-1]``; ``iou_pred`` (T_iou, sum np) / ``iou_gt`` (T_iou, sum ng): ``compute_3d_matches``' tables;
        ``pose_pred`` (D+1, S+1, sum kept_np) / ``pose_gt`` (D+1, S+1, sum kept_ng): ``compute_match_from_degree_cm``'s;
        ``iou`` fp32 / ``degree`` / ``shift``: the pair values, per group (np, ng) row-major in the image's own order."""
        out = self._evaluate()
        lay = out["layout"]
        table = lay["table"]
        T, D1, S1 = len(self.iou_thres_list), len(self.degree_thres_list), len(self.shift_thres_list)
        n_groups = len(table)
        res = dict(group_class=lay["g_cls"].astype(np.int32), group_image=lay["g_img"].astype(np.int32),
                   group_np=table[:, 1].copy(), group_ng=table[:, 3].copy())
        if n_groups == 0:
            z = np.zeros(0, np.int32)
            res.update(kept_np=z, kept_ng=z, order=np.zeros(0, np.int8), iou_pred=np.zeros((T, 0), np.int8), iou_gt=np.zeros((T, 0), np.int8),
                       pose_pred=np.zeros((D1, S1, 0), np.int8), pose_gt=np.zeros((D1, S1, 0), np.int8), iou=np.zeros(0, np.float32),
                       degree=np.zeros(0), shift=np.zeros(0))
            return res
        P, G = out["P"], out["G"]
        kept = out["kept"].cpu().numpy()
        kp = np.repeat(kept[:, 0], table[:, 1])
        kg = np.repeat(kept[:, 1], table[:, 3])
        ppos = np.concatenate([np.arange(n) for n in table[:, 1]] + [np.zeros(0, np.int64)])
        gpos = np.concatenate([np.arange(n) for n in table[:, 3]] + [np.zeros(0, np.int64)])
        h = lambda k, n: out[k].cpu().numpy()[:n]
        res.update(kept_np=kept[:, 0].copy(), kept_ng=kept[:, 1].copy(), order=h("order", P), iou_pred=h("iou_pred", P).T.copy(),
                   iou_gt=h("iou_gt", G).T.copy(),
                   pose_pred=h("pose_pred", P)[ppos < kp].T.reshape(D1, S1, -1).copy(),
                   pose_gt=h("pose_gt", G)[gpos < kg].T.reshape(D1, S1, -1).copy(),
                   iou=h("iou", lay["n_pairs"]), degree=h("degree", lay["n_pairs"]), shift=h("shift", lay["n_pairs"]))
        return res


def compute_degree_cm_mAP(final_results, synset_names, log_dir=None, degree_thresholds=[360], shift_thresholds=[100],
                          iou_3d_thresholds=[0.1], iou_pose_thres=0.1, use_matches_for_pose=False, eval_recon=False, plot_figure=True):
    """The reference's function (eval_utils_v1.py:430) on the device: same arguments, same ``(iou_3d_aps, pose_aps)``.  No figure is
    drawn (``plot_figure`` is accepted and ignored); ``mAP_data.npz`` with the reference's keys is written only where ``log_dir`` is
    given.  ``eval_recon`` (the reconstruction distances, not a metric of this package's outputs) is refused."""
    if eval_recon:
        raise HspError("compute_degree_cm_mAP: eval_recon is not built")
    ev = PoseEvaluator(synset_names, degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres, use_matches_for_pose)
    ev.add_results(final_results)
    iou_aps, pose_aps = ev.compute()
    if log_dir is not None:
        np.savez(os.path.join(log_dir, "mAP_data.npz"), pose_aps=pose_aps, degree_thres_list=ev.degree_thres_list,
                 shift_thres_list=ev.shift_thres_list, iou_thres_list=ev.iou_thres_list, iou_3d_aps=iou_aps)
    return iou_aps, pose_aps


HEADLINE = ("3D IoU at 25", "3D IoU at 50", "3D IoU at 75", "5 degree, 2cm", "5 degree, 5cm", "10 degree, 2cm", "10 degree, 5cm",
            "10 degree, 10cm", "5 degree", "10 degree", "2cm", "5cm", "10cm")


def headline(iou_aps, pose_aps, degree_thresholds=tuple(range(0, 61)), shift_thresholds=tuple(i / 2 for i in range(21)),
             iou_3d_thresholds=tuple(i / 100 for i in range(101)), row=-1):
    """the thirteen figures evaluate.py:157-169 logs, in its order, as {name: percent}: row -1 is the mean over classes, row c the
    class synset_names[c].  The threshold lists are those the arrays were computed with (without the appended 360 / 100)."""
    dl, sl, il = list(degree_thresholds), list(shift_thresholds), list(iou_3d_thresholds)
    d5, d10, s2, s5, s10 = dl.index(5), dl.index(10), sl.index(2), sl.index(5), sl.index(10)
    vals = [iou_aps[row, il.index(0.25)], iou_aps[row, il.index(0.5)], iou_aps[row, il.index(0.75)], pose_aps[row, d5, s2],
            pose_aps[row, d5, s5], pose_aps[row, d10, s2], pose_aps[row, d10, s5], pose_aps[row, d10, s10], pose_aps[row, d5, -1],
            pose_aps[row, d10, -1], pose_aps[row, -1, s2], pose_aps[row, -1, s5], pose_aps[row, -1, s10]]
    return {k: float(v) * 100 for k, v in zip(HEADLINE, vals)}
