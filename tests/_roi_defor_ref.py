"""numpy RESTATEMENT of the training loader's front end, written from the text of include/hsp.h (section "the training loader's
front end": THE MASK RULE, hsp_crop_compact), not from the kernels; on top of tests/_sample_ids_ref.py (absorb, the instance
key, the permutation P) and the crop map of tests/test_frame_host.py.  What the kernels are held to bit for bit
(tests/test_gpu_train_frontend.py), what the morphology and distribution checks run on (tests/test_train_frontend_host.py) and
what tools/time_train_frontend.py times as the host column."""
import numpy as np

import _sample_ids_ref as sref
import test_frame_host as fh

GATE_DOMAIN, SUBSET_DOMAIN = 0xfffffffe, 0xfffffffd


def crop_m(belongs, xf, O):
    """m (O,O) uint8: 1 where the frame pixel the map gives carries the instance (``belongs`` (H,W) bool), 0 where that pixel
    lies outside the frame"""
    H, W = belongs.shape
    p = fh.ref_source(xf, O, H, W)
    return np.where(p >= 0, belongs.reshape(-1)[np.maximum(p, 0)], False).astype(np.uint8)


def erode_dilate(m, r):
    """(E, D) over the triangle T_r = {(i, j): i, j >= 0, i + j <= r} up and to the left; positions outside the crop left out"""
    O0, O1 = m.shape
    E, D = m.copy(), m.copy()
    for j in range(r + 1):                       # rows up
        for i in range(r + 1 - j):               # columns to the left
            if j >= O0 or i >= O1:
                continue
            E[j:, i:] &= m[:O0 - j, :O1 - i]
            D[j:, i:] |= m[:O0 - j, :O1 - i]
    return E, D


def one_step_loops(m, op):
    """ONE iteration of the 2 x 2 element [[0,1],[1,1]] with anchor (1,1), as plain loops: the pixel, the one above it and the
    one to its left, those inside the image only; op = min (erode) or max (dilate)"""
    out = m.copy()
    for v in range(m.shape[0]):
        for u in range(m.shape[1]):
            vals = [m[v, u]]
            if v >= 1:
                vals.append(m[v - 1, u])
            if u >= 1:
                vals.append(m[v, u - 1])
            out[v, u] = op(vals)
    return out


def gate_draw(seed, call, j):
    return int(sref.absorb(sref.absorb(sref.instance_key(seed, call, j), GATE_DOMAIN), 0)[0])


def subset_zero(l, seed, call, j):
    """(l,) bool: the band ranks that become 0"""
    kd = sref.absorb(sref.instance_key(seed, call, j), SUBSET_DOMAIN)
    return sref.permute(np.arange(l), l, kd) < l // 2


def defor(m, r, gate, seed, call, j):
    """-> (crop_mask bytes (O,O) uint8: bit 0 after the rule, bit 1 = m; [l, deformed])"""
    E, D = erode_dilate(m, r)
    band = E != D
    l = int(band.sum())
    deformed = l >= 1 and gate_draw(seed, call, j) < gate
    out = m.copy()
    if deformed:
        out[band] = np.where(subset_zero(l, seed, call, j), 0, 1)       # boolean indexing: row-major rank order
    return (out | (m << 1)).astype(np.uint8), [l, int(deformed)]


def crop_compact(depth, cbytes, xf, O):
    """-> (src int64 (count,), [bit-0-and-depth valid, depth valid], pre): hsp_crop_compact of one instance on its own frame"""
    H, W = depth.shape
    p = fh.ref_source(xf, O, H, W).reshape(-1)
    dvalid = (p >= 0) & (depth.reshape(-1)[np.maximum(p, 0)] > 0)
    c = cbytes.reshape(-1)
    valid = dvalid & ((c & 1) != 0)
    return p[valid], [int(valid.sum()), int(dvalid.sum())], int((dvalid & ((c & 2) != 0)).sum())


def cpu_train_batch_to_pcl(depth, belongs, centers, scales, K, n_pts, O, r, gate, seed, call, min_pts=50):
    """the whole chain on the CPU for frames depth (B,H,W) and instance masks belongs (B,H,W) bool: crops, the mask rule, the
    three rejection tests, the loader's float64 back-projection / 1000, the rows of _sample_ids_ref -> (PC (B,n_pts,3) float32
    with NaN rows where rejected, status (B,))"""
    K = np.asarray(K, dtype=np.float64).reshape(-1)
    B = len(scales)
    PC = np.full((B, n_pts, 3), np.nan, np.float32)
    counts, pres = [], []
    kept = []
    for j in range(B):
        xf = fh.ref_xf(centers[j], scales[j], O)
        cb, _ = defor(crop_m(belongs[j], xf, O), r, gate, seed, call, j)
        src, cnt, pre = crop_compact(depth[j], cb, xf, O)
        counts.append(cnt)
        pres.append(pre)
        kept.append(src)
    choose, status = sref.sample_ids(np.array(counts), n_pts, seed, call, min_pts, 2, 0)
    status = status | (np.array(pres) <= 1).astype(np.int32) * 4
    W = depth.shape[2]
    for j in range(B):
        if status[j]:
            continue
        p = kept[j][choose[j]]
        d = depth[j].reshape(-1)[p].astype(np.float64)
        x = ((p % W).astype(np.float32) - K[2]) * d / K[0]
        y = ((p // W).astype(np.float32) - K[5]) * d / K[4]
        PC[j] = np.stack((x, y, d), axis=-1).astype(np.float32) / np.float32(1000.0)
    return PC, status
