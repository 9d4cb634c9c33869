"""numpy RESTATEMENT of hsp_fps_ids_*, written from the text of include/hsp.h (section "the rows each instance keeps, picked by
farthest-point sampling"), not from the kernel: the status and tiling rules, the thinning g(t) in Python integers, the loader's
float64-then-float32 back-projection (evaluation/load_data_eval.py ``_depth_to_pcl(...) / 1000``) and fp32 farthest-point picks
with the never-repick rule.  What the kernel is held to bit for bit (tests/test_gpu_fps_ids.py) and what
tests/test_fps_ids_host.py runs the hand-made cases on."""
import numpy as np

CAP = 12288
_F32 = np.float32


def g_of(t, c, cap=CAP):
    """the src entry candidate t of an instance with c candidates names (Python integers, no overflow)"""
    t, c = int(t), int(c)
    return t if c <= cap else (t * c) // cap


def candidate_entries(c, cap=CAP):
    """g(t) for t in [0, min(c, cap)) -> int64"""
    return np.array([g_of(t, c, cap) for t in range(min(int(c), cap))], dtype=np.int64)


def back_project(depth, K, pix):
    """frame pixel ids -> (len, 3) float32 metres: u = float32(p % W), v = float32(p // W), ((u - cx) * d / fx, (v - cy) * d / fy,
    d) in float64 with a float64 K, rounded to float32, then / 1000 in float32"""
    H, W = depth.shape
    pix = np.asarray(pix, dtype=np.int64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    u = (pix % W).astype(_F32).astype(np.float64)
    v = (pix // W).astype(_F32).astype(np.float64)
    d = depth.reshape(-1)[pix].astype(np.float64)
    xyz = np.stack([(u - K[0, 2]) * d / K[0, 0], (v - K[1, 2]) * d / K[1, 1], d], axis=1).astype(_F32)
    return xyz / _F32(1000.0)


def fps_never_repick(xyz, S):
    """hsp_fps_levels_f32's rule: start at 0, running minimum of the fp32 distance (dx*dx + dy*dy) + dz*dz under a correctly
    rounded sqrt, the largest wins, the lowest index among equals, a picked point ranks below every unpicked one -> (S,) int64"""
    x = np.ascontiguousarray(xyz, dtype=_F32)
    m = x.shape[0]
    dist = np.full(m, np.inf, dtype=_F32)
    picked = np.zeros(m, dtype=bool)
    picks = np.empty(S, dtype=np.int64)
    cur = 0
    for s in range(S):
        picks[s] = cur
        d = x - x[cur]
        dd = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        assert dd.dtype == _F32
        dist = np.fmin(dist, dd)
        picked[cur] = True
        cur = int(np.argmax(np.where(picked, _F32(-1.0), dist)))        # (argmax: the first of equal maxima)
    return picks


def fps_ids(depth, K, src, count, S, min_pts, min_depth_pts=2, cap=CAP):
    """depth (H,W), K (3,3) or (n,3,3), src (n,L) frame pixel ids, count (n,2) -> (choose (n,S) int32, status (n,) int32)"""
    src, count = np.asarray(src), np.asarray(count)
    n = src.shape[0]
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3)
    choose = np.full((n, S), -1, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    for j in range(n):
        c = int(count[j, 0])
        status[j] = (1 if c < min_pts else 0) | (2 if int(count[j, 1]) < min_depth_pts else 0)
        if status[j] != 0 or c <= 0:
            continue
        if c <= S:
            choose[j] = np.arange(S) % c
            continue
        g = candidate_entries(c, cap)
        xyz = back_project(depth, K[j if K.shape[0] > 1 else 0], src[j, g])
        choose[j] = g[fps_never_repick(xyz, S)]
    return choose, status
