"""The contract of "instances followed from frame to frame" (include/hsp.h: hsp_pose_windows, hsp_roi_compact_box_*,
hsp_track_update) in numpy float64, term for term, written from the header and independently of the kernels and of
pc_sample.py.  The crop map and the compaction are the restatement the frame tests already use (tests/test_frame_host.py).

Every float64 operation below is one IEEE rounding in the header's order, as the kernels' ``_rn`` forms are, so the two agree
bit for bit whatever the inputs.  The case generators still redraw until two margins hold -- every projected u, v extreme at
least ``UV_MARGIN`` from an integer, every ``|q_i| - h_i`` at least ``Q_MARGIN`` metres from zero -- so that the box and the
inside decisions are the same under ANY faithful evaluation; tests/test_track_host.py checks on the CPU that the committed seeds
satisfy both, and no case is left out of any comparison."""
import numpy as np

import test_frame_host as fh

UV_MARGIN = 1e-6
Q_MARGIN = 1e-9
F64 = np.float64


def half_extents(size, pad):
    """h_i = (0.5 * pad) * double(size_i)"""
    return (F64(0.5) * F64(pad)) * np.asarray(size, dtype=np.float32).astype(F64)


def _k_row(K, j):
    K = np.asarray(K, dtype=F64).reshape(-1, 9)
    return K[j if K.shape[0] > 1 else 0]


def corner_uv(RT, size, K, pad):
    """(u (8,), v (8,), Z (8,)) float64 of the eight corners of one instance: e_i = +h_i where bit i of k is set"""
    RT = np.asarray(RT, dtype=np.float32).reshape(4, 4).astype(F64)
    R, t, h = RT[:3, :3], RT[:3, 3], half_extents(size, pad)
    u, v, Z = np.zeros(8), np.zeros(8), np.zeros(8)
    with np.errstate(all="ignore"):
        for k in range(8):
            e = [h[i] if (k >> i) & 1 else -h[i] for i in range(3)]
            c = [((R[r, 0] * e[0] + R[r, 1] * e[1]) + R[r, 2] * e[2]) + t[r] for r in range(3)]
            u[k] = (K[0] * c[0]) / c[2] + K[2]
            v[k] = (K[4] * c[1]) / c[2] + K[5]
            Z[k] = c[2]
    return u, v, Z


def window(RT, size, K, H, W, pad):
    """one instance -> (box (x1, y1, x2, y2) ints, wstatus, margin): margin is the least distance of the four extremes from an
    integer (inf for a flagged instance: its decision does not hang on them)"""
    u, v, Z = corner_uv(RT, size, K, pad)
    h = half_extents(size, pad)
    inputs = np.concatenate([np.asarray(RT, dtype=F64).reshape(4, 4)[:3].reshape(-1), np.asarray(size, dtype=F64).reshape(-1),
                             [K[0], K[2], K[4], K[5]]])
    if not (np.isfinite(inputs).all() and np.isfinite(u).all() and np.isfinite(v).all() and (h > 0).all() and (Z > 0).all()):
        return (0, 0, 0, 0), 4, np.inf
    ext = np.array([u.min(), v.min(), u.max(), v.max()])
    x1, y1 = max(0.0, np.floor(ext[0])), max(0.0, np.floor(ext[1]))
    x2, y2 = min(float(W - 1), np.ceil(ext[2])), min(float(H - 1), np.ceil(ext[3]))
    if x2 <= x1 or y2 <= y1:
        return (0, 0, 0, 0), 4, np.inf
    return (int(x1), int(y1), int(x2), int(y2)), 0, float(np.abs(ext - np.rint(ext)).min())


def windows(RT, size, K, H, W, O, pad):
    """-> dict(boxes (n,4) int32, wstatus (n,) int32, centers (n,2), scales (n,), xf (n,3) float64, margin): centre
    ((x1 + x2) / 2, (y1 + y2) / 2), scale max(x2 - x1, y2 - y1), xf the restatement's ``ref_xf`` of them; a flagged instance has
    zeros everywhere"""
    n = len(size)
    out = dict(boxes=np.zeros((n, 4), np.int32), wstatus=np.zeros(n, np.int32), centers=np.zeros((n, 2)), scales=np.zeros(n),
               xf=np.zeros((n, 3)), margin=np.inf)
    for j in range(n):
        box, ws, margin = window(RT[j], size[j], _k_row(K, j), H, W, pad)
        out["boxes"][j], out["wstatus"][j] = box, ws
        out["margin"] = min(out["margin"], margin)
        if ws == 0:
            x1, y1, x2, y2 = box
            out["centers"][j] = (x1 + x2) / 2, (y1 + y2) / 2
            out["scales"][j] = max(x2 - x1, y2 - y1)
            out["xf"][j] = fh.ref_xf(out["centers"][j], out["scales"][j], O)
    return out


def frame_xyz(depth, K):
    """(H,W,3) float32: the loader's back-projection of every frame pixel / 1000 -- float64 ((u - K2) * d) / K0, rounded to
    float32, divided by 1000 in float32 (what hsp_frame_to_pcl_* writes)"""
    H, W = depth.shape
    d = depth.astype(F64)
    u, v = np.arange(W, dtype=np.float32).astype(F64)[None, :], np.arange(H, dtype=np.float32).astype(F64)[:, None]
    x = ((u - K[2]) * d / K[0]).astype(np.float32)
    y = ((v - K[5]) * d / K[4]).astype(np.float32)
    return np.stack([x, y, d.astype(np.float32)], axis=-1) / np.float32(1000.0)


def inside(depth, RT, size, K, pad):
    """one instance -> (mask (H,W) bool over the pixels with depth > 0, margin): q_i = ((R0i px + R1i py) + R2i pz) -
    ((R0i tx + R1i ty) + R2i tz), inside iff |q_i| <= h_i for all i; margin = the least | |q_i| - h_i | over the depth-valid
    pixels"""
    RT = np.asarray(RT, dtype=np.float32).reshape(4, 4).astype(F64)
    R, t, h = RT[:3, :3], RT[:3, 3], half_extents(size, pad)
    p = frame_xyz(depth, K).astype(F64)
    valid = depth > 0
    mask, margin = valid.copy(), np.inf
    with np.errstate(all="ignore"):
        for i in range(3):
            q = ((R[0, i] * p[..., 0] + R[1, i] * p[..., 1]) + R[2, i] * p[..., 2]) - ((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2])
            mask &= np.abs(q) <= h[i]
            if valid.any():
                margin = min(margin, float(np.abs(np.abs(q[valid]) - h[i]).min()))
    return mask, margin


def masks(depth, RT, size, K, pad, wstatus):
    """(masks (n,H,W) uint8, margin): the inside-masks of all instances, zeros for a flagged one"""
    out, margin = np.zeros((len(size),) + depth.shape, np.uint8), np.inf
    for j in range(len(size)):
        if wstatus[j] == 0:
            m, mg = inside(depth, RT[j], size[j], _k_row(K, j), pad)
            out[j], margin = m, min(margin, mg)
    return out, margin


def compact(depth, RT, size, K, O, pad, win):
    """what hsp_roi_compact_box_* lists -> [(src int64 (count,), [inside-and-depth valid, depth valid])] per instance"""
    m, _ = masks(depth, RT, size, K, pad, win["wstatus"])
    return [fh.ref_compact(depth, m[j] != 0, tuple(win["xf"][j].tolist()), O) if win["wstatus"][j] == 0
            else (np.zeros(0, np.int64), [0, 0]) for j in range(len(size))]


def update(rt_new, size_new, status, rt_state, size_state, lost):
    """hsp_track_update -> (rt_state, size_state, lost) after it"""
    good = np.asarray(status) == 0
    return (np.where(good[:, None, None], rt_new, rt_state), np.where(good[:, None], size_new, size_state),
            np.where(good, 0, lost + 1).astype(np.int32))


def chain_inputs(depth, RT, size, K, O, pad):
    """what the mask-fed chain (pc_sample.frame_to_pcl_device) needs to cut the crops the tracked chain cuts -> (masks (n,H,W)
    uint8, centers (n,2), scales (n,), wstatus (n,), margins (uv, q)).  A flagged instance gets an empty mask and a unit window
    at the origin: the mask-fed chain then counts nothing for it, as the tracked one does."""
    H, W = depth.shape
    win = windows(RT, size, K, H, W, O, pad)
    m, qm = masks(depth, RT, size, K, pad, win["wstatus"])
    centers, scales = win["centers"].copy(), win["scales"].copy()
    scales[win["wstatus"] != 0] = 1.0
    return m, centers, scales, win["wstatus"], (win["margin"], qm)


# ---- cases: seeded, redrawn until both margins hold ---------------------------------------------------------------------------

def rotation(rng):
    """a random rotation as float32 (orthonormal to fp32 rounding, det +1)"""
    q, r = np.linalg.qr(rng.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def pose(R, t):
    RT = np.eye(4, dtype=np.float32)
    RT[:3, :3], RT[:3, 3] = R, t
    return RT


def small_K(H, W, rows=1, rng=None):
    """a pinhole camera for a small frame: a 0.2 m object at 1 m spans about a fifth of the frame's width"""
    K = np.array([[W * 1.1, 0.0, W / 2 - 0.37], [0.0, W * 1.13, H / 2 + 0.21], [0.0, 0.0, 1.0]])
    if rows == 1:
        return K
    return np.stack([K + np.array([[rng.rand() * 3, 0, rng.rand()], [0, rng.rand() * 3, rng.rand()], [0, 0, 0]]) for _ in range(rows)])


def depth_frame(rng, H, W, dtype, lo=500, hi=1500, holes=0.25):
    """millimetres between lo and hi with ``holes`` of the pixels 0; the fp32 form also holds fractions and negatives"""
    d = rng.randint(lo, hi, size=(H, W)).astype(np.float32)
    if dtype == "f32":
        d += rng.rand(H, W).astype(np.float32)
        d[rng.rand(H, W) < 0.03] = -3.0
    d[rng.rand(H, W) < holes] = 0
    return d if dtype == "f32" else d.astype(np.uint16)


def _redraw(make, seed):
    """the first of make(RandomState(seed + 1000 * attempt)) whose margins hold -> (case, attempt)"""
    for attempt in range(50):
        case = make(np.random.RandomState(seed + 1000 * attempt))
        if case["uv_margin"] >= UV_MARGIN and case["q_margin"] >= Q_MARGIN:
            return case
    raise AssertionError(f"no draw of seed {seed} holds the margins")


PAD = 1.5


def windows_case():
    """n = 3 accepted windows and one instance per rejection cause on a 48 x 64 frame -> dict(RT, size, K, H, W, O, pad, win,
    causes): instances 0-2 good (one over the frame's edge), 3 a corner behind the camera, 4 off the frame, 5 a negative size,
    6 a NaN in the pose, 7 an infinite size"""
    H, W, O = 48, 64, 32

    def make(rng):
        K = small_K(H, W)
        RT = np.stack([pose(rotation(rng), t) for t in ([0.05, -0.03, 1.0], [-0.2, 0.1, 0.8], [0.38, 0.2, 1.3],
                                                        [0.0, 0.0, 0.1], [3.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0],
                                                        [0.0, 0.0, 1.0])])
        size = (0.1 + 0.15 * rng.rand(8, 3)).astype(np.float32)
        size[5, 1] = -0.1
        RT[6, 1, 2] = np.nan
        size[7, 0] = np.inf
        win = windows(RT, size, K, H, W, O, PAD)
        return dict(RT=RT, size=size, K=K, H=H, W=W, O=O, pad=PAD, win=win, uv_margin=win["margin"], q_margin=np.inf)
    return _redraw(make, 11)


def compaction_case(O, dtype, k_rows):
    """48 x 64 frame, n = 3: instance 0 a small far box (its window is smaller than every O: source pixels repeat), instance 1 a
    box that fills the frame (the largest window the frame allows, 63: larger than O = 48), instance 2 an ordinary one; 25 %
    holes -> dict(depth, RT, size, K, O, pad, win, want)"""
    H, W = 48, 64

    def make(rng):
        K = small_K(H, W, k_rows, rng)
        depth = depth_frame(rng, H, W, dtype, 600, 1400)
        RT = np.stack([pose(rotation(rng), [0.1, -0.05, 1.2]), pose(np.eye(3, dtype=np.float32), [0.0, 0.0, 1.0]),
                       pose(rotation(rng), [-0.15, 0.08, 0.9])])
        size = np.array([[0.08, 0.1, 0.3], [0.9, 0.7, 0.4], [0.2, 0.25, 0.3]], dtype=np.float32)
        win = windows(RT, size, K, H, W, O, PAD)
        _, qm = masks(depth, RT, size, K, PAD, win["wstatus"])
        return dict(depth=depth, RT=RT, size=size, K=K, O=O, pad=PAD, win=win, uv_margin=win["margin"], q_margin=qm)
    case = _redraw(make, 100 + O + (7 if dtype == "u16" else 0) + 3 * k_rows)
    case["want"] = compact(case["depth"], case["RT"], case["size"], case["K"], O, PAD, case["win"])
    return case


COMPACTION_CASES = [(O, dtype, k_rows) for O in (48, 64, 80) for dtype in ("f32", "u16") for k_rows in (1, 3)]


def clouds_case():
    """96 x 128 frame, n_pts = 256, O = 64, min_pts = 50, three instances: short (at least 50 and fewer than 256 inside: tiled),
    long, rejected (fewer than 50 inside) -> dict(depth, RT, size, K, O, n_pts, min_pts, pad, masks, centers, scales, counts)"""
    H, W, O, n_pts = 96, 128, 64, 256

    def make(rng):
        K = small_K(H, W)
        depth = depth_frame(rng, H, W, "u16", 300, 3000, holes=0.2)      # a wide range: few pixels fall inside a box's depth
        RT = np.stack([pose(rotation(rng), [0.1, -0.1, 1.0]), pose(rotation(rng), [-0.1, 0.05, 1.0]),
                       pose(rotation(rng), [0.2, 0.15, 1.0])])
        size = np.array([[0.1, 0.1, 0.1], [0.4, 0.4, 0.4], [0.02, 0.02, 0.02]], dtype=np.float32)
        m, centers, scales, ws, (uvm, qm) = chain_inputs(depth, RT, size, K, O, PAD)
        counts = [fh.ref_compact(depth, m[j] != 0, fh.ref_xf(centers[j], scales[j], O), O)[1][0] for j in range(3)]
        good = ws.tolist() == [0, 0, 0] and 50 <= counts[0] < n_pts < counts[1] and counts[2] < 50
        return dict(depth=depth, RT=RT, size=size, K=K, O=O, n_pts=n_pts, min_pts=50, pad=PAD, masks=m, centers=centers,
                    scales=scales, counts=counts, uv_margin=uvm if good else 0.0, q_margin=qm)
    return _redraw(make, 21)


def all_cases():
    """every committed case by name, for the margin check on the CPU"""
    yield "windows", windows_case()
    for args in COMPACTION_CASES:
        yield f"compaction{args}", compaction_case(*args)
    yield "clouds", clouds_case()
