"""The contract of "depth frames rendered from meshes and poses" (include/hsp.h: hsp_render_depth_*, hsp_label_boxes) in numpy
float64, term for term, written from the header and independently of the kernels and of hs_pose_amd/render.py.  It loops over
instances and triangles and is vectorised over the candidate pixels of a triangle.

Every float64 operation below is one IEEE rounding in the header's order, as the kernels' ``_rn`` forms are (numpy does not
contract a product into a sum), so the two agree bit for bit whatever the inputs: no margin is needed and none is used."""
import numpy as np

F64 = np.float64
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
KEEP = np.uint64(0xFFFFFFFF)
K4 = np.array([60.0, 0, 31.5, 0, 60.0, 23.5, 0, 0, 1.0])            # the tests' camera: K = (60, 60, 31.5, 23.5)
H, W = 48, 64                                                        # and frame


def project(verts, RT, scale, K):
    """(u, v, Z) float64 (V,) of every vertex of a mesh under one pose: m_i = double(scale_i) * double(v_i);
    X = ((R00 m0 + R01 m1) + R02 m2) + t_x, ...; u = (K0 X) / Z + K2, v = (K4 Y) / Z + K5"""
    RT = np.asarray(RT, dtype=np.float32).reshape(4, 4).astype(F64)
    m = np.asarray(scale, dtype=np.float32).astype(F64)[None, :] * np.asarray(verts, dtype=np.float32).astype(F64)
    with np.errstate(all="ignore"):
        X, Y, Z = (((RT[r, 0] * m[:, 0] + RT[r, 1] * m[:, 1]) + RT[r, 2] * m[:, 2]) + RT[r, 3] for r in range(3))
        u = (K[0] * X) / Z + K[2]
        v = (K[4] * Y) / Z + K[5]
    return u, v, Z


def triangle_keys(u, v, Z, tri, j, Hh, Ww, f32):
    """one triangle -> (ys, xs, keys uint64, candidates) of its kept fragments and the size of its candidate box, or None
    where the contract drops it or the frame holds no candidate"""
    tri = [int(i) for i in tri]
    if len(set(tri)) < 3:
        return None
    uu, vv, zz = u[tri], v[tri], Z[tri]
    if not (np.isfinite(uu).all() and np.isfinite(vv).all() and np.isfinite(zz).all() and (zz > 0).all()):
        return None
    x0, x1 = max(0.0, np.floor(uu.min())), min(float(Ww - 1), np.ceil(uu.max()))
    y0, y1 = max(0.0, np.floor(vv.min())), min(float(Hh - 1), np.ceil(vv.max()))
    edges = []
    for k in range(3):
        a, b = sorted((tri[(k + 1) % 3], tri[(k + 2) % 3]))
        c = tri[k]
        dx, dy, ua, va = u[b] - u[a], v[b] - v[a], u[a], v[a]
        with np.errstate(all="ignore"):
            A = dx * (v[c] - va) - dy * (u[c] - ua)
        if A == 0 or not np.isfinite(A):
            return None
        edges.append((dx, dy, ua, va, A))
    if not (x0 <= x1 and y0 <= y1):
        return None
    py, px = np.mgrid[int(y0):int(y1) + 1, int(x0):int(x1) + 1]
    qx, qy = px.astype(F64), py.astype(F64)
    inside, lam = np.ones(px.shape, bool), []
    with np.errstate(all="ignore"):
        for dx, dy, ua, va, A in edges:
            e = dx * (qy - va) - dy * (qx - ua)
            inside &= (e >= 0) if A > 0 else (e <= 0)
            lam.append(e / A)
        inv = (lam[0] / zz[0] + lam[1] / zz[1]) + lam[2] / zz[2]
        zmm = (((lam[0] + lam[1]) + lam[2]) / inv) * 1000.0
        if f32:
            f = zmm.astype(np.float32)
            good = inside & np.isfinite(f) & (f > 0)
            word = np.where(good, f, np.float32(1)).astype(np.float32).view(np.uint32).astype(np.uint64)
        else:
            q = np.rint(zmm)
            good = inside & (q >= 1) & (q <= 65535)
            word = np.where(good, q, 0).astype(np.uint64)
    return py[good], px[good], (word[good] << np.uint64(32)) | np.uint64(j), px.size


def render(meshes, mesh_id, frame_id, label, RT, scale, K, F, Hh, Ww, dtype=np.uint16, depth=None, labels=None, stats=None):
    """-> (depth (F,H,W) dtype, labels (F,H,W) uint8).  meshes: [(verts, tris)]; K (9,) or (F,9); ``depth`` / ``labels``: the
    existing frames to composite over (``over``), None to clear.  An instance with a mesh_id, frame_id or label out of range
    draws nothing.  ``stats`` (a dict): gets the number of fragments and the candidate-box sizes of the triangles drawn."""
    f32 = np.dtype(dtype) == np.float32
    K = np.asarray(K, dtype=F64).reshape(-1, 9)
    key = np.full((F, Hh, Ww), EMPTY, np.uint64)
    if depth is not None:
        d = np.asarray(depth)
        valid = (np.isfinite(d) & (d > 0)) if f32 else (d > 0)
        word = d.astype(np.float32).view(np.uint32) if f32 else d.astype(np.uint32)
        key = np.where(valid, (word.astype(np.uint64) << np.uint64(32)) | KEEP, EMPTY)
    frags, boxes = 0, []
    for j in range(len(mesh_id)):
        m, f, l = int(mesh_id[j]), int(frame_id[j]), int(label[j])
        if not (0 <= m < len(meshes) and 0 <= f < F and 1 <= l <= 255):
            continue
        verts, tris = meshes[m]
        u, v, Z = project(verts, RT[j], scale[j], K[f if K.shape[0] > 1 else 0])
        for tri in np.asarray(tris):
            got = triangle_keys(u, v, Z, tri, j, Hh, Ww, f32)
            if got is None:
                continue
            ys, xs, keys, cand = got
            frags += len(keys)
            boxes.append(cand)
            key[f, ys, xs] = np.minimum(key[f, ys, xs], keys)
    hi, lo = (key >> np.uint64(32)).astype(np.uint32), (key & KEEP).astype(np.uint32)
    empty, kept = key == EMPTY, (key != EMPTY) & (lo == 0xFFFFFFFF)
    out_d = np.where(empty, 0, hi).astype(np.uint32)
    out_d = out_d.view(np.float32) if f32 else out_d.astype(np.uint16)
    lab = np.asarray(label, dtype=np.int64)
    out_l = np.where(empty | kept, 0, lab[np.minimum(lo, max(len(lab) - 1, 0))] if len(lab) else 0).astype(np.uint8)
    if labels is not None:
        out_l = np.where(kept, np.asarray(labels, dtype=np.uint8), out_l)
    if stats is not None:
        stats["fragments"], stats["boxes"] = frags, np.array(boxes, dtype=np.int64)
    return out_d, out_l


def label_boxes(labels_img, frame_id, label):
    """-> (boxes (n,4) int32 = (x1, y1, x2 + 1, y2 + 1), count (n,) int32), zeros where the frame holds no such pixel"""
    F = labels_img.shape[0]
    boxes, count = np.zeros((len(label), 4), np.int32), np.zeros(len(label), np.int32)
    for j, (f, l) in enumerate(zip(frame_id, label)):
        if not (0 <= f < F and 1 <= l <= 255):
            continue
        ys, xs = np.where(labels_img[f] == l)
        if len(ys):
            boxes[j] = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
            count[j] = len(ys)
    return boxes, count


# ---- geometry the host tests hold the statement to (independent of it) and the cases both test files share ---------------------
def rays(K=K4, Hh=H, Ww=W):
    """(H,W,3) float64: ((px - K2) / K0, (py - K5) / K4, 1), the ray a pixel is sampled on"""
    py, px = np.mgrid[0:Hh, 0:Ww].astype(F64)
    return np.stack([(px - K[2]) / K[0], (py - K[5]) / K[4], np.ones_like(px)], -1)


def rotation(seed):
    """a rotation drawn from ``seed``: made orthonormal in float64 (QR), then rounded to float32"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def pose(R, t):
    RT = np.eye(4, dtype=np.float32)
    RT[:3, :3], RT[:3, 3] = R, t
    return RT


def box_pose(seed):
    """(RT (4,4) fp32, size (3,) fp32) of box case ``seed``: t_z in [0.5, 1.2] m, sides 8-30 cm"""
    rng = np.random.default_rng(100 + seed)
    t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.5, 1.2)], np.float32)
    return pose(rotation(seed), t), rng.uniform(0.08, 0.3, 3).astype(np.float32)


def box_distance(q, h):
    """distance of points q (...,3) in the object frame to the SURFACE of the box of half extents h"""
    d = np.abs(q) - h
    return np.abs(np.linalg.norm(np.maximum(d, 0), axis=-1) + np.minimum(d.max(-1), 0))


def backproject(depth, K=K4):
    """(H,W,3) float64 metres of every pixel by the project's own rule (hsp_frame_to_pcl_*): float64 ((u - K2) * d) / K0
    rounded to float32, then / 1000 in float32"""
    Hh, Ww = depth.shape
    d = depth.astype(F64)
    u, v = np.arange(Ww, dtype=F64)[None, :], np.arange(Hh, dtype=F64)[:, None]
    x = ((u - K[2]) * d / K[0]).astype(np.float32)
    y = ((v - K[5]) * d / K[4]).astype(np.float32)
    return (np.stack([x, y, d.astype(np.float32)], -1) / np.float32(1000.0)).astype(F64)
