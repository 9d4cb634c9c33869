"""numpy RESTATEMENT of the scenes drawn under a step's key, written from the text of include/hsp.h (section "scenes drawn under
a step's key"), not from the kernels: the two streams, and the float64 arithmetic of hsp_scene_draw and hsp_mesh_sample step by
step -- every numpy operation below is one IEEE operation per element, in the header's order.  What the kernels are held to
(tests/test_gpu_scene.py) and what the geometry and distribution checks run on (tests/test_scene_host.py)."""
import numpy as np

from _sample_ids_ref import absorb, instance_key
from _step_draws_ref import uniform_f64

SCENE_J, MODEL_J = 0x84000000, 0x85000000
SCENE_TAG, MODEL_TAG = 0xfffffff9, 0xfffffff8
DEG = np.float64(np.pi) / np.float64(180.0)
f64, f32 = np.float64, np.float32


def stream(seed, call, j, tag, idx):
    """word(q) for every q of idx under the instance indices j -> (len(j), len(idx)) uint32"""
    kj = absorb(instance_key(seed, call, np.asarray(j, dtype=np.uint32)), tag)
    return absorb(kj[:, None], np.asarray(idx, dtype=np.uint32)[None, :])


def lerp(lo, hi, u):
    return f64(lo) + (f64(hi) - f64(lo)) * u


def matmul3(A, B):
    """(M,3,3) x (M,3,3): every entry (a0 b0 + a1 b1) + a2 b2"""
    C = np.empty_like(A)
    for r in range(3):
        for c in range(3):
            C[:, r, c] = (A[:, r, 0] * B[:, 0, c] + A[:, r, 1] * B[:, 1, c]) + A[:, r, 2] * B[:, 2, c]
    return C


def rot(axis, deg):
    a = np.asarray(deg, dtype=f64) * DEG
    c, s, R = np.cos(a), np.sin(a), np.zeros((len(a), 3, 3))
    if axis == "x":
        R[:, 0, 0], R[:, 1, 1], R[:, 1, 2], R[:, 2, 1], R[:, 2, 2] = 1.0, c, -s, s, c
    elif axis == "y":
        R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = c, s, 1.0, -s, c
    else:
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = c, -s, s, c, 1.0
    return R


def scene_draw(seed, call, M, ext, cls, mean_shape, sym, params, distractors=(), R=None):
    """ext (n_mesh,3) float64, cls (n_mesh,), mean_shape (n_mesh,3), sym (n_mesh,4) float32; params: the 13 numbers of the
    header's row; distractors (D,8) rows.  R (M,3,3) float32, optional: the rounded rotation to derive from instead of the
    statement's own (a device's, say) -- gt_R, RT and the distractors' translations then follow from IT.
    -> a dict of the header's outputs under ops.scene_draw's names, plus centre (M,2) float64 = (px, py)."""
    ext = np.asarray(ext, dtype=f64).reshape(-1, 3)
    mean_shape, sym = np.asarray(mean_shape, dtype=f32).reshape(-1, 3), np.asarray(sym, dtype=f32).reshape(-1, 4)
    cls = np.asarray(cls, dtype=f32).reshape(-1)
    slo, shi, dlo, dhi, elo, ehi, r, W, H, fx, fy, cx0, cy0 = (f64(v) for v in params)
    dist = np.asarray(distractors, dtype=f64).reshape(-1, 8)
    D, n_mesh = len(dist), len(ext)
    w = stream(seed, call, SCENE_J | np.arange(M, dtype=np.uint32), SCENE_TAG, np.arange(17))
    u = uniform_f64(w)
    k = ((w[:, 0].astype(np.uint64) * np.uint64(n_mesh)) >> np.uint64(32)).astype(np.int32)
    e = ext[k]
    s = (lerp(slo, shi, u[:, 1]) / np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2])).astype(f32)
    dims = e * s.astype(f64)[:, None]
    z = lerp(dlo, dhi, u[:, 2])
    px, py = (W - f64(1)) * u[:, 3], (H - f64(1)) * u[:, 4]
    t = np.stack([(z * (px - cx0)) / fx, (z * (py - cy0)) / fy, z], axis=1).astype(f32)
    yaw, elev, roll = f64(360) * u[:, 5], lerp(elo, ehi, u[:, 6]), (-r) + (f64(2) * r) * u[:, 7]
    if R is None:
        R = matmul3(matmul3(rot("z", roll), rot("x", f64(180) + elev)), rot("y", yaw)).astype(f32)
    R = np.asarray(R, dtype=f32).reshape(M, 3, 3)
    ax, ay, az = (f64(-15) + f64(30) * u[:, 11 + i] for i in range(3))
    aug_r = matmul3(matmul3(rot("z", az), rot("y", ay)), rot("x", ax)).astype(f32)
    n = M * (1 + D)
    out = dict(mesh_id=np.empty(n, np.int32), frame_id=np.tile(np.arange(M, dtype=np.int32), 1 + D), label=np.empty(n, np.int32),
               RT=np.zeros((n, 4, 4), f32), scale=np.empty((n, 3), f32))
    out["RT"][:, 3, 3] = 1
    out["mesh_id"][:M], out["label"][:M] = k, 1
    out["RT"][:M, :3, :3], out["RT"][:M, :3, 3] = R, t
    out["scale"][:M] = s[:, None]
    out.update(obj_id=cls[k], gt_R=R.copy(), gt_t=t.copy(), gt_s=(dims - mean_shape[k].astype(f64)).astype(f32),
               mean_shape=mean_shape[k], sym=sym[k],
               nocs_scale=np.sqrt((dims[:, 0] * dims[:, 0] + dims[:, 1] * dims[:, 1]) + dims[:, 2] * dims[:, 2]).astype(f32),
               aug_bb=(f64(0.8) + f64(0.4) * u[:, 8:11]).astype(f32),
               aug_rt_t=((f64(-50) + f64(100) * u[:, 14:17]) / f64(1000)).astype(f32), aug_rt_r=aug_r,
               angles=np.stack([yaw, elev, roll, ax, ay, az], axis=1), centre=np.stack([px, py], axis=1), dims=dims)
    R64, t64 = R.astype(f64), t.astype(f64)
    for d, row in enumerate(dist):
        rows = slice((1 + d) * M, (2 + d) * M)
        known = bool(row[0] >= 0 and row[0] < n_mesh)
        m = int(row[0]) if known else 0
        off = np.tile(row[4:7], (M, 1))
        if row[7] != 0:
            off[:, 1] = off[:, 1] - (f64(0.5) * dims[:, 1] + f64(0.5) * row[2])
        td = ((R64[:, :, 0] * off[:, None, 0] + R64[:, :, 1] * off[:, None, 1]) + R64[:, :, 2] * off[:, None, 2]) + t64
        out["mesh_id"][rows], out["label"][rows] = (m if known else -1), 2 + d
        out["RT"][rows, :3, :3], out["RT"][rows, :3, 3] = R, td.astype(f32)
        out["scale"][rows] = (row[1:4] / ext[m]).astype(f32) if known else 0
    return out


def cum_area(verts, faces):
    """the running sum of a mesh's triangle areas in float64, as render.MeshSet.cum_area makes it"""
    a, b, c = (np.asarray(verts, dtype=f32)[np.asarray(faces)[:, i]].astype(f64) for i in range(3))
    return np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))


def mesh_sample(seed, call, meshes, mesh_id, scale, n_model, with_tri=False):
    """meshes: a list of (verts (v,3) float32, faces (t,3)); mesh_id (M,), scale (M,3) float32 -> model_point (M,n_model,3)
    float32 (with_tri: also the triangle of every point, (M,n_model))"""
    M = len(mesh_id)
    scale = np.asarray(scale, dtype=f32).reshape(M, 3)
    out, tris = np.empty((M, n_model, 3), f32), np.empty((M, n_model), np.int64)
    for i in range(M):
        v, fc = meshes[int(mesh_id[i])]
        v = np.asarray(v, dtype=f32).astype(f64)
        cum = cum_area(v, fc)
        ext = v.max(0) - v.min(0)
        u = uniform_f64(stream(seed, call, [MODEL_J | i], MODEL_TAG, np.arange(3 * n_model))[0]).reshape(n_model, 3)
        x = u[:, 0] * cum[-1]
        tri = np.minimum(np.searchsorted(cum, x, side="right"), len(fc) - 1)
        u1, u2 = u[:, 1].copy(), u[:, 2].copy()
        flip = u1 + u2 > 1
        u1[flip], u2[flip] = f64(1) - u1[flip], f64(1) - u2[flip]
        a, b, c = (v[np.asarray(fc)[tri, q]] for q in range(3))
        p = (a + u1[:, None] * (b - a)) + u2[:, None] * (c - a)
        sc = scale[i].astype(f64)
        dims = ext * sc
        diag = np.sqrt((dims[0] * dims[0] + dims[1] * dims[1]) + dims[2] * dims[2])
        out[i] = ((p * sc) / diag).astype(f32)
        tris[i] = tri
    return (out, tris) if with_tri else out


# ---- cases the host and the GPU tests share ------------------------------------------------------------------------------------
PARAMS = dict(size_lo=0.08, size_hi=0.3, distance_lo=0.6, distance_hi=1.4, elev_lo=10.0, elev_hi=60.0, roll=10.0, W=640.0, H=480.0,
              fx=577.5, fy=577.5, cx0=319.5, cy0=239.5)


def zero_area_mesh():
    """the unit box with a vertex in the middle of an edge and two triangles without area on it, one first, one amid the rest"""
    from hs_pose_amd import render
    v, f = render.shapes.box()
    v = np.concatenate([v, 0.5 * (v[0:1] + v[1:2])])
    flat = np.array([[0, 8, 1]], np.int32)
    return v.astype(f32), np.concatenate([flat, f[:5], flat, f[5:]]).astype(np.int32)
