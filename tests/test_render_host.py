"""CPU: the numpy statement of the renderer's contract (tests/_render_ref.py, written from include/hsp.h) held to geometry that
is independent of it, so that "the kernels equal the statement" (tests/test_gpu_render.py) is not only "equal to itself".

The subject is a box of 12 triangles under 40 seeded poses (t_z in [0.5, 1.2] m, sides 8-30 cm, the rotation made orthonormal in
float64 and rounded to fp32), in both depth types, on the tests' 48 x 64 frame with K = (60, 60, 31.5, 23.5).  The analytic side
is a slab test of every pixel's ray against the box in the object frame, with inv(R) of the ROUNDED matrix (not its transpose).

Bounds, none of them tuned:
  coverage   a pixel whose ray passes through the box by more than 1e-9 m is covered, one whose ray misses it by more than 1e-9 m
             is not
  depth      uint16: within 0.5 mm of the analytic nearest hit (one rint); fp32: within 2^-23 relative (one rounding to fp32 is
             2^-24, the rest is room for the float64 path)
  surface    every covered pixel's point, back-projected by the project's own rule and moved into the object frame, lies within
             0.5 mm * |((px - K2) / K0, (py - K5) / K4, 1)| of the box's surface
Then a sphere whose triangles are smaller than a pixel (no hole inside the inscribed sphere, nothing outside the radius), exact
ties and compositing, and the triangles the contract drops."""
import math

import numpy as np
import pytest

import _render_ref as rr
from hs_pose_amd.render import MeshSet, shapes

K, H, W = rr.K4, rr.H, rr.W
BOX = shapes.box()
SEEDS = range(40)


def slab(RT, size):
    """(tn, tf, Ri, t, h): entry and exit parameter of every pixel's ray (direction z = 1, so the parameter IS the depth in
    metres) through the box, in the object frame"""
    R, t = RT[:3, :3].astype(np.float64), RT[:3, 3].astype(np.float64)
    Ri = np.linalg.inv(R)
    o, dl, h = -(Ri @ t), rr.rays() @ Ri.T, 0.5 * size.astype(np.float64)
    with np.errstate(all="ignore"):
        t1, t2 = (-h - o) / dl, (h - o) / dl
    return np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1), Ri, t, h


@pytest.fixture(scope="module")
def box_renders():
    out = {}
    for seed in SEEDS:
        RT, size = rr.box_pose(seed)
        for dtype in (np.uint16, np.float32):
            d, l = rr.render([BOX], [0], [0], [1], RT[None], size[None], K, 1, H, W, dtype=dtype)
            out[seed, dtype] = (RT, size, d[0], l[0])
    return out


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_box_coverage_and_depth(box_renders, dtype):
    worst = 0.0
    for seed in SEEDS:
        RT, size, d, l = box_renders[seed, dtype]
        tn, tf, _, _, _ = slab(RT, size)
        hit = l == 1
        assert ((d > 0) == hit).all()
        assert hit[(tf - tn > 1e-9) & (tn > 0)].all(), f"seed {seed}: a hole"
        assert not hit[tn - tf > 1e-9].any(), f"seed {seed}: a spill"
        assert hit.sum() > 20
        err = np.abs(d[hit].astype(np.float64) - tn[hit] * 1000.0)
        if dtype == np.uint16:
            worst = max(worst, err.max())
            assert err.max() <= 0.5, f"seed {seed}: {err.max()} mm from the analytic hit"
        else:
            rel = (err / (tn[hit] * 1000.0)).max()
            worst = max(worst, rel)
            assert rel <= 2.0 ** -23, f"seed {seed}: {rel} relative"
    print(f"{np.dtype(dtype).name}: worst {'mm' if dtype == np.uint16 else 'relative'} error {worst:.3e}")


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_box_points_lie_on_the_surface(box_renders, dtype):
    worst = -np.inf
    norm = np.linalg.norm(rr.rays(), axis=-1)
    for seed in SEEDS:
        RT, size, d, l = box_renders[seed, dtype]
        _, _, Ri, t, h = slab(RT, size)
        hit = l == 1
        q = (rr.backproject(d)[hit] - t) @ Ri.T
        excess = rr.box_distance(q, h) - 0.0005 * norm[hit]
        worst = max(worst, excess.max())
        assert excess.max() <= 0, f"seed {seed}: {excess.max()} m beyond the bound"
    print(f"{np.dtype(dtype).name}: largest distance minus bound {worst:.3e} m")


def test_sphere_has_no_hole():
    nu, nv, r = 48, 32, 0.1
    sph = shapes.uv_sphere(nu, nv)
    rin = r * math.cos(math.pi / nu) * math.cos(math.pi / (2 * nv))
    dn = rr.rays() / np.linalg.norm(rr.rays(), axis=-1, keepdims=True)
    small = 0
    for seed, z in enumerate(np.linspace(0.9, 1.45, 12)):
        t = np.array([0.05, -0.03, z], np.float32)
        stats = {}
        d, l = rr.render([sph], [0], [0], [1], rr.pose(rr.rotation(seed), t)[None], np.full((1, 3), 2 * r, np.float32), K, 1, H, W,
                         stats=stats)
        hit = l[0] == 1
        perp = np.linalg.norm(t.astype(np.float64) - (dn @ t.astype(np.float64))[..., None] * dn, axis=-1)
        assert hit[perp < rin - 1e-9].all(), f"pose {seed}: a hole"
        assert not hit[perp > r + 1e-9].any(), f"pose {seed}: a spill"
        small += stats["fragments"] < 2976               # fewer fragments than triangles: triangles under a pixel
    assert small == 12


def _one(meshes, mesh_id, label, RT, scale, dtype=np.uint16, **kw):
    n = len(mesh_id)
    d, l = rr.render(meshes, mesh_id, [0] * n, label, np.asarray(RT), np.asarray(scale, dtype=np.float32), K, 1, H, W, dtype=dtype, **kw)
    return d[0], l[0]


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_ties_and_compositing(dtype):
    RT, size = rr.box_pose(5)
    d1, l1 = _one([BOX], [0], [7], [RT], [size], dtype)
    # two coincident instances: the lower index owns every shared pixel
    d2, l2 = _one([BOX], [0, 0], [9, 7], [RT, RT], [size, size], dtype)
    assert (d2 == d1).all() and (l2[l1 == 7] == 9).all() and (l2[l1 == 0] == 0).all()
    # over a background at the same depth word the rendered surface wins; behind a nearer background it does not
    bg_l = np.full((1, H, W), 200, np.uint8)
    d3, l3 = _one([BOX], [0], [7], [RT], [size], dtype, depth=d1[None].copy(), labels=bg_l)
    assert (d3 == d1).all() and (l3[l1 == 7] == 7).all() and (l3[l1 == 0] == 0).all()
    near = np.where(d1 > 0, d1 - d1.dtype.type(1), d1.dtype.type(300))
    d4, l4 = _one([BOX], [0], [7], [RT], [size], dtype, depth=near[None].copy(), labels=bg_l)
    assert (d4 == near).all() and (l4 == 200).all()
    # a background pixel that does not count (0; fp32: negative, NaN, inf) is empty: written as zeros where nothing is drawn
    junk = np.zeros((H, W), d1.dtype)
    if dtype == np.float32:
        junk[0, 0], junk[0, 1], junk[0, 2] = -5.0, np.nan, np.inf
    d5, l5 = _one([BOX], [0], [7], [RT], [size], dtype, depth=junk[None].copy(), labels=bg_l)
    assert (d5 == d1).all() and (l5 == l1).all()


def test_dropped_triangles():
    v, f = BOX
    RT, size = rr.box_pose(8)
    want = _one([BOX], [0], [1], [RT], [size])
    # a repeated index and a zero-area triangle (three vertices on one line) draw nothing; the other triangles are drawn
    v2 = np.concatenate([v, [[0.0, 0.0, 0.0], [0.1, 0.1, 0.1], [0.2, 0.2, 0.2]]]).astype(np.float32)
    f2 = np.concatenate([f, [[0, 0, 5], [8, 9, 10]]]).astype(np.int32)
    got = _one([(v2, f2)], [0], [1], [RT], [size])
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and want[1].any()
    # a vertex behind the camera drops every triangle that names it, and only those
    RTn = rr.pose(rr.rotation(8), np.array([0.0, 0.0, 0.12], np.float32))
    big = np.full(3, 0.3, np.float32)
    u, vv, Z = rr.project(v, RTn, big, K)
    assert (Z <= 0).any() and (Z > 0).any()
    d, l = _one([BOX], [0], [1], [RTn], [big])
    keep = np.array([(Z[t] > 0).all() for t in f])
    assert 0 < keep.sum() < 12
    dk, lk = _one([(v, f[keep])], [0], [1], [RTn], [big])
    assert (d == dk).all() and (l == lk).all()
    # a pose that is not finite draws nothing
    for bad in (np.nan, np.inf):
        RTb = RT.copy()
        RTb[1, 3] = bad
        d, l = _one([BOX], [0], [1], [RTb], [size])
        assert not d.any() and not l.any()
    # ids out of range draw nothing
    d, l = rr.render([BOX], [1, 0, 0], [0, 1, 0], [1, 1, 256], np.stack([RT] * 3), np.stack([size] * 3), K, 1, H, W)
    assert not d.any() and not l.any()


def test_label_boxes_statement():
    img = np.zeros((2, H, W), np.uint8)
    img[0, 3:7, 10:12] = 4
    img[1, 47, 63] = 9
    boxes, count = rr.label_boxes(img, [0, 1, 1, 5], [4, 9, 4, 4])
    assert boxes.tolist() == [[10, 3, 12, 7], [63, 47, 64, 48], [0, 0, 0, 0], [0, 0, 0, 0]] and count.tolist() == [8, 1, 0, 0]


def test_meshset_validates_and_samples():
    with pytest.raises(ValueError, match="index"):
        MeshSet([(BOX[0], np.array([[0, 1, 8]]))], device="cpu")
    with pytest.raises(ValueError, match="finite"):
        MeshSet([(np.array([[0, 0, np.inf], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))], device="cpu")
    with pytest.raises(ValueError, match="integers"):
        MeshSet([(BOX[0], BOX[1].astype(np.float32))], device="cpu")
    ms = MeshSet([BOX, shapes.mug(12)], device="cpu")
    assert ms.table.tolist() == [[0, 8, 0, 12], [8, len(ms.meshes[1][0]), 12, len(ms.meshes[1][1])]]
    assert np.allclose(ms.extent(0), 1.0) and ms.extent(1)[0] > 1.0          # the handle widens the mug along +x
    p = ms.sample_points(0, 500, np.random.default_rng(1))
    assert p.shape == (500, 3) and p.dtype == np.float32 and np.abs(rr.box_distance(p.astype(np.float64), np.full(3, 0.5))).max() < 1e-6
    # closed, consistently wound, outward: every directed edge once, its reverse once, positive volume
    for v, f in (BOX, shapes.cylinder(24), shapes.uv_sphere(12, 8), shapes.mug(16)):
        edges = {}
        for tri in f:
            for k in range(3):
                edges[(tri[k], tri[(k + 1) % 3])] = edges.get((tri[k], tri[(k + 1) % 3]), 0) + 1
        assert all(c == 1 and edges.get((b, a)) == 1 for (a, b), c in edges.items())
        a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
        assert np.einsum("ij,ij->i", a, np.cross(b, c)).sum() > 0
        assert np.allclose(v.max(0) + v.min(0), 0, atol=1e-6)
    assert shapes.mug(16)[0][:, 0].max() > 0.6                               # the handle is on +x
