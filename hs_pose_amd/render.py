"""Depth frames and label images rendered on the device from triangle meshes and poses (include/hsp.h: "depth frames rendered
from meshes and poses"; csrc/render.hip), in the formats the front ends read: uint16 or fp32 millimetres and a uint8 label image.

``shapes``          procedural closed meshes (box, cylinder, uv_sphere, mug): geometry without asset files
``MeshSet``         a list of meshes validated on the host, packed and uploaded once
``render_frames``   instances of a mesh set under poses and scales -> (depth, labels)
``label_boxes``     the tight box and pixel count of each instance's label, on the device
``SyntheticItems``  seeded training items -- pose, size, rendered frame, ground truth -- as the two dicts ``train.FrameTrainStep`` takes
``SceneSource``     the same items drawn on the device under a step's key: no host generator, no upload, no read-back

There is no CPU path: the frames are made by the kernels or not at all.  The numpy statement the kernels are held to lives with
the tests (tests/_render_ref.py)."""
import math
import types

import numpy as np
import torch

from . import ops


# ------------------------------------------------------------------------------------------------
# procedural meshes: closed, wound so that the normals point outward, centred on their bounding box; y is up
# ------------------------------------------------------------------------------------------------

def _outward(verts, faces):
    """faces of a closed, consistently wound surface, flipped as a whole where its signed volume is negative"""
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum()
    return faces if vol > 0 else faces[:, ::-1].copy()


def _mesh(verts, faces, centre=True):
    verts = np.asarray(verts, dtype=np.float64)
    if centre:
        verts = verts - 0.5 * (verts.min(0) + verts.max(0))
    return verts.astype(np.float32), _outward(verts, np.asarray(faces, dtype=np.int32))


def _box():
    """the unit cube [-0.5, 0.5]^3: 8 vertices, 12 triangles"""
    verts = [[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]       # index = 4 ix + 2 iy + iz
    faces = []
    for axis in range(3):
        o1, o2 = [a for a in range(3) if a != axis]
        for side in (0, 1):
            corner = lambda i, j: (side << (2 - axis)) | (i << (2 - o1)) | (j << (2 - o2))
            quad = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
            if (side == 1) != (axis == 1):                  # (e_o1 x e_o2 = +e_axis for axes 0 and 2, -e_axis for axis 1)
                quad.reverse()
            faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return _mesh(verts, faces)


def _ring(r, y, seg):
    return [[r * math.cos(2 * math.pi * i / seg), y, r * math.sin(2 * math.pi * i / seg)] for i in range(seg)]


def _band(lo, hi, seg):
    """the quads between two rings of ``seg`` vertices that start at indices lo and hi"""
    faces = []
    for i in range(seg):
        j = (i + 1) % seg
        faces += [(lo + i, hi + i, hi + j), (lo + i, hi + j, lo + j)]
    return faces


def _cylinder(seg):
    """radius 0.5, height 1 about the y axis: two rings, two cap centres, 4 seg triangles"""
    seg = int(seg)
    if seg < 3:
        raise ValueError(f"shapes.cylinder: seg {seg} < 3")
    verts = _ring(0.5, -0.5, seg) + _ring(0.5, 0.5, seg) + [[0, -0.5, 0], [0, 0.5, 0]]
    faces = _band(0, seg, seg)
    for i in range(seg):
        j = (i + 1) % seg
        faces += [(2 * seg, i, j), (2 * seg + 1, seg + j, seg + i)]
    return _mesh(verts, faces)


def _uv_sphere(nu, nv):
    """radius 0.5: poles on the y axis, nv - 1 rings of nu vertices at the polar angles pi i / nv"""
    nu, nv = int(nu), int(nv)
    if nu < 3 or nv < 2:
        raise ValueError(f"shapes.uv_sphere: nu {nu} < 3 or nv {nv} < 2")
    verts = [[0, 0.5, 0]]
    for i in range(1, nv):
        th = math.pi * i / nv
        verts += _ring(0.5 * math.sin(th), 0.5 * math.cos(th), nu)
    verts.append([0, -0.5, 0])
    last = len(verts) - 1
    faces = []
    for i in range(nu):
        j = (i + 1) % nu
        faces += [(0, 1 + i, 1 + j), (last, last - nu + j, last - nu + i)]
    for r in range(nv - 2):
        faces += _band(1 + r * nu, 1 + (r + 1) * nu, nu)
    return _mesh(verts, faces)


def _mug(seg):
    """a cup of radius 0.5 and height 1 with a cavity (wall and floor 0.06 thick) and a handle on +x: the cup is one closed
    surface (outside, rim, inside, floor), the handle a closed bar bent through five segments whose ends lie inside the wall"""
    seg = int(seg)
    if seg < 3:
        raise ValueError(f"shapes.mug: seg {seg} < 3")
    ro, ri, fl = 0.5, 0.44, -0.44
    verts = _ring(ro, -0.5, seg) + _ring(ro, 0.5, seg) + _ring(ri, 0.5, seg) + _ring(ri, fl, seg) + [[0, -0.5, 0], [0, fl, 0]]
    faces = _band(0, seg, seg) + _band(seg, 2 * seg, seg) + _band(2 * seg, 3 * seg, seg)
    for i in range(seg):
        j = (i + 1) % seg
        faces += [(4 * seg, i, j), (4 * seg + 1, 3 * seg + j, 3 * seg + i)]
    cup_v, cup_f = np.asarray(verts, dtype=np.float64), _outward(np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int32))
    # the handle's centre line in the xy plane, a square section of side 0.08 swept along it
    path = [(0.47, 0.3), (0.72, 0.3), (0.8, 0.15), (0.8, -0.15), (0.72, -0.3), (0.47, -0.3)]
    hv, hf, w = [], [], 0.04
    for k, (x, y) in enumerate(path):
        (xa, ya), (xb, yb) = path[max(k - 1, 0)], path[min(k + 1, len(path) - 1)]
        tx, ty = xb - xa, yb - ya
        n = math.hypot(tx, ty)
        nx, ny = -ty / n, tx / n                            # the in-plane normal of the centre line
        hv += [[x + w * nx, y + w * ny, -w], [x + w * nx, y + w * ny, w], [x - w * nx, y - w * ny, w], [x - w * nx, y - w * ny, -w]]
    for k in range(len(path) - 1):
        hf += _band(4 * k, 4 * k + 4, 4)
    e = 4 * (len(path) - 1)
    hf += [(0, 1, 2), (0, 2, 3), (e, e + 2, e + 1), (e, e + 3, e + 2)]
    hv = np.asarray(hv, dtype=np.float64)
    hf = _outward(hv, np.asarray(hf, dtype=np.int32))
    verts = np.concatenate([cup_v, hv])
    verts = verts - 0.5 * (verts.min(0) + verts.max(0))
    return verts.astype(np.float32), np.concatenate([cup_f, hf + len(cup_v)]).astype(np.int32)


shapes = types.SimpleNamespace(box=_box, cylinder=_cylinder, uv_sphere=_uv_sphere, mug=_mug)


# ------------------------------------------------------------------------------------------------
# mesh sets
# ------------------------------------------------------------------------------------------------

class MeshSet:
    """``meshes``: a list of (verts (v,3) float, faces (t,3) int) numpy arrays, validated here -- finite vertices, every index
    inside its own mesh, sizes within int32 -- packed as include/hsp.h lays them out and uploaded once: ``verts`` (V,3) fp32,
    ``tris`` (T,3) int32 with indices relative to their mesh, ``table`` (n_mesh,4) int32 = (first vertex, vertex count, first
    triangle, triangle count).  The host copies stay for ``extent`` and ``sample_points``."""

    def __init__(self, meshes, device="cuda"):
        if len(meshes) == 0:
            raise ValueError("MeshSet: expects at least one mesh")
        self.meshes, rows, v0, t0 = [], [], 0, 0
        for k, (v, f) in enumerate(meshes):
            v, f = np.asarray(v), np.asarray(f)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or len(v) == 0 or len(f) == 0:
                raise ValueError(f"MeshSet: mesh {k} expects verts (v,3) and faces (t,3), both non-empty, got {v.shape}, {f.shape}")
            if not np.issubdtype(f.dtype, np.integer):
                raise ValueError(f"MeshSet: mesh {k}: faces expects integers, got {f.dtype}")
            v = v.astype(np.float32)
            if not np.isfinite(v).all():
                raise ValueError(f"MeshSet: mesh {k} has a vertex that is not finite (as float32)")
            if f.min() < 0 or f.max() >= len(v):
                raise ValueError(f"MeshSet: mesh {k} has a vertex index outside [0, {len(v)})")
            self.meshes.append((np.ascontiguousarray(v), np.ascontiguousarray(f, dtype=np.int32)))
            rows.append((v0, len(v), t0, len(f)))
            v0, t0 = v0 + len(v), t0 + len(f)
        if v0 >= 2 ** 31 or t0 >= 2 ** 31:
            raise ValueError(f"MeshSet: {v0} vertices / {t0} triangles do not fit int32")
        self.device = torch.device(device)
        self.verts = torch.from_numpy(np.concatenate([v for v, _ in self.meshes])).to(self.device)
        self.tris = torch.from_numpy(np.concatenate([f for _, f in self.meshes])).to(self.device)
        self.table = torch.tensor(rows, dtype=torch.int32).to(self.device)
        self._cum = self._ext = None

    def __len__(self):
        return len(self.meshes)

    @property
    def cum_area(self):
        """(T,) float64 on the device, built on first use: per mesh the running sum of its triangles' areas
        0.5 |(b - a) x (c - a)| in float64, restarting at each mesh (include/hsp.h: hsp_mesh_sample).  A mesh without area is
        refused, as ``sample_points`` refuses it."""
        if self._cum is None:
            cums = []
            for k, (v, f) in enumerate(self.meshes):
                a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
                cum = np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))
                if not cum[-1] > 0:
                    raise ValueError(f"MeshSet.cum_area: mesh {k} has no area")
                cums.append(cum)
            self._cum = torch.from_numpy(np.concatenate(cums)).to(self.device)
        return self._cum

    @property
    def extents(self):
        """(n_mesh,3) float64 on the device, built on first use: ``extent(k)`` of every mesh"""
        if self._ext is None:
            self._ext = torch.from_numpy(np.stack([self.extent(k) for k in range(len(self))])).to(self.device)
        return self._ext

    def extent(self, k):
        """(3,) float64: max - min of mesh k's vertices along each axis, in model units"""
        v = self.meshes[k][0].astype(np.float64)
        return v.max(0) - v.min(0)

    def sample_points(self, k, n, rng):
        """(n,3) float32 in model units: points drawn on mesh k's surface, a triangle chosen in proportion to its area and a
        point uniformly inside it, on the numpy ``Generator`` rng (2 n uniforms for the triangles' interiors after n for the choice)"""
        v, f = self.meshes[k]
        a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
        cum = np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))
        if not cum[-1] > 0:
            raise ValueError(f"MeshSet.sample_points: mesh {k} has no area")
        t = np.minimum(np.searchsorted(cum, rng.random(n) * cum[-1], side="right"), len(f) - 1)
        r1, r2 = np.sqrt(rng.random(n))[:, None], rng.random(n)[:, None]
        return ((1 - r1) * a[t] + r1 * (1 - r2) * b[t] + r1 * r2 * c[t]).astype(np.float32)


def _dev(x, dtype, dev, shape=None):
    """x as a contiguous tensor of dtype on dev: a device tensor is taken as it is (inside a capture nothing else is allowed),
    anything else goes up with an ordinary copy"""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        t = x if x.dtype == dtype else x.to(dtype)
    else:
        t = torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x), dtype=dtype).to(dev)
    return t.reshape(shape) if shape is not None else t


def render_frames(meshes, mesh_ids, RT, scale, K, H, W, frame_ids=None, labels=None, F=None, out=None, over=False,
                  dtype=torch.uint16):
    """n instances of ``meshes`` (a MeshSet) -> (depth (F,H,W) ``dtype`` millimetres, labels (F,H,W) uint8), on the device.

    mesh_ids (n,), RT (n,4,4) fp32 poses in metres, scale (n,3) fp32 metres per model unit, K (3,3) or (F,3,3);
    frame_ids (n,): the frame each instance is drawn into, default one frame per instance; labels (n,) in 1..255, default
    1, 2, ...; F defaults to n with the default frame_ids, else to ``out``'s or max(frame_ids) + 1 (read on the host: pass F when
    frame_ids is a device tensor).  ``out`` = (depth, labels): caller-owned frames; with ``over`` the instances are composited
    over what they hold.  The z-buffer is the device's: the nearest surface wins a pixel, and at equal depth words the lower
    instance.  Given device tensors throughout, the call uploads nothing and can be captured."""
    dev = meshes.device
    mesh_ids = _dev(mesh_ids, torch.int32, dev, (-1,))
    n = mesh_ids.numel()
    if out is not None and F is None:
        F = out[0].shape[0]
    if frame_ids is None:
        F = n if F is None else F
        frame_ids = torch.arange(n, dtype=torch.int32, device=dev)
    elif F is None:
        F = int(np.asarray(frame_ids.cpu() if isinstance(frame_ids, torch.Tensor) else frame_ids).max()) + 1 if n else 1
    if labels is None:
        labels = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    K64 = _dev(K, torch.float64, dev, (-1, 9))
    depth, lab = out if out is not None else (None, None)
    return ops.render_depth(meshes.verts, meshes.tris, meshes.table, mesh_ids, _dev(frame_ids, torch.int32, dev, (-1,)),
                            _dev(labels, torch.int32, dev, (-1,)), _dev(RT, torch.float32, dev, (n, 16)),
                            _dev(scale, torch.float32, dev, (n, 3)), K64, max(int(F), 1), H, W, over=over, depth=depth, labels=lab,
                            dtype=dtype)


def label_boxes(labels_img, frame_ids, label_vals):
    """(boxes (n,4) int32 = (x1, y1, x2, y2) with x2, y2 exclusive, count (n,) int32) on the device: the extent in frame
    frame_ids[j] of labels_img (F,H,W) uint8 of the pixels that carry label_vals[j]; zeros where there is none"""
    dev = labels_img.device
    return ops.label_boxes(labels_img, _dev(frame_ids, torch.int32, dev, (-1,)), _dev(label_vals, torch.int32, dev, (-1,)))


def euler_zyx(x_deg, y_deg, z_deg):
    """Rz Ry Rx of three angles in degrees, float64: the composition the reference's augmentation draws its small rotation by"""
    x, y, z = (math.radians(a) for a in (x_deg, y_deg, z_deg))
    Rx = np.array([[1, 0, 0], [0, math.cos(x), -math.sin(x)], [0, math.sin(x), math.cos(x)]])
    Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    Rz = np.array([[math.cos(z), -math.sin(z), 0], [math.sin(z), math.cos(z), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


class SyntheticItems:
    """Seeded training items rendered from a mesh set, as the two dicts ``train.FrameTrainStep`` takes.

    ``meshes`` a MeshSet; ``class_ids`` (n_mesh,) the category of each mesh (``obj_id``, 0-based), ``mean_shapes`` (n_mesh,3)
    metres and ``sym_infos`` (n_mesh,4) its category's mean size and symmetry row; K (3,3), H, W the camera; ``distance``
    (lo, hi) metres; ``size`` (lo, hi) metres, the range of an item's LARGEST side; ``rng`` a numpy ``Generator`` the caller
    seeds (default: ``default_rng(0)``); ``n_model`` points of ``model_point``.

    ``draw(M)`` draws, per item and in this order on rng: the mesh (``integers``); the largest side, uniform in ``size`` (the
    mesh keeps its proportions); the depth t_z, uniform in ``distance``; the pixel its centre projects to, uniform over
    [0, W - 1] x [0, H - 1] -- so every centre lies inside the frame; the rotation R = Rz(roll) Rx(180 + elev) Ry(yaw) with yaw
    uniform in [0, 360) degrees about the object's up axis y, elev uniform in ``elev`` (default 10 ... 60 degrees: the camera,
    whose y axis points down, looks onto the object from above) and roll uniform in [-``roll``, ``roll``] (default 10 degrees);
    the model points (``MeshSet.sample_points``); then the augmentation parameters with the reference's distributions and order
    (datasets/load_data.py generate_aug_parameters): three uniforms in [0.8, 1.2] for aug_bb, three angles uniform in [-15, 15]
    degrees for aug_rt_r = Rz Ry Rx, three uniforms in [-50, 50] mm for aug_rt_t.  Pose and scale are rounded to fp32 before
    anything is derived from them, so the ground truth is the rendered pose exactly.

    It renders one frame per item under label 1 and returns
      frames: depth (M,H,W) uint16 mm, labels (M,H,W) uint8, inst_ids (M,) -- all 1 --, bboxes_xyxy (M,4) int64 on the host and
              bboxes_d (M,4) int32 on the device, both ``label_boxes``' (x2, y2 exclusive; one small device->host copy), K
      items:  obj_id (M,), gt_R (M,3,3), gt_t (M,3), gt_s (M,3) = size - mean shape (the reference's get_fs_net_scale rule),
              mean_shape (M,3), sym (M,4), model_point (M,n_model,3) in units of the object's diagonal, nocs_scale (M,) = that
              diagonal in metres, aug_bb (M,3), aug_rt_t (M,3), aug_rt_r (M,3,3): fp32 device tensors
    and keeps the render's inputs of the last draw in ``last`` (RT, scale, mesh_ids, sizes: numpy).

    ``distractors``: a list of dicts(mesh=k, size=(sx, sy, sz) metres, offset=(ox, oy, oz) metres in the item's frame,
    rest=bool): further instances drawn into every item's frame under labels 2, 3, ..., which no item names, posed with the
    item's rotation at t + R offset; with ``rest`` the offset's y is lowered by half the item's height plus half the
    distractor's, so a slab comes to lie under the object.  The device's z-buffer does the occlusion."""

    def __init__(self, meshes, class_ids, mean_shapes, sym_infos, K, H, W, distance=(0.6, 1.4), size=(0.08, 0.3), rng=None,
                 n_model=1024, elev=(10.0, 60.0), roll=10.0, distractors=()):
        self.meshes = meshes
        self.class_ids = np.asarray(class_ids, dtype=np.float32).reshape(-1)
        self.mean_shapes = np.asarray(mean_shapes, dtype=np.float32).reshape(-1, 3)
        self.sym_infos = np.asarray(sym_infos, dtype=np.float32).reshape(-1, 4)
        if not len(meshes) == len(self.class_ids) == len(self.mean_shapes) == len(self.sym_infos):
            raise ValueError("SyntheticItems: class_ids, mean_shapes and sym_infos expect one row per mesh")
        self.K = np.asarray(K, dtype=np.float64).reshape(3, 3)
        self.H, self.W = int(H), int(W)
        self.distance, self.size, self.elev, self.roll = tuple(distance), tuple(size), tuple(elev), float(roll)
        if not (0 < self.distance[0] <= self.distance[1] and 0 < self.size[0] <= self.size[1]):
            raise ValueError(f"SyntheticItems: distance {distance} / size {size} expect 0 < lo <= hi")
        self.rng = np.random.default_rng(0) if rng is None else rng
        self.n_model = int(n_model)
        self.distractors = list(distractors)
        if len(self.distractors) > 254:
            raise ValueError("SyntheticItems: at most 254 distractors (labels 2 ... 255)")
        self.last = None

    def draw(self, M):
        rng, K, M = self.rng, self.K, int(M)
        mesh_ids = np.zeros(M, np.int32)
        RT = np.tile(np.eye(4, dtype=np.float32), (M, 1, 1))
        scale, dims = np.zeros((M, 3), np.float32), np.zeros((M, 3), np.float64)
        model = np.zeros((M, self.n_model, 3), np.float32)
        nocs, aug_bb, aug_t = np.zeros(M, np.float32), np.zeros((M, 3), np.float32), np.zeros((M, 3), np.float32)
        aug_r = np.zeros((M, 3, 3), np.float32)
        for i in range(M):
            k = mesh_ids[i] = rng.integers(len(self.meshes))
            ext = self.meshes.extent(k)
            scale[i] = np.float32(rng.uniform(*self.size) / ext.max())
            dims[i] = ext * scale[i].astype(np.float64)
            z = rng.uniform(*self.distance)
            cx, cy = rng.uniform(0, self.W - 1), rng.uniform(0, self.H - 1)
            yaw, elev, roll = rng.uniform(0, 360), rng.uniform(*self.elev), rng.uniform(-self.roll, self.roll)
            RT[i, :3, :3] = euler_zyx(0, 0, roll) @ euler_zyx(180 + elev, 0, 0) @ euler_zyx(0, yaw, 0)
            RT[i, :3, 3] = z * (cx - K[0, 2]) / K[0, 0], z * (cy - K[1, 2]) / K[1, 1], z
            diag = np.linalg.norm(dims[i])
            nocs[i] = diag
            model[i] = self.meshes.sample_points(k, self.n_model, rng).astype(np.float64) * scale[i].astype(np.float64) / diag
            aug_bb[i] = rng.random(3) * 0.4 + 0.8
            aug_r[i] = euler_zyx(rng.uniform(-15, 15), rng.uniform(-15, 15), rng.uniform(-15, 15))
            aug_t[i] = (rng.random(3) * 100 - 50) / 1000.0
        # the instances: item i under label 1 in frame i, then its distractors under 2, 3, ...
        ids, fr, lab, rts, scs = [mesh_ids], [np.arange(M, dtype=np.int32)], [np.ones(M, np.int32)], [RT], [scale]
        for d, spec in enumerate(self.distractors):
            dsize = np.asarray(spec["size"], dtype=np.float64)
            off = np.tile(np.asarray(spec.get("offset", (0, 0, 0)), dtype=np.float64), (M, 1))
            if spec.get("rest", False):
                off[:, 1] -= 0.5 * dims[:, 1] + 0.5 * dsize[1]
            rt = RT.copy()
            rt[:, :3, 3] = RT[:, :3, 3].astype(np.float64) + np.einsum("mij,mj->mi", RT[:, :3, :3].astype(np.float64), off)
            ids.append(np.full(M, int(spec["mesh"]), np.int32))
            fr.append(np.arange(M, dtype=np.int32))
            lab.append(np.full(M, 2 + d, np.int32))
            rts.append(rt)
            scs.append(np.tile((dsize / self.meshes.extent(int(spec["mesh"]))).astype(np.float32), (M, 1)))
        depth, labels = render_frames(self.meshes, np.concatenate(ids), np.concatenate(rts), np.concatenate(scs), K, self.H, self.W,
                                      frame_ids=np.concatenate(fr), labels=np.concatenate(lab), F=max(M, 1))
        dev = self.meshes.device
        inst = torch.ones(M, dtype=torch.int32, device=dev)
        boxes_d, _ = label_boxes(labels, fr[0], lab[0])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        frames = dict(depth=depth, labels=labels, inst_ids=inst, bboxes_xyxy=boxes_d.cpu().numpy().astype(np.int64),
                      bboxes_d=boxes_d, K=K.copy())
        mean = self.mean_shapes[mesh_ids]
        items = dict(obj_id=up(self.class_ids[mesh_ids]), gt_R=up(RT[:, :3, :3]), gt_t=up(RT[:, :3, 3]), gt_s=up(dims - mean),
                     mean_shape=up(mean), sym=up(self.sym_infos[mesh_ids]), model_point=up(model), nocs_scale=up(nocs),
                     aug_bb=up(aug_bb), aug_rt_t=up(aug_t), aug_rt_r=up(aug_r))
        self.last = dict(RT=RT, scale=scale, mesh_ids=mesh_ids, sizes=dims)
        return frames, items


class SceneSource:
    """``SyntheticItems`` with every draw made on the device under a step's key (include/hsp.h: "scenes drawn under a step's
    key"): the same arguments without ``rng``, the same distributions, not the same draws.  The per-mesh tables, the camera and
    the distractor table go up once, here.

    ``draw(M, key, out=None)``: key the (2,) int64 device tensor {seed, call} of a ``pc_sample.DeviceSampler`` -> the two dicts
    ``train.FrameTrainStep`` takes, with ``bboxes_d`` (M,4) int32 on the device -- ``ops.label_boxes_guarded``'s, so a label
    without a pixel has the box (0, 0, 1, 1) and the front end rejects it by count --, no ``bboxes_xyxy``, ``inst_ids`` all 1 on
    the device and K (1,9) float64 on the device.  Four steps: ``ops.scene_draw`` -> ``ops.mesh_sample`` ->
    ``render_frames(out=...)`` -> ``ops.label_boxes_guarded``.  ``out``: ``buffers(M)``, with any of its tensors replaced
    by the caller's own static ones; given it the call allocates no output, uploads nothing, reads nothing back and can be
    captured.
    ``last`` keeps the device tensors of the last draw (the render's instance rows, angles, count among them)."""

    def __init__(self, meshes, class_ids, mean_shapes, sym_infos, K, H, W, distance=(0.6, 1.4), size=(0.08, 0.3), n_model=1024,
                 elev=(10.0, 60.0), roll=10.0, distractors=()):
        dev = meshes.device
        host = [np.asarray(class_ids, dtype=np.float32).reshape(-1), np.asarray(mean_shapes, dtype=np.float32).reshape(-1, 3),
                np.asarray(sym_infos, dtype=np.float32).reshape(-1, 4)]
        if not len(meshes) == len(host[0]) == len(host[1]) == len(host[2]):
            raise ValueError("SceneSource: class_ids, mean_shapes and sym_infos expect one row per mesh")
        self.meshes, self.H, self.W, self.n_model = meshes, int(H), int(W), int(n_model)
        K = np.asarray(K, dtype=np.float64).reshape(3, 3)
        distance, size, elev = tuple(distance), tuple(size), tuple(elev)
        if not (0 < distance[0] <= distance[1] and 0 < size[0] <= size[1]):
            raise ValueError(f"SceneSource: distance {distance} / size {size} expect 0 < lo <= hi")
        self.params = (*size, *distance, *elev, float(roll), self.W, self.H, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        if len(distractors) > 254:
            raise ValueError("SceneSource: at most 254 distractors (labels 2 ... 255)")
        rows = []
        for spec in distractors:
            if not 0 <= int(spec["mesh"]) < len(meshes):
                raise ValueError(f"SceneSource: distractor mesh {spec['mesh']} outside [0, {len(meshes)})")
            rows.append([int(spec["mesh"]), *spec["size"], *spec.get("offset", (0, 0, 0)), 1.0 if spec.get("rest", False) else 0.0])
        self.D = len(rows)
        self.cls, self.mean_shapes, self.sym_infos = (torch.from_numpy(a).to(dev) for a in host)
        self.distractors = torch.tensor(rows, dtype=torch.float64).reshape(-1, 8).to(dev) if rows else None
        self.K = torch.from_numpy(K.reshape(1, 9).copy()).to(dev)
        self.ext, self.cum = meshes.extents, meshes.cum_area            # (built and uploaded here, not inside a capture)
        self.last = None

    def buffers(self, M):
        """every device tensor one ``draw(M)`` writes, by name: what ``out`` may hold"""
        dev, M = self.meshes.device, int(M)
        n, f32, i32 = M * (1 + self.D), torch.float32, torch.int32
        spec = dict(mesh_id=((n,), i32), frame_id=((n,), i32), label=((n,), i32), RT=((n, 4, 4), f32), scale=((n, 3), f32),
                    obj_id=((M,), f32), gt_R=((M, 3, 3), f32), gt_t=((M, 3), f32), gt_s=((M, 3), f32), mean_shape=((M, 3), f32),
                    sym=((M, 4), f32), nocs_scale=((M,), f32), aug_bb=((M, 3), f32), aug_rt_t=((M, 3), f32),
                    aug_rt_r=((M, 3, 3), f32), angles=((M, 6), torch.float64), model_point=((M, self.n_model, 3), f32),
                    depth=((M, self.H, self.W), torch.uint16), labels=((M, self.H, self.W), torch.uint8), bboxes_d=((M, 4), i32),
                    count=((M,), i32))
        out = {k: torch.zeros(shape, dtype=dtype, device=dev) for k, (shape, dtype) in spec.items()}
        out["inst_ids"] = torch.ones(M, dtype=i32, device=dev)
        return out

    ITEM_KEYS = ("obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "model_point", "nocs_scale", "aug_bb", "aug_rt_t", "aug_rt_r")

    def draw(self, M, key, out=None):
        M, ms = int(M), self.meshes
        o = self.buffers(M) if out is None else dict(out)
        o.update(ops.scene_draw(key, self.ext, self.cls, self.mean_shapes, self.sym_infos, self.params, self.distractors, M, out=o))
        ops.mesh_sample(ms.verts, ms.tris, ms.table, self.cum, self.ext, o["mesh_id"][:M], o["scale"][:M], key, self.n_model,
                        out=o["model_point"])
        render_frames(ms, o["mesh_id"], o["RT"], o["scale"], self.K, self.H, self.W, frame_ids=o["frame_id"], labels=o["label"],
                      F=M, out=(o["depth"], o["labels"]))
        ops.label_boxes_guarded(o["labels"], o["frame_id"][:M], o["label"][:M], out=(o["bboxes_d"], o["count"]))
        self.last = o
        frames = dict(depth=o["depth"], labels=o["labels"], inst_ids=o["inst_ids"], bboxes_d=o["bboxes_d"], K=self.K)
        return frames, {k: o[k] for k in self.ITEM_KEYS}
