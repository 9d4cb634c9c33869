"""The renderer on the GPU (csrc/render.hip: hsp_render_depth_*, hsp_label_boxes; ops.render_depth / label_boxes;
hs_pose_amd/render.py) against the numpy statement of its contract (tests/_render_ref.py, itself held to analytic geometry by
tests/test_render_host.py).  Everything is compared as integers or bit patterns, with no tolerance; frames are 48 x 64 with
K = (60, 60, 31.5, 23.5) unless a case says otherwise.

Then what the renderer is for: the mask-fed and the pose-fed crop chains list the same pixels on a rendered scene, and the training
chain cuts clouds that lie on the surface that was in front of the camera -- under the bound tests/test_render_host.py derives,
0.5 mm * |ray| (one rint of the depth along the ray), not a tuned one."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _render_ref as rr
from hs_pose_amd.render import MeshSet, SyntheticItems, euler_zyx, label_boxes, render_frames, shapes

pytestmark = pytest.mark.gpu
K, H, W = rr.K4, rr.H, rr.W
MESHES = [shapes.box(), shapes.cylinder(24), shapes.uv_sphere(48, 32), shapes.mug(16)]
BOX, CYL, SPH, MUG = range(4)
NP_OF = {torch.uint16: np.uint16, torch.float32: np.float32}
DTYPES = [torch.uint16, torch.float32]


@pytest.fixture(scope="module")
def ms(dev):
    return MeshSet(MESHES, device=dev)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def slab_under(RT, size, thick=0.02, side=0.8):
    """a ground slab under a posed object: (RT, size) of a box of ``side`` x ``thick`` x ``side`` whose top touches the object's
    underside (the object's -y)"""
    rt = RT.copy()
    rt[:3, 3] = RT[:3, 3].astype(np.float64) + RT[:3, :3].astype(np.float64) @ np.array([0.0, -0.5 * size[1] - 0.5 * thick, 0.0])
    return rt, np.array([side, thick, side], np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(mesh_id, frame_id, label, RT, scale, K, F): seeded instances, shared by the tests below"""
    rng = np.random.default_rng(sum(map(ord, name)))
    one = lambda m, RT, s, **kw: dict(mesh_id=[m], frame_id=[0], label=[1], RT=RT[None], scale=np.asarray(s, np.float32)[None], K=K, F=1, **kw)
    if name == "box":
        return one(BOX, *rr.box_pose(3))
    if name == "cylinder":
        return one(CYL, rr.pose(rr.rotation(21), [0.03, -0.02, 0.7]), [0.2, 0.3, 0.2])
    if name == "sphere":
        return one(SPH, rr.pose(rr.rotation(22), [0.05, -0.03, 0.9]), [0.2, 0.2, 0.2])
    if name == "half_off":                                          # centre near the left edge: the boxes are clamped
        return one(BOX, rr.pose(rr.rotation(23), [-0.33, 0.2, 0.65]), [0.25, 0.2, 0.3])
    if name == "behind":                                            # some vertices behind the camera: those triangles are dropped
        return one(BOX, rr.pose(rr.rotation(8), [0.0, 0.0, 0.12]), [0.3, 0.3, 0.3])
    if name == "mug_slab":                                          # camera above (slab occluded by the mug) and below (slab occludes)
        out = dict(mesh_id=[], frame_id=[], label=[], RT=[], scale=[], K=K, F=2)
        for f, elev in enumerate((35.0, -25.0)):
            R = euler_zyx(180.0 + elev, 0, 0) @ euler_zyx(0, 30.0, 0)
            RT, size = rr.pose(R.astype(np.float32), [0.02, 0.03, 0.8]), np.array([0.16, 0.2, 0.16], np.float32)
            srt, ssize = slab_under(RT, size * (MESHES[MUG][0].max(0) - MESHES[MUG][0].min(0)))
            out["mesh_id"] += [MUG, BOX]; out["frame_id"] += [f, f]; out["label"] += [1, 2]
            out["RT"] += [RT, srt]; out["scale"] += [size, ssize]
        out["RT"], out["scale"] = np.stack(out["RT"]), np.stack(out["scale"])
        return out
    if name in ("frames3", "frames3_cams"):                         # 5 instances over 3 frames, unevenly: 3 + 0 + 2
        fr, me = [0, 2, 0, 2, 0], [BOX, CYL, MUG, BOX, CYL]
        RT = np.stack([rr.pose(rr.rotation(40 + j), [rng.uniform(-0.2, 0.2), rng.uniform(-0.12, 0.12), rng.uniform(0.5, 1.0)]) for j in range(5)])
        Ks = K if name == "frames3" else np.stack([K * s for s in (1.0, 0.9, 1.15)])
        return dict(mesh_id=me, frame_id=fr, label=[3, 1, 250, 2, 9], RT=RT, scale=rng.uniform(0.1, 0.3, (5, 3)).astype(np.float32), K=Ks, F=3)
    if name == "both_paths":                                        # a triangle over 1000 pixels and triangles under a pixel
        RT = np.stack([rr.pose(rr.rotation(51), [0.0, 0.0, 0.42]), rr.pose(rr.rotation(52), [0.1, 0.05, 1.3])])
        return dict(mesh_id=[BOX, SPH], frame_id=[0, 0], label=[1, 2], RT=RT, scale=np.array([[0.3] * 3, [0.2] * 3], np.float32), K=K, F=1)
    if name == "queue_full":                                        # more chunks than the queue holds: lanes draw the rest
        n = 6
        RT = np.stack([rr.pose(rr.rotation(60 + j), [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(0.4, 0.5)]) for j in range(n)])
        return dict(mesh_id=[BOX] * n, frame_id=[0] * n, label=list(range(1, n + 1)), RT=RT, scale=np.full((n, 3), 0.3, np.float32), K=K, F=1)
    if name == "bad_ids":                                           # instances that name nothing draw nothing; the good one is drawn
        RT, size = rr.box_pose(4)
        return dict(mesh_id=[len(MESHES), -1, BOX, BOX, BOX, BOX, BOX], frame_id=[0, 0, 1, -1, 0, 0, 0], label=[1, 1, 1, 1, 0, 256, 5],
                    RT=np.stack([RT] * 7), scale=np.stack([size] * 7), K=K, F=1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def want(name, dtype):
    c, stats = case(name), {}
    d, l = rr.render(MESHES, c["mesh_id"], c["frame_id"], c["label"], c["RT"], c["scale"], c["K"], c["F"], H, W, dtype=NP_OF[dtype], stats=stats)
    return d, l, stats


def gpu(ms, c, dtype=torch.uint16, **kw):
    return render_frames(ms, c["mesh_id"], c["RT"], c["scale"], np.asarray(c["K"]).reshape(-1, 3, 3), H, W, frame_ids=c["frame_id"],
                         labels=c["label"], F=c["F"], dtype=dtype, **kw)


CASES = ["box", "cylinder", "sphere", "mug_slab", "frames3", "frames3_cams", "half_off", "behind", "both_paths", "queue_full", "bad_ids"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["u16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_render_equals_the_statement(ms, name, dtype):
    d, l = gpu(ms, case(name), dtype)
    wd, wl, stats = want(name, dtype)
    assert d.dtype == dtype and l.dtype == torch.uint8 and tuple(d.shape) == (case(name)["F"], H, W)
    assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(l), wl)
    assert wl.any(), "the case draws nothing"
    if name == "mug_slab":                                          # the slab is occluded in frame 0 and occludes in frame 1
        alone = rr.render(MESHES, [MUG, MUG], [0, 1], [1, 1], case(name)["RT"][::2], case(name)["scale"][::2], K, 2, H, W)[1]
        assert ((alone[0] == 1) == (wl[0] == 1)).all() and (wl[0] == 2).any() and ((alone[1] == 1) & (wl[1] == 2)).any()
    if name == "both_paths":                                        # (the sizes that decide the kernel's path, from the statement)
        assert stats["boxes"].max() > 1000 and stats["boxes"].min() <= 4 and stats["fragments"] > 0
    if name == "queue_full":                                        # 16 frames' worth of chunks is the queue: 16 * 3 here
        chunks = sum(int(np.ceil(b / 1024)) for b in stats["boxes"] if b > 64)
        assert chunks > 16 * 3
    if name == "behind":
        assert len(stats["boxes"]) < 12
    if name == "bad_ids":
        assert set(np.unique(wl)) == {0, 5}


@pytest.mark.parametrize("dtype", DTYPES, ids=["u16", "f32"])
def test_render_is_order_free(ms, dtype):
    c = case("both_paths")
    a, b = gpu(ms, c, dtype), gpu(ms, c, dtype)
    assert np.array_equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])
    rng = np.random.default_rng(5)
    shuffled = MeshSet([(v, f[rng.permutation(len(f))]) for v, f in MESHES], device=ms.device)
    s = gpu(shuffled, c, dtype)
    assert np.array_equal(bits(s[0]), bits(a[0])) and torch.equal(s[1], a[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["u16", "f32"])
def test_render_over_a_prefilled_frame(ms, dev, dtype):
    c, npd = case("frames3"), NP_OF[dtype]
    rng = np.random.default_rng(9)
    bg_d = rng.integers(0, 1400, (3, H, W)).astype(npd)
    bg_d[rng.random((3, H, W)) < 0.3] = 0                          # holes: empty pixels
    if dtype == torch.float32:
        bg_d[0, 0, :4] = [-1.0, np.nan, np.inf, 1e-3]
    bg_l = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    wd, wl = rr.render(MESHES, c["mesh_id"], c["frame_id"], c["label"], c["RT"], c["scale"], K, 3, H, W, dtype=npd, depth=bg_d, labels=bg_l)
    # caller-owned frames, once on aligned buffers (four pixels per lane) and once on views that are not (one pixel per lane)
    for shift in (0, 1):
        buf_d = torch.zeros(3 * H * W + shift, dtype=dtype, device=dev)
        buf_l = torch.zeros(3 * H * W + shift, dtype=torch.uint8, device=dev)
        d, l = buf_d[shift:].view(3, H, W), buf_l[shift:].view(3, H, W)
        d.copy_(torch.from_numpy(bg_d)); l.copy_(torch.from_numpy(bg_l))
        got = gpu(ms, c, dtype, out=(d, l), over=True)
        assert got[0].data_ptr() == d.data_ptr() and got[1].data_ptr() == l.data_ptr()
        assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(l), wl)
    assert (wl != bg_l).any() and ((wl == bg_l) & (bg_d > 0)).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["u16", "f32"])
def test_render_nothing(ms, dev, dtype):
    none = dict(mesh_id=[], frame_id=[], label=[], RT=np.zeros((0, 4, 4), np.float32), scale=np.zeros((0, 3), np.float32), K=K, F=2)
    d, l = gpu(ms, none, dtype)
    assert tuple(d.shape) == (2, H, W) and not bits(d).any() and not l.any()
    d = torch.from_numpy(np.full((2, H, W), 7, NP_OF[dtype])).to(dev)
    l = torch.full((2, H, W), 3, dtype=torch.uint8, device=dev)
    gpu(ms, none, dtype, out=(d, l), over=True)
    assert (d.cpu().numpy() == 7).all() and (l == 3).all()
    # an odd frame: the vector tail of the resolve, and boxes clamped at an odd width
    c = case("box")
    odd = render_frames(ms, c["mesh_id"], c["RT"], c["scale"], K.reshape(3, 3), 47, 61, dtype=dtype)
    wd, wl = rr.render(MESHES, c["mesh_id"], [0], [1], c["RT"], c["scale"], K, 1, 47, 61, dtype=NP_OF[dtype])
    assert np.array_equal(bits(odd[0]), bits(wd)) and np.array_equal(bits(odd[1]), wl)


def test_label_boxes_equal_np_where(dev):
    rng = np.random.default_rng(3)
    for shape in ((3, 47, 61), (2, H, W), (1, 5, 7)):              # odd frames start off a 16-byte boundary: head, body and tail
        img = rng.integers(0, 6, shape).astype(np.uint8)
        img[0, :, :2] = 0
        img[-1][img[-1] == 4] = 0                                   # label 4 has no pixel in the last frame
        fid = np.array([0, shape[0] - 1, shape[0] - 1, 0, 0, shape[0], -1, 0, 0], np.int32)
        lab = np.array([1, 4, 5, 5, 200, 1, 1, 0, 256], np.int32)
        boxes, count = label_boxes(torch.from_numpy(img).to(dev), fid, lab)
        wb, wc = rr.label_boxes(img, fid, lab)
        assert boxes.dtype == torch.int32 and count.dtype == torch.int32
        assert np.array_equal(boxes.cpu().numpy(), wb) and np.array_equal(count.cpu().numpy(), wc)
        assert wc[1] == 0 and wc[4] == 0 and wc[0] > 0
    one = np.zeros((1, H, W), np.uint8)
    one[0, H - 1, W - 1] = 255
    boxes, count = label_boxes(torch.from_numpy(one).to(dev), [0], [255])
    assert boxes.tolist() == [[W - 1, H - 1, W, H]] and count.tolist() == [1]


def test_bad_arguments_launch_nothing(ms, dev):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import ERR_BAD_ARG, ERR_WORKSPACE, HspError, lib
    L, p, null = lib(), (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(0)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    zero, one_, four = i32(0), i32(1), i32(0, 0, 0, 0)
    RT, sc, Kd = torch.eye(4, device=dev).reshape(1, 16), torch.ones(1, 3, device=dev), torch.from_numpy(K).to(dev)
    d = torch.from_numpy(np.full((1, H, W), 9, np.uint16)).to(dev)
    l = torch.full((1, H, W), 9, dtype=torch.uint8, device=dev)
    wsb = L.hsp_render_workspace_bytes(1, H, W, 1)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)

    def call(**kw):
        a = dict(verts=p(ms.verts), V=ms.verts.shape[0], tris=p(ms.tris), T=ms.tris.shape[0], mesh=p(ms.table), n_mesh=len(ms),
                 mesh_id=p(zero), frame_id=p(zero), label=p(one_), rt=p(RT), scale=p(sc), camK=p(Kd), camK_rows=1, n=1, F=1, H=H,
                 W=W, over=0, depth=p(d), labels=p(l), ws=p(ws), ws_bytes=wsb, stream=null)
        a.update(kw)
        return L.hsp_render_depth_u16(*a.values())
    for kw in (dict(verts=null), dict(labels=null), dict(n=65536), dict(over=2), dict(camK_rows=3), dict(W=0)):
        assert call(**kw) == ERR_BAD_ARG, kw
    assert call(ws_bytes=wsb - 1) == ERR_WORKSPACE
    assert L.hsp_label_boxes(p(l), p(zero), p(one_), 0, 1, H, W, p(four), p(zero), null) == ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 9).all() and (l == 9).all()          # nothing ran
    with pytest.raises(HspError):
        ops.render_depth(ms.verts, ms.tris, ms.table, zero, zero, one_, RT, sc, Kd.reshape(1, 9), 1, H, W, over=True)


# ---- what the renderer is for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("background", [False, True], ids=["empty", "plane"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u16", "f32"])
def test_mask_fed_equals_pose_fed(ms, dev, dtype, background):
    """one box over an empty frame, and over a plane 0.5 m behind it: cut by its label and cut by its true pose padded by 1.2,
    the crop chains list the same pixels.  The box's points lie within 0.61 mm of its surface (0.5 mm * |ray| <= 0.5 * 1.22) and the
    padded half extents are at least 0.1 * 8 cm = 8 mm further out; the plane is 0.5 m behind, the padded half diagonal at most
    0.6 * 0.3 * sqrt(3) = 0.31 m."""
    from hs_pose_amd import ops
    O = 32
    for seed in (3, 7, 12):
        RT, size = rr.box_pose(seed)
        plane = round((float(RT[2, 3]) + 0.5) * 1000) if background else 0
        d = torch.from_numpy(np.full((1, H, W), plane, NP_OF[dtype])).to(dev)
        l = torch.zeros(1, H, W, dtype=torch.uint8, device=dev)
        render_frames(ms, [BOX], RT[None], size[None], K.reshape(3, 3), H, W, labels=[7], out=(d, l), over=True)
        assert (l == 7).sum() > 20 and (d.cpu().numpy()[l.cpu().numpy() == 0] == plane).all()
        RTd, sd = torch.from_numpy(RT[None]).to(dev), torch.from_numpy(size[None]).to(dev)
        Kd = torch.from_numpy(K.reshape(1, 9)).to(dev)
        boxes, xf, wstatus = ops.pose_windows(RTd, sd, Kd, H, W, O, 1.2)
        assert wstatus.tolist() == [0]
        src_p, cnt_p = ops.roi_compact_box(d[0], RTd, sd, 1.2, Kd, xf, O)
        src_m, cnt_m = ops.roi_compact(d[0], (l == 7).to(torch.uint8), xf, O)
        n = int(cnt_m[0, 0])
        assert n > 50 and cnt_p.tolist() == cnt_m.tolist()
        assert torch.equal(src_p[0, :n], src_m[0, :n])


def test_training_chain_on_rendered_items(dev, flags):
    """pc_sample.train_batch_to_pcl on SyntheticItems.draw(6): every item is accepted and every cloud row, moved into its item's
    object frame by gt_R, gt_t, lies within 0.5 mm * |ray| of the box's surface; an item rendered off the frame is rejected"""
    from hs_pose_amd import ops, pc_sample
    msb = MeshSet([shapes.box()], device=dev)
    src = SyntheticItems(msb, [0], [[0.1, 0.2, 0.1]], [[0, 0, 0, 0]], K.reshape(3, 3), H, W, distance=(0.5, 0.8), size=(0.15, 0.3),
                         rng=np.random.default_rng(17), n_model=64)
    frames, items = src.draw(6)
    assert frames["depth"].dtype == torch.uint16 and tuple(frames["depth"].shape) == (6, H, W)
    assert np.array_equal(frames["bboxes_xyxy"], rr.label_boxes(frames["labels"].cpu().numpy(), range(6), [1] * 6)[0])
    assert torch.allclose(items["gt_s"] + items["mean_shape"], torch.from_numpy(src.last["sizes"]).float().to(dev))
    sampler = pc_sample.DeviceSampler(21, dev)
    Kd = torch.from_numpy(K.reshape(1, 9)).to(dev)

    def clouds(fr):
        xf = ops.dzi_windows_device(frames["bboxes_d"], sampler.advance(), H, W, 32, float(flags.DZI_PAD_SCALE), 0.0, 0.0)
        return pc_sample.train_batch_to_pcl(fr["depth"], fr["labels"], fr["inst_ids"], xf, None, Kd, n_pts=64, out_size=32, mask_pro=0,
                                            sampler=sampler)
    PC, status = clouds(frames)
    assert status.tolist() == [0] * 6
    P = PC.cpu().numpy().astype(np.float64)
    R, t = items["gt_R"].cpu().numpy().astype(np.float64), items["gt_t"].cpu().numpy().astype(np.float64)
    worst = -np.inf
    for i in range(6):
        q = (P[i] - t[i]) @ R[i]                                    # R^T (p - t), row-wise
        bound = 0.0005 * np.linalg.norm(P[i] / P[i][:, 2:3], axis=-1)
        excess = rr.box_distance(q, 0.5 * src.last["sizes"][i]) - bound
        worst = max(worst, excess.max())
        assert excess.max() <= 0, f"item {i}: {excess.max()} m beyond the bound"
    print(f"largest distance minus bound {worst:.3e} m")
    # item 0 again, moved off the frame: its frame is empty, the box a detector would still pass is not
    far = src.last["RT"][:1].copy()
    far[0, 0, 3] += 5.0
    d0, l0 = render_frames(msb, [0], far, src.last["scale"][:1], K.reshape(3, 3), H, W)
    assert not l0.any() and label_boxes(l0, [0], [1])[1].tolist() == [0]
    depth = frames["depth"].clone()
    depth[:1].copy_(d0)
    gone = dict(frames, depth=depth, labels=torch.cat([l0, frames["labels"][1:]]))
    status = clouds(gone)[1]
    assert status[0].item() != 0 and status[1:].tolist() == [0] * 5


def test_render_is_capturable(ms, dev):
    c = case("frames3")
    n, F = 5, 3
    up = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)
    mesh_id, frame_id, label = (up(c[k], torch.int32) for k in ("mesh_id", "frame_id", "label"))
    RT, scale, Kd = up(c["RT"], torch.float32), up(c["scale"], torch.float32), up(K.reshape(1, 3, 3), torch.float64)
    d = torch.zeros(F, H, W, dtype=torch.uint16, device=dev)
    l = torch.zeros(F, H, W, dtype=torch.uint8, device=dev)

    def body():
        render_frames(ms, mesh_id, RT, scale, Kd, H, W, frame_ids=frame_id, labels=label, F=F, out=(d, l))
        return label_boxes(l, frame_id, label)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        boxes, count = body()
    moved = c["RT"].copy()
    moved[:, :3, 3] += np.array([0.03, -0.02, 0.1], np.float32)
    RT.copy_(up(moved, torch.float32))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (d, l, boxes, count)]
    ed, el = render_frames(ms, mesh_id, RT, scale, Kd, H, W, frame_ids=frame_id, labels=label, F=F)
    eb, ec = label_boxes(el, frame_id, label)
    wd, wl = rr.render(MESHES, c["mesh_id"], c["frame_id"], c["label"], moved, c["scale"], K, F, H, W)
    assert np.array_equal(bits(ed), wd) and np.array_equal(bits(el), wl) and not np.array_equal(wl, want("frames3", torch.uint16)[1])
    for a, b in zip(got, (ed, el, eb, ec)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
