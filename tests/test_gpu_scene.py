"""GPU: scenes drawn under a step's key (include/hsp.h; csrc/scene.hip) against their numpy statement (tests/_scene_ref.py), bit
for bit wherever the header promises bits -- everything but the two rotations, whose float64 sines and cosines may differ in
the last place between two libraries: those agree to one fp32 rounding, and what is derived from them is compared bit for bit
against the statement evaluated from the device's own rotation -- and what they are for: ``render.SceneSource`` feeding the
training front end without a host draw, an upload or a read-back, eagerly and as one captured graph."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _render_ref as rr
import _scene_ref as sr
from hs_pose_amd import ops, pc_sample
from hs_pose_amd.render import MeshSet, SceneSource, label_boxes, render_frames, shapes

pytestmark = pytest.mark.gpu
K, H, W = rr.K4, rr.H, rr.W
SEED = 20240607
PARAMS = sr.PARAMS
MESHES = [shapes.box(), shapes.uv_sphere(8, 6), sr.zero_area_mesh()]
MEAN = np.array([[0.1, 0.2, 0.1], [0.05, 0.1, 0.05], [0.2, 0.2, 0.2]], np.float32)
SYM = np.arange(12, dtype=np.float32).reshape(3, 4)
CLS = np.array([0, 3, 5], np.float32)
DIST = [[0, 0.5, 0.02, 0.4, 0.0, 0.0, 0.0, 1.0], [0, 0.05, 0.06, 0.07, 0.1, -0.02, 0.03, 0.0]]       # a slab that rests, a box beside
ROT_TOL = 2.0 ** -23      # entries lie in [-1, 1] and float64 sine / cosine errors are ~1e-16: the two can differ only where
#                           that moves a value across an fp32 rounding boundary, by one ulp <= 2^-23


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def key_of(seed, call, dev):
    return torch.tensor([seed, call], dtype=torch.int64, device=dev)


def tables(n_mesh, dev):
    ext = np.stack([v.astype(np.float64).max(0) - v.astype(np.float64).min(0) for v, _ in MESHES[:n_mesh]])
    host = (ext, CLS[:n_mesh], MEAN[:n_mesh], SYM[:n_mesh])
    return host, tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)


def device_scene(dev, M, D, n_mesh, call=0):
    host, d = tables(n_mesh, dev)
    dist = torch.tensor(DIST[:D], dtype=torch.float64, device=dev) if D else None
    return host, ops.scene_draw(key_of(SEED, call, dev), *d, list(PARAMS.values()), dist, M)


@pytest.mark.parametrize("n_mesh", [1, 3])
@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("M", [1, 5, 70])
def test_scene_draw_equals_the_statement(dev, M, D, n_mesh):
    host, got = device_scene(dev, M, D, n_mesh)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    want = sr.scene_draw(SEED, 0, M, *host, list(PARAMS.values()), DIST[:D])
    assert np.array_equal(bits(got["angles"]), bits(want["angles"]))
    for k in ("gt_R", "aug_rt_r"):
        worst = np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)).max()
        print(f"{k}: largest difference to the statement {worst:.3e} (bound {ROT_TOL:.3e})")
        assert worst <= ROT_TOL, k
    # everything that does not come from R: bit for bit; everything that does: bit for bit from the device's own R
    own = sr.scene_draw(SEED, 0, M, *host, list(PARAMS.values()), DIST[:D], R=got["gt_R"])
    for k in got:
        if k != "aug_rt_r":
            assert got[k].shape == own[k].shape and np.array_equal(bits(got[k]), bits(own[k])), k
    for k in ("mesh_id", "frame_id", "label", "scale", "obj_id", "gt_t", "gt_s", "mean_shape", "sym", "nocs_scale", "aug_bb", "aug_rt_t"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(bits(got["RT"][:M, :, 3]), bits(want["RT"][:M, :, 3])) and np.array_equal(bits(got["RT"][:, 3]), bits(want["RT"][:, 3]))
    if n_mesh == 3 and M == 70:
        assert set(got["mesh_id"][:M].tolist()) == {0, 1, 2}


def test_scene_draw_is_a_function_of_key_and_index(dev):
    _, a = device_scene(dev, 70, 2, 3)
    _, again = device_scene(dev, 70, 2, 3)
    _, five = device_scene(dev, 5, 2, 3)
    _, nxt = device_scene(dev, 70, 2, 3, call=1)
    for k in a:
        assert torch.equal(a[k], again[k]), k
    for k in ("obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "nocs_scale", "aug_bb", "aug_rt_t", "aug_rt_r", "angles"):
        assert torch.equal(a[k][:5], five[k]), k                    # an item depends on its index, not on M
    for d in range(3):                                              # the instance rows of items and of each distractor
        for k in ("mesh_id", "RT", "scale"):
            assert torch.equal(a[k][d * 70:d * 70 + 5], five[k][d * 5:d * 5 + 5]), (k, d)
    assert bool((a["angles"] != nxt["angles"]).all()) and bool((a["gt_t"] != nxt["gt_t"]).any(dim=1).all())


def test_scene_draw_into_caller_owned_outputs(dev):
    _, fresh = device_scene(dev, 5, 2, 3)
    (_, d), out = tables(3, dev), {k: torch.full_like(v, 7) for k, v in fresh.items() if k in ("RT", "gt_R", "angles", "label")}
    got = ops.scene_draw(key_of(SEED, 0, dev), *d, list(PARAMS.values()), torch.tensor(DIST, dtype=torch.float64, device=dev), 5, out=out)
    assert all(got[k] is out[k] for k in out) and all(torch.equal(got[k], fresh[k]) for k in fresh)


@pytest.mark.parametrize("n_model", [1, 64, 1000])
def test_mesh_sample_equals_the_statement(dev, n_model):
    ms = MeshSet(MESHES, device=dev)
    mesh_id = np.array([0, 1, 2], np.int32)
    scale = np.array([[0.07] * 3, [0.31] * 3, [0.1, 0.2, 0.15]], np.float32)           # three scales, one of them per axis
    got = ops.mesh_sample(ms.verts, ms.tris, ms.table, ms.cum_area, ms.extents, torch.from_numpy(mesh_id).to(dev),
                          torch.from_numpy(scale).to(dev), key_of(SEED, 2, dev), n_model)
    want = sr.mesh_sample(SEED, 2, MESHES, mesh_id, scale, n_model)
    assert tuple(got.shape) == (3, n_model, 3) and np.array_equal(bits(got), bits(want))
    assert np.isfinite(want).all() and np.abs(want).max() <= 0.5 * (1 + 2.0 ** -20)    # units of the diagonal: inside the half diagonal
    # a mesh the table does not hold gives zero points, and reads nothing
    off = ops.mesh_sample(ms.verts, ms.tris, ms.table, ms.cum_area, ms.extents, torch.tensor([3, -1, 0], dtype=torch.int32, device=dev),
                          torch.from_numpy(scale).to(dev), key_of(SEED, 2, dev), n_model)
    assert not off[:2].any() and np.array_equal(bits(off[2]), bits(sr.mesh_sample(SEED, 2, MESHES, [0, 0, 0], scale, n_model)[2]))


@pytest.mark.parametrize("shape", [(2, 48, 64), (3, 37, 53)])
def test_label_boxes_guarded(dev, shape):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 5, shape).astype(np.uint8)
    img[img == 4] = 0                                               # label 4 is absent everywhere
    img[0][img[0] == 3] = 0
    img[0, 0, 7], img[0, -1, 9], img[0, 5, 0], img[0, 11, -1] = 3, 3, 3, 3      # label 3 of frame 0 touches all four borders
    fid = np.array([0, 0, shape[0] - 1, 0, shape[0] - 1, shape[0], 0], np.int32)
    lab = np.array([1, 3, 4, 4, 2, 1, 0], np.int32)
    d = torch.from_numpy(img).to(dev)
    boxes, count = ops.label_boxes_guarded(d, torch.from_numpy(fid).to(dev), torch.from_numpy(lab).to(dev))
    plain_b, plain_c = label_boxes(d, fid, lab)
    wb, wc = rr.label_boxes(img, fid, lab)
    assert np.array_equal(plain_b.cpu().numpy(), wb) and np.array_equal(count.cpu().numpy(), wc) and torch.equal(count, plain_c)
    assert boxes[1].tolist() == [0, 0, shape[2], shape[1]] and wc.tolist()[2:4] == [0, 0] and wc[0] > 0 and wc[4] > 0
    some = torch.from_numpy(wc > 0).to(dev)
    assert torch.equal(boxes[some], plain_b[some])
    assert boxes[~some].tolist() == [[0, 0, 1, 1]] * int((wc == 0).sum()) and not plain_b[~some].any()


# ---- what it is for ----------------------------------------------------------------------------------------------------------

def box_source(dev, **kw):
    msb = MeshSet([shapes.box()], device=dev)
    slab = dict(mesh=0, size=(0.8, 0.02, 0.8), rest=True)
    return SceneSource(msb, [0], [[0.1, 0.2, 0.1]], [[0, 0, 0, 0]], K.reshape(3, 3), H, W, distance=(0.5, 0.8), size=(0.15, 0.3),
                       n_model=64, distractors=[slab], **kw)


def test_scene_source_feeds_the_training_chain(dev, flags):
    """SceneSource.draw(6), a box with a slab under it: the frames are an eager render of the drawn instance rows; every accepted
    item's cloud rows, moved into its object frame by the drawn pose, lie within 0.5 mm * |ray| of the box's surface (one rint of
    the depth along the ray); an item hidden behind a nearer full-frame instance gets the guarded box, a finite window and a
    rejection"""
    src = box_source(dev)
    frames, items = src.draw(6, key_of(26, 0, dev))
    o = src.last
    assert "bboxes_xyxy" not in frames and frames["inst_ids"].tolist() == [1] * 6 and frames["bboxes_d"].dtype == torch.int32
    assert tuple(items["model_point"].shape) == (6, 64, 3) and tuple(o["mesh_id"].shape) == (12,)
    ed, el = render_frames(src.meshes, o["mesh_id"], o["RT"], o["scale"], src.K, H, W, frame_ids=o["frame_id"], labels=o["label"], F=6)
    assert torch.equal(ed, frames["depth"]) and torch.equal(el, frames["labels"]) and bool((el == 2).any())
    wb, wc = rr.label_boxes(el.cpu().numpy(), range(6), [1] * 6)
    assert np.array_equal(o["count"].cpu().numpy(), wc) and (wc > 0).all() and np.array_equal(frames["bboxes_d"].cpu().numpy(), wb)
    sampler = pc_sample.DeviceSampler(21, dev)

    def clouds(fr, boxes):
        xf = ops.dzi_windows_device(boxes, sampler.advance(), H, W, 32, float(flags.DZI_PAD_SCALE), 0.0, 0.0)
        return xf, pc_sample.train_batch_to_pcl(fr["depth"], fr["labels"], fr["inst_ids"], xf, None, src.K, n_pts=64, out_size=32,
                                                mask_pro=0, sampler=sampler)
    _, (PC, status) = clouds(frames, frames["bboxes_d"])
    good = [i for i in range(6) if status[i].item() == 0]
    assert len(good) >= 3, status.tolist()
    P = PC.cpu().numpy().astype(np.float64)
    R, t = items["gt_R"].cpu().numpy().astype(np.float64), items["gt_t"].cpu().numpy().astype(np.float64)
    half = 0.5 * o["scale"][:6].cpu().numpy().astype(np.float64)   # the unit box: its sides are the scale, exactly
    assert torch.allclose(items["gt_s"] + items["mean_shape"], o["scale"][:6])
    worst = -np.inf
    for i in good:
        q = (P[i] - t[i]) @ R[i]                                    # R^T (p - t), row-wise
        bound = 0.0005 * np.linalg.norm(P[i] / P[i][:, 2:3], axis=-1)
        excess = rr.box_distance(q, half[i]) - bound
        worst = max(worst, excess.max())
        assert excess.max() <= 0, f"item {i}: {excess.max()} m beyond the bound"
    print(f"accepted {good}; largest distance minus bound {worst:.3e} m")
    # item good[0] again behind a wall 5 cm from the camera, nearer than any item: its label has no pixel
    g, wall = good[0], torch.eye(4, device=dev).reshape(1, 4, 4).clone()
    wall[0, 2, 3] = 0.05
    cat = lambda a, b: torch.cat([a, torch.as_tensor(b, dtype=a.dtype, device=dev)])
    d2, l2 = render_frames(src.meshes, cat(o["mesh_id"], [0]), cat(o["RT"], wall), cat(o["scale"], [[0.5, 0.5, 0.001]]), src.K, H, W,
                           frame_ids=cat(o["frame_id"], [g]), labels=cat(o["label"], [3]), F=6)
    assert not bool((l2[g] == 1).any()) and bool((l2[g] == 3).any())
    b2, c2 = ops.label_boxes_guarded(l2, o["frame_id"][:6], o["label"][:6])
    assert b2[g].tolist() == [0, 0, 1, 1] and c2[g].item() == 0 and torch.equal(b2[good[1:]], frames["bboxes_d"][good[1:]])
    xf, (_, status2) = clouds(dict(frames, depth=d2, labels=l2), b2)
    assert bool(torch.isfinite(xf).all()) and status2[g].item() != 0 and status2[good[1:]].tolist() == [0] * (len(good) - 1)


def test_scene_source_draw_is_capturable(dev):
    src, sampler = box_source(dev), pc_sample.DeviceSampler(26, dev)
    bufs = src.buffers(6)
    sampler.advance()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src.draw(6, sampler.key, out=bufs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frames, items = src.draw(6, sampler.key, out=bufs)
    assert frames["depth"] is bufs["depth"] and items["gt_R"] is bufs["gt_R"] and frames["bboxes_d"] is bufs["bboxes_d"]
    first = bufs["gt_t"].clone()
    sampler.advance()
    sampler.advance()                                               # the key now holds call 2
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in bufs.items()}
    src.draw(6, key_of(26, 2, dev))
    assert not torch.equal(got["gt_t"], first)
    for k, v in src.last.items():
        assert torch.equal(got[k], v), k


@pytest.mark.parametrize("mode", ["twin", "occluded"])
def test_rendered_train_step(mode):
    """tests/_rendered_train_check.py in a fresh process (a capture must precede the network's first eager backward)"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_rendered_train_check.py")
    r = subprocess.run([sys.executable, script, mode], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
