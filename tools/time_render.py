"""The renderer (hs_pose_amd/render.py: render_frames + label_boxes) at the batch one training step consumes -- F = M = 24
frames of 480 x 640 uint16, one item each -- timed in ONE process beside what it replaces and what it feeds:

  render_<geometry>   one hipGraph replay of render_frames + label_boxes into static frames, for
                        box          the 12-triangle box, sides 20 cm, at 0.8 m
                        sphere_near  uv_sphere(128, 64), 16 128 triangles, 20 cm across, at 0.6 m
                        sphere_far   the same at 1.5 m
                        *_slab       the same with a 1.2 m ground slab under every item (48 instances)
  render_empty        the same call with no instance: the key buffer initialised and resolved, no raster pass
  label_boxes_box     label_boxes alone on the box frames.  A geometry's figure minus render_empty minus this one is its raster
                      pass (prefix + both raster kernels)
  load_pinned         ``FrameTrainStep.load(frames=...)`` of 24 such frames and label images from pinned host memory
  step                ``FrameTrainStep.run(check=False)`` at 16 kept of 24 sent, N = 1028, O = 256, on items ``SyntheticItems``
                      drew and rendered

All forms are built first, then timed ALTERNATELY in rounds like tools/time_pool_sampler.py: every round a window of ``--steps``
calls between device events after a synchronise, wall clock alongside; the figures are the median over the rounds with the
min - max spread.  ``--fragments`` counts, on the host with the tests' numpy statement and without a GPU, the fragments each
geometry issues (slow: minutes).  Run on the GPU box:  python tools/time_render.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

F, H, W = 24, 480, 640
K = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]], dtype=np.float64)
BOX, SPHERE = 0, 1
GEOMETRIES = {"box": (BOX, 0.8, False), "sphere_near": (SPHERE, 0.6, False), "sphere_far": (SPHERE, 1.5, False),
              "box_slab": (BOX, 0.8, True), "sphere_near_slab": (SPHERE, 0.6, True), "sphere_far_slab": (SPHERE, 1.5, True)}


def meshes():
    from hs_pose_amd.render import shapes
    return [shapes.box(), shapes.uv_sphere(128, 64)]


def instances(mesh, z, slab, seed=0):
    """F items of ``mesh``, 20 cm across, at depth z, centred within 60 pixels of the principal point, seen from 30 degrees above
    under a seeded yaw; with ``slab`` a 1.2 x 0.02 x 1.2 m box under each -> dict(mesh_id, frame_id, label, RT, scale)"""
    from hs_pose_amd.render import euler_zyx
    rng = np.random.default_rng(seed)
    out = dict(mesh_id=[], frame_id=[], label=[], RT=[], scale=[])
    for f in range(F):
        RT = np.eye(4, dtype=np.float32)
        RT[:3, :3] = euler_zyx(210.0, 0, 0) @ euler_zyx(0, rng.uniform(0, 360), 0)
        cx, cy = K[0, 2] + rng.uniform(-60, 60), K[1, 2] + rng.uniform(-60, 60)
        RT[:3, 3] = z * (cx - K[0, 2]) / K[0, 0], z * (cy - K[1, 2]) / K[1, 1], z
        todo = [(mesh, RT, (0.2, 0.2, 0.2), 1)]
        if slab:
            rt = RT.copy()
            rt[:3, 3] = RT[:3, 3].astype(np.float64) + RT[:3, :3].astype(np.float64) @ np.array([0.0, -0.11, 0.0])
            todo.append((BOX, rt, (1.2, 0.02, 1.2), 2))
        for m, rt, s, l in todo:
            out["mesh_id"].append(m); out["frame_id"].append(f); out["label"].append(l); out["RT"].append(rt); out["scale"].append(s)
    return {k: np.asarray(v, dtype=np.float32 if k in ("RT", "scale") else np.int32) for k, v in out.items()}


def count_fragments():
    import _render_ref as rr
    res = {}
    for name, (mesh, z, slab) in GEOMETRIES.items():
        c, stats = instances(mesh, z, slab), {}
        d, l = rr.render(meshes(), c["mesh_id"], c["frame_id"], c["label"], c["RT"], c["scale"], K.reshape(-1), F, H, W, stats=stats)
        b = stats["boxes"]
        res[name] = dict(triangles_drawn=int(len(b)), fragments=int(stats["fragments"]), candidate_pixels=int(b.sum()),
                         triangles_queued=int((b > 64).sum()), covered_pixels=int((l > 0).sum()))
        print(name, res[name], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fragments", action="store_true", help="count the fragments on the host instead of timing (no GPU)")
    ap.add_argument("--no-step", action="store_true", help="leave the training step and its loader out")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if args.fragments:
        res = {"fragments": count_fragments()}
    else:
        res = measure(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def measure(args):
    assert torch.cuda.is_available(), "time_render.py measures the HIP path; it needs a GPU"
    from time_pool_sampler import alternate, graph_of
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.render import MeshSet, SyntheticItems, label_boxes, render_frames
    from hs_pose_amd.train import FrameTrainStep, TrainDriver

    dev = torch.device("cuda:0")
    ms = MeshSet(meshes(), device=dev)
    Kd = torch.from_numpy(K).to(dev)
    depth = torch.zeros(F, H, W, dtype=torch.uint16, device=dev)
    labels = torch.zeros(F, H, W, dtype=torch.uint8, device=dev)
    up = lambda a, dt: torch.as_tensor(a, dtype=dt).to(dev)
    forms, keep, covered = {}, [], {}

    def form(c):
        t = {k: up(v, torch.float32 if k in ("RT", "scale") else torch.int32) for k, v in c.items()}
        keep.append(t)
        items = slice(0, None, len(c["label"]) // F) if len(c["label"]) else slice(0, 0)

        def fn():
            render_frames(ms, t["mesh_id"], t["RT"], t["scale"], Kd, H, W, frame_ids=t["frame_id"], labels=t["label"], F=F,
                          out=(depth, labels))
            if len(c["label"]):
                return label_boxes(labels, t["frame_id"][items], t["label"][items])
        return fn

    for name, (mesh, z, slab) in GEOMETRIES.items():
        fn = form(instances(mesh, z, slab))
        boxes, count = fn()
        covered[name] = dict(item_pixels=int(count.sum()), frame_pixels_covered=int((labels > 0).sum()))
        forms["render_" + name] = graph_of(fn)
        if name == "box":                                        # (timed right behind render_box: the frames then hold the boxes)
            t = keep[-1]
            forms["label_boxes_box"] = graph_of(lambda: label_boxes(labels, t["frame_id"], t["label"]))
    empty = {k: v[:0] for k, v in instances(BOX, 0.8, False).items()}
    forms["render_empty"] = graph_of(form(empty))
    res = {"F": F, "H": H, "W": W, "rounds": args.rounds, "steps_per_round": args.steps, "covered": covered}

    if not args.no_step:
        B, N, O = 16, 1028, 256
        FLAGS.reset()
        FLAGS.train = 1
        src = SyntheticItems(ms, [0, 1], [[0.1, 0.2, 0.1], [0.15, 0.15, 0.15]], [[0, 0, 0, 0], [1, 1, 1, 1]], K, H, W, distance=(0.6, 1.5),
                             size=(0.1, 0.3), rng=np.random.default_rng(1))
        frames, items = src.draw(F)
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).train()
        drv = TrainDriver(net, total_iters=10 ** 6, check_nan=False)
        step = FrameTrainStep(net, drv.optimizer, frames, items, B, scheduler=drv.scheduler, sampler=pc_sample.DeviceSampler(1, dev),
                              n_pts=N, out_size=O)
        pinned = dict(depth=frames["depth"].cpu().pin_memory(), labels=frames["labels"].cpu().pin_memory())
        forms["load_pinned"] = lambda: step.load(frames=pinned)
        forms["step"] = lambda: step.run(check=False)
        res.update(B=B, N=N, O=O)
    res["forms"] = alternate(forms, args.rounds, args.steps, args.warmup)
    torch.cuda.synchronize()
    if not args.no_step:
        res["step_last_info"] = step.info.cpu().tolist()
    return res


if __name__ == "__main__":
    main()
