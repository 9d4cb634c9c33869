"""The rendered training step (hs_pose_amd/train.py: RenderedTrainStep over render.SceneSource) beside what it is made of and
what it replaces, timed in ONE process at the batch of tools/time_render.py's step -- F = M = 24 frames of 480 x 640 uint16, 16
kept, N = 1028, O = 256, ``SyntheticItems``' default distances and sizes, four procedural meshes and one slab under every item:

  rendered_step   ``RenderedTrainStep.run(check=False)``: the scene drawn, sampled, rendered and boxed inside the replay
  rendered_fixed  a second ``RenderedTrainStep`` whose key stays at {1, 0}: replay and optimizer launch without ``advance()``, so
                  every replay draws the one scene frame_step holds -- rendered_step minus this is what the scenes' variety costs
  frame_step      ``FrameTrainStep(draws='device').run(check=False)`` on the frames one eager ``SceneSource.draw`` made under {1, 0}
  render          one hipGraph replay of ``render_frames`` + ``label_boxes`` on that draw's 48 instance rows
  scene_kernels   one hipGraph replay of ``ops.scene_draw`` + ``ops.mesh_sample`` alone (the two new launches)
  host_path       ``SyntheticItems.draw(24)`` + ``FrameTrainStep.load`` + ``run(check=False)``: the host draw end to end; its
                  wall clock is the figure (the device figure leaves out the time the device waits for the host)

Device criterion: rendered_step - (frame_step + render) within the min - max spread of rendered_step.  Host criterion:
rendered_step's wall clock per step below host_path's.  The protocol is tools/time_render.py's: all forms built first, then
timed ALTERNATELY in rounds, a window of ``--steps`` calls between device events after a synchronise with the wall clock
alongside, median and min - max over the rounds.  Run on the GPU box:  python tools/time_rendered_step.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

from time_render import F, H, K, W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_rendered_step.py measures the HIP path; it needs a GPU"
    from time_pool_sampler import alternate, graph_of
    from hs_pose_amd import ops, pc_sample
    from hs_pose_amd.config import FLAGS
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.render import MeshSet, SceneSource, SyntheticItems, label_boxes, render_frames, shapes
    from hs_pose_amd.train import FrameTrainStep, RenderedTrainStep, TrainDriver

    dev = torch.device("cuda:0")
    B, N, O = 16, 1028, 256
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.step_draws = "device"
    ms = MeshSet([shapes.box(), shapes.cylinder(24), shapes.uv_sphere(48, 32), shapes.mug(16)], device=dev)
    tables = dict(class_ids=[0, 1, 2, 5], mean_shapes=[[0.1, 0.2, 0.1], [0.1, 0.15, 0.1], [0.15, 0.15, 0.15], [0.12, 0.1, 0.1]],
                  sym_infos=[[0, 0, 0, 0], [1, 1, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0]])
    slab = [dict(mesh=0, size=(1.2, 0.02, 1.2), rest=True)]
    source = lambda: SceneSource(ms, K=K, H=H, W=W, distractors=slab, **tables)

    def network():
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).train()
        return net, TrainDriver(net, total_iters=10 ** 6, check_nan=False)

    net_a, drv_a = network()
    rendered = RenderedTrainStep(net_a, drv_a.optimizer, source(), F, B, scheduler=drv_a.scheduler,
                                 sampler=pc_sample.DeviceSampler(1, dev), n_pts=N, out_size=O)
    net_c, drv_c = network()
    fixed = RenderedTrainStep(net_c, drv_c.optimizer, source(), F, B, scheduler=drv_c.scheduler,
                              sampler=pc_sample.DeviceSampler(1, dev), n_pts=N, out_size=O)
    fixed.sampler.advance()                                     # the key now holds {1, 0}, and stays
    eager = source()
    key = torch.tensor([1, 0], dtype=torch.int64, device=dev)
    frames, items = eager.draw(F, key)
    o = eager.last
    host = lambda fr: dict(fr, bboxes_xyxy=fr["bboxes_d"].cpu().numpy())
    net_b, drv_b = network()
    frame = FrameTrainStep(net_b, drv_b.optimizer, host(frames), items, B, scheduler=drv_b.scheduler,
                           sampler=pc_sample.DeviceSampler(1, dev), n_pts=N, out_size=O, draws="device")
    synth = SyntheticItems(ms, K=K, H=H, W=W, distractors=slab, rng=np.random.default_rng(1), **tables)
    depth, labels = torch.zeros_like(frames["depth"]), torch.zeros_like(frames["labels"])

    def render():
        render_frames(ms, o["mesh_id"], o["RT"], o["scale"], eager.K, H, W, frame_ids=o["frame_id"], labels=o["label"], F=F,
                      out=(depth, labels))
        return label_boxes(labels, o["frame_id"][:F], o["label"][:F])

    bufs = eager.buffers(F)

    def scene_kernels():
        s = ops.scene_draw(key, eager.ext, eager.cls, eager.mean_shapes, eager.sym_infos, eager.params, eager.distractors, F, out=bufs)
        return ops.mesh_sample(ms.verts, ms.tris, ms.table, eager.cum, eager.ext, s["mesh_id"][:F], s["scale"][:F], key, eager.n_model,
                               out=bufs["model_point"])

    def host_path():
        fr, it = synth.draw(F)
        boxes = fr["bboxes_xyxy"]                               # the host form of the guard: a hidden item's box made harmless
        boxes[(boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])] = (0, 0, 1, 1)
        frame.load(frames=fr, items=it)
        return frame.run(check=False)

    forms = {"rendered_step": lambda: rendered.run(check=False),
             "rendered_fixed": lambda: (fixed.graphed.replay(), fixed.graphed.apply()), "frame_step": lambda: frame.run(check=False),
             "render": graph_of(render), "scene_kernels": graph_of(scene_kernels), "host_path": host_path}
    res = {"F": F, "H": H, "W": W, "B": B, "N": N, "O": O, "rounds": args.rounds, "steps_per_round": args.steps,
           "forms": alternate(forms, args.rounds, args.steps, args.warmup)}
    torch.cuda.synchronize()
    f = res["forms"]
    r = f["rendered_step"]
    res["device_excess_ms"] = round(r["device_ms"] - f["frame_step"]["device_ms"] - f["render"]["device_ms"], 4)
    res["device_excess_fixed_ms"] = round(f["rendered_fixed"]["device_ms"] - f["frame_step"]["device_ms"] - f["render"]["device_ms"], 4)
    res["device_spread_ms"] = round(r["device_ms_max"] - r["device_ms_min"], 4)
    res["host_ratio"] = round(f["host_path"]["wall_ms"] / r["wall_ms"], 3)
    res["last_info"] = {"rendered_step": rendered.info.cpu().tolist(), "frame_step": frame.info.cpu().tolist()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
