"""Run by test_gpu_bf16_heads.py in a fresh process: one GraphedTrainStep replay of a bf16 network (HSPose with every layer
on bf16 feature rows, ops_bf16) against the same step issued eagerly on a twin -- every loss term, every parameter gradient
and every parameter after the Ranger step must be EQUAL (the bf16 kernels are deterministic, no float atomics on outputs).
``order``: "driver_first" builds the TrainDriver (fused optimizer, re-seats the parameters) and then sets the dtype;
"dtype_first" sets it before (the driver re-applies it after seating).
usage: python tests/_train_graph_bf16_check.py B N order
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch

from hs_pose_amd import augment, gcn3d
from hs_pose_amd.config import FLAGS
from hs_pose_amd.graph import GraphedTrainStep
from hs_pose_amd.HSPose import HSPose
from hs_pose_amd.train import TrainDriver
import ref_cpu as oc

KEYS = ("PC", "obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point",
        "nocs_scale")


def make(dev, order):
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).train()
    for m in net.modules():                      # dropout draws come from the device generator: not comparable
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    if order == "dtype_first":
        net.set_feature_dtype(torch.bfloat16)
        drv = TrainDriver(net, total_iters=1000, check_nan=False)
    else:
        drv = TrainDriver(net, total_iters=1000, check_nan=False)
        net.set_feature_dtype(torch.bfloat16)
    return net, drv


def main():
    B, N, order = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 1
    FLAGS.aug_bb_pro = FLAGS.aug_rt_pro = FLAGS.aug_bc_pro = FLAGS.aug_pc_pro = -1.0   # device-generator draws off
    case = {k: v.to(dev) for k, v in oc.hspose_train_case(B, N, 7).items()}
    batch = {k: case[k] for k in KEYS}

    net_g, drv_g = make(dev, order)
    torch.manual_seed(3)
    graphed = GraphedTrainStep(net_g, drv_g.optimizer, batch, scheduler=drv_g.scheduler, warmup=2)
    graphed.run()
    torch.cuda.synchronize()
    pool = [p.clone() for p in graphed.pool_idx]
    noise = graphed.noise.clone()
    grads_g = {k: p.grad.detach().clone() for k, p in net_g.named_parameters()}
    loss_g = {f"{g}.{k}": float(v) for g, d in graphed.loss_dict.items() for k, v in d.items()}

    net_e, drv_e = make(dev, order)
    with gcn3d.pool_index_feed(pool), augment.jitter_noise_feed(noise):
        _, ld = net_e(do_loss=True, **batch)
    total = sum(sum(d.values()) for d in ld.values())
    drv_e.optimizer.zero_grad()
    total.backward()
    grads_e = {k: p.grad.detach().clone() for k, p in net_e.named_parameters() if p.grad is not None}
    drv_e.optimizer.clip_grad_norm_(5)
    drv_e.optimizer.step()
    torch.cuda.synchronize()

    bad = []
    finite = all(torch.isfinite(v).all().item() for v in grads_e.values())
    for g, d in ld.items():
        for k, v in d.items():
            a, b = float(v), loss_g[f"{g}.{k}"]
            finite = finite and abs(a) < float("inf")
            if a != b:
                bad.append(f"loss {g}.{k}: eager {a!r} graph {b!r}")
    if set(grads_e) != set(grads_g):
        bad.append("gradient sets differ")
    for k, v in grads_e.items():
        if not torch.equal(v, grads_g[k]):
            bad.append(f"grad {k}: |diff| {(v - grads_g[k]).abs().max().item():.3e}")
    pe = dict(net_e.named_parameters())
    for k, p in net_g.named_parameters():
        if not torch.equal(p, pe[k]):
            bad.append(f"param after step {k}: |diff| {(p - pe[k]).abs().max().item():.3e}")
    if not finite:
        bad.append("non-finite loss or gradient")
    print(f"bf16 B={B} N={N} {order}: total loss eager {float(total):.6f} graph {float(graphed.total):.6f}; {len(bad)} mismatches")
    for line in bad[:20]:
        print("  " + line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
