"""How far the columns of the network's BatchNorm inputs sit from the shift of their shifted sums; run on the GPU box.

One eager training step of the benchmark's own configuration (bench.py: FaceRecon under torch.manual_seed(0), default
initialisation, B = 16 clouds of N = 1028 points from make_inputs(seed 0), Pool_layer draws under torch.manual_seed(1), fp32
rows).  For every train-mode BatchNorm call, one line: its shape, the path its first pass takes and

    rho = max over columns of |mean - shift| / sigma        (fp64 statistics of the call's input)

for the shift that path uses -- row 0 of the partial buffer for a first pass left by the producing product's epilogue (one shift
per column: residual row 0 + per-cloud bias row 0, or the Linear's bias), each row chunk's own first row for the three-launch
form (the maximum over the chunks is printed: chunk mean against chunk shift, in chunk deviations) -- and the largest error of
the call's fp32 output against y = relu((x - mean) / sqrt(var + eps) * gamma + beta) in fp64, as a fraction of max(1, |y|max):
the figure the 2e-5 tolerance of the BatchNorm tests is about.  DESIGN.md section 2 sets these figures against the rho at which
each path leaves that tolerance.  --heads adds FaceRecon's train-only heads.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from hs_pose_amd import ops
from hs_pose_amd._lib import lib
from hs_pose_amd.config import FLAGS
from hs_pose_amd.FaceRecon import FaceRecon


def _rho(x64, shift64):
    mean = x64.mean(0)
    sigma = ((x64 - mean) ** 2).mean(0).sqrt()
    r = (mean - shift64).abs() / sigma.clamp_min(1e-300)
    return r[sigma > 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--heads", action="store_true", help="FLAGS.train = 1: the recon / face heads of FaceRecon run too")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    FLAGS.reset()
    FLAGS.train = 1 if args.heads else 0
    torch.manual_seed(0)
    net = FaceRecon().to(dev).train()
    centred, obj, dfeat = bench.make_inputs(args.batch, args.points, dev, seed=0)
    torch.manual_seed(1)
    real = ops.bn_relu
    calls = []

    def recording_bn_relu(x, bn, relu=True, out_dtype=None, fork=False, partial=None):
        C = x.shape[-1]
        if bn.training:
            x64 = x.detach().reshape(-1, C).double()
            R = x64.shape[0]
            if partial is not None and partial.numel():
                path, rho = "epilogue", _rho(x64, partial[0].double())
            else:
                rpb = max(32, (R + 511) // 512)                 # norm.hip: at most 512 chunks of at least 32 rows
                assert lib().hsp_bn_workspace_bytes(R, C) == (R + rpb - 1) // rpb * 8 * C
                path = "three-launch"
                rho = torch.cat([_rho(x64[r0:r0 + rpb], x64[r0]) for r0 in range(0, R, rpb) if min(R, r0 + rpb) - r0 > 1] or
                                [torch.zeros(1, dtype=torch.float64, device=x.device)])
            mean = x64.mean(0)
            want = (x64 - mean) / (((x64 - mean) ** 2).mean(0) + bn.eps).sqrt() * bn.weight.detach().double() + bn.bias.detach().double()
            want = want.clamp_min(0.0) if relu else want
        out = real(x, bn, relu=relu, out_dtype=out_dtype, fork=fork, partial=partial)
        if bn.training:
            y = (out[0] if isinstance(out, tuple) else out).detach().reshape(-1, C)
            err = ((y.double() - want).abs().max() / want.abs().max().clamp_min(1.0)).item() if y.dtype == torch.float32 else float("nan")
            calls.append((R, C, path, rho.max().item(), rho.median().item(), err))
        return out

    ops.bn_relu = recording_bn_relu
    try:
        recon, face, feat = net(centred, obj)
        loss = (feat * dfeat).sum()
        if recon is not None:
            loss = loss + recon.sum() + face.sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.bn_relu = real
        FLAGS.reset()
    for i, (R, C, path, worst, median, err) in enumerate(calls):
        print(f"bn call {i}: R {R} C {C} {path}: rho max {worst:.2f} (median over columns and chunks {median:.2f}), "
              f"y error {err:.1e} of scale")


if __name__ == "__main__":
    main()
