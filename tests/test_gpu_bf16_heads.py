"""GPU: the bf16 mode of the whole network (heads included; hs_pose_amd/ops_bf16.py).

Kernel contracts: the ragged bf16 weight gradient (fp64 reference at fp32-accumulation tolerance 4e-6 (mag + 1), reproducible,
partial + fold equal to the direct form), points_max on bf16 rows (equal to the fp32 kernel on the widened rows), the fp32-residual
bf16 product, and the input gradient of feat's four consumers (the fp64 sum of the four widened products, rounded once).
Network: PoseNet9D forward + backward in training (B=4, N=1028) and in eval configuration against the fp32 path on the same
weights, pool draws and (replayed) feature-space neighbour lists; GraphedInference and GraphedTrainStep on a bf16 network
against their eager twins, bit for bit; 30 training steps fp32 vs bf16 from one init."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
OUT_NAMES = ("recon", "face_normal", "face_dis", "face_f", "p_green_R", "p_red_R", "f_green_R", "f_red_R", "Pred_T", "Pred_s")
# bounds against the fp32 path: outputs (max error / scale, RMS error / RMS); parameter gradients (norm ratio, cosine).
# Eval configuration: 0.15 / 0.1 (measured <= 9.6e-3 / 8.4e-3).  Training, B=4 N=1028 on four distinct object clouds
# (ref_cpu.hspose_train_case), every head layer a batch-statistic BatchNorm on top of the stack's own 4e-2 -- about 2x what this
# test measures:
#   recon .115/.119  face_normal -/.253  face_dis .162/.167  face_f .078/.028  p_green .206/.134  p_red .348/.237
#   f_green .052/.033  f_red .074/.063  Pred_T .072/.097  Pred_s .189/.167
# (face_normal's max is not bounded: normalising a near-zero raw normal turns any error into a direction flip, up to 2)
EVAL_BOUNDS = {k: (0.15, 0.1) for k in OUT_NAMES}
TRAIN_BOUNDS = {"recon": (0.23, 0.24), "face_normal": (2.0, 0.51), "face_dis": (0.32, 0.33), "face_f": (0.16, 0.056),
                "p_green_R": (0.41, 0.27), "p_red_R": (0.70, 0.47), "f_green_R": (0.10, 0.066), "f_red_R": (0.15, 0.13),
                "Pred_T": (0.15, 0.19), "Pred_s": (0.38, 0.33)}
# gradients of the whole network: measured worst |norm ratio - 1| 0.34 and worst cosine 0.48 (rot_red's conv1 / conv2; the
# stack-only figure is 0.91-0.999, bound 0.88): every head layer's train-mode BatchNorm amplifies the bf16 rounding once more.
# Bounds: twice the norm deviation, cosine 0.4.  Parameters whose fp32 gradient is numerically zero (a Conv1d bias ahead of a
# BatchNorm; < 1e-4 of the largest gradient norm) compare noise with noise and are skipped.
GRAD_NORM_TOL, GRAD_COS_TOL = 0.68, 0.4


def _h(ref, shape, seed, scale=1.0):
    return ref.hash_tensor(shape, seed, scale)


def _pitched(rows, k, dev, seed):
    """(rows, k) bf16 on a 16-byte pitch with zeroed pad columns (feat's layout)"""
    p = (k + 7) // 8 * 8
    full = torch.zeros(rows, p, dtype=BF, device=dev)
    g = torch.Generator(device="cpu").manual_seed(seed)
    full[:, :k] = torch.randn(rows, k, generator=g).to(dev, BF)
    return full[:, :k]


@pytest.mark.parametrize("K,M,N", [(4112, 1286, 1024), (16448, 1286, 512), (4112, 1286, 256)])
def test_wgrad_ragged_bf16(dev, K, M, N):
    from hs_pose_amd import ops
    A = _pitched(K, M, dev, 1)
    Bm = torch.randn(K, N, generator=torch.Generator().manual_seed(2)).to(dev, BF)
    gw, cs = ops.wgrad(A, Bm, colsum=True)
    A64, B64 = A.double(), Bm.double()
    want, mag = A64.t() @ B64, A64.abs().t() @ B64.abs()
    assert ((gw.double() - want).abs() <= 4e-6 * (mag + 1)).all()
    assert ((cs.double() - B64.sum(0)).abs() <= 4e-6 * (B64.abs().sum(0) + 1)).all()
    again = ops.wgrad(A, Bm, colsum=True)
    assert torch.equal(gw, again[0]) and torch.equal(cs, again[1])
    with ops.WgradBatch():                                        # the partial form + the (batched) fold
        late = ops.wgrad(A, Bm, colsum=True)
    torch.cuda.synchronize()
    assert torch.equal(gw, late[0]) and torch.equal(cs, late[1])


def test_points_max_bf16_equals_fp32_kernel(dev):
    from hs_pose_amd import ops
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(-20, 20, (3, 1028, 256), generator=g).float() / 4).to(dev, BF)   # many ties: the first-winner rule
    x.requires_grad_(True)
    xf = x.detach().float().requires_grad_(True)
    v, vf = ops.points_max(x), ops.points_max(xf)
    assert v.dtype == torch.float32 and torch.equal(v, vf)
    gout = torch.randn(3, 256, generator=g).to(dev)
    v.backward(gout)
    vf.backward(gout)
    assert x.grad.dtype == BF and torch.equal(x.grad, xf.grad.bfloat16())


def test_gemm_rows_acc_bf16(dev):
    from hs_pose_amd import ops_bf16
    g = torch.Generator().manual_seed(4)
    M, N, K1, K2 = 4112, 1286, 1024, 512
    A1, A2 = (torch.randn(M, k, generator=g).to(dev, BF) for k in (K1, K2))
    B1, B2 = (torch.randn(N, k, generator=g).to(dev, BF) for k in (K1, K2))
    r = torch.randn(M, N, generator=g).to(dev) * 10
    want = A1.double() @ B1.double().t() + A2.double() @ B2.double().t() + r.double()
    mag = A1.double().abs() @ B1.double().abs().t() + A2.double().abs() @ B2.double().abs().t() + r.double().abs()
    out = ops_bf16.gemm_rows_acc(A1, B1, A2, B2, r, torch.empty(M, N, device=dev))
    assert ((out.double() - want).abs() <= 4e-6 * (mag + 1)).all()
    ob = ops_bf16.gemm_rows_acc(A1, B1, A2, B2, r, torch.empty(M, N, dtype=BF, device=dev))
    # rounded once: within half a bf16 ulp of the fp32 result (ties aside)
    assert torch.equal(ob, out.bfloat16())


@pytest.mark.parametrize("M,K,N,extra", [(16448, 1286, 1024, ""), (16448, 1286, 512, ""), (16448, 1286, 1024, "xyz"),
                                         (16448, 512, 512, ""), (16448, 512, 256, ""), (16448, 256, 128, ""),
                                         (16448, 1024, 256, ""), (16448, 256, 512, "cloud+xyz"), (4100, 1286, 1024, "")])
def test_gemm_rows_bn_bf16(dev, M, K, N, extra):
    """the bf16 product with the BatchNorm first pass in its epilogue: C against fp64, bn_part against fp64 sums of the returned C,
    and the mixed fold (bn_relu partials) against hsp_bn_relu_fwd_mixed on the same C"""
    import ctypes
    from hs_pose_amd import ops, ops_bf16
    from hs_pose_amd._lib import lib
    g = torch.Generator().manual_seed(M + K + N)
    A = _pitched(M, K, dev, 7)
    W = (torch.randn(N, (K + 7) // 8 * 8, generator=g) / K ** 0.5).to(dev, BF)[:, :K]
    bias = (torch.randn(N, generator=g) + 3).to(dev)
    cb = xyz3 = w3 = None
    rpc = 0
    if "cloud" in extra:
        rpc = 1028
        cb = torch.randn((M + rpc - 1) // rpc, N, generator=g).to(dev)
    if "xyz" in extra:
        xyz3, w3 = torch.randn(M, 3, generator=g).to(dev), torch.randn(N, 3, generator=g).to(dev)
    L = lib()
    tiles = L.hsp_gemm_rows_bn_tiles_bf16(M, N, K)
    assert 0 < tiles <= 512
    C = torch.empty(M, N, device=dev)
    buf = torch.full((1 + 2 * tiles, N), float("nan"), device=dev)
    p = ops._p
    rc = L.hsp_gemm_rows_bn_bf16(p(A), A.stride(0), p(W), W.stride(0), K, M, N, p(bias), p(cb), rpc, p(xyz3), p(w3), p(C), N,
                                 p(buf[0]), p(buf[1:]), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    c64 = A.double() @ W.double().t() + bias.double()
    mag = A.double().abs() @ W.double().abs().t() + bias.double().abs()
    shift = bias.double().clone()
    if cb is not None:
        idx = torch.arange(M, device=dev) // rpc
        c64 = c64 + cb.double()[idx]
        mag = mag + cb.double().abs()[idx]
        shift = shift + cb.double()[0]
    if xyz3 is not None:
        c64 = c64 + xyz3.double() @ w3.double().t()
        mag = mag + xyz3.double().abs() @ w3.double().abs().t()
    assert ((C.double() - c64).abs() <= 4e-6 * (mag + 1)).all()
    assert torch.equal(buf[0], shift.float())
    bm = (M + tiles - 1) // tiles
    bm = 64 if bm <= 64 else 128
    d = C.double() - buf[0].double()
    for t in range(tiles):
        blk = d[t * bm:(t + 1) * bm]
        s1, s2 = blk.sum(0), (blk * blk).sum(0)
        assert ((buf[1 + 2 * t] - s1).abs() <= 1e-5 * (blk.abs().sum(0) + 1)).all(), t
        assert ((buf[2 + 2 * t] - s2).abs() <= 1e-5 * (s2 + 1)).all(), t
    # fold + apply (bf16 rows) against the two-pass mixed BatchNorm on the same C
    bn1, bn2 = _bn(N, dev, 1), _bn(N, dev, 1)
    y1 = torch.empty(M, N, dtype=BF, device=dev)
    m1, i1 = torch.empty(N, device=dev), torch.empty(N, device=dev)
    rc = L.hsp_bn_relu_fwd_partials_mixed(p(C), M, N, p(bn1.weight), p(bn1.bias), ctypes.c_float(bn1.eps), ctypes.c_float(0.1), 1,
                                          p(y1), p(m1), p(i1), p(bn1.running_mean), p(bn1.running_var),
                                          p(bn1.num_batches_tracked), p(buf[1:]), tiles, p(buf[0]), ops._stream())
    assert rc == 0
    y2, m2, i2 = ops_bf16._bn_fwd(C, bn2)
    torch.cuda.synchronize()
    ulp = (y2.float().abs() * 2.0 ** -7).clamp_min(2.0 ** -17)        # (outputs within 1e-3 of zero: that ulp, absolute)
    assert ((y1.float() - y2.float()).abs() <= ulp).all()
    for a_, b_ in ((bn1.running_mean, bn2.running_mean), (bn1.running_var, bn2.running_var), (m1, m2), (i1, i2)):
        rel = ((a_ - b_).abs() / b_.abs().clamp_min(1e-6 * b_.abs().max().item())).max().item()
        print(f"partials fold vs two-pass: max relative difference {rel:.2e}")
        assert rel <= 1e-5                # (single-pass shifted sums folded over <= 257 tiles against the two-pass statistics)
    assert int(bn1.num_batches_tracked) == int(bn2.num_batches_tracked) == 1


def _bn(c, dev, seed):
    bn = torch.nn.BatchNorm1d(c).to(dev).train()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * torch.randn(c, generator=g))
        bn.bias.copy_(0.1 * torch.randn(c, generator=g))
    return bn


def test_fan_input_gradient_rounded_once(dev, monkeypatch):
    """the gradient reaching feat = the fp64 sum of the four widened products g_i W_i, rounded to bf16 once"""
    from hs_pose_amd import ops_bf16
    B, N, K = 4, 1028, 1286
    R = B * N
    g = torch.Generator().manual_seed(5)
    x = _pitched(R, K, dev, 6).requires_grad_(True)
    xyz = torch.randn(B, N, 3, generator=g).to(dev) * 0.1
    shapes = [(1024, K), (1024, K), (1024, K + 3), (512, K)]
    ws = [(torch.randn(o, i, generator=g) / i ** 0.5).to(dev).requires_grad_(True) for o, i in shapes]
    bs = [(0.1 * torch.randn(o, generator=g)).to(dev).requires_grad_(True) for o, _ in shapes]
    bns = [_bn(o, dev, 10 + j) for j, (o, _) in enumerate(shapes)]
    prm = ops_bf16.Bf16Params([(w.detach()[:, :K], True, True, True) for w in ws])
    prm.refresh()
    gs = []
    real = ops_bf16._bn_bwd

    def rec(*a):
        out = real(*a)
        gs.append(out[0])
        return out
    monkeypatch.setattr(ops_bf16, "_bn_bwd", rec)
    outs = ops_bf16.fan_bn(x, xyz, list(zip(ws, bs, bns)))
    das = [torch.randn(o.shape, generator=g).to(dev, BF) for o in outs]
    torch.autograd.backward(outs, das)
    want = sum(gi.double() @ w.detach()[:, :K].bfloat16().double() for gi, w in zip(gs, ws))
    mag = sum(gi.double().abs() @ w.detach()[:, :K].bfloat16().double().abs() for gi, w in zip(gs, ws))
    got = x.grad.double()
    assert x.grad.dtype == BF
    assert ((got - want).abs() <= want.abs() * 2.0 ** -8 + 4e-6 * (mag + 1)).all()        # half a bf16 ulp: 2^-8 relative
    # the translation head's coordinate block: g^T xyz, from the per-cloud moments (no product)
    gxyz = gs[2].double().t() @ xyz.reshape(R, 3).double()
    assert torch.allclose(ws[2].grad[:, K:].double(), gxyz, rtol=1e-5, atol=1e-5 * gxyz.abs().max().item())


class _Replay:
    """record the fp32 path's feature-space neighbour lists, replay them in the bf16 path (the idea of tests/test_gpu_bf16.py)"""

    def __init__(self, monkeypatch):
        from hs_pose_amd import ops
        self.real, self.lists, self.mode, self.pos = ops.knn, [], "record", 0
        monkeypatch.setattr(ops, "knn", self)

    def __call__(self, x, k, drop_first=True, **kw):
        own = self.real(x, k, drop_first, **kw)
        if x.shape[-1] == 3:
            return own
        if self.mode == "record":
            self.lists.append(own)
            return own
        want = self.lists[self.pos]
        self.pos += 1
        return want


def _twins(dev, train):
    from hs_pose_amd.PoseNet9D import PoseNet9D
    nets = []
    for dt in (torch.float32, BF):
        torch.manual_seed(0)
        net = PoseNet9D().to(dev)
        net = net.train() if train else net.eval()
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        nets.append(net.set_feature_dtype(dt))
    return nets


def _compare_outputs(of, ob, names, bounds):
    worst = {}
    for name, a, b in zip(OUT_NAMES, of, ob):
        if name not in names:
            continue
        assert b.dtype == torch.float32 and torch.isfinite(b).all(), name
        err = (b - a).double()
        scale, rms = a.abs().max().item(), a.double().pow(2).mean().sqrt().item()
        worst[name] = (err.abs().max().item() / scale, err.pow(2).mean().sqrt().item() / rms)
    print("outputs (max / scale, rms / rms):", {k: (round(v[0], 4), round(v[1], 4)) for k, v in worst.items()})
    return [(name, emax, erms) for name, (emax, erms) in worst.items()
            if emax > bounds[name][0] or erms > bounds[name][1]]


def test_posenet_bf16_training_vs_fp32(dev, ref, flags, monkeypatch):
    flags.train = 1
    B, N = 4, 1028                    # (B=2: the towers' bn3 over two per-cloud rows outputs +-1 whatever its input -- its
    net_f, net_b = _twins(dev, True)  # exact gradient is zero, and both paths' head gradients are rounding noise)
    case = ref.hspose_train_case(B, N, 11)      # four distinct object clouds (not statistically identical hash points)
    pts, obj = case["PC"].to(dev), case["obj_id"].reshape(B, 1).float().to(dev)
    rp = _Replay(monkeypatch)
    torch.manual_seed(5)
    of = net_f(pts, obj)
    rp.mode = "replay"
    torch.manual_seed(5)
    ob = net_b(pts, obj)
    out_bad = _compare_outputs(of, ob, OUT_NAMES, TRAIN_BOUNDS)
    g = torch.Generator().manual_seed(9)
    probes = [torch.randn(t.shape, generator=g).to(dev) for t in of]
    sum((t * p).sum() for t, p in zip(of, probes)).backward()
    sum((t * p).sum() for t, p in zip(ob, probes)).backward()
    pb = dict(net_b.named_parameters())
    worst_n, worst_c, grad_bad = 0.0, 1.0, []
    gmax = max(p.grad.norm().item() for p in net_f.parameters() if p.grad is not None)
    for k, p in net_f.named_parameters():
        gf, gb = p.grad, pb[k].grad
        assert gb is not None and torch.isfinite(gb).all(), k
        if gf.norm().item() < 1e-4 * gmax:
            continue
        nr = (gb.norm() / gf.norm()).item()
        cos = torch.nn.functional.cosine_similarity(gb.flatten().double(), gf.flatten().double(), dim=0).item()
        worst_n, worst_c = max(worst_n, abs(nr - 1)), min(worst_c, cos)
        if abs(nr - 1) > GRAD_NORM_TOL or cos < GRAD_COS_TOL:
            grad_bad.append((k, round(nr, 4), round(cos, 4)))
    print(f"gradients: worst |norm ratio - 1| {worst_n:.4f}, worst cosine {worst_c:.4f}; outside the bounds: {grad_bad}")
    assert not out_bad, out_bad
    assert not grad_bad, grad_bad


def test_posenet_bf16_eval_and_graphed_inference(dev, ref, flags, monkeypatch):
    from hs_pose_amd import gcn3d
    from hs_pose_amd.graph import GraphedInference
    from hs_pose_amd.HSPose import HSPose
    flags.train = 0
    B, N = 2, 1028
    net_f, net_b = _twins(dev, False)
    pts = _h(ref, (B, N, 3), 72, 0.05).to(dev)
    obj = torch.tensor([[1.0], [4.0]]).to(dev)
    rp = _Replay(monkeypatch)
    with torch.no_grad():
        torch.manual_seed(6)
        of = net_f(pts, obj)
        rp.mode = "replay"
        torch.manual_seed(6)
        ob = net_b(pts, obj)
    bad = _compare_outputs(of, ob, OUT_NAMES[4:], EVAL_BOUNDS)
    assert not bad, bad
    monkeypatch.undo()
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).eval().set_feature_dtype(BF)
    ms = torch.full((B, 3), 0.1, device=dev)
    sym = torch.zeros(B, 4, device=dev)
    gi = GraphedInference(net, pts.clone(), obj.clone(), ms, sym)
    rt, s, out = gi.run()
    rt, s = rt.clone(), s.clone()
    outs = {k: out[k].clone() for k in OUT_NAMES[4:]}
    with torch.no_grad(), gcn3d.pool_index_feed(gi.pool_idx):
        eager = net(PC=pts, obj_id=obj, mean_shape=ms, sym=sym)
    for k in OUT_NAMES[4:]:
        assert torch.equal(outs[k], eager[k]), k
    assert torch.equal(s, eager["Pred_s"] + ms)


@pytest.mark.parametrize("B,N,order", [(4, 256, "driver_first"), (4, 256, "dtype_first"), (16, 1028, "driver_first")])
def test_graphed_train_step_bf16_matches_eager(B, N, order):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_train_graph_bf16_check.py"), str(B), str(N), order],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


class _ConstLr:
    def step(self):
        pass

    def state_dict(self):
        return {}


def _train(dev, ref, dt, steps, case):
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.train import TrainDriver
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.set_feature_dtype(dt)
    drv = TrainDriver(net, scheduler=_ConstLr(), check_nan=False)
    curve = []
    torch.manual_seed(1)
    for _ in range(steps):
        _, ld = net(do_loss=True, **case)
        total = HSPose.total_loss(ld)
        curve.append(float(total))
        drv.step(total)
    return curve


def test_bf16_training_tracks_fp32(dev, ref, flags):
    """30 steps on ref_cpu.hspose_train_case from one init at a constant lr (FLAGS.lr * lr_pose), fp32 then bf16: the bf16
    total loss falls and ends within 15 % of the fp32 run's.  Measured (the per-step loss varies with the pool draws):
    fp32 [66.429, 48.0185, 65.0302, 51.7197, 55.0346, 62.2521, 60.6701, 49.1377, 65.8121, 59.4588, 57.794, 60.3376, 55.0017, 65.9162, 55.7416, 53.6562, 41.008, 56.3074, 62.5473, 66.1127, 50.6923, 43.9587, 44.9559, 38.7558, 67.6362, 49.6731, 60.6864, 45.8095, 67.8576, 51.3024]
    bf16 [63.426, 49.0972, 63.3919, 49.6543, 52.0289, 61.3064, 65.3591, 48.6983, 64.2765, 61.3664, 54.8776, 60.517, 52.1527, 68.6546, 55.1539, 52.9586, 43.4722, 55.449, 60.3075, 63.6075, 50.583, 45.6688, 46.828, 39.8809, 70.0686, 53.8352, 57.1216, 42.2947, 68.4071, 52.0015]
    last five steps: fp32 275.3, bf16 273.7 (sum); first five: bf16 277.6."""
    flags.train = 1
    flags.aug_bb_pro = flags.aug_rt_pro = flags.aug_bc_pro = flags.aug_pc_pro = -1.0
    keys = ("PC", "obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point",
            "nocs_scale")
    case = {k: v.to(dev) for k, v in ref.hspose_train_case(4, 1028, 11).items() if k in keys}
    f32 = _train(dev, ref, torch.float32, 30, case)
    b16 = _train(dev, ref, BF, 30, case)
    print("fp32:", [round(v, 4) for v in f32])
    print("bf16:", [round(v, 4) for v in b16])
    assert all(v == v for v in b16)
    assert sum(b16[-5:]) < sum(b16[:5])
    assert abs(sum(b16[-5:]) - sum(f32[-5:])) <= 0.15 * sum(f32[-5:])
