"""GPU: the Chamfer reconstruction term 'Prop_sym_cd' (include/hsp.h: hsp_recon_chamfer_fwd / _bwd, hsp_chamfer_bwd_ordered;
ops.recon_chamfer, ops.chamfer under FLAGS.reproducible; fused_losses.pose_losses) against the fp64
restatement of tests/_recon_chamfer_ref.py and the C oracle, and whole steps in a child process
(tests/_recon_chamfer_step_check.py).  Every bound is stated where it is used; u = 2^-24."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _recon_chamfer_ref as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
W = 0.75                      # the term's weight in the kernel-level cases
GSCALE = 0.5                  # the gradient arriving at the term

# (B, N, the clouds' symmetry rows in turn, the tiled cloud): one point; an odd size below a workgroup; exactly one 64-query
# workgroup per direction; one past a whole number of 64-query (and 4-row backward) workgroups; the step's size; one past a
# 2048-point LDS chunk; skip clouds only; the four classes, one tiled
CASES = {"1x1": (1, 1, (rc.SYM_YX,), None), "2x7": (2, 7, (rc.SYM_Y, rc.SYM_NONE), None),
         "3x64": (3, 64, (rc.SYM_Y, rc.SYM_YX, rc.SYM_NONE), None), "2x257": (2, 257, (rc.SYM_YX, rc.SYM_Y), None),
         "1x1028": (1, 1028, (rc.SYM_Y,), None), "1x2049": (1, 2049, (rc.SYM_YX,), None),
         "skip_only": (2, 64, (rc.SYM_SKIP,), None), "mixed": (4, 100, rc.ALL_CLASSES, 1)}


def _np(t):
    return t.detach().cpu().numpy()


def _forward(batch, dev, w=W):
    """hsp_recon_chamfer_fwd on buffers of its own -> dict of device tensors (term, G, idx1, idx2, d (2,B,N))"""
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    B, N, _ = batch["PC"].shape
    t = {k: v.to(dev) for k, v in batch.items()}
    out = dict(term=torch.full((1,), float("nan"), device=dev), G=torch.full((B, N, 3), float("nan"), device=dev),
               idx1=torch.full((B, N), -1, dtype=torch.int32, device=dev), idx2=torch.full((B, N), -1, dtype=torch.int32, device=dev))
    wsb = lib().hsp_recon_chamfer_fwd_workspace_bytes(B, N)
    assert wsb == 8 * B * N
    d = torch.full((2, B, N), float("nan"), device=dev)
    ops._run("hsp_recon_chamfer_fwd", (ops._p(t["PC"]), ops._p(t["gt_R"]), ops._p(t["gt_t"]), ops._p(t["sym"]), ops._p(t["recon"]), B, N,
                                       w, ops._p(out["term"]), ops._p(out["G"]), ops._p(out["idx1"]), ops._p(out["idx2"]), ops._p(d),
                                       wsb, ops._stream()))
    out.update(d=d, dev=t)
    return out


def _backward(fw, w=W, g=GSCALE):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    t = fw["dev"]
    B, N, _ = t["recon"].shape
    gx = torch.full((B, N, 3), float("nan"), device=t["recon"].device)
    gt = torch.tensor([g], device=gx.device)
    wsb = lib().hsp_recon_chamfer_bwd_workspace_bytes(B, N)
    ws = torch.empty(wsb, dtype=torch.uint8, device=gx.device)
    ops._run("hsp_recon_chamfer_bwd", (ops._p(t["recon"]), ops._p(fw["G"]), ops._p(fw["idx1"]), ops._p(fw["idx2"]), ops._p(t["sym"]),
                                       ops._p(gt), B, N, w, ops._p(gx), ops._p(ws), wsb, ops._stream()))
    return gx


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case's batch, the kernels' outputs (numpy) and the fp64 target: computed once, shared by the tests, never written to"""
    import ref_cpu as ref
    B, N, syms, tiled = CASES[name]
    batch = rc.batch(ref, B, N, syms, seed=11 + len(name), tiled=tiled)
    dev = torch.device("cuda:0")
    fw = _forward(batch, dev)
    gx = _backward(fw)
    torch.cuda.synchronize()
    got = {k: _np(fw[k]) for k in ("term", "G", "idx1", "idx2", "d")}
    got["gx"] = _np(gx)
    for v in got.values():
        v.setflags(write=False)
    return batch, got, fw


@pytest.mark.parametrize("name", list(CASES))
def test_target_against_fp64(dev, name):
    """G per component within 2^-23 (4 sum_k |p_k - t_k| + |G64|): twice the worst-case count of roundings of two 3-term
    products, a subtraction and an add; a copied cloud (no symmetry) and a skip cloud's zeros exactly"""
    batch, got, _ = _case(name)
    G64, mag = rc.target64(batch["PC"], batch["gt_R"], batch["gt_t"], batch["sym"])
    err = np.abs(got["G"].astype(np.float64) - G64)
    bound = 2.0 ** -23 * (4 * mag[..., None] + np.abs(G64))
    print(f"{name}: worst |G - G64| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    _, _, cls_none, skip = rc.classes(batch["sym"])
    assert np.array_equal(got["G"][cls_none], batch["PC"].numpy()[cls_none]) and np.all(got["G"][skip] == 0)


@pytest.mark.parametrize("name", list(CASES))
def test_distances_and_argmins(dev, oc, name):
    """on the kernel's own (P, G): distances and arg-mins bit-equal to the C oracle's (the same expression, first minimum, the
    tiled cloud's exact ties included); arg-mins equal to an fp64 brute-force first-minimum search wherever the fp64 gap between
    best and runner-up exceeds 2^-18 of the runner-up (64 x the fp32 error of the expression) -- an exact tie is not excused --,
    at most 0.5 % of the points excused; a skip cloud: zeros"""
    batch, got, _ = _case(name)
    skip = rc.classes(batch["sym"])[3]
    P, G = batch["recon"].numpy(), got["G"]
    d1, d2, i1, i2 = oc.chamfer_fwd(P, G)
    keep = ~skip
    for mine, want in ((got["d"][0], d1), (got["d"][1], d2)):
        assert np.array_equal(mine[keep].view(np.int32), want[keep].view(np.int32))
        assert np.all(mine[skip].view(np.int32) == 0)
    for mine, want in ((got["idx1"], i1), (got["idx2"], i2)):
        assert np.array_equal(mine[keep], want[keep]) and np.all(mine[skip] == 0)
    excused = total = 0
    for b in np.nonzero(keep)[0]:
        for q, c, mine in ((P[b], G[b], got["idx1"][b]), (G[b], P[b], got["idx2"][b])):
            best, i, runner, _ = rc.search64(q, c)
            loose = rc.near_tie(best, runner)
            assert np.array_equal(mine[~loose], i[~loose])
            excused += int(loose.sum()); total += len(loose)
    print(f"{name}: {excused} of {total} arg-mins excused")
    assert excused <= 0.005 * total


@pytest.mark.parametrize("name", list(CASES))
def test_term_and_gradient(dev, name):
    """the term against the fp64 sum of the kernel's distances within (B N) u of the sum of magnitudes (its own count of
    roundings per element is ceil(2 B N / 1024) + 12); a gradient component against the fp64 restatement on the kernel's lists
    within (c_i + 4) u |s| sum |terms|, c_i the row's in-degree: one rounding per difference, c_i adds, two in s, one product;
    a skip cloud's rows, and a skip-only batch's term, exactly 0"""
    batch, got, _ = _case(name)
    B, N, _, _ = CASES[name]
    skip = rc.classes(batch["sym"])[3]
    S = got["d"].astype(np.float64).sum()
    want = W * S / (B * N)
    print(f"{name}: term {float(got['term'][0])!r}, fp64 {want!r}")
    assert abs(float(got["term"][0]) - want) <= (B * N) * U * want
    s = 2.0 * GSCALE * W / (B * N)
    worst = 0.0
    for b in range(B):
        if skip[b]:
            assert np.all(got["gx"][b].view(np.int32) == 0)
            continue
        g64, mag, deg = rc.grad64(batch["recon"][b].numpy(), got["G"][b], got["idx1"][b], got["idx2"][b], s)
        err, bound = np.abs(got["gx"][b] - g64), (deg[:, None] + 4) * U * s * mag
        assert np.all(err <= bound), (b, float(np.max(err - bound)))
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert name != "mixed" or b != 1 or deg.max() >= 2                 # the tiled cloud: duplicates all choose the first
    print(f"{name}: worst gradient error / bound = {worst:.3f}")
    if name == "skip_only":
        assert float(got["term"][0]) == 0.0 and not np.any(got["gx"])
    else:
        assert float(got["term"][0]) > 0


@pytest.mark.parametrize("name", ["2x7", "1x2049", "mixed"])
def test_two_calls_give_equal_bits(dev, name):
    batch, got, _ = _case(name)
    fw = _forward(batch, dev)
    gx = _backward(fw)
    for k in ("term", "G", "idx1", "idx2", "d"):
        assert np.array_equal(_np(fw[k]).view(np.int32), got[k].view(np.int32)), k
    assert np.array_equal(_np(gx).view(np.int32), got["gx"].view(np.int32))


def test_node_equals_the_entry_points(dev, flags):
    """ops.recon_chamfer: the term and d term / d recon of the two entry points bit for bit, nothing for the other inputs, the
    launches it says it issues, and inside a captured graph the same bits"""
    from hs_pose_amd import ops
    batch, got, fw = _case("mixed")
    t = {k: v.clone() for k, v in fw["dev"].items()}
    recon = t["recon"].requires_grad_(True)
    PC = t["PC"].requires_grad_(True)
    timer = ops.KernelTimer()
    prev = ops.set_timer(timer)
    try:
        term = ops.recon_chamfer(recon, PC, t["gt_R"], t["gt_t"], t["sym"], W)
        (GSCALE * term).backward()
    finally:
        ops.set_timer(prev)
    assert [r[0] for r in timer.records] == ["hsp_recon_chamfer_fwd", "hsp_recon_chamfer_bwd"]
    assert term.dim() == 0 and np.array_equal(_np(term).reshape(1).view(np.int32), got["term"].view(np.int32))
    assert np.array_equal(_np(recon.grad).view(np.int32), got["gx"].view(np.int32)) and PC.grad is None
    # captured (no host sync, no size decided by data): warm-up and capture on one side stream, the gradient asked for by
    # torch.autograd.grad so that no accumulator of a leaf is involved
    stat = t["recon"].detach().clone().requires_grad_(True)

    def body():
        out = ops.recon_chamfer(stat, t["PC"].detach(), t["gt_R"], t["gt_t"], t["sym"], W)
        return out, torch.autograd.grad(GSCALE * out, stat)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        out, gx = body()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np(out).reshape(1).view(np.int32), got["term"].view(np.int32))
    assert np.array_equal(_np(gx).view(np.int32), got["gx"].view(np.int32))


# ---- hsp_chamfer_bwd_ordered ---------------------------------------------------------------------------------------------------
BWD_CASES = {"1x1x1": (1, 1, 1), "2x100x50": (2, 100, 50), "3x7x2500": (3, 7, 2500), "2x2049x3": (2, 2049, 3), "hub": (2, 300, 40)}


@functools.lru_cache(maxsize=None)
def _bwd_case(name):
    import ref_cpu as ref
    B, n, m = BWD_CASES[name]
    x1 = ref.hash_tensor((B, n, 3), 50 + n, 0.3)
    x2 = ref.hash_tensor((B, m, 3), 51 + m, 0.3)
    if name == "hub":                              # one point of cloud 2 sits amid cloud 1, the rest far away: every point of 1 chooses it
        x2 = x2 + 5.0
        x2[:, 17] = 0.0
    g1 = ref.hash_tensor((B, n), 52, 1.0)
    g2 = ref.hash_tensor((B, m), 53, 1.0)
    return x1, x2, g1, g2


def _ordered(dev, x1, x2, i1, i2, g1, g2, want1=True, want2=True):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    B, n, _ = x1.shape
    m = x2.shape[1]
    a = [torch.as_tensor(v).to(dev).contiguous() for v in (x1, x2, i1, i2, g1, g2)]
    gx1 = torch.full((B, n, 3), float("nan"), device=dev)
    gx2 = torch.full((B, m, 3), float("nan"), device=dev)
    wsb = lib().hsp_chamfer_bwd_ordered_workspace_bytes(B, n, m)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ops._run("hsp_chamfer_bwd_ordered", tuple(ops._p(v) for v in a) + (B, n, m, ops._p(gx1) if want1 else ctypes.c_void_p(0),
                                                                      ops._p(gx2) if want2 else ctypes.c_void_p(0), ops._p(ws), wsb,
                                                                      ops._stream()))
    torch.cuda.synchronize()
    return _np(gx1), _np(gx2)


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_ordered_backward(dev, oc, flags, name):
    """hsp_chamfer_bwd_ordered on the oracle's arg-mins: every component within (c_i + 4) u sum |terms| of the fp64 contract and of
    the C oracle's serial scatter (c_i the row's in-degree); two runs bit-equal; one output alone (the other NULL) the same bits
    and the unwanted buffer untouched; through ops.chamfer with FLAGS.reproducible the same bits, with it off today's launch"""
    from hs_pose_amd import ops
    x1, x2, g1, g2 = _bwd_case(name)
    B, n, m = BWD_CASES[name]
    _, _, i1, i2 = oc.chamfer_fwd(x1.numpy(), x2.numpy())
    if name == "hub":
        assert np.all(i1 == 17)
    o1, o2 = oc.chamfer_bwd(x1.numpy(), x2.numpy(), i1, i2, g1.numpy(), g2.numpy())
    gx1, gx2 = _ordered(dev, x1, x2, i1, i2, g1, g2)
    worst = 0.0
    for b in range(B):
        w1, w2, m1, m2, c1, c2 = rc.bwd64(x1[b].numpy(), x2[b].numpy(), i1[b], i2[b], g1[b].numpy(), g2[b].numpy())
        for got, want, orc, mag, deg in ((gx1[b], w1, o1[b], m1, c1), (gx2[b], w2, o2[b], m2, c2)):
            bound = (deg[:, None] + 4) * U * mag
            assert np.all(np.abs(got - want) <= bound) and np.all(np.abs(got - orc) <= bound)
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300))))
    print(f"{name}: worst error / bound = {worst:.3f}")
    again = _ordered(dev, x1, x2, i1, i2, g1, g2)
    assert np.array_equal(again[0].view(np.int32), gx1.view(np.int32)) and np.array_equal(again[1].view(np.int32), gx2.view(np.int32))
    only1 = _ordered(dev, x1, x2, i1, i2, g1, g2, want2=False)
    only2 = _ordered(dev, x1, x2, i1, i2, g1, g2, want1=False)
    assert np.array_equal(only1[0].view(np.int32), gx1.view(np.int32)) and np.all(np.isnan(only1[1]))
    assert np.array_equal(only2[1].view(np.int32), gx2.view(np.int32)) and np.all(np.isnan(only2[0]))
    # through autograd
    names, grads = {}, {}
    for on in (False, True):
        flags.reproducible = on
        a, c = x1.to(dev).requires_grad_(True), x2.to(dev).requires_grad_(True)
        d1, d2, j1, j2 = ops.chamfer(a, c)
        assert np.array_equal(_np(j1), i1) and np.array_equal(_np(j2), i2)
        timer = ops.KernelTimer()
        prev = ops.set_timer(timer)
        try:
            torch.autograd.backward([d1, d2], [g1.to(dev), g2.to(dev)])
        finally:
            ops.set_timer(prev)
        torch.cuda.synchronize()
        names[on] = [(r[0], r[1]) for r in timer.records]
        grads[on] = (_np(a.grad), _np(c.grad))
    assert names[False] == [("hsp_chamfer_bwd", f"B{B}n{n}m{m}")], names[False]
    assert names[True] == [("hsp_chamfer_bwd_ordered", f"B{B}n{n}m{m}")], names[True]
    assert np.array_equal(grads[True][0].view(np.int32), gx1.view(np.int32))
    assert np.array_equal(grads[True][1].view(np.int32), gx2.view(np.int32))
    for b in range(B):                                                      # the atomic form: the same terms in another order
        _, _, m1, m2, c1, c2 = rc.bwd64(x1[b].numpy(), x2[b].numpy(), i1[b], i2[b], g1[b].numpy(), g2[b].numpy())
        assert np.all(np.abs(grads[False][0][b] - gx1[b]) <= 2 * (c1[:, None] + 4) * U * m1)
        assert np.all(np.abs(grads[False][1][b] - gx2[b]) <= 2 * (c2[:, None] + 4) * U * m2)


# ---- the fused path ------------------------------------------------------------------------------------------------------------
NET = ("recon", "face_normal", "face_dis", "face_f", "p_green_R", "p_red_R", "f_green_R", "f_red_R", "Pred_T", "Pred_s")


def test_pose_losses_with_the_term(dev, ref, flags):
    """fused_losses.pose_losses on a fixed net_out: the 19 terms torch.equal with the weight on and off; the 20th equal to
    ops.recon_chamfer's own bits and within (2 B N + 8) u + the target's bound of the readable statement in losses.py;
    total == old total + term, one fp32 add; d total / d recon equal to the sum of the two nodes' gradients; the other outputs'
    gradients untouched; untouched() true for the dict as built and false once the term is dropped or replaced"""
    from hs_pose_amd import ops
    from hs_pose_amd.fused_losses import EXTRA_TERM, LossDict, N_TERMS, TERMS, pose_losses, total_loss
    from hs_pose_amd.losses import prop_rot_loss
    gt, pred = ref.loss_case(96, 4000)
    gt = {k: v.to(dev) for k, v in gt.items()}

    def run(w):
        flags.prop_sym_cd_w = w
        p = {k: v.detach().to(dev).requires_grad_(True) for k, v in pred.items()}
        ld = pose_losses(p, gt["PC"], gt["gt_R"], gt["gt_t"], gt["gt_s"], gt["mean_shape"], gt["sym"], gt["obj_id"])
        return p, ld
    p0, ld0 = run(0.0)
    p1, ld1 = run(1.5)
    assert isinstance(ld1, LossDict) and len(ld1.terms) == N_TERMS == 19
    assert {g: list(d) for g, d in ld0.items()} == {g: list(k) for g, k in TERMS}
    assert {g: list(d) for g, d in ld1.items()} == {g: list(k) + (["Prop_sym_cd"] if g == "prop_loss" else []) for g, k in TERMS}
    assert EXTRA_TERM == ("prop_loss", "Prop_sym_cd") and ld0.extra is None and ld1.extra is ld1["prop_loss"]["Prop_sym_cd"]
    for g, keys in TERMS:
        for k in keys:
            assert torch.equal(ld0[g][k], ld1[g][k]), (g, k)
    cd = ld1["prop_loss"]["Prop_sym_cd"]
    B, N, _ = gt["PC"].shape
    alone = p1["recon"].detach().clone().requires_grad_(True)
    own = ops.recon_chamfer(alone, gt["PC"], gt["gt_R"], gt["gt_t"], gt["sym"], 1.5)
    assert cd.dim() == 0 and torch.equal(cd, own) and float(cd.detach()) > 0
    cpu = lambda t: t.detach().cpu()                                                                      # noqa: E731
    readable = prop_rot_loss().prop_sym_chamfer_loss(cpu(gt["PC"]), cpu(p1["recon"]), cpu(gt["gt_R"]), cpu(gt["gt_t"]), cpu(gt["sym"]), 1.5)
    # The two statements make G in fp32 by different operations, each within dG = 2^-23 (4 sum_k |p_k - t_k| + |G64|) of the fp64
    # target per component, so their targets differ by e <= 2 max dG and a squared distance by 2 |diff|_1 e + 3 e^2, with
    # |diff|_1 <= sqrt(3 d); summed over the 2 B N distances and scaled by w / (B N)
    cg = {k: cpu(v).numpy() for k, v in gt.items()}
    G64, mag = rc.target64(cg["PC"], cg["gt_R"], cg["gt_t"], cg["sym"])
    e = 2 * float(np.max(2.0 ** -23 * (4 * mag[..., None] + np.abs(G64))))
    dmax = 0.0
    for b in np.nonzero(~rc.classes(cg["sym"])[3])[0]:
        P = cpu(p1["recon"])[b].numpy()
        dmax = max(dmax, float(rc.search64(P, G64[b])[0].max()), float(rc.search64(G64[b], P)[0].max()))
    slack = 1.5 * 2 * (2 * np.sqrt(3 * dmax) * e + 3 * e * e)
    print(f"Prop_sym_cd fused {float(cd.detach())!r} readable {float(readable)!r} slack {slack:.3e}")
    assert abs(float(cd.detach()) - float(readable)) <= (2 * B * N + 8) * U * float(readable) + slack
    assert total_loss(ld1) is ld1.total and ld1.untouched() and ld0.untouched()
    assert torch.equal(ld1.total, ld0.total + cd) and torch.equal(ld0.total, total_loss(ld0))
    total_loss(ld0).backward()
    total_loss(ld1).backward()
    own.backward()
    for k in NET:
        if k == "recon":
            assert torch.equal(p1[k].grad, p0[k].grad + alone.grad) and float(alone.grad.abs().max()) > 0
        else:
            assert torch.equal(p1[k].grad, p0[k].grad), k
    # an edited dict is summed as it stands
    _, ld = run(1.5)
    ld["prop_loss"].pop("Prop_sym_cd")
    assert not ld.untouched() and abs(float(total_loss(ld).detach()) - float(ld0.total.detach())) <= 2e-6 * abs(float(ld0.total.detach()))
    _, ld = run(1.5)
    ld["prop_loss"]["Prop_sym_cd"] = 2.0 * ld["prop_loss"]["Prop_sym_cd"]
    assert not ld.untouched() and abs(float(total_loss(ld).detach()) - (float(ld0.total.detach()) + 2 * float(cd.detach()))) <= 2e-6 * abs(float(ld0.total.detach()))
    _, ld = run(0.0)
    ld["prop_loss"]["Prop_sym_cd"] = cd.detach()
    assert not ld.untouched()


# ---- whole steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train2x_f32", "train2x_bf16", "weight0"])
def test_steps_with_the_term(dev, mode):
    """tests/_recon_chamfer_step_check.py in a fresh process (a capture must precede the network's first eager backward)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_recon_chamfer_step_check.py"), mode], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
