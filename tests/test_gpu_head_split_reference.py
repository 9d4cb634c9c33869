"""GPU: the face head's split (hsp_face_split_fwd / _bwd) and a rotation head's split (hsp_axis_conf_fwd / _bwd) of
csrc/losses.hip against the float64 references of tests/_aug_heads_ref.py, every element within its own bound, through
ops.face_split / ops.axis_conf and -- where an upstream gradient is absent, and to see every column written -- through the C
entry points on a sentinel-filled gradient.

Bounds (derived in tests/_aug_heads_ref.py; tests/test_aug_heads_reference_host.py shows three wrong formulas leave them by 10x):
    normal           (5 + 2) 2^-24 |u|                                   its gradient   (11 + 2) 2^-24 (|a| + |u| sum|a_i||u_i|) / |v|
    axis             (6 + 2) 2^-24 |v| / d                               its gradient   (10 + 2) 2^-24 (|a| / d + sum|a_i||v_i| |v| / (|v| d^2))
    sigmoid          s (1 - s) de + 2 * 2^-24 s + 2^-126,  de = 2 (|x| + 2) 2^-23
    its gradient     |g| s (1 - s) de + (4 + 2) 2^-24 |g| s (1 + s) + (|g| + 1) 2^-126
    distances and their gradient: an exact copy; the columns of an absent upstream gradient: exactly 0.
Non-finite logits and a zero normal: the class (nan, or exactly 0 / 1) of the fp32 torch composition on the same input.

Rounding counts n and the largest err / (2^-24 mag) over the cases of this file on an MI355X (recorded by the last test, not
asserted: the bound is the derived n + 2):
    normals        n = 5    3.4        their gradient   n = 11   8.0
    axis           n = 6    2.5        its gradient     n = 10   3.9   a zero row (n = 1): 0.89
    sigmoid, err / bound:   face conf 0.71   its gradient 0.25   axis conf 0.35   its gradient 0.16
The fp32 torch composition on the CPU, same inputs (tests/test_aug_heads_reference_host.py): normals 1.9, their gradient 4.1, axis 1.6,
its gradient 3.7; sigmoid 0.52 and its gradient 0.13 of their bounds.
"""
import numpy as np
import pytest
import torch

import _aug_heads_cases as C
import _aug_heads_ref as A

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678e30
GRID_THREADS = 256 * 256 * 8                      # the grid cap of the stride kernels: HSP_NUM_CU * 8 workgroups of 256 threads
RATIOS = {}                                       # output -> worst measured err / bound, printed by the last test
SUBSETS3 = [s for s in ([a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)) if any(s)]


def _within(name, got, want, bound, mask=None, n=None):
    """every (selected) element of got within bound of want (float64, on the device).  Records the worst err / bound, or -- with the
    rounding count n of a bound (n + 2) 2^-24 mag -- the worst err / (2^-24 mag)"""
    err = (got.double() - want).abs()
    if mask is not None:
        err, bound = err[mask], bound[mask]
    if err.numel() == 0:
        return
    assert not torch.isnan(err).any(), name
    ratio = float(torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max()) * (1 if n is None else n + 2)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    over = err > bound
    assert not bool(over.any()), (name, int(over.sum()), ratio, torch.nonzero(over)[:4].tolist())


def _same_class(name, got, comp):
    """nan where the composition gives nan, not finite where it is not finite, bit-equal values (0 or 1) elsewhere"""
    nan = torch.isnan(comp)
    assert bool(torch.isnan(got[nan]).all()), name
    fin = torch.isfinite(comp)
    assert bool((~torch.isfinite(got[~fin])).all()), name
    assert torch.equal(got[fin], comp[fin]), (name, got[fin].tolist(), comp[fin].tolist())


def _face_bwd_raw(face, ups):
    """hsp_face_split_bwd with the absent gradients NULL, into a sentinel-filled g_face"""
    from hs_pose_amd import ops
    g = torch.full_like(face, SENTINEL)
    ops._run("hsp_face_split_bwd", (ops._p(face), ops._p(ups[0]), ops._p(ups[1]), ops._p(ups[2]), face.shape[0], ops._p(g), ops._stream()))
    torch.cuda.synchronize()
    return g


def _check_face_grad(label, g, face, ups, mask=None):
    """g (R, 30) from the upstream subset ``ups``: no sentinel left, absent columns exactly 0, distance columns an exact copy, the
    rest within the bound"""
    _, mags, want, gm = A.face_split64(face, *ups)
    b_g = A.face_split_bounds(face, mags, gm, ups[2])[3]
    assert not bool((g == SENTINEL).any()), label
    for u, cols in zip(ups, (slice(0, 18), slice(18, 24), slice(24, 30))):
        if u is None:
            assert bool((g[:, cols] == 0).all()), (label, cols)
    if ups[1] is not None:
        assert torch.equal(g[:, 18:24].view(torch.int32), ups[1].reshape(-1, 6).view(torch.int32)), label
    for u, cols, name, n in ((ups[0], slice(0, 18), "face grad normals", A.N_FACE_GRAD), (ups[2], slice(24, 30), "face grad conf", None)):
        if u is not None:
            _within(name, g[:, cols], want[:, cols], b_g[:, cols], None if mask is None else mask[:, cols], n=n)


@pytest.mark.parametrize("R", [1, 7, 43, 87400])
def test_face_split_rows(dev, R):
    """87 400 rows: 6 R = 524 400 > 256 * HSP_NUM_CU * 8 = 524 288 threads, so the stride loop of either kernel makes its second
    trip (the reference is computed on the device in float64)"""
    from hs_pose_amd import ops
    if R == 87400:
        assert 6 * (R - 100) <= GRID_THREADS < 6 * R
    face, gn, gd, gc = [torch.from_numpy(a).to(dev) for a in C.face_generic(R)]
    leaf = face.view(1, R, 30).clone().requires_grad_(True)
    nrm, dis, conf = ops.face_split(leaf)
    assert [tuple(o.shape) for o in (nrm, dis, conf)] == [(1, R, 6, 3), (1, R, 6), (1, R, 6)]
    outs, mags, _, _ = A.face_split64(face)
    b_n, _, b_c, _ = A.face_split_bounds(face, mags)
    _within("normals", nrm.detach().view(R, 6, 3), outs[0], b_n, n=A.N_FACE_NRM)
    _within("conf", conf.detach().view(R, 6), outs[2], b_c)
    assert torch.equal(dis.detach().view(R, 6).view(torch.int32), face[:, 18:24].contiguous().view(torch.int32))
    # all three upstream gradients through autograd, then each of the 7 subsets through the entry point on a sentinel-filled buffer
    (g_all,) = torch.autograd.grad([nrm, dis, conf], [leaf], [gn.view(1, R, 6, 3), gd.view(1, R, 6), gc.view(1, R, 6)], retain_graph=True)
    (g_nc,) = torch.autograd.grad([nrm, conf], [leaf], [gn.view(1, R, 6, 3), gc.view(1, R, 6)])
    for use in SUBSETS3:
        ups = [u if on else None for u, on in zip((gn, gd, gc), use)]
        g = _face_bwd_raw(face, ups)
        _check_face_grad(f"R={R} {use}", g, face, ups)
        if use == [1, 1, 1]:
            assert torch.equal(g.view(torch.int32), g_all.view(R, 30).view(torch.int32))
        if use == [1, 0, 1]:
            assert torch.equal(g.view(torch.int32), g_nc.view(R, 30).view(torch.int32))


def test_face_split_lengths_directions_and_logits(dev, monkeypatch):
    """|v| from 1e-12 to 1e12 by decades, upstream gradients parallel, antiparallel and orthogonal to the normal (where the
    projector a - u (a . u) cancels), the sigmoid from its bend to beyond fp32's range; non-finite logits and a zero normal follow
    the fp32 torch composition's class"""
    from hs_pose_amd import ops, PoseNet9D as P9
    face, gn, gd, gc, sp_n, sp_c = C.face_edges()
    assert sp_n.sum() == 1 and sp_c.sum() >= 3 * 3 and set(face[:, 24:][~sp_c].tolist()) == {float(np.float32(v)) for v in C.LOGITS if np.isfinite(v)}
    face, gn, gd, gc = [torch.from_numpy(a).to(dev) for a in (face, gn, gd, gc)]
    sp_n, sp_c = torch.from_numpy(sp_n).to(dev), torch.from_numpy(sp_c).to(dev)
    Rr = face.shape[0]
    ok_n = (~sp_n)[:, :, None].expand(Rr, 6, 3)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(P9, "FUSED_FACE_SPLIT", fused)
        leaf = face.view(1, Rr, 30).clone().requires_grad_(True)
        outs = P9._split_face_head(leaf)
        (g,) = torch.autograd.grad(outs, [leaf], [gn.view(1, Rr, 6, 3), gd.view(1, Rr, 6), gc.view(1, Rr, 6)])
        res.append((outs[0].detach().view(Rr, 6, 3), outs[1].detach().view(Rr, 6), outs[2].detach().view(Rr, 6), g.view(Rr, 30)))
    (nrm, dis, conf, g), (c_nrm, _, c_conf, c_g) = res
    outs, mags, _, _ = A.face_split64(face)
    b_n, _, b_c, _ = A.face_split_bounds(face, mags)
    _within("normals", nrm, outs[0], b_n, ok_n, n=A.N_FACE_NRM)
    _within("conf", conf, outs[2], b_c, ~sp_c)
    assert torch.equal(dis.view(torch.int32), face[:, 18:24].contiguous().view(torch.int32))
    ok_g = torch.cat([ok_n.reshape(Rr, 18), torch.ones(Rr, 6, dtype=torch.bool, device=dev), ~sp_c], dim=1)
    raw = _face_bwd_raw(face, [gn, gd, gc])
    assert bool(((g == raw) | (torch.isnan(g) & torch.isnan(raw))).all())
    _check_face_grad("edges", raw, face, [gn, gd, gc], ok_g)
    _same_class("normals of a zero vector", nrm[~ok_n], c_nrm[~ok_n])
    _same_class("conf of a non-finite logit", conf[sp_c], c_conf[sp_c])
    _same_class("gradient at a zero vector / a non-finite logit", g[~ok_g], c_g[~ok_g])
    assert int((~ok_g).sum()) == 3 + int(sp_c.sum())


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_axis_conf_rows(dev, monkeypatch, B):
    """rows on both sides of the 64-thread workgroup edge; |v| in {0, 1e-7, 1e-6, 1e-3, 1, 1e3}; the logits of the face test; a zero
    row gives the axis exactly 0 and the gradient g / float32(1e-6)"""
    from hs_pose_amd import ops, PoseNet9D as P9
    h_np, ga_np, gc_np, zero, special = C.axis_case(B)
    h, ga, gc = [torch.from_numpy(a).to(dev) for a in (h_np, ga_np, gc_np)]
    zero_d, sp = torch.from_numpy(zero).to(dev), torch.from_numpy(special).to(dev)
    if B >= 63:
        assert zero.sum() >= 10 and special.sum() >= 3 and len(set(np.linalg.norm(h_np[:, 1:], axis=1).round(9))) >= 6
    leaf = h.clone().requires_grad_(True)
    axis, conf = ops.axis_conf(leaf)
    assert tuple(axis.shape) == (B, 3) and tuple(conf.shape) == (B,)
    outs, mags, _, _ = A.axis_conf64(h)
    b_a, b_c, _ = A.axis_conf_bounds(h, mags)
    _within("axis", axis.detach(), outs[0], b_a, n=A.N_AXIS)
    _within("axis conf", conf.detach(), outs[1], b_c, ~sp)
    assert bool((axis.detach()[zero_d] == 0).all())
    (g_both,) = torch.autograd.grad([axis, conf], [leaf], [ga, gc])
    monkeypatch.setattr(P9, "FUSED_FACE_SPLIT", False)
    leaf2 = h.clone().requires_grad_(True)
    comp = P9._axis_and_confidence(leaf2)
    (c_g,) = torch.autograd.grad(comp, [leaf2], [ga, gc])
    _same_class("axis conf of a non-finite logit", conf.detach()[sp], comp[1].detach()[sp])
    for use in ([1, 1], [1, 0], [0, 1]):
        ups = [u if on else None for u, on in zip((ga, gc), use)]
        g = torch.full_like(h, SENTINEL)
        ops._run("hsp_axis_conf_bwd", (ops._p(h), ops._p(ups[0]), ops._p(ups[1]), B, ops._p(g), ops._stream()))
        torch.cuda.synchronize()
        assert not bool((g == SENTINEL).any()), use
        _, mags2, want, gm = A.axis_conf64(h, *ups)
        b_g = A.axis_conf_bounds(h, mags2, gm, ups[1])[2]
        if ups[0] is None:
            assert bool((g[:, 1:] == 0).all())
        else:
            _within("axis grad", g[:, 1:], want[:, 1:], b_g[:, 1:], n=A.N_AXIS_GRAD)
            # a zero row: g / float32(1e-6), one rounding (+ the usual 2 of slack)
            exact = ga.double()[zero_d] / A.EPS32
            _within("axis grad, zero row", g[:, 1:][zero_d], exact, (1 + 2) * A.U * exact.abs(), n=1)
        if ups[1] is None:
            assert bool((g[:, 0] == 0).all())
        else:
            _within("axis grad conf", g[:, 0], want[:, 0], b_g[:, 0], ~sp)
            _same_class("axis grad conf of a non-finite logit", g[:, 0][sp], c_g[:, 0][sp])
        if use == [1, 1]:
            same = (g == g_both) | (torch.isnan(g) & torch.isnan(g_both))
            assert bool(same.all())


def test_report_measured_ratios():
    """not a check: prints the worst measured err / bound of the cases above (the figures quoted at the head of this file)"""
    print("\n  head splits, worst err / (2^-24 mag) (conf: err / bound): " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))
