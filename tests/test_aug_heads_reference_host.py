"""Host: the float64 references of tests/_aug_heads_ref.py (augmentation, face split, axis / confidence split) are held to
independent statements of the same operations, and their error bound is shown to be honest and to have teeth, before the GPU
suites (tests/test_gpu_augment_reference.py, tests/test_gpu_head_split_reference.py) hold the kernels to them.

    anchor      augment64 on the draws the CPU generator hands out under seed 5 reproduces the reference-written fixture
                tests/golden/losses_augment.npz (tags all / half / none) within the bound.
    honest      the fp32 torch composition (augment.FUSED = False on the CPU, torch.rand handing out the test's draws) stays within
                HALF the bound on every input the GPU suite uses.
    teeth       every mutant of AUGMENT_MUTANTS / FACE_MUTANTS / AXIS_MUTANTS, evaluated in float64, leaves the bound by 10x or more.
    derivatives face_split64 / axis_conf64 backward equal torch.autograd in float64 on the composition of PoseNet9D.py:31-46 to 1e-12.

Rounding counts n per fired stage (bound = (sum of n + 2) 2^-24 mag):   PC: box 9, rigid 4, taper 13, jitter 3;  R: rigid 3;
t: rigid 4;  s: box 3, taper 9.
Largest err / (2^-24 mag) of the CPU fp32 composition over the GPU suite's inputs (recorded by
test_fp32_composition_within_half_the_bound, not asserted beyond the half bound):   PC 3.8   R 2.0   t 2.1   s 0.93
-- each below n + 2 of the shortest fired stage (3 + 2), and every element below half its own bound.
The head splits (n: normals 5, their gradient 11, axis 6, its gradient 10; the sigmoid's bound is derived from exp2), fp32 torch
composition on the CPU (test_fp32_head_compositions_within_the_bound):   normals 1.9   their gradient 4.1   axis 1.6   its gradient 3.7
sigmoid 0.52 and its gradient 0.13 of their bounds.
"""
import numpy as np
import pytest
import torch

import _aug_heads_cases as C
import _aug_heads_ref as A
from conftest import golden


def _worst(got, want, bound):
    """largest err / bound over the elements (bound 0 and err 0 -> 0)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)))


# ---- anchor ------------------------------------------------------------------------------------------------------------------------

def test_augment64_reproduces_the_reference_written_fixture(ref, flags):
    g = golden("losses_augment")
    gt = ref.augment_case()
    B, N = gt["PC"].shape[:2]
    assert (B, N) == (7, 64)
    for tag, pro in (("all", 1.1), ("half", 0.6), ("none", -1.0)):
        torch.manual_seed(5)                                    # the order check_augment (tests/test_losses.py) relies on
        draws = torch.cat([torch.rand((B, 1)) for _ in range(6)], dim=1).t().numpy()
        noise = (torch.rand((B, N, 3)) * flags.aug_pc_r).numpy()
        outs, mags = A.augment64(gt, draws, noise, pro, pro, pro, pro)
        fired = A.augment_fired(gt, draws, pro, pro, pro, pro)
        if tag == "half":
            assert all(0 < f.sum() for f in fired) and any(f.sum() < B for f in fired)
        for name, o, b in zip(("PC", "R", "t", "s"), outs, A.augment_bound(mags, fired)):
            want = g[f"{tag}.{name}"].astype(np.float64).reshape(o.shape)
            assert _worst(want, o, b) <= 1.0, (tag, name, _worst(want, o, b))


# ---- honest ------------------------------------------------------------------------------------------------------------------------

def _gpu_suite_cases():
    yield "combinations", C.case_all_combinations()[:3]
    for M in (1, 255, 256, 257):
        for N in (1, 255):
            yield f"all_fire_N{N}_M{M}", C.case_all_fire(N, M)
    yield "planted", C.case_planted_extremes()[:3]
    inp, settings = C.case_probability_edges()
    for i, (draws, p, _) in enumerate(settings):
        yield f"edges{i}", (inp, draws, p)


def _composition_fp32(monkeypatch, flags, inp, draws, p):
    """augment.data_augment's torch composition on the CPU in fp32, with torch.rand handing out ``draws`` and the raw jitter"""
    from hs_pose_amd import augment
    B, N = inp["PC"].shape[:2]
    queue = [torch.from_numpy(draws[q].reshape(B, 1).copy()) for q in range(6)] + [torch.from_numpy(inp["noise_raw"].copy())]

    def handed_out(*shape, **kw):
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        out = queue.pop(0)
        assert tuple(out.shape) == shape, (tuple(out.shape), shape)
        return out
    flags.aug_bb_pro, flags.aug_rt_pro, flags.aug_bc_pro, flags.aug_pc_pro = p
    assert np.float32(flags.aug_pc_r) == C.AUG_PC_R
    monkeypatch.setattr(augment, "FUSED", False)
    with monkeypatch.context() as m:
        m.setattr(torch, "rand", handed_out)
        got = augment.data_augment(*[torch.from_numpy(inp[k].copy()) for k in A.INPUT_KEYS])
    assert not queue
    return [o.numpy() for o in got]


def test_fp32_composition_within_half_the_bound(monkeypatch, flags, capsys):
    worst_u = dict(PC=0.0, R=0.0, t=0.0, s=0.0)
    for label, (inp, draws, p) in _gpu_suite_cases():
        got = _composition_fp32(monkeypatch, flags, inp, draws, p)
        outs, mags = A.augment64(inp, draws, inp["noise"], *p)
        fired = A.augment_fired(inp, draws, *p)
        for name, o32, o64, m, b in zip(("PC", "R", "t", "s"), got, outs, mags, A.augment_bound(mags, fired)):
            assert o32.dtype == np.float32
            worst_u[name] = max(worst_u[name], _worst(o32, o64, A.U * m))
            assert _worst(o32, o64, b) <= 0.5, (label, name, _worst(o32, o64, b))
    with capsys.disabled():
        print("\n  fp32 composition, worst err / (2^-24 mag): " + "  ".join(f"{k} {v:.2f}" for k, v in worst_u.items()))
    # the composition does round: a bound that an exact evaluation would also meet proves nothing
    assert worst_u["PC"] > 0.5 and worst_u["s"] > 0.5
    assert max(worst_u.values()) < min(A.N_PC["pc"], A.N_R["rt"], A.N_T["rt"], A.N_S["bb"]) + 2


def test_planted_extremes_decide_the_size():
    """without its planted point a cloud's size moves by far more than the bound: the planted index is the extreme"""
    inp, draws, p, plants = C.case_planted_extremes()
    outs, mags = A.augment64(inp, draws, inp["noise"], *p)
    b_s = A.augment_bound(mags, A.augment_fired(inp, draws, *p))[3]
    assert sorted({i for _, _, i in plants}) == [0, 255, 256, 1023]
    for b, (ax, _, i) in enumerate(plants):
        cut = dict(inp, model_point=inp["model_point"].copy())
        cut["model_point"][b, i] = 0.0
        s_cut = A.augment64(cut, draws, inp["noise"], *p)[0][3]
        assert abs(s_cut[b, ax] - outs[3][b, ax]) > 100.0 * b_s[b, ax], (b, ax, i)


# ---- teeth -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", A.AUGMENT_MUTANTS)
def test_augment_mutants_leave_the_bound(mutant):
    if mutant == "le_fires":                                    # shows only where a draw equals its probability
        inp, settings = C.case_probability_edges()
        draws, p, fires = settings[0]
        assert not fires
    else:
        inp, draws, p = C.case_all_combinations(N=33, M=257)
    outs, mags = A.augment64(inp, draws, inp["noise"], *p)
    bad = A.augment64(inp, draws, inp["noise"], *p, mutant=mutant)[0]
    # the true stages decide the budget (a mutant that fires another stage is judged by the bound of the cloud as it should be)
    bound = A.augment_bound(mags, A.augment_fired(inp, draws, *p))
    worst = max(_worst(o, w, b) for o, w, b in zip(bad, outs, bound))
    assert worst >= 10.0, (mutant, worst)


def _t(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


@pytest.mark.parametrize("mutant", A.FACE_MUTANTS)
def test_face_split_mutants_leave_the_bound(mutant):
    face, gn, gd, gc = _t(*C.face_generic(43))
    outs, mags, g, gm = A.face_split64(face, gn, gd, gc)
    bounds = A.face_split_bounds(face, mags, gm, gc)
    bo, _, bg, _ = A.face_split64(face, gn, gd, gc, mutant=mutant)
    worst = max([_worst(bg.numpy(), g.numpy(), bounds[3].numpy())] +
                [_worst(o.numpy(), w.numpy(), b.numpy()) for o, w, b in zip(bo, outs, bounds[:3])])
    assert worst >= 10.0, (mutant, worst)


@pytest.mark.parametrize("mutant", A.AXIS_MUTANTS)
def test_axis_conf_mutants_leave_the_bound(mutant):
    h, ga, gc, _, special = C.axis_case(130)
    keep = ~special
    h, ga, gc = _t(h[keep], ga[keep], gc[keep])
    outs, mags, g, gm = A.axis_conf64(h, ga, gc)
    bounds = A.axis_conf_bounds(h, mags, gm, gc)
    bo, _, bg, _ = A.axis_conf64(h, ga, gc, mutant=mutant)
    assert _worst(bo[0].numpy(), outs[0].numpy(), bounds[0].numpy()) >= 10.0
    assert _worst(bg.numpy(), g.numpy(), bounds[2].numpy()) >= 10.0


# ---- derivatives -------------------------------------------------------------------------------------------------------------------

SUBSETS3 = [s for s in ([a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)) if any(s)]


@pytest.mark.parametrize("use", SUBSETS3, ids=lambda s: "".join("ndc"[i] for i in range(3) if s[i]))
def test_face_split64_backward_equals_autograd(use):
    face, *ups = _t(*C.face_generic(43))
    ups = [u.double() if on else None for u, on in zip(ups, use)]
    f = face.double().requires_grad_(True)
    normals = f[:, :18].view(43, 6, 3)                          # PoseNet9D.py:31-35
    comp = (normals / normals.norm(dim=-1, keepdim=True), f[:, 18:24], f[:, 24:].sigmoid())
    (want,) = torch.autograd.grad([c for c, u in zip(comp, ups) if u is not None], [f], [u for u in ups if u is not None])
    outs, _, g, gm = A.face_split64(face, *ups)
    for o, c in zip(outs, comp):
        assert float((o - c.detach()).abs().max()) <= 1e-12
    assert bool(((g - want).abs() <= 1e-12 * torch.clamp(gm, min=1e-300)).all())
    assert float(want.abs().max()) > 0.1


@pytest.mark.parametrize("use", [[1, 1], [1, 0], [0, 1]], ids=["axis+conf", "axis", "conf"])
def test_axis_conf64_backward_equals_autograd(use):
    h, ga, gc, zero, special = C.axis_case(130)
    keep = ~special
    assert zero[keep].any()
    h, ga, gc = _t(h[keep], ga[keep], gc[keep])
    ups = [u.double() if on else None for u, on in zip((ga, gc), use)]
    x = h.double().requires_grad_(True)
    v = x[:, 1:]                                                # PoseNet9D.py:40-46, the guard as the fp32 code has it
    comp = (v / (v.norm(dim=1, keepdim=True) + A.EPS32), x[:, 0].sigmoid())
    (want,) = torch.autograd.grad([c for c, u in zip(comp, ups) if u is not None], [x], [u for u in ups if u is not None])
    outs, _, g, gm = A.axis_conf64(h, *ups)
    for o, c in zip(outs, comp):
        assert float((o - c.detach()).abs().max()) <= 1e-12
    assert bool(((g - want).abs() <= 1e-12 * torch.clamp(gm, min=1e-300)).all())


def test_fp32_head_compositions_within_the_bound(capsys):
    """the fp32 torch compositions of PoseNet9D.py:31-46 on the CPU (autograd's chain for the gradients) stay within the bounds of
    the closed formulas on the GPU suite's inputs; prints their worst err / (2^-24 mag) (sigmoid: err / bound)"""
    from hs_pose_amd import PoseNet9D as P9
    worst = {}

    def hold(name, got, want, bound, mag=None, mask=None):
        err = (got.double() - want).abs()
        unit = bound if mag is None else A.U * mag
        sel = (lambda x: x) if mask is None else (lambda x: x[mask])
        err, bound, unit = sel(err), sel(bound), sel(unit)
        worst[name] = max(worst.get(name, 0.0), float(torch.where(err > 0, err / unit.clamp(min=1e-300), torch.zeros_like(err)).max()))
        assert bool((err <= bound).all()), name
    edges = C.face_edges()
    for arrays, ok_n, ok_c in ((C.face_generic(43), None, None), (edges[:4], ~edges[4], ~edges[5])):
        face, gn, gd, gc = _t(*arrays)
        Rr = face.shape[0]
        leaf = face.view(1, Rr, 30).clone().requires_grad_(True)
        comp = P9._split_face_head(leaf)
        (g,) = torch.autograd.grad(comp, [leaf], [gn.view(1, Rr, 6, 3), gd.view(1, Rr, 6), gc.view(1, Rr, 6)])
        outs, mags, want, gm = A.face_split64(face, gn, gd, gc)
        b_n, _, b_c, b_g = A.face_split_bounds(face, mags, gm, gc)
        m_n = None if ok_n is None else torch.from_numpy(ok_n)[:, :, None].expand(Rr, 6, 3)
        m_c = None if ok_c is None else torch.from_numpy(ok_c)
        hold("normals", comp[0].detach().view(Rr, 6, 3), outs[0], b_n, mags[0], m_n)
        hold("normals' gradient", g.view(Rr, 30)[:, :18], want[:, :18], b_g[:, :18], gm[:, :18], None if m_n is None else m_n.reshape(Rr, 18))
        hold("sigmoid", comp[2].detach().view(Rr, 6), outs[2], b_c, None, m_c)
        hold("sigmoid's gradient", g.view(Rr, 30)[:, 24:], want[:, 24:], b_g[:, 24:], None, m_c)
        assert torch.equal(g.view(Rr, 30)[:, 18:24], gd)
    h, ga, gc, _, special = C.axis_case(130)
    h, ga, gc = _t(h[~special], ga[~special], gc[~special])
    leaf = h.clone().requires_grad_(True)
    comp = P9._axis_and_confidence(leaf)
    (g,) = torch.autograd.grad(comp, [leaf], [ga, gc])
    outs, mags, want, gm = A.axis_conf64(h, ga, gc)
    b_a, b_c, b_g = A.axis_conf_bounds(h, mags, gm, gc)
    hold("axis", comp[0].detach(), outs[0], b_a, mags[0])
    hold("axis' gradient", g[:, 1:], want[:, 1:], b_g[:, 1:], gm[:, 1:])
    hold("sigmoid", comp[1].detach(), outs[1], b_c)
    hold("sigmoid's gradient", g[:, 0], want[:, 0], b_g[:, 0])
    with capsys.disabled():
        print("\n  fp32 head compositions, worst err / (2^-24 mag) (sigmoid: err / bound): " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_sigmoid_bound_covers_an_fp32_exp2_evaluation():
    """the derivation beside sigmoid_bound, replayed in numpy fp32: e = exp2(fl(-x * fl(log2 e))) with a correctly rounded exp2,
    sigma = fl(1 / fl(1 + e)), with and without flushing denormals, stays within the bound at every finite logit of the suite"""
    x = np.array([v for v in C.LOGITS if np.isfinite(v)], np.float32)
    want = torch.sigmoid(torch.from_numpy(x).double()).numpy()
    bound = A.sigmoid_bound(torch.from_numpy(x)).numpy()
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2((-x * np.float32(np.log2(np.e))).astype(np.float64)).astype(np.float32)
        for flush in (False, True):
            ee = np.where(np.abs(e) < A.TINY, np.float32(0), e) if flush else e
            sg = (np.float32(1) / (np.float32(1) + ee)).astype(np.float32)
            sg = np.where(np.abs(sg) < A.TINY, np.float32(0), sg) if flush else sg
            assert (np.abs(sg.astype(np.float64) - want) <= bound).all(), (flush, x[np.abs(sg - want) > bound])
