"""GPU: every train-mode BatchNorm path (csrc/norm.hip and the first pass three products leave in their epilogues) against a plain
float64 reference on the CPU, computed from the same stored input values (bf16 inputs widened exactly) by the textbook formulas:

    mean = sum x / R          var = sum (x - mean)^2 / R          xhat = (x - mean) / sqrt(var + eps)
    y = relu?(xhat * gamma + beta)
    running_mean = (1 - m) rm + m mean        running_var = (1 - m) rv + m var R / (R - 1)   (R = 1: the biased var)
    dbeta = sum dz      dgamma = sum dz xhat      dx = gamma invstd (dz - dbeta / R - xhat dgamma / R),   dz = dy [y_ref > 0]

Part A: the entry points one by one at the widths, row counts and fold regimes no other test enters, their side effects, declines
and edge values.  Part B: the shifted per-tile sums of hsp_gemm_x3_bn_f32 / hsp_gemm_x3_bias_bn_f32 / hsp_gemm_rows_bn_bf16
against fp64 sums of the stored product, and their fold.  Part C: columns whose mean is far from zero (C1) and columns whose
mean is far from the SHIFT of the shifted sums (C2), where a one-pass fp32 variance loses digits.

Tolerances (the project's own): outputs and statistics 2e-5 of max(1, |ref|max); gradients 1e-4 of the reference's scale; a
bf16 output additionally one round-to-nearest-even of the value, 2^-8 |value|.

Part C2 as measured on an MI355X (error of y = xhat gamma + beta rebuilt from the saved statistics; rho = |mean - shift| / sigma):
    three-launch forms, row 0 a rho-sigma outlier, R = 2100, rho = 0 / 3 / 10 / 30 / 100:  1.1e-6 / 8.1e-7 / 1.9e-6 / 3.3e-5 /
    1.6e-4 (torch's fp32 batch_norm: 6.1e-7 / 5.2e-7 / 1.6e-6 / 4.9e-6 / 7.0e-6; the last two are on the outlier's own element,
    |y| = 33 and 50).  With one shift per tensor (row 0, the code before the per-chunk shift) the same cases gave 9.4e-6 / 4.5e-4 /
    4.0e-3 / 1.8e-2 from rho = 3 on and failed from rho = 10 on.
    epilogue forms, one shift per column, 256 rows: within the part-A tolerance up to rho = 10, outside it at 30 and 100 and there
    within 0.4 ... 0.8 of the emulation's error; the table is in DESIGN.md section 2.0.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_bf16_heads import _pitched

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
EPS = float(np.float32(1e-5))
TOL, GTOL = 2e-5, 1e-4
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
# entry-point suffix, storage type of x, storage type of y / dy / dx
FORMS = {"f32": ("", torch.float32, torch.float32), "bf16": ("_bf16", BF, BF), "mixed": ("_mixed", torch.float32, BF)}
RHOS = (0.0, 3.0, 10.0, 30.0, 100.0)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def _nblk(R, C):
    """row chunks of the three-launch forms, from the workspace the library asks for: [nblk][2][C] floats"""
    b = _L().hsp_bn_workspace_bytes(R, C)
    assert b > 0 and b % (8 * C) == 0
    return b // (8 * C)


def _ws(R, C, dev):
    return torch.empty(max(_L().hsp_bn_workspace_bytes(R, C), 16), dtype=torch.uint8, device=dev)


# ---- the float64 reference ------------------------------------------------------------------------------------------------------

def _d(t):
    return t.detach().cpu().double()


def _ref_fwd(x, gamma, beta, relu, eps=EPS):
    x, g, b = _d(x), _d(gamma), _d(beta)
    R = x.shape[0]
    mean = x.sum(0) / R
    var = ((x - mean) ** 2).sum(0) / R
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * invstd
    a = xhat * g + b
    return SimpleNamespace(R=R, mean=mean, var=var, invstd=invstd, xhat=xhat, a=a, y=a.clamp_min(0.0) if relu else a, gamma=g,
                           unbiased=var * R / (R - 1) if R > 1 else var)


def _ref_running(r, rm0, rv0, mom):
    m = float(np.float32(mom))
    return (1 - m) * _d(rm0) + m * r.mean, (1 - m) * _d(rv0) + m * r.unbiased


def _ref_bwd(r, dz, relu):
    dz = _d(dz)
    if relu:
        dz = dz * (r.y > 0)
    db = dz.sum(0)
    dg = (dz * r.xhat).sum(0)
    dx = r.gamma * r.invstd * (dz - db / r.R - r.xhat * dg / r.R)
    return dx, dg, db


def _err(got, want):
    got = _d(got)
    assert torch.isfinite(got).all()
    return (got - want).abs().max().item()


def _close(got, want, what, tol=TOL):
    scale = max(1.0, want.abs().max().item())
    err = _err(got, want)
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol * scale:.3e}"


def _close_bf16(got, want, what, floor):
    """a bf16 output: one round-to-nearest-even of a value that is itself within `floor` of the reference"""
    got = _d(got)
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    over = (got - want).abs() - (2.0 ** -8 * (want.abs() + floor) + floor)
    assert over.max().item() <= 0, f"{what}: {over.max().item():.3e} beyond one bf16 rounding + {floor:.3e}"


def _close_out(got, want, what):
    if got.dtype == BF:
        _close_bf16(got, want, what, TOL * max(1.0, want.abs().max().item()))
    else:
        _close(got, want, what)


def _gclose(got, want, what):
    scale = max(want.abs().max().item(), 1e-12)
    if got.dtype == BF:
        _close_bf16(got, want, what, GTOL * scale)
        return
    err = _err(got, want)
    assert err <= GTOL * scale, f"{what}: grad max abs err {err:.3e} vs scale {scale:.3e}"


# ---- the entry points ------------------------------------------------------------------------------------------------------------

def _affine(C, seed, dev):
    g = _gen(seed)
    return (1 + 0.3 * torch.randn(C, generator=g)).to(dev), (0.2 * torch.randn(C, generator=g)).to(dev)


def _running(C, seed, dev):
    g = _gen(seed)
    return [torch.randn(C, generator=g).to(dev), (0.5 + torch.rand(C, generator=g)).to(dev), torch.tensor([7], device=dev)]


def _benign(R, C, seed, dtype, dev, spread=1.0):
    """columns with their own deviation (0.5 ... 2, times `spread`) and a mean within two deviations of zero"""
    g = _gen(seed)
    sig = (0.5 + 1.5 * torch.rand(C, generator=g)) * spread
    x = torch.randn(R, C, generator=g) * sig + sig * (4 * torch.rand(C, generator=g) - 2)
    return x.to(dev, dtype)


def _fwd(form, x, gamma, beta, relu, mom=0.1, running=(None, None, None), ws=None, ws_bytes=None):
    sfx, _, yt = FORMS[form]
    R, C = x.shape
    y = torch.full((R, C), NAN, dtype=yt, device=x.device)
    mean, invstd = torch.full((C,), NAN, device=x.device), torch.full((C,), NAN, device=x.device)
    ws = _ws(R, C, x.device) if ws is None else ws
    rc = getattr(_L(), "hsp_bn_relu_fwd" + sfx)(_vp(x), R, C, _vp(gamma), _vp(beta), EPS, mom, relu, _vp(y), _vp(mean), _vp(invstd),
                                                _vp(running[0]), _vp(running[1]), _vp(running[2]), _vp(ws),
                                                ws.numel() if ws_bytes is None else ws_bytes, _stream())
    torch.cuda.synchronize()
    return rc, y, mean, invstd


def _bwd(form, x, dy, gamma, beta, mean, invstd, relu, ws_bytes=None):
    sfx, _, yt = FORMS[form]
    R, C = x.shape
    dx = torch.full((R, C), NAN, dtype=yt, device=x.device)
    dg, db = torch.full((C,), NAN, device=x.device), torch.full((C,), NAN, device=x.device)
    ws = _ws(R, C, x.device)
    rc = getattr(_L(), "hsp_bn_relu_bwd" + sfx)(_vp(x), _vp(dy), R, C, _vp(gamma), _vp(beta), _vp(mean), _vp(invstd), relu, _vp(dx),
                                                _vp(dg), _vp(db), _vp(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
    torch.cuda.synchronize()
    return rc, dx, dg, db


def _bwd2(x, dy, ldy, dy2, ldy2, gamma, beta, mean, invstd, relu):
    R, C = x.shape
    dx = torch.full((R, C), NAN, device=x.device)
    dg, db = torch.full((C,), NAN, device=x.device), torch.full((C,), NAN, device=x.device)
    ws = _ws(R, C, x.device)
    rc = _L().hsp_bn_relu_bwd2(_vp(x), _vp(dy), ldy, _vp(dy2), ldy2, R, C, _vp(gamma), _vp(beta), _vp(mean), _vp(invstd), relu, _vp(dx),
                               _vp(dg), _vp(db), _vp(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc, dx, dg, db


def _upstream(ref, r, relu, seed, dtype, dev):
    """an incoming gradient; where the pre-activation is within 1e-4 of the ReLU kink it is zero, so that an fp32 and an fp64
    evaluation of the mask cannot disagree about an element that matters"""
    dy = ref.hash_tensor(tuple(r.a.shape), seed, 1.0)
    if relu:
        dy[r.a.abs() < 1e-4] = 0.0
    return dy.to(dev, dtype)


# ==== Part A: shapes and fold regimes, benign columns ==============================================================================

# (R, C, row chunks the case is there for)
WIDTHS = [(100, 4, 4), (100, 8, 4), (100, 32, 4), (100, 512, 4), (100, 1024, 4)]
ROWS = [(1, 8, 1), (2, 8, 1), (31, 8, 1), (33, 8, 2),           # a single row; a last chunk of one row
        (6144, 8, 192), (6145, 8, 193),                         # the folds' "8 loads in flight" loop is entered from 193 chunks on
        (8192, 8, 256), (8193, 8, 257),
        (14369, 8, 450),                                        # ... and runs twice for some slices
        (16384, 8, 512), (16385, 8, 497)]                       # the cap; one more row: 33 rows per chunk


@pytest.mark.parametrize("R,C,nblk", WIDTHS + ROWS)
@pytest.mark.parametrize("form", list(FORMS))
def test_forward_and_backward_against_fp64(dev, ref, form, R, C, nblk):
    assert _nblk(R, C) == nblk            # (a change of the chunking rule must move these cases, not silently empty them)
    _, xt, yt = FORMS[form]
    for relu, mom in ((0, 0.37), (1, 0.1)):
        # R = 2: dx = gamma invstd (dz_0 - dz_1) / 2 * eps / (var + eps), what two terms of size |dz| leave of each other -- its
        # condition number is var / eps, so the two rows are drawn eps-close (var ~ eps) to keep dx a quantity fp32 resolves
        x = _benign(R, C, 100 + R + C + relu, xt, dev, spread=0.003 if R == 2 else 1.0)
        gamma, beta = _affine(C, 7 + relu, dev)
        run = _running(C, 9 + relu, dev)
        run0 = [t.clone() for t in run]
        r = _ref_fwd(x, gamma, beta, relu)
        rc, y, mean, invstd = _fwd(form, x, gamma, beta, relu, mom, run)
        assert rc == 0
        _close_out(y, r.y, f"y relu={relu}")
        _close(mean, r.mean, "save_mean")
        _close(invstd, r.invstd, "save_invstd")
        want_rm, want_rv = _ref_running(r, run0[0], run0[1], mom)
        _close(run[0], want_rm, "running_mean")
        _close(run[1], want_rv, "running_var")
        assert int(run[2]) == 8
        # no running statistics: accepted, and the same bits out
        rc, y2, mean2, invstd2 = _fwd(form, x, gamma, beta, relu, mom)
        assert rc == 0 and torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(invstd, invstd2)
        dy = _upstream(ref, r, relu, 11 + R + C, yt, dev)
        rc, dx, dg, db = _bwd(form, x, dy, gamma, beta, r.mean.float().to(dev), r.invstd.float().to(dev), relu)
        assert rc == 0
        want_dx, want_dg, want_db = _ref_bwd(r, dy, relu)
        _gclose(dx, want_dx, f"dx relu={relu}")
        _gclose(dg, want_dg, "dgamma")
        _gclose(db, want_db, "dbeta")


def test_num_batches_tracked_counts_calls(dev):
    x = _benign(100, 8, 1, torch.float32, dev)
    gamma, beta = _affine(8, 2, dev)
    run = _running(8, 3, dev)
    for k in range(3):
        assert _fwd("f32", x, gamma, beta, 1, 0.1, run)[0] == 0
        assert int(run[2]) == 8 + k


@pytest.mark.parametrize("nblk", [1, 64, 192, 193, 256, 257, 450, 512])
@pytest.mark.parametrize("mixed", [False, True])
def test_fold_of_given_partials(dev, mixed, nblk):
    """hsp_bn_relu_fwd_partials[_mixed] on [nblk][2][C] sums formed on the CPU (fp64 sums of 32-row tiles, the last one ragged,
    rounded to fp32 once; one shift per column, 0.3 sigma off the mean): what is left to go wrong is the fold and the apply"""
    L = _L()
    C, h = 8, 32
    R = h * nblk - 5
    x = _benign(R, C, 300 + nblk, torch.float32, dev)
    gamma, beta = _affine(C, 4, dev)
    x64 = _d(x)
    shift = (x64.mean(0) + 0.3 * x64.std(0)).float()
    shift_dev = shift.to(dev)
    d = torch.cat([x64 - shift.double(), torch.zeros(5, C, dtype=torch.float64)]).view(nblk, h, C)
    part = torch.stack([d.sum(1), (d * d).sum(1)], dim=1).float().to(dev)
    run = _running(C, 5, dev)
    run0 = [t.clone() for t in run]
    y = torch.full((R, C), NAN, dtype=BF if mixed else torch.float32, device=dev)
    mean, invstd = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
    fn = L.hsp_bn_relu_fwd_partials_mixed if mixed else L.hsp_bn_relu_fwd_partials
    rc = fn(_vp(x), R, C, _vp(gamma), _vp(beta), EPS, 0.37, 1, _vp(y), _vp(mean), _vp(invstd), _vp(run[0]), _vp(run[1]), _vp(run[2]),
            _vp(part), nblk, _vp(shift_dev), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    r = _ref_fwd(x, gamma, beta, 1)
    _close_out(y, r.y, "y")
    _close(mean, r.mean, "save_mean")
    _close(invstd, r.invstd, "save_invstd")
    want_rm, want_rv = _ref_running(r, run0[0], run0[1], 0.37)
    _close(run[0], want_rm, "running_mean")
    _close(run[1], want_rv, "running_var")
    assert int(run[2]) == 8


@pytest.mark.parametrize("R,C", [(37, 32), (3, 1024), (1000, 4)])
@pytest.mark.parametrize("form", list(FORMS))
def test_apply_with_given_statistics(dev, form, R, C):
    sfx, xt, yt = FORMS[form]
    x = _benign(R, C, 400 + R, xt, dev)
    gamma, beta = _affine(C, 6, dev)
    g = _gen(8)
    mean, invstd = torch.randn(C, generator=g).to(dev), (0.5 + torch.rand(C, generator=g)).to(dev)
    for relu in (0, 1):
        y = torch.full((R, C), NAN, dtype=yt, device=dev)
        rc = getattr(_L(), "hsp_bn_relu_apply" + ("" if form == "f32" else sfx))(_vp(x), R, C, _vp(mean), _vp(invstd), _vp(gamma), _vp(beta),
                                                                                relu, _vp(y), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        a = (_d(x) - _d(mean)) * _d(invstd) * _d(gamma) + _d(beta)
        _close_out(y, a.clamp_min(0.0) if relu else a, f"apply relu={relu}")


@pytest.mark.parametrize("given_invstd", [True, False])
def test_eval_against_fp64(dev, given_invstd):
    R, C = 37, 32
    x = _benign(R, C, 500, torch.float32, dev)
    gamma, beta = _affine(C, 6, dev)
    rm, rv, _ = _running(C, 12, dev)
    inv64 = 1.0 / torch.sqrt(_d(rv) + EPS)
    invstd = inv64.float().to(dev) if given_invstd else None
    for relu in (0, 1):
        y = torch.full((R, C), NAN, device=dev)
        rc = _L().hsp_bn_eval_f32(_vp(x), R, C, _vp(rm), _vp(rv), _vp(invstd), _vp(gamma), _vp(beta), EPS, relu, _vp(y), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        a = ((_d(x) - _d(rm)) * inv64) * _d(gamma) + _d(beta)
        _close(y, a.clamp_min(0.0) if relu else a, f"eval relu={relu}")


# dy: (pitch, column offset) or None = dense; the same for dy2, or "none"
@pytest.mark.parametrize("dy_at,dy2_at", [((1286, 6), "none"), ((1286, 6), None), ((1288, 8), "none"), ((1288, 8), None),
                                          (None, (1286, 6)), ((1286, 6), (1288, 8))])
def test_bwd2_pitched_gradients_against_fp64(dev, ref, dy_at, dy2_at):
    """pitch 1286 at column 6: even, ld & 3 == 2, rows 8-byte aligned -- the two 8-byte loads; pitch 1288 at column 8: 16-byte"""
    R, C = 300, 64
    x = _benign(R, C, 600, torch.float32, dev)
    gamma, beta = _affine(C, 6, dev)

    def place(at, seed):
        if at is None:
            t = ref.hash_tensor((R, C), seed, 1.0).to(dev)
            return t, C
        wide = ref.hash_tensor((R, at[0]), seed, 1.0).to(dev)
        blk = wide[:, at[1]:at[1] + C]
        assert blk.data_ptr() % 8 == 0 and (at[0] & 3) == (2 if at[0] == 1286 else 0)
        return blk, at[0]

    for relu in (0, 1):
        r = _ref_fwd(x, gamma, beta, relu)
        dy, ldy = place(dy_at, 21)
        dy2, ldy2 = (None, 0) if dy2_at == "none" else place(dy2_at, 22)
        total = _d(dy) + (_d(dy2) if dy2 is not None else 0.0)
        if relu:                                               # (see _upstream)
            near = (r.a.abs() < 1e-4).to(dev)
            dy[near] = 0.0
            if dy2 is not None:
                dy2[near] = 0.0
            total[near.cpu()] = 0.0
        rc, dx, dg, db = _bwd2(x, dy, ldy, dy2, ldy2, gamma, beta, r.mean.float().to(dev), r.invstd.float().to(dev), relu)
        assert rc == 0
        want_dx, want_dg, want_db = _ref_bwd(r, total, relu)
        _gclose(dx, want_dx, f"dx relu={relu}")
        _gclose(dg, want_dg, "dgamma")
        _gclose(db, want_db, "dbeta")


def test_declines_leave_the_outputs_untouched(dev):
    L = _L()
    x = _benign(100, 64, 700, torch.float32, dev)
    gamma, beta = _affine(64, 6, dev)

    def untouched(*ts):
        return all(torch.isnan(t).all().item() for t in ts)

    for form in FORMS:
        for C in (12, 6):                                      # 256 % (C / 4) != 0; C % 4 != 0
            xs = x[:, :C].contiguous().to(FORMS[form][1])
            rc, y, mean, invstd = _fwd(form, xs, gamma, beta, 1, ws=torch.empty(1 << 16, dtype=torch.uint8, device=dev))
            assert rc == UNSUPPORTED and untouched(y, mean, invstd), (form, C)
            rc, dx, dg, db = _bwd(form, xs, xs.to(FORMS[form][2]), gamma, beta, gamma, gamma, 1, ws_bytes=1 << 16)
            assert rc == UNSUPPORTED and untouched(dx, dg, db), (form, C)
            y = torch.full((100, C), NAN, dtype=FORMS[form][2], device=dev)
            rc = getattr(L, "hsp_bn_relu_apply" + FORMS[form][0])(_vp(xs), 100, C, _vp(gamma), _vp(gamma), _vp(gamma), _vp(beta), 1, _vp(y),
                                                                  _stream())
            assert rc == UNSUPPORTED and untouched(y), (form, C)
        xs = x.to(FORMS[form][1])
        need = L.hsp_bn_workspace_bytes(100, 64)
        rc, y, mean, invstd = _fwd(form, xs, gamma, beta, 1, ws_bytes=need - 1)
        assert rc == WORKSPACE and untouched(y, mean, invstd), form
        rc, dx, dg, db = _bwd(form, xs, xs.to(FORMS[form][2]), gamma, beta, gamma, gamma, 1, ws_bytes=need - 1)
        assert rc == WORKSPACE and untouched(dx, dg, db), form
    wide = torch.randn(100, 132, generator=_gen(1)).to(dev)
    odd = torch.randn(100, 131, generator=_gen(2)).to(dev)
    for dy, ldy, dy2, ldy2 in ((odd[:, 2:66], 131, None, 0),               # an odd pitch
                               (wide[:, :64], 60, None, 0),                # a pitch below C
                               (wide[:, 3:67], 132, None, 0),              # rows only 4-byte aligned
                               (wide[:, 4:68], 132, odd[:, 2:66], 131),    # the same faults in the second gradient
                               (wide[:, 4:68], 132, wide[:, 5:69], 132)):
        rc, dx, dg, db = _bwd2(x, dy, ldy, dy2, ldy2, gamma, beta, gamma, gamma, 1)
        assert rc == BAD_ARG and untouched(dx, dg, db), (ldy, ldy2)
    for nblk in (0, 513):
        part = torch.zeros(513, 2, 64, device=dev)
        for mixed in (False, True):
            y = torch.full((100, 64), NAN, dtype=BF if mixed else torch.float32, device=dev)
            mean, invstd = torch.full((64,), NAN, device=dev), torch.full((64,), NAN, device=dev)
            fn = L.hsp_bn_relu_fwd_partials_mixed if mixed else L.hsp_bn_relu_fwd_partials
            rc = fn(_vp(x), 100, 64, _vp(gamma), _vp(beta), EPS, 0.1, 1, _vp(y), _vp(mean), _vp(invstd), None, None, None, _vp(part), nblk,
                    _vp(gamma), _stream())
            torch.cuda.synchronize()
            assert rc == BAD_ARG and untouched(y, mean, invstd), nblk


@pytest.mark.parametrize("form", list(FORMS))
def test_edge_columns(dev, ref, form):
    """column 0 constant (var = 0, invstd = 1 / sqrt(eps), y = relu(beta), dx finite), column 1 with gamma = 0, column 2 in
    {-1, 0, 1} with mean exactly 0 and beta = 0: x-hat gamma + beta is exactly 0 on a third of its rows, where the mask (> 0)
    passes nothing"""
    _, xt, yt = FORMS[form]
    R, C = 90, 8
    x = _benign(R, C, 800, torch.float32, dev)
    x[:, 0] = 3.25
    x[:, 2] = torch.tensor([-1.0, 0.0, 1.0], device=dev).repeat(R // 3)
    x = x.to(xt)
    gamma, beta = _affine(C, 6, dev)
    gamma[1] = 0.0
    gamma[2], beta[2] = 1.0, 0.0
    beta[0] = 0.125
    for relu in (0, 1):
        r = _ref_fwd(x, gamma, beta, relu)
        assert r.var[0] == 0 and r.mean[2] == 0 and (r.a[:, 2] == 0).sum() == R // 3
        run = _running(C, 9, dev)
        run0 = [t.clone() for t in run]
        rc, y, mean, invstd = _fwd(form, x, gamma, beta, relu, 0.1, run)
        assert rc == 0
        _close_out(y, r.y, "y")
        assert (y[:, 0].float() == 0.125).all() and invstd[0].item() == pytest.approx(EPS ** -0.5, rel=1e-6)
        assert (y[:, 1] == (beta[1].clamp_min(0.0) if relu else beta[1]).to(yt)).all()
        _close(mean, r.mean, "save_mean")
        _close(invstd, r.invstd, "save_invstd")
        want_rm, want_rv = _ref_running(r, run0[0], run0[1], 0.1)
        _close(run[0], want_rm, "running_mean")
        _close(run[1], want_rv, "running_var")
        dy = _upstream(ref, r, 0, 31, yt, dev)                  # (no kink guard: the exact zeros are the point)
        if relu:
            keep = (r.a.abs() >= 1e-4) | (r.a == 0)
            dy = (dy.cpu() * keep).to(dev, yt)
            dy[x[:, 2] == 0, 2] = 1.0
        m32 = r.mean.float().to(dev)
        assert m32[2] == 0
        rc, dx, dg, db = _bwd(form, x, dy, gamma, beta, m32, r.invstd.float().to(dev), relu)
        assert rc == 0 and torch.isfinite(dx.float()).all()
        want_dx, want_dg, want_db = _ref_bwd(r, dy, relu)
        _gclose(dx, want_dx, "dx")
        _gclose(dg, want_dg, "dgamma")
        _gclose(db, want_db, "dbeta")
        # (relu: the rows at exactly 0 carry dy = 1 -- a mask of >= 0 would move dbeta[2] by 30)


# ==== Part B: the first pass three products leave in their epilogues ===============================================================

ENTRIES = ("x3_out", "x3_bias", "rows_bf16")
# (M, rows per cloud): whole tiles; one live row in the last tile; clouds that end inside a tile
EPI_SHAPES = [(256, 0), (257, 0), (300, 100)]
EPI_N = 128


def _tile_height(M, tiles):
    hs = [h for h in (64, 128) if (M + h - 1) // h == tiles]
    assert len(hs) == 1, (M, tiles)
    return hs[0]


def _epilogue(entry, A, W, bias, resid, cb, rpc, xyz3=None, w3=None):
    """run one product with its BatchNorm first pass.  A (M, K) rows (x3_out: the two sources are the column halves of A and W),
    W (N, K).  Returns rc, C (M, N) fp32, shift (N), part (tiles, 2, N), tiles, the two guard rows behind part."""
    from hs_pose_amd import ops
    L = _L()
    M, N = A.shape[0], W.shape[0]
    dev = A.device
    if entry == "rows_bf16":
        K = A.shape[1]
        tiles = L.hsp_gemm_rows_bn_tiles_bf16(M, N, K)
    else:
        tiles = L.hsp_gemm_x3_bn_tiles(M, N)
        if entry == "x3_out":
            assert tiles == (M + 63) // 64
    assert 0 < tiles <= 512
    out = torch.full((M, N), NAN, device=dev)
    buf = torch.full((1 + 2 * tiles + 2, N), NAN, device=dev)
    part = buf[1:1 + 2 * tiles]
    if entry == "rows_bf16":
        rc = L.hsp_gemm_rows_bn_bf16(_vp(A), A.stride(0), _vp(W), W.stride(0), K, M, N, _vp(bias), _vp(cb), rpc, _vp(xyz3), _vp(w3), _vp(out),
                                     N, _vp(buf[0]), _vp(part), _stream())
    elif entry == "x3_bias":
        P, ldp, ps = ops.x3_planes.planes(W, False)
        rc = L.hsp_gemm_x3_bias_bn_f32(_vp(A), A.stride(0), _vp(P), ldp, ps, A.shape[1], M, N, _vp(bias), _vp(out), N, _vp(buf[0]), _vp(part),
                                       _stream())
    else:
        K1 = A.shape[1] // 2
        A1, A2, W1, W2 = A[:, :K1], A[:, K1:], W[:, :K1].contiguous(), W[:, K1:].contiguous()
        P1, ldp1, ps1 = ops.x3_planes.planes(W1, False)
        P2, ldp2, ps2 = ops.x3_planes.planes(W2, False)
        rc = L.hsp_gemm_x3_bn_f32(_vp(A1), A.stride(0), _vp(P1), ldp1, ps1, K1, _vp(A2), A.stride(0), _vp(P2), ldp2, ps2, K1, M, N,
                                  _vp(resid), N, _vp(cb), rpc, _vp(out), N, _vp(buf[0]), _vp(part), _stream())
    torch.cuda.synchronize()
    return rc, out, buf[0], part.view(tiles, 2, N), tiles, buf[1 + 2 * tiles:]


def _epi_operands(entry, M, N, rpc, seed, dev):
    """operands as tests/test_gpu_gemm_x3.py and test_gpu_bf16_heads.py draw them; K = 1024 fp32 (the shallowest product
    hsp_gemm_x3_supported takes at so few rows), 64 bf16"""
    g = _gen(seed)
    bias = resid = cb = None
    if entry == "rows_bf16":
        K = 64
        A = _pitched(M, K, dev, seed)
        W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev, BF)
        bias = (torch.randn(N, generator=g) + 3).to(dev)
        if rpc:
            cb = torch.randn((M + rpc - 1) // rpc, N, generator=g).to(dev)
        return A, W, bias, resid, cb
    K = 1024
    assert _L().hsp_gemm_x3_supported(M, N, K if entry == "x3_bias" else K // 2, 0 if entry == "x3_bias" else K // 2) == 1
    A = (torch.randn(M, K, generator=g) * (1.0 + 3.0 * torch.rand(M, 1, generator=g))).to(dev)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dev)
    if entry == "x3_bias":
        bias = torch.randn(N, generator=g).to(dev)
    else:
        resid = torch.randn(M, N, generator=g).to(dev)
        cb = torch.randn((M + rpc - 1) // rpc if rpc else 1, N, generator=g).to(dev)
    return A, W, bias, resid, cb


def _documented_shift(bias, resid, cb):
    """include/hsp.h: the bias (+ cloud 0's per-cloud bias), or row 0 of the residual + cloud 0's per-cloud bias"""
    s = torch.zeros_like(bias if bias is not None else resid[0])
    for t in (bias, resid[0] if resid is not None else None, cb[0] if cb is not None else None):
        if t is not None:
            s = s + t
    return s


def _check_tile_sums(out, shift, part, tiles, guard):
    M = out.shape[0]
    h = _tile_height(M, tiles)
    assert torch.isnan(guard).all() and torch.isfinite(part).all()
    d = _d(out) - _d(shift)
    for t in range(tiles):
        blk = d[t * h:(t + 1) * h]
        s1, s2 = blk.sum(0), (blk * blk).sum(0)
        assert ((_d(part[t, 0]) - s1).abs() <= 1e-5 * blk.abs().sum(0)).all(), ("sum", t)
        assert ((_d(part[t, 1]) - s2).abs() <= 1e-5 * s2).all(), ("sum of squares", t)
    return h


def _fold(entry, out, part, tiles, shift, gamma, beta, mom, run):
    L = _L()
    M, N = out.shape
    mixed = entry == "rows_bf16"
    y = torch.full((M, N), NAN, dtype=BF if mixed else torch.float32, device=out.device)
    mean, invstd = torch.full((N,), NAN, device=out.device), torch.full((N,), NAN, device=out.device)
    fn = L.hsp_bn_relu_fwd_partials_mixed if mixed else L.hsp_bn_relu_fwd_partials
    rc = fn(_vp(out), M, N, _vp(gamma), _vp(beta), EPS, mom, 1, _vp(y), _vp(mean), _vp(invstd), _vp(run[0]), _vp(run[1]), _vp(run[2]),
            _vp(part), tiles, _vp(shift), _stream())
    torch.cuda.synchronize()
    return rc, y, mean, invstd


def _check_fold(entry, out, part, tiles, shift):
    N = out.shape[1]
    gamma, beta = _affine(N, 6, out.device)
    run = _running(N, 9, out.device)
    run0 = [t.clone() for t in run]
    rc, y, mean, invstd = _fold(entry, out, part, tiles, shift, gamma, beta, 0.1, run)
    assert rc == 0
    r = _ref_fwd(out, gamma, beta, 1)
    _close_out(y, r.y, "y")
    _close(mean, r.mean, "save_mean")
    _close(invstd, r.invstd, "save_invstd")
    want_rm, want_rv = _ref_running(r, run0[0], run0[1], 0.1)
    _close(run[0], want_rm, "running_mean")
    _close(run[1], want_rv, "running_var")
    assert int(run[2]) == 8


@pytest.mark.parametrize("M,rpc", EPI_SHAPES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_epilogue_first_pass_against_fp64_sums(dev, entry, M, rpc):
    if entry == "x3_bias" and rpc:
        rpc = 0                                # (no per-cloud term in this form: the ragged row count is the case)
    A, W, bias, resid, cb = _epi_operands(entry, M, EPI_N, rpc, 900 + M, dev)
    clouds = rpc
    if entry == "x3_out" and not rpc:
        rpc = M                                # (this form always has its per-cloud term: one cloud)
    rc, out, shift, part, tiles, guard = _epilogue(entry, A, W, bias, resid, cb, rpc)
    assert rc == 0 and torch.isfinite(out).all()
    assert torch.equal(shift, _documented_shift(bias, resid, cb))
    h = _check_tile_sums(out, shift, part, tiles, guard)
    rpc = clouds
    if M == 257:
        assert M % h == 1                      # the last tile has one live row
    if M == 256:
        assert M % h == 0
    if rpc:
        assert rpc % h != 0
    _check_fold(entry, out, part, tiles, shift)


@pytest.mark.parametrize("N,rider", [(128, True), (96, False), (96, True)])
def test_gemm_rows_bn_bf16_rider_and_ragged_columns(dev, N, rider):
    """the xyz3 . w3 rider, and N = 96: the second 64-column tile has 32 live columns.  96 is no BatchNorm width (256 % 24), so
    the fold declines it and writes nothing"""
    M, rpc = 300, 100
    A, W, bias, _, cb = _epi_operands("rows_bf16", M, N, rpc, 950 + N, dev)
    xyz3 = w3 = None
    if rider:
        g = _gen(3)
        xyz3, w3 = torch.randn(M, 3, generator=g).to(dev), torch.randn(N, 3, generator=g).to(dev)
    rc, out, shift, part, tiles, guard = _epilogue("rows_bf16", A, W, bias, None, cb, rpc, xyz3, w3)
    assert rc == 0 and torch.isfinite(out).all()
    c64 = _d(A) @ _d(W).t() + _d(bias) + _d(cb)[torch.arange(M) // rpc]
    mag = _d(A).abs() @ _d(W).abs().t() + _d(bias).abs() + _d(cb).abs()[torch.arange(M) // rpc]
    if rider:
        c64 = c64 + _d(xyz3) @ _d(w3).t()
        mag = mag + _d(xyz3).abs() @ _d(w3).abs().t()
    assert ((_d(out) - c64).abs() <= 4e-6 * (mag + 1)).all()
    assert torch.equal(shift, bias + cb[0])
    _check_tile_sums(out, shift, part, tiles, guard)
    if N == 96:
        gamma, beta = _affine(N, 6, dev)
        rc, y, mean, invstd = _fold("rows_bf16", out, part, tiles, shift, gamma, beta, 0.1, (None, None, None))
        assert rc == UNSUPPORTED and torch.isnan(y.float()).all() and torch.isnan(mean).all() and torch.isnan(invstd).all()
    else:
        _check_fold("rows_bf16", out, part, tiles, shift)


# ==== Part C: columns that make the shift matter ===================================================================================

C_ROWS, C_COLS = 2100, 64                                                    # eight groups of eight columns
MEAN_OVER_SIGMA = (0.0, 3.0, -10.0, 30.0, 100.0, -300.0, 1000.0, -1000.0)    # C1, per column group


def _group_rho(C):
    return torch.tensor([RHOS[(j // 8) % len(RHOS)] for j in range(C)], dtype=torch.float64)


def _stat_y(x, mean, invstd, gamma, beta):
    """y = xhat gamma + beta rebuilt in fp64 from saved statistics: the statistics' error alone, whatever the storage type of y"""
    return (_d(x) - _d(mean)) * _d(invstd) * _d(gamma) + _d(beta)


@pytest.mark.parametrize("form", list(FORMS))
def test_c1_three_launch_mean_far_from_zero(dev, form):
    """x = mu + sigma noise with |mu| / sigma up to 1000 and row 0 a typical row: the shift sits at the mean"""
    _, xt, _ = FORMS[form]
    g = _gen(41)
    sig = 0.5 + 1.5 * torch.rand(C_COLS, generator=g)
    mu = torch.tensor([MEAN_OVER_SIGMA[j // 8] for j in range(C_COLS)]) * sig
    x = (torch.randn(C_ROWS, C_COLS, generator=g) * sig + mu).to(dev, xt)
    gamma, beta = _affine(C_COLS, 6, dev)
    run = _running(C_COLS, 9, dev)
    run0 = [t.clone() for t in run]
    r = _ref_fwd(x, gamma, beta, 0)
    rc, y, mean, invstd = _fwd(form, x, gamma, beta, 0, 0.1, run)
    assert rc == 0
    _close_out(y, r.y, "y")
    _close(_stat_y(x, mean, invstd, gamma, beta), r.y, "y from the saved statistics")
    _close(mean, r.mean, "save_mean")
    _close(invstd, r.invstd, "save_invstd")
    want_rm, want_rv = _ref_running(r, run0[0], run0[1], 0.1)
    _close(run[0], want_rm, "running_mean")
    _close(run[1], want_rv, "running_var")


def _torch_fp32_yardstick(x, gamma, beta, rv0, mom):
    """torch's own fp32 batch_norm on the CPU, same stored values: (y, running_var)"""
    rm, rv = torch.zeros(x.shape[1]), rv0.detach().cpu().clone()
    y = torch.nn.functional.batch_norm(x.detach().cpu().float(), rm, rv, gamma.cpu(), beta.cpu(), True, mom, EPS)
    return y.double(), rv.double()


@pytest.mark.parametrize("form", list(FORMS))
def test_c2_three_launch_row0_outlier(dev, form):
    """row 0 sits rho sigma from its column's mean, rho in {0, 3, 10, 30, 100} by column group: against fp64, the error of y
    (rebuilt from the saved statistics; the fp32 rows themselves too) and of running_var may be the part-A tolerance or 8 x the
    error torch's fp32 batch_norm commits on the same tensor, whichever is larger"""
    _, xt, _ = FORMS[form]
    g = _gen(43)
    sig = 0.5 + 1.5 * torch.rand(C_COLS, generator=g)
    x = torch.randn(C_ROWS, C_COLS, generator=g) * sig + 0.5 * sig
    rho = _group_rho(C_COLS)
    x[0] = x[1:].mean(0) + rho.float() * x[1:].std(0)
    x = x.to(dev, xt)
    gamma, beta = _affine(C_COLS, 6, dev)
    run = _running(C_COLS, 9, dev)
    rv0 = run[1].clone()
    r = _ref_fwd(x, gamma, beta, 0)
    _, want_rv = _ref_running(r, run[0], rv0, 0.1)
    rc, y, mean, invstd = _fwd(form, x, gamma, beta, 0, 0.1, run)
    assert rc == 0
    ty, trv = _torch_fp32_yardstick(x, gamma, beta, rv0, 0.1)
    ys = _stat_y(x, mean, invstd, gamma, beta)
    bad = []
    for k, rh in enumerate(RHOS):
        cols = rho == rh
        tol_y = TOL * max(1.0, r.y[:, cols].abs().max().item())
        tol_v = TOL * max(1.0, want_rv[cols].abs().max().item())
        e_y, t_y = (ys - r.y)[:, cols].abs().max().item(), (ty - r.y)[:, cols].abs().max().item()
        e_v, t_v = (_d(run[1]) - want_rv)[cols].abs().max().item(), (trv - want_rv)[cols].abs().max().item()
        e_o = (_d(y) - r.y)[:, cols].abs().max().item() if y.dtype == torch.float32 else 0.0
        print(f"C2 {form} rho {rh:5.0f}: y err {e_y:.2e} (rows {e_o:.2e}; torch fp32 {t_y:.2e}), running_var err {e_v:.2e} (torch fp32 {t_v:.2e})")
        if max(e_y, e_o) > max(tol_y, 8 * t_y) or e_v > max(tol_v, 8 * t_v):
            bad.append(rh)
    assert not bad, f"beyond max(part-A tolerance, 8 x torch fp32) at rho {bad}"
    _close_out(y, r.y, "y")


def _c_operands(entry, M, N, kind, seed, dev):
    """part-C operands for an epilogue form.  C1: the additive terms (bias / residual row 0 + per-cloud bias) carry a column mean
    of MEAN_OVER_SIGMA x the product's deviation.  C2: no additive term at all (shift 0) and a positive A (1 + 0.1 |noise|: what a
    ReLU leaves) against weight rows with a mean, so that the product's own column mean is rho deviations from 0."""
    g = _gen(seed)
    K = 64 if entry == "rows_bf16" else 1024
    bias = resid = cb = None
    if kind == "C1":
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) * (0.05 if K == 1024 else K ** -0.5)
        sigma = (A.double() @ W.double().t()).std(0).float()
        mu = torch.tensor([MEAN_OVER_SIGMA[(j // 8) % 8] for j in range(N)]) * sigma
    else:
        A = 1.0 + 0.1 * torch.randn(M, K, generator=g).abs()
        tau = 0.05
        q = (_group_rho(N) * (A.std().item() / A.mean().item()) / K ** 0.5).float()       # w0 / sqrt(w0^2 + tau^2)
        assert q.max() < 0.9
        noise = torch.randn(N, K, generator=g)
        noise -= noise.mean(1, keepdim=True)                   # (a row sum of the noise would be a column mean of its own)
        W = noise * tau + (tau * q / torch.sqrt(1 - q * q)).unsqueeze(1)
        mu = torch.zeros(N)
    if entry == "rows_bf16":
        Ap = torch.zeros(M, K, dtype=BF, device=dev)
        Ap[:] = A.to(dev, BF)
        A, W = Ap, W.to(dev, BF)
        bias = mu.to(dev)
    else:
        A, W = A.to(dev), W.to(dev)
        if entry == "x3_bias":
            bias = mu.to(dev)
        else:
            scale = 0.0 if kind == "C2" else 0.1
            resid = (scale * torch.randn(M, N, generator=g)).to(dev)
            cb = (mu + scale * torch.randn(1, N, generator=g)).to(dev)
    return A, W, bias, resid, cb


@pytest.mark.parametrize("entry", ENTRIES)
def test_c1_epilogue_mean_far_from_zero(dev, entry):
    M = EPI_SHAPES[0][0]
    A, W, bias, resid, cb = _c_operands(entry, M, EPI_N, "C1", 51, dev)
    rc, out, shift, part, tiles, guard = _epilogue(entry, A, W, bias, resid, cb, M if cb is not None else 0)
    assert rc == 0
    assert torch.equal(shift, _documented_shift(bias, resid, cb))
    _check_tile_sums(out, shift, part, tiles, guard)
    _check_fold(entry, out, part, tiles, shift)


def _emulate_documented_sums(out, shift, h, rv0, mom):
    """numpy float32, as the headers document it: d = c - shift; per tile of h rows sum d and sum d^2 over the rows; tiles folded
    in ascending order; mean = shift + s1 / R, var = s2 / R - (s1 / R)^2, running_var with the unbiased variance"""
    f = np.float32
    c, s = out.detach().cpu().numpy().astype(f), shift.detach().cpu().numpy().astype(f)
    R, N = c.shape
    d = c - s
    S1, S2 = np.zeros(N, f), np.zeros(N, f)
    for t0 in range(0, R, h):
        s1, s2 = np.zeros(N, f), np.zeros(N, f)
        for row in d[t0:t0 + h]:
            s1 = s1 + row
            s2 = s2 + row * row
        S1, S2 = S1 + s1, S2 + s2
    inv_r = f(1.0) / f(R)
    ms = S1 * inv_r
    var = np.maximum(S2 * inv_r - ms * ms, f(0.0))
    mean, invstd = s + ms, f(1.0) / np.sqrt(var + f(EPS))
    rv = (f(1.0) - f(mom)) * rv0.detach().cpu().numpy().astype(f) + f(mom) * (var * (f(R) / f(R - 1)))
    return torch.from_numpy(mean), torch.from_numpy(invstd), torch.from_numpy(rv).double()


@pytest.mark.parametrize("entry", ENTRIES)
def test_c2_epilogue_shift_far_from_mean(dev, entry):
    """the product's column mean is rho deviations from the shift (0).  The one-shift sums are not reworked here; they are pinned to
    their documentation: the error of y (rebuilt from the saved statistics) and of running_var against fp64 may be the part-A
    tolerance -- the resolution every BatchNorm output is held to -- or 4 x the error of the fp32 emulation of the documented
    summation, whichever is larger.  Prints the measured error per rho (DESIGN.md section 2 records it)."""
    M = EPI_SHAPES[0][0]
    A, W, bias, resid, cb = _c_operands(entry, M, EPI_N, "C2", 53, dev)
    rc, out, shift, part, tiles, guard = _epilogue(entry, A, W, bias, resid, cb, M if cb is not None else 0)
    assert rc == 0 and (shift == 0).all()
    h = _check_tile_sums(out, shift, part, tiles, guard)
    gamma, beta = _affine(EPI_N, 6, dev)
    run = _running(EPI_N, 9, dev)
    rv0 = run[1].clone()
    rc, y, mean, invstd = _fold(entry, out, part, tiles, shift, gamma, beta, 0.1, run)
    assert rc == 0
    r = _ref_fwd(out, gamma, beta, 1)
    _, want_rv = _ref_running(r, run[0], rv0, 0.1)
    rho_real = (r.mean - _d(shift)).abs() * r.invstd
    e_mean, e_invstd, e_rv = _emulate_documented_sums(out, shift, h, rv0, 0.1)
    ys, es = _stat_y(out, mean, invstd, gamma, beta), _stat_y(out, e_mean, e_invstd, gamma, beta)
    rho, bad = _group_rho(EPI_N), []
    for rh in RHOS:
        cols = rho == rh
        tol_y = TOL * max(1.0, r.a[:, cols].abs().max().item())
        tol_v = TOL * max(1.0, want_rv[cols].abs().max().item())
        e_y, m_y = (ys - r.a)[:, cols].abs().max().item(), (es - r.a)[:, cols].abs().max().item()
        e_v, m_v = (_d(run[1]) - want_rv)[cols].abs().max().item(), (e_rv - want_rv)[cols].abs().max().item()
        rel_var = ((_d(invstd) ** -2 - EPS) / r.var - 1)[cols].abs().max().item()
        print(f"C2 {entry} rho {rh:5.0f} (measured {rho_real[cols].min().item():.1f} ... {rho_real[cols].max().item():.1f}): y err {e_y:.2e} "
              f"of tolerance {tol_y:.2e} (emulation {m_y:.2e}), running_var err {e_v:.2e} (emulation {m_v:.2e}), "
              f"relative variance error {rel_var:.2e}" + (f" = {rel_var / (rh * rh * 2.0 ** -24):.1f} x rho^2 2^-24" if rh else ""))
        if e_y > max(tol_y, 4 * m_y) or e_v > max(tol_v, 4 * m_v):
            bad.append(rh)
    assert not bad, f"beyond max(part-A tolerance, 4 x the documented summation in fp32) at rho {bad}"
