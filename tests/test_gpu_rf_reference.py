"""GPU: the neighbourhood kernels of csrc/rfconv.hip (receptive-field graph convolution: forward, column-tile scatter backward,
gather-form backward) and the column-tile scatter of csrc/gather.hip against a plain float64 reference on the CPU, written
here from the formulas and fed the same stored values (bf16 inputs widened exactly):

    Dh      = D / max(||D||_col, 1e-12)                      (the 1e-12 is the kernels' constant, the fp32 nearest to 1e-12)
    R(i->m) = (x_m - x_i) / max(|x_m - x_i|, 1e-12)
    theta   = relu(R . Dh)
    surface: out[i,c] = mean_s max_n theta[i,n,sC+c]
    conv:    out[i,c] = fm[i,c] + mean_s max_n theta[i,n,sC+c] * fm[idx[i,n], C+sC+c]

    gfm[b,m,C+j] = sum_i [argrow[b,i,j]==m] g[b,i,j%C]/S * theta64         gfm[b,m,c] = g[b,m,c]   (bit for bit)
    gDh[d,j]     = sum [theta>0] g/S * fm[argrow,C+j] * R_d                gD = fp64 autograd of F.normalize(D, dim=0) on gDh

Selection is discontinuous, so the comparison is ROUTE-FORCED instead of allowing outliers: the forward's argrow must be a row
of the point's list whose fp64 product is within the forward tolerance of the fp64 maximum, and the FIRST slot holding the
maximum wherever the fp64 runner-up is further away than that (bit-equal products: the earliest slot); the backward is checked
against the sums over the kernel's own argrow.  The one other discontinuity, the mask [theta > 0] of the direction gradient,
is forced the same way: an element whose |theta64| is within the tolerance of zero may count or not.

Tolerances, per ELEMENT:  float sums  A * 2^-24 * sum|terms|  (terms: the products R_d Dh_d f / S of an output, g/S R_d Dh_d of
a grad_fm cell, J_de g/S f R_e of a direction gradient, J the normalisation Jacobian);  fixed-point cells (the tile backward)
additionally  n_terms * q / 2,  q = 2^(ex + ceil(log2 N) - 30),  ex the frexp exponent of max|g|/S over the aligned 64-channel
block of the column (a block is at least as wide as any tile);  bf16 gradients additionally 2^-8 |value|.  The bf16 forward
must equal twin(widened).bfloat16() bit for bit (tests/test_gpu_bf16.py).
A is 4x the worst ratio err / (2^-24 sum|terms|) of the fp32 torch composition of the same formulas on the same cases, rounded
up to a power of two (test_fp32_composition_sets_A holds that rule): the margin covers another association order.

Every case asserts the plan it enters (hsp_rf_fwd_plan, hsp_rf_bwd_scatter_plan, hsp_scatter_tile_plan: the dispatch calls the
same functions), so a change of a pick rule moves a case loudly instead of emptying it.

Measured ratios err / (2^-24 sum|terms|), worst over the cases of this file (composition on the CPU; kernels on an MI355X):
    composition:  out 3.1   product 4.9   grad_fm 4.8   grad_dirs 3.1      ->  A = 32 (4 x 4.9 = 19.6, rounded up)
    kernels:      out 4.5   product 0.0 (the winner is the fp64 maximum itself)   grad_fm, gather form 4.9   grad_dirs 10.2
                  column-tile scatter of gather.hip (float LDS adds) 3.5   ORL fg 2.7
                  grad_fm of the tile backward against its whole bound at A = 1, 2^-24 sum|terms| + n_terms q / 2:  2.4
    No kernel is above 10.2: the largest is the direction gradient, a sequential sum over a workgroup's points where torch sums
    pairwise.  The same table is in DESIGN.md section 2.0a.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
NAN = float("nan")
U = 2.0 ** -24
EPS = float(np.float32(1e-12))
A = 32.0
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
RATIOS = {}          # what -> worst measured err / (2^-24 sum|terms|), printed by the last test


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _u16(shape, dev):
    return torch.full(shape, -1, dtype=torch.int16, device=dev)         # 0xffff: no row of any cloud (N <= 65535)


def _rows16(t):
    return t.cpu().to(torch.int64) & 0xFFFF


def fwd_plan(k, S, C):
    p = ctypes.c_int(-1)
    return _L().hsp_rf_fwd_plan(k, S, C, ctypes.byref(p)), p.value


def bwd_plan(B, N, S, C, surface=0):
    r = ctypes.c_int(-1)
    return _L().hsp_rf_bwd_scatter_plan(B, N, S, C, surface, ctypes.byref(r)), r.value


def tile_plan(B, Nsrc, C):
    t = ctypes.c_int(-1)
    return _L().hsp_scatter_tile_plan(B, Nsrc, C, ctypes.byref(t)), t.value


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def _lists(B, N, k, g):
    """(B,N,k) neighbour lists with distinct rows per list (the gather-form backward needs that)"""
    if N <= 700:
        return torch.rand(B, N, N, generator=g).argsort(-1)[..., :k].to(torch.int32).contiguous()
    off = torch.randperm(N - 1, generator=g)[:k] + 1
    if N > 40000:
        off[-1] = 40000                                                  # rows >= 32768 behind the uint16 packing
    return ((torch.arange(N)[:, None] + off[None, :]) % N).to(torch.int32).expand(B, N, k).contiguous()


def _case(B, N, k, S, C, seed, surface=False, dtype=torch.float32):
    g = _gen(seed)
    xyz = 0.5 * torch.randn(B, N, 3, generator=g)
    idx = _lists(B, N, k, g)
    dirs = torch.randn(3, S * C, generator=g)
    fm = None if surface else torch.randn(B, N, (S + 1) * C, generator=g).to(dtype)
    return SimpleNamespace(B=B, N=N, k=k, S=S, C=C, xyz=xyz, idx=idx, dirs=dirs, fm=fm, surface=surface, dtype=dtype)


def _grad(c, seed, scale=1.0):
    return (scale * torch.randn(c.B, c.N, c.C, generator=_gen(seed))).to(c.dtype)


# ---- the float64 reference (dt = float32: the torch composition that sets A) ------------------------------------------------------

def _dh(dirs, dt):
    D = dirs.to(dt)
    return D / D.norm(dim=0).clamp_min(EPS)


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(EPS)


def _take(t, rows):
    """t (B,N,W), rows (B,N,m) int64 -> (B,N,m,W): t[b, rows[b,i,j], :]"""
    B, N, m = rows.shape
    return torch.gather(t, 1, rows.reshape(B, N * m, 1).expand(-1, -1, t.shape[2])).view(B, N, m, t.shape[2])


def _ref_fwd(c, dt=F64):
    B, N, k, S, C = c.B, c.N, c.k, c.S, c.C
    x, idx, Dh = c.xyz.to(dt), c.idx.long(), _dh(c.dirs, dt)
    R = _unit(_take(x, idx) - x[:, :, None, :])                          # (B,N,k,3)
    P = (R @ Dh).clamp_min(0)                                            # theta (B,N,k,SC)
    T = R.abs() @ Dh.abs()                                               # sum_d |R_d Dh_d|
    if not c.surface:
        f = torch.gather(c.fm.to(dt)[:, :, C:], 1, idx.reshape(B, N * k, 1).expand(-1, -1, S * C)).view(B, N, k, S * C)
        P, T = P * f, T * f.abs()
    mx = P.max(2).values
    Tm = T.max(2).values
    out = mx.view(B, N, S, C).sum(2) / S
    out_abs = Tm.view(B, N, S, C).sum(2) / S
    if not c.surface:
        ctr = c.fm.to(dt)[:, :, :C]
        out, out_abs = ctr + out, ctr.abs() + out_abs
    return SimpleNamespace(P=P, mx=mx, Tm=Tm, out=out, out_abs=out_abs)


def _ref_bwd(c, arg, g, dt=F64):
    """the sums over a given argrow (B,N,SC) int64; *_abs: sum|terms| of the same cell"""
    B, N, S, C = c.B, c.N, c.S, c.C
    SC = S * C
    x, DhT = c.xyz.to(dt), _dh(c.dirs, dt).t()                          # (SC,3)
    R = _unit(_take(x, arg) - x[:, :, None, :])                          # (B,N,SC,3)
    th = (R * DhT).sum(-1)
    tabs = (R.abs() * DhT.abs()).sum(-1)
    ga = g.to(dt).repeat(1, 1, S) / S
    pos = th > 0
    z = torch.zeros(B, N, SC, dtype=dt)
    sup = z.clone().scatter_add_(1, arg, ga * th * pos)
    sup_abs = z.clone().scatter_add_(1, arg, ga.abs() * tabs)
    marg = (th.abs() <= A * U * tabs) & (tabs > 0)                       # the mask [theta > 0] is undecided in fp32
    cnt = z.clone().scatter_add_(1, arg, ((ga != 0) & (pos | marg)).to(dt))   # terms the kernel can add: one per routed point, theta > 0
    w = ga if c.surface else ga * torch.gather(c.fm.to(dt)[:, :, C:], 1, arg)
    wR = w[..., None] * R
    gDh = (wR * pos[..., None]).sum((0, 1)).t().contiguous()             # (3,SC)
    gDh_abs = (wR.abs() * pos[..., None]).sum((0, 1)).t()
    gDh_marg = (wR.abs() * marg[..., None]).sum((0, 1)).t()
    D = c.dirs.to(dt).clone().requires_grad_(True)
    F.normalize(D, dim=0, eps=EPS).backward(gDh)
    n = c.dirs.to(dt).norm(dim=0)
    Dh = DhT.t()
    # the terms of gD_d = (gDh_d - Dh_d sum_e Dh_e gDh_e) / n, taken one by one: |1 - Dh_d^2| would hide what cancels in between
    Ja = (torch.eye(3, dtype=dt)[:, :, None] + (Dh[:, None, :] * Dh[None, :, :]).abs() * (n > EPS)) / n.clamp_min(EPS)
    gD_abs = torch.einsum("dej,ej->dj", Ja, gDh_abs)
    gD_marg = torch.einsum("dej,ej->dj", Ja, gDh_marg)
    return SimpleNamespace(sup=sup, sup_abs=sup_abs, cnt=cnt, gD=D.grad, gD_abs=gD_abs, gD_marg=gD_marg)


def _quantum(g, S, N, SC):
    """q (B,1,SC): 2^(ex + ceil(log2 N) - 30), ex from max|g|/S over the aligned 64-channel block of the column; 0 for a zero block"""
    B, _, C = g.shape
    gm = g.double().abs().amax(1) / S                                    # (B,C)
    nb = (C + 63) // 64
    pad = torch.zeros(B, nb * 64, dtype=F64)
    pad[:, :C] = gm
    bm = pad.view(B, nb, 64).amax(2)                                     # (B,nb)
    ex = torch.frexp(bm).exponent.double()
    q = torch.where(bm > 0, 2.0 ** (ex + (N - 1).bit_length() - 30), torch.zeros_like(bm))
    col = (torch.arange(SC) % C) // 64
    return q[:, col][:, None, :]


def _ratio(what, err, terms):
    ok = terms > 0
    r = (err[ok] / (U * terms[ok])).max().item() if ok.any() else 0.0
    RATIOS[what] = max(RATIOS.get(what, 0.0), r)
    return r


def _hold(got, want, tol, what, kind=None, terms=None):
    """|got - want| <= tol element by element; a sentinel left behind (NaN) fails"""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    err = (got - want).abs()
    if kind is not None:
        print(f"  {what}: ratio {_ratio(kind, err, terms):.3f}")
    over = err - tol
    i = over.argmax()
    assert over.flatten()[i] <= 0, (f"{what}: |err| {err.flatten()[i]:.3e} > tol {tol.flatten()[i]:.3e} at {np.unravel_index(int(i), over.shape)}"
                                    f" (want {want.flatten()[i]:.6e})")


# ---- the entry points -------------------------------------------------------------------------------------------------------------

def _sfx(c):
    return "_bf16" if c.dtype == BF else ""


def _run_fwd(c, dev, want_fwin=True):
    B, N, k, S, C = c.B, c.N, c.k, c.S, c.C
    out = torch.full((B, N, C), NAN, dtype=c.dtype, device=dev)
    arg = _u16((B, N, S * C), dev)
    xyz, idx, dirs = c.xyz.to(dev), c.idx.to(dev), c.dirs.to(dev)
    if c.surface:
        rc = getattr(_L(), "hsp_rf_surface_fwd" + _sfx(c))(_vp(xyz), _vp(idx), _vp(dirs), B, N, k, S, C, _vp(out), _vp(arg), _stream())
        fwin = None
    else:
        fm = c.fm.to(dev)
        fwin = torch.full((B, N, S * C), NAN, dtype=c.dtype, device=dev) if want_fwin else None
        rc = getattr(_L(), "hsp_rf_conv_fwd" + _sfx(c))(_vp(xyz), _vp(idx), _vp(dirs), _vp(fm), B, N, k, S, C, _vp(out), _vp(arg),
                                                        _vp(fwin), _stream())
    torch.cuda.synchronize()
    return rc, out, arg, fwin


def _run_scatter(c, arg, g, dev, fwin=None, use_fwin=True):
    """hsp_rf_conv_bwd_scatter* / hsp_rf_surface_bwd*; arg: the uint16 rows as stored (int16 bits) on the device"""
    B, N, S, C = c.B, c.N, c.S, c.C
    SC = S * C
    wsb = _L().hsp_rf_bwd_scatter_workspace_bytes(B, SC)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    gd = torch.full((3, SC), NAN, device=dev)
    xyz, dirs, gg = c.xyz.to(dev), c.dirs.to(dev), g.to(dev)
    if c.surface:
        rc = getattr(_L(), "hsp_rf_surface_bwd" + _sfx(c))(_vp(xyz), _vp(dirs), _vp(arg), _vp(gg), B, N, S, C, _vp(gd), _vp(ws), wsb,
                                                           _stream())
        gfm = None
    else:
        gfm = torch.full((B, N, (S + 1) * C), NAN, dtype=c.dtype, device=dev)
        fm = c.fm.to(dev)
        rc = getattr(_L(), "hsp_rf_conv_bwd_scatter" + _sfx(c))(_vp(xyz), _vp(dirs), _vp(None if use_fwin else fm),
                                                                _vp(fwin if use_fwin else None), _vp(arg), _vp(gg), B, N, S, C,
                                                                _vp(gfm), _vp(gd), _vp(ws), wsb, _stream())
    torch.cuda.synchronize()
    return rc, gfm, gd


def _run_csr(c, arg, g, dev):
    B, N, k, S, C = c.B, c.N, c.k, c.S, c.C
    SC = S * C
    idx = c.idx.to(dev)
    off = torch.empty(B, N + 1, dtype=torch.int32, device=dev)
    edge = torch.empty(B, N * k, dtype=torch.int32, device=dev)
    assert _L().hsp_rev_build(_vp(idx), B, N, N, k, k, _vp(off), _vp(edge), _stream()) == 0
    wsb = _L().hsp_rf_bwd_workspace_bytes(SC)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    gfm = torch.full((B, N, (S + 1) * C), NAN, device=dev)
    gd = torch.full((3, SC), NAN, device=dev)
    xyz, dirs, fm, gg = c.xyz.to(dev), c.dirs.to(dev), c.fm.to(dev), g.to(dev)
    rc = _L().hsp_rf_conv_bwd(_vp(xyz), _vp(dirs), _vp(fm), _vp(arg), _vp(gg), _vp(off), _vp(edge), B, N, k, S, C, _vp(gfm), _vp(gd),
                              _vp(ws), wsb, _stream())
    torch.cuda.synchronize()
    return rc, gfm, gd


# ---- the checks -------------------------------------------------------------------------------------------------------------------

def _check_fwd(c, out, arg, fwin, what="fwd"):
    B, N, k, S, C = c.B, c.N, c.k, c.S, c.C
    r = _ref_fwd(c)
    rows = _rows16(arg)                                                  # (B,N,SC)
    hit = c.idx.long()[:, :, :, None] == rows[:, :, None, :]             # (B,N,k,SC)
    assert hit.any(2).all(), f"{what}: argrow is not a row of the point's list"
    slots = torch.arange(k)[None, None, :, None]
    slot = torch.where(hit, slots, k).min(2).values
    Pw = r.P.gather(2, slot[:, :, None, :]).squeeze(2)
    tol = A * U * r.Tm
    print(f"  {what}: product ratio {_ratio('product', r.mx - Pw, r.Tm):.3f}")
    assert (r.mx - Pw <= tol).all(), f"{what}: the winner's fp64 product is not the maximum"
    first = torch.where(r.P == r.mx[:, :, None, :], slots, k).min(2).values
    second = torch.where(r.P < r.mx[:, :, None, :], r.P, torch.full_like(r.P, -float("inf"))).max(2).values
    clear = (r.mx - second) > tol
    assert clear.float().mean() > 0.9
    assert (slot[clear] == first[clear]).all(), f"{what}: not the first slot holding the maximum"
    otol = A * U * r.out_abs
    if c.dtype == BF:
        otol = otol + 2.0 ** -8 * r.out.abs()
    _hold(out, r.out, otol, what + " out", None if c.dtype == BF else "out", r.out_abs)
    if fwin is not None:
        assert torch.equal(fwin.cpu(), torch.gather(c.fm[:, :, C:], 1, rows)), f"{what}: fwin != fm[argrow, C+j]"
    return rows


def _check_bwd(c, rows, g, gfm, gd, fixed, what):
    C = c.C
    r = _ref_bwd(c, rows, g)
    bf = 2.0 ** -8 if c.dtype == BF else 0.0
    if gfm is not None:
        gfm = gfm.cpu()
        assert torch.equal(gfm[:, :, :C], g), f"{what}: centre columns are not a copy of grad_out"
        tol = A * U * r.sup_abs + bf * r.sup.abs()
        terms = r.sup_abs
        if fixed:                                                         # (reported against 2^-24 sum|terms| + n_terms q / 2)
            fx = r.cnt * _quantum(g, c.S, c.N, c.S * C) / 2
            tol, terms = tol + fx, terms + fx / U
        _hold(gfm[:, :, C:], r.sup, tol, what + " grad_fm", None if bf else "grad_fm" + (" (fixed point)" if fixed else ""), terms)
    # (grad_dirs is fp32 whatever the rows' type: the same arithmetic on the widened values, nothing is rounded to bf16)
    _hold(gd, r.gD, A * U * r.gD_abs + r.gD_marg, what + " grad_dirs", "grad_dirs", r.gD_abs)
    return r


# ==== the rule that sets A ========================================================================================================

COMPOSITION = [(3, 41, 6, 3, 64), (2, 150, 8, 2, 192), (1, 33, 5, 7, 512), (1, 1079, 4, 1, 16)]


def test_fp32_composition_sets_A():
    """A = 4 x the worst ratio of the fp32 torch composition of the reference's own formulas, rounded up to a power of two"""
    worst = {}
    for n, (B, N, k, S, C) in enumerate(COMPOSITION):
        c = _case(B, N, k, S, C, 900 + n)
        r64, r32 = _ref_fwd(c), _ref_fwd(c, torch.float32)
        worst["out"] = max(worst.get("out", 0), _ratio("composition out", (r32.out.double() - r64.out).abs(), r64.out_abs))
        worst["product"] = max(worst.get("product", 0), _ratio("composition product", (r32.mx.double() - r64.mx).abs(), r64.Tm))
        rows = torch.gather(c.idx.long(), 2, r64.P.argmax(2))               # the fp64 winners' rows
        g = _grad(c, 950 + n)
        b64, b32 = _ref_bwd(c, rows, g), _ref_bwd(c, rows, g, torch.float32)
        worst["grad_fm"] = max(worst.get("grad_fm", 0), _ratio("composition grad_fm", (b32.sup.double() - b64.sup).abs(), b64.sup_abs))
        worst["grad_dirs"] = max(worst.get("grad_dirs", 0), _ratio("composition grad_dirs",
                                                                 ((b32.gD.double() - b64.gD).abs() - b64.gD_marg).clamp_min(0), b64.gD_abs))
    print("  composition ratios:", {k: round(v, 3) for k, v in worst.items()})
    w = max(worst.values())
    rule = 2.0 ** np.ceil(np.log2(4 * w))
    assert rule <= A <= 2 * rule, f"the composition's worst ratio {w:.3f} asks for A = {rule}"


# ==== forward ======================================================================================================================

# B, N, k, S, C, column slots, pipelined
FWD = [(3, 41, 6, 3, 64, 1, 1), (1, 33, 6, 3, 512, 2, 1), (1, 33, 5, 5, 512, 3, 1), (1, 33, 5, 7, 512, 4, 1),
       (2, 33, 8, 8, 128, 1, 0), (1, 20, 8, 8, 512, 4, 0),                # the plain kernel
       (1, 40, 32, 7, 128, 1, 1), (1, 40, 33, 7, 128, 1, 0),              # the pipeline boundary
       (2, 9, 1, 1, 4, 1, 1),                                             # C = 4, S = 1, k = 1
       (1, 310, 300, 1, 16, 1, 0)]                                        # k > 256: the plain kernel's fill loop strides


@pytest.mark.parametrize("B,N,k,S,C,nch,pipe", FWD)
def test_conv_forward(dev, B, N, k, S, C, nch, pipe):
    assert fwd_plan(k, S, C) == (nch, pipe)
    c = _case(B, N, k, S, C, 1000 + N + k + C)
    rc, out, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    _check_fwd(c, out, arg, fwin)
    rc, out2, arg2, _ = _run_fwd(c, dev, want_fwin=False)               # without the fwin stream: the same bits
    assert rc == 0 and torch.equal(out, out2) and torch.equal(arg, arg2)


@pytest.mark.parametrize("B,N,k,S,C,nch,pipe", [FWD[0], FWD[2], FWD[4], FWD[5]])
def test_conv_forward_bf16_is_the_rounded_twin(dev, B, N, k, S, C, nch, pipe):
    assert fwd_plan(k, S, C) == (nch, pipe)
    c = _case(B, N, k, S, C, 1100 + N + C, dtype=BF)
    rc, out, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    _check_fwd(c, out, arg, fwin, "bf16 fwd")
    twin = SimpleNamespace(**{**vars(c), "fm": c.fm.float(), "dtype": torch.float32})
    rc, out32, arg32, fwin32 = _run_fwd(twin, dev)
    assert rc == 0 and torch.equal(arg, arg32) and torch.equal(out, out32.bfloat16()) and torch.equal(fwin, fwin32.bfloat16())


@pytest.mark.parametrize("B,N,k,S,C,nch,pipe", [FWD[0], FWD[4], (1, 30, 5, 4, 1024, 4, 0)])
def test_surface_forward(dev, B, N, k, S, C, nch, pipe):
    assert fwd_plan(k, S, C) == (nch, pipe)
    c = _case(B, N, k, S, C, 1200 + N + C, surface=True)
    rc, out, arg, _ = _run_fwd(c, dev)
    assert rc == 0
    _check_fwd(c, out, arg, None, "surface fwd")


@pytest.mark.parametrize("B", [1, 3, 5, 8, 9])
@pytest.mark.parametrize("N,k,S,C", [(5, 3, 3, 64), (11, 4, 8, 128)])     # pipelined / plain; some workgroups get no point
def test_forward_point_schedule(dev, B, N, k, S, C):
    c = _case(B, N, k, S, C, 1300 + B + N)
    rc, out, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    _check_fwd(c, out, arg, fwin)


def test_forward_rows_above_32768(dev):
    """N = 65535: the winning rows fill the uint16, neighbour rows >= 32768 (and the 32-bit byte offsets of the pipelined gather)"""
    assert fwd_plan(4, 1, 4) == (1, 1)
    c = _case(1, 65535, 4, 1, 4, 1400)
    assert (c.idx >= 32768).any()
    rc, out, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    rows = _check_fwd(c, out, arg, fwin)
    assert (rows >= 32768).any()


def _tied_case(zero, S=3, C=64):
    """rows duplicated in xyz AND fm under different row numbers: their products are bit-equal, the earliest slot must win.
    zero: every neighbour direction is orthogonal to every support direction (all products exactly +-0); else equal, nonzero"""
    c = _case(2, 24, 6, S, C, 1500 + zero)
    c.xyz[:, 12:] = c.xyz[:, :12]
    c.fm[:, 12:] = c.fm[:, :12]
    idx = c.idx.clone()
    half = idx[:, :, :3] % 12
    half[:, :, 1] = (half[:, :, 0] + 1) % 12                              # three distinct rows of the first half ...
    half[:, :, 2] = (half[:, :, 0] + 2) % 12
    c.idx = torch.cat([half + 12, half], 2).contiguous()                  # ... their copies first: slot n and slot n + 3 tie
    if zero:
        c.xyz[:, :, 1:] = 0.0                                             # neighbours differ in x only: R = (+-1, 0, 0) ...
        c.dirs[0, :] = 0.0                                                # ... and no direction has an x part: theta = +-0
    return c


SCHEDULES = [(3, 64, 1), (8, 128, 0)]          # S, C, pipelined: both forward kernels at k = 6


@pytest.mark.parametrize("S,C,pipe", SCHEDULES)
@pytest.mark.parametrize("zero", [0, 1])
def test_forward_ties_take_the_earliest_slot(dev, zero, S, C, pipe):
    assert fwd_plan(6, S, C) == (1, pipe)
    c = _tied_case(zero, S, C)
    rc, out, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    r = _ref_fwd(c)
    tied = (r.P[:, :, :3] == r.P[:, :, 3:]).all()
    assert tied and ((r.P == 0).all() if zero else (r.mx != 0).float().mean() > 0.5)
    rows = _rows16(arg)
    hit = c.idx.long()[:, :, :, None] == rows[:, :, None, :]
    slot = torch.where(hit, torch.arange(6)[None, None, :, None], 6).min(2).values
    first = torch.where(r.P == r.mx[:, :, None, :], torch.arange(6)[None, None, :, None], 6).min(2).values
    assert (slot < 3).all() and ((slot == 0).all() if zero else True)
    tol = A * U * r.Tm
    second = torch.where(r.P < r.mx[:, :, None, :], r.P, torch.full_like(r.P, -float("inf"))).max(2).values
    clear = (r.mx - second) > tol
    assert (slot[clear] == first[clear]).all()
    _hold(out, r.out, A * U * r.out_abs, "tied out")
    assert torch.equal(fwin.cpu(), torch.gather(c.fm[:, :, c.C:], 1, rows))


# ==== the column-tile scatter backward =============================================================================================

# B, N, S, C, tile width, row ranges, workgroup map, what the case is there for
TILES = [(8, 37, 8, 512, 64, 1, "cloud", "tile 64"), (9, 35, 8, 512, 64, 1, "group", "tile 64"),
         (4, 70, 8, 512, 32, 1, "group", "tile 32"), (8, 70, 4, 512, 32, 1, "cloud", "tile 32"),
         (3, 150, 3, 16, 16, 1, "plain", "tile 16"), (2, 257, 7, 64, 16, 1, "plain", "tile 16 (T % 4 == 0, groups % 8 != 0)"),
         (4, 131, 8, 16, 16, 1, "group", "tile 16"), (8, 130, 1, 16, 16, 1, "cloud", "tile 16"),
         (16, 40, 2, 16, 16, 1, "cloud", "tile 16, two clouds per XCD"),
         (1, 600, 2, 8, 8, 1, "plain", "tile 8"), (1, 2926, 1, 8, 8, 1, "plain", "tile 8, pass 1 (156 KB)"),
         (3, 530, 3, 4, 4, 1, "plain", "tile 4"), (1, 2926, 1, 4, 4, 1, "plain", "tile 4, pass 1"),
         (1, 4203, 1, 16, 4, 1, "plain", "tile 4, pass 1, past the half-cloud form"),
         (1, 1078, 1, 16, 16, 2, "plain", "half-cloud tiles, the smallest N"), (2, 1079, 2, 16, 16, 2, "plain", "half-cloud tiles, the smallest odd N"),
         (1, 4202, 1, 16, 16, 2, "plain", "half-cloud tiles, the largest N"), (8, 1079, 1, 16, 16, 2, "cloud", "half-cloud tiles")]
TILE_IDS = [f"B{t[0]}-N{t[1]}-S{t[2]}-C{t[3]}" for t in TILES]


def _wg_map(B, T):
    """how rf_bwd_tile_kernel maps its grid (T column tiles, B clouds) to (cloud, tile): every tile of a cloud on one XCD when
    B % 8 == 0, groups of four adjacent tiles per XCD when they divide evenly, else the plain order"""
    if B % 8 == 0:
        return "cloud"
    return "group" if T % 4 == 0 and ((T // 4) * B) % 8 == 0 else "plain"


def _lds_pass1(N, tc):
    return (N * tc + 3 * N) * 4 > 80 * 1024


@pytest.mark.parametrize("B,N,S,C,tc,rs,wgmap,why", TILES, ids=TILE_IDS)
def test_scatter_backward(dev, B, N, S, C, tc, rs, wgmap, why):
    assert bwd_plan(B, N, S, C) == (tc, rs), why
    assert _wg_map(B, S * C // tc) == wgmap
    assert ("pass 1" in why) == (rs == 1 and _lds_pass1(N, tc))
    c = _case(B, N, 4, S, C, 2000 + B + N + C)
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    rows = _rows16(arg)
    g = _grad(c, 2100 + N)
    rc, gfm, gd = _run_scatter(c, arg, g, dev, fwin)
    assert rc == 0
    _check_bwd(c, rows, g, gfm, gd, True, why)
    rc, gfm2, gd2 = _run_scatter(c, arg, g, dev, use_fwin=False)          # support values gathered from fm: the same integers
    assert rc == 0 and torch.equal(gfm, gfm2)
    _check_bwd(c, rows, g, None, gd2, True, why + " (fm gather)")


def test_half_cloud_form_limits():
    """two half-cloud tiles of 16 columns from the first N whose whole-cloud tile is narrower than 16, while a half fits 156 KB"""
    for C in (16, 64):
        assert [bwd_plan(1, N, 1, C) for N in (1077, 1078, 4202, 4203)] == [(16, 1), (16, 2), (16, 2), (4, 1)]
    assert bwd_plan(1, 2000, 1, 8) == (4, 1) and bwd_plan(1, 2000, 1, 24) == (4, 1)          # C % 16 != 0: never


@pytest.mark.parametrize("B,N,S,C,tc,rs,wgmap,why", [TILES[4], TILES[9], TILES[15]], ids=[TILE_IDS[4], TILE_IDS[9], TILE_IDS[15]])
def test_scatter_backward_bf16(dev, B, N, S, C, tc, rs, wgmap, why):
    assert bwd_plan(B, N, S, C) == (tc, rs)
    c = _case(B, N, 4, S, C, 2200 + N, dtype=BF)
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    g = _grad(c, 2300 + N)
    rc, gfm, gd = _run_scatter(c, arg, g, dev, fwin)
    assert rc == 0
    _check_bwd(c, _rows16(arg), g, gfm, gd, True, "bf16 " + why)


@pytest.mark.parametrize("B,N,S,C,tc", [(2, 150, 3, 16, 16), (8, 150, 2, 8, 8), (3, 530, 2, 4, 4)])
def test_surface_backward(dev, B, N, S, C, tc):
    assert bwd_plan(B, N, S, C, 1) == (tc, 1)
    c = _case(B, N, 5, S, C, 2400 + N, surface=True)
    rc, _, arg, _ = _run_fwd(c, dev)
    assert rc == 0
    g = _grad(c, 2500 + N)
    rc, _, gd = _run_scatter(c, arg, g, dev)
    assert rc == 0
    _check_bwd(c, _rows16(arg), g, None, gd, False, "surface")


# ==== the gather-form backward ======================================================================================================

@pytest.mark.parametrize("B,N,k,S,C,nch", [(3, 41, 6, 3, 64, 1), (1, 33, 6, 3, 512, 2), (2, 33, 5, 5, 512, 3), (1, 33, 5, 7, 512, 4)])
def test_csr_backward(dev, B, N, k, S, C, nch):
    assert fwd_plan(k, S, C)[0] == nch                                    # (the gather form has the forward's column slots)
    c = _case(B, N, k, S, C, 3000 + N + C)
    rc, _, arg, _ = _run_fwd(c, dev)
    assert rc == 0
    g = _grad(c, 3100 + N)
    rc, gfm, gd = _run_csr(c, arg, g, dev)
    assert rc == 0
    _check_bwd(c, _rows16(arg), g, gfm, gd, False, "csr")
    rc, gfm2, gd2 = _run_csr(c, arg, g, dev)
    assert rc == 0 and torch.equal(gfm, gfm2) and torch.equal(gd, gd2)    # fixed summation order


def test_csr_backward_in_degrees_and_hub(dev):
    """in-degree 0, 8 (one full batch of staged edges), 9 (one more) and a hub that every point lists"""
    B, N, k, S, C = 3, 40, 4, 3, 64
    c = _case(B, N, k, S, C, 3200)
    i = torch.arange(N)
    idx = torch.stack([torch.zeros(N, dtype=torch.long), 1 + (i % 8) // 8, 3 + i % 30, 3 + (i + 7) % 30], 1)   # hub 0; rows 3 ... 32
    idx[:8, 1] = 1                                                        # row 1: listed by points 0 ... 7 (in-degree 8)
    idx[8:, 1] = 2
    idx[17:, 1] = 33 + i[17:] % 6                                         # row 2: points 8 ... 16 (in-degree 9); rows 39: in-degree 0
    c.idx = idx.to(torch.int32)[None].expand(B, N, k).contiguous()
    deg = torch.bincount(c.idx[0].flatten().long(), minlength=N)
    assert deg[0] == N and deg[1] == 8 and deg[2] == 9 and deg[39] == 0
    assert all(len(set(r.tolist())) == k for r in c.idx[0])
    rc, out, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    rows = _check_fwd(c, out, arg, fwin)
    g = _grad(c, 3300)
    rc, gfm, gd = _run_csr(c, arg, g, dev)
    assert rc == 0
    _check_bwd(c, rows, g, gfm, gd, False, "csr hub")
    assert (gfm[:, 39, C:] == 0).all()
    rc, gfm, gd = _run_scatter(c, arg, g, dev, fwin)
    assert rc == 0
    _check_bwd(c, rows, g, gfm, gd, True, "scatter hub")


# ==== the fixed-point accumulator ===================================================================================================

def _fx_case(N=150, seed=4000):
    c = _case(2, N, 6, 2, 192, seed + N)
    assert bwd_plan(2, N, 2, 192) == (16, 1)
    return c


def _fx_run(c, g, dev, what, check=True):
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    rc, gfm, gd = _run_scatter(c, arg, g, dev, fwin)
    assert rc == 0
    rows = _rows16(arg)
    return rows, gfm, gd, (_check_bwd(c, rows, g, gfm, gd, True, what) if check else None)


@pytest.mark.parametrize("scales", [(1.0, 2.0 ** -20, 2.0 ** 20), (2.0 ** 20, 0.0, 1.0), (1e-30, 1.0, 1e30)])
def test_fixed_point_blocks_keep_their_own_bound(dev, scales):
    """magnitudes that differ by 2^40 (or vanish) on neighbouring 64-channel blocks: every block is held to its OWN quantum"""
    c = _fx_case()
    g = _grad(c, 4100)
    for blk, s in enumerate(scales):
        g[:, :, 64 * blk:64 * (blk + 1)] *= s
    rows, gfm, gd, r = _fx_run(c, g, dev, f"blocks {scales}")
    if 0.0 in scales:
        blk = scales.index(0.0)
        sup = gfm[:, :, c.C:].view(2, c.N, 2, 192)[..., 64 * blk:64 * (blk + 1)]
        assert (sup == 0).all()


def test_fixed_point_outlier_inside_a_tile(dev):
    """one point's gradient 2^12 above the rest of its tile: the rest is held to the bound the outlier sets, not a looser one"""
    c = _fx_case()
    g = _grad(c, 4200)
    g[0, 77, 0:16] *= 2.0 ** 12
    _fx_run(c, g, dev, "outlier")


@pytest.mark.parametrize("N,scale,emin", [(150, 1.0, 0), (12, 1e-30, 124)])
def test_fixed_point_cells_are_multiples_of_the_tile_quantum(dev, N, scale, emin):
    """the documented quantum, exactly: a support cell is an integer times q = 2^(ex + ceil(log2 N) - 30), ex from the TILE's own
    max|g|/S, and not always an even one.  Neither N is a power of two, so a floor(log2 N) would leave odd multiples of q / 2.
    Gradients of 1e-30 on 12 points put the scale 1/q at 2^124 and above: an exponent clamped below that leaves every cell a
    multiple of 16 q"""
    c = _fx_case(N)
    g = _grad(c, 4300, scale)
    rows, gfm, gd, _ = _fx_run(c, g, dev, "quantum")
    tc = 16
    gm = (g.double().abs().amax(1) / c.S).view(2, 192 // tc, tc).amax(2)                 # (B, tiles per support)
    e = 30 - torch.frexp(gm).exponent.double() - (c.N - 1).bit_length()
    assert emin <= e.min() and e.max() <= 126                                            # (2^126: the last scale the kernel keeps)
    sup = gfm.cpu()[:, :, c.C:].double().view(2, c.N, c.S, 192 // tc, tc)
    m = sup * 2.0 ** e[:, None, None, :, None]
    assert (m == m.round()).all()
    odd = (m % 2 == 1).flatten(3).any(3).any(1).any(1)                                   # (B, tiles): per tile
    assert odd.all(), "every cell of a tile is a multiple of twice its quantum: the scale is coarser than documented"


def test_fixed_point_zero_gradient(dev):
    c = _fx_case()
    g = torch.zeros(2, c.N, 192)
    rows, gfm, gd, _ = _fx_run(c, g, dev, "zero", check=False)
    assert (gfm == 0).all() and (gd == 0).all()


@pytest.mark.parametrize("N", [128, 129, 1024, 1025])
def test_fixed_point_hub_cannot_overflow(dev, N):
    """a hub row wins every column for every point, at the tile's largest |g| and theta ~ 1: the largest sum a cell can hold"""
    B, S, C = 1, 1, 16
    c = _case(B, N, 4, S, C, 4400 + N)
    assert bwd_plan(B, N, S, C) == (16, 1)
    c.xyz[0, 0] = torch.tensor([60.0, 0.0, 0.0])
    c.dirs = torch.tensor([1.0, 0.0, 0.0])[:, None] + 0.02 * c.dirs       # theta > 0.999
    rows = torch.zeros(B, N, S * C, dtype=torch.int64)
    arg = rows.to(torch.int16).to(dev)
    fwin = torch.gather(c.fm[:, :, C:], 1, rows).to(dev)
    g = torch.full((B, N, C), float(np.nextafter(np.float32(2.0), np.float32(0.0))))    # max|g|/S just below 2^ex
    rc, gfm, gd = _run_scatter(c, arg, g, dev, fwin)
    assert rc == 0
    r = _check_bwd(c, rows, g, gfm, gd, True, f"hub N={N}")
    assert (r.sup[0, 0] > 1.99 * (N - 1)).all()


def test_nan_gradient_is_confined(dev):
    """include/hsp.h: the centre column carries the NaN; every cell the element does not feed is finite and correct"""
    c = _fx_case()
    g = _grad(c, 4500)
    b0, i0, c0 = 1, 33, 70
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    rows = _rows16(arg)
    gn = g.clone()
    gn[b0, i0, c0] = NAN
    rc, gfm, gd = _run_scatter(c, arg, gn, dev, fwin)
    assert rc == 0
    gfm, gd = gfm.cpu(), gd.cpu()
    assert torch.isnan(gfm[b0, i0, c0])
    g0 = g.clone()
    g0[b0, i0, c0] = 0.0
    fed = [(int(rows[b0, i0, s * c.C + c0]), s * c.C + c0) for s in range(c.S)]
    centre = gfm[:, :, :c.C].clone()
    centre[b0, i0, c0] = 0.0
    sup = gfm[:, :, c.C:].clone()
    for m, j in fed:
        sup[b0, m, j] = 0.0                                               # (unspecified: taken out of the comparison ...)
        gd[:, j] = 0.0
    r = _ref_bwd(c, rows, g0)
    for m, j in fed:                                                      # (... on both sides)
        r.sup[b0, m, j] = 0.0
        r.gD[:, j] = 0.0
    assert torch.equal(centre, g0)
    _hold(sup, r.sup, A * U * r.sup_abs + r.cnt * _quantum(g0, c.S, c.N, c.S * c.C) / 2, "grad_fm beside a NaN")
    _hold(gd, r.gD, A * U * r.gD_abs + r.gD_marg, "grad_dirs beside a NaN")


# ==== geometry and directions ========================================================================================================

@pytest.mark.parametrize("S,C,pipe", SCHEDULES)
def test_degenerate_geometry_and_directions(dev, S, C, pipe):
    """a coincident neighbour (zero direction), the point itself in its list, direction columns of norm 0, 1e-20 and 1e6"""
    B, N, k = 2, 60, 6
    assert fwd_plan(k, S, C) == (1, pipe)
    c = _case(B, N, k, S, C, 5000)
    c.xyz[:, 1::2] = c.xyz[:, 0::2]                                       # rows 2t and 2t+1 coincide
    i = torch.arange(N)
    c.idx[:, :, 0] = (i ^ 1).to(torch.int32)                              # slot 0: the coincident twin
    c.idx[:, :, 1] = i.to(torch.int32)                                    # slot 1: the point itself
    c.idx[:, :, 2:] = ((i[:, None] + torch.tensor([2, 4, 6, 8])[None, :] + (i[:, None] % 2)) % N).to(torch.int32)
    assert all(len(set(r.tolist())) == k for r in c.idx[0])
    c.dirs[:, 0] = 0.0
    c.dirs[:, 1] *= 1e-20 / c.dirs[:, 1].norm()
    c.dirs[:, 2] *= 1e6 / c.dirs[:, 2].norm()
    rc, out, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    rows = _check_fwd(c, out, arg, fwin)
    assert (rows[:, :, 0] == c.idx[:, :, 0].long()).all()                 # a zero direction column: all products +-0, slot 0 wins
    g = _grad(c, 5100)
    for what, (rc, gfm, gd) in (("scatter", _run_scatter(c, arg, g, dev, fwin)), ("csr", _run_csr(c, arg, g, dev))):
        assert rc == 0
        _check_bwd(c, rows, g, gfm, gd, what == "scatter", "degenerate " + what)
        assert (gd[:, 0] == 0).all()


# ==== declines =======================================================================================================================

def test_rf_declines_leave_outputs_untouched(dev):
    buf = torch.zeros(4 << 20, dtype=torch.int32, device=dev)            # every input points here: zeros are valid rows and values
    one = _vp(buf)

    def fwd(N, k, S, C, want):                                            # (no buffer is read: the call returns before any launch)
        out = torch.full((64,), NAN, device=dev)
        arg = _u16((64,), dev)
        rc = _L().hsp_rf_conv_fwd(one, one, one, one, 1, N, k, S, C, _vp(out), _vp(arg), None, _stream())
        torch.cuda.synchronize()
        assert rc == want and torch.isnan(out).all() and (arg == -1).all(), (N, k, S, C)

    assert fwd_plan(8, 5, 1024) == (0, 0) and fwd_plan(8, 7, 126) == (0, 0) and fwd_plan(3300, 1, 4) == (0, 0)
    fwd(8, 8, 5, 1024, UNSUPPORTED)                                       # S*C > 4096
    fwd(8, 4, 7, 126, UNSUPPORTED)                                        # C % 4
    fwd(8, 3300, 1, 4, UNSUPPORTED)                                       # (S*C + 5 k) floats of LDS
    fwd(65536, 4, 1, 4, UNSUPPORTED)                                      # uint16 rows
    fwd(8, 0, 1, 4, BAD_ARG)
    # the tile backward: no tile fits
    assert bwd_plan(1, 5706, 1, 4) == (0, 0) and bwd_plan(1, 5705, 1, 4) == (4, 1)
    gfm = torch.full((64,), NAN, device=dev)
    gd = torch.full((12,), NAN, device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    rc = _L().hsp_rf_conv_bwd_scatter(one, one, one, one, one, one, 1, 5706, 1, 4, _vp(gfm), _vp(gd), _vp(ws), 4096, _stream())
    assert rc == UNSUPPORTED
    rc = _L().hsp_rf_conv_bwd_scatter(one, one, one, one, one, one, 1, 64, 1, 4, _vp(gfm), _vp(gd), _vp(ws), 8, _stream())
    assert rc == WORKSPACE
    rc = _L().hsp_rf_conv_bwd(one, one, one, one, one, one, one, 1, 8, 4, 5, 1024, _vp(gfm), _vp(gd), _vp(ws), 1 << 30, _stream())
    assert rc == UNSUPPORTED                                              # S*C > 4096
    rc = _L().hsp_rf_conv_bwd(one, one, one, one, one, one, one, 1, 8, 4, 1, 2048, _vp(gfm), _vp(gd), _vp(ws), 1 << 30, _stream())
    assert rc == UNSUPPORTED                                              # 8 staged edges x (C + 8) floats > 64 KiB of LDS
    rc = _L().hsp_rf_conv_bwd(one, one, one, one, one, one, one, 1, 8, 4, 1, 64, _vp(gfm), _vp(gd), _vp(ws), 8, _stream())
    assert rc == WORKSPACE
    rc = _L().hsp_rf_conv_bwd(one, one, one, one, one, one, one, 1, 8, 4, 1, 64, _vp(gfm), None, _vp(ws), 1 << 30, _stream())
    assert rc == BAD_ARG
    # the surface layer
    out = torch.full((64,), NAN, device=dev)
    arg = _u16((64,), dev)
    for (N, k, S, C), want in (((8, 4, 7, 126), UNSUPPORTED), ((8, 4, 5, 1024), UNSUPPORTED), ((65536, 4, 1, 4), UNSUPPORTED),
                               ((8, 3300, 1, 4), UNSUPPORTED), ((0, 4, 1, 4), BAD_ARG)):
        assert _L().hsp_rf_surface_fwd(one, one, one, 1, N, k, S, C, _vp(out), _vp(arg), _stream()) == want, (N, k, S, C)
    for (N, S, C, wsb), want in (((8, 1, 6, 4096), UNSUPPORTED), ((65536, 1, 4, 4096), UNSUPPORTED), ((8, 1, 4, 8), WORKSPACE),
                                 ((8, 0, 4, 4096), BAD_ARG)):
        assert _L().hsp_rf_surface_bwd(one, one, one, one, 1, N, S, C, _vp(gd), _vp(ws), wsb, _stream()) == want, (N, S, C)
    torch.cuda.synchronize()
    assert torch.isnan(gfm).all() and torch.isnan(gd).all() and torch.isnan(out).all() and (arg == -1).all()


def test_gather_declines_leave_outputs_untouched(dev):
    buf = torch.zeros(1 << 20, dtype=torch.int32, device=dev)            # every input points here
    one = _vp(buf)
    gf = torch.full((4096,), NAN, device=dev)
    L = _L()
    # hsp_gather_max_bwd(grad_out, bcast, idx, qsel, argmax, B, Nsrc, Nidx, Nq, kstride, C, grad_feat, accumulate, extra, stream)
    assert L.hsp_gather_max_bwd(one, 0, one, None, one, 1, 8, 8, 8, 4, 6, _vp(gf), 0, None, _stream()) == UNSUPPORTED     # C % 4
    assert L.hsp_gather_max_bwd(one, 0, one, None, one, 1, 8, 8, 5, 4, 8, _vp(gf), 0, None, _stream()) == BAD_ARG         # Nq != Nidx, no qsel
    assert L.hsp_gather_max_bwd(one, 0, one, None, one, 1, 8, 8, 8, 0, 8, _vp(gf), 0, None, _stream()) == BAD_ARG         # kstride
    # hsp_orl_global_fwd(feat, idx, B, N, k, kstride, C, fg, argmax, ws, ws_bytes, stream)
    fg = torch.full((64,), NAN, device=dev)
    am = torch.full((4096,), 255, dtype=torch.uint8, device=dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    for sfx in ("", "_bf16"):
        f = getattr(L, "hsp_orl_global_fwd" + sfx)
        assert f(one, one, 1, 16, 4, 4, 20, _vp(fg), _vp(am), _vp(ws), 1 << 16, _stream()) == UNSUPPORTED                 # 256 % (C / 4)
        assert f(one, one, 1, 16, 4, 4, 18, _vp(fg), _vp(am), _vp(ws), 1 << 16, _stream()) == UNSUPPORTED                 # C % 4
        assert f(one, one, 1, 300, 256, 256, 16, _vp(fg), _vp(am), _vp(ws), 1 << 16, _stream()) == UNSUPPORTED            # k > 255
        assert L.hsp_orl_workspace_bytes(1, 16, 16) > 8
        assert f(one, one, 1, 16, 4, 4, 16, _vp(fg), _vp(am), _vp(ws), 8, _stream()) == WORKSPACE
        assert f(one, one, 1, 16, 4, 4, 16, _vp(fg), _vp(am), None, 0, _stream()) == WORKSPACE
        assert f(one, one, 1, 16, 4, 3, 16, _vp(fg), _vp(am), _vp(ws), 1 << 16, _stream()) == BAD_ARG                     # kstride < k
    torch.cuda.synchronize()
    assert torch.isnan(gf).all() and torch.isnan(fg).all() and (am == 255).all()


# ==== csrc/gather.hip: the column-tile scatter =====================================================================================

def _gm_case(B, Nsrc, Nq, k, kstride, C, seed, qsel=False, dtype=torch.float32):
    g = _gen(seed)
    Nidx = Nq + 5 if qsel else Nq
    feat = torch.randn(B, Nsrc, C, generator=g).to(dtype)
    idx = torch.randint(0, Nsrc, (B, Nidx, kstride), generator=g, dtype=torch.int32)
    sel = torch.randperm(Nidx, generator=g)[:Nq].to(torch.int32) if qsel else None
    return SimpleNamespace(B=B, Nsrc=Nsrc, Nq=Nq, Nidx=Nidx, k=k, kstride=kstride, C=C, feat=feat, idx=idx, qsel=sel, dtype=dtype)


def _gm_fwd(c, dev):
    out = torch.full((c.B, c.Nq, c.C), NAN, dtype=c.dtype, device=dev)
    am = torch.full((c.B, c.Nq, c.C), 255, dtype=torch.uint8, device=dev)
    feat, idx = c.feat.to(dev), c.idx.to(dev)
    sel = c.qsel.to(dev) if c.qsel is not None else None
    rc = getattr(_L(), "hsp_gather_max_fwd" + _sfx(c))(_vp(feat), _vp(idx), _vp(sel), c.B, c.Nsrc, c.Nidx, c.Nq, c.k, c.kstride, c.C,
                                                       _vp(out), _vp(am), _stream())
    torch.cuda.synchronize()
    return rc, out, am


def _gm_rows(c, am):
    """source row behind every (b, q, c): idx[b, qsel[q], argmax[b,q,c]]"""
    lists = c.idx.long() if c.qsel is None else c.idx.long()[:, c.qsel.long()]
    return torch.gather(lists, 2, am.cpu().long())


def _gm_check_fwd(c, out, am):
    lists = c.idx.long()[:, :, :c.k] if c.qsel is None else c.idx.long()[:, c.qsel.long(), :c.k]
    vals = _take(c.feat.double(), lists)                                  # (B,Nq,k,C)
    mx = vals.max(2).values
    first = torch.where(vals == mx[:, :, None, :], torch.arange(c.k)[None, None, :, None], c.k).min(2).values
    assert torch.equal(out.cpu().double(), mx) and torch.equal(am.cpu().long(), first)


def _gm_bwd(c, am, gout, bcast, dev, accumulate=0, extra=None, init=None):
    gf = (torch.full((c.B, c.Nsrc, c.C), NAN, dtype=c.dtype) if init is None else init.clone()).to(dev)
    idx = c.idx.to(dev)
    sel = c.qsel.to(dev) if c.qsel is not None else None
    go, ex = gout.to(dev), (extra.to(dev) if extra is not None else None)
    rc = getattr(_L(), "hsp_gather_max_bwd" + _sfx(c))(_vp(go), bcast, _vp(idx), _vp(sel), _vp(am), c.B, c.Nsrc, c.Nidx, c.Nq, c.kstride,
                                                       c.C, _vp(gf), accumulate, _vp(ex), _stream())
    torch.cuda.synchronize()
    return rc, gf


def _scatter64(c, rows, terms):
    z = torch.zeros(c.B, c.Nsrc, c.C, dtype=F64)
    return z.clone().scatter_add_(1, rows, terms.double()), z.clone().scatter_add_(1, rows, terms.double().abs())


# B, C, tile width, threads
SCATTER = [(1, 16, 16, 1024), (1, 8, 8, 1024), (3, 4, 4, 1024), (8, 512, 16, 512), (9, 512, 16, 256)]


@pytest.mark.parametrize("B,C,tc,nt", SCATTER)
@pytest.mark.parametrize("qsel,kstride", [(False, 5), (True, 5), (False, 9)])
def test_scatter_tile_mode0(dev, B, C, tc, nt, qsel, kstride):
    Nsrc, Nq, k = 23, 70, 5
    assert tile_plan(B, Nsrc, C) == (tc, nt)
    c = _gm_case(B, Nsrc, Nq, k, kstride, C, 7000 + B + C, qsel)
    rc, out, am = _gm_fwd(c, dev)
    assert rc == 0
    _gm_check_fwd(c, out, am)
    rows = _gm_rows(c, am)
    # a broadcast gradient: integer counts, fp32(g / N) * count bit for bit
    gb = torch.randn(B, C, generator=_gen(7100)) / Nq
    rc, gf = _gm_bwd(c, am, gb, 1, dev)
    assert rc == 0
    cnt = torch.zeros(B, Nsrc, C).scatter_add_(1, rows, torch.ones(B, Nq, C))
    assert torch.equal(gf.cpu(), gb[:, None, :] * cnt)
    # per-query gradients: float LDS adds in any order
    go = torch.randn(B, Nq, C, generator=_gen(7200))
    rc, gf = _gm_bwd(c, am, go, 0, dev)
    assert rc == 0
    want, terms = _scatter64(c, rows, go)
    _hold(gf, want, A * U * terms, "scatter tile", "scatter_tile", terms)


@pytest.mark.parametrize("accumulate,extra", [(1, False), (0, True), (1, True)])
@pytest.mark.parametrize("bcast", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_scatter_tile_fused_adds(dev, accumulate, extra, bcast, dtype):
    """accumulate / extra: the form the fused layer backward uses (ops._orl_bwd_accumulate_raw)"""
    B, Nsrc, Nq, k, C = 3, 23, 70, 5, 64
    c = _gm_case(B, Nsrc, Nq, k, k, C, 7300, dtype=dtype)
    rc, out, am = _gm_fwd(c, dev)
    assert rc == 0
    rows = _gm_rows(c, am)
    g = _gen(7400)
    old = torch.randn(B, Nsrc, C, generator=g).to(dtype)
    ex = torch.randn(B, Nsrc, C, generator=g).to(dtype) if extra else None
    if bcast:
        go = torch.randn(B, C, generator=g) / Nq
        per_q = go[:, None, :].expand(B, Nq, C)
    else:
        go = torch.randn(B, Nq, C, generator=g).to(dtype)
        per_q = go
    rc, gf = _gm_bwd(c, am, go, bcast, dev, accumulate, ex, init=old)
    assert rc == 0
    want, terms = _scatter64(c, rows, per_q)
    if accumulate:
        want, terms = want + old.double(), terms + old.double().abs()
    if extra:
        want, terms = want + ex.double(), terms + ex.double().abs()
    _hold(gf, want, A * U * terms + (2.0 ** -8 * want.abs() if dtype == BF else 0), f"fused adds acc={accumulate} extra={extra}")


@pytest.mark.parametrize("Nq", [1, 255, 256, 1024, 1025])              # 1, PL-1, PL, 4 PL, 4 PL + 1 at 16 columns on 1024 threads
def test_scatter_tile_query_counts(dev, Nq):
    B, Nsrc, k, C = 2, 19, 3, 16
    assert tile_plan(B, Nsrc, C) == (16, 1024)
    c = _gm_case(B, Nsrc, Nq, k, k, C, 7500 + Nq)
    rc, out, am = _gm_fwd(c, dev)
    assert rc == 0
    rows = _gm_rows(c, am)
    gb = torch.randn(B, C, generator=_gen(7600))
    rc, gf = _gm_bwd(c, am, gb, 1, dev)
    assert rc == 0
    cnt = torch.zeros(B, Nsrc, C).scatter_add_(1, rows, torch.ones(B, Nq, C))
    assert cnt.sum() == B * Nq * C and torch.equal(gf.cpu(), gb[:, None, :] * cnt)
    go = torch.randn(B, Nq, C, generator=_gen(7700))
    rc, gf = _gm_bwd(c, am, go, 0, dev)
    assert rc == 0
    want, terms = _scatter64(c, rows, go)
    _hold(gf, want, A * U * terms, f"Nq={Nq}", "scatter_tile", terms)


@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("B,C,tc,nt", SCATTER)
def test_scatter_tile_mode1_pitched_rows(dev, shared, B, C, tc, nt):
    """hsp_gather_rows_bwd on a column block of a wider tensor whose rows are only 8-byte aligned"""
    Nsrc, Nq, W, col0 = 23, 300, C + 6, 2
    assert tile_plan(B, Nsrc, C) == (tc, nt)
    g = _gen(7800 + B + C)
    wide = torch.randn(B, Nq, W, generator=g).to(dev)
    idx = torch.randint(0, Nsrc, (1 if shared else B, Nq), generator=g, dtype=torch.int32)
    block = wide[:, :, col0:col0 + C]
    assert block.data_ptr() % 16 == 8 and W % 4 == 2
    gf = torch.full((B, Nsrc, C), NAN, device=dev)
    idx_d = idx.to(dev)
    rc = _L().hsp_gather_rows_bwd(_vp(block), W, _vp(idx_d), shared, B, Nsrc, Nq, C, _vp(gf), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    rows = idx.long().expand(B, Nq)[:, :, None].expand(B, Nq, C)
    c = SimpleNamespace(B=B, Nsrc=Nsrc, C=C)
    want, terms = _scatter64(c, rows, block.cpu())
    _hold(gf, want, A * U * terms, "row scatter", "scatter_tile", terms)


def test_scatter_global_atomic_fallback_and_declines(dev):
    """no tile fits (Nsrc * 4 columns * 4 bytes > 144 KiB): fp32 falls back to memset + global atomics; `extra` and bf16 decline"""
    B, Nsrc, Nq, k, C = 1, 9217, 50, 3, 4
    assert tile_plan(B, Nsrc, C) == (0, 0) and tile_plan(B, 9216, C) == (4, 1024)
    c = _gm_case(B, Nsrc, Nq, k, k, C, 7900)
    rc, out, am = _gm_fwd(c, dev)
    assert rc == 0
    rows = _gm_rows(c, am)
    go = torch.randn(B, Nq, C, generator=_gen(7901))
    want, terms = _scatter64(c, rows, go)
    rc, gf = _gm_bwd(c, am, go, 0, dev)
    assert rc == 0
    _hold(gf, want, A * U * terms, "global atomics")
    old = torch.randn(B, Nsrc, C, generator=_gen(7902))
    rc, gf = _gm_bwd(c, am, go, 0, dev, accumulate=1, init=old)
    assert rc == 0
    _hold(gf, want + old.double(), A * U * (terms + old.double().abs()), "global atomics, accumulate")
    gb = torch.randn(B, C, generator=_gen(7903))
    rc, gf = _gm_bwd(c, am, gb, 1, dev)
    assert rc == 0
    w2, t2 = _scatter64(c, rows, gb[:, None, :].expand(B, Nq, C))
    _hold(gf, w2, A * U * t2, "global atomics, broadcast")
    rc, gf = _gm_bwd(c, am, go, 0, dev, extra=old)
    assert rc == UNSUPPORTED and torch.isnan(gf).all()
    cb = SimpleNamespace(**{**vars(c), "dtype": BF})
    rc, gf = _gm_bwd(cb, am, go.bfloat16(), 0, dev)
    assert rc == UNSUPPORTED and torch.isnan(gf.float()).all()
    # the row scatter's fallback (C % 4 != 0): global atomics as well
    idx = torch.randint(0, 23, (2, 40), generator=_gen(7904), dtype=torch.int32)
    go = torch.randn(2, 40, 6, generator=_gen(7905))
    gf = torch.full((2, 23, 6), NAN, device=dev)
    go_d, idx_d = go.to(dev), idx.to(dev)
    rc = _L().hsp_gather_rows_bwd(_vp(go_d), 6, _vp(idx_d), 0, 2, 23, 40, 6, _vp(gf), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    want, terms = _scatter64(SimpleNamespace(B=2, Nsrc=23, C=6), idx.long()[:, :, None].expand(2, 40, 6), go)
    _hold(gf, want, A * U * terms, "row scatter fallback")


@pytest.mark.parametrize("k,want", [(1, 0), (255, 0), (256, UNSUPPORTED)])
def test_gather_max_forward_k_limits(dev, k, want):
    """the arg-max is a byte: k = 255 is the last supported, 256 declines and leaves the outputs alone"""
    c = _gm_case(2, 300, 20, k, k, 16, 8000 + k)
    rc, out, am = _gm_fwd(c, dev)
    assert rc == want
    if want:
        assert torch.isnan(out).all() and (am == 255).all()
    else:
        _gm_check_fwd(c, out, am)


def test_gather_max_forward_ties_zeros_and_minus_infinity(dev):
    c = _gm_case(2, 12, 30, 6, 6, 16, 8100)
    c.feat[:, :4] = 0.0
    c.feat[:, 1, :] = -0.0                                                # +-0 compare equal: the earliest slot
    c.feat[:, 4:8] = c.feat[:, 8:12]                                      # equal nonzero values under different rows
    c.feat[0, :, 3] = -float("inf")                                       # a column of -inf only: slot 0, value -inf
    rc, out, am = _gm_fwd(c, dev)
    assert rc == 0
    _gm_check_fwd(c, out, am)
    assert (out[0, :, 3] == -float("inf")).all() and (am[0, :, 3] == 0).all()


# ==== csrc/gather.hip: the ORL global feature and the max over points ===============================================================

@pytest.mark.parametrize("B,N,k,kstride,C,dtype,slab", [(2, 130, 20, 20, 64, torch.float32, 1), (2, 130, 20, 20, 64, BF, 1),
                                                         (3, 130, 7, 9, 64, torch.float32, 0), (2, 100, 20, 20, 64, BF, 0),
                                                         (2, 128, 20, 20, 64, torch.float32, 1), (2, 127, 20, 20, 64, torch.float32, 0)])
def test_orl_forward_and_backward(dev, B, N, k, kstride, C, dtype, slab):
    """fg = mean_i max_n feat[idx[i,n]] and its backward, d fg / N broadcast over the points through the arg-max, in the form the
    fused layer backward uses (accumulate into the layer's gradient, plus an extra tensor) and alone"""
    c = _gm_case(B, N, N, k, kstride, C, 8200 + N + k, dtype=dtype)
    feat, idx = c.feat.to(dev), c.idx.to(dev)
    wsb = _L().hsp_orl_workspace_bytes(B, N, C)
    ws = torch.full((max(wsb, 16),), 0xA5, dtype=torch.uint8, device=dev)
    fg = torch.full((B, C), NAN, device=dev)
    am = torch.full((B, N, C), 255, dtype=torch.uint8, device=dev)
    rc = getattr(_L(), "hsp_orl_global_fwd" + _sfx(c))(_vp(feat), _vp(idx), B, N, k, kstride, C, _vp(fg), _vp(am), _vp(ws), wsb, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    # which form ran: the slab kernel writes fg itself, the chunked form leaves its per-chunk partials in the workspace
    assert wsb >= 16 and bool((ws[:wsb] == 0xA5).all()) == bool(slab)
    vals = _take(c.feat.double(), c.idx.long()[:, :, :k])
    mx = vals.max(2).values
    first = torch.where(vals == mx[:, :, None, :], torch.arange(k)[None, None, :, None], k).min(2).values
    assert torch.equal(am.cpu().long(), first)
    _hold(fg, mx.sum(1) / N, A * U * mx.abs().sum(1) / N, "fg", "orl fg", mx.abs().sum(1) / N)
    rows = _gm_rows(c, am)
    cnt = torch.zeros(B, N, C).scatter_add_(1, rows, torch.ones(B, N, C))
    gb = torch.randn(B, C, generator=_gen(8300)) / N
    rc, gf = _gm_bwd(c, am, gb, 1, dev)
    assert rc == 0
    want = gb[:, None, :] * cnt
    assert torch.equal(gf.cpu(), want.to(dtype))
    g = _gen(8400)
    old, ex = torch.randn(B, N, C, generator=g).to(dtype), torch.randn(B, N, C, generator=g).to(dtype)
    rc, gf = _gm_bwd(c, am, gb, 1, dev, 1, ex, init=old)
    assert rc == 0
    w64 = want.double() + old.double() + ex.double()
    t64 = want.double().abs() + old.double().abs() + ex.double().abs()
    _hold(gf, w64, A * U * t64 + (2.0 ** -8 * w64.abs() if dtype == BF else 0), "orl backward, accumulate + extra")


def _points_max_ref(x):
    """(B,N,C) -> value and FIRST row: a NaN wins (torch.max), the first of them; else the first row holding the maximum"""
    x = x.double()
    N = x.shape[1]
    nan = torch.isnan(x)
    has = nan.any(1)
    mx = torch.where(nan, torch.full_like(x, -float("inf")), x).max(1).values
    rows = torch.arange(N)[None, :, None]
    first = torch.where(x == mx[:, None, :], rows, N).min(1).values
    first_nan = torch.where(nan, rows, N).min(1).values
    return torch.where(has, torch.full_like(mx, NAN), mx), torch.where(has, first_nan, first)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_points_max_every_row_count(dev, dtype):
    """N = 1 ... 65 (the four-rows-in-flight loop, its tail, the 16 row groups), C no multiple of 64, ties, NaN, all -inf"""
    B, C = 2, 72
    sfx = "_bf16" if dtype == BF else ""
    for N in range(1, 66):
        g = _gen(8500 + N)
        x = torch.randint(-3, 4, (B, N, C), generator=g).to(dtype)        # few distinct values: ties in every column
        x[:, :, 5] = -float("inf")
        x[0, N // 2, 6] = NAN
        x[1, :, 7] = NAN
        if N > 1:
            x[1, N - 1, 8] = NAN
            x[1, 0, 8] = float("inf")
        xd = x.to(dev)
        out = torch.full((B, C), 7.0, device=dev)
        arg = torch.full((B, C), -1, dtype=torch.int32, device=dev)
        rc = getattr(_L(), "hsp_points_max_fwd" + sfx)(_vp(xd), B, N, C, _vp(out), _vp(arg), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        wv, wa = _points_max_ref(x)
        got = out.cpu().double()
        assert torch.equal(torch.isnan(got), torch.isnan(wv)) and torch.equal(got.nan_to_num(7.0), wv.nan_to_num(7.0)), N
        assert torch.equal(arg.cpu().long(), wa), N
        go = torch.randn(B, C, generator=g)
        gx = torch.full((B, N, C), NAN, dtype=dtype, device=dev)
        go_d = go.to(dev)
        rc = getattr(_L(), "hsp_points_max_bwd" + sfx)(_vp(go_d), _vp(arg), B, N, C, _vp(gx), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        want = torch.zeros(B, N, C).scatter_(1, wa[:, None, :], go[:, None, :]).to(dtype)
        assert torch.equal(gx.cpu(), want), N
    out = torch.full((B, 70), 7.0, device=dev)
    arg = torch.full((B, 70), -1, dtype=torch.int32, device=dev)
    x = torch.randn(B, 9, 70, generator=_gen(8600)).to(dtype)            # C % 4 != 0: the forward takes it, the backward declines
    xd = x.to(dev)
    assert getattr(_L(), "hsp_points_max_fwd" + sfx)(_vp(xd), B, 9, 70, _vp(out), _vp(arg), _stream()) == 0
    torch.cuda.synchronize()
    wv, wa = _points_max_ref(x)
    assert torch.equal(out.cpu().double(), wv) and torch.equal(arg.cpu().long(), wa)
    gx = torch.full((B, 9, 70), NAN, dtype=dtype, device=dev)
    assert getattr(_L(), "hsp_points_max_bwd" + sfx)(_vp(out), _vp(arg), B, 9, 70, _vp(gx), _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(gx.float()).all()


@pytest.mark.parametrize("k,want", [(1, 0), (255, 0), (256, UNSUPPORTED)])
def test_pool_layer_forward(dev, k, want):
    """hsp_pool_fwd: the kept rows' neighbourhood max and their coordinates in one launch"""
    B, N, Nq, C = 2, 300, 40, 16
    c = _gm_case(B, N, Nq, k, k, C, 8700 + k, qsel=True)
    c.idx = torch.randint(0, N, (B, N, k), generator=_gen(8701), dtype=torch.int32)
    c.Nidx = N
    c.qsel = torch.randperm(N, generator=_gen(8702))[:Nq].to(torch.int32)
    xyz = torch.randn(B, N, 3, generator=_gen(8703))
    feat, idx, sel, xd = c.feat.to(dev), c.idx.to(dev), c.qsel.to(dev), xyz.to(dev)
    out = torch.full((B, Nq, C), NAN, device=dev)
    am = torch.full((B, Nq, C), 255, dtype=torch.uint8, device=dev)
    xs = torch.full((B, Nq, 3), NAN, device=dev)
    rc = _L().hsp_pool_fwd(_vp(feat), _vp(xd), _vp(idx), _vp(sel), B, N, Nq, k, k, C, _vp(out), _vp(am), _vp(xs), _stream())
    torch.cuda.synchronize()
    assert rc == want
    if want:
        assert torch.isnan(out).all() and (am == 255).all() and torch.isnan(xs).all()
    else:
        _gm_check_fwd(c, out, am)
        assert torch.equal(xs.cpu(), xyz[:, c.qsel.long()])


def test_zz_measured_ratios():
    """prints the worst ratios of this run (pytest -s): the table of the docstring and of DESIGN.md"""
    for k in sorted(RATIOS):
        print(f"  {k:28s} {RATIOS[k]:.3f}")
