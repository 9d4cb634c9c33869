"""GPU: the two schedules of rf_bwd_tile_kernel (csrc/rfconv.hip; hsp_rf_bwd_set_schedule) compute the same bits.

The batched schedule (the default) issues a workgroup's set-up loads as register batches, keeps the scale pass's grad_out rows in
registers where ceil(N / PL) <= RG (PL = 512 / (TC / 4) point lanes), sweeps with a register ring D stages deep and spreads the
centre-column copy over all tiles of a cloud; the legacy schedule is the first form of the kernel.  The tile sums are integers
and each thread keeps its point order, so grad_fm and the direction gradient must be torch.equal between the two -- and the new
schedule is held to the fp64 reference of tests/test_gpu_rf_reference.py at the sizes where its ring wraps.

Sizes follow the kernel's own constants (RfSched in csrc/rfconv.hip), restated here:

    plan                      PL    RG (resident rows)   D resident / streamed
    TC = 16                   128   9 (every N it plans)  3 / -
    TC = 32                    64   5                     1 / 1
    TC = 64                    32   2                     2 / 1
    TC = 8, TC = 4        256, 512  -                     - / 3
    half-cloud form (RS = 2)  128   -                     - / 4
    surface (TC = 16)         128   -                     - / 2

Every case asserts the plan it enters and restores the switch in a finally.
"""
import contextlib

import pytest
import torch

from test_gpu_rf_reference import BF, NAN, _L, _case, _check_bwd, _grad, _rows16, _run_fwd, _run_scatter, _stream, _vp, bwd_plan

pytestmark = pytest.mark.gpu

BAD_ARG = -1
D16, D64, D32, DSURF = 3, 2, 1, 2


@contextlib.contextmanager
def schedule(legacy):
    prev = _L().hsp_rf_bwd_set_schedule(legacy)
    assert prev in (0, 1)
    try:
        yield
    finally:
        _L().hsp_rf_bwd_set_schedule(prev)


def _both(c, arg, g, dev, fwin=None, use_fwin=True):
    """(grad_fm, grad_dirs) under the legacy and under the batched schedule"""
    out = []
    for legacy in (1, 0):
        with schedule(legacy):
            rc, gfm, gd = _run_scatter(c, arg, g, dev, fwin, use_fwin)
        assert rc == 0
        out.append((gfm, gd))
    return out


def _same(c, g, dev, what):
    """legacy == batched, bit for bit, with the fwin stream and gathering from fm; returns what the batched schedule gave with fwin"""
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    (gfm_l, gd_l), (gfm_n, gd_n) = _both(c, arg, g, dev, fwin)
    assert torch.equal(gd_l, gd_n), f"{what}: direction gradient differs between the schedules"
    if not c.surface:
        assert torch.equal(gfm_l, gfm_n), f"{what}: grad_fm differs between the schedules"
        (gfm_l2, gd_l2), (gfm_n2, gd_n2) = _both(c, arg, g, dev, use_fwin=False)
        assert torch.equal(gfm_l2, gfm_n2) and torch.equal(gd_l2, gd_n2), f"{what}: (fm gather) the schedules differ"
        assert torch.equal(gfm_n, gfm_n2), f"{what}: the fm gather changes the integers"
    return arg, gfm_n, gd_n


# ==== bit-equality of the two schedules ============================================================================================

# B, N, S, C, tile width, row ranges, why
CONV = ([(2, N, 2, 16, 16, 1, why) for N, why in (
            (5, "one partial iteration"), (127, "one partial iteration"), (128, "exactly one"), (129, "one more than a multiple"),
            (128 * D16 - 1, "the ring's wrap"), (128 * D16, "the ring's wrap"), (128 * D16 + 1, "the ring's wrap"),
            (128 * (D16 + 1) + 4, "a four-lane tail"), (1028, "the benchmark's count with its four-lane tail"))]
        + [(8, 37, 8, 512, 64, 1, "tile 64, resident"), (8, 64, 8, 512, 64, 1, "tile 64, exactly the resident rows"),
           (8, 32 * D64 + 1, 8, 512, 64, 1, "tile 64, one row past the resident bound: grad_out in the ring")]
        + [(4, 70, 8, 512, 32, 1, "tile 32"), (4, 64 * D32 + 1, 8, 512, 32, 1, "tile 32, the ring's wrap"),
           (4, 320, 8, 512, 32, 1, "tile 32, exactly the resident rows"), (4, 321, 8, 512, 32, 1, "tile 32, grad_out in the ring")]
        + [(1, 600, 2, 8, 8, 1, "tile 8"), (3, 530, 3, 4, 4, 1, "tile 4"),
           (1, 1078, 1, 16, 16, 2, "half-cloud tiles"), (2, 1079, 2, 16, 16, 2, "half-cloud tiles, odd N")])
CONV_IDS = [f"B{t[0]}-N{t[1]}-S{t[2]}-C{t[3]}" for t in CONV]
HALF = [t for t in CONV if t[5] == 2]


@pytest.mark.parametrize("B,N,S,C,tc,rs,why", CONV, ids=CONV_IDS)
def test_schedules_agree(dev, B, N, S, C, tc, rs, why):
    assert bwd_plan(B, N, S, C) == (tc, rs), why
    c = _case(B, N, min(4, N - 1), S, C, 7000 + B + N + C)
    _same(c, _grad(c, 7100 + N), dev, why)


@pytest.mark.parametrize("B,N,S,C,tc,rs,why", HALF, ids=[f"B{t[0]}-N{t[1]}" for t in HALF])
def test_schedules_agree_bf16_half_cloud(dev, B, N, S, C, tc, rs, why):
    assert bwd_plan(B, N, S, C) == (tc, rs), why
    c = _case(B, N, 4, S, C, 7200 + N, dtype=BF)
    _same(c, _grad(c, 7300 + N), dev, "bf16 " + why)


@pytest.mark.parametrize("N", [129, 128 * D16 + 1])
def test_schedules_agree_bf16_rows(dev, N):
    assert bwd_plan(2, N, 2, 16) == (16, 1)
    c = _case(2, N, 4, 2, 16, 7400 + N, dtype=BF)
    _same(c, _grad(c, 7500 + N), dev, "bf16 tile 16")


@pytest.mark.parametrize("N", [150, 128 * DSURF + 1])
def test_schedules_agree_surface(dev, N):
    B, S, C = 2, 3, 16
    assert bwd_plan(B, N, S, C, 1) == (16, 1)
    c = _case(B, N, 5, S, C, 7600 + N, surface=True)
    _same(c, _grad(c, 7700 + N), dev, "surface")


# ==== gradients that stress the scale pass =========================================================================================

def _stress(kind, c):
    g = _grad(c, 7800 + c.N)
    if kind == "zero":
        g.zero_()
    elif kind == "column":
        g[:, :, 5] *= 2.0 ** 40
    elif kind == "last row":
        g[1, c.N - 1, 9] *= 2.0 ** 40          # row N - 1: the lone row of the last partial batch
    return g


@pytest.mark.parametrize("kind", ["zero", "column", "last row"])
@pytest.mark.parametrize("N", [129, 128 * D16 + 1])
def test_scale_pass_sees_every_row(dev, N, kind):
    assert bwd_plan(2, N, 2, 16) == (16, 1)
    c = _case(2, N, 4, 2, 16, 7900 + N)
    g = _stress(kind, c)
    arg, gfm, gd = _same(c, g, dev, kind)
    if kind == "zero":
        assert (gfm == 0).all() and (gd == 0).all()
    else:                                        # (a scale chosen without the outlier would overflow or round the rest away)
        _check_bwd(c, _rows16(arg), g, gfm, gd, True, kind)


@pytest.mark.parametrize("N", [129, 128 * D16 + 1])
def test_nan_stays_in_its_tiles(dev, N):
    """a NaN at grad_out[b0,i0,c0] feeds the tiles of cloud b0 only: every cell it does not feed is equal under both schedules (and
    finite), the other cloud's tiles are untouched"""
    B, S, C = 2, 2, 16
    assert bwd_plan(B, N, S, C) == (16, 1)
    c = _case(B, N, 4, S, C, 8000 + N)
    g = _grad(c, 8100 + N)
    b0, i0, c0 = 1, N - 1, 6
    g[b0, i0, c0] = NAN
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    rows = _rows16(arg)
    (gfm_l, gd_l), (gfm_n, gd_n) = _both(c, arg, g, dev, fwin)
    keep = torch.ones_like(gfm_l, dtype=torch.bool).cpu()
    keep[b0, i0, c0] = False                                              # the centre column carries the NaN
    cols = torch.ones(S * C, dtype=torch.bool)
    for s in range(S):
        keep[b0, int(rows[b0, i0, s * C + c0]), C + s * C + c0] = False   # (fed cells: unspecified)
        cols[s * C + c0] = False
    gl, gn = gfm_l.cpu(), gfm_n.cpu()
    assert torch.isnan(gn[b0, i0, c0]) and torch.isnan(gl[b0, i0, c0])
    assert torch.isfinite(gn[keep]).all() and torch.equal(gl[keep], gn[keep])
    assert torch.isfinite(gd_n[:, cols.to(gd_n.device)]).all() and torch.equal(gd_l[:, cols.to(gd_l.device)], gd_n[:, cols.to(gd_n.device)])
    g0 = g.clone()
    g0[b0, i0, c0] = 0.0
    with schedule(0):
        rc, gfm0, _ = _run_scatter(c, arg, g0, dev, fwin)
    assert rc == 0
    assert torch.equal(gfm0[1 - b0], gfm_n[1 - b0]), "the other cloud's tiles changed with the NaN"


# ==== against fp64 ==================================================================================================================

FP64 = ([(2, 128 * D16 - 1, 2, 16, 16, 1, torch.float32), (2, 128 * D16 + 1, 2, 16, 16, 1, torch.float32)]
        + [t[:6] + (dt,) for t in HALF for dt in (torch.float32, BF)])


@pytest.mark.parametrize("B,N,S,C,tc,rs,dtype", FP64, ids=[f"B{t[0]}-N{t[1]}-{'bf16' if t[6] == BF else 'f32'}" for t in FP64])
def test_batched_schedule_against_fp64(dev, B, N, S, C, tc, rs, dtype):
    assert bwd_plan(B, N, S, C) == (tc, rs)
    c = _case(B, N, 4, S, C, 8200 + N, dtype=dtype)
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    g = _grad(c, 8300 + N)
    with schedule(0):
        rc, gfm, gd = _run_scatter(c, arg, g, dev, fwin)
        assert rc == 0
        _check_bwd(c, _rows16(arg), g, gfm, gd, True, f"batched N={N}")
        rc, gfm2, gd2 = _run_scatter(c, arg, g, dev, use_fwin=False)
        assert rc == 0 and torch.equal(gfm, gfm2)
        _check_bwd(c, _rows16(arg), g, None, gd2, True, f"batched N={N} (fm gather)")


# ==== centre columns ================================================================================================================

@pytest.mark.parametrize("B,N,S,C,T", [(2, 70, 2, 32, 4), (3, 151, 3, 16, 3), (2, 1079, 2, 16, 2)])
def test_centre_columns_are_a_copy(dev, B, N, S, C, T):
    """C / TC = 2 tiles hold centre columns under the legacy schedule; T tiles share them under the batched one, T not dividing N (nor N C / 4)"""
    tc, rs = bwd_plan(B, N, S, C)
    assert tc == 16 and S * C // tc == T and N % T != 0
    for dtype in (torch.float32, BF):
        c = _case(B, N, 4, S, C, 8400 + N, dtype=dtype)
        rc, _, arg, fwin = _run_fwd(c, dev)
        assert rc == 0
        g = _grad(c, 8500 + N)
        with schedule(0):
            rc, gfm, _ = _run_scatter(c, arg, g, dev, fwin)
        assert rc == 0
        assert torch.equal(gfm[:, :, :C].cpu(), g)


# ==== replay ========================================================================================================================

def test_captured_call_replays_to_the_eager_bits(dev):
    B, N, S, C = 2, 129, 2, 16
    assert bwd_plan(B, N, S, C) == (16, 1)
    c = _case(B, N, 4, S, C, 8600)
    rc, _, arg, fwin = _run_fwd(c, dev)
    assert rc == 0
    g = _grad(c, 8700)
    with schedule(0):
        rc, want_fm, want_gd = _run_scatter(c, arg, g, dev, fwin)
        assert rc == 0
        SC = S * C
        wsb = _L().hsp_rf_bwd_scatter_workspace_bytes(B, SC)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        xyz, dirs, gg = c.xyz.to(dev), c.dirs.to(dev), g.to(dev)
        gfm = torch.full((B, N, (S + 1) * C), NAN, device=dev)
        gd = torch.full((3, SC), NAN, device=dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = _L().hsp_rf_conv_bwd_scatter(_vp(xyz), _vp(dirs), None, _vp(fwin), _vp(arg), _vp(gg), B, N, S, C, _vp(gfm), _vp(gd),
                                              _vp(ws), wsb, _stream())
        assert rc == 0
    for _ in range(2):
        gfm.fill_(NAN)
        gd.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gfm, want_fm) and torch.equal(gd, want_gd)


# ==== the switch ====================================================================================================================

def test_switch():
    L = _L()
    first = L.hsp_rf_bwd_set_schedule(0)
    try:
        assert first == 0, "the default is the batched schedule"
        assert L.hsp_rf_bwd_set_schedule(1) == 0 and L.hsp_rf_bwd_set_schedule(1) == 1
        for bad in (2, -1):
            assert L.hsp_rf_bwd_set_schedule(bad) == BAD_ARG
        assert L.hsp_rf_bwd_set_schedule(0) == 1, "a refused value changed the switch"
        assert L.hsp_rf_bwd_set_schedule(0) == 0
    finally:
        L.hsp_rf_bwd_set_schedule(first if first in (0, 1) else 0)
