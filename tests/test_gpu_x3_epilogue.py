"""GPU: the epilogue of the x3 tile kernel (csrc/gemm_x3.hip).

The residual + per-cloud-bias epilogue issues its loads up front and its stores back to back, through buffer descriptors of the
tile's rows; the arithmetic per element is (alpha acc + bias) + resid, + cloud_bias, in that order, so the call with the
epilogue must equal, BIT FOR BIT, the call without one followed by the same two fp32 adds (the library is built with
-ffp-contract=off; both calls run the same k-loop).  Ragged last row tile (4 of 64 rows), ragged column tile, pitched result and
residual with guard rows / columns behind them, clouds of 257 / 65 / 64 / 40 rows (two clouds per tile at most; a boundary that
walks through the tiles; tile = cloud; the per-row form), and the 128-row kernel once.

BatchNorm partials of hsp_gemm_x3_bn_f32: the shift is row 0's residual + per-cloud bias, the per-tile sums are the fp64 shifted
sums of the kernel's own result rows within the bound of tests/test_gpu_bn_reference.py part B (_check_tile_sums: 1e-5 of the
column's sum of magnitudes / of the sum of squares), and the result itself is held to fp64 by the rule of
tests/test_gpu_gemm_x3.py (max <= max(3.5 x the fp32 library product's own error, 2e-6 of scale)).

(The in-workgroup K split the same work built -- tools/experiments/gemm_x3_kgroups.patch -- did not pay and does not ship; its
tests went with it.)"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

M, RAGGED_N = 4100, 200                   # 65 row tiles, the last with 4 rows; x 2 column tiles = 130 tiles: the x3 tile kernel
NAN = float("nan")


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_OPERANDS = {}


def _operands(dev, M_, N, K1, K2):
    """rows with uneven magnitudes, weights of 0.05, bias, a pitched residual, per-cloud rows; the fp64 product and the fp32 library
    product of the same operands -- drawn and computed once per shape"""
    key = (M_, N, K1, K2)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(M_ + N + K1 + 7 * K2)
        o = {}
        scale = 1.0 + 3.0 * torch.rand(M_, 1, generator=g)
        o["A1"] = (torch.randn(M_, K1, generator=g) * scale).to(dev)
        o["B1"] = (torch.randn(N, K1, generator=g) * 0.05).to(dev)
        o["A2"] = torch.randn(M_, K2, generator=g).to(dev) if K2 else None
        o["B2"] = (torch.randn(N, K2, generator=g) * 0.05).to(dev) if K2 else None
        o["bias"] = torch.randn(N, generator=g).to(dev)
        o["resid"] = torch.randn(M_, N + 4, generator=g).to(dev)[:, :N]          # ldr > N
        o["cb"] = torch.randn(M_, N, generator=g).to(dev)                          # rows for any rows_per_cloud >= 1
        p64 = o["A1"].double() @ o["B1"].double().t()
        p32 = o["A1"] @ o["B1"].t()
        if K2:
            p64 = p64 + o["A2"].double() @ o["B2"].double().t()
            p32 = p32 + o["A2"] @ o["B2"].t()
        o["p64"], o["p32"] = p64, p32.double()
        _OPERANDS[key] = o
    return _OPERANDS[key]


def _x3(o, epi, rpc=0, alpha=1.0, pitch=0):
    from hs_pose_amd import ops
    M_, N = o["A1"].shape[0], o["B1"].shape[0]
    buf = torch.full((M_ + 1, N + pitch), NAN, device=o["A1"].device)               # (a guard row and guard columns)
    out = buf[:M_, :N]
    clouds = (M_ + rpc - 1) // rpc if rpc else 0
    ops.gemm_x3(o["A1"], o["B1"], False, o["A2"], o["B2"], False, bias=o["bias"] if epi == "bias" else None,
                resid=o["resid"] if epi == "rc" else None, cloud_bias=o["cb"][:clouds] if epi == "rc" else None,
                rows_per_cloud=rpc, out=out, alpha=alpha)
    torch.cuda.synchronize()
    assert torch.isnan(buf[M_]).all() and (pitch == 0 or torch.isnan(buf[:, N:]).all()), "wrote outside its rows / columns"
    return out


def _epilogue_bitwise(dev, M_, N, rpc):
    o = _operands(dev, M_, N, 96, 64)
    got = _x3(o, "rc", rpc, pitch=8)
    plain = _x3(o, "none", pitch=8)
    assert torch.isfinite(got).all()
    cb_rows = o["cb"][:(M_ + rpc - 1) // rpc].repeat_interleave(rpc, dim=0)[:M_]
    want = (plain + o["resid"]) + cb_rows
    assert torch.equal(got, want), f"rpc={rpc}: {(got != want).sum().item()} elements differ, max {(got - want).abs().max().item():.3e}"


@pytest.mark.parametrize("rpc", [257, 65, 64, 40])
@pytest.mark.parametrize("N", [256, RAGGED_N])
def test_epilogue_is_the_plain_product_plus_two_adds(dev, N, rpc):
    out = (ctypes.c_int * 4)()
    for epi in (0, 6):                                         # both calls: the 64-row tile kernel, no K split
        assert _L().hsp_gemm_x3_plan(M, N, 96, 64, epi, N + 8, out) == 0 and list(out)[:3] == [0, 1, 1]
    _epilogue_bitwise(dev, M, N, rpc)


@pytest.mark.parametrize("rpc", [1000, 100])
def test_epilogue_of_the_128_row_kernel(dev, rpc):
    """M = 8192, N = 128 is 64 tiles of 128 rows: such a call runs 64-row tiles (the 128-row kernel starts at 512 tiles), so the
    128-row epilogue is not reachable there; it is at 129 x 4 = 516 tiles -- a ragged last tile of 4 rows, clouds longer and
    shorter than a tile"""
    out = (ctypes.c_int * 4)()
    Mt, Nt = 16388, 512
    assert _L().hsp_gemm_x3_plan(8192, 128, 96, 64, 6, 128, out) == 0 and out[1] == 1
    assert _L().hsp_gemm_x3_plan(Mt, Nt, 96, 64, 6, Nt + 8, out) == 0 and list(out)[:3] == [0, 2, 1]
    assert _L().hsp_gemm_x3_plan(Mt, Nt, 96, 64, 0, Nt + 8, out) == 0 and list(out)[:3] == [0, 2, 1]
    _epilogue_bitwise(dev, Mt, Nt, rpc)


def test_bn_partials_against_fp64_sums(dev):
    from hs_pose_amd import ops
    L = _L()
    N, K1, K2, rpc = 256, 128, 256, 257
    o = _operands(dev, M, N, K1, K2)
    tiles = (M + 63) // 64
    P1, ldp1, ps1 = ops.x3_planes.planes(o["B1"], False)
    P2, ldp2, ps2 = ops.x3_planes.planes(o["B2"], False)
    resid, cb = o["resid"], o["cb"][:(M + rpc - 1) // rpc]
    want = (o["p64"] + resid.double()) + cb.double().repeat_interleave(rpc, dim=0)[:M]
    lib_err = ((o["p32"] + resid.double() + cb.double().repeat_interleave(rpc, dim=0)[:M]) - want).abs().max().item()
    out = torch.full((M, N), NAN, device=dev)
    buf = torch.full((1 + 2 * tiles + 2, N), NAN, device=dev)
    part = buf[1:1 + 2 * tiles]
    rc = L.hsp_gemm_x3_bn_f32(_vp(o["A1"]), K1, _vp(P1), ldp1, ps1, K1, _vp(o["A2"]), K2, _vp(P2), ldp2, ps2, K2, M, N,
                              _vp(resid), resid.stride(0), _vp(cb), rpc, _vp(out), N, _vp(buf[0]), _vp(part), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(out).all()
    err = (out.double() - want).abs().max().item()
    print(f"bn_out: max err {err:.2e} (fp32 library {lib_err:.2e})")
    assert err <= max(3.5 * lib_err, 2e-6 * want.abs().max().item())
    assert torch.equal(buf[0], resid[0] + cb[0])                                       # the documented shift
    assert torch.isnan(buf[1 + 2 * tiles:]).all() and torch.isfinite(part).all()
    d = out.double() - buf[0].double()
    pt = part.view(tiles, 2, N).double()
    for t in range(tiles):                                                             # (the bound of test_gpu_bn_reference part B)
        blk = d[t * 64:(t + 1) * 64]
        s1, s2 = blk.sum(0), (blk * blk).sum(0)
        assert ((pt[t, 0] - s1).abs() <= 1e-5 * blk.abs().sum(0)).all(), ("sum", t)
        assert ((pt[t, 1] - s2).abs() <= 1e-5 * s2).all(), ("sum of squares", t)
