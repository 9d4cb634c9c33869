"""GPU: every row of tests/_takes_cases.py whose buffers stay under 64 MB, on the entry point the query speaks for: return code 0
exactly where the query says it takes the shape, HSP_ERR_UNSUPPORTED exactly where it declines, and on a decline every output
buffer still holds the sentinel it was filled with -- nothing was launched.  What the kernels compute at these edges is the
business of the reference tests."""
import ctypes

import pytest
import torch

import _takes_cases as tc

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
SENTINEL = -77
F32, BF16, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def _too_large(c):
    """rows whose buffers pass 64 MB: host-only"""
    if c.query == "hsp_knn_exact_takes" and c.args[2] != 3:
        B, N = c.args[:2]
        return 4 * B * N * N > (64 << 20)                              # (the distance matrix in the workspace)
    if c.query == "hsp_gemm_rows_bn_tiles_bf16":
        M, N, K = c.args
        return 2 * M * K + 4 * M * N > (64 << 20)
    return False


GPU_CASES = [c for c in tc.CASES if not _too_large(c)]


class Bufs:
    def __init__(self, dev):
        self.dev, self.outs = dev, []

    def rand(self, *shape, dtype=F32):
        g = torch.Generator().manual_seed(len(shape) + sum(shape))
        return torch.randn(*shape, generator=g).to(device=self.dev, dtype=dtype)

    def ints(self, high, *shape):
        g = torch.Generator().manual_seed(high)
        return torch.randint(0, high, shape, generator=g, dtype=I32).to(self.dev)

    def perm(self, n, keep):
        g = torch.Generator().manual_seed(n)
        return torch.randperm(n, generator=g)[:keep].to(device=self.dev, dtype=I32)

    def out(self, *shape, dtype=F32):
        """an output buffer full of the sentinel"""
        t = torch.full(shape, SENTINEL % 256 if dtype == U8 else SENTINEL, dtype=dtype, device=self.dev)
        self.outs.append(t)
        return t

    def ws(self, nbytes):
        return torch.empty(max(int(nbytes), 16), dtype=U8, device=self.dev), int(nbytes)

    def untouched(self, outs=None):
        torch.cuda.synchronize()
        return all(bool((t == (SENTINEL % 256 if t.dtype == U8 else SENTINEL)).all()) for t in (self.outs if outs is None else outs))


def _knn_xyz(L, b, B, N, k, drop):
    x, idx = b.rand(B, N, 3), b.out(B, N, k, dtype=I32)
    ws, wsb = b.ws(L.hsp_knn_xyz_workspace_bytes(B, N))
    return [(L.hsp_knn_xyz_f32(_vp(x), B, N, k, 0, drop, _vp(idx), None, _vp(ws), wsb, None, _stream()), [idx])]


def _knn_exact(L, b, B, N, C, k, drop):
    x, idx = b.rand(B, N, C), b.out(B, N, k, dtype=I32)
    ws, wsb = b.ws(L.hsp_knn_exact_workspace_bytes(B, N, C, k, drop))
    return [(L.hsp_knn_exact_f32(_vp(x), B, N, C, k, drop, 0, _vp(idx), _vp(ws), wsb, None, _stream()), [idx])]


def _geometry_levels(L, b, N0, N1, N2, k1, kpool, k2, drop, B=2):
    x, s1, s2 = b.rand(B, N0, 3), b.perm(N0, min(N1, N0)), b.perm(N1, min(N2, N1))
    if s1.numel() < N1 or s2.numel() < N2:                  # (a level larger than its source: declined before sel is read)
        s1, s2 = b.ints(N0, N1), b.ints(N1, N2)
    o = [b.out(B, N1, 3), b.out(B, N2, 3), b.out(B, N1, k1, dtype=I32), b.out(B, N1, kpool, dtype=I32), b.out(B, N2, k2, dtype=I32),
         b.out(B, N0, dtype=I32), b.out(B, N0, dtype=I32)]
    return [(L.hsp_geometry_levels_f32(_vp(x), B, N0, _vp(s1), N1, _vp(s2), N2, k1, kpool, k2, drop, *[_vp(t) for t in o], _stream()), o)]


def _geometry_all(L, b, B, N0, k0, kpool0, N1, N2, k1, kpool, k2, drop):
    x, s1, s2 = b.rand(B, N0, 3), b.perm(N0, N1), b.perm(N1, N2)
    o = [b.out(B, N0, k0, dtype=I32), b.out(B, N0, kpool0, dtype=I32), b.out(B, N1, 3), b.out(B, N2, 3), b.out(B, N1, k1, dtype=I32),
         b.out(B, N1, kpool, dtype=I32), b.out(B, N2, k2, dtype=I32), b.out(B, N0, dtype=I32), b.out(B, N0, dtype=I32)]
    ws, wsb = b.ws(L.hsp_geometry_all_workspace_bytes(B, N0))
    return [(L.hsp_geometry_all_f32(_vp(x), B, N0, k0, kpool0, _vp(s1), N1, _vp(s2), N2, k1, kpool, k2, drop, *[_vp(t) for t in o],
                                    _vp(ws), wsb, _stream()), o)]


def _rev_build(L, b, n_src, Nq=64):
    idx, off, edge = b.ints(n_src, 1, Nq), b.out(1, n_src + 1, dtype=I32), b.out(1, Nq, dtype=I32)
    return [(L.hsp_rev_build(_vp(idx), 1, Nq, n_src, 1, 1, _vp(off), _vp(edge), _stream()), [off, edge])]


def _gather_csr(L, b, es, C, stride, align, B=2, Nsrc=24, Nq=40):
    dt = F32 if es == 4 else BF16
    idx = b.ints(Nsrc, B, Nq)
    off = torch.empty(B, Nsrc + 1, dtype=I32, device=b.dev)
    edge = torch.empty(B, Nq, dtype=I32, device=b.dev)
    assert L.hsp_rev_build(_vp(idx), B, Nq, Nsrc, 1, 1, _vp(off), _vp(edge), _stream()) == 0
    raw = torch.zeros(B * Nq * stride * es + 16, dtype=U8, device=b.dev)
    assert raw.data_ptr() % 16 == 0
    g = raw[align:align + B * Nq * stride * es].view(dt)
    g.copy_(b.rand(B * Nq * stride, dtype=dt))
    gfeat = b.out(B, Nsrc, C, dtype=dt)
    fn = L.hsp_gather_rows_bwd_csr if es == 4 else L.hsp_gather_rows_bwd_csr_bf16
    return [(fn(_vp(g), stride, _vp(off), _vp(edge), B, Nsrc, Nq, C, _vp(gfeat), _stream()), [gfeat])]


def _colsum_rows(L, b, C, es, B=2, N=40):
    x, out = b.rand(B, N, C, dtype=F32 if es == 4 else BF16), b.out(B, C)
    ws, wsb = b.ws(L.hsp_orl_workspace_bytes(B, N, C))
    fn = L.hsp_colsum_rows if es == 4 else L.hsp_colsum_rows_bf16
    return [(fn(_vp(x), B, N, C, _vp(out), _vp(ws), wsb, _stream()), [out])]


def _colsum_rows_xyz(L, b, C, B=2, N=40):
    x, xyz, out = b.rand(B, N, C), b.rand(B, N, 3), b.out(B, 4 * C)
    ws, wsb = b.ws(4 * L.hsp_orl_workspace_bytes(B, N, C))
    return [(L.hsp_colsum_rows_xyz(_vp(x), _vp(xyz), B, N, C, _vp(out), _vp(ws), wsb, _stream()), [out])]


def _bn(L, b, R, C):
    x, gamma, beta = b.rand(R, C), b.rand(C), b.rand(C)
    o = [b.out(R, C), b.out(C), b.out(C), b.out(C), b.out(C), b.out(1, dtype=torch.int64)]
    ws, wsb = b.ws(L.hsp_bn_workspace_bytes(R, C))
    return [(L.hsp_bn_relu_fwd(_vp(x), R, C, _vp(gamma), _vp(beta), 1e-5, 0.1, 1, *[_vp(t) for t in o], _vp(ws), wsb, _stream()), o)]


def _small_outer(L, b, B, Ma=8, Nb=12):
    a, c, out = b.rand(B, Ma), b.rand(B, Nb), b.out(Ma, Nb)
    return [(L.hsp_small_outer_f32(_vp(a), Ma, _vp(c), Nb, B, Ma, Nb, _vp(out), Nb, None, 0, 0, None, _stream()), [out])]


def _small_pair(L, b, B, Ma):
    Nn = Nb = Ma                                            # (the layer's shapes: Wb and gWb are (C, C))
    gt, W, c = b.rand(B, Ma), b.rand(Ma, Nn), b.rand(B, Nb)
    out_nn, out_o = b.out(B, Nn), b.out(Ma, Nb)
    return [(L.hsp_small_pair_f32(_vp(gt), Ma, B, Ma, _vp(W), Nn, Nn, 1.0, _vp(out_nn), Nn, _vp(c), Nb, Nb, _vp(out_o), Nb, None, 0, 0, None,
                                  _stream()), [out_nn, out_o])]


def _exact_layer(L, b, N, Cin, C, B=2, k=4):
    """the reference-order entry points of one layer, each on its own outputs: the fm product over K = Cin (not for the surface
    layer), the ORL, the out product in the chain form C selects"""
    R, calls = B * N, []
    if Cin != 3:
        X2, W, fm = b.rand(R, Cin), b.rand(Cin, C), b.out(R, C)
        calls.append((L.hsp_gemm_wave_f32(_vp(X2), Cin, _vp(W), C, 1, Cin, None, 0, None, 0, 0, 0, R, C, None, None, 0, None, 0, 1.0, None, None,
                                          _vp(fm), C, 0, _stream()), [fm]))
    F3, idx = b.rand(B, N, C), b.ints(N, B, N, k)
    fg, arg = b.out(B, C), b.out(B, N, C, dtype=U8)
    ws, wsb = b.ws(L.hsp_orl_exact_workspace_bytes(B, N, C))
    calls.append((L.hsp_orl_global_exact_f32(_vp(F3), _vp(idx), B, N, k, k, C, _vp(fg), _vp(arg), _vp(ws), wsb, _stream()), [fg, arg]))
    w2, fgin, ste, out = b.rand(C, 2 * C), b.rand(B, C), b.rand(R, C), b.out(R, C)
    Wa, Wb = w2[:, :C], w2[:, C:]
    two = 2 * C > 256
    t2 = b.rand(B, C) if two else None
    calls.append((L.hsp_layer_out_exact_f32(_vp(F3), C, _vp(Wa), 2 * C, _vp(None if two else fgin), 0 if two else C, _vp(None if two else Wb),
                                            0 if two else 2 * C, _vp(t2), int(two), _vp(ste), C, None, None, 0, R, C, N, _vp(out), C,
                                            _stream()), [out]))
    return calls


def _fps_levels(L, b, N0, B=1):
    N1, N2 = N0 // 4, N0 // 16
    x, sel1, v1, v2 = b.rand(B, N0, 3), b.out(B, N1, dtype=I32), b.out(B, N1, 3), b.out(B, N2, 3)
    return [(L.hsp_fps_levels_f32(_vp(x), B, N0, N1, N2, _vp(sel1), _vp(v1), _vp(v2), _stream()), [sel1, v1, v2])]


def _rows_bn(L, b, M, N, K):
    A, W, bias = b.rand(M, K, dtype=BF16), b.rand(N, K, dtype=BF16), b.rand(N)
    o = [b.out(M, N), b.out(N), b.out((M + 63) // 64, 2, N)]            # (partials: room for 64-row tiles whatever the kernel's)
    return [(L.hsp_gemm_rows_bn_bf16(_vp(A), K, _vp(W), K, K, M, N, _vp(bias), None, 0, None, None, _vp(o[0]), N, _vp(o[1]), _vp(o[2]),
                                     _stream()), o)]


ENTRY = {"hsp_knn_xyz_takes": _knn_xyz, "hsp_knn_exact_takes": _knn_exact, "hsp_geometry_levels_takes": _geometry_levels,
         "hsp_geometry_all_takes": _geometry_all, "hsp_rev_build_takes": _rev_build, "hsp_gather_rows_bwd_csr_takes": _gather_csr,
         "hsp_colsum_rows_takes": _colsum_rows, "hsp_colsum_rows_xyz_takes": _colsum_rows_xyz, "hsp_bn_takes": _bn,
         "hsp_small_outer_takes": _small_outer, "hsp_small_pair_takes": _small_pair, "hsp_exact_layer_takes": _exact_layer,
         "hsp_fps_levels_takes": _fps_levels, "hsp_gemm_rows_bn_tiles_bf16": _rows_bn}


def test_every_query_has_an_entry_point_here():
    assert set(ENTRY) == set(tc.QUERIES)


@pytest.mark.parametrize("c", GPU_CASES, ids=tc.case_id)
def test_entry_point_declines_exactly_where_its_query_does(dev, c):
    L, b = _L(), Bufs(dev)
    takes = getattr(L, c.query)(*c.args) > 0
    assert takes == (c.want > 0)
    calls = ENTRY[c.query](L, b, *c.args)
    rcs = [rc for rc, _ in calls]
    print(f"{tc.case_id(c)}: query {int(takes)}, return codes {rcs}")
    if takes:
        torch.cuda.synchronize()
        assert rcs == [0] * len(calls)
        return
    assert UNSUPPORTED in rcs and set(rcs) <= {0, UNSUPPORTED}, f"return codes {rcs}"
    declined = [t for rc, outs in calls if rc == UNSUPPORTED for t in outs]
    assert b.untouched(declined), "a declined call wrote to its outputs"
