"""Host: the references of tests/_rows_ref.py against independent torch compositions (torch.cat, index_select, fp64 index_add_,
bincount), the condition that keeps the column-sum bound meaningful for every case the GPU test runs (the bound at most a quarter
of a column's largest term, that term on an edge row), hsp_colsum_rows_plan against hsp::colsum_cloud_plan and its own argument
checks, and the two route queries' arithmetic.  No GPU: the plan queries are host functions of libhsp.so."""
import ctypes

import numpy as np
import pytest
import torch

import _pool_bwd_ref as pref
import _rows_ref as R

BAD_ARG = -1
BF = torch.bfloat16


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def plan(B, N, C, eb):
    v = [ctypes.c_int(-7) for _ in range(4)]
    rc = _L().hsp_colsum_rows_plan(B, N, C, eb, *[ctypes.byref(x) for x in v])
    assert rc == 0, (rc, B, N, C, eb)
    return tuple(x.value for x in v)


# ---- the plan query ---------------------------------------------------------------------------------------------------------------

def test_plan_query_argument_checks():
    L = _L()
    v = [ctypes.c_int(-7) for _ in range(4)]
    p = [ctypes.byref(x) for x in v]
    for args in ((0, 10, 64, 4), (1, 0, 64, 4), (1, 10, 0, 4), (-1, 10, 64, 4), (1, 10, 64, 3), (1, 10, 64, 8), (1, 10, 64, 0)):
        assert L.hsp_colsum_rows_plan(*args, *p) == BAD_ARG, args
    for hole in range(4):
        q = list(p)
        q[hole] = None
        assert L.hsp_colsum_rows_plan(2, 100, 64, 4, *q) == BAD_ARG
    assert [x.value for x in v] == [-7] * 4                              # a refused call writes nothing
    # declines: form -1 and zeros, HSP_OK
    for C, eb in ((260, 4), (2048, 4), (48, 2), (6, 2), (1028, 4)):
        assert plan(3, 100, C, eb) == (0, 0, 0, -1), (C, eb)
        assert L.hsp_colsum_rows_takes(C, eb) == 0
    assert plan(3, 100, 64, 4)[3] == 0 and plan(3, 100, 64, 2)[3] == 0 and plan(3, 100, 48, 4)[3] == 1
    assert plan(1, 100, 1, 4)[2:] == (256, 1) and plan(1, 100, 255, 4)[2:] == (1, 1) and plan(1, 100, 100, 4)[2:] == (2, 1)
    assert plan(1, 100, 1024, 4)[2:] == (1, 0) and plan(1, 100, 4, 4)[2:] == (256, 0)


def test_plan_query_is_a_cover_of_the_rows():
    """whatever the chunking, it covers the N rows: nchunk = ceil(N / rows), rows >= 1, and the form follows the takes queries"""
    L = _L()
    for B in (1, 3, 16, 64):
        for N in (1, 2, 7, 31, 32, 33, 257, 1028, 4096, 4097, 5000, 100000):
            for C in R.VEC_WIDTHS + R.SCALAR_WIDTHS + (16, 32, 256, 260, 2048):
                for eb in (2, 4):
                    rows, nchunk, lanes, form = plan(B, N, C, eb)
                    assert (form >= 0) == bool(L.hsp_colsum_rows_takes(C, eb))
                    if form < 0:
                        continue
                    assert rows >= 1 and lanes >= 1 and nchunk == -(-N // rows)
                    assert (form == 0) == bool(L.hsp_colsum_rows_xyz_takes(C))
                    assert lanes == (256 // (C // 4) if form == 0 else 256 // C)
                    assert L.hsp_orl_workspace_bytes(B, N, C) == B * nchunk * C * 4


def test_cloud_plan_agrees_with_the_plan_query():
    """hsp::colsum_cloud_plan (what the weight-gradient rider chunks by) == hsp_colsum_rows_plan wherever hsp_colsum_cloud_ok"""
    L = _L()
    cloud_plan = getattr(ctypes.CDLL(L._name), "_ZN3hsp17colsum_cloud_planEiiiPiS0_")
    cloud_plan.restype = ctypes.c_int
    cloud_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    seen = [0, 0]
    for B in (1, 2, 3, 16, 64, 65535, 65536):
        for N in (1, 2, 7, 31, 32, 33, 100, 257, 1028, 4096, 4097, 5000, 12288, 12289, 100000, 393216, 393217):
            for C in (16, 32, 48, 64, 96, 128, 256, 512, 1024, 2048):
                r, n = ctypes.c_int(-7), ctypes.c_int(-7)
                took = cloud_plan(B, N, C, ctypes.byref(r), ctypes.byref(n))
                assert took == L.hsp_colsum_cloud_ok(B, N, C, 0)
                seen[took] += 1
                if took:
                    assert (r.value, n.value) == plan(B, N, C, 4)[:2] and plan(B, N, C, 4)[3] == 0
                else:
                    assert (r.value, n.value) == (-7, -7)
    assert min(seen) > 50


def test_rev_build_route_query():
    """hsp_rev_build_edges_in_lds: the documented arithmetic ((Nsrc + 1) * 4 + Nq * k * 4 bytes against 140 KiB), the GPU
    test's two shapes on either side of it, the declines"""
    q = _L().hsp_rev_build_edges_in_lds
    lim = 140 * 1024
    for nsrc, nq, k in ((1700, 1700, 20), (1792, 1792, 20), (4096, 4096, 20), (64, 300, 1), (35839, 50, 4), (35839, 1, 1), (1, 35839, 1),
                        (100, 35814, 1), (100, 35815, 1), (1024, 1707, 20), (1024, 1708, 20)):
        assert q(nsrc, nq, k) == (1 if (nsrc + 1) * 4 + nq * k * 4 <= lim else 0), (nsrc, nq, k)
    assert q(1700, 1700, 20) == 1 and q(1792, 1792, 20) == 0
    assert 1700 * 20 * 4 + 1701 * 4 < lim < 1792 * 20 * 4 + 1793 * 4
    assert q(35840, 10, 1) == -1 and q(0, 10, 1) == -1 and q(10, 0, 1) == -1 and q(10, 10, 0) == -1
    assert _L().hsp_rev_build_takes(35839) == 1 and _L().hsp_rev_build_takes(35840) == 0


# ---- the column-sum cases: the condition of every case the GPU test runs ------------------------------------------------------------

def _widths(form):
    return R.VEC_WIDTHS + (R.SCALAR_WIDTHS if form == "rows" else ())


@pytest.mark.parametrize("form", R.FORMS)
def test_colsum_cases_keep_the_bound_meaningful(form):
    dtype = BF if form.endswith("bf16") else torch.float32
    eb = 2 if dtype == BF else 4
    for C in _widths(form):
        cases = R.colsum_cases(plan, form, C)
        got = {plan(B, N, C, eb)[1] for B, N, _, _ in cases}
        assert set(R.CHUNKS) <= got and max(got) > 32, (C, sorted(got))
        assert {1, 3} <= {B for B, _, _, _ in cases} and {"range", "cancel"} == {k for _, _, k, _ in cases}
        for B, N, kind, seed in cases:
            rows, nchunk, lanes, f = plan(B, N, C, eb)
            assert f == (0 if C in R.VEC_WIDTHS else 1)
            x, xyz = R.colsum_data(B, N, C, kind, seed, rows, nchunk, dtype, form.startswith("xyz"))
            bad = R.colsum_condition(x, xyz, N, rows, nchunk, R.colsum_depth(rows, lanes, nchunk))
            assert bad is None, (form, B, N, C, kind, bad)


@pytest.mark.parametrize("with_xyz", [0, 1])
def test_cloud_cases_keep_the_bound_meaningful(with_xyz):
    ok = _L().hsp_colsum_cloud_ok
    for C in R.CLOUD_WIDTHS:
        cases = R.cloud_cases(plan, ok, C, with_xyz)
        assert sum(acc for *_, acc in cases) >= 3 and cases[-2][-1] and not cases[-1][-1]
        assert ok(1, cases[-2][1], C, with_xyz) == 1 and ok(1, cases[-2][1] + 1, C, with_xyz) == 0 and ok(1, cases[-1][1], C, with_xyz) == 0
        for B, N, kind, seed, quiet, acc in cases:
            if acc:
                rows, nchunk, lanes, _ = plan(B, N, C, 4)
                x, xyz = R.colsum_data(B, N, C, kind, seed, rows, nchunk, torch.float32, bool(with_xyz), quiet)
                bad = R.colsum_condition(x, xyz, N, rows, nchunk, R.colsum_depth(rows, lanes, nchunk))
                assert bad is None, (with_xyz, B, N, C, kind, bad)
    for C in (16, 48):
        assert not any(ok(B, N, C, with_xyz) for B in (1, 3) for N in (1, 7, 100, 1028))


def test_colsum_cases_hit_both_sizes_of_every_chunk_count():
    for C in (4, 64, 1024, 3, 255):
        ns = {(plan(B, N, C, 4)[:2], N) for B, N, _, _ in R.colsum_cases(plan, "rows", C)}
        for nchunk in R.CHUNKS:
            exact = [N for (rows, nc), N in ns if nc == nchunk and N == rows * nc]
            plus1 = [N for (rows, nc), N in ns if nc == nchunk and N == rows * (nc - 1) + 1]
            assert exact and plus1, (C, nchunk)


def test_colsum_condition_notices():
    """the condition is not vacuous: data without the planted edge rows fails it, and so does a bound blown up"""
    rows, nchunk, lanes, _ = plan(1, 1000, 64, 4)
    x, _ = R.colsum_data(1, 1000, 64, "range", 5, rows, nchunk)
    D = R.colsum_depth(rows, lanes, nchunk)
    assert R.colsum_condition(x, None, 1000, rows, nchunk, D) is None
    y = x.clone()
    y[:, R.edge_rows(1000, rows, nchunk)] = 0
    assert "edge row" in R.colsum_condition(y, None, 1000, rows, nchunk, D)
    assert "quarter" in R.colsum_condition(x, None, 1000, rows, nchunk, 10 ** 6)
    assert R.edge_rows(10, 4, 3) == [3, 7, 8, 9] and R.edge_rows(1, 1, 1) == [0] and R.edge_rows(8, 4, 2) == [3, 4, 7]
    assert R.colsum_depth(128, 16, 40) == 8 + 15 + 5 + 3


def test_colsum_ref_is_the_fp64_sum():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 37, 8, generator=g).to(BF)
    xyz = torch.randn(2, 37, 3, generator=g)
    want, T = R.colsum_ref(x, xyz)
    xd = x.float().double()                                              # bf16 -> fp32 -> fp64: exact widening
    assert torch.equal(want[:, 0], xd.sum(1)) and torch.equal(T[:, 0], xd.abs().sum(1))
    assert torch.allclose(want[:, 1:], torch.einsum("bnc,bnq->bqc", xd, xyz.double()), rtol=1e-13, atol=0)
    assert torch.allclose(T[:, 1:], torch.einsum("bnc,bnq->bqc", xd.abs(), xyz.double().abs()), rtol=1e-13, atol=0)
    tol = R.colsum_tol(T, 10, moments=True)
    assert torch.equal(tol[:, 0], 10 * R.U / (1 - 10 * R.U) * T[:, 0]) and torch.equal(tol[:, 3], 11 * R.U / (1 - 11 * R.U) * T[:, 3])


# ---- row assembly, gather, reverse map, fused passes --------------------------------------------------------------------------------

def test_concat_ref_is_torch_cat():
    g = torch.Generator().manual_seed(2)
    B, N = 3, 5
    a = torch.randn(B * N, 4, generator=g)
    src1 = torch.randn(B * 7, 2, generator=g)
    idx = torch.randint(0, 7, (B * N,), generator=g, dtype=torch.int32)
    per = torch.randn(B, 3, generator=g)
    ids = torch.tensor([0.0, 2.7, 5.0])
    segs = [dict(kind=0, width=4, src=a), dict(kind=3, width=6, src=ids), dict(kind=1, width=2, src=src1, idx=idx, nsrc=7),
            dict(kind=2, width=3, src=per)]
    onehot = torch.zeros(B, 6)
    onehot[0, 0] = onehot[1, 2] = onehot[2, 5] = 1
    rows1 = torch.cat([src1.view(B, 7, 2)[b].index_select(0, idx.view(B, N)[b].long()) for b in range(B)])
    want = torch.cat([a, onehot.repeat_interleave(N, 0), rows1, per.repeat_interleave(N, 0)], 1)
    assert torch.equal(R.concat_ref(segs, B, N), want)
    # out of range ids: an all-zero row; bf16: kind 2 / 3 rounded to the output type
    segs = [dict(kind=0, width=4, src=a.to(BF)), dict(kind=3, width=6, src=torch.tensor([-1.0, 6.0, 1e9])), dict(kind=2, width=3, src=per)]
    got = R.concat_ref(segs, B, N)
    assert got.dtype == BF and not got[:, 4:10].any() and torch.equal(got[:, 10:], per.to(BF).repeat_interleave(N, 0))


def test_concat_form_follows_the_documented_conditions():
    f = R.concat_form
    assert f(4, 904, [(0, 128, 0), (3, 8, 4), (1, 256, 16), (0, 512, 32)], 64) == "v16"
    assert f(4, 1288, [(0, 1280, 0), (3, 6, 4)], 0) == "v16"             # a kind 3 segment last: any width
    assert f(4, 906, [(0, 128, 0), (3, 8, 4), (1, 256, 16), (0, 512, 32)], 64) == "pair"
    assert f(4, 904, [(0, 128, 8), (0, 776, 0)], 0) == "pair"            # a base on 8 bytes
    assert f(4, 904, [(0, 128, 0), (3, 6, 4), (0, 768, 0)], 0) == "pair"  # a column offset of 134
    assert f(4, 18, [(0, 6, 0), (0, 10, 8), (0, 2, 0)], 8) == "pair"
    assert f(4, 9, [(0, 3, 0), (0, 5, 0)], 0) == "scalar" and f(4, 8, [(0, 3, 0), (0, 5, 0)], 0) == "scalar"
    assert f(4, 8, [(0, 4, 4), (0, 4, 0)], 0) == "scalar" and f(4, 8, [(0, 4, 0), (0, 4, 0)], 4) == "scalar"
    assert f(2, 976, [(0, 128, 0), (0, 256, 16), (0, 512, 32), (3, 8, 4)], 0) == "v16"
    assert f(2, 972, [(0, 128, 0), (0, 256, 16), (0, 512, 32), (3, 8, 4)], 0) == "pair"
    assert f(2, 18, [(0, 4, 0), (0, 12, 4), (0, 2, 8)], 4) == "pair" and f(2, 18, [(0, 4, 2)], 0) == "scalar"


def test_gather_refs_are_index_select_and_index_add():
    g = torch.Generator().manual_seed(3)
    B, Nsrc, Nq, C = 3, 9, 40, 6
    feat = torch.randn(B, Nsrc, C, generator=g)
    idx = torch.randint(0, Nsrc, (B, Nq), generator=g, dtype=torch.int32)
    out = R.gather_fwd_ref(feat, idx)
    for b in range(B):
        assert torch.equal(out[b], feat[b].index_select(0, idx[b].long()))
    assert torch.equal(R.gather_fwd_ref(feat, idx[0])[2], feat[2].index_select(0, idx[0].long()))
    gr = torch.randn(B, Nq, C, generator=g)
    want, T, n = R.gather_bwd_ref(gr, idx, Nsrc)
    onehot = torch.nn.functional.one_hot(idx.long(), Nsrc).double()      # (B,Nq,Nsrc)
    assert torch.allclose(want, onehot.transpose(1, 2) @ gr.double(), rtol=1e-13, atol=1e-15)
    assert torch.allclose(T, onehot.transpose(1, 2) @ gr.double().abs(), rtol=1e-13, atol=1e-15)
    assert torch.equal(n, onehot.sum(1))
    # the serial form: within n u T of the fp64 sum, exactly the loop, and sensitive to the order
    off, edge = R.rev_ref(idx.numpy(), Nsrc)
    ser = R.gather_bwd_serial(gr, off, edge, Nsrc)
    assert bool(((ser.double() - want).abs() <= n[..., None] * R.U * T).all())
    loop = np.zeros((B, Nsrc, C), np.float32)
    for b in range(B):
        for q in range(Nq):
            loop[b, idx[b, q]] = loop[b, idx[b, q]] + gr[b, q].numpy()
    assert np.array_equal(loop, ser.numpy())
    rev = R.gather_bwd_serial(gr, off, np.stack([np.concatenate([e[o[m]:o[m + 1]][::-1] for m in range(Nsrc)]) for o, e in zip(off, edge)]),
                              Nsrc)
    assert not torch.equal(rev, ser)
    # bf16: widened, summed in fp32, rounded once
    gb = gr.to(BF)
    sb = R.gather_bwd_serial(gb, off, edge, Nsrc)
    assert sb.dtype == BF and torch.equal(sb, R.gather_bwd_serial(gb.float(), off, edge, Nsrc).to(BF))


def test_rev_ref_and_the_pool_restatement_agree():
    rng = np.random.RandomState(4)
    B, Nidx, Nsrc, k, ks = 3, 50, 17, 4, 6
    idx = rng.randint(0, Nsrc, size=(B, Nidx, ks)).astype(np.int32)
    for qsel in (None, rng.randint(0, Nidx, size=31).astype(np.int32), rng.randint(0, Nidx, size=(B, 70)).astype(np.int32)):
        tg = R.rev_targets(idx, k, qsel)
        off, edge = R.rev_ref(tg, Nsrc)
        o2, e2 = pref.rev_index(idx, qsel, Nsrc, k)
        assert np.array_equal(off, o2) and np.array_equal(edge, e2) and off.dtype == np.int32 and edge.dtype == np.int32
        for b in range(B):
            t = torch.from_numpy(tg[b]).long()
            assert torch.equal(torch.from_numpy(off[b, 1:]).long(), torch.bincount(t, minlength=Nsrc).cumsum(0))
            for m in range(Nsrc):
                lst = edge[b, off[b, m]:off[b, m + 1]]
                assert np.array_equal(lst, np.nonzero(tg[b] == m)[0])     # every edge of the row, ascending


def test_fused_pass_refs():
    g = torch.Generator().manual_seed(5)
    o, f, t = torch.randn(2, 5, 4, generator=g), torch.randn(2, 5, 4, generator=g) * 1e3, torch.randn(2, 4, generator=g) * 1e-3
    want = R.residual_bias_ref(o.numpy(), f.numpy(), t.numpy())
    assert np.array_equal(want, (o + (f + t[:, None, :])).numpy())
    assert not np.array_equal(want, ((o + f) + t[:, None, :]).numpy())   # the association is part of the statement
    tiny, sub = np.float32(2.0 ** -126), np.float32(2.0 ** -140)
    y = np.array([0.0, -0.0, tiny, sub, -sub, np.nan, 1.0, -1.0], np.float32)
    ga, gb = np.arange(1, 9, dtype=np.float32), np.full(8, 0.5, np.float32)
    assert np.array_equal(R.add_relu_bwd_ref(ga, gb, y), np.array([0, 0, 3.5, 4.5, 0, 0, 7.5, 0], np.float32))
    assert np.array_equal(R.add_relu_bwd_ref(ga, None, y), np.array([0, 0, 3, 4, 0, 0, 7, 0], np.float32))
    yt = torch.from_numpy(y[[0, 1, 2, 3, 4, 6, 7]])                       # (NaN aside) autograd's threshold_backward
    gt = torch.from_numpy((ga + gb)[[0, 1, 2, 3, 4, 6, 7]])
    assert torch.equal(torch.ops.aten.threshold_backward(gt, yt, 0.0), torch.from_numpy(R.add_relu_bwd_ref(ga, gb, y)[[0, 1, 2, 3, 4, 6, 7]]))
