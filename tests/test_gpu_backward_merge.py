"""GPU: the merged launches of the backward pass against the launches they replace, bit for bit (``torch.equal``):
``hsp_gather_rows_bwd_csr_multi`` / ``hsp_rev_build_multi`` (the backward of the feat concat's gathered segments in two launches
where it was one per segment and one per reverse map) and ``hsp_wgrad_partial_pair_colsum_f32`` (an HS layer's per-cloud column
sum as a rider of its weight-gradient pair launch) -- entry point by entry point, then the autograd nodes end to end."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

_vpt = ctypes.c_void_p


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptrs(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), _vpt)


def _ints(vs):
    return ctypes.cast((ctypes.c_int * len(vs))(*vs), _vpt)


def _row_map(B, Nq, Ns, seed):
    """(B, Nq) int32 map into Ns source rows: row 0 is chosen by no query, row 1 by 9 (not a multiple of 4), row 2 by exactly one,
    the other queries spread over the remaining rows by a fixed shuffle -- repeated targets throughout"""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(B, Nq, dtype=torch.int32)
    for b in range(B):
        rest = 3 + torch.randint(0, Ns - 3, (Nq - 10,), generator=g)
        m = torch.cat([torch.full((9,), 1), torch.full((1,), 2), rest])
        out[b] = m[torch.randperm(Nq, generator=g)].to(torch.int32)
        cnt = torch.bincount(out[b].long(), minlength=Ns)
        assert cnt[0] == 0 and cnt[1] == 9 and cnt[2] == 1
    return out


def _rev_build(idx, Ns):
    from hs_pose_amd._lib import lib
    B, Nq = idx.shape
    off = torch.full((B, Ns + 1), -1, dtype=torch.int32, device=idx.device)
    edge = torch.full((B, Nq), -1, dtype=torch.int32, device=idx.device)
    assert lib().hsp_rev_build(_vp(idx), B, Nq, Ns, 1, 1, _vp(off), _vp(edge), _stream()) == 0
    return off, edge


def test_rev_build_multi_equals_rev_build_per_map(dev):
    from hs_pose_amd._lib import lib
    B, Nq = 3, 50
    maps = [(_row_map(B, Nq, 13, 1).to(dev), 13), (_row_map(B, Nq, 5, 2).to(dev), 5)]
    want = [_rev_build(idx, Ns) for idx, Ns in maps]
    offs = [torch.full((B, Ns + 1), -1, dtype=torch.int32, device=dev) for _, Ns in maps]
    edges = [torch.full((B, Nq), -1, dtype=torch.int32, device=dev) for _ in maps]
    rc = lib().hsp_rev_build_multi(2, _ptrs([m[0] for m in maps]), B, _ints([Nq, Nq]), _ints([13, 5]), _ints([1, 1]), _ints([1, 1]),
                                   _ptrs(offs), _ptrs(edges), _stream())
    assert rc == 0
    for (woff, wedge), off, edge in zip(want, offs, edges):
        assert torch.equal(off, woff) and torch.equal(edge, wedge)
    # a neighbour list (k = 4 of kstride 5) beside a row map: the two maps of one launch need not look alike
    knn = torch.randint(0, 13, (B, Nq, 5), generator=torch.Generator().manual_seed(3)).to(dev, torch.int32)
    woff = torch.empty(B, 14, dtype=torch.int32, device=dev)
    wedge = torch.empty(B, Nq * 4, dtype=torch.int32, device=dev)
    assert lib().hsp_rev_build(_vp(knn), B, Nq, 13, 4, 5, _vp(woff), _vp(wedge), _stream()) == 0
    off2 = [torch.full((B, 14), -1, dtype=torch.int32, device=dev), torch.full((B, 6), -1, dtype=torch.int32, device=dev)]
    edge2 = [torch.full((B, Nq * 4), -1, dtype=torch.int32, device=dev), torch.full((B, Nq), -1, dtype=torch.int32, device=dev)]
    rc = lib().hsp_rev_build_multi(2, _ptrs([knn, maps[1][0]]), B, _ints([Nq, Nq]), _ints([13, 5]), _ints([4, 1]), _ints([5, 1]),
                                   _ptrs(off2), _ptrs(edge2), _stream())
    assert rc == 0
    assert torch.equal(off2[0], woff) and torch.equal(edge2[0], wedge)
    assert torch.equal(off2[1], want[1][0]) and torch.equal(edge2[1], want[1][1])


# (B, leading columns, dtype): case 1 -- 16-byte aligned segments; case 2 -- behind a 2-element leading segment the offsets are
# only 8-byte (bf16: 4-byte) aligned, the two-column path; case 3 -- one cloud, both storage types
@pytest.mark.parametrize("B,lead,dtype", [(3, 0, "f32"), (3, 2, "f32"), (1, 0, "f32"), (1, 0, "bf16"), (1, 2, "bf16"), (3, 0, "bf16")])
def test_gather_rows_bwd_csr_multi_equals_the_launch_per_segment(dev, ref, B, lead, dtype):
    from hs_pose_amd._lib import lib
    L = lib()
    Nq, pitch = 50, 592
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    sfx = "_bf16" if dtype == "bf16" else ""
    segs = [(13, 8), (13, 64), (5, 512)]
    idx13, idx5 = _row_map(B, Nq, 13, 11), _row_map(B, Nq, 5, 12)
    rev = {13: _rev_build(idx13.to(dev), 13), 5: _rev_build(idx5.to(dev), 5)}
    g_cpu = ref.hash_tensor((B, Nq, pitch), 21, 1.0).to(dt)
    g = g_cpu.to(dev)
    col, views = lead, []
    for Ns, w in segs:
        views.append(g[:, :, col:col + w])
        col += w
    assert col <= pitch
    want = []
    for (Ns, w), v in zip(segs, views):
        o = torch.full((B, Ns, w), float("nan"), dtype=dt, device=dev)
        assert getattr(L, "hsp_gather_rows_bwd_csr" + sfx)(_vp(v), pitch, _vp(rev[Ns][0]), _vp(rev[Ns][1]), B, Ns, Nq, w, _vp(o),
                                                           _stream()) == 0
        want.append(o)
    got = [torch.full((B, Ns, w), float("nan"), dtype=dt, device=dev) for Ns, w in segs]
    rc = getattr(L, "hsp_gather_rows_bwd_csr_multi" + sfx)(3, _ptrs(views), pitch, _ptrs([rev[Ns][0] for Ns, _ in segs]),
                                                           _ptrs([rev[Ns][1] for Ns, _ in segs]), B, _ints([s[0] for s in segs]), Nq,
                                                           _ints([s[1] for s in segs]), _ptrs(got), _stream())
    assert rc == 0
    for a, b in zip(got, want):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    # and the sums themselves: fp32 adds from 0 in ascending query order, rounded once to the storage type
    col = lead
    for (Ns, w), a in zip(segs, got):
        idx = idx13 if Ns == 13 else idx5
        acc = torch.zeros(B, Ns, w, dtype=torch.float32)
        for b in range(B):
            for q in range(Nq):
                acc[b, idx[b, q]] += g_cpu[b, q, col:col + w].float()
        assert torch.equal(a.cpu(), acc.to(dt))
        assert (a[:, 0] == 0).all()                               # the row no query chose
        col += w


def test_gather_rows_bwd_csr_multi_declines_what_the_single_launch_declines(dev, ref):
    """an odd width: HSP_ERR_UNSUPPORTED from both, and nothing written"""
    from hs_pose_amd._lib import lib
    B, Nq = 1, 50
    idx = _row_map(B, Nq, 5, 5).to(dev)
    off, edge = _rev_build(idx, 5)
    g = ref.hash_tensor((B, Nq, 592), 22, 1.0).to(dev)
    outs = [torch.full((B, 5, 8), float("nan"), device=dev), torch.full((B, 5, 7), float("nan"), device=dev)]
    assert lib().hsp_gather_rows_bwd_csr(_vp(g[:, :, 8:15]), 592, _vp(off), _vp(edge), B, 5, Nq, 7, _vp(outs[1]), _stream()) == -2
    rc = lib().hsp_gather_rows_bwd_csr_multi(2, _ptrs([g[:, :, 0:8], g[:, :, 8:15]]), 592, _ptrs([off, off]), _ptrs([edge, edge]), B,
                                             _ints([5, 5]), Nq, _ints([8, 7]), _ptrs(outs), _stream())
    assert rc == -2
    assert torch.isnan(outs[0]).all() and torch.isnan(outs[1]).all()


class _Calls:
    """records the C-ABI calls a backward issues, by entry point"""

    def __init__(self, ops, monkeypatch):
        self.names = []
        real = ops._run

        def run(name, args, **kw):
            self.names.append(name)
            return real(name, args, **kw)
        monkeypatch.setattr(ops, "_run", run)


def _nan_fill_hook(t):
    junk = [torch.full_like(t, float("nan")) for _ in range(4)]
    del junk


def test_assemble_feat_backward_merged_equals_the_five_launches(dev, ref, monkeypatch):
    """the feat concat's backward: two direct 128-wide segments, three gathered ones ((25, 256), (25, 256) sharing a map, (7, 512))
    and the id segment -- every returned gradient with CONCAT_BWD_MERGE on and off, and with NaN-filled allocations between
    the merged launches"""
    from hs_pose_amd import ops
    B, N = 2, 100
    gen = torch.Generator().manual_seed(7)
    near1 = torch.randint(0, 25, (B, N), generator=gen).to(dev, torch.int32)
    near2 = torch.randint(0, 7, (B, N), generator=gen).to(dev, torch.int32)
    srcs = [ref.hash_tensor(s, 30 + i, 1.0).to(dev) for i, s in enumerate([(B, N, 128), (B, N, 128), (B, 25, 256), (B, 25, 256),
                                                                          (B, 7, 512)])]
    ids = torch.tensor([2.0, 5.0], device=dev)
    up = ref.hash_tensor((B, N, 1286), 36, 1.0).to(dev)
    calls = _Calls(ops, monkeypatch)

    def run(merge, hook=False):
        monkeypatch.setattr(ops, "CONCAT_BWD_MERGE", merge)
        ts = [t.clone().requires_grad_(True) for t in srcs]
        n1, n2 = near1.clone(), near2.clone()                     # (fresh maps: the reverse index is memoised on the tensor)
        feat = ops.assemble_feat([(ts[0], None, 0), (ts[1], None, 0), (ts[2], n1, 1), (ts[3], n1, 1), (ts[4], n2, 1), (ids, None, 3)])
        assert feat.shape == (B, N, 1286)
        calls.names.clear()
        if hook:
            real = ops._run

            def run_and_fill(name, args, **kw):
                r = real(name, args, **kw)
                _nan_fill_hook(up)
                return r
            monkeypatch.setattr(ops, "_run", run_and_fill)
        feat.backward(up)
        if hook:
            monkeypatch.setattr(ops, "_run", real)
        return [t.grad.clone() for t in ts], list(calls.names)

    old, old_calls = run(False)
    new, new_calls = run(True)
    hooked, _ = run(True, hook=True)
    assert old_calls.count("hsp_rev_build") == 2 and old_calls.count("hsp_gather_rows_bwd_csr") == 3
    assert new_calls == ["hsp_rev_build_multi", "hsp_gather_rows_bwd_csr_multi"]
    for a, b, c in zip(old, new, hooked):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c)


def _pair_args(g2, F2, out0, X2, out1, ws0, ws1, pend):
    from hs_pose_amd._lib import lib
    (K, M), N0, N1 = g2.shape, F2.shape[1], X2.shape[1]
    return (_vp(g2), g2.stride(0), _vp(F2), F2.stride(0), M, N0, K, _vp(out0), out0.stride(0), _vp(ws0), ws0.numel(),
            _vp(g2), g2.stride(0), _vp(X2), X2.stride(0), M, N1, K, _vp(out1), out1.stride(0), _vp(ws1), ws1.numel(), pend)


@pytest.mark.parametrize("B,N,C", [(3, 100, 128), (16, 64, 256), (2, 257, 512)])
def test_colsum_rider_equals_the_separate_launches(dev, ref, B, N, C):
    """mom == hsp_colsum_cloud_f32's and both weight gradients, after the pending fold, == hsp_wgrad_partial_pair_f32's alone"""
    from hs_pose_amd._lib import HspWgradPending, lib
    L = lib()
    Cin = 128
    g = ref.hash_tensor((B, N, C), 41, 1.0).to(dev)
    F = ref.hash_tensor((B, N, C), 42, 1.0).to(dev)
    X = ref.hash_tensor((B, N, Cin), 43, 1.0).to(dev)
    g2, F2, X2 = g.view(B * N, C), F.view(B * N, C), X.view(B * N, Cin)
    want_mom = torch.full((B, C), float("nan"), device=dev)
    assert L.hsp_colsum_cloud_f32(_vp(g), None, B, N, C, _vp(want_mom), _stream()) == 0

    def products(rider):
        conv2 = torch.full((C, 2 * C), float("nan"), device=dev)
        ste = torch.full((C, Cin), float("nan"), device=dev)
        ws0 = torch.empty(max(L.hsp_wgrad_workspace_bytes(C, C, B * N), 16), dtype=torch.uint8, device=dev)
        ws1 = torch.empty(max(L.hsp_wgrad_workspace_bytes(C, Cin, B * N), 16), dtype=torch.uint8, device=dev)
        pend = (HspWgradPending * 2)()
        args = _pair_args(g2, F2, conv2[:, :C], X2, ste, ws0, ws1, pend)
        mom = torch.full((B, C), float("nan"), device=dev)
        if rider:
            rc = L.hsp_wgrad_partial_pair_colsum_f32(*args, _vp(g), B, N, C, _vp(mom), _stream())
        else:
            rc = L.hsp_wgrad_partial_pair_f32(*args, _stream())
        assert rc == 0
        assert L.hsp_wgrad_fold(pend, 2, _stream()) == 0
        torch.cuda.synchronize()
        return conv2, ste, mom

    want_conv2, want_ste, _ = products(False)
    conv2, ste, mom = products(True)
    assert torch.equal(mom, want_mom)
    assert torch.equal(conv2[:, :C], want_conv2[:, :C]) and torch.isnan(conv2[:, C:]).all()
    assert torch.equal(ste, want_ste) and torch.isfinite(ste).all()


def test_colsum_rider_declines_a_width_the_column_sum_declines(dev, ref):
    """C = 48 (hsp_colsum_cloud_ok == 0): HSP_ERR_UNSUPPORTED, nothing launched, nothing written"""
    from hs_pose_amd._lib import HspWgradPending, lib
    L = lib()
    B, N, C = 2, 64, 48
    assert L.hsp_colsum_cloud_ok(B, N, C, 0) == 0
    g = ref.hash_tensor((B, N, 128), 44, 1.0).to(dev)
    x = ref.hash_tensor((B, N, C), 45, 1.0).to(dev)
    g2 = g.view(B * N, 128)
    conv2 = torch.full((128, 256), float("nan"), device=dev)
    ste = torch.full((128, 128), float("nan"), device=dev)
    ws = [torch.empty(max(L.hsp_wgrad_workspace_bytes(128, 128, B * N), 16), dtype=torch.uint8, device=dev) for _ in range(2)]
    pend = (HspWgradPending * 2)()
    mom = torch.full((B, C), float("nan"), device=dev)
    rc = L.hsp_wgrad_partial_pair_colsum_f32(*_pair_args(g2, g2, conv2[:, :128], g2, ste, ws[0], ws[1], pend), _vp(x), B, N, C,
                                             _vp(mom), _stream())
    assert rc == -2
    torch.cuda.synchronize()
    assert torch.isnan(mom).all() and torch.isnan(ste).all() and torch.isnan(conv2).all()


def _hs_layer_runner(dev, ref, monkeypatch, B, N, Cin, C, k, S, seed=61):
    from hs_pose_amd import gcn3d, ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    m = gcn3d.HS_layer(Cin, C, S)
    sd = m.state_dict()
    ref.fill_state_closed_form(sd)
    m.load_state_dict(sd)
    m = m.to(dev)
    xyz = ref.hash_tensor((B, N, 3), seed, 0.1).to(dev)
    fmap0 = torch.relu(ref.hash_tensor((B, N, Cin), seed + 1, 1.0)).to(dev)
    up = ref.hash_tensor((B, N, C), seed + 2, 1.0).to(dev)
    calls = _Calls(ops, monkeypatch)

    def run(diet, rider, hook=None):
        monkeypatch.setattr(ops, "LAUNCH_DIET", diet)
        monkeypatch.setattr(ops, "COLSUM_RIDER", rider)
        monkeypatch.setattr(ops, "_between_launches_hook", hook)
        m.zero_grad(set_to_none=True)
        fmap = fmap0.clone().requires_grad_(True)
        calls.names.clear()
        (m(xyz, fmap, k) * up).sum().backward()
        return [fmap.grad.clone()] + [p.grad.clone() for p in m.parameters()], list(calls.names)
    return run


@pytest.mark.parametrize("B,N,Cin,C,k,S", [(16, 1028, 128, 128, 20, 7), (2, 128, 128, 128, 8, 3)])
def test_hs_layer_backward_rider_order_equals_the_earlier_orders(dev, ref, monkeypatch, B, N, Cin, C, k, S):
    """every gradient of the HS-layer node, deterministic backward: the rider order (pair + column sum, small pair) == the
    separate two-launch chain ahead of the pair == the four-launch chain; also with NaN-filled allocations after the rider"""
    run = _hs_layer_runner(dev, ref, monkeypatch, B, N, Cin, C, k, S)
    four, four_calls = run(False, True)
    two, two_calls = run(True, False)
    new, new_calls = run(True, True)
    hooked, _ = run(True, True, _nan_fill_hook)
    assert "hsp_small_outer_f32" in four_calls and "hsp_wgrad_partial_pair_colsum_f32" not in four_calls
    assert "hsp_colsum_cloud_f32" in two_calls and "hsp_wgrad_partial_pair_f32" in two_calls
    assert two_calls.index("hsp_colsum_cloud_f32") < two_calls.index("hsp_wgrad_partial_pair_f32")
    assert "hsp_wgrad_partial_pair_colsum_f32" in new_calls and "hsp_colsum_cloud_f32" not in new_calls
    assert "hsp_wgrad_partial_pair_f32" not in new_calls
    assert new_calls.index("hsp_wgrad_partial_pair_colsum_f32") < new_calls.index("hsp_small_pair_f32")
    assert len(four) == len(two) == len(new) == len(hooked)
    for a, b, c, d in zip(four, two, new, hooked):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


@pytest.mark.parametrize("B,N,Cin,C,k,S", [(2, 128, 16, 32, 8, 3), (65, 64, 128, 128, 8, 3)])
def test_shapes_the_rider_declines_keep_the_old_launches(dev, ref, monkeypatch, B, N, Cin, C, k, S):
    """C = 32 and B = 65: outside the per-cloud chain's small form, so the node issues the launches it issued before -- no rider
    call -- and the gradients agree with the four-launch chain"""
    run = _hs_layer_runner(dev, ref, monkeypatch, B, N, Cin, C, k, S, seed=71)
    chain = ("hsp_colsum_rows", "hsp_colsum_cloud_f32", "hsp_small_outer_f32", "hsp_small_rows_f32", "hsp_small_pair_f32",
             "hsp_wgrad_partial_pair_f32", "hsp_wgrad_partial_pair_colsum_f32", "hsp_wgrad_f32", "hsp_wgrad_partial_f32")
    old, old_calls = run(False, False)
    new, new_calls = run(True, True)
    assert "hsp_wgrad_partial_pair_colsum_f32" not in new_calls and "hsp_small_pair_f32" not in new_calls
    assert [n for n in new_calls if n in chain] == [n for n in old_calls if n in chain] != []
    for a, b in zip(old, new):
        assert torch.isfinite(a).all() and torch.equal(a, b)
