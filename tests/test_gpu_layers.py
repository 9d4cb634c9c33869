"""GPU parity: fused graph-conv / pooling / gather kernels and the mirrored layers vs the CPU oracle
(oracle/ref_cpu.py, itself pinned to the reference) and the reference's golden outputs.
Tolerance (BASELINE north_star): 1e-4 fp32 on outputs; gradients 1e-4 of the tensor's scale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden

pytestmark = pytest.mark.gpu

ATOL = 1e-4


def close(a, b, tol=ATOL, what=""):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol * scale:.3e}"


def gclose(a, b, what=""):
    """gradient check: 1e-4 of the reference gradient's scale"""
    a = a.detach().cpu().double(); b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item()
    assert err <= 1e-4 * scale, f"{what}: grad max abs err {err:.3e} vs scale {scale:.3e}"


def gclose_kinks(a, b, what="", max_outliers=8):
    """gradient check for the dense-cloud cases: 1e-4 of the gradient's scale everywhere except a handful of entries.
    With N*k*S*C ~ 10^8 arg-max decisions per launch a near-tie is decided differently by two correct fp32 evaluations
    now and then (tools/oracle_sensitivity.py: the CPU oracle disagrees with its own float64 run in the same way); one
    flipped winner moves one summand of one column of dD (3 entries) or between two rows of dfm."""
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs()
    out = int((err > 1e-4 * scale).sum().item())
    assert out <= max_outliers, f"{what}: {out} entries beyond 1e-4 of the scale (max err {err.max().item():.3e}, scale {scale:.3e})"
    assert err.max().item() <= 2e-2 * scale, f"{what}: grad max abs err {err.max().item():.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("B,N,k,S,K", [(2, 128, 8, 3, 16), (1, 257, 20, 7, 128), (3, 64, 8, 7, 512), (9, 40, 4, 2, 8),
                                       (1, 4096, 20, 7, 128)])          # dense cloud (BASELINE configs[3] point count)
def test_rf_surface_fwd_bwd(dev, ref, B, N, k, S, K):
    from hs_pose_amd import ops
    xyz = ref.hash_tensor((B, N, 3), 1, 0.1)
    D = ref.hash_tensor((3, S * K), 2, 1.0).requires_grad_(True)
    up = ref.hash_tensor((B, N, K), 3, 1.0)
    idx = ref.knn_index(xyz, k)
    want = ref.surface_graph_conv(ref.neighbor_dirs(xyz, idx), D, S, K)
    (want * up).sum().backward()
    Dg = D.detach().clone().to(dev).requires_grad_(True)
    got = ops.rf_surface(xyz.to(dev), idx.int().to(dev), Dg, S)
    close(got, want, what="rf_surface out")
    (got * up.to(dev)).sum().backward()
    (gclose_kinks if N >= 2048 else gclose)(Dg.grad, D.grad, "rf_surface dD")


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("B,N,k,S,Cin,C", [(2, 128, 8, 3, 16, 32), (1, 257, 20, 7, 128, 128), (2, 64, 8, 7, 256, 512),
                                           (10, 48, 5, 2, 8, 12), (1, 1028, 20, 7, 32, 128), (1, 4096, 20, 7, 32, 128)])
def test_rf_conv_fwd_bwd(dev, ref, monkeypatch, B, N, k, S, Cin, C, deterministic):
    """both backward forms: column-tile LDS scatter (default) and CSR gather (HSP_DETERMINISTIC=1)"""
    from hs_pose_amd import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", deterministic)
    xyz = ref.hash_tensor((B, N, 3), 11, 0.1)
    x = torch.relu(ref.hash_tensor((B, N, Cin), 12, 1.0))
    W = ref.hash_tensor((Cin, (S + 1) * C), 13, 1.0 / Cin ** 0.5)
    bias = ref.hash_tensor(((S + 1) * C,), 14, 0.1)
    D = ref.hash_tensor((3, S * C), 15, 1.0).requires_grad_(True)
    up = ref.hash_tensor((B, N, C), 16, 1.0)
    idx = ref.knn_index(x, k)
    # oracle: graph conv from an explicit fm leaf so d(fm) can be compared directly
    fm = (x @ W + bias).detach().requires_grad_(True)
    rf = ref.neighbor_dirs(xyz, idx)
    theta = torch.relu(rf @ F.normalize(D, dim=0))
    act = (theta * ref.gather_rows(fm[:, :, C:], idx)).view(B, N, k, S, C).max(dim=2)[0].mean(dim=2)
    want = fm[:, :, :C] + act
    (want * up).sum().backward()
    fmg = fm.detach().clone().to(dev).requires_grad_(True)
    Dg = D.detach().clone().to(dev).requires_grad_(True)
    got = ops.rf_conv(xyz.to(dev), idx.int().to(dev), Dg, fmg, S)
    close(got, want, what="rf_conv out")
    (got * up.to(dev)).sum().backward()
    check = gclose_kinks if N >= 2048 else gclose
    check(fmg.grad, fm.grad, "rf_conv dfm")
    check(Dg.grad, D.grad, "rf_conv dD")


@pytest.mark.parametrize("B,N,C,k,kstride,nq", [(2, 200, 32, 4, 20, 50), (3, 64, 512, 8, 8, None), (1, 1028, 128, 20, 20, None),
                                                (1, 4096, 128, 20, 20, None), (1, 4096, 128, 4, 20, 1024),
                                                (2, 257, 256, 4, 20, 64)])
def test_gather_max_fwd_bwd(dev, ref, B, N, C, k, kstride, nq):
    from hs_pose_amd import ops
    xyz = ref.hash_tensor((B, N, 3), 21, 0.1)
    feat = ref.hash_tensor((B, N, C), 22, 1.0).requires_grad_(True)
    idx = ref.knn_index(xyz, kstride)
    sel = None
    pooled = ref.gather_rows(feat, idx[:, :, :k]).max(dim=2)[0]
    if nq is not None:
        sel = torch.from_numpy(np.argsort(ref.hash_unit(N, 5))[:nq].copy())
        pooled = pooled[:, sel, :]
    up = ref.hash_tensor(tuple(pooled.shape), 23, 1.0)
    (pooled * up).sum().backward()
    fg = feat.detach().clone().to(dev).requires_grad_(True)
    got = ops.gather_max(fg, idx.int().to(dev), k, qsel=None if sel is None else sel.int().to(dev))
    close(got, pooled, tol=0, what="gather_max out")       # pure selection: exact
    (got * up.to(dev)).sum().backward()
    gclose(fg.grad, feat.grad, "gather_max dfeat")


@pytest.mark.parametrize("B,N,C,ties", [(2, 200, 32, False), (16, 1028, 256, False), (3, 64, 512, True), (1, 17, 100, True),
                                        (16, 1, 256, False)])
def test_points_max_fwd_bwd(dev, ref, B, N, C, ties):
    from hs_pose_amd import ops
    feat = ref.hash_tensor((B, N, C), 24, 1.0)
    if ties:                                    # relu-like plateaus: the gradient must go to the FIRST winning row
        feat = (feat * 2).round().clamp_min(0.0)
    feat.requires_grad_(True)
    want = ref.points_max(feat)
    up = ref.hash_tensor(tuple(want.shape), 25, 1.0)
    (want * up).sum().backward()
    if C % 4:
        with torch.no_grad():
            close(ops.points_max(feat.detach().to(dev)), want, tol=0, what="points_max out")
        return
    fg = feat.detach().clone().to(dev).requires_grad_(True)
    got = ops.points_max(fg)
    close(got, want, tol=0, what="points_max out")
    (got * up.to(dev)).sum().backward()
    close(fg.grad, feat.grad, tol=0, what="points_max dfeat")


@pytest.mark.parametrize("deterministic", [False, True])
def test_orl_global_fwd_bwd(dev, ref, monkeypatch, deterministic):
    from hs_pose_amd import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", deterministic)
    B, N, C, k = 3, 257, 64, 20
    xyz = ref.hash_tensor((B, N, 3), 31, 0.1)
    feat = ref.hash_tensor((B, N, C), 32, 1.0).requires_grad_(True)
    want = ref.orl_global(feat, xyz, k)[:, 0, :]
    up = ref.hash_tensor((B, C), 33, 1.0)
    (want * up).sum().backward()
    fg = feat.detach().clone().to(dev).requires_grad_(True)
    got = ops.orl_global(fg, ref.knn_index(xyz, k).int().to(dev), k)
    close(got, want, tol=1e-6, what="orl fg")
    (got * up.to(dev)).sum().backward()
    gclose(fg.grad, feat.grad, "orl dfeat")


@pytest.mark.parametrize("dtype,B,N,C,k", [("f32", 16, 1028, 128, 20), ("f32", 3, 257, 256, 20), ("f32", 2, 2500, 64, 20),
                                          ("bf16", 3, 4096, 128, 20), ("bf16", 2, 1024, 256, 20), ("f32", 2, 300, 64, 8),
                                          ("f32", 1, 128, 64, 20), ("f32", 1, 129, 8, 20), ("f32", 1, 2850, 8, 20),
                                          ("f32", 1, 3000, 8, 20), ("bf16", 1, 5000, 8, 20), ("f32", 9, 257, 128, 20)])
def test_orl_global_slab_form(dev, dtype, B, N, C, k):
    """hsp_orl_global_fwd(_bf16) at the shapes that take the LDS column-slab kernel (k = 20; k = 8 and the 3000-point fp32 cloud,
    whose slab is past the 144 KB limit, keep the chunked form; 128 is the smallest cloud that takes it, B = 9 the plain tile -> XCD map):
    the winning slot is torch.max's (first maximum) for every (point, channel), the mean agrees to fp32 summation-order error.
    Duplicated rows make equal maxima common (the tiled-cloud case)."""
    from hs_pose_amd import ops
    g = torch.Generator().manual_seed(N + C)
    xyz = (torch.randn(B, N, 3, generator=g) * 0.05).to(dev)
    feat = torch.randn(B, N, C, generator=g)
    feat[:, N // 2:] = feat[:, : N - N // 2].clone()            # exact duplicates among the neighbours' values
    feat = feat.to(dev)
    idx = ops.knn(xyz, k)
    if dtype == "bf16":
        fb = feat.bfloat16()
        fg, arg = ops._orl_fwd_raw(fb, idx, k)
        vals = fb.float()
    else:
        fg, arg = ops._orl_fwd_raw(feat, idx, k)
        vals = feat
    nb = torch.gather(vals.unsqueeze(1).expand(B, N, N, C), 2, idx.long().unsqueeze(-1).expand(B, N, k, C)) if N <= 300 else None
    if nb is None:                                               # (B, N, k, C) gather without the (B, N, N, C) view
        nb = vals[torch.arange(B, device=dev)[:, None, None], idx.long()]
    mx, am = nb.max(dim=2)
    first = (nb == mx.unsqueeze(2)).float().argmax(dim=2)        # first slot holding the maximum
    assert torch.equal(arg.long(), first)
    want = mx.double().mean(dim=1)
    assert (fg.double() - want).abs().max().item() <= 2e-6 * want.abs().max().item() + 1e-7


@pytest.mark.parametrize("shared", [False, True])
def test_gather_rows_fwd_bwd(dev, ref, shared):
    from hs_pose_amd import ops
    B, Nsrc, Nq, C = 3, 64, 300, 48
    feat = ref.hash_tensor((B, Nsrc, C), 41, 1.0).requires_grad_(True)
    if shared:
        idx = torch.from_numpy((ref.hash_unit(Nq, 42) * Nsrc).astype(np.int64))
        want = feat[:, idx, :]
    else:
        idx = torch.from_numpy((ref.hash_unit(B * Nq, 42) * Nsrc).astype(np.int64)).view(B, Nq)
        want = ref.gather_rows(feat, idx.unsqueeze(-1)).squeeze(2)
    up = ref.hash_tensor((B, Nq, C), 43, 1.0)
    (want * up).sum().backward()
    fg = feat.detach().clone().to(dev).requires_grad_(True)
    got = ops.gather_rows(fg, idx.int().to(dev))
    close(got, want, tol=0, what="gather_rows out")
    (got * up.to(dev)).sum().backward()
    gclose(fg.grad, feat.grad, "gather_rows dfeat")
    # xyz rows (C = 3, scalar path)
    v = ref.hash_tensor((B, Nsrc, 3), 44, 1.0)
    got = ops.gather_rows(v.to(dev), idx.int().to(dev))
    want = v[:, idx, :] if shared else ref.gather_rows(v, idx.unsqueeze(-1)).squeeze(2)
    close(got, want, tol=0, what="gather_rows xyz")


def _load_state(mod, ref):
    sd = mod.state_dict()
    ref.fill_state_closed_form(sd)
    return sd


def test_surface_layer_golden(dev, ref):
    """HSlayer_surface end to end vs the reference's stored output + parameter gradients."""
    from hs_pose_amd import gcn3d
    for name, full in (("surface_small", True), ("surface_full", False)):
        g = golden(name)
        K, S, N, k, B, seed = (int(v) for v in g["meta"])
        m = gcn3d.HSlayer_surface(K, S)
        _load_state(m, ref)
        m = m.to(dev)
        xyz = ref.hash_tensor((B, N, 3), seed, 0.1).to(dev)
        up = ref.hash_tensor((B, N, K), seed + 1, 1.0).to(dev)
        out = m(xyz, k)
        if full:
            close(out, g["out"], what=name)
        else:
            close(out.reshape(-1)[::997], g["out_sample"], what=name)
            close(out.mean(dim=(0, 1)), g["out_chmean"], what=name + " chmean")
        (out * up).sum().backward()
        for pn, p in m.named_parameters():
            gclose(p.grad, g["grad." + pn], f"{name} grad {pn}")


def test_hs_layer_golden(dev, ref):
    from hs_pose_amd import gcn3d, ops
    for name, full in (("hs_small", True), ("hs_full_128", False), ("hs_full_512", False)):
        g = golden(name)
        Cin, Cout, S, N, k, B, seed = (int(v) for v in g["meta"])
        m = gcn3d.HS_layer(Cin, Cout, S)
        _load_state(m, ref)
        m = m.to(dev)
        xyz = ref.hash_tensor((B, N, 3), seed, 0.1).to(dev)
        fmap = torch.relu(ref.hash_tensor((B, N, Cin), seed + 2, 1.0)).to(dev).requires_grad_(True)
        up = ref.hash_tensor((B, N, Cout), seed + 1, 1.0).to(dev)
        # feature-space neighbours: bit-exact with the reference
        assert np.array_equal(ops.knn(fmap, k).cpu().numpy(), g["knn_idx"].astype(np.int32)), name
        out = m(xyz, fmap, k)
        (out * up).sum().backward()
        if full:
            close(out, g["out"], what=name)
            gclose(fmap.grad, g["grad_fmap"], name + " dfmap")
            for pn, p in m.named_parameters():
                gclose(p.grad, g["grad." + pn], f"{name} grad {pn}")
        else:
            close(out.reshape(-1)[::997], g["out_sample"], what=name)
            close(out.mean(dim=(0, 1)), g["out_chmean"], what=name + " chmean")
            gclose(fmap.grad.reshape(-1)[::997], g["grad_fmap_sample"], name + " dfmap")
            for pn, p in m.named_parameters():
                want = g["gradsample." + pn]
                scale = float(g["gradnorm." + pn][0])
                err = (p.grad.reshape(-1)[::499].cpu().double() - torch.from_numpy(want).double()).abs().max().item()
                assert err <= 1e-4 * max(np.abs(want).max(), scale / max(p.numel(), 1) ** 0.5, 1e-12), (name, pn, err)


def test_pool_layer_golden(dev, ref):
    """Pool_layer consumes the CPU generator like the reference: seed 1 -> same kept points."""
    from hs_pose_amd import gcn3d
    g = golden("pool_1028")
    xyz = ref.hash_tensor((2, 1028, 3), 61, 0.1).to(dev)
    fmap = ref.hash_tensor((2, 1028, 32), 62, 1.0).to(dev)
    pool = gcn3d.Pool_layer(4, 4)
    torch.manual_seed(1)
    vp, fp = pool(xyz, fmap)
    close(vp, g["v_pool"], tol=0, what="v_pool")
    close(fp, g["f_pool"], tol=0, what="f_pool")
    # second draw of the same generator stream == the reference's pool_2 draw
    assert np.array_equal(torch.randperm(257)[:64].numpy(), g["perm_seed1_b"].astype(np.int64))


def test_reference_api_helpers(dev, ref):
    """indexing_neighbor_new / get_neighbor_direction_norm / get_ORL_global keep the reference's
    shapes and values (gcn3d.py:39-59, :211-218)."""
    from hs_pose_amd import gcn3d
    B, N, C, k = 2, 100, 16, 6
    xyz = ref.hash_tensor((B, N, 3), 71, 0.1)
    feat = ref.hash_tensor((B, N, C), 72, 1.0)
    idx = ref.knn_index(xyz, k)
    got = gcn3d.indexing_neighbor_new(feat.to(dev), idx.to(dev))
    close(got, ref.gather_rows(feat, idx), tol=0)
    close(gcn3d.get_neighbor_direction_norm(xyz.to(dev), idx.to(dev)), ref.neighbor_dirs(xyz, idx), tol=1e-6)
    close(gcn3d.get_ORL_global(feat.to(dev), xyz.to(dev), k), ref.orl_global(feat, xyz, k), tol=1e-6)
    rf, ni = gcn3d.get_receptive_fields(k, xyz.to(dev), feature_map=feat.to(dev), mode='RF-F')
    assert np.array_equal(ni.cpu().numpy(), ref.knn_index(feat, k).numpy())
    assert rf.shape == (B, N, k, 3)


@pytest.mark.parametrize("B,Nq,Nsrc,k,kstride", [(2, 100, 100, 8, 8), (3, 257, 257, 20, 20), (1, 1028, 1028, 4, 20), (2, 50, 300, 5, 6)])
def test_rev_build(dev, ref, B, Nq, Nsrc, k, kstride):
    """reverse-edge index: every edge appears exactly once, in its target's list, lists ascending."""
    from hs_pose_amd import ops
    idx = torch.from_numpy((ref.hash_unit(B * Nq * kstride, 7) * Nsrc).astype(np.int32)).view(B, Nq, kstride)
    idx[:, :, 0] = 3                                   # a hub: every query lists row 3
    off, edge = ops.rev_index(idx.to(dev), k, Nsrc)
    off, edge = off.cpu().numpy(), edge.cpu().numpy()
    inp = idx.numpy()
    for b in range(B):
        assert off[b, 0] == 0 and off[b, -1] == Nq * k and (np.diff(off[b]) >= 0).all()
        assert np.array_equal(np.sort(edge[b]), np.arange(Nq * k))
        tgt = inp[b, edge[b] // k, edge[b] % k]
        assert np.array_equal(tgt, np.repeat(np.arange(Nsrc), np.diff(off[b])))
        for m in (0, 3, Nsrc - 1):
            lst = edge[b, off[b, m]:off[b, m + 1]]
            assert (np.diff(lst) > 0).all()


def test_backward_is_bit_reproducible(dev, ref, monkeypatch):
    """HSP_DETERMINISTIC mode: gather-form backward has a fixed summation order -> identical bits."""
    from hs_pose_amd import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    B, N, k, S, C = 2, 257, 20, 7, 128
    xyz = ref.hash_tensor((B, N, 3), 11, 0.1).to(dev)
    fm = ref.hash_tensor((B, N, (S + 1) * C), 12, 1.0).to(dev)
    D = ref.hash_tensor((3, S * C), 15, 1.0).to(dev)
    up = ref.hash_tensor((B, N, C), 16, 1.0).to(dev)
    idx = ops.knn(xyz, k)
    outs = []
    for _ in range(2):
        f = fm.clone().requires_grad_(True)
        d = D.clone().requires_grad_(True)
        (ops.rf_conv(xyz, idx, d, f, S) * up).sum().backward()
        g2 = ref.hash_tensor((B, C), 17, 1.0).to(dev)
        ff = fm[:, :, :C].clone().requires_grad_(True)
        (ops.orl_global(ff, idx, k) * g2).sum().backward()
        outs.append((f.grad.clone(), d.grad.clone(), ff.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("K,M,N,lda_pad,ldc_pad", [(16448, 128, 1024, 0, 0), (4112, 256, 2048, 0, 0), (1024, 512, 512, 0, 512),
                                                   (1000, 64, 64, 64, 0), (4113, 128, 128, 0, 128), (37, 64, 128, 0, 0)])
def test_wgrad_gemm(dev, ref, monkeypatch, K, M, N, lda_pad, ldc_pad):
    """split-K MFMA weight-gradient GEMM vs fp64: A^T B, fused column sum, strided operands / output."""
    from hs_pose_amd import ops
    Afull = ref.hash_tensor((K, M + lda_pad), 1, 1.0).to(dev)
    B = ref.hash_tensor((K, N), 2, 1.0).to(dev)
    A = Afull[:, :M]
    outfull = torch.full((M, N + ldc_pad), 7.0, device=dev)
    out, cs = ops.wgrad(A, B, out=outfull[:, ldc_pad:], colsum=True)
    want = (A.double().t() @ B.double())
    scale = want.abs().max().item()
    assert (out.double() - want).abs().max().item() <= 2e-6 * scale * max(1.0, (K / 1000) ** 0.5)
    assert (cs.double() - B.double().sum(0)).abs().max().item() <= 2e-6 * B.double().sum(0).abs().max().item() + 1e-4
    if ldc_pad:
        assert (outfull[:, :ldc_pad] == 7.0).all()          # the neighbouring column block is untouched
    # bit-reproducible (fixed-order fold of the K slices)
    out2 = ops.wgrad(A, B)
    assert torch.equal(out2, out.contiguous())


@pytest.mark.parametrize("K,M,N,pad_nan", [(16448, 1286, 1024, True), (5000, 1289, 1024, False), (4113, 771, 512, True),
                                            (700, 130, 512, False)])
def test_wgrad_ragged_m(dev, ref, K, M, N, pad_nan):
    """the heads' first-layer weight gradients (K = 1286 / 1289 / 771 input columns: PoseR.py:27, PoseTs.py:32, FaceRecon.py:38,116)
    on the x3 kernel: A's rows on a 16-byte pitch >= ceil4(M), the last row tile ragged.  vs fp64; the pad columns (whatever
    they hold) reach no output; output rows past M are never written."""
    from hs_pose_amd import ops
    pitch = (M + 3) // 4 * 4
    if pitch == M:
        pitch += 4
    Afull = ref.hash_tensor((K, pitch), 21, 1.0).to(dev)
    if pad_nan:
        Afull[:, M:] = float("nan")
    A = Afull[:, :M]
    Bm = ref.hash_tensor((K, N), 22, 1.0).to(dev)
    import ctypes
    from hs_pose_amd._lib import lib
    plan = (ctypes.c_int * 4)()                        # the ragged plan: the x3 form, and M off the 64-wide tiles of every other
    assert M % 64 and ops._wgrad_entry_of(A, Bm, Bm) == "hsp_wgrad"
    assert lib().hsp_wgrad_plan(M, N, K, 4, 1, pitch, N, 0, plan) == 0 and plan[0] == 3         # HSP_WGRAD_FORM_X3
    guard = torch.full((M + 8, N), 7.0, device=dev)
    out, cs = ops.wgrad(A, Bm, out=guard[:M], colsum=True)
    want = A.double().t() @ Bm.double()
    scale = want.abs().max().item()
    assert torch.isfinite(out).all()
    assert (out.double() - want).abs().max().item() <= 2e-6 * scale * max(1.0, (K / 1000) ** 0.5)
    assert (cs.double() - Bm.double().sum(0)).abs().max().item() <= 2e-6 * Bm.double().sum(0).abs().max().item() + 1e-4
    assert (guard[M:] == 7.0).all()
    out2 = ops.wgrad(A, Bm)
    assert torch.equal(out2, out)
    # inside a WgradBatch the fold is left pending and runs at the exit: same bits
    out3 = torch.empty(M, N, device=dev)
    with ops.WgradBatch():
        ops.wgrad(A, Bm, out=out3)
    assert torch.equal(out3, out)


@pytest.mark.parametrize("Cin,Cout", [(128, 3), (128, 30), (1286, 1024), (771, 512)])
def test_linear_rows_backward_own_kernels(dev, ref, Cin, Cout):
    """linear_rows' backward on the shapes that used to fall to the BLAS library (thin per-point outputs, ragged input widths):
    weight / bias / input gradients vs fp64"""
    from hs_pose_amd import ops
    R = 16448
    pitch = (Cin + 3) // 4 * 4
    xfull = ref.hash_tensor((R, pitch), 31, 1.0).to(dev)
    x = xfull[:, :Cin].requires_grad_(True) if pitch != Cin else xfull.requires_grad_(True)
    w = (ref.hash_tensor((Cout, Cin), 32, 1.0) * 0.05).to(dev).requires_grad_(True)
    b = ref.hash_tensor((Cout,), 33, 1.0).to(dev).requires_grad_(True)
    up = ref.hash_tensor((R, Cout), 34, 1.0).to(dev)
    timer = ops.KernelTimer()
    prev = ops.set_timer(timer)
    try:
        y = ops.linear_rows(x, w, b)
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), up)
    finally:
        ops.set_timer(prev)
    torch.cuda.synchronize()
    assert any(r[0].startswith("hsp_wgrad") for r in timer.records)
    xd, wd, ud = x.detach().double(), w.detach().double(), up.double()
    for got, want in ((y, xd @ wd.t() + b.detach().double()), (gw, ud.t() @ xd), (gb, ud.sum(0)), (gx, ud @ wd)):
        sc = want.abs().max().item()
        assert (got.double() - want).abs().max().item() <= 1e-5 * sc, (Cin, Cout)


@pytest.mark.parametrize("R,Cin,Cout", [(16448, 1024, 256), (16448, 512, 512), (2100, 256, 128)])
def test_linear_rows_leaves_the_batchnorm_first_pass(dev, ref, R, Cin, Cout):
    """linear_rows(..., bn_partials=True) + bn_relu(..., partial=) == linear_rows + bn_relu (the BatchNorm statistics from the
    product's epilogue against the two-pass kernel): output, running statistics, input / weight gradients"""
    from hs_pose_amd import ops
    x = ref.hash_tensor((R, Cin), 71, 1.0).to(dev)
    w = (ref.hash_tensor((Cout, Cin), 72, 1.0) * 0.05).to(dev)
    b = (ref.hash_tensor((Cout,), 73, 1.0) * 3.0).to(dev)               # |mean| >> std for some columns
    up = ref.hash_tensor((R, Cout), 74, 1.0).to(dev)
    res = []
    for fused in (False, True):
        bn = torch.nn.BatchNorm1d(Cout).to(dev).train()
        xx, ww, bb = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        if fused:
            y, part = ops.linear_rows(xx, ww, bb, bn_partials=True)
            assert (part.numel() > 0) == (R >= 16448)            # (too few tiles for the x3 kernel: an empty buffer, the plain path)
            out = ops.bn_relu(y, bn, partial=part)
        else:
            out = ops.bn_relu(ops.linear_rows(xx, ww, bb), bn)
        # (the Linear's bias gradient is identically zero behind a BatchNorm: rounding noise, not compared)
        g = torch.autograd.grad(out, (xx, ww, bn.weight, bn.bias), up)
        res.append((out.detach(), bn.running_mean.clone(), bn.running_var.clone(), *g))
    for a, c in zip(*res):
        sc = max(a.abs().max().item(), 1e-6)
        assert (a - c).abs().max().item() <= 2e-5 * sc


@pytest.mark.parametrize("B,N", [(16, 1028), (5, 300)])
def test_cloud_cat_linear(dev, ref, B, N):
    """the face head's first Conv1d on cat[f_global over the cloud, h, xyz] (FaceRecon.py:113-117) as a K = 259 product with a
    per-cloud bias: output and the gradients of f_global, h, the (512, 771) weight and the bias vs the fp64 composition"""
    from hs_pose_amd import ops
    R, Cg, Cx, Cout = B * N, 512, 256, 512
    fg = ref.hash_tensor((B, Cg), 81, 1.0).to(dev).requires_grad_(True)
    x = ref.hash_tensor((R, Cx), 82, 1.0).to(dev).requires_grad_(True)
    xyz = (ref.hash_tensor((B, N, 3), 83, 1.0) * 0.3).to(dev)
    W = (ref.hash_tensor((Cout, Cg + Cx + 3), 84, 1.0) * 0.04).to(dev).requires_grad_(True)
    b = ref.hash_tensor((Cout,), 85, 1.0).to(dev).requires_grad_(True)
    up = ref.hash_tensor((R, Cout), 86, 1.0).to(dev)
    assert ops.cloud_cat_linear_ok(fg, x, xyz, W)
    y = ops.cloud_cat_linear(fg, x, xyz, W, b)
    got = torch.autograd.grad(y, (fg, x, W, b), up)
    fd, xd, Wd, bd = (t.detach().double().requires_grad_(True) for t in (fg, x, W, b))
    full = torch.cat([fd.unsqueeze(1).expand(-1, N, -1).reshape(R, Cg), xd, xyz.reshape(R, 3).double()], dim=1)
    want_y = full @ Wd.t() + bd
    want = torch.autograd.grad(want_y, (fd, xd, Wd, bd), up.double())
    assert (y.double() - want_y).abs().max().item() <= 1e-5 * want_y.abs().max().item()
    for a, c, name in zip(got, want, ("f_global", "x", "W", "b")):
        assert a.shape == c.shape, name
        assert (a.double() - c).abs().max().item() <= 2e-5 * c.abs().max().item(), name


@pytest.mark.parametrize("B,N", [(16, 1028), (3, 700)])
def test_fan_linear_rows(dev, ref, B, N):
    """the first layers of every consumer of feat's rows as one node (PoseR.py:27 x2, PoseTs.py:32 on cat[feat, xyz],
    FaceRecon.py:38): outputs, the summed input gradient (accumulated in the products' epilogues), weight / bias gradients
    incl. the coordinate columns of the (1024, 1289) weight -- vs fp64; one upstream gradient missing (an unused head)"""
    from hs_pose_amd import ops
    R, K = B * N, 1286
    xfull = ref.hash_tensor((R, 1288), 41, 1.0).to(dev)
    xfull[:, K:] = 0.0
    x = xfull[:, :K].requires_grad_(True)
    xyz = (ref.hash_tensor((B, N, 3), 42, 1.0) * 0.3).to(dev)
    shapes = [(1024, K), (1024, K), (1024, K + 3), (512, K)]
    ws = [(ref.hash_tensor(sh, 43 + i, 1.0) * 0.03).to(dev).requires_grad_(True) for i, sh in enumerate(shapes)]
    bs = [ref.hash_tensor((sh[0],), 53 + i, 1.0).to(dev).requires_grad_(True) for i, sh in enumerate(shapes)]
    ups = [ref.hash_tensor((R, sh[0]), 63 + i, 1.0).to(dev) for i, sh in enumerate(shapes)]
    assert ops.fan_linear_rows_ok(x, xyz, ws)
    outs = ops.fan_linear_rows(x, xyz, list(zip(ws, bs)))
    ys = [y for y, _ in outs]
    for (y, part), w in zip(outs, ws):
        # the BatchNorm first pass left by the product: row 0 = the shift, then per row tile the shifted column sums
        assert part.numel() and part.shape[1] == w.shape[0] and (part.shape[0] - 1) % 2 == 0
        tiles = (part.shape[0] - 1) // 2
        sums = part[1:].view(tiles, 2, -1).double().sum(0)
        d = y.detach().double() - part[0].double()
        assert (sums[0] - d.sum(0)).abs().max().item() <= 1e-5 * d.abs().sum(0).max().item()
        assert (sums[1] - (d * d).sum(0)).abs().max().item() <= 1e-5 * (d * d).sum(0).max().item()
    xd = x.detach().double()
    xcat = torch.cat([xd, xyz.reshape(R, 3).double()], dim=1)
    want_gx = torch.zeros(R, K, dtype=torch.float64, device=dev)
    for y, w, b, up in zip(ys, ws, bs, ups):
        src = xd if w.shape[1] == K else xcat
        want = src @ w.detach().double().t() + b.detach().double()
        assert (y.double() - want).abs().max().item() <= 1e-5 * want.abs().max().item()
        want_gx += (up.double() @ w.detach().double())[:, :K]
    grads = torch.autograd.grad(ys, [x] + ws + bs, ups)
    gx, gws, gbs = grads[0], grads[1:5], grads[5:]
    assert (gx.double() - want_gx).abs().max().item() <= 1e-5 * want_gx.abs().max().item()
    for gw, gb, w, up in zip(gws, gbs, ws, ups):
        src = xd if w.shape[1] == K else xcat
        want_w = up.double().t() @ src
        assert gw.shape == w.shape
        assert (gw.double() - want_w).abs().max().item() <= 1e-5 * want_w.abs().max().item()
        assert (gb.double() - up.double().sum(0)).abs().max().item() <= 1e-5 * up.double().sum(0).abs().max().item() + 1e-4
    # a consumer of x OUTSIDE the group: its gradient is added to the group's once that is complete
    ys = [y for y, _ in ops.fan_linear_rows(x, xyz, list(zip(ws, bs)))]
    other = x * 2.0
    (gx3,) = torch.autograd.grad(ys + [other], [x], ups + [torch.ones_like(other)])
    assert (gx3.double() - (want_gx + 2.0)).abs().max().item() <= 1e-5 * want_gx.abs().max().item()
    # one consumer without a gradient (its head's loss switched off): the chain skips it
    ys = [y for y, _ in ops.fan_linear_rows(x, xyz, list(zip(ws, bs)))]
    (gx2,) = torch.autograd.grad([ys[0], ys[2], ys[3]], [x], [ups[0], ups[2], ups[3]])
    want2 = sum((ups[i].double() @ ws[i].detach().double())[:, :K] for i in (0, 2, 3))
    assert (gx2.double() - want2).abs().max().item() <= 1e-5 * want2.abs().max().item()


@pytest.mark.parametrize("B,N,C,relu", [(16, 1028, 128, True), (2, 257, 256, True), (3, 100, 64, False)])
def test_bn_relu_fused(dev, ref, B, N, C, relu):
    """fused train-mode BatchNorm1d+ReLU vs torch's module on the same rows: output, input / affine
    gradients, running statistics and num_batches_tracked."""
    from hs_pose_amd import ops
    x = (ref.hash_tensor((B, N, C), 5, 1.0) * 0.3 + ref.hash_tensor((1, 1, C), 6, 2.0)).to(dev)   # |mean| >> std
    up = ref.hash_tensor((B, N, C), 7, 1.0).to(dev)
    mods = []
    for _ in range(2):
        bn = torch.nn.BatchNorm1d(C).to(dev)
        with torch.no_grad():
            bn.weight.copy_(ref.hash_tensor((C,), 8, 0.3).to(dev) + 1.0)
            bn.bias.copy_(ref.hash_tensor((C,), 9, 0.2).to(dev))
        mods.append(bn)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    got = ops.bn_relu(a, mods[0], relu=relu)
    want = mods[1](b.reshape(B * N, C)).view(B, N, C)
    if relu:
        want = torch.relu(want)
    close(got, want, tol=2e-5, what="bn_relu out")
    (got * up).sum().backward()
    (want * up).sum().backward()
    gclose(a.grad, b.grad, "bn_relu dx")
    gclose(mods[0].weight.grad, mods[1].weight.grad, "bn_relu dgamma")
    gclose(mods[0].bias.grad, mods[1].bias.grad, "bn_relu dbeta")
    close(mods[0].running_mean, mods[1].running_mean, tol=1e-5, what="running_mean")
    close(mods[0].running_var, mods[1].running_var, tol=1e-5, what="running_var")
    assert int(mods[0].num_batches_tracked) == 1
    # eval mode goes through the module itself
    mods[0].eval(); mods[1].eval()
    close(ops.bn_relu(x, mods[0], relu=relu), torch.relu(mods[1](x.reshape(-1, C))).view_as(x) if relu else mods[1](x.reshape(-1, C)).view_as(x), tol=2e-5)


def test_rf_conv_backward_fwin_stream_equals_fm_gather(dev, ref):
    """the column-tile backward takes the winners' support values either from the forward's fwin stream (large
    layers) or by gathering fm (small ones): same numbers, so the same gradients up to LDS-add order."""
    from hs_pose_amd import ops
    from hs_pose_amd.ops import _p, _run, _stream, _ws
    from hs_pose_amd._lib import lib
    B, N, k, S, C = 2, 300, 8, 7, 64
    SC = S * C
    xyz = ref.hash_tensor((B, N, 3), 501, 0.5).to(dev)
    fm = ref.hash_tensor((B, N, (S + 1) * C), 502, 1.0).to(dev)
    dirs = ref.hash_tensor((3, SC), 503, 1.0).to(dev)
    g = ref.hash_tensor((B, N, C), 504, 1.0).to(dev)
    idx = ops.knn(xyz, k)
    out = torch.empty(B, N, C, device=dev)
    arg = torch.empty(B, N, SC, dtype=torch.uint16, device=dev)
    fwin = torch.empty(B, N, SC, device=dev)
    _run("hsp_rf_conv_fwd", (_p(xyz), _p(idx), _p(dirs), _p(fm), B, N, k, S, C, _p(out), _p(arg), _p(fwin), _stream()))
    want = torch.gather(fm[:, :, C:], 1, arg.to(torch.int64))                 # fm[b, argrow[b,i,j], C+j]
    assert torch.equal(fwin, want)
    wsb = lib().hsp_rf_bwd_scatter_workspace_bytes(B, SC)
    res = []
    for a_fm, a_fw in ((fm, None), (None, fwin)):
        gfm = torch.empty(B, N, (S + 1) * C, device=dev)
        gd = torch.empty(3, SC, device=dev)
        ws = _ws(wsb, dev)
        _run("hsp_rf_conv_bwd_scatter", (_p(xyz), _p(dirs), _p(a_fm), _p(a_fw), _p(arg), _p(g), B, N, S, C, _p(gfm), _p(gd),
                                         _p(ws), wsb, _stream()))
        res.append((gfm, gd))
    # the tile accumulates in fixed point (integer LDS adds: exact, order-independent): both forms route the same terms
    assert torch.equal(res[0][0], res[1][0])
    assert torch.allclose(res[0][1], res[1][1], rtol=1e-5, atol=1e-5)
    # ... and the same launch twice gives the same bits
    gfm2 = torch.empty(B, N, (S + 1) * C, device=dev)
    gd2 = torch.empty(3, SC, device=dev)
    _run("hsp_rf_conv_bwd_scatter", (_p(xyz), _p(dirs), _p(None), _p(fwin), _p(arg), _p(g), B, N, S, C, _p(gfm2), _p(gd2),
                                     _p(_ws(wsb, dev)), wsb, _stream()))
    assert torch.equal(gfm2, res[1][0]) and torch.equal(gd2, res[1][1])
    # round 3: the stream is always wanted (the backward's 4-byte gathers cost more than the forward's extra store)
    assert lib().hsp_rf_conv_wants_fwin(1028, 7, 128) == 1 and lib().hsp_rf_conv_wants_fwin(64, 7, 512) == 1


@pytest.mark.parametrize("B,Ns,Nq,C,W", [(3, 37, 150, 64, 200), (2, 64, 1028, 512, 1286), (2, 257, 1028, 256, 1286)])
def test_gather_rows_bwd_csr_matches_scatter(dev, ref, B, Ns, Nq, C, W):
    """nearest-up-sampling backward, gather form over the reverse map == the column-tile scatter form == index_add."""
    from hs_pose_amd import ops
    from hs_pose_amd.ops import _p, _run, _stream
    g_full = ref.hash_tensor((B, Nq, W), 610 + C, 1.0).to(dev)
    gs = g_full[:, :, 6:6 + C]                                   # a column block of a wider gradient (8-byte aligned)
    idx = torch.from_numpy((ref.hash_unit(B * Nq, 611) * Ns).astype(np.int32)).view(B, Nq).to(dev)
    idx[:, :5] = 0                                               # a small hub
    off, edge = ops.rev_index(idx, 1, Ns)
    a = torch.empty(B, Ns, C, device=dev)
    b_ = torch.empty(B, Ns, C, device=dev)
    _run("hsp_gather_rows_bwd_csr", (_p(gs), W, _p(off), _p(edge), B, Ns, Nq, C, _p(a), _stream()))
    _run("hsp_gather_rows_bwd", (_p(gs), W, _p(idx), 0, B, Ns, Nq, C, _p(b_), _stream()))
    want = torch.zeros(B, Ns, C, device=dev)
    for bb in range(B):
        want[bb].index_add_(0, idx[bb].long(), gs[bb])
    assert torch.allclose(a, want, rtol=1e-5, atol=1e-5) and torch.allclose(b_, want, rtol=1e-5, atol=1e-5)
    a2 = torch.empty_like(a)
    _run("hsp_gather_rows_bwd_csr", (_p(gs), W, _p(off), _p(edge), B, Ns, Nq, C, _p(a2), _stream()))
    assert torch.equal(a, a2)                                    # fixed summation order


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("align", [8, 1])
def test_assemble_feat_pitched_rows(dev, ref, monkeypatch, dtype, align):
    """feat assembly (FaceRecon.py:108-114: direct levels, nearest-up-sampled coarse levels, one-hot category columns) into
    rows padded to a 16-byte pitch (align 8: a (B,N,W) view of a wider buffer, 16-byte kernel path) and dense (align 1):
    both equal the torch cat / gather composition exactly (a copy kernel), and the backward returns the column blocks."""
    from hs_pose_amd import ops
    monkeypatch.setattr(ops, "FEAT_PITCH_ALIGN", align)
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    B, N, N1, N2 = 3, 1028, 257, 64
    h = lambda shape, seed: ref.hash_tensor(shape, seed, 1.0).to(dev)
    a0, a1 = h((B, N, 128), 1).to(dt).requires_grad_(True), h((B, N, 128), 2).to(dt).requires_grad_(True)
    c2, c3 = h((B, N1, 256), 3).to(dt).requires_grad_(True), h((B, N1, 256), 4).to(dt).requires_grad_(True)
    c4 = h((B, N2, 512), 5).to(dt).requires_grad_(True)
    g = torch.Generator().manual_seed(3)
    near1 = torch.randint(0, N1, (B, N), generator=g).int().to(dev)
    near2 = torch.randint(0, N2, (B, N), generator=g).int().to(dev)
    one_hot = torch.zeros(B, 6, device=dev).scatter_(1, torch.tensor([[1], [4], [0]], device=dev), 1.0)
    feat = ops.assemble_feat([(a0, None, 0), (a1, None, 0), (c2, near1, 1), (c3, near1, 1), (c4, near2, 1), (one_hot, None, 2)])
    assert feat.shape == (B, N, 1286) and feat.dtype == dt
    assert feat.stride(1) == (1288 if align == 8 else 1286) and feat.stride(2) == 1
    gat = lambda c, near: torch.gather(c, 1, near.long().unsqueeze(-1).expand(-1, -1, c.shape[2]))
    want = torch.cat([a0, a1, gat(c2, near1), gat(c3, near1), gat(c4, near2), one_hot.to(dt).unsqueeze(1).expand(-1, N, -1)], dim=2)
    assert torch.equal(feat, want)
    rows = feat.reshape(B * N, 1286)
    assert rows.data_ptr() == feat.data_ptr()                   # the heads take the strided rows: no copy
    up = h((B, N, 1286), 9).to(dt)
    feat.backward(up)
    assert torch.equal(a1.grad, up[:, :, 128:256])
    ref_c4 = torch.zeros(B, N2, 512, device=dev, dtype=torch.float32)
    ref_c4.scatter_add_(1, near2.long().unsqueeze(-1).expand(-1, -1, 512), up[:, :, 768:1280].float())
    tol = 1e-5 if dtype == "f32" else 2.0 ** -7
    assert float((c4.grad.float() - ref_c4).abs().max()) <= tol * max(1.0, float(ref_c4.abs().max()))


# ---- round 3: two-consumer nodes and the BatchNorm first pass from the producing product ---------------------------------------

def test_add_relu_bwd_kernel(dev):
    """hsp_add_relu_bwd: (ga + gb) * [y > 0] with gb a column block of a wider, 8-byte pitched tensor; against torch"""
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib, check
    g_ = torch.Generator().manual_seed(5)
    R, C = 1000, 128
    y = torch.randn(R, C, generator=g_).to(dev)
    ga = torch.randn(R, C, generator=g_).to(dev)
    wide = torch.randn(R, 1286, generator=g_).to(dev)
    gb = wide[:, 130:130 + C]                                  # pitch 1286 (even), 8-byte aligned, not 16
    out = torch.empty(R, C, device=dev)
    check(lib().hsp_add_relu_bwd(ga.data_ptr(), C, gb.data_ptr(), 1286, y.data_ptr(), R, C, out.data_ptr(), ops._stream()), "add_relu_bwd")
    assert torch.equal(out, (ga + gb) * (y > 0))
    check(lib().hsp_add_relu_bwd(ga.data_ptr(), C, None, 0, y.data_ptr(), R, C, out.data_ptr(), ops._stream()), "add_relu_bwd")
    assert torch.equal(out, ga * (y > 0))


@pytest.mark.parametrize("R,C", [(4112, 256), (16448, 128), (300, 64)])
def test_bn_relu_fork_equals_plain(dev, R, C):
    """the forked BatchNorm node (one output per consumer, both gradients -- one a pitched column block -- added inside the
    backward kernels) gives the gradients of the plain node fed with their sum, bit for bit"""
    from hs_pose_amd import ops
    g_ = torch.Generator().manual_seed(R + C)
    x0 = torch.randn(R, C, generator=g_).to(dev) * 2 + 3
    d1 = torch.randn(R, C, generator=g_).to(dev)
    wide = torch.randn(R, C + 70, generator=g_).to(dev)
    d2 = wide[:, 6:6 + C]
    res = []
    for fork in (False, True):
        bn = torch.nn.BatchNorm1d(C).to(dev).train()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
        bn.weight.data.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.data.copy_(torch.linspace(-0.5, 0.5, C))
        x = x0.clone().requires_grad_(True)
        if fork:
            ya, yb = ops.bn_relu(x, bn, fork=True)
            assert ya.data_ptr() == yb.data_ptr()
            torch.autograd.backward([ya, yb], [d1, d2])
        else:
            ya = ops.bn_relu(x, bn)
            ya.backward(d1 + d2)
        res.append((ya.detach().clone(), x.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone(), bn.running_var.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N,Cin,C", [(16, 1028, 128, 128), (16, 257, 128, 256), (3, 300, 64, 128)])
def test_out_product_leaves_batchnorm_first_pass(dev, B, N, Cin, C):
    """hsp_gemm_x3_bn_f32 + hsp_bn_relu_fwd_partials: the layer's out product with the BatchNorm statistics' first pass in its
    epilogue against the plain product followed by the three-launch BatchNorm (mean / invstd / y to 1e-5 of scale: the shifted
    sums are cut into other chunks)"""
    from hs_pose_amd import ops
    g_ = torch.Generator().manual_seed(B * N + C)
    M = B * N
    x2 = torch.randn(M, Cin, generator=g_).to(dev)
    F2 = torch.relu(torch.randn(M, C, generator=g_)).to(dev) + 2.0
    w_ste = (torch.randn(C, Cin, generator=g_) * 0.05).to(dev)
    Wa = (torch.randn(C, 2 * C, generator=g_) * 0.05).to(dev)[:, :C]
    t2 = torch.randn(B, C, generator=g_).to(dev)
    out_a = torch.empty(B, N, C, device=dev)
    part = ops._layer_out_rows(x2, w_ste, F2, Wa, t2, out_a, bn_shift=True)
    out_b = torch.empty(B, N, C, device=dev)
    assert ops._layer_out_rows(x2, w_ste, F2, Wa, t2, out_b) is None
    if part is None:
        pytest.skip("shape not taken by the x3 out product")
    assert torch.equal(out_a, out_b)
    outs = []
    for p_ in (part, None):
        bn = torch.nn.BatchNorm1d(C).to(dev).train()
        y = ops.bn_relu(out_a, bn, partial=p_)
        outs.append((y, bn.running_mean.clone(), bn.running_var.clone()))
    for a, b in zip(*outs):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())
