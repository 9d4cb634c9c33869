"""GPU: the two-launch form of the per-cloud chain of an HS layer's backward (hsp_colsum_cloud_f32, hsp_small_pair_f32) against
the four launches it replaces (column sum = partials + fold, hsp_small_outer_f32, hsp_small_rows_f32), bit for bit
(``torch.equal``) -- entry point by entry point, then the HS-layer and surface-layer backward nodes end to end."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# the three levels of the HS stack at B = 16, then awkward cloud counts / sizes
SHAPES = [(16, 1028, 128), (16, 257, 256), (16, 64, 512), (1, 100, 128), (3, 1000, 256), (3, 100, 512), (40, 33, 128)]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _colsum_cloud(g, xyz):
    from hs_pose_amd._lib import lib
    B, N, C = g.shape
    out = torch.full((B, (4 if xyz is not None else 1) * C), float("nan"), dtype=torch.float32, device=g.device)
    assert lib().hsp_colsum_cloud_f32(_vp(g), _vp(xyz), B, N, C, _vp(out), _stream()) == 0
    return out


@pytest.mark.parametrize("with_xyz", [False, True])
@pytest.mark.parametrize("B,N,C", SHAPES + [(2, 5000, 64), (3, 100, 32), (2, 40, 1024)])
def test_colsum_cloud_equals_the_two_launch_column_sum(dev, ref, B, N, C, with_xyz):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    assert lib().hsp_colsum_cloud_ok(B, N, C, int(with_xyz)) == 1
    g = ref.hash_tensor((B, N, C), 31, 1.0).to(dev)
    xyz = ref.hash_tensor((B, N, 3), 32, 0.1).to(dev) if with_xyz else None
    want = ops.colsum_rows_xyz(g, xyz) if with_xyz else ops.colsum_rows(g)
    got = _colsum_cloud(g, xyz)
    assert torch.equal(got, want)


def _pair(gt, Wb, alpha, fg, out_o, mom=None, Cm=0, gste=None):
    from hs_pose_amd._lib import lib
    B, Ma = gt.shape
    out_nn = torch.full((B, Wb.shape[1]), float("nan"), dtype=torch.float32, device=gt.device)
    rc = lib().hsp_small_pair_f32(_vp(gt), gt.stride(0), B, Ma, _vp(Wb), Wb.stride(0), Wb.shape[1], alpha, _vp(out_nn), out_nn.stride(0),
                                  _vp(fg), fg.stride(0), fg.shape[1], _vp(out_o), out_o.stride(0),
                                  _vp(mom), mom.stride(0) if mom is not None else 0, Cm, _vp(gste), _stream())
    assert rc == 0
    return out_nn


@pytest.mark.parametrize("rider", [False, True])
@pytest.mark.parametrize("B,N,C", SHAPES)
def test_small_pair_equals_the_two_products(dev, ref, B, N, C, rider):
    """gfg / N = gt Wb / N and gWb = gt^T fg: gt a column block of the moments (ld = 4C) with the rider, Wb and gWb column
    blocks of (C, 2C) matrices (ld > width, as w_conv2[:, C:] and g_conv2[:, C:])"""
    from hs_pose_amd import ops
    mom = ref.hash_tensor((B, 4 * C), 41, 1.0).to(dev)
    gt = mom[:, :C] if rider else mom[:, :C].contiguous()
    w2 = ref.hash_tensor((C, 2 * C), 42, 0.1).to(dev)
    fg = ref.hash_tensor((B, C), 43, 1.0).to(dev)
    Wb = w2[:, C:]
    want_g2 = torch.full((C, 2 * C), float("nan"), dtype=torch.float32, device=dev)
    want_ste = torch.full((C, 3), float("nan"), dtype=torch.float32, device=dev) if rider else None
    ops._tiny_tn(gt, fg, want_g2[:, C:], **(dict(mom=mom, gste=want_ste) if rider else {}))
    want_nn = ops.small_rows(gt, Wb, True, alpha=1.0 / N)
    got_g2 = torch.full((C, 2 * C), float("nan"), dtype=torch.float32, device=dev)
    got_ste = torch.full((C, 3), float("nan"), dtype=torch.float32, device=dev) if rider else None
    got_nn = _pair(gt, Wb, 1.0 / N, fg, got_g2[:, C:], mom[:, C:] if rider else None, C if rider else 0, got_ste)
    assert torch.equal(got_nn, want_nn)
    assert torch.equal(got_g2[:, C:], want_g2[:, C:])
    assert torch.isnan(got_g2[:, :C]).all()                    # the neighbouring column block is not touched
    if rider:
        assert torch.equal(got_ste, want_ste)


def test_small_pair_rectangular(dev, ref):
    """the entry point is not tied to square blocks: Nn != Ma != Nb"""
    from hs_pose_amd import ops
    B, Ma, Nn, Nb = 5, 256, 72, 200
    gt = ref.hash_tensor((B, Ma), 51, 1.0).to(dev)
    W = ref.hash_tensor((Ma, Nn), 52, 0.1).to(dev)
    c = ref.hash_tensor((B, Nb), 53, 1.0).to(dev)
    want_o = torch.empty(Ma, Nb, dtype=torch.float32, device=dev)
    ops._tiny_tn(gt, c, want_o)
    want_nn = ops.small_rows(gt, W, True, alpha=0.25)
    got_o = torch.empty(Ma, Nb, dtype=torch.float32, device=dev)
    got_nn = _pair(gt, W, 0.25, c, got_o)
    assert torch.equal(got_nn, want_nn) and torch.equal(got_o, want_o)


def _grads(run, monkeypatch, ops, diet, hook=None):
    monkeypatch.setattr(ops, "LAUNCH_DIET", diet)
    monkeypatch.setattr(ops, "_between_launches_hook", hook)
    return run()


class _Calls:
    """counts the C-ABI calls a backward issues, by entry point"""

    def __init__(self, ops, monkeypatch):
        self.names = []
        real = ops._run

        def run(name, args, **kw):
            self.names.append(name)
            return real(name, args, **kw)
        monkeypatch.setattr(ops, "_run", run)


def _nan_fill_hook(t):
    # unrelated allocations of the intermediate's size, filled with NaN, between the chain's two launches: the caching
    # allocator hands out whatever the node no longer references
    junk = [torch.full_like(t, float("nan")) for _ in range(4)]
    del junk


@pytest.mark.parametrize("B,N,Cin,C,k,S", [(16, 1028, 128, 128, 20, 7), (16, 257, 128, 256, 20, 7), (16, 64, 256, 512, 8, 7),
                                           (3, 100, 128, 128, 20, 7), (1, 1000, 128, 128, 20, 7), (2, 128, 16, 32, 8, 3)])
def test_hs_layer_backward_equals_the_four_launch_chain(dev, ref, monkeypatch, B, N, Cin, C, k, S):
    """every gradient the HS-layer node returns, deterministic backward: two-launch chain == four-launch chain, also with
    NaN-filled allocations between the chain's launches; C = 32 is a width the two-launch form declines (same launches both ways)"""
    from hs_pose_amd import gcn3d, ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    m = gcn3d.HS_layer(Cin, C, S)
    sd = m.state_dict()
    ref.fill_state_closed_form(sd)
    m.load_state_dict(sd)
    m = m.to(dev)
    xyz = ref.hash_tensor((B, N, 3), 61, 0.1).to(dev)
    fmap0 = torch.relu(ref.hash_tensor((B, N, Cin), 62, 1.0)).to(dev)
    up = ref.hash_tensor((B, N, C), 63, 1.0).to(dev)
    calls = _Calls(ops, monkeypatch)

    def run():
        m.zero_grad(set_to_none=True)
        fmap = fmap0.clone().requires_grad_(True)
        calls.names.clear()
        (m(xyz, fmap, k) * up).sum().backward()
        return [fmap.grad.clone()] + [p.grad.clone() for p in m.parameters()], list(calls.names)

    (old, old_calls) = _grads(run, monkeypatch, ops, False)
    (new, new_calls) = _grads(run, monkeypatch, ops, True)
    (hooked, _) = _grads(run, monkeypatch, ops, True, _nan_fill_hook)
    takes = C % 128 == 0
    assert ("hsp_small_pair_f32" in new_calls) == takes and "hsp_small_pair_f32" not in old_calls
    assert ("hsp_small_outer_f32" in new_calls) == (not takes) and "hsp_small_outer_f32" in old_calls
    assert len(old) == len(new) == len(hooked) == 1 + len(list(m.parameters()))
    for a, b, c in zip(old, new, hooked):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("B,N,C,k,S", [(16, 1028, 128, 20, 7), (3, 100, 128, 20, 7), (1, 1000, 256, 20, 7), (2, 128, 16, 8, 3)])
def test_surface_layer_backward_equals_the_four_launch_chain(dev, ref, monkeypatch, B, N, C, k, S):
    """the surface layer's node: the STE gradient rides in the pair launch (mom / gste); C = 16: a width the form declines"""
    from hs_pose_amd import gcn3d, ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    m = gcn3d.HSlayer_surface(C, S)
    sd = m.state_dict()
    ref.fill_state_closed_form(sd)
    m.load_state_dict(sd)
    m = m.to(dev)
    xyz = ref.hash_tensor((B, N, 3), 71, 0.1).to(dev)
    up = ref.hash_tensor((B, N, C), 72, 1.0).to(dev)
    calls = _Calls(ops, monkeypatch)

    def run():
        m.zero_grad(set_to_none=True)
        calls.names.clear()
        (m(xyz, k) * up).sum().backward()
        return [p.grad.clone() for p in m.parameters()], list(calls.names)

    (old, old_calls) = _grads(run, monkeypatch, ops, False)
    (new, new_calls) = _grads(run, monkeypatch, ops, True)
    (hooked, _) = _grads(run, monkeypatch, ops, True, _nan_fill_hook)
    takes = C % 128 == 0
    assert ("hsp_colsum_cloud_f32" in new_calls) == takes and "hsp_colsum_cloud_f32" not in old_calls
    assert "hsp_colsum_rows_xyz" in old_calls
    assert len(old) == len(new) == len(hooked) == len(list(m.parameters())) > 0
    for a, b, c in zip(old, new, hooked):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c)


def test_more_than_64_clouds_keep_the_old_launches(dev, ref, monkeypatch):
    """B > 64: hsp_small_pair_f32 declines (a row per lane holds 64 clouds), the node keeps its general path and still agrees"""
    from hs_pose_amd import gcn3d, ops
    from hs_pose_amd._lib import lib
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    B, N, C, k, S = 70, 64, 128, 8, 3
    one = ctypes.c_void_p(256)
    assert lib().hsp_small_pair_f32(one, C, B, C, one, C, C, 1.0, one, C, one, C, C, one, C, None, 0, 0, None, None) == -2
    m = gcn3d.HSlayer_surface(C, S)
    sd = m.state_dict()
    ref.fill_state_closed_form(sd)
    m.load_state_dict(sd)
    m = m.to(dev)
    xyz = ref.hash_tensor((B, N, 3), 81, 0.1).to(dev)
    up = ref.hash_tensor((B, N, C), 82, 1.0).to(dev)
    calls = _Calls(ops, monkeypatch)
    res = []
    for diet in (False, True):
        monkeypatch.setattr(ops, "LAUNCH_DIET", diet)
        m.zero_grad(set_to_none=True)
        calls.names.clear()
        (m(xyz, k) * up).sum().backward()
        assert "hsp_small_pair_f32" not in calls.names
        res.append([p.grad.clone() for p in m.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
