"""GPU: the ORL forward's winner counts and the stream-pass backward that reads them.

hsp_orl_global_fwd, given a workspace with room for them (hsp_orl_counts_offset), leaves counts[b][m][c] = the number of points
whose winning neighbour for channel c is row m; hsp_gather_max_bwd(grad_bcast = 2) turns them into the ORL gradient in one stream
pass.  Counts are integers and the stream pass evaluates the scatter flush's expression in its order, so every comparison here
is exact: integer equality for the counts, torch.equal for everything downstream."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_vp = ctypes.c_void_p


def _lists(B, N, k, dev, seed):
    """(B, N, k) int32 nearest-neighbour lists of a random cloud, self included (N = k: every list is the whole cloud)"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(B, N, 3, generator=g).to(dev)
    return torch.cdist(xyz, xyz).topk(k, dim=2, largest=False).indices.int().contiguous()


def _features(kind, B, N, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        f = torch.randn(B, N, C, generator=g)
    elif kind == "equal":                       # every winner is slot 0: the counts pile onto the rows many lists start with
        f = torch.full((B, N, C), 0.75)
    else:                                       # two values: ties everywhere
        f = (torch.rand(B, N, C, generator=g) < 0.3).float() * 2.0 - 1.0
    return f.to(dev)


def _counts_cpu(idx, arg):
    """counts rebuilt from the arg-max bytes and the lists"""
    B, N, C = arg.shape
    rows = torch.gather(idx.cpu().long(), 2, arg.cpu().long())            # (B, N, C): the winning row of (point, channel)
    return torch.zeros(B, N, C, dtype=torch.int64).scatter_add_(1, rows, torch.ones(B, N, C, dtype=torch.int64))


@pytest.mark.parametrize("kind", ["random", "equal", "two"])
@pytest.mark.parametrize("B,N,C,k", [(1, 20, 8, 20), (3, 100, 128, 20), (8, 257, 256, 20), (2, 1028, 128, 20)])
def test_counts_are_the_winner_counts(dev, B, N, C, k, kind):
    from hs_pose_amd import ops
    assert ops.ORL_COUNTS
    idx = _lists(B, N, k, dev, 7 * N + C)
    feat = _features(kind, B, N, C, dev, N + C)
    fg, arg, cnt = ops._orl_fwd_counts_raw(feat, idx, k)
    assert cnt is not None and cnt.dtype == torch.uint16 and tuple(cnt.shape) == (B, N, C)
    fg0, arg0 = ops._orl_fwd_raw(feat, idx, k)                            # today's workspace size
    torch.cuda.synchronize()
    assert torch.equal(fg, fg0) and torch.equal(arg, arg0)
    got = cnt.cpu().to(torch.int64)
    want = _counts_cpu(idx, arg)
    print(f"{kind} {(B, N, C, k)}: largest count {int(want.max())}, cells that differ {int((got != want).sum())}")
    assert torch.equal(got, want)
    assert torch.equal(got.sum(dim=1), torch.full((B, C), N, dtype=torch.int64))
    if kind == "equal":
        assert int(arg.max()) == 0


def _bwd(L, mode, gbc, idx, arg_or_cnt, gF, accumulate, extra):
    from hs_pose_amd.ops import _p, _stream
    B, N, C = gF.shape
    sfx = "_bf16" if gF.dtype == BF else ""
    rc = getattr(L, "hsp_gather_max_bwd" + sfx)(_p(gbc), mode, _p(idx) if mode == 1 else _vp(0), _vp(0), _p(arg_or_cnt), B, N, N, N,
                                                idx.shape[2], C, _p(gF), accumulate, _p(extra), _stream())
    assert rc == 0, rc


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,N,C", [(3, 100, 128), (8, 257, 256)])
def test_stream_backward_equals_the_scatter(dev, B, N, C, accumulate, with_extra, dtype):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    k = 20
    idx = _lists(B, N, k, dev, N)
    feat = _features("random", B, N, C, dev, C)
    feat[:, N // 2:] = feat[:, : N - N // 2].clone()                       # equal maxima among the neighbours
    _, arg, cnt = ops._orl_fwd_counts_raw(feat, idx, k)
    g = torch.Generator().manual_seed(5)
    gbc = torch.randn(B, C, generator=g)
    gbc[:, 0::7] = 0.0
    gbc[:, 1::7] = -gbc[:, 1::7].abs()
    gbc[:, 2::7] *= 1e-39                                                  # denormal scale
    gbc = gbc.to(dev)
    base = torch.randn(B, N, C, generator=g).to(dev).to(dtype)
    extra = torch.randn(B, N, C, generator=g).to(dev).to(dtype) if with_extra else None
    out = {}
    for mode, src in ((1, arg), (2, cnt)):
        gF = base.clone()
        _bwd(lib(), mode, gbc, idx, src, gF, accumulate, extra)
        out[mode] = gF
    torch.cuda.synchronize()
    assert torch.isfinite(out[1].float()).all()
    assert not torch.equal(out[1], base)
    assert torch.equal(out[1], out[2])


class _Calls:
    """the C-ABI calls issued, by entry point, and the grad_bcast argument of the ORL backward among them"""

    def __init__(self, monkeypatch):
        from hs_pose_amd import ops, ops_bf16
        self.names, self.modes = [], []
        real = ops._run

        def run(name, args, **kw):
            self.names.append(name)
            if name == "hsp_gather_max_bwd":
                self.modes.append(args[1])
            return real(name, args, **kw)
        monkeypatch.setattr(ops, "_run", run)
        monkeypatch.setattr(ops_bf16, "_run", run)


def _closed_form(ref, dev, m):
    sd = m.state_dict()
    ref.fill_state_closed_form(sd)
    m.load_state_dict(sd)
    return m.to(dev)


def _on_and_off(monkeypatch, rec, run):
    """run() -> tensors, once with ops.ORL_COUNTS on and once off: ([tensors], names, modes) of each"""
    from hs_pose_amd import ops
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "ORL_COUNTS", on)
        rec.names.clear()
        rec.modes.clear()
        with ops.x3_scope(ops.X3Planes()):
            tensors = [t.detach().clone() for t in run()]
        res[on] = (tensors, list(rec.names), list(rec.modes))
    torch.cuda.synchronize()
    return res


def _same(res):
    (a, na, _), (b, nb, _) = res[True], res[False]
    assert na == nb
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _hs_run(m, xyz, X, k, up, idx_x=None):
    from hs_pose_amd import ops

    def run():
        m.zero_grad(set_to_none=True)
        x = X.clone().requires_grad_(True)
        if idx_x is None:
            out = m(xyz, x, k)
        else:
            out = ops.hs_layer(xyz, x, ops.knn(x, k), idx_x, k, m.support_num, m.weights, m.bias, m.directions, m.STE_layer.weight,
                               m.conv2.weight)
        (out * up).sum().backward()
        return [out, x.grad] + [p.grad for p in m.parameters()]
    return run


# N = 100: the pinned test's shapes -- under ops.ORL_COUNTS_MIN_N points the nodes do not ask (the forward would pay a third launch
# for the counts) and run today's calls either way; N = 257 (a ragged last pass of the slab kernel): they ask, and get mode 2
@pytest.mark.parametrize("N", [100, 257])
def test_hs_layer_same_bits_with_and_without_counts(dev, ref, monkeypatch, N):
    from hs_pose_amd import gcn3d, ops
    B, Cin, C, k, S = 3, 128, 128, 20, 7
    m = _closed_form(ref, dev, gcn3d.HS_layer(Cin, C, S))
    xyz = ref.hash_tensor((B, N, 3), 91, 0.1).to(dev)
    X = torch.relu(ref.hash_tensor((B, N, Cin), 92, 1.0)).to(dev)
    up = ref.hash_tensor((B, N, C), 93, 1.0).to(dev)
    res = _on_and_off(monkeypatch, _Calls(monkeypatch), _hs_run(m, xyz, X, k, up))
    assert res[True][2] == ([2] if N >= ops.ORL_COUNTS_MIN_N else [1]) and res[False][2] == [1]
    _same(res)


@pytest.mark.parametrize("N", [100, 257])
def test_surface_layer_same_bits_with_and_without_counts(dev, ref, monkeypatch, N):
    from hs_pose_amd import gcn3d, ops
    B, C, k, S = 3, 128, 20, 7
    m = _closed_form(ref, dev, gcn3d.HSlayer_surface(C, S))
    xyz = ref.hash_tensor((B, N, 3), 94, 0.1).to(dev)
    up = ref.hash_tensor((B, N, C), 95, 1.0).to(dev)

    def run():
        m.zero_grad(set_to_none=True)
        out = m(xyz, k)
        (out * up).sum().backward()
        return [out] + [p.grad for p in m.parameters()]
    res = _on_and_off(monkeypatch, _Calls(monkeypatch), run)
    assert res[True][2] == ([2] if N >= ops.ORL_COUNTS_MIN_N else [1]) and res[False][2] == [1]
    _same(res)


@pytest.mark.parametrize("no_grad", [False, True])
@pytest.mark.parametrize("layer", ["hs", "surface"])
def test_frozen_layer_forward_with_and_without_counts(dev, ref, monkeypatch, layer, no_grad):
    """nothing requires a gradient (frozen parameters, an input without one): the nodes' forward asks for no counts and gives the
    same bits through the same calls with the switch on and off"""
    from hs_pose_amd import gcn3d
    B, N, Cin, C, k, S = 3, 160, 128, 128, 20, 7
    m = _closed_form(ref, dev, gcn3d.HS_layer(Cin, C, S) if layer == "hs" else gcn3d.HSlayer_surface(C, S))
    m.requires_grad_(False)
    xyz = ref.hash_tensor((B, N, 3), 51, 0.1).to(dev)
    X = torch.relu(ref.hash_tensor((B, N, Cin), 52, 1.0)).to(dev)

    def run():
        with torch.no_grad() if no_grad else torch.enable_grad():
            out = m(xyz, X, k) if layer == "hs" else m(xyz, k)
        assert not out.requires_grad
        return [out]
    res = _on_and_off(monkeypatch, _Calls(monkeypatch), run)
    assert "hsp_orl_global_fwd" in res[True][1] and res[True][2] == []
    assert torch.isfinite(res[True][0][0]).all() and res[True][0][0].abs().sum().item() > 0
    _same(res)


def test_misaligned_larger_workspace_gets_the_plain_call(dev):
    """a caller's scratch buffer larger than hsp_orl_workspace_bytes but not 16-byte aligned: no counts, no error, the plain result"""
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    from hs_pose_amd.ops import _p, _stream
    B, N, C, k = 3, 100, 128, 20
    L = lib()
    idx = _lists(B, N, k, dev, 11)
    feat = _features("random", B, N, C, dev, 12)
    fg0, arg0 = ops._orl_fwd_raw(feat, idx, k)
    base = L.hsp_orl_workspace_bytes(B, N, C)
    full = ((base + 255) & ~255) + 2 * B * N * C
    assert L.hsp_orl_counts_offset(B, N, k, k, C, full) >= 0
    buf = torch.full((full + 16,), 0xA5, dtype=torch.uint8, device=dev)
    ws = buf[4:]
    assert ws.data_ptr() % 16 == 4
    fg, arg = torch.empty_like(fg0), torch.empty_like(arg0)
    rc = L.hsp_orl_global_fwd(_p(feat), _p(idx), B, N, k, k, C, _p(fg), _p(arg), _p(ws), full, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert torch.equal(fg, fg0) and torch.equal(arg, arg0)
    assert bool((buf[4 + ((base + 255) & ~255):] == 0xA5).all())           # the counts region is untouched


def test_k8_layer_keeps_todays_calls(dev, ref, monkeypatch):
    from hs_pose_amd import gcn3d
    B, N, Cin, C, k, S = 2, 128, 64, 64, 8, 3
    m = _closed_form(ref, dev, gcn3d.HS_layer(Cin, C, S))
    xyz = ref.hash_tensor((B, N, 3), 81, 0.1).to(dev)
    X = torch.relu(ref.hash_tensor((B, N, Cin), 82, 1.0)).to(dev)
    up = ref.hash_tensor((B, N, C), 83, 1.0).to(dev)
    res = _on_and_off(monkeypatch, _Calls(monkeypatch), _hs_run(m, xyz, X, k, up))
    assert res[True][2] == [1] and res[False][2] == [1]
    _same(res)


def test_strided_lists_keep_todays_calls(dev, ref, monkeypatch):
    from hs_pose_amd import gcn3d, ops
    B, N, Cin, C, k, S = 3, 160, 128, 128, 20, 7                           # (enough points that the stride is the only reason)
    m = _closed_form(ref, dev, gcn3d.HS_layer(Cin, C, S))
    xyz = ref.hash_tensor((B, N, 3), 71, 0.1).to(dev)
    X = torch.relu(ref.hash_tensor((B, N, Cin), 72, 1.0)).to(dev)
    up = ref.hash_tensor((B, N, C), 73, 1.0).to(dev)
    wide = ops.knn(xyz, k + 4)                                             # (B, N, 24): the layer reads the first 20 columns
    assert wide.shape[2] == k + 4 and wide.is_contiguous()
    res = _on_and_off(monkeypatch, _Calls(monkeypatch), _hs_run(m, xyz, X, k, up, idx_x=wide))
    assert res[True][2] == [1] and res[False][2] == [1]
    _same(res)


def test_replay_equals_eager_with_counts(dev, ref):
    """one HS layer's forward + backward captured and replayed, counts on, against the same step run eagerly"""
    from hs_pose_amd import gcn3d, ops
    assert ops.ORL_COUNTS
    B, N, Cin, C, k, S = 2, 257, 128, 128, 20, 7
    m = _closed_form(ref, dev, gcn3d.HS_layer(Cin, C, S))
    xyz = ref.hash_tensor((B, N, 3), 61, 0.1).to(dev)
    X = torch.relu(ref.hash_tensor((B, N, Cin), 62, 1.0)).to(dev).requires_grad_(True)
    up = ref.hash_tensor((B, N, C), 63, 1.0).to(dev)
    params = list(m.parameters())
    state = {}

    def body():
        X.grad = None
        for p in params:
            p.grad = None
        out = m(xyz, X, k)
        out.backward(up)
        state["out"] = out.detach()

    with ops.x3_scope(ops.X3Planes()):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        eager = [state["out"].clone(), X.grad.clone()] + [p.grad.clone() for p in params]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            body()
        for t in [state["out"], X.grad] + [p.grad for p in params]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    replayed = [state["out"], X.grad] + [p.grad for p in params]
    assert all(t.abs().sum().item() > 0 for t in replayed)
    assert all(torch.equal(a, b) for a, b in zip(eager, replayed))
