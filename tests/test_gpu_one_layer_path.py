"""GPU: the HS layers are ONE autograd node per layer for fp32 and bf16 feature rows (ops._HSLayer / ops._SurfaceLayer).  For
one forward + backward of the gcn3d module in each dtype: the C-ABI entry points issued are the literal lists below -- recorded
from the two separate sets of nodes this one replaced, with this very recorder: an exact sequence for fp32 (graph captures and
launch counts depend on it), a multiset for bf16 (its parameter gradients are order-fixed split-K sums: when they are issued
does not change a bit) -- and the bf16 output agrees with the fp32 one on the same bf16-rounded inputs, parameters and
neighbour lists within the one-layer bound of tests/test_gpu_bf16.py::test_hs_layer_bf16_vs_cpu_oracle (1e-2 of scale)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ONE_LAYER_TOL = 1e-2              # tests/test_gpu_bf16.py::test_hs_layer_bf16_vs_cpu_oracle

# (B, N, Cin, C, k, S): 64 channels = the smallest the bf16 weight-gradient kernel takes and a width the two-launch per-cloud
# chain declines; then an odd batch of odd clouds at a width that takes it
HS_SMALL, HS_ODD = (2, 128, 64, 64, 8, 3), (3, 100, 128, 128, 20, 7)
SURFACE = (3, 100, 128, 20, 7)    # (B, N, C, k, S)

EXPECT = {
    ("hs", HS_SMALL, "f32"): [
        "hsp_knn_f32", "hsp_knn_xyz_f32", "hsp_gemm_rows_f32", "hsp_rf_conv_fwd", "hsp_orl_global_fwd", "hsp_small_rows_f32",
        "hsp_gemm_rows_f32", "hsp_colsum_rows", "hsp_wgrad_partial_pair_f32", "hsp_small_outer_f32", "hsp_gemm_rows_f32",
        "hsp_small_rows_f32", "hsp_gather_max_bwd", "hsp_rf_conv_bwd_scatter", "hsp_wgrad_partial_f32", "hsp_gemm_rows_f32",
        "hsp_wgrad_fold"
    ],
    ("hs", HS_SMALL, "bf16"): [
        "hsp_knn_bf16", "hsp_knn_xyz_f32", "hsp_gemm_rows_bf16", "hsp_rf_conv_fwd_bf16", "hsp_orl_global_fwd_bf16",
        "hsp_small_rows_f32", "hsp_gemm_rows_bf16", "hsp_colsum_rows_bf16", "hsp_wgrad_partial_bf16", "hsp_small_outer_f32",
        "hsp_gemm_rows_bf16", "hsp_small_rows_f32", "hsp_gather_max_bwd_bf16", "hsp_rf_conv_bwd_scatter_bf16",
        "hsp_wgrad_partial_bf16", "hsp_wgrad_partial_bf16", "hsp_gemm_rows_bf16", "hsp_wgrad_fold"
    ],
    ("hs", HS_ODD, "f32"): [
        "hsp_knn_f32", "hsp_knn_xyz_f32", "hsp_gemm_rows_f32", "hsp_rf_conv_fwd", "hsp_orl_global_fwd", "hsp_small_rows_f32",
        "hsp_gemm_rows_f32", "hsp_colsum_cloud_f32", "hsp_small_pair_f32", "hsp_wgrad_partial_pair_f32", "hsp_gemm_rows_f32",
        "hsp_gather_max_bwd", "hsp_rf_conv_bwd_scatter", "hsp_wgrad_partial_f32", "hsp_split_params_x3",
        "hsp_split_params_x3", "hsp_gemm_x3_f32", "hsp_wgrad_fold"
    ],
    ("hs", HS_ODD, "bf16"): [
        "hsp_knn_bf16", "hsp_knn_xyz_f32", "hsp_gemm_rows_bf16", "hsp_rf_conv_fwd_bf16", "hsp_orl_global_fwd_bf16",
        "hsp_small_rows_f32", "hsp_gemm_rows_bf16", "hsp_colsum_rows_bf16", "hsp_wgrad_partial_bf16", "hsp_small_outer_f32",
        "hsp_gemm_rows_bf16", "hsp_small_rows_f32", "hsp_gather_max_bwd_bf16", "hsp_rf_conv_bwd_scatter_bf16",
        "hsp_wgrad_partial_bf16", "hsp_wgrad_partial_bf16", "hsp_gemm_rows_bf16", "hsp_wgrad_fold"
    ],
    ("surface", SURFACE, "f32"): [
        "hsp_knn_xyz_f32", "hsp_rf_surface_fwd", "hsp_orl_global_fwd", "hsp_small_rows_f32", "hsp_gemm_rows_f32",
        "hsp_colsum_cloud_f32", "hsp_small_pair_f32", "hsp_wgrad_partial_f32", "hsp_wgrad_fold", "hsp_gemm_rows_f32",
        "hsp_gather_max_bwd", "hsp_rf_surface_bwd"
    ],
    ("surface", SURFACE, "bf16"): [
        "hsp_knn_xyz_f32", "hsp_rf_surface_fwd_bf16", "hsp_orl_global_fwd_bf16", "hsp_small_rows_f32", "hsp_gemm_rows_bf16",
        "hsp_colsum_rows_xyz_bf16", "hsp_wgrad_bf16", "hsp_small_outer_f32", "hsp_gemm_rows_bf16", "hsp_small_rows_f32",
        "hsp_gather_max_bwd_bf16", "hsp_rf_surface_bwd_bf16"
    ],
}


class _Calls:
    """records the C-ABI calls issued, by entry point (the recorder of tests/test_gpu_launch_diet.py, on every module that
    holds a reference to ops._run)"""

    def __init__(self, monkeypatch):
        from hs_pose_amd import ops, ops_bf16
        self.names = []
        real = ops._run

        def run(name, args, **kw):
            self.names.append(name)
            return real(name, args, **kw)
        monkeypatch.setattr(ops, "_run", run)
        monkeypatch.setattr(ops_bf16, "_run", run)


class _SameLists:
    """ops.knn that hands the bf16 run the fp32 run's feature-space neighbour lists (its own search still runs and is recorded)"""

    def __init__(self, monkeypatch):
        from hs_pose_amd import ops
        self.real, self.lists, self.pos = ops.knn, [], None
        monkeypatch.setattr(ops, "knn", self)

    def __call__(self, x, k, *a, **kw):
        own = self.real(x, k, *a, **kw)
        if x.shape[-1] == 3:
            return own
        if self.pos is None:
            self.lists.append(own)
            return own
        self.pos += 1
        return self.lists[self.pos - 1]


def _module(ref, dev, make, specs_of):
    """the module with closed-form weights rounded to bf16, and its bf16 working copies (FaceRecon.set_feature_dtype's specs)"""
    from hs_pose_amd.ops_bf16 import Bf16Params
    m = make()
    sd = m.state_dict()
    ref.fill_state_closed_form(sd)
    m.load_state_dict({k_: v.bfloat16().float() for k_, v in sd.items()})
    m = m.to(dev)
    prm = Bf16Params(specs_of(m))
    prm.refresh()
    return m, prm


def _check(kind, shape, calls, outs):
    for dt in ("f32", "bf16"):
        print(f"{kind} {shape} {dt}: {calls[dt]}")
    assert calls["f32"] == EXPECT[(kind, shape, "f32")]
    assert sorted(calls["bf16"]) == sorted(EXPECT[(kind, shape, "bf16")])
    want, got = outs["f32"], outs["bf16"].float()
    assert outs["bf16"].dtype == BF and torch.isfinite(got).all()
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"{kind} {shape}: bf16 against fp32, max err {err:.2e} of scale")
    assert err <= ONE_LAYER_TOL


@pytest.mark.parametrize("shape", [HS_SMALL, HS_ODD])
def test_hs_layer_one_node_two_dtypes(dev, ref, monkeypatch, shape):
    from hs_pose_amd import gcn3d, ops
    B, N, Cin, C, k, S = shape
    m, prm = _module(ref, dev, lambda: gcn3d.HS_layer(Cin, C, S),
                     lambda m: [(m.weights.detach(), True, True), (m.STE_layer.weight.detach().squeeze(-1), True, True),
                                (m.conv2.weight.detach().squeeze(-1), True, True)])
    xyz = ref.hash_tensor((B, N, 3), 91, 0.1).to(dev)
    X = torch.relu(ref.hash_tensor((B, N, Cin), 92, 1.0)).bfloat16().to(dev)
    up = ref.hash_tensor((B, N, C), 93, 1.0).bfloat16().to(dev)
    rec, lists = _Calls(monkeypatch), _SameLists(monkeypatch)
    calls, outs = {}, {}
    for name, dt in (("f32", torch.float32), ("bf16", BF)):
        m.zero_grad(set_to_none=True)
        x = X.to(dt).requires_grad_(True)
        lists.pos = None if name == "f32" else 0
        rec.names.clear()
        with ops.x3_scope(ops.X3Planes()):      # a registry of its own: the x3 products see their weights for the first time
            out = m(xyz, x, k)
        (out * up.to(dt)).sum().backward()
        calls[name], outs[name] = list(rec.names), out.detach()
        assert x.grad.dtype == dt and all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    _check("hs", shape, calls, outs)


def test_surface_layer_one_node_two_dtypes(dev, ref, monkeypatch):
    from hs_pose_amd import gcn3d, ops
    B, N, C, k, S = SURFACE
    m, prm = _module(ref, dev, lambda: gcn3d.HSlayer_surface(C, S), lambda m: [(m.conv2.weight.detach().squeeze(-1), True, True)])
    xyz = ref.hash_tensor((B, N, 3), 94, 0.1).to(dev)
    up = ref.hash_tensor((B, N, C), 95, 1.0).bfloat16().to(dev)
    rec = _Calls(monkeypatch)
    calls, outs = {}, {}
    for name, dt in (("f32", torch.float32), ("bf16", BF)):
        m.zero_grad(set_to_none=True)
        m.out_dtype = dt
        rec.names.clear()
        with ops.x3_scope(ops.X3Planes()):
            out = m(xyz, k)
        (out * up.to(dt)).sum().backward()
        calls[name], outs[name] = list(rec.names), out.detach()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    _check("surface", SURFACE, calls, outs)
