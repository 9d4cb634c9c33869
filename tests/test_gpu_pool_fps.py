"""The 'fps' pool sampler on the GPU: gcn3d.Pool_layer(sampler="fps") / config.FLAGS.pool_sampler = 'fps' keeps, per cloud, the rows
farthest-point sampling picks on that cloud, computed on the device inside the forward (and inside a captured graph).

  1. ops.fps_levels (hsp_fps_levels_f32) against the C oracle's FPS and the numpy statement of the rule
     (tests/test_pool_sampler_host.py::fps_never_repick), tiled and all-identical clouds included; level 2 is a prefix.
  2. pooling forward with a kept-row list PER CLOUD: exact equality with a torch composition (max is exact), first-slot tie rule.
  3. its backward against an fp64 composition, within A 2^-24 sum|terms| (+ 2^-8 |value| on bf16 rows), A = 32 -- the bounds and
     constants of tests/test_gpu_rf_reference.py --, on the column-tile LDS scatter and on the global-atomics fallback.
  4. a (B,Nq) list whose rows are one vector == the shared-list entry points, bit for bit.
  5. the default sampler still consumes the host generator exactly as graph.draw_pool_indices.
  6. - 8. the network under 'fps': eval mode (a function of the cloud alone; every cloud equals itself run alone through the
     random-sampler path fed its own picks), train mode against the fed random path, and the captured graphs.
"""
import numpy as np
import pytest
import torch

from test_pool_sampler_host import clouds, fps_never_repick

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U = 2.0 ** -24
A = 32.0


# ==== 1. the sampler =================================================================================================================

def _check_levels(pts, dev, want_sel, n1=None):
    from hs_pose_amd import ops
    B, N, _ = pts.shape
    n1 = N // 4 if n1 is None else n1
    n2 = n1 // 4
    sel1, v1, v2 = ops.fps_levels(pts.to(dev), n1, n2)
    assert sel1.dtype == torch.int32 and sel1.shape == (B, n1) and v1.shape == (B, n1, 3) and v2.shape == (B, n2, 3)
    got = sel1.cpu().numpy()
    assert np.array_equal(got, want_sel), "picks differ"
    assert all(len(set(r.tolist())) == n1 for r in got), "a row was picked twice"
    assert torch.equal(v1.cpu(), torch.gather(pts, 1, sel1.cpu().long().unsqueeze(-1).expand(-1, -1, 3))), "v1 != xyz[sel1]"
    assert torch.equal(v2, v1[:, :n2]), "v2 != v1[:, :n2]"
    ar = torch.arange(n2, dtype=torch.int32, device=dev).expand(B, n2)
    assert torch.equal(ops.fps_levels(v1, n2, 0)[0], ar), "the sampler on level 1 does not return the prefix"
    return sel1, v1


@pytest.mark.parametrize("B,N", [(3, 70), (2, 257), (5, 1028)])
def test_fps_levels_matches_the_oracle(dev, ref, oc, B, N):
    from hs_pose_amd import ops
    pts = ref.hash_tensor((B, N, 3), 40 + N, 0.1)
    n1 = N // 4
    want = oc.fps_f32(pts.numpy(), n1)
    assert all(len(set(r.tolist())) == n1 for r in want)          # distinct under the plain rule: the added rule changes nothing
    sel1, v1 = _check_levels(pts, dev, want)
    assert np.array_equal(want, np.stack([fps_never_repick(p, n1) for p in pts.numpy()]))
    assert not np.array_equal(want[0], want[1])                    # the clouds of a batch keep different rows
    assert torch.equal(ops.fps(v1, n1 // 4), torch.arange(n1 // 4, dtype=torch.int32, device=dev).expand(B, n1 // 4))
    assert ops.fps_levels(pts.to(dev), n1, 0)[2] is None


# (names, n1): 100 distinct points of 256 rows (128 picks) and of 1028 rows (257 picks), one point 64 times -- each batched with
# another cloud
@pytest.mark.parametrize("names,n1", [(("tiled256", "random257_0"), 128), (("tiled1028", "random1028_1"), 257),
                                      (("identical64", "identical64"), 16)])
def test_fps_levels_never_picks_a_row_twice(dev, names, n1):
    """fewer distinct points than picks: the plain rule returns row 0 over and over, the sampler the lowest-index unpicked rows"""
    cl = clouds()
    N = min(cl[n].shape[0] for n in names)
    pts = torch.from_numpy(np.stack([cl[n][:N] for n in names]))
    plain = fps_never_repick(pts[0].numpy(), n1, never_repick=False)
    assert len(set(plain.tolist())) < n1                           # the added rule is what this case is about
    want = np.stack([fps_never_repick(p, n1) for p in pts.numpy()])
    _check_levels(pts, dev, want, n1)


def test_fps_levels_rejects_what_it_cannot_do(dev):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError
    x = torch.zeros(1, 64, 3, device=dev)
    for n1, n2 in ((0, 0), (65, 1), (16, 17)):
        with pytest.raises(HspError):
            ops.fps_levels(x, n1, n2)
    with pytest.raises(HspError, match="no fall-back to random"):
        ops.fps_levels(torch.zeros(1, 12289, 3, device=dev), 16, 4)
    with pytest.raises(HspError):
        ops.fps_levels(torch.zeros(1, 64, 4, device=dev), 16, 4)


# ==== 2. - 4. pooling with kept rows per cloud =======================================================================================

class _Pool:
    """feat (B,N,C), neighbour lists (B,N,k+1) of which k are used, xyz, and a kept-row list per cloud: all different, one of them
    naming a row twice; ``plant``: a dominant feature row listed by ten kept rows of every cloud; ``ties``: few distinct values"""

    def __init__(self, ref, B, N, Nq, C, k, seed, dtype=torch.float32, ties=False, plant=False):
        g = torch.Generator().manual_seed(seed)
        self.B, self.N, self.Nq, self.C, self.k = B, N, Nq, C, k
        feat = ref.hash_tensor((B, N, C), seed, 1.0)
        if ties:
            feat = torch.round(feat * 2) / 2
        self.idx = torch.randint(0, N, (B, N, k + 1), generator=g, dtype=torch.int32)
        self.qsel = torch.stack([torch.randperm(N, generator=g)[:Nq] for _ in range(B)]).to(torch.int32)
        self.qsel[0, 1] = self.qsel[0, 0]                          # a row kept twice (a tiled cloud)
        if plant:
            for b in range(B):
                r = int(torch.randint(0, N, (1,), generator=g))
                feat[b, r] = 4.0 + feat[b, r].abs()
                self.idx[b, self.qsel[b, :10].long(), 1] = r
        self.feat = feat.to(dtype)
        self.xyz = ref.hash_tensor((B, N, 3), seed + 1, 0.1)

    def route(self):
        """per cloud: (values (Nq,C), source row of the FIRST slot holding the maximum (Nq,C))"""
        out = []
        for b in range(self.B):
            nb = self.idx[b, self.qsel[b].long(), :self.k].long()                      # (Nq,k)
            rows = self.feat[b].double()[nb]                                           # (Nq,k,C)
            m = rows.max(dim=1).values
            slot = ((rows == m.unsqueeze(1)).cumsum(1) == 0).sum(1)                    # leading non-maxima = the first slot
            out.append((m, torch.gather(nb, 1, slot)))
        return out

    def backward_ref(self, g):
        """fp64 (grad_feat, sum|terms|, number of terms) of out.backward(g)"""
        want = torch.zeros(self.B, self.N, self.C, dtype=torch.float64)
        terms, cnt = torch.zeros_like(want), torch.zeros_like(want)
        for b, (_, src) in enumerate(self.route()):
            gb = g[b].double()
            want[b].scatter_add_(0, src, gb)
            terms[b].scatter_add_(0, src, gb.abs())
            cnt[b].scatter_add_(0, src, torch.ones_like(gb))
        return want, terms, cnt


FWD = [(3, 70, 17, 12, 4, False), (2, 257, 64, 256, 4, False), (16, 1028, 257, 128, 4, False), (3, 70, 17, 16, 4, True)]


@pytest.mark.parametrize("B,N,Nq,C,k,ties", FWD)
def test_per_cloud_pooling_forward_is_exact(dev, ref, B, N, Nq, C, k, ties):
    from hs_pose_amd import ops
    c = _Pool(ref, B, N, Nq, C, k, 7 + N + C, ties=ties)
    want = torch.stack([m for m, _ in c.route()]).float()
    if ties:                                                       # the tie rule is exercised: slots of different rows tie
        nb = c.idx[0, c.qsel[0].long(), :k].long()
        rows = c.feat[0][nb]
        assert ((rows == rows.max(1, keepdim=True).values).sum(1) > 1).any()
    feat, idx, qsel, xyz = c.feat.to(dev), c.idx.to(dev), c.qsel.to(dev), c.xyz.to(dev)
    want_v = torch.gather(c.xyz, 1, c.qsel.long().unsqueeze(-1).expand(-1, -1, 3))
    for grad in (False, True):                                     # (both take the ctypes entry: the compiled form is shared-only)
        with torch.set_grad_enabled(grad):
            out, v = ops.pool_layer(feat, xyz, idx, qsel, k)
        assert torch.equal(out.cpu(), want) and torch.equal(v.cpu(), want_v)
    assert torch.equal(ops.gather_max(feat, idx, k, qsel=qsel).cpu(), want)
    fb = c.feat.to(BF)
    cb = _Pool.__new__(_Pool)
    cb.__dict__.update(c.__dict__, feat=fb)
    assert torch.equal(ops.gather_max(fb.to(dev), idx, k, qsel=qsel).cpu(), torch.stack([m for m, _ in cb.route()]).to(BF))
    # the gradient of ones: integer counts, exact -- each listing routed to the FIRST slot holding the maximum
    f = feat.clone().requires_grad_(True)
    ops.pool_layer(f, xyz, idx, qsel, k)[0].backward(torch.ones(B, Nq, C, device=dev))
    assert torch.equal(f.grad.cpu().double(), c.backward_ref(torch.ones(B, Nq, C))[2])


def test_kept_rows_of_another_shape_are_refused(dev, ref):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError
    c = _Pool(ref, 3, 70, 17, 12, 4, 5)
    feat, idx, xyz = c.feat.to(dev), c.idx.to(dev), c.xyz.to(dev)
    for bad in (c.qsel[:2], c.qsel[:1], c.qsel.unsqueeze(-1), c.qsel.reshape(-1).reshape(1, 1, -1), c.qsel[:, :0]):
        with pytest.raises(HspError):
            ops.gather_max(feat, idx, 4, qsel=bad.contiguous().to(dev))
        with pytest.raises(HspError):
            ops.pool_layer(feat, xyz, idx, bad.contiguous().to(dev), 4)
        with pytest.raises(HspError):
            ops.gather_max(feat.to(BF), idx, 4, qsel=bad.contiguous().to(dev))


# (B, N, Nq, C, k, tile): the column-tile LDS scatter at its three widths' shapes; one cloud too long for any tile (fp32 only)
BWD = [(3, 70, 17, 12, 4, True), (2, 257, 64, 256, 4, True), (16, 1028, 257, 128, 4, True), (2, 9300, 300, 12, 4, False)]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,Nq,C,k,tile", BWD)
def test_per_cloud_pooling_backward_against_fp64(dev, ref, B, N, Nq, C, k, tile, dtype):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError, lib
    assert (lib().hsp_scatter_tile_plan(B, N, C, None) != 0) == tile
    c = _Pool(ref, B, N, Nq, C, k, 70 + N, dtype=dtype, ties=(C == 12), plant=True)
    g = ref.hash_tensor((B, Nq, C), 71 + N, 1.0).to(dtype)
    want, terms, cnt = c.backward_ref(g)
    assert cnt.max().item() >= 8, "no source row collects 8 contributions"
    feat, idx, qsel, xyz = c.feat.to(dev).requires_grad_(True), c.idx.to(dev), c.qsel.to(dev), c.xyz.to(dev)
    tol = A * U * terms + (2.0 ** -8 * want.abs() if dtype == BF else 0)
    forms = [lambda: ops.gather_max(feat, idx, k, qsel=qsel)]
    if dtype == torch.float32:
        forms.append(lambda: ops.pool_layer(feat, xyz, idx, qsel, k)[0])
    if dtype == BF and not tile:                                   # bf16 rows: the LDS tile form only -- an error, not another sampler
        with pytest.raises(HspError):
            forms[0]().backward(g.to(dev))
        return
    for form in forms:
        feat.grad = None
        form().backward(g.to(dev))
        err = (feat.grad.cpu().double() - want).abs()
        worst = (err / (U * terms).clamp_min(1e-300))[terms > 0].max().item() if dtype != BF else float("nan")
        print(f"  per-cloud pooling backward B{B} N{N} C{C} {dtype}: max err {err.max().item():.3e}, worst err / (2^-24 sum|terms|) {worst:.2f}")
        assert (err <= tol).all(), f"max excess {(err - tol).max().item():.3e}"
        assert (feat.grad.cpu()[terms == 0] == 0).all()


# (the cloud too long for an LDS tile: fp32 only -- bf16 rows have no backward there, through either entry)
SAME = [(3, 70, 17, 12, 4, torch.float32), (3, 70, 17, 12, 4, BF), (16, 1028, 257, 128, 4, torch.float32), (16, 1028, 257, 128, 4, BF),
        (2, 9300, 300, 12, 4, torch.float32)]


@pytest.mark.parametrize("B,N,Nq,C,k,dtype", SAME)
def test_one_list_for_all_clouds_equals_the_shared_entry(dev, ref, B, N, Nq, C, k, dtype):
    from hs_pose_amd import ops
    c = _Pool(ref, B, N, Nq, C, k, 90 + N, dtype=dtype, plant=True)
    shared = c.qsel[0].contiguous().to(dev)
    each = shared.expand(B, Nq).contiguous()
    g = torch.randint(-8, 9, (B, Nq, C), generator=torch.Generator().manual_seed(3)).to(dtype).to(dev)   # exact partial sums
    idx, xyz = c.idx.to(dev), c.xyz.to(dev)
    forms = [lambda f, q: ops.gather_max(f, idx, k, qsel=q)]
    if dtype == torch.float32:
        forms.append(lambda f, q: ops.pool_layer(f, xyz, idx, q, k)[0])
    for form in forms:
        res = []
        for q in (shared, each):
            f = c.feat.to(dev).requires_grad_(True)
            out = form(f, q)
            out.backward(g)
            res.append((out.detach(), f.grad))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert res[0][1].abs().max().item() > 8                    # (sums of several terms were compared)


def test_pool_layer_alone_samples_its_own_input(dev, ref):
    """Pool_layer's meaning is uniform -- FPS on ITS input --; the network's level-2 prefix is an exact shortcut of it"""
    from hs_pose_amd import gcn3d, ops
    B, N, C = 2, 257, 16
    xyz, feat = ref.hash_tensor((B, N, 3), 3, 0.1).to(dev), ref.hash_tensor((B, N, C), 4, 1.0).to(dev)
    pool = gcn3d.Pool_layer(4, 4, sampler="fps")
    state = torch.get_rng_state()
    v1, f1 = pool(xyz, feat)
    v2, f2 = pool(v1, f1)
    assert torch.equal(torch.get_rng_state(), state)
    sel1, w1, w2 = ops.fps_levels(xyz, 64, 16)
    assert torch.equal(v1, w1) and torch.equal(v2, w2)
    assert torch.equal(f1, ops.gather_max(feat, ops.knn(xyz, 4), 4, qsel=sel1))
    assert torch.equal(f2, ops.gather_max(f1, ops.knn(v1, 4), 4, qsel=torch.arange(16, dtype=torch.int32, device=dev)))
    for dt in (BF,):                                               # bf16 rows take the same rows
        assert torch.equal(pool(xyz, feat.to(dt))[1], ops.gather_max(feat.to(dt), ops.knn(xyz, 4), 4, qsel=sel1))


# ==== 5. - 8. the network ============================================================================================================

def _face_recon(dev, flags):
    from hs_pose_amd.FaceRecon import FaceRecon
    flags.train = 0                                                # (the stack alone, no train-only heads)
    torch.manual_seed(0)
    return FaceRecon().to(dev)


def _cloud(ref, B, N, seed, dev):
    pc = ref.hash_tensor((B, N, 3), seed, 0.05)
    obj = (torch.arange(B) % 6).float().reshape(B, 1)
    return (pc - pc.mean(dim=1, keepdim=True)).to(dev), obj.to(dev)


@pytest.mark.parametrize("N", [256, 1028])
def test_default_sampler_consumes_the_generator_as_before(dev, ref, flags, N):
    from hs_pose_amd.graph import draw_pool_indices
    net = _face_recon(dev, flags).eval()
    pc, obj = _cloud(ref, 2, N, 11, dev)
    assert flags.pool_sampler == "random"
    torch.manual_seed(77)
    with torch.no_grad():
        net(pc, obj)
    after_forward = torch.get_rng_state()
    torch.manual_seed(77)
    draw_pool_indices(N)
    assert torch.equal(after_forward, torch.get_rng_state())


@pytest.mark.parametrize("N", [256, 1028])
def test_network_eval_is_a_function_of_the_cloud(dev, ref, flags, N):
    """(a) no host generator, the same feat twice; (b) every cloud of the batch equals that cloud run ALONE through the existing
    random-sampler path fed its own picks [sel1[b], 0 .. n2-1].  Both are the eval arithmetic, which the project pins to 2e-6 of
    scale against the CPU reference, hence 4e-6 of feat's maximum between the two (a wrong cloud's selection shows as O(1))."""
    from hs_pose_amd import gcn3d, ops
    net = _face_recon(dev, flags).eval()
    pc, obj = _cloud(ref, 2, N, 12, dev)
    n1 = N // 4
    n2 = n1 // 4
    flags.pool_sampler = "fps"
    state = torch.get_rng_state()
    with torch.no_grad():
        feat = net(pc, obj)[2]
        again = net(pc, obj)[2]
    assert torch.equal(torch.get_rng_state(), state), "the 'fps' sampler consumed the host generator"
    assert torch.equal(feat, again)
    sel1 = ops.fps_levels(pc, n1, n2)[0]
    assert not torch.equal(sel1[0], sel1[1])
    flags.pool_sampler = "random"
    scale = feat.abs().max().item()
    for b in range(2):
        feed = [sel1[b].contiguous(), torch.arange(n2, dtype=torch.int32, device=dev)]
        with torch.no_grad(), gcn3d.pool_index_feed(feed):
            alone = net(pc[b:b + 1].contiguous(), obj[b:b + 1].contiguous())[2]
        diff = (feat[b:b + 1] - alone).abs().max().item()
        print(f"  eval N={N} cloud {b}: |batched fps - alone, fed| {diff:.3e} = {diff / scale:.2e} of max|feat| {scale:.3f}")
        assert diff <= 4e-6 * scale
    assert torch.equal(torch.get_rng_state(), state)              # (the fed path draws nothing either)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_network_train_equals_the_fed_random_path(dev, ref, flags, dtype):
    """B = 2 copies of one cloud: every cloud selects the same rows, so the random path fed [sel1[0], 0 .. n2-1] computes the
    same thing -- feat bit for bit (pooling forward is a max), gradients to the repeat-run bound 1e-4 of each gradient's maximum
    (the column-tile backward's float LDS adds are order-dependent; two runs of one code differ by 0.7 - 1.2e-5)."""
    from hs_pose_amd import gcn3d, ops
    N = 256
    net = _face_recon(dev, flags).train()
    if dtype == BF:
        net.set_feature_dtype(BF)
    one, _ = _cloud(ref, 1, N, 13, dev)
    pc, obj = one.expand(2, N, 3).contiguous(), torch.tensor([[1.0], [4.0]], device=dev)
    dfeat = None
    res = {}
    for how in ("fps", "random"):
        flags.pool_sampler = how
        sel1 = ops.fps_levels(pc, N // 4, N // 16)[0]
        feed = [sel1[0].contiguous(), torch.arange(N // 16, dtype=torch.int32, device=dev)]
        net.zero_grad(set_to_none=True)
        state = torch.get_rng_state()
        fed = iter(feed)
        with gcn3d.pool_index_feed(fed):
            feat = net(pc, obj)[2]
        assert torch.equal(torch.get_rng_state(), state)
        assert len(list(fed)) == (2 if how == "fps" else 0)        # 'fps' takes nothing from the feed either
        if dfeat is None:
            dfeat = ref.hash_tensor(tuple(feat.shape), 14, 1.0).to(dev).to(feat.dtype)
        feat.backward(dfeat)
        res[how] = (feat.detach(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert res["fps"][0].dtype == dtype and torch.equal(res["fps"][0], res["random"][0])
    assert res["fps"][1].keys() == res["random"][1].keys() and len(res["fps"][1]) > 20
    worst = 0.0
    for k, gr in res["random"][1].items():
        rel = (res["fps"][1][k] - gr).abs().max().item() / max(gr.abs().max().item(), 1e-30)
        worst = max(worst, rel)
        assert rel <= 1e-4, f"{k}: {rel:.3e} of max|grad|"
    print(f"  train {dtype}: worst |grad fps - grad fed| / max|grad| {worst:.2e}")


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
def test_graphed_step_samples_inside_the_graph(dev, ref, flags, split):
    from hs_pose_amd.graph import GraphedStep
    B, N = 2, 1028
    flags.pool_sampler = "fps"
    net_g, net_e = _face_recon(dev, flags).train(), _face_recon(dev, flags).train()
    pc, obj = _cloud(ref, B, N, 15, dev)
    other, _ = _cloud(ref, B, N, 16, dev)
    dfeat = ref.hash_tensor((B, N, 1286), 17, 1.0).to(dev)
    graphed = GraphedStep(net_g, pc.clone(), obj, dfeat, warmup=2, split=split)
    assert graphed.pool_idx is None, "index buffers under the 'fps' sampler"
    state = torch.get_rng_state()
    for cloud in (pc, other):                                      # the second: the selection is computed in the graph, not baked
        graphed.load_inputs(centred=cloud)
        for _ in range(2):
            feat_g = graphed.run()
        torch.cuda.synchronize()
        assert torch.equal(torch.get_rng_state(), state), "run() consumed the host generator"
        feat_e = net_e(cloud, obj)[2]
        assert torch.equal(feat_g, feat_e.detach())


def test_graphed_inference_samples_inside_the_graph(dev, ref, flags):
    from hs_pose_amd.geom_utils import generate_RT
    from hs_pose_amd.graph import GraphedInference
    from hs_pose_amd.HSPose import HSPose
    flags.train = 0
    flags.pool_sampler = "fps"
    torch.manual_seed(0)
    net = HSPose("PoseNet_only").to(dev).eval()
    N = 1028
    shift = torch.tensor([0.0, 0.0, 0.8])
    PC, other = ((ref.hash_tensor((1, N, 3), s, 0.05) + shift).to(dev) for s in (18, 19))
    obj = torch.tensor([2], device=dev)
    mean_shape = torch.tensor([[0.2, 0.15, 0.25]], device=dev)
    sym = torch.tensor([[1, 0, 0, 0]], dtype=torch.int32, device=dev)
    graphed = GraphedInference(net, PC.clone(), obj, mean_shape, sym)
    assert graphed.pool_idx is None
    state = torch.get_rng_state()
    for cloud in (PC, other):
        graphed.load(PC=cloud)
        for _ in range(2):
            RT_g, s_g, out_g = graphed.run()
        torch.cuda.synchronize()
        assert torch.equal(torch.get_rng_state(), state), "run() consumed the host generator"
        with torch.no_grad():
            out = net(PC=cloud, obj_id=obj, mean_shape=mean_shape, sym=sym)
            RT = generate_RT([out['p_green_R'], out['p_red_R']], [out['f_green_R'], out['f_red_R']], out['Pred_T'], mode='vec', sym=sym)
        for k in ('p_green_R', 'p_red_R', 'f_green_R', 'f_red_R', 'Pred_T', 'Pred_s'):
            assert torch.equal(out_g[k], out[k]), k
        assert torch.equal(RT_g, RT) and torch.equal(s_g, out['Pred_s'] + mean_shape)


def test_pool_layer_alone_with_coordinates_that_need_a_gradient(dev, ref):
    """the sampler's copy of the kept coordinates carries no gradient: the layer then gathers them (per-cloud rows) itself"""
    from hs_pose_amd import gcn3d, ops
    B, N, C = 2, 70, 16
    xyz = ref.hash_tensor((B, N, 3), 5, 0.1).to(dev).requires_grad_(True)
    feat = ref.hash_tensor((B, N, C), 6, 1.0).to(dev).requires_grad_(True)
    v1, f1 = gcn3d.Pool_layer(4, 4, sampler="fps")(xyz, feat)
    sel1, w1, _ = ops.fps_levels(xyz, 17, 0)
    assert torch.equal(v1.detach(), w1) and torch.equal(f1.detach(), ops.gather_max(feat.detach(), ops.knn(xyz, 4), 4, qsel=sel1))
    g = ref.hash_tensor((B, 17, 3), 7, 1.0).to(dev)
    (v1 * g).sum().backward()
    want = torch.zeros(B, N, 3, device=dev).scatter_add_(1, sel1.long().unsqueeze(-1).expand(-1, -1, 3), g)
    assert torch.equal(xyz.grad, want)                             # (the picks are different rows: one term per entry)


def test_network_exact_train_under_fps(dev, ref, flags):
    """the reference-order arithmetic under train-mode BatchNorm (FaceRecon.exact_train) with the 'fps' sampler: the same feat as
    the random path fed the picks, bit for bit, and nothing drawn on the host"""
    from hs_pose_amd import gcn3d, ops
    N = 256
    net = _face_recon(dev, flags).train()
    net.exact_train = True
    pc, obj = _cloud(ref, 1, N, 21, dev)
    pc, obj = pc.expand(2, N, 3).contiguous(), torch.tensor([[0.0], [3.0]], device=dev)
    sel1 = ops.fps_levels(pc, N // 4, N // 16)[0]
    state = torch.get_rng_state()
    flags.pool_sampler = "fps"
    feat = net(pc, obj)[2]
    feat.backward(torch.ones_like(feat))
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
    flags.pool_sampler = "random"
    with gcn3d.pool_index_feed([sel1[0].contiguous(), torch.arange(N // 16, dtype=torch.int32, device=dev)]):
        fed = net(pc, obj)[2]
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(feat.detach(), fed.detach())


def test_graphed_network_samples_inside_the_graph(dev, flags):
    """GraphedNetwork (posenet's forward / backward as two graphs behind one autograd node) under 'fps': no index buffers, and the
    step's losses and gradients equal the eager step's to the bounds tests/test_gpu_graph.py holds the random path to"""
    import ref_cpu as oc
    from hs_pose_amd.HSPose import HSPose
    B, N = 4, 256
    flags.train = 1
    flags.pool_sampler = "fps"
    flags.aug_bb_pro = flags.aug_rt_pro = flags.aug_bc_pro = flags.aug_pc_pro = -1.0
    keys = ("PC", "obj_id", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale")
    case = {k: v.to(dev) for k, v in oc.hspose_train_case(B, N, 7).items()}
    batch = {k: case[k] for k in keys}

    def make():
        torch.manual_seed(0)
        net = HSPose("PoseNet_only").to(dev).train()
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        return net

    def total_of(ld):
        return sum(sum(d.values()) for d in ld.values())

    net_g = make()
    runner = net_g.enable_graphed_posenet(batch["PC"], batch["obj_id"])
    assert runner.pool_idx is None
    for _ in range(2):
        net_g.zero_grad(set_to_none=True)
        _, ld_g = net_g(do_loss=True, **batch)
        total_of(ld_g).backward()
    net_e = make()
    _, ld_e = net_e(do_loss=True, **batch)
    total_of(ld_e).backward()
    torch.cuda.synchronize()
    for g in ld_e:
        for k in ld_e[g]:
            a, b = float(ld_e[g][k]), float(ld_g[g][k])
            assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), f"loss {g}.{k}: eager {a} graph {b}"
    grads_g = {k: p.grad for k, p in net_g.named_parameters()}
    gmax = max(p.grad.abs().max().item() for p in net_e.parameters() if p.grad is not None)
    for k, p in net_e.named_parameters():
        if p.grad is not None:
            assert (p.grad - grads_g[k]).abs().max().item() <= 1e-4 * gmax, k
