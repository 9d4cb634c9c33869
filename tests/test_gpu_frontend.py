"""GPU parity (through the C-ABI): depth -> cloud front end, pose-matrix back end and the HSPose facade
against the fixtures written by the reference (tests/golden/frontend_*.npz) and the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu


def _inputs(ref):
    g = golden("frontend_pc_sample")
    return g, ref.frontend_inputs(3, 64, 80, 900, [float(r) for r in g["radii"]])


def test_pc_compact_is_row_major_boolean_indexing(dev, ref):
    from hs_pose_amd import ops
    g, (mask, depth, camK, coor) = _inputs(ref)
    pix, count = ops.pc_compact(mask.reshape(3, -1).to(dev), depth.reshape(3, -1).to(dev))
    assert list(count.cpu().numpy()) == list(g["counts"])
    for b in range(3):
        want = ref.valid_pixels(mask[b], depth[b]).numpy()
        assert np.array_equal(pix[b, :len(want)].cpu().numpy(), want)          # integer work: bit-exact


@pytest.mark.parametrize("HW", [1, 63, 1024, 1025, 4095, 4096, 4097, 65536, 256 * 256 + 7, 480 * 640])
def test_pc_compact_sizes(dev, ref, HW):
    from hs_pose_amd import ops
    m = (ref.hash_tensor((2, HW), 31, 0.5, 0.5) > 0.4).float()
    d = ref.hash_tensor((2, HW), 32, 1.0) * 900.0                               # about half non-positive
    pix, count = ops.pc_compact(m.to(dev), d.to(dev))
    for b in range(2):
        want = ref.valid_pixels(m[b], d[b]).numpy()
        assert int(count[b]) == len(want)
        assert np.array_equal(pix[b, :len(want)].cpu().numpy(), want)


def test_pc_compact_past_256_chunks(dev):
    """258 chunks: the write kernel's sum over the earlier chunks' counts, one count per thread, makes a second trip"""
    from hs_pose_amd import ops
    HW = 257 * 4096 + 5
    rng = np.random.RandomState(41)
    m = (rng.rand(1, HW) < 0.3).astype(np.float32)
    d = (rng.rand(1, HW) * 900.0).astype(np.float32)
    d[rng.rand(1, HW) < 0.2] = 0.0
    m[0, -1], d[0, -1] = 1.0, 5.0                                               # (the five-pixel last chunk is not empty)
    pix, count = ops.pc_compact(torch.from_numpy(m).to(dev), torch.from_numpy(d).to(dev))
    want = np.flatnonzero((m[0] > 0) & (d[0] > 0))
    assert (want >= 256 * 4096).sum() > 1000 and want[-1] == HW - 1
    assert int(count[0]) == len(want)
    assert np.array_equal(pix[0, :len(want)].cpu().numpy(), want)


def test_pc_compact_all_and_none(dev, ref):
    """every pixel valid (the ids fill the whole row) and no pixel valid (count 0), several chunks per image"""
    from hs_pose_amd import ops
    HW = 3 * 4096 + 100
    ones = torch.ones(2, HW)
    depth = torch.full((2, HW), 700.0)
    depth[1] = 0.0
    pix, count = ops.pc_compact(ones.to(dev), depth.to(dev))
    assert count.cpu().tolist() == [HW, 0]
    assert torch.equal(pix[0].cpu(), torch.arange(HW, dtype=torch.int32))


def test_pc_sample_matches_reference(dev, ref, flags):
    from hs_pose_amd.pc_sample import PC_sample
    g, (mask, depth, camK, coor) = _inputs(ref)
    flags.random_points = 1028
    np.random.seed(7)
    pc = PC_sample(mask.to(dev), depth.to(dev), camK.to(dev), coor.to(dev))
    assert pc.shape == (3, 1028, 3) and pc.dtype == torch.float32
    assert np.array_equal(pc.cpu().numpy(), g["pc"])                            # same fp32 op order: exact
    # the global numpy generator was consumed exactly like the reference: the next draw agrees
    rs = np.random.RandomState(7)
    for c in g["counts"]:
        rs.choice(int(c), 1028, replace=int(c) < 1028)
    assert np.random.randint(1 << 30) == rs.randint(1 << 30)
    logits = torch.cat([ref.hash_tensor((3, 1, 64, 80), 950, 1.0),
                        2.0 * mask - 1.0 + ref.hash_tensor((3, 1, 64, 80), 951, 0.5)], dim=1)
    np.random.seed(8)
    pc2 = PC_sample(logits.to(dev), depth.to(dev), camK.to(dev), coor.to(dev))
    assert np.array_equal(pc2.cpu().numpy(), g["pc_logits"])


def test_pc_sample_too_few_pixels_returns_none_pair(dev, ref, flags):
    from hs_pose_amd.pc_sample import PC_sample
    from hs_pose_amd.HSPose import HSPose
    g, (mask, depth, camK, coor) = _inputs(ref)
    mask[1] = 0
    mask[1, 0, 3, 4] = 1.0
    depth[1, 0, 3, 4] = 700.0
    np.random.seed(9)
    assert PC_sample(mask.to(dev), depth.to(dev), camK.to(dev), coor.to(dev)) == (None, None)   # pc_sample.py:59-60
    flags.train = 0
    net = HSPose("PoseNet_only").to(dev).eval()
    out = net(depth=depth.to(dev), camK=camK.to(dev), gt_2D=coor.to(dev), def_mask=mask.to(dev),
              obj_id=torch.zeros(3, 1, device=dev))
    assert out == ({}, None)                                                    # HSPose.py:47-48


def test_depth_to_pcl_matches_loader(dev, ref):
    from hs_pose_amd.pc_sample import depth_to_pcl
    g = golden("frontend_depth_to_pcl")
    _, (mask, depth, camK, coor) = _inputs(ref)
    for b, seed in ((0, 11), (1, 12)):
        np.random.seed(seed)
        pcl = depth_to_pcl(depth[b:b + 1].to(dev), g["K"], coor[b:b + 1].to(dev), mask[b:b + 1].to(dev), n_pts=1028)
        assert np.array_equal(pcl[0].cpu().numpy(), g[f"pcl{b}"])              # float64 arithmetic, one rounding
    few = mask.clone()
    few[0] = 0
    few[0, 0, :5, :5] = 1.0                                                     # < 50 valid pixels: item rejected
    assert depth_to_pcl(depth.to(dev), g["K"], coor.to(dev), few.to(dev)) is None


def test_generate_rt_matches_reference(dev, ref):
    from hs_pose_amd.geom_utils import generate_RT, to_R_matrices
    g = golden("frontend_generate_rt")
    pg, pr, fg, fr, T, sym = [t.to(dev) for t in ref.generate_rt_inputs()]
    rt = generate_RT([pg, pr], [fg, fr], T, mode="vec", sym=sym)
    assert rt.shape == (16, 4, 4)
    assert np.abs(rt.cpu().numpy() - g["rt"]).max() < 1e-5                      # sin/cos/acos: device libm
    R = to_R_matrices(fg, fr, pg, pr)
    nosym = (sym[:, 0] != 1).cpu()
    assert np.abs(R.cpu().numpy()[nosym] - g["rt"][nosym][:, :3, :3]).max() < 1e-5
    gt = generate_RT(torch.eye(3, device=dev).expand(16, 3, 3), None, T, mode="gt", sym=sym)
    assert torch.equal(gt[:, :3, :3].cpu(), torch.eye(3).expand(16, 3, 3)) and torch.equal(gt[:, :3, 3], T)


def test_hspose_eval_matches_posenet_fixture(dev, ref, flags, monkeypatch):
    """evaluation/evaluate.py:91-106: network(PC=, obj_id=, mean_shape=, sym=) -> generate_RT -> pred_s."""
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.geom_utils import generate_RT
    from test_gpu_stack import ForcedFeatKnn, _inputs as stack_inputs
    g = golden("stack_eval_256")
    train_flag, B, N, seed, bn_training = (int(v) for v in g["meta"])
    flags.train = train_flag
    net = HSPose("PoseNet_only")
    sd = net.posenet.state_dict()
    ref.fill_state_closed_form(sd)
    net = net.to(dev).eval()
    PC, obj = stack_inputs(ref, B, N, seed, dev)
    sym = torch.zeros(B, 4, device=dev)
    sym[0, 0] = 1.0
    ForcedFeatKnn(monkeypatch, g, dev)
    torch.manual_seed(1)
    out = net(PC=PC, obj_id=obj, mean_shape=torch.zeros(B, 3, device=dev), sym=sym)
    assert list(out) == ["mask", "sketch", "recon", "PC", "face_normal", "face_dis", "face_f", "p_green_R", "p_red_R",
                         "f_green_R", "f_red_R", "Pred_T", "Pred_s", "gt_R", "gt_t", "gt_s"]
    names = ("p_green_R", "p_red_R", "f_green_R", "f_red_R", "Pred_T", "Pred_s")
    for k in names:
        assert np.abs(out[k].detach().cpu().numpy() - g["out." + k]).max() <= 1e-4, k
    assert out["recon"] is None and out["mask"] is None and torch.equal(out["PC"], PC)
    rt = generate_RT([out["p_green_R"], out["p_red_R"]], [out["f_green_R"], out["f_red_R"]], out["Pred_T"],
                     mode="vec", sym=sym)
    want = ref.generate_rt(*[torch.from_numpy(g["out." + k]) for k in names[:5]], sym.cpu())
    assert (rt.cpu() - want).abs().max() < 1e-3                                 # 1e-4 inputs through acos


def test_hspose_branches_the_reference_does_not_implement(dev, flags):
    """the depth entry exists only for 'PoseNet_only' (HSPose.py:49-50 raises otherwise); unknown stages have no loss set"""
    from hs_pose_amd.HSPose import HSPose
    flags.train = 0
    with pytest.raises(NotImplementedError):
        HSPose("FSNet_only").to(dev)(depth=torch.zeros(1, 1, 4, 4, device=dev))
    with pytest.raises(NotImplementedError):
        HSPose("Backbone_only")


def test_eval_loop_surrogate(dev, ref, flags, tmp_path):
    """BASELINE configs[4]'s pinned SURROGATE (the REAL275 dataset / detections / published checkpoint are not available offline):
    the loop of evaluation/evaluate.py end to end against the imported reference (oracle/gen_golden_eval_loop.py) --
      1. the mirrored HSPose built under FLAGS.train = 1 and the reference's seed writes the reference's checkpoint (samples + sums
         of all 160 tensors), BatchNorm running statistics moved off their defaults;
      2. the file is reloaded as evaluate.py:39,58-73 does: FLAGS.train = False before construction, train-only heads dropped,
         'resconv' -> 'STE_layer', strict=True, eval();
      3. images of 1, 4 and 6 instances x 1028 points (each image holds a TILED short crop): network(PC=, obj_id=, mean_shape=, sym=)
         -> generate_RT(mode='vec') -> pred_s, FREE-RUNNING (nothing replayed), issued eagerly through the compiled binding AND as
         a hipGraph replay: pred_RT and pred_s within 1e-5 of the reference's."""
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.geom_utils import generate_RT
    from hs_pose_amd.graph import GraphedInference, draw_pool_indices
    g = golden("eval_loop_1028")
    flags.train = 1
    torch.manual_seed(0)
    trained = HSPose("PoseNet_only")
    sd = trained.state_dict()
    ref.eval_loop_move_bn_stats(sd)
    assert len(sd) == int(g["meta"][2]) == 160
    for k_, v in sd.items():
        if v.is_floating_point():
            flat = v.reshape(-1)
            assert np.array_equal(flat[::997].numpy(), g["wsample." + k_]), f"checkpoint tensor {k_} differs from the reference's"
            assert abs(flat.double().sum().item() - g["wsum." + k_][0]) <= 1e-9 * max(1.0, g["wsum." + k_][1]), k_
    path = str(tmp_path / "model_149.pth")
    torch.save({"seed": 0, "epoch": 149, "posenet_state_dict": sd, "scheduler": {}, "optimizer": {}}, path)
    # evaluation/evaluate.py:39,58-73
    flags.train = False
    network = HSPose("PoseNet_only").to(dev)
    state_dict = torch.load(path)["posenet_state_dict"]
    unnecessary_nets = ["posenet.face_recon.conv1d_block", "posenet.face_recon.face_head", "posenet.face_recon.recon_head"]
    for key in list(state_dict.keys()):
        for net_to_delete in unnecessary_nets:
            if key.startswith(net_to_delete):
                state_dict.pop(key)
        if "resconv" in key:
            state_dict[key.replace("resconv", "STE_layer")] = state_dict.pop(key)
    network.load_state_dict(state_dict, strict=True)
    network = network.eval()
    # eval BatchNorm's 1 / sqrt(var + eps) comes from the HOST's ATen (ops._eval_invstd: the reference's own is MKL's vector sqrt,
    # within an ulp but host-specific).  Where this host rounds a channel differently from the host that wrote the fixture, the
    # fixture's value is used for the three BatchNorms whose outputs are ranked -- what is under test is the device path
    from hs_pose_amd import ops
    for nm in ("bn1", "bn2", "bn3"):
        bn = getattr(network.posenet.face_recon, nm)
        inv = ops._eval_invstd(bn)
        differ = int((inv.cpu().numpy() != g["invstd." + nm]).sum())
        if differ:
            print(f"{nm}: this host's 1 / sqrt(var + eps) differs from the fixture host's in {differ} of {inv.numel()} channels")
            bn._hsp_invstd = (bn._hsp_invstd[0], torch.from_numpy(g["invstd." + nm]).to(dev))
    lists = []
    real_knn = ops.knn

    def rec(x, k, *a, **kw):
        o = real_knn(x, k, *a, **kw)
        if x.shape[-1] != 3:
            lists.append(o)
        return o
    # the Pool_layer randperm stream is consumed image after image (gcn3d.py:243): the generator state before each image
    torch.manual_seed(1)
    states = {}
    for n_inst in sorted(ref.EVAL_LOOP_IMAGES):
        states[n_inst] = torch.get_rng_state()
        draw_pool_indices(1028)
    worst = {}
    for n_inst in sorted(ref.EVAL_LOOP_IMAGES):
        PC, obj, mean_shape, sym = (t.to(dev) for t in ref.eval_loop_inputs(n_inst))
        # (a) eagerly, evaluate.py:90-106 as written
        torch.set_rng_state(states[n_inst])
        del lists[:]
        ops.knn = rec
        try:
            with torch.no_grad():
                out = network(PC=PC, obj_id=obj, mean_shape=mean_shape, sym=sym)
        finally:
            ops.knn = real_knn
        if n_inst == 4:
            agree = [float((l_.cpu().numpy() == g[f"n4.featknn{i + 1}"]).all(-1).mean()) for i, l_ in enumerate(lists[:4])]
            print("4-instance image: rows with the reference's ordered feature-space list per HS layer", agree)
            assert agree == [1.0, 1.0, 1.0, 1.0], agree
        errs = {k_: float(np.abs(out[k_].cpu().numpy() - g[f"n{n_inst}.{k_}"]).max())
                for k_ in ("p_green_R", "p_red_R", "f_green_R", "f_red_R", "Pred_T", "Pred_s")}
        print(f"{n_inst}-instance image, network outputs:", {k_: float(f"{v:.2e}") for k_, v in errs.items()})
        pred_s = out["Pred_s"].detach() + mean_shape
        pred_RT = generate_RT([out["p_green_R"].detach(), out["p_red_R"].detach()], [out["f_green_R"].detach(), out["f_red_R"].detach()],
                              out["Pred_T"].detach(), mode="vec", sym=sym)
        assert out["recon"] is None
        e_rt = float(np.abs(pred_RT.cpu().numpy() - g[f"n{n_inst}.pred_RT"]).max())
        e_s = float(np.abs(pred_s.cpu().numpy() - g[f"n{n_inst}.pred_s"]).max())
        # (b) the same image as a hipGraph replay
        gi = GraphedInference(network, PC.clone(), obj.clone(), mean_shape.clone(), sym.clone())
        torch.set_rng_state(states[n_inst])
        rt_g, s_g, _ = gi.run()
        torch.cuda.synchronize()
        g_rt = float(np.abs(rt_g.cpu().numpy() - g[f"n{n_inst}.pred_RT"]).max())
        g_s = float(np.abs(s_g.cpu().numpy() - g[f"n{n_inst}.pred_s"]).max())
        worst[n_inst] = (e_rt, e_s, g_rt, g_s)
    print("EVAL LOOP SURROGATE (n instances: max abs error of pred_RT / pred_s eager, then graph replay):",
          {n_: tuple(float(f"{v:.2e}") for v in w) for n_, w in worst.items()})
    for n_inst, w in worst.items():
        assert max(w) <= 1e-5, (n_inst, w)
