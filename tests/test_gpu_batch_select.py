"""hsp_batch_select on the GPU (csrc/frontend.hip; ops.batch_select, pc_sample.train_batch_select) against the numpy restatement
of its rule (tests/_batch_select_ref.py, written from include/hsp.h).  Everything compared is bytes: equality is exact."""
import numpy as np
import pytest
import torch

import _batch_select_ref as br

pytestmark = pytest.mark.gpu

GUARD = 64                                                           # guard bytes either side of every dst
# 16 segments: (row bytes, dtype, misalign the base by 4 bytes, fill row).  12-byte rows on a base that is only 4-byte aligned,
# 16-byte-multiple rows on such a base too (the 4-byte path), an int32 and an int64 segment, 12 KB rows (model_point)
SEGS = [(4, np.float32, False, False), (12, np.float32, True, False), (16, np.float32, False, True), (36, np.float32, False, False),
        (3072, np.float32, False, True), (12288, np.float32, False, False), (4, np.int32, False, True), (12, np.int32, False, True),
        (16, np.int32, True, False), (8, np.int64, False, False), (36, np.float32, True, True), (3072, np.uint8, True, False),
        (12288, np.float32, True, True), (48, np.float32, False, False), (20, np.int32, False, False), (4100, np.float32, False, False)]


def _random_cases():
    rng = np.random.RandomState(5)
    out = []
    for M in (63, 64, 65, 129, 1024):
        st = br.random_status(rng, M)
        out += [(st.tolist(), keep) for keep in (1, M // 2, M)]
    return out


CASES = [([0], 1), ([0, 0, 0, 0], 4), ([0, 1, 0, 4, 0, 0], 4), ([2, 0, 1, 4, 0, 3], 4), ([0, 0, 0, 0, 7, -1], 4),
         ([1, 2, 4, 7, -2 ** 31], 4), ([0, 3, 0, 0, 5], 4), ([0, 3, 0, 0, 0], 4)] + _random_cases()


def _rows(rng, M, row_bytes, dtype, status):
    """M rows of random bytes as ``dtype``; a rejected item's row is all 0xFF (a NaN as fp32), so a stray read shows"""
    a = rng.randint(0, 256, size=(M, row_bytes)).astype(np.uint8)
    a[np.asarray(status) != 0] = 0xFF
    return a.view(dtype)


def _on_device(a, dev, misalign):
    """a (rows, ...) -> a device tensor with those bytes whose base is 16-byte aligned + 4 when ``misalign``"""
    flat = torch.from_numpy(a.view(np.uint8).reshape(-1).copy())
    buf = torch.zeros(flat.numel() + 32, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 16 + (4 if misalign else 0)
    buf[off:off + flat.numel()] = flat.to(dev)
    return buf[off:off + flat.numel()].view(torch.from_numpy(a[:0].reshape(-1)).dtype).view(a.shape)


def _guarded(keep, row_bytes, dtype, dev, misalign):
    """-> (buffer, dst view (keep, elems) inside it): 0xA5 everywhere, GUARD bytes (+ the misalignment) on either side"""
    n = keep * row_bytes
    buf = torch.full((n + 2 * GUARD + 32,), 0xA5, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 16 + GUARD + (4 if misalign else 0)
    tdt = torch.from_numpy(np.zeros(0, dtype)).dtype
    return buf, buf[off:off + n].view(tdt).view(keep, -1), off, n


@pytest.mark.parametrize("status,keep", CASES, ids=[f"M{len(s)}k{k}V{sum(1 for v in s if v == 0)}" for s, k in CASES])
def test_sel_info_and_sixteen_segments_equal_restatement(dev, status, keep):
    from hs_pose_amd import ops
    M = len(status)
    rng = np.random.RandomState(M * 7 + keep)
    want_sel, want_info = br.select(status, keep)
    V = int(want_info[0])
    status_d = torch.tensor(status, dtype=torch.int32, device=dev)
    srcs, fills, segs, guards = [], [], [], []
    for row_bytes, dtype, misalign, with_fill in SEGS:
        src = _rows(rng, M, row_bytes, dtype, status)
        fill = rng.randint(0, 256, size=(1, row_bytes)).astype(np.uint8).view(dtype) if with_fill else None
        src_d = _on_device(src, dev, misalign)
        fill_d = None if fill is None else _on_device(fill, dev, misalign)[0]
        assert src_d.data_ptr() % 16 == (4 if misalign else 0) and src_d.is_contiguous()
        buf, dst, off, n = _guarded(keep, row_bytes, dtype, dev, misalign)
        assert dst.data_ptr() % 16 == (4 if misalign else 0)
        srcs.append(src)
        fills.append(None if fill is None else fill[0])
        segs.append((src_d, dst, fill_d))
        guards.append((buf, off, n))
    assert len(segs) == 16
    sel = torch.full((keep + 2,), -7, dtype=torch.int32, device=dev)
    info = torch.full((4,), -7, dtype=torch.int32, device=dev)
    dsts, got_sel, got_info = ops.batch_select(status_d, keep, segs, sel=sel[1:-1], info=info[1:3])
    torch.cuda.synchronize()
    assert np.array_equal(got_sel.cpu().numpy(), want_sel) and got_info.cpu().tolist() == want_info.tolist()
    assert sel[[0, -1]].cpu().tolist() == [-7, -7] and info[[0, 3]].cpu().tolist() == [-7, -7]
    for s, (src, fill, dst, (buf, off, n)) in enumerate(zip(srcs, fills, dsts, guards)):
        want = br.gather(src, want_sel, V, fill)
        got = dst.cpu().numpy().view(src.dtype).reshape(want.shape)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (s, SEGS[s])
        host = buf.cpu().numpy()
        assert (host[:off] == 0xA5).all() and (host[off + n:] == 0xA5).all(), (s, "guard bytes changed")
        if V >= 1:
            assert not (got.view(np.uint8).reshape(keep, -1) == 0xFF).all(axis=1).any(), (s, "a rejected item's row")
        elif fill is not None:
            assert all(np.array_equal(got[j].view(np.uint8).reshape(-1), fill.view(np.uint8).reshape(-1)) for j in range(keep))
        else:
            assert np.array_equal(got.view(np.uint8), src[:keep].view(np.uint8))


@pytest.mark.parametrize("status,keep", [([0, 5, 0], 2), ([3, 3, 3], 3), ([0] * 1024, 1024)])
def test_no_segments(dev, status, keep):
    from hs_pose_amd import ops
    dsts, sel, info = ops.batch_select(torch.tensor(status, dtype=torch.int32, device=dev), keep)
    want_sel, want_info = br.select(status, keep)
    assert dsts == [] and np.array_equal(sel.cpu().numpy(), want_sel) and info.cpu().tolist() == want_info.tolist()


def test_fresh_outputs_and_wrapper_refusals(dev):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError
    status = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device=dev)
    a = torch.arange(4 * 6, dtype=torch.float32, device=dev).reshape(4, 2, 3)
    ids = torch.tensor([10, 11, 12, 13], dtype=torch.int64, device=dev)
    (ga, gi), sel, info = ops.batch_select(status, 3, [(a, None, None), (ids, None, None)])
    assert ga.shape == (3, 2, 3) and torch.equal(ga, a[[0, 2, 3]]) and gi.tolist() == [10, 12, 13] and gi.dtype == torch.int64
    assert sel.tolist() == [0, 2, 3] and info.tolist() == [3, 3]
    with pytest.raises(HspError):
        ops.batch_select(status, 5)                                                   # keep > M
    with pytest.raises(HspError):
        ops.batch_select(status, 2, [(torch.zeros(4, 3, dtype=torch.uint8, device=dev), None, None)])   # a 3-byte row
    with pytest.raises(HspError):
        ops.batch_select(status, 2, [(a, None, None)] * 17)
    with pytest.raises(HspError):
        ops.batch_select(status, 2, [(a[:3], None, None)])                            # M rows expected
    with pytest.raises(HspError):
        ops.batch_select(status.cpu(), 2)


# ---- the chain: train_batch_to_pcl -> train_batch_select --------------------------------------------------------------------------

K_SMALL = np.array([[120.0, 0.0, 32.0], [0.0, 120.0, 24.0], [0.0, 0.0, 1.0]])
EXTRA_SHAPES = dict(obj_id=(), gt_R=(3, 3), gt_t=(3,), gt_s=(3,), mean_shape=(3,), sym=(4,), aug_bb=(3,), aug_rt_t=(3,),
                    aug_rt_r=(3, 3), model_point=(1024, 3), nocs_scale=())


def _chain_batch(rng):
    """M = 6 items on 48 x 64 frames: items 0, 2 and 5 good (a disc of depth each); item 1's inst_id is absent from its label
    image (status bit 2, with 0 and... whatever follows from an empty mask), item 3's mask is 3 x 3 pixels (bit 0), item 4's
    mask lies over zero depth (bit 1)"""
    M, H, W = 6, 48, 64
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (700 + 40 * np.sin(xx / 5.0) + 30 * np.cos(yy / 4.0))[None].repeat(M, 0) + rng.randint(0, 20, size=(M, H, W))
    depth = depth.astype(np.uint16)
    labels = np.zeros((M, H, W), np.uint8)
    ids = np.array([3, 9, 5, 2, 6, 1], dtype=np.int32)
    boxes = np.zeros((M, 4), np.int64)
    for j, (cy, cx, r) in enumerate([(24, 30, 14), (20, 30, 12), (26, 34, 13), (24, 32, 12), (22, 30, 13), (25, 28, 14)]):
        labels[j][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = ids[j]
        boxes[j] = (cx - r, cy - r, cx + r, cy + r)
    labels[1][labels[1] == 9] = 8                                   # inst_id 9 is nowhere in item 1's label image
    labels[3] = 0
    labels[3][23:26, 31:34] = ids[3]                                # a 3 x 3 mask
    depth[4] = 0                                                    # a mask over zero depth
    return depth, labels, ids, boxes


def _extras(rng, M, dev):
    out = {}
    for k, shape in EXTRA_SHAPES.items():
        if k == "obj_id":
            out[k] = torch.from_numpy(rng.randint(0, 6, size=(M,)).astype(np.int64)).to(dev)
        else:
            out[k] = torch.from_numpy(rng.randn(M, *shape).astype(np.float32)).to(dev)
    return out


def _select_chain(dev, depth, labels, ids, centers, scales, extras, seed, keep=4):
    from hs_pose_amd.pc_sample import DeviceSampler, train_batch_select, train_batch_to_pcl
    args = dict(n_pts=64, out_size=32, min_pts=50, mask_pro=1.0)
    d, l = torch.from_numpy(depth).to(dev), torch.from_numpy(labels).to(dev)
    PC, status = train_batch_to_pcl(d, l, ids, centers, scales, K_SMALL, sampler=DeviceSampler(seed, dev), **args)
    batch, sel, info = train_batch_select(PC, status, keep, extras)
    twin_PC, twin_status = train_batch_to_pcl(d, l, ids, centers, scales, K_SMALL, sampler=DeviceSampler(seed, dev), **args)
    assert torch.equal(status, twin_status)
    return batch, sel, info, twin_PC, status


def test_chain_picks_the_good_items_and_ignores_the_rejected(dev, flags):
    from hs_pose_amd.pc_sample import dzi_windows
    flags.DZI_TYPE = "none"                                         # (the undrawn windows: the boxes' own centres and sides)
    rng = np.random.RandomState(31)
    depth, labels, ids, boxes = _chain_batch(rng)
    centers, scales = dzi_windows(boxes, 48, 64)
    extras = _extras(rng, 6, dev)
    batch, sel, info, twin_PC, status = _select_chain(dev, depth, labels, ids, centers, scales, extras, 11)
    st = status.cpu().numpy()
    assert (st[[0, 2, 5]] == 0).all() and st[1] & 4 and st[3] & 1 and st[4] & 2, st
    assert st[3] == 1                                               # (the 3 x 3 mask: fewer than min_pts, nothing else)
    sel_ref, info_ref = br.select(st, 4)
    assert sel_ref.tolist() == [0, 2, 5, 0] and info_ref.tolist() == [3, 3]
    assert np.array_equal(sel.cpu().numpy(), sel_ref) and info.cpu().tolist() == info_ref.tolist()
    idx = torch.from_numpy(sel_ref.astype(np.int64)).to(dev)
    assert set(batch) == {"PC"} | set(extras)
    assert batch["PC"].shape == (4, 64, 3) and torch.isfinite(batch["PC"]).all() and torch.isnan(twin_PC[[1, 3, 4]]).all()
    assert torch.equal(batch["PC"].view(torch.int32), twin_PC[idx].view(torch.int32))
    for k, v in extras.items():
        assert batch[k].dtype == v.dtype and batch[k].shape == (4,) + v.shape[1:], k
        assert torch.equal(batch[k].view(torch.int32), v[idx].contiguous().view(torch.int32)), k
    # a rejected item's depth, labels and ground truth change while it stays rejected: the selected batch keeps every bit
    depth2, labels2 = depth.copy(), labels.copy()
    depth2[1] = rng.randint(1, 3000, size=depth[1].shape)
    labels2[1] = rng.randint(10, 20, size=labels[1].shape)          # (still without id 9)
    depth2[3] += 100
    labels2[4] = np.roll(labels[4], 3, axis=1)                      # (still over zero depth)
    extras2 = {k: v.clone() for k, v in extras.items()}
    for k, v in extras2.items():
        v[[1, 3, 4]] = (v[[1, 3, 4]] * 0 + 7) if v.dtype.is_floating_point else 5
    batch2, sel2, info2, _, status2 = _select_chain(dev, depth2, labels2, ids, centers, scales, extras2, 11)
    assert ((status2 != 0) == (status != 0)).all() and torch.equal(sel2, sel) and torch.equal(info2, info)
    for k in batch:
        assert torch.equal(batch2[k].view(torch.int32), batch[k].view(torch.int32)), k


def test_chain_all_rejected_gives_the_stand_in(dev, flags):
    from hs_pose_amd.pc_sample import dzi_windows, stand_in_cloud
    flags.DZI_TYPE = "none"
    rng = np.random.RandomState(32)
    depth, labels, ids, boxes = _chain_batch(rng)
    centers, scales = dzi_windows(boxes, 48, 64)
    extras = _extras(rng, 6, dev)
    batch, sel, info, twin_PC, status = _select_chain(dev, depth, labels, ids + 100, centers, scales, extras, 12)
    assert (status != 0).all() and torch.isnan(twin_PC).all()
    assert sel.tolist() == [0, 1, 2, 3] and info.tolist() == [0, 0]
    want = stand_in_cloud(64, dev)
    g = torch.Generator().manual_seed(0)
    assert torch.equal(want.cpu(), (torch.rand(64, 3, generator=g) - 0.5) * 0.2)         # FramePipeline's stand-in, value for value
    assert all(torch.equal(batch["PC"][j], want) for j in range(4))
    for k, v in extras.items():
        assert torch.equal(batch[k], v[:4]), k


def test_select_is_capturable_with_caller_buffers(dev):
    from hs_pose_amd.pc_sample import stand_in_cloud, train_batch_select
    M, keep, n = 5, 3, 16
    PC = torch.randn(M, n, 3, device=dev)
    status = torch.tensor([0, 1, 0, 0, 2], dtype=torch.int32, device=dev)
    extras = {"gt_t": torch.randn(M, 3, device=dev), "obj_id": torch.arange(M, device=dev)}
    out = {"PC": torch.empty(keep, n, 3, device=dev), "gt_t": torch.empty(keep, 3, device=dev),
           "obj_id": torch.empty(keep, dtype=torch.int64, device=dev)}
    sel, info = torch.empty(keep, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    stand_in_cloud(n, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        train_batch_select(PC, status, keep, extras, out=out, sel=sel, info=info)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        batch, s2, i2 = train_batch_select(PC, status, keep, extras, out=out, sel=sel, info=info)
    assert s2 is sel and i2 is info and all(batch[k] is out[k] for k in out)
    for st in ([0, 1, 0, 0, 2], [1, 1, 0, 1, 1], [4, 4, 4, 4, 4]):
        status.copy_(torch.tensor(st, dtype=torch.int32, device=dev))
        g.replay()
        want_sel, want_info = br.select(st, keep)
        assert sel.tolist() == want_sel.tolist() and info.tolist() == want_info.tolist()
        idx = torch.from_numpy(want_sel.astype(np.int64)).to(dev)
        assert torch.equal(out["gt_t"], extras["gt_t"][idx]) and torch.equal(out["obj_id"], extras["obj_id"][idx])
        want_PC = PC[idx] if want_info[0] else stand_in_cloud(n, dev).expand(keep, n, 3)
        assert torch.equal(out["PC"], want_PC)
