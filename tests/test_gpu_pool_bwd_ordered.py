"""The ORDERED pooling backward (config.FLAGS.reproducible; csrc/csr.hip: hsp_rev_build_sel, csrc/gather.hip:
hsp_gather_max_bwd_csr / _bf16) against the numpy restatement of include/hsp.h's contract (tests/_pool_bwd_ref.py), BIT for bit, in
fp32 and bf16 storage: one fp32 sum per (cloud, source row, column) over the queries in ascending order.  The gradients spread
over 17 binades, so another order changes bits (tests/test_reproducible_host.py measures how many).  Then the same through
autograd under the switch, the launches of the switch-off path unchanged, and the bad-argument codes."""
import numpy as np
import pytest
import torch

import _pool_bwd_ref as pref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _grad(ref, shape, seed):
    """hash_tensor scaled by 2^(h mod 17 - 8), h a 24-bit hash of the element: magnitudes over 17 binades"""
    n = int(np.prod(shape))
    h = (ref.hash_unit(n, seed + 1000) * (1 << 24)).astype(np.int64)
    return ref.hash_tensor(shape, seed, 1.0) * torch.from_numpy(2.0 ** (h % 17 - 8)).float().view(*shape)


def _case(ref, name):
    """-> dict(idx (B,Nidx,kstride) int32, qsel None / (Nq,) / (B,Nq) int32, argmax (B,Nq,C) uint8, g (B,Nq,C) fp32, Nsrc, k)"""
    rng = np.random.RandomState(sum(map(ord, name)))
    kpad, qsel = 0, None
    if name.startswith("plain"):
        B, Nsrc, Nq, k, C = {"plain0": (2, 16, 4, 4, 4), "plain1": (2, 19, 4, 4, 132), "plain2": (3, 257, 64, 4, 128),
                             "plain3": (2, 64, 64, 8, 128)}[name]
        Nidx = Nq
        idx = rng.randint(0, Nsrc, size=(B, Nidx, k))
    elif name == "kstride":                                   # lists wider than k: the columns past k are never read
        B, Nsrc, Nidx, Nq, k, C, kpad = 2, 33, 12, 12, 4, 8, 3
        idx = rng.randint(0, Nsrc, size=(B, Nidx, k))
    elif name in ("shared", "percloud", "repeated"):
        B, Nsrc, Nidx, Nq, k, C = 3, 64, 64, 16, 4, 128
        idx = rng.randint(0, Nsrc, size=(B, Nidx, k))
        if name == "shared":
            qsel = rng.permutation(Nidx)[:Nq]
        elif name == "percloud":
            qsel = np.stack([rng.permutation(Nidx)[:Nq] for _ in range(B)])
        else:                                                 # a tiled cloud's list: rows named more than once
            qsel = rng.randint(0, 5, size=(B, Nq))
    elif name == "hub":                                       # every slot of every list names row 0 or 1: in-degree ~ Nq / 2
        B, Nsrc, Nidx, Nq, k, C = 2, 64, 64, 64, 8, 128
        idx = rng.randint(0, 2, size=(B, Nidx, k))
    elif name == "empty_rows":                                # odd source rows receive nothing
        B, Nsrc, Nidx, Nq, k, C = 2, 40, 24, 24, 4, 12
        idx = 2 * rng.randint(0, Nsrc // 2, size=(B, Nidx, k))
    elif name == "large":                                     # past the LDS tile of the scatter form (Nsrc * 16 B > 144 KiB) and
        B, Nsrc, Nidx, Nq, k, C = 1, 30000, 1500, 1500, 4, 4  # past the reverse build's in-LDS edge array
        idx = rng.randint(0, Nsrc, size=(B, Nidx, k))
    else:
        raise KeyError(name)
    if kpad:
        idx = np.concatenate([idx, rng.randint(0, Nsrc, size=(B, Nidx, kpad))], axis=2)
    seed = 50 + sum(map(ord, name))
    return dict(idx=np.ascontiguousarray(idx, dtype=np.int32), qsel=None if qsel is None else np.ascontiguousarray(qsel, dtype=np.int32),
                argmax=rng.randint(0, k, size=(B, Nq, C)).astype(np.uint8), g=_grad(ref, (B, Nq, C), seed), Nsrc=Nsrc, k=k)


CASES = ["plain0", "plain1", "plain2", "plain3", "kstride", "shared", "percloud", "repeated", "hub", "empty_rows", "large"]


def _qargs(qsel_d):
    """(pointer, qsel_stride) of a kept-row list on the device"""
    from hs_pose_amd import ops
    if qsel_d is None:
        return ops._vp(0), 0
    return ops._p(qsel_d), (0 if qsel_d.dim() == 1 else qsel_d.shape[1])


def _rev(dev, c):
    from hs_pose_amd import ops
    idx = torch.from_numpy(c["idx"]).to(dev)
    qsel = None if c["qsel"] is None else torch.from_numpy(c["qsel"]).to(dev)
    B, Nidx, kstride = idx.shape
    Nq = Nidx if qsel is None else qsel.shape[-1]
    off = torch.full((B, c["Nsrc"] + 1), -7, dtype=torch.int32, device=dev)
    edge = torch.full((B, Nq * c["k"]), -7, dtype=torch.int32, device=dev)
    qp, qs = _qargs(qsel)
    ops._run("hsp_rev_build_sel", (ops._p(idx), qp, qs, B, Nidx, Nq, c["Nsrc"], c["k"], kstride, ops._p(off), ops._p(edge), ops._stream()))
    return idx, qsel, off, edge


@pytest.mark.parametrize("name", CASES)
def test_ordered_backward_equals_restatement(dev, ref, name):
    from hs_pose_amd import ops
    c = _case(ref, name)
    idx, qsel, off, edge = _rev(dev, c)
    B, Nq, C = c["g"].shape
    Nsrc, k = c["Nsrc"], c["k"]
    want_off, want_edge = pref.rev_index(c["idx"], c["qsel"], Nsrc, k)
    assert np.array_equal(off.cpu().numpy(), want_off), "rev_off"
    assert np.array_equal(edge.cpu().numpy(), want_edge), "rev_edge (ascending edge ids per source row)"
    if c["qsel"] is None:                                     # the same map as hsp_rev_build's
        off0, edge0 = torch.empty_like(off), torch.empty_like(edge)
        ops._run("hsp_rev_build", (ops._p(idx), B, Nq, Nsrc, k, idx.shape[2], ops._p(off0), ops._p(edge0), ops._stream()))
        assert torch.equal(off0, off) and torch.equal(edge0, edge)
    arg = torch.from_numpy(c["argmax"]).to(dev)
    for dtype in (torch.float32, BF16):
        g = c["g"].to(dev).to(dtype).contiguous()
        gfeat = torch.full((B, Nsrc, C), float("nan"), dtype=dtype, device=dev)        # every row must be written, none added to
        ops._run("hsp_gather_max_bwd_csr" + ops._sfx(g), (ops._p(g), 0, ops._p(arg), ops._p(off), ops._p(edge), B, Nsrc, Nq, k, C,
                                                          ops._p(gfeat), ops._stream()))
        want = pref.pool_bwd(g.float().cpu().numpy(), c["idx"], c["argmax"], c["qsel"], Nsrc)
        if dtype is BF16:
            got = gfeat.view(torch.int16).cpu().numpy().view(np.uint16)
            assert np.array_equal(got, pref.bf16_bits(want)), f"{name} bf16: {(got != pref.bf16_bits(want)).sum()} cells differ"
        else:
            got = gfeat.view(torch.int32).cpu().numpy()
            assert np.array_equal(got, want.view(np.int32)), f"{name} fp32: {(got != want.view(np.int32)).sum()} cells differ"
        if name == "empty_rows":
            bits = gfeat[:, 1::2].contiguous().view(torch.int16 if dtype is BF16 else torch.int32)
            assert int(bits.count_nonzero()) == 0, "rows no query won must be +0"
            assert bool((gfeat[:, 0::2] != 0).any())


def test_broadcast_row(dev, ref):
    """grad_bcast = 1 in both storage types: the per-cloud fp32 row times the number of winning queries, one rounding"""
    from hs_pose_amd import ops
    c = _case(ref, "plain2")
    idx, qsel, off, edge = _rev(dev, c)
    B, Nq, C = c["g"].shape
    Nsrc, k = c["Nsrc"], c["k"]
    arg = torch.from_numpy(c["argmax"]).to(dev)
    row = c["g"][:, 0].contiguous()
    ones = pref.pool_bwd(np.ones((B, Nq, C), np.float32), c["idx"], c["argmax"], None, Nsrc)          # the counts, exact
    want = (row.numpy()[:, None, :] * ones).astype(np.float32)
    for dtype in (torch.float32, BF16):
        gfeat = torch.full((B, Nsrc, C), float("nan"), dtype=dtype, device=dev)
        ops._run("hsp_gather_max_bwd_csr" + ops._sfx(gfeat), (ops._p(row.to(dev)), 1, ops._p(arg), ops._p(off), ops._p(edge), B, Nsrc, Nq, k,
                                                              C, ops._p(gfeat), ops._stream()))
        if dtype is BF16:
            assert np.array_equal(gfeat.view(torch.int16).cpu().numpy().view(np.uint16), pref.bf16_bits(want))
        else:
            assert np.array_equal(gfeat.view(torch.int32).cpu().numpy(), want.view(np.int32))


def _forward_argmax(feat, idx, qsel, k):
    """the arg-max bytes the autograd forward keeps to itself: the same entry point on the same operands"""
    from hs_pose_amd import ops
    B, Nsrc, C = feat.shape
    Nidx, kstride = idx.shape[1], idx.shape[2]
    Nq = Nidx if qsel is None else qsel.shape[-1]
    out = torch.empty(B, Nq, C, dtype=feat.dtype, device=feat.device)
    arg = torch.empty(B, Nq, C, dtype=torch.uint8, device=feat.device)
    qp, qs = _qargs(qsel)
    ops._run("hsp_gather_max_fwd_sel" + ops._sfx(feat), (ops._p(feat), ops._p(idx), qp, qs, B, Nsrc, Nidx, Nq, k, kstride, C, ops._p(out),
                                                         ops._p(arg), ops._stream()))
    return arg.cpu().numpy()


def _bwd_launches(timer):
    """every C-ABI call the timed backward issued, in order"""
    return [r[0] for r in timer.records]


@pytest.mark.parametrize("name", ["plain2", "shared", "repeated"])
def test_autograd_under_the_switch(dev, ref, flags, name):
    """ops.gather_max (fp32 and bf16 rows) and ops.pool_layer (fp32) backward with FLAGS.reproducible on equal the restatement;
    with it off the launches are today's and the result agrees to rounding"""
    from hs_pose_amd import ops
    c = _case(ref, name)
    B, Nq, C = c["g"].shape
    Nsrc, k = c["Nsrc"], c["k"]
    idx = torch.from_numpy(c["idx"]).to(dev)
    qsel = None if c["qsel"] is None else torch.from_numpy(c["qsel"]).to(dev)
    xyz = ref.hash_tensor((B, Nsrc, 3), 5, 0.05).to(dev)
    per_cloud = qsel is not None and qsel.dim() == 2
    for dtype in (torch.float32, BF16):
        feat0 = ref.hash_tensor((B, Nsrc, C), 77, 1.0).to(dev).to(dtype)
        g = c["g"].to(dev).to(dtype)
        arg = _forward_argmax(feat0, idx, qsel, k)
        want = pref.pool_bwd(g.float().cpu().numpy(), c["idx"], arg, c["qsel"], Nsrc)
        # (a fresh idx tensor per call: the reverse map is memoised on it, once per step and Pool_layer)
        forms = [("gather_max", lambda f: ops.gather_max(f, idx.clone(), k, qsel=qsel))]
        if dtype is torch.float32 and qsel is not None and idx.shape[1] == Nsrc:
            forms.append(("pool_layer", lambda f: ops.pool_layer(f, xyz, idx.clone(), qsel, k)[0]))
        for what, fn in forms:
            grads = {}
            for on in (True, False):
                flags.reproducible = on
                feat = feat0.clone().requires_grad_(True)
                out = fn(feat)
                timer = ops.KernelTimer()
                prev = ops.set_timer(timer)
                try:
                    out.backward(g)
                finally:
                    ops.set_timer(prev)
                torch.cuda.synchronize()
                grads[on] = feat.grad
                sfx = "_bf16" if dtype is BF16 else ""
                if on:
                    assert _bwd_launches(timer) == ["hsp_rev_build" + ("_sel" if qsel is not None else ""), "hsp_gather_max_bwd_csr" + sfx], \
                        (what, _bwd_launches(timer))
                else:                                         # exactly today's launch
                    assert _bwd_launches(timer) == ["hsp_gather_max_bwd" + ("_sel" if per_cloud else "") + sfx], (what, _bwd_launches(timer))
            if dtype is BF16:
                assert np.array_equal(grads[True].view(torch.int16).cpu().numpy().view(np.uint16), pref.bf16_bits(want)), what
            else:
                assert np.array_equal(grads[True].view(torch.int32).cpu().numpy(), want.view(np.int32)), what
            # the default form sums the same <= Nq terms in another order: every partial sum is at most Nq * max|g|, every add
            # rounds by at most 2^-24 of it, two orders -> 2 Nq^2 2^-24 max|g|; a bf16 store adds 2^-9 of the result, twice
            scale = float(np.abs(c["g"].numpy()).max())
            tol = (2 * Nq * Nq * 2.0 ** -24 + (2 * Nq * 2.0 ** -9 if dtype is BF16 else 0.0)) * scale
            assert float((grads[True].float() - grads[False].float()).abs().max()) <= tol, what


@pytest.mark.parametrize("C", [16, 12])
def test_gather_rows_under_the_switch(dev, ref, flags, C):
    """ops.gather_rows backward: the gather form over rev_index(idx, 1, Nsrc) under the switch wherever that entry takes the
    operands (a per-cloud map, C / 2 columns dividing the workgroup: C = 16) -- the ordered sum of each source row's queries, bit
    for bit; where it would decline (C = 12) and without the switch, today's launch and nothing else"""
    from hs_pose_amd import ops
    B, Nsrc, Nq = 2, 19, 64
    rng = np.random.RandomState(3)
    idx_np = rng.randint(0, Nsrc, size=(B, Nq)).astype(np.int32)
    g = _grad(ref, (B, Nq, C), 9)
    # a row map is a pool of k = 1 whose arg-max bytes are all 0
    want = pref.pool_bwd(g.numpy(), idx_np[:, :, None], np.zeros((B, Nq, C), np.uint8), None, Nsrc)
    names = {}
    for on in (True, False):
        flags.reproducible = on
        feat = ref.hash_tensor((B, Nsrc, C), 4, 1.0).to(dev).requires_grad_(True)
        out = ops.gather_rows(feat, torch.from_numpy(idx_np).to(dev))
        timer = ops.KernelTimer()
        prev = ops.set_timer(timer)
        try:
            out.backward(g.to(dev))
        finally:
            ops.set_timer(prev)
        torch.cuda.synchronize()
        names[on] = [r[0] for r in timer.records]
        if on and C == 16:
            assert np.array_equal(feat.grad.view(torch.int32).cpu().numpy(), want.view(np.int32))
        else:
            # (another order of the same <= Nq terms: 2 Nq^2 2^-24 max|g|, as in test_autograd_under_the_switch)
            assert float((feat.grad.cpu() - torch.from_numpy(want)).abs().max()) <= 2 * Nq * Nq * 2.0 ** -24 * float(g.abs().max())
    assert names[False] == ["hsp_gather_rows_bwd"], names
    assert names[True] == (["hsp_rev_build", "hsp_gather_rows_bwd_csr"] if C == 16 else ["hsp_gather_rows_bwd"]), names


def test_bad_arguments(dev):
    """the codes of include/hsp.h with real device pointers around the bad one: nothing is launched"""
    from hs_pose_amd import _lib, ops
    L, K = _lib.lib(), _lib.CONSTANTS
    bad, uns = K["ERR_BAD_ARG"], K["ERR_UNSUPPORTED"]
    t = torch.zeros(4096, dtype=torch.int32, device=dev)
    p, null, st = ops._p(t), ops._vp(0), ops._stream()
    assert L.hsp_rev_build_sel(null, p, 0, 1, 8, 4, 8, 4, 4, p, p, st) == bad
    assert L.hsp_rev_build_sel(p, p, 0, 1, 8, 4, 8, 4, 4, null, p, st) == bad
    assert L.hsp_rev_build_sel(p, p, 0, 1, 8, 4, 8, 4, 4, p, null, st) == bad
    assert L.hsp_rev_build_sel(p, p, 0, 1, 0, 4, 8, 4, 4, p, p, st) == bad
    assert L.hsp_rev_build_sel(p, p, 0, 1, 8, 4, 0, 4, 4, p, p, st) == bad
    assert L.hsp_rev_build_sel(p, p, 3, 1, 8, 4, 8, 4, 4, p, p, st) == bad                    # 0 < stride < Nq
    assert L.hsp_rev_build_sel(p, null, 0, 1, 8, 4, 8, 4, 4, p, p, st) == bad                 # no list: Nq must be Nidx
    for fn in (L.hsp_gather_max_bwd_csr, L.hsp_gather_max_bwd_csr_bf16):
        assert fn(p, 0, p, p, p, 1, 8, 8, 4, 6, p, st) == uns                                 # C % 4
        assert fn(null, 0, p, p, p, 1, 8, 8, 4, 8, p, st) == bad
        assert fn(p, 0, null, p, p, 1, 8, 8, 4, 8, p, st) == bad
        assert fn(p, 0, p, null, p, 1, 8, 8, 4, 8, p, st) == bad
        assert fn(p, 0, p, p, null, 1, 8, 8, 4, 8, p, st) == bad
        assert fn(p, 0, p, p, p, 1, 8, 8, 4, 8, null, st) == bad
        assert fn(p, 0, p, p, p, 0, 8, 8, 4, 8, p, st) == bad
        assert fn(p, 0, p, p, p, 1, 8, 0, 4, 8, p, st) == bad
    torch.cuda.synchronize()
    assert int(t.count_nonzero()) == 0
