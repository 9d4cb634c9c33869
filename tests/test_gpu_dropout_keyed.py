"""The keyed Dropout (csrc/losses.hip: hsp_dropout_keyed_fwd / hsp_dropout_bwd; ops.dropout_keyed) against the numpy restatement
of include/hsp.h's rule (tests/_dropout_ref.py), bit for bit, and the heads' use of it: training mode under FLAGS.reproducible
inside a device draw scope only, torch's Dropout everywhere else, the identity in eval mode."""
import numpy as np
import pytest
import torch

import _dropout_ref as dref

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15                                                        # (high bits set)
CALLS = (0, 2 ** 32 + 5)                                                         # call below and above 2^32


def _sampler(dev, call):
    from hs_pose_amd.pc_sample import DeviceSampler
    s = DeviceSampler(SEED, dev)
    s.set_state((SEED, call))
    return s


@pytest.mark.parametrize("p", [0.0, 0.2, 0.999])
@pytest.mark.parametrize("R,C", [(1, 4), (3, 256), (16, 256)])
def test_forward_and_backward_equal_restatement(dev, ref, R, C, p):
    from hs_pose_amd import ops
    x = ref.hash_tensor((R, C), 21, 2.0)
    g = ref.hash_tensor((R, C), 22, 1.0)
    for call in CALLS:
        for site in (0, 2, 2 ** 24 - 1):
            key = _sampler(dev, call).advance()
            xd = x.to(dev).requires_grad_(True)
            out = ops.dropout_keyed(xd, key, site, p)
            out.backward(g.to(dev))
            torch.cuda.synchronize()
            want, keep = dref.dropout(x.numpy(), SEED, call, site, p)
            assert np.array_equal(out.detach().view(torch.int32).cpu().numpy(), want.view(np.int32)), (call, site)
            if p == 0.0:
                assert keep.all() and torch.equal(out.detach().cpu(), x)
            want_g = (g.numpy() * keep.astype(np.float32) * dref.scale_of(p)).astype(np.float32)
            assert np.array_equal(xd.grad.cpu().numpy(), want_g), (call, site)


def test_grid_stride_wraps(dev, ref):
    """2049 x 256 = 524 544 elements, more than the 256 * HSP_NUM_CU * 8 = 524 288 threads of the capped grid: the second trip of
    either kernel's stride loop; forward, mask and backward bit for bit"""
    from hs_pose_amd import ops
    R, C, p, call, site = 2049, 256, 0.2, CALLS[0], 2
    assert R * C > 256 * 256 * 8 >= (R - 1) * C
    x = ref.hash_tensor((R, C), 24, 2.0)
    g = ref.hash_tensor((R, C), 25, 1.0)
    key = _sampler(dev, call).advance()
    xd, gd = x.to(dev), g.to(dev)
    out, keep, gx = torch.full_like(xd, float("nan")), torch.full((R, C), 9, dtype=torch.uint8, device=dev), torch.full_like(xd, float("nan"))
    ops._run("hsp_dropout_keyed_fwd", (ops._p(xd), ops._p(key), site, p, R, C, ops._p(out), ops._p(keep), ops._stream()))
    ops._run("hsp_dropout_bwd", (ops._p(gd), ops._p(keep), p, R, C, ops._p(gx), ops._stream()))
    torch.cuda.synchronize()
    want, want_keep = dref.dropout(x.numpy(), SEED, call, site, p)
    assert 0 < want_keep[-1].sum() < C                                            # (the rows of the second trip keep and drop)
    assert np.array_equal(keep.cpu().numpy(), want_keep)
    assert np.array_equal(out.view(torch.int32).cpu().numpy(), want.view(np.int32))
    want_g = (g.numpy() * want_keep.astype(np.float32) * dref.scale_of(p)).astype(np.float32)
    assert np.array_equal(gx.view(torch.int32).cpu().numpy(), want_g.view(np.int32))
    # and through the autograd node, as the cases above
    xa = xd.clone().requires_grad_(True)
    oa = ops.dropout_keyed(xa, key, site, p)
    oa.backward(gd)
    assert torch.equal(oa.detach().view(torch.int32), out.view(torch.int32)) and torch.equal(xa.grad.view(torch.int32), gx.view(torch.int32))


def test_keep_bytes_and_two_forwards_before_a_backward(dev, ref):
    """the mask the C entry writes equals the restatement's; a backward uses ITS forward's saved mask although another forward
    under another key ran in between"""
    from hs_pose_amd import ops
    R, C, p = 3, 256, 0.2
    x = ref.hash_tensor((R, C), 23, 1.0).to(dev)
    sampler = _sampler(dev, 7)
    key = sampler.advance()
    out, keep = torch.empty_like(x), torch.full((R, C), 9, dtype=torch.uint8, device=dev)
    ops._run("hsp_dropout_keyed_fwd", (ops._p(x), ops._p(key), 1, p, R, C, ops._p(out), ops._p(keep), ops._stream()))
    assert np.array_equal(keep.cpu().numpy(), dref.keep_mask(SEED, 7, 1, p, R, C).astype(np.uint8))
    xa = x.clone().requires_grad_(True)
    a = ops.dropout_keyed(xa, key, 1, p)
    torch.cuda.synchronize()
    key2 = sampler.advance()                                                      # (the same buffer, now call 8)
    xb = x.clone().requires_grad_(True)
    b = ops.dropout_keyed(xb, key2, 1, p)
    a.sum().backward()
    b.sum().backward()
    s = dref.scale_of(p)
    for grad, call in ((xa.grad, 7), (xb.grad, 8)):
        assert np.array_equal(grad.cpu().numpy(), dref.keep_mask(SEED, call, 1, p, R, C).astype(np.float32) * s)
    assert not torch.equal(xa.grad, xb.grad)


def test_head_uses_it_only_where_it_should(dev, ref, flags):
    """Rot_green's Dropout: eval mode = the head without Dropout; training under the switch in a device draw scope = the keyed mask
    of the head's site and no draw on torch's device generator; without a scope, or with the switch off, torch's Dropout"""
    from hs_pose_amd import ops, pc_sample
    from hs_pose_amd.PoseNet9D import PoseNet9D
    from hs_pose_amd.PoseR import Rot_red
    flags.train = 0
    torch.manual_seed(0)
    net = PoseNet9D()
    assert [h.drop_site for h in (net.rot_green, net.rot_red, net.ts)] == [dref.SITES[n] for n in ("Rot_green", "Rot_red", "Pose_Ts")]
    head = Rot_red().to(dev)
    head.drop_site = 1
    h = ref.hash_tensor((4, 256), 31, 1.0).to(dev)
    head.eval()
    flags.reproducible = True
    with pc_sample.draw_scope(_sampler(dev, 3), dev):
        assert torch.equal(head._drop(h), h)                                      # eval: the identity, as nn.Dropout
    x = ref.hash_tensor((2, 64, flags.feat_c_R), 33, 1.0).to(dev)                # the whole head in eval mode, (B,N,f) rows
    with torch.no_grad(), pc_sample.draw_scope(_sampler(dev, 3), dev):
        with_dropout = head.forward_rows(x)
        drop1, head.drop1 = head.drop1, torch.nn.Identity()
        without = head.forward_rows(x)
        head.drop1 = drop1
    assert with_dropout.shape == (2, 4) and torch.equal(with_dropout, without)
    head.train()
    sampler = _sampler(dev, 3)
    rng0 = torch.cuda.get_rng_state()
    with pc_sample.draw_scope(sampler, dev):                                      # (advances the sampler: the draws are call 3's)
        got = head._drop(h)
    torch.cuda.synchronize()
    assert torch.equal(rng0, torch.cuda.get_rng_state()), "the keyed Dropout drew on torch's device generator"
    want, _ = dref.dropout(h.cpu().numpy(), SEED, 3, 1, head.drop1.p)
    assert np.array_equal(got.view(torch.int32).cpu().numpy(), want.view(np.int32))
    # no device scope: torch's Dropout, under the switch or not
    for on in (True, False):
        flags.reproducible = on
        torch.manual_seed(5)
        a = head._drop(h)
        torch.manual_seed(5)
        assert torch.equal(a, torch.nn.functional.dropout(h, head.drop1.p, True))
    # a device scope with the switch off: torch's as well
    flags.reproducible = False
    with pc_sample.draw_scope(sampler, dev):
        torch.manual_seed(5)
        a = head._drop(h)
    torch.manual_seed(5)
    assert torch.equal(a, torch.nn.functional.dropout(h, head.drop1.p, True))
