"""GPU, two devices: a kernel that needs more than 64 KiB of dynamic LDS launches on every device of one process.  The limit is a
per-device attribute of the kernel; wgrad_pair_kernel (67 584 B) used to raise it once per process, so its launch on a second
device was refused.  The same host inputs go to cuda:0, then to cuda:1: both calls return 0 and leave the same bits.

(The other launch sites that kept such a flag stay at or below 64 KiB: gemm_rows_plan_of picks 64 x 64 or 128 x 128 tiles only,
256 (BM + BN) <= 65 536 B; wgrad_bf16_mfma_kernel takes 65 536 B; the x3 panel kernel 48 KiB.)"""
import ctypes

import pytest
import torch

from hs_pose_amd._lib import HspWgradPending

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs in one process")]


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _smallest_pair(L):
    """one 64 x 64 tile per problem and the shortest K at which hsp_wgrad_pair_plan puts the pair into one launch"""
    out = (ctypes.c_int * 7)()
    for K in range(1, 1025):
        assert L.hsp_wgrad_pair_plan(64, 64, K, 64, 64, K, out) == 0
        if out[0]:
            return 64, 64, K
    raise AssertionError("no pair of 64 x 64 problems shares a launch")


def _pair_on(L, dev, a, b):
    """both weight gradients A^T B of the pair launch and its fold on `dev`; (rc of the launch, rc of the fold, C0, C1)"""
    (K, M), N = a[0].shape, b[0].shape[1]
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        keep, args = [], []
        for i in range(2):
            av, bv = a[i].to(dev), b[i].to(dev)
            out = torch.full((M, N), float("nan"), device=dev)
            ws = torch.zeros(L.hsp_wgrad_workspace_bytes(M, N, K), dtype=torch.uint8, device=dev)
            keep.append((av, bv, out, ws))
            args += [_vp(av), M, _vp(bv), N, M, N, K, _vp(out), N, _vp(ws), ws.numel()]
        pend = (HspWgradPending * 2)()
        rc = L.hsp_wgrad_partial_pair_f32(*args, pend, st)
        rc_fold = L.hsp_wgrad_fold(pend, 2, st) if rc == 0 else None
        torch.cuda.synchronize(dev)
        return rc, rc_fold, keep[0][2].cpu(), keep[1][2].cpu()


def test_wgrad_pair_on_two_devices():
    L = _L()
    M, N, K = _smallest_pair(L)
    g = torch.Generator().manual_seed(11)
    a = [torch.randn(K, M, generator=g) for _ in range(2)]
    b = [torch.randn(K, N, generator=g) for _ in range(2)]
    got = [_pair_on(L, torch.device("cuda", d), a, b) for d in (0, 1)]
    for d, (rc, rc_fold, _, _) in enumerate(got):
        assert (rc, rc_fold) == (0, 0), f"cuda:{d}: launch {rc}, fold {rc_fold}"
    for i in (2, 3):
        assert torch.isfinite(got[0][i]).all()
        assert torch.equal(got[0][i], got[1][i]), f"problem {i - 2}: cuda:0 and cuda:1 differ"
    # (the kernel is held to its reference in test_gpu_gemm_reference.py; here only that the product is the one asked for)
    want = a[0].double().t() @ b[0].double()
    assert (got[0][2].double() - want).abs().max() <= 1e-4 * want.abs().max()
