"""CPU: hsp_orl_counts_offset, the host-side query that says whether a call of hsp_orl_global_fwd will leave winner counts in its
workspace and where (include/hsp.h); it declines whatever does not take the LDS slab kernel."""
HUGE = 1 << 40


def test_query_declines():
    from hs_pose_amd._lib import lib
    L = lib()
    q = L.hsp_orl_counts_offset
    base = L.hsp_orl_workspace_bytes(3, 100, 128)
    off = (base + 255) & ~255
    assert q(3, 100, 20, 20, 128, off + 2 * 3 * 100 * 128) == off
    assert q(3, 100, 20, 20, 128, off + 2 * 3 * 100 * 128 - 1) == -1       # one byte short
    assert q(3, 100, 20, 20, 128, base) == -1                              # today's callers
    assert q(2, 128, 8, 8, 64, HUGE) == -1                                 # k != 20: the chunked form
    assert q(3, 100, 20, 24, 128, HUGE) == -1                              # lists of a wider tensor
    assert q(1, 3000, 20, 20, 8, HUGE) == -1                               # slab past the LDS limit
    assert q(1, 2850, 20, 20, 8, HUGE) >= 0
    assert q(2, 100, 20, 20, 24, HUGE) == -1                               # 256 % (C / 4): a width the forward itself declines
    assert q(2, 100, 20, 20, 132, HUGE) == -1                              # C % 8


def test_stream_backward_validates_arguments():
    """hsp_gather_max_bwd(grad_bcast = 2) takes no lists; it declines what its 32-bit unit index cannot address and checks its
    pointers before any launch"""
    import ctypes
    from hs_pose_amd._lib import lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    for f in (L.hsp_gather_max_bwd, L.hsp_gather_max_bwd_bf16):
        assert f(one, 2, null, null, null, 2, 8, 8, 8, 20, 16, one, 1, null, null) == -1           # no counts
        assert f(one, 2, null, null, one, 2, 8, 8, 8, 20, 18, one, 1, null, null) == -2            # C % 4
        assert f(one, 2, null, null, ctypes.c_void_p(68), 2, 8, 8, 8, 20, 16, one, 1, null, null) == -2   # counts not 8-byte aligned
        assert f(one, 2, null, null, one, 65, 65535, 8, 8, 20, 2048, one, 1, null, null) == -2     # past 2^31 float4 units
        assert f(one, 1, null, null, one, 2, 8, 8, 8, 20, 16, one, 1, null, null) == -1            # mode 1 still needs idx
