"""CPU: the merged-launch entry points of the backward pass (hsp_rev_build_multi, hsp_gather_rows_bwd_csr_multi[_bf16],
hsp_wgrad_partial_pair_colsum_f32) reject bad arguments and decline unsupported shapes before any launch."""
import ctypes


def _arr(t, vs):
    return ctypes.cast((t * len(vs))(*vs), ctypes.c_void_p)


def test_merged_entry_points_validate_arguments_without_gpu():
    from hs_pose_amd._lib import HspWgradPending, lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
    p2 = _arr(ctypes.c_void_p, [256, 256])
    i2 = lambda a, b: _arr(ctypes.c_int, [a, b])
    # reverse maps: count, table pointers, kstride < k
    assert L.hsp_rev_build_multi(0, p2, 1, i2(8, 8), i2(4, 4), i2(1, 1), i2(1, 1), p2, p2, null) == -1
    assert L.hsp_rev_build_multi(5, p2, 1, i2(8, 8), i2(4, 4), i2(1, 1), i2(1, 1), p2, p2, null) == -1
    assert L.hsp_rev_build_multi(2, null, 1, i2(8, 8), i2(4, 4), i2(1, 1), i2(1, 1), p2, p2, null) == -1
    assert L.hsp_rev_build_multi(2, p2, 1, i2(8, 8), i2(4, 4), i2(2, 1), i2(1, 1), p2, p2, null) == -1
    assert L.hsp_rev_build_multi(2, _arr(ctypes.c_void_p, [256, 0]), 1, i2(8, 8), i2(4, 4), i2(1, 1), i2(1, 1), p2, p2, null) == -1
    assert L.hsp_rev_build_multi(2, p2, 1, i2(8, 8), i2(4, 40000), i2(1, 1), i2(1, 1), p2, p2, null) == -2     # histogram > LDS
    # gathers: count, a null segment, stride < width, an odd width (what the single launch declines)
    for name in ("hsp_gather_rows_bwd_csr_multi", "hsp_gather_rows_bwd_csr_multi_bf16"):
        f = getattr(L, name)
        assert f(0, p2, 64, p2, p2, 1, i2(4, 4), 8, i2(8, 8), p2, null) == -1
        assert f(5, p2, 64, p2, p2, 1, i2(4, 4), 8, i2(8, 8), p2, null) == -1
        assert f(2, _arr(ctypes.c_void_p, [256, 0]), 64, p2, p2, 1, i2(4, 4), 8, i2(8, 8), p2, null) == -1
        assert f(2, p2, 4, p2, p2, 1, i2(4, 4), 8, i2(8, 8), p2, null) == -1
        assert f(2, p2, 64, p2, p2, 1, i2(4, 4), 8, i2(8, 7), p2, null) == -2
        assert f(2, p2, 63, p2, p2, 1, i2(4, 4), 8, i2(8, 8), p2, null) == -2                                # odd pitch
    # the column-sum rider: no tensor, no pending table, a width / pair the one-launch forms do not take
    pend = (HspWgradPending * 2)()
    pair = [one, 128, one, 128, 128, 128, 4096, one, 128, one, 1 << 30] * 2
    assert L.hsp_wgrad_partial_pair_colsum_f32(*pair, pend, null, 4, 1024, 128, one, null) == -1
    assert L.hsp_wgrad_partial_pair_colsum_f32(*pair, null, one, 4, 1024, 128, one, null) == -1
    assert L.hsp_wgrad_partial_pair_colsum_f32(*pair, pend, one, 4, 1024, 48, one, null) == -2               # hsp_colsum_cloud_ok == 0
    odd = [one, 128, one, 128, 100, 128, 4096, one, 128, one, 1 << 30] * 2                                   # M % 64
    assert L.hsp_wgrad_partial_pair_colsum_f32(*odd, pend, one, 4, 1024, 128, one, null) == -2
    short = [one, 128, one, 128, 128, 128, 64, one, 128, one, 1 << 30] * 2                                   # K too short to slice
    assert L.hsp_wgrad_partial_pair_colsum_f32(*short, pend, one, 4, 16, 128, one, null) == -2
