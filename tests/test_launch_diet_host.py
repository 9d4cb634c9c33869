"""CPU: the entry points of the two-launch per-cloud backward chain (hsp_colsum_cloud_f32, hsp_small_pair_f32) reject bad
arguments and decline unsupported shapes before any launch."""
import ctypes


def test_launch_diet_entry_points_validate_arguments_without_gpu():
    from hs_pose_amd._lib import lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    f = ctypes.c_float
    # hsp_colsum_cloud_ok(B, N, C, with_xyz): the three levels of the stack, then widths / sizes the form does not take
    for B, N, C in ((16, 1028, 128), (16, 257, 256), (16, 64, 512), (1, 100, 32), (2, 40, 1024)):
        assert L.hsp_colsum_cloud_ok(B, N, C, 0) == 1 and L.hsp_colsum_cloud_ok(B, N, C, 1) == 1
    assert L.hsp_colsum_cloud_ok(16, 1028, 100, 0) == 0           # C % 32
    assert L.hsp_colsum_cloud_ok(16, 1028, 96, 0) == 0            # C / 4 does not divide 256
    assert L.hsp_colsum_cloud_ok(16, 1028, 16, 0) == 0            # narrower than one column tile of four
    assert L.hsp_colsum_cloud_ok(0, 1028, 128, 0) == 0 and L.hsp_colsum_cloud_ok(16, 0, 128, 0) == 0
    assert L.hsp_colsum_cloud_ok(70000, 64, 128, 0) == 0          # clouds ride in grid.y
    assert L.hsp_colsum_cloud_ok(2, 60000, 1024, 1) == 0          # 469 chunk sums x 4 slots x 128 columns: beyond the LDS
    assert L.hsp_colsum_cloud_ok(3, 1000, 1024, 0) == 1 and L.hsp_colsum_cloud_ok(3, 1000, 1024, 1) == 0     # (32 x 4 x 128 too)
    # hsp_colsum_cloud_f32(x, xyz, B, N, C, out, stream)
    assert L.hsp_colsum_cloud_f32(null, null, 16, 1028, 128, one, null) == -1
    assert L.hsp_colsum_cloud_f32(one, null, 16, 1028, 128, null, null) == -1
    assert L.hsp_colsum_cloud_f32(one, null, 16, 0, 128, one, null) == -1
    assert L.hsp_colsum_cloud_f32(one, null, 16, 1028, 100, one, null) == -2
    assert L.hsp_colsum_cloud_f32(one, one, 2, 60000, 1024, one, null) == -2
    # hsp_small_pair_f32(gt, ldgt, B, Ma, W, ldw, Nn, alpha, out_nn, ldnn, c, ldc, Nb, out_o, ldo, mom, ldm, Cm, gste, stream)
    p = lambda *a: L.hsp_small_pair_f32(*a)
    ok = [one, 128, 16, 128, one, 256, 128, f(1.0), one, 128, one, 128, 128, one, 256, null, 0, 0, null, null]

    def with_(**kw):
        names = ["gt", "ldgt", "B", "Ma", "W", "ldw", "Nn", "alpha", "out_nn", "ldnn", "c", "ldc", "Nb", "out_o", "ldo", "mom", "ldm",
                 "Cm", "gste", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a
    for name in ("gt", "W", "out_nn", "c", "out_o"):
        assert p(*with_(**{name: null})) == -1, name
    assert p(*with_(ldgt=64)) == -1 and p(*with_(ldw=64)) == -1 and p(*with_(ldnn=64)) == -1       # pitches below the widths
    assert p(*with_(ldc=64)) == -1 and p(*with_(ldo=64)) == -1
    assert p(*with_(B=0)) == -1 and p(*with_(Nn=0)) == -1 and p(*with_(Nb=0)) == -1
    assert p(*with_(mom=one, ldm=384, Cm=128)) == -1                                               # rider without its output
    assert p(*with_(mom=one, ldm=100, Cm=128, gste=one)) == -1                                     # ldm < 3 Cm
    assert p(*with_(Ma=100, ldgt=128)) == -2                                                       # Ma % 128
    assert p(*with_(Ma=4096, ldgt=4096)) == -2 and p(*with_(B=65)) == -2
