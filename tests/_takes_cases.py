"""The case table of the host queries the non-GEMM entry points decline by (``hsp_*_takes``, include/hsp.h): rows (query,
arguments, expected answer) placed at each limit, the last shape taken and the first declined.  tests/test_takes_host.py asserts
the rows on the CPU (the queries are host code); tests/test_gpu_takes.py calls the entry point of every row on real buffers and
holds its return code to the query."""
from collections import namedtuple

T = namedtuple("T", "query args want")


def _t(query, *args, want):
    return T(query, args, want)


CASES = (
    # hsp_knn_xyz_takes(B, N, k, drop_first): the tie pass's row of N candidates in 160 KB of LDS (16 bytes each), lists of k + drop <= 32
    _t("hsp_knn_xyz_takes", 2, 10240, 20, 1, want=1),
    _t("hsp_knn_xyz_takes", 2, 10241, 20, 1, want=0),
    _t("hsp_knn_xyz_takes", 2, 64, 31, 1, want=1),
    _t("hsp_knn_xyz_takes", 2, 64, 32, 1, want=0),
    _t("hsp_knn_xyz_takes", 2, 64, 32, 0, want=1),
    # hsp_knn_exact_takes(B, N, C, k, drop_first): the same list bound; the replay's LDS row holds the query's C columns as well
    # (C = 128: N <= 10 208; the search at that size wants a 420 MB workspace); coordinates go to the xyz search
    _t("hsp_knn_exact_takes", 1, 10208, 128, 20, 1, want=1),
    _t("hsp_knn_exact_takes", 1, 10209, 128, 20, 1, want=0),
    _t("hsp_knn_exact_takes", 2, 64, 32, 31, 1, want=1),
    _t("hsp_knn_exact_takes", 2, 64, 32, 32, 1, want=0),
    _t("hsp_knn_exact_takes", 2, 33, 32, 32, 1, want=0),               # k + drop == N: still one rank past the list
    _t("hsp_knn_exact_takes", 2, 10240, 3, 20, 1, want=1),
    _t("hsp_knn_exact_takes", 2, 10241, 3, 20, 1, want=0),
    # hsp_geometry_levels_takes(N0, N1, N2, k1, kpool, k2, drop_first): 64 <= N2 <= N1 <= 576 <= N0, lists of k + drop <= 32
    _t("hsp_geometry_levels_takes", 2304, 576, 144, 20, 4, 18, 1, want=1),
    _t("hsp_geometry_levels_takes", 2308, 577, 144, 20, 4, 18, 1, want=0),
    _t("hsp_geometry_levels_takes", 1028, 257, 64, 20, 4, 8, 1, want=1),
    _t("hsp_geometry_levels_takes", 1028, 257, 63, 20, 4, 7, 1, want=0),
    _t("hsp_geometry_levels_takes", 1028, 257, 64, 31, 4, 8, 1, want=1),
    _t("hsp_geometry_levels_takes", 1028, 257, 64, 32, 4, 8, 1, want=0),
    _t("hsp_geometry_levels_takes", 1028, 257, 64, 20, 4, 63, 0, want=0),    # k2 + drop + 1 > 33
    _t("hsp_geometry_levels_takes", 256, 64, 64, 8, 4, 8, 1, want=1),
    _t("hsp_geometry_levels_takes", 256, 64, 65, 8, 4, 8, 1, want=0),        # level 2 larger than level 1
    _t("hsp_geometry_levels_takes", 200, 257, 64, 20, 4, 8, 1, want=0),      # level 1 larger than the cloud
    # hsp_geometry_all_takes(B, N0, k0, kpool0, N1, N2, k1, kpool, k2, drop_first): the levels' limits, 576 < N0 <= 1088, B N0 < 131 072
    # (131 071 is prime: no cloud count times a size in that range gives it; 170 x 771 = 131 070)
    _t("hsp_geometry_all_takes", 4, 576, 20, 4, 144, 64, 18, 4, 8, 1, want=0),
    _t("hsp_geometry_all_takes", 4, 577, 20, 4, 144, 64, 18, 4, 8, 1, want=1),
    _t("hsp_geometry_all_takes", 4, 1088, 20, 4, 272, 68, 20, 4, 8, 1, want=1),
    _t("hsp_geometry_all_takes", 4, 1089, 20, 4, 272, 68, 20, 4, 8, 1, want=0),
    _t("hsp_geometry_all_takes", 170, 771, 20, 4, 192, 64, 20, 4, 8, 1, want=1),
    _t("hsp_geometry_all_takes", 128, 1024, 20, 4, 256, 64, 20, 4, 8, 1, want=0),
    _t("hsp_geometry_all_takes", 4, 1028, 31, 4, 257, 64, 20, 4, 8, 1, want=1),
    _t("hsp_geometry_all_takes", 4, 1028, 32, 4, 257, 64, 20, 4, 8, 1, want=0),
    _t("hsp_geometry_all_takes", 4, 1028, 20, 4, 257, 63, 20, 4, 7, 1, want=0),     # (the levels decline)
    # hsp_rev_build_takes(n_src): n_src + 1 counters in 140 KB
    _t("hsp_rev_build_takes", 35839, want=1),
    _t("hsp_rev_build_takes", 35840, want=0),
    # hsp_gather_rows_bwd_csr_takes(elem_bytes, C, grad_stride, grad_align): even C and stride, a 2-element-aligned address,
    # C / 2 >= 256 or a divisor of 256
    _t("hsp_gather_rows_bwd_csr_takes", 4, 8, 8, 0, want=1),
    _t("hsp_gather_rows_bwd_csr_takes", 4, 6, 6, 0, want=0),            # three column pairs do not divide 256
    _t("hsp_gather_rows_bwd_csr_takes", 4, 7, 8, 0, want=0),
    _t("hsp_gather_rows_bwd_csr_takes", 4, 8, 9, 0, want=0),
    _t("hsp_gather_rows_bwd_csr_takes", 4, 8, 12, 8, want=1),
    _t("hsp_gather_rows_bwd_csr_takes", 4, 8, 12, 4, want=0),
    _t("hsp_gather_rows_bwd_csr_takes", 2, 8, 12, 4, want=1),
    _t("hsp_gather_rows_bwd_csr_takes", 2, 8, 12, 2, want=0),
    _t("hsp_gather_rows_bwd_csr_takes", 4, 512, 1286, 0, want=1),
    _t("hsp_gather_rows_bwd_csr_takes", 4, 516, 1286, 0, want=1),       # 258 pairs: whole rows of 256 lanes
    _t("hsp_gather_rows_bwd_csr_takes", 4, 510, 1286, 0, want=0),       # 255 pairs
    # hsp_colsum_rows_takes(C, elem_bytes) / hsp_colsum_rows_xyz_takes(C) / hsp_bn_takes(R, C): four-column lanes, C / 4 | 256;
    # fp32 column sums also one column per lane up to 256 columns
    _t("hsp_colsum_rows_takes", 1024, 4, want=1),
    _t("hsp_colsum_rows_takes", 1028, 4, want=0),
    _t("hsp_colsum_rows_takes", 6, 4, want=1),
    _t("hsp_colsum_rows_takes", 256, 4, want=1),
    _t("hsp_colsum_rows_takes", 250, 4, want=1),
    _t("hsp_colsum_rows_takes", 260, 4, want=0),
    _t("hsp_colsum_rows_takes", 1024, 2, want=1),
    _t("hsp_colsum_rows_takes", 1028, 2, want=0),
    _t("hsp_colsum_rows_takes", 6, 2, want=0),
    _t("hsp_colsum_rows_xyz_takes", 1024, want=1),
    _t("hsp_colsum_rows_xyz_takes", 1028, want=0),
    _t("hsp_colsum_rows_xyz_takes", 6, want=0),
    _t("hsp_colsum_rows_xyz_takes", 4, want=1),
    _t("hsp_bn_takes", 64, 1024, want=1),
    _t("hsp_bn_takes", 64, 1028, want=0),
    _t("hsp_bn_takes", 64, 6, want=0),
    _t("hsp_bn_takes", 64, 4, want=1),
    _t("hsp_bn_takes", 2, 128, want=1),
    # hsp_small_outer_takes(B) / hsp_small_pair_takes(B, C): a cloud's row per lane; the pair's nn product in 128-column MFMA blocks
    _t("hsp_small_outer_takes", 64, want=1),
    _t("hsp_small_outer_takes", 65, want=0),
    _t("hsp_small_pair_takes", 64, 2048, want=1),
    _t("hsp_small_pair_takes", 64, 2176, want=0),
    _t("hsp_small_pair_takes", 65, 2048, want=0),
    _t("hsp_small_pair_takes", 16, 128, want=1),
    _t("hsp_small_pair_takes", 16, 192, want=0),
    # hsp_exact_layer_takes(N, Cin, C): its four conditions -- C and Cin (but the surface layer's 3) multiples of 32, conv2 over at
    # most 512 channels, a 32-row tile inside one cloud
    _t("hsp_exact_layer_takes", 64, 128, 128, want=1),
    _t("hsp_exact_layer_takes", 64, 128, 144, want=0),
    _t("hsp_exact_layer_takes", 64, 3, 128, want=1),
    _t("hsp_exact_layer_takes", 64, 32, 128, want=1),
    _t("hsp_exact_layer_takes", 64, 48, 128, want=0),
    _t("hsp_exact_layer_takes", 64, 256, 256, want=1),
    _t("hsp_exact_layer_takes", 64, 256, 288, want=0),
    _t("hsp_exact_layer_takes", 32, 128, 128, want=1),
    _t("hsp_exact_layer_takes", 31, 128, 128, want=0),
    # hsp_fps_levels_takes(N0): the register-resident kernel
    _t("hsp_fps_levels_takes", 12288, want=1),
    _t("hsp_fps_levels_takes", 12289, want=0),
    # hsp_gemm_rows_bn_tiles_bf16(M, N, K): the row tiles of the product's BatchNorm partials (64 rows at K = 128, 128 rows at
    # K = 1024 on these widths), 0 past the 512 the fold takes
    _t("hsp_gemm_rows_bn_tiles_bf16", 32768, 128, 128, want=512),
    _t("hsp_gemm_rows_bn_tiles_bf16", 32769, 128, 128, want=0),
    _t("hsp_gemm_rows_bn_tiles_bf16", 65536, 128, 1024, want=512),
    _t("hsp_gemm_rows_bn_tiles_bf16", 65537, 128, 1024, want=0),
)

QUERIES = tuple(dict.fromkeys(c.query for c in CASES))


def case_id(c):
    return c.query[len("hsp_"):] + "-" + "-".join(str(a) for a in c.args)


# ---- the shapes FaceRecon and the heads reach: the sweep of tests/test_takes_host.py ------------------------------------------------
SWEEP_N = (64, 256, 1028, 4096)
SWEEP_B = (1, 16, 64)
WIDTHS = (3, 6, 64, 128, 256, 512, 1024, 1286, 1289)       # layer widths, the concatenated feature, the heads' inputs and outputs
HEAD_WIDTHS = (4, 6, 128, 256, 512, 1024)


def sweep(query):
    """argument tuples of ``query`` over every (B, N) of the sweep: the three resolutions of the stack at that N (N, N / 4,
    N / 16 points; k = min(20, N // 8) neighbours, Pool_layer's 4), every layer / head width"""
    out = []
    for B in SWEEP_B:
        for N0 in SWEEP_N:
            N1, N2 = N0 // 4, N0 // 16
            levels = [(n, min(20, n // 8) if n < N0 else 20) for n in (N0, N1, N2) if n >= 1]
            k1, k2 = min(20, N1 // 8), min(20, N2 // 8)
            if query == "hsp_knn_xyz_takes":
                out += [(B, n, k, d) for n, kn in levels for k in (kn, 4) for d in (0, 1)]
            elif query == "hsp_knn_exact_takes":
                out += [(B, n, C, k, 1) for n, k in levels for C in (3, 128, 256, 512)]
            elif query == "hsp_geometry_levels_takes":
                out += [(N0, N1, N2, k1, 4, k2, 1)]
            elif query == "hsp_geometry_all_takes":
                out += [(B, N0, 20, 4, N1, N2, k1, 4, k2, 1)]
            elif query == "hsp_rev_build_takes":
                out += [(n,) for n, _ in levels]
            elif query == "hsp_gather_rows_bwd_csr_takes":
                out += [(es, C, W, al) for es in (2, 4) for C in WIDTHS for W in (C, 1286, 1288, 1289) if W >= C for al in (0, 2, 4, 8, 12)]
            elif query == "hsp_colsum_rows_takes":
                out += [(C, es) for C in WIDTHS + HEAD_WIDTHS for es in (2, 4)]
            elif query == "hsp_colsum_rows_xyz_takes":
                out += [(C,) for C in WIDTHS + HEAD_WIDTHS]
            elif query == "hsp_bn_takes":
                out += [(R, C) for R in (B, B * N0, B * N1) for C in WIDTHS + HEAD_WIDTHS]
            elif query == "hsp_small_outer_takes":
                out += [(B,), (B * 4,)]
            elif query == "hsp_small_pair_takes":
                out += [(B, C) for C in WIDTHS + HEAD_WIDTHS]
            elif query == "hsp_exact_layer_takes":
                out += [(n, Cin, C) for n, _ in levels for Cin in (3, 64, 128, 256, 512) for C in (64, 128, 256, 512, 1024)]
            elif query == "hsp_fps_levels_takes":
                out += [(N0,)]
            elif query == "hsp_gemm_rows_bn_tiles_bf16":
                out += [(R, C, K) for R in (B, B * N0) for C in HEAD_WIDTHS for K in (128, 1024, 1286, 1289)]
            else:
                raise KeyError(query)
    return sorted(set(out))
