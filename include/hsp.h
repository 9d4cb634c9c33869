/*
 * hsp.h -- C-ABI of libhsp.so: the MI355X (gfx950) hybrid-scope point-cloud feature-extractor kernels.
 *
 * This is the drop-in boundary for the HS-Pose hot path.  The reference has no
 * C/FFI boundary for its live path -- the boundary there is the Python module API of
 * network/fs_net_repo/gcn3d.py -- so every entry point below cites the reference Python function
 * whose device work it replaces.  The only FFI the reference does have is the pybind module of its
 * (dead) Chamfer extension, tools/pyTorchChamferDistance/chamfer_distance.cpp:180-185; hsp_chamfer_*
 * keep that module's argument roles.
 *
 * Conventions
 *   - every pointer is DEVICE memory, row-major contiguous, fp32 / int32 / uint8 as typed;
 *   - the caller owns every buffer; kernels allocate nothing.  Ops that need scratch take a
 *     caller-supplied workspace (`ws`, `ws_bytes`) sized by the matching *_workspace_bytes() query;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is stream-ordered
 *     and re-entrant, safe to capture into a hipGraph;
 *   - return value: 0 = HSP_OK, negative = error code (see hsp_error_string); nothing throws;
 *   - index tensors are int32 (the Python mirror widens to int64 at its edge because the reference
 *     API returns int64, gcn3d.py:22-23);
 *   - "cloud" = one (N,3) point set of the batch; B clouds are independent in every op.
 */
#ifndef HSP_H_
#define HSP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSP_OK 0
#define HSP_ERR_BAD_ARG (-1)      /* null pointer, non-positive size, k out of range ...       */
#define HSP_ERR_UNSUPPORTED (-2)  /* shape outside what the kernels were built for             */
#define HSP_ERR_WORKSPACE (-3)    /* ws == NULL or ws_bytes too small                          */
#define HSP_ERR_LAUNCH (-4)       /* hipLaunch / hipMemsetAsync reported an error              */

#define HSP_MAX_K 32              /* largest neighbour count (k + drop_first <= 33)            */

typedef void *hspStream_t;
typedef uint16_t hsp_bf16_t;      /* bfloat16 bits (the upper half of an fp32), for the *_bf16 entry points */

int hsp_version(void);
const char *hsp_error_string(int code);
/* last HIP error text recorded by a failing launch on this thread ("" if none) */
const char *hsp_last_hip_error(void);

/* ---- neighbour search ------------------------------------------------------------------------
 * replaces get_neighbor_index(vertices, k)            network/fs_net_repo/gcn3d.py:15-24
 * x (B,N,C) -> idx (B,N,k): the k rows nearest to each row under the reference's expanded fp32
 * distance ((inner*-2)+quad[j])+quad[i], inner = k-ordered fma chain (== torch.bmm on CPU), quad in
 * ATen's row-sum order; ascending distance, lowest index first on exact ties; with drop_first=1 the
 * rank-0 entry of the (k+1) nearest is dropped (the reference's [:, :, 1:]), which is NOT "exclude
 * self".  C==3 runs the LDS-resident xyz kernel, any other C the f32-MFMA distance-tile kernel.
 */
size_t hsp_knn_workspace_bytes(int B, int N, int C, int k);
int hsp_knn_f32(const float *x, int B, int N, int C, int k, int drop_first, int32_t *idx,
                void *ws, size_t ws_bytes, hspStream_t stream);
/* get_neighbor_index with torch.topk's OWN order among exactly equal distances (ATen's CPU topk = libstdc++'s
 * nth_element + sort, or partial_sort for (k + drop_first) * 64 <= N, under a comparator that only sees the value: restated in
 * csrc/knn_exact.hip and oracle/hsp_oracle.c, pinned against torch.topk on tie-rich rows).  hsp_knn_f32 breaks ties by the lowest
 * index; on tie-free rows the two agree.  Used by the eval-mode forward (exact scope).  k + drop_first + 1 <= 33.
 * quad_mode (C != 3): how torch.sum(x ** 2, dim=2) of gcn3d.py:20 rounds -- 0: x is a contiguous (B,N,C) tensor (ATen's
 * vectorised row sum), 1: x is the transposed VIEW of a (B,C,N) tensor, which is what FaceRecon.py:94-95 hands conv_3 (ATen then
 * sums the channels as an outer reduction: cascade for the first 32 floor(N/32) points, four interleaved cascades for the rest).
 * The search flags the rows that hold two equal distances among their k + drop_first + 1 nearest and a fixed-grid pass replays only
 * those (round 5; while B N N floats stay below 512 MB the search also leaves the distance matrix in ws, so a replayed row reads its
 * distances instead of recomputing ~0.5 MB of feature rows).
 * ws: hsp_knn_exact_workspace_bytes; tie_rows (may be NULL): a device int that is incremented once per row that held a tie.
 * hsp_knn_exact_takes: 1 where hsp_knn_exact_f32 runs the search -- the function that entry point itself declines by, before its
 * first launch: the list length above and the replay's LDS row (N candidates and, for C != 3, the query's C columns; C == 3:
 * hsp_knn_xyz_takes) -- else 0; the caller then takes hsp_knn_f32. */
size_t hsp_knn_exact_workspace_bytes(int B, int N, int C, int k, int drop_first);
int hsp_knn_exact_takes(int B, int N, int C, int k, int drop_first);
int hsp_knn_exact_f32(const float *x, int B, int N, int C, int k, int drop_first, int quad_mode, int32_t *idx, void *ws,
                      size_t ws_bytes, int *tie_rows, hspStream_t stream);
/* get_neighbor_index on COORDINATES (C == 3), torch.topk's order among equal distances included, for up to two list lengths of
 * the same search: idx (B,N,k) and, when k2 > 0, idx2 (B,N,k2), k2 <= k -- the layers' k-list and Pool_layer's 4-list of one
 * resolution (gcn3d.py:236; on a tiled cloud, datasets/load_data.py:314-316, the short list is NOT the prefix of the long one:
 * ATen takes std::partial_sort for (k2 + drop) * 64 <= N and nth_element + sort otherwise).  The search itself is hsp_knn_f32's
 * xyz kernel run one rank past the answer; it flags the rows that hold two equal distances among those k + drop + 1 nearest, and
 * a fixed-grid pass replays only the flagged rows through libstdc++'s routines (csrc/knn_exact.hip).  A tie-free batch pays one
 * small launch.  This is what every xyz search of the package goes through, training included.
 * N <= 10 240 (the replay keeps one row of candidates in LDS; beyond it HSP_ERR_UNSUPPORTED is returned before any launch and the
 * caller falls back on hsp_knn_f32's (distance, index) order).
 * ws: hsp_knn_xyz_workspace_bytes (the row flags); tie_rows (may be NULL): device int, += number of flagged rows -- counted by
 * the SEPARATE replay pass only: for N <= 576 with B N < 131 072 the selection kernel replays its flagged rows inline and leaves
 * tie_rows untouched.
 * hsp_knn_xyz_takes: 1 where hsp_knn_xyz_f32 runs the search (k + drop_first + 1 <= 33, N <= 10 240) -- the function that entry
 * point itself declines by -- else 0. */
size_t hsp_knn_xyz_workspace_bytes(int B, int N);
int hsp_knn_xyz_takes(int B, int N, int k, int drop_first);
int hsp_knn_xyz_f32(const float *xyz, int B, int N, int k, int k2, int drop_first, int32_t *idx, int32_t *idx2, void *ws,
                    size_t ws_bytes, int *tie_rows, hspStream_t stream);
/* The coordinate work of the stack's two coarse levels in ONE launch (FaceRecon.py:91-101, gcn3d.py:236,243-245).  Pool_layer keeps
 * rows sel1 (N1 of them, int32, device) of the input cloud and then rows sel2 (N2) of that level; the draws are host-side and known
 * before the forward, and everything later asked of the two clouds depends on coordinates only:
 *   v1 (B,N1,3), v2 (B,N2,3)                      the levels' vertices
 *   idx1 (B,N1,k1), idx1_pool (B,N1,kpool)        get_neighbor_index(v1, k1) and Pool_layer's own list (kpool = 0: none, pass NULL)
 *   idx2 (B,N2,k2)                                get_neighbor_index(v2, k2)
 *   up1, up2 (B,N0)                               get_nearest_index(vertices, v1 / v2)
 * Four independent small searches that cost a launch each (6-13 us, mostly latency); here they are block ranges of one grid.  Same
 * results as hsp_knn_xyz_f32 / hsp_nn1_f32 (torch.topk's order among equal distances included).  64 <= N2 <= N1 <= 576, else
 * HSP_ERR_UNSUPPORTED (the caller keeps the separate calls).  hsp_geometry_levels_takes: 1 where the entry point runs the shapes
 * (the levels' sizes, k + drop_first + 1 <= 33 per list, the kernel's LDS) -- the function that entry point itself declines by. */
int hsp_geometry_levels_takes(int N0, int N1, int N2, int k1, int kpool, int k2, int drop_first);
int hsp_geometry_levels_f32(const float *xyz, int B, int N0, const int32_t *sel1, int N1, const int32_t *sel2, int N2, int k1,
                            int kpool, int k2, int drop_first, float *v1, float *v2, int32_t *idx1, int32_t *idx1_pool,
                            int32_t *idx2, int32_t *up1, int32_t *up2, hspStream_t stream);
/* hsp_knn_xyz_f32 on the input cloud (idx0 (B,N0,k0), idx0_pool (B,N0,kpool0)) AND hsp_geometry_levels_f32 in two launches instead of
 * three: the level-0 search's tie pass depends on that search's flags only, so it rides in the levels' launch as a further block
 * range (a flagged row is ~14 us of latency during which the chip would otherwise idle).  576 < N0 <= 1088 and the levels' limits,
 * else HSP_ERR_UNSUPPORTED (the caller keeps the separate calls).  ws: hsp_geometry_all_workspace_bytes (the level-0 flags).
 * hsp_geometry_all_takes: 1 where the entry point runs the shapes (hsp_geometry_levels_takes, the range of N0, B N0 < 131 072, the
 * LDS with the tie pass's rows) -- the function that entry point itself declines by, before its first launch. */
int hsp_geometry_all_takes(int B, int N0, int k0, int kpool0, int N1, int N2, int k1, int kpool, int k2, int drop_first);
size_t hsp_geometry_all_workspace_bytes(int B, int N0);
int hsp_geometry_all_f32(const float *xyz, int B, int N0, int k0, int kpool0, const int32_t *sel1, int N1, const int32_t *sel2, int N2,
                         int k1, int kpool, int k2, int drop_first, int32_t *idx0, int32_t *idx0_pool, float *v1, float *v2,
                         int32_t *idx1, int32_t *idx1_pool, int32_t *idx2, int32_t *up1, int32_t *up2, void *ws, size_t ws_bytes,
                         hspStream_t stream);
/* hsp_knn_f32 with the |x|^2 order chosen as above */
int hsp_knn_quadmode_f32(const float *x, int B, int N, int C, int k, int drop_first, int32_t *idx, void *ws, size_t ws_bytes,
                         int quad_mode, hspStream_t stream);
/* |x|^2 per row in the transposed-view order (quad_mode 1) */
int hsp_quad_outer_f32(const float *x, int B, int N, int C, float *quad, hspStream_t stream);
/* PoseNet9D.py:25: centred = pts - mean over the N points, mean (B,3) in ATen's summation order for a contiguous (B,N,3) tensor
 * (an outer sum over 3 columns: four interleaved 16-element cascades per column) divided by N */
int hsp_center_cloud_f32(const float *pts, int B, int N, float *centred, float *mean, hspStream_t stream);

/* replaces get_nearest_index(target, source)          network/fs_net_repo/gcn3d.py:27-36
 * tgt (B,Nt,3), src (B,Ns,3) -> idx (B,Nt): top-1 source row, d = (s2[j]+t2[i]) - 2*inner. */
int hsp_nn1_f32(const float *tgt, int Nt, const float *src, int Ns, int B, int32_t *idx,
                hspStream_t stream);

/* ---- receptive-field graph convolution -------------------------------------------------------
 * replaces HSlayer_surface.graph_conv                 gcn3d.py:92-107   (+ directions of :49-59)
 * xyz (B,N,3), idx (B,N,k), dirs (3, S*K) = the RAW support-direction parameter; the kernels apply
 * F.normalize(dim=0) (gcn3d.py:100,166: D / max(||D||_col, 1e-12)) themselves, and the backward entry
 * points return the gradient w.r.t. the RAW parameter (normalisation Jacobian included).
 * out (B,N,K) = mean_s max_n relu(R[b,i,n,:] . D^[:, s*K+c]);
 * argrow (B,N,S*K) uint16 = the SOURCE ROW idx[b,i,n*] of the winning neighbour (N <= 65535): all a
 * backward needs -- neither idx nor the slot n is read again.
 * R = normalize(xyz[idx]-xyz) is recomputed in-kernel, never materialised.
 */
int hsp_rf_surface_fwd(const float *xyz, const int32_t *idx, const float *dirs, int B, int N, int k,
                       int S, int K, float *out, uint16_t *argrow, hspStream_t stream);
/* grad_dirs (3,S*K) is OVERWRITTEN with d(loss)/d(raw directions).
 * ws: hsp_rf_bwd_scatter_workspace_bytes(B, S*K). */
size_t hsp_rf_bwd_scatter_workspace_bytes(int B, int SC);
int hsp_rf_surface_bwd(const float *xyz, const float *dirs, const uint16_t *argrow, const float *grad_out,
                       int B, int N, int S, int K, float *grad_dirs, void *ws, size_t ws_bytes,
                       hspStream_t stream);

/* replaces HS_layer.graph_conv after its fm GEMM      gcn3d.py:158-181  (gather of :39-47 fused)
 * fm (B,N,(S+1)*C) = feature_map @ weights + bias: columns [0,C) centre, [C+s*C+c] support s.
 * out (B,N,C) = fm[b,i,c] + mean_s max_n relu(R.D^[:,sC+c]) * fm[b, idx[b,i,n], C+sC+c]
 * argrow (B,N,S*C) uint16 as above.  The (B,N,k,S*C) tensors of the reference are never formed.
 * fwin (B,N,S*C) fp32 or NULL: the winner's support value fm[b, argrow[b,i,j], C+j], which
 * hsp_rf_conv_bwd_scatter reads as a stream (inference passes NULL).
 */
int hsp_rf_conv_wants_fwin(int N, int S, int C);
/* Which forward kernel a (k, S, C) runs, for every hsp_rf_*_fwd* entry point (the dispatch decides by the same function): returns the
 * column slots per thread, 1 ... 4 = ceil(S*C / 1024), or 0 where the call is declined (HSP_ERR_UNSUPPORTED: C % 4, S*C > 4096,
 * (S*C + 5 k) floats > 64 KiB of LDS); *pipelined (may be NULL) = 1 for the pipelined schedule, taken wherever
 * S*C/4 - (slots-1)*256 + k <= 256, else 0 for the plain one (which serves any k the LDS holds, k > 256 included). */
int hsp_rf_fwd_plan(int k, int S, int C, int *pipelined);
int hsp_rf_conv_fwd(const float *xyz, const int32_t *idx, const float *dirs, const float *fm, int B,
                    int N, int k, int S, int C, float *out, uint16_t *argrow, float *fwin,
                    hspStream_t stream);
/* Backward, COLUMN-TILE LDS-SCATTER form (the default of the Python mirror): a (cloud, 16-column) tile
 * of grad_fm plus the cloud's xyz live in LDS; gradients are routed to row argrow[b,i,j] with integer LDS adds
 * (immune to the in-degree hubs of feature-space graphs) and every row segment is written once.
 * grad_fm (B,N,(S+1)*C) and grad_dirs (3,S*C) are OVERWRITTEN.  hsp_rf_conv_bwd is the gather-form twin.
 * fwin: the forward's (B,N,S*C) winner support values (then fm may be NULL), or NULL: the values are
 * gathered from fm (B,N,(S+1)*C).  hsp_rf_conv_wants_fwin(N,S,C) says which is faster (fwin once a cloud's
 * fm outgrows the L2 share it gets).
 * ws: hsp_rf_bwd_scatter_workspace_bytes(B, S*C).
 * The tile accumulates in 32-bit fixed point: per (cloud, column tile) the quantum is q = 2^(ex + ceil(log2 N) - 30), 2^ex the
 * power of two above max |grad_out| / S over the tile's channels, so a grad_fm support cell is a multiple of q, carries at
 * most q/2 of rounding per routed term, cannot overflow (a cell receives at most one term per point, |theta| <= 1), and is
 * the same bits on every run.  A tile whose gradients are all zero gives exact zeros.
 * Non-finite gradients: a NaN at grad_out[b,i,c] arrives in the centre column grad_fm[b,i,c] as it is (a copy); every cell
 * that this element does not feed -- all of grad_fm but the support cells (argrow[b,i,s*C+c], C+s*C+c), all of grad_dirs but
 * the columns s*C+c -- is finite and correct (a NaN is ignored where the tile's scale is chosen).  What the fed cells
 * hold is unspecified. */
int hsp_rf_conv_bwd_scatter(const float *xyz, const float *dirs, const float *fm, const float *fwin,
                            const uint16_t *argrow,
                            const float *grad_out, int B, int N, int S, int C, float *grad_fm,
                            float *grad_dirs, void *ws, size_t ws_bytes, hspStream_t stream);
/* Which tile kernel hsp_rf_conv_bwd_scatter* (surface = 0) / hsp_rf_surface_bwd* (surface != 0) run for a shape (the dispatch
 * decides by the same function): returns the tile width in columns (64, 32, 16, 8 or 4) or 0 where the call is declined
 * (HSP_ERR_UNSUPPORTED); *row_split (may be NULL) = 1 for one whole-cloud tile per workgroup, 2 for the two half-cloud tiles
 * of 16 columns that dense clouds take, 0 with a decline. */
int hsp_rf_bwd_scatter_plan(int B, int N, int S, int C, int surface, int *row_split);
/* How the tile kernel of hsp_rf_conv_bwd_scatter* / hsp_rf_surface_bwd* (and their _partial forms) schedules its loads; what it
 * computes is the same bits under both values.  legacy = 0 (the default): every independent load of a workgroup's set-up is issued
 * as register batches before anything waits, grad_out is read once where the rows a thread visits fit its registers, the sweep
 * runs a register ring several points deep and the centre columns are copied by all tiles of a cloud.  legacy = 1: the first
 * form (one load per wait, a sweep one point ahead, grad_out read twice, the first C / tile-width tiles copy the centre
 * columns), kept for the A/B and the tests.  Process-wide; read when a call is issued, so a captured graph keeps the schedule it
 * was captured with.  Returns the previous value, or HSP_ERR_BAD_ARG (and changes nothing) for anything but 0 / 1. */
int hsp_rf_bwd_set_schedule(int legacy);
/* Host-only: bind a column-normalised copy `hat` (3, SC) fp32, 16-byte aligned, of the raw direction parameter `dirs` (3, SC).
 * Every hsp_rf_* forward and backward entry point (fp32 and bf16 rows, scatter, gather and _partial forms) called with that `dirs`
 * address and that S*C afterwards loads `hat` instead of normalising `dirs` in each workgroup's prologue; the direction
 * gradient's Jacobian still reads `dirs`.  `hat` must hold, when such a kernel runs, exactly what the kernel would compute --
 * hsp_split_params_x3 writes it for an HspSplitDesc with transpose = 2 -- so results are the same bits bound or unbound.  The
 * caller keeps both buffers alive while bound.  hat = NULL unbinds.  Process-wide; read when a call is issued, so a captured graph
 * keeps the table it was captured with.  Launches nothing.  hsp_rf_dirs_hat_lookup returns the table bound to (dirs, SC) or NULL. */
int hsp_rf_dirs_hat_bind(const float *dirs, int SC, const float *hat);
const float *hsp_rf_dirs_hat_lookup(const float *dirs, int SC);
/* Backward, GATHER form over rev_off/rev_edge = hsp_rev_build(idx) of the SAME idx the forward used:
 * every grad_fm row is summed in ascending edge order (no atomics, bit-reproducible).
 * The rows of one neighbour list idx[b,i,:] must be DISTINCT: a hit is "the winner of (i, j) is this row", so a row listed
 * in two slots of the same list would be counted once per slot.  (KNN lists are; the scatter form has no such requirement.)
 * ws: hsp_rf_bwd_workspace_bytes(S*C). */
size_t hsp_rf_bwd_workspace_bytes(int SC);
int hsp_rf_conv_bwd(const float *xyz, const float *dirs, const float *fm, const uint16_t *argrow,
                    const float *grad_out, const int32_t *rev_off, const int32_t *rev_edge, int B, int N,
                    int k, int S, int C, float *grad_fm, float *grad_dirs, void *ws, size_t ws_bytes,
                    hspStream_t stream);

/* ---- reverse-edge (CSR) index of a neighbour graph --------------------------------------------
 * replaces the accumulate-scatter (_index_put_impl_) that autograd runs for the gather of
 * indexing_neighbor_new (gcn3d.py:39-47): idx (B,Nq,kstride), first k columns used ->
 * rev_off (B,Nsrc+1), rev_edge (B,Nq*k): for source row m the ascending edge ids e = i*k + n with
 * idx[b,i,n] == m are rev_edge[b][rev_off[b][m] .. rev_off[b][m+1]).
 */
/* 1 where hsp_rev_build, hsp_rev_build_sel and (per map) hsp_rev_build_multi take a cloud of n_src source rows: its histogram of
 * n_src + 1 counters within 140 KB of LDS (n_src <= 35 839) -- the function those entry points themselves decline by */
int hsp_rev_build_takes(int n_src);
/* the form a map of n_q queries with k slots each over n_src source rows takes in those entry points: 1 -- the cloud's edges are
 * assembled and sorted in LDS ((n_src + 1) * 4 + n_q * k * 4 bytes <= 140 KiB), 0 -- in global memory (rev_edge itself), -1 --
 * declined (hsp_rev_build_takes(n_src) == 0, or n_q / k <= 0).  The same rev_off / rev_edge either way; answered by the
 * function the launches pick their kernel with. */
int hsp_rev_build_edges_in_lds(int n_src, int n_q, int k);
int hsp_rev_build(const int32_t *idx, int B, int Nq, int Nsrc, int k, int kstride, int32_t *rev_off,
                  int32_t *rev_edge, hspStream_t stream);
/* nmaps <= 4 such indices over the same B clouds in ONE launch (map i: idx[i], Nq[i], Nsrc[i], k[i], kstride[i] ->
 * rev_off[i], rev_edge[i]); the outputs of hsp_rev_build map by map. */
int hsp_rev_build_multi(int nmaps, const int32_t *const *idx, int B, const int *Nq, const int *Nsrc, const int *k,
                        const int *kstride, int32_t *const *rev_off, int32_t *const *rev_edge, hspStream_t stream);

/* hsp_rev_build over the lists of a Pool_layer's KEPT rows: query q (of Nq) reads idx row r = qsel[b * qsel_stride + q] (of the
 * cloud's Nidx), so for source row m the ascending edge ids e = q*k + n with idx[b, r, n] == m are
 * rev_edge[b][rev_off[b][m] .. rev_off[b][m+1]); rev_off (B,Nsrc+1), rev_edge (B,Nq*k).  qsel_stride: 0 -- one list (Nq) shared by
 * the batch -- or >= Nq -- a list per cloud, the rules of hsp_gather_max_fwd_sel; a list may name a row more than once, each
 * listing is a query of its own.  qsel == NULL (then Nq == Nidx and qsel_stride == 0) is hsp_rev_build itself.  The entries of
 * qsel and idx are device data and are not range-checked.  A NULL idx / rev_off / rev_edge, a size <= 0, kstride < k or a bad
 * stride: HSP_ERR_BAD_ARG, nothing launched; (Nsrc + 1) * 4 bytes > 140 KiB of LDS (Nsrc > 35 839): HSP_ERR_UNSUPPORTED, as
 * hsp_rev_build. */
int hsp_rev_build_sel(const int32_t *idx, const int32_t *qsel, int qsel_stride, int B, int Nidx, int Nq, int Nsrc, int k,
                      int kstride, int32_t *rev_off, int32_t *rev_edge, hspStream_t stream);

/* ---- neighbourhood max-pool (ORL global branch, Pool_layer) ----------------------------------
 * replaces indexing_neighbor_new(...) + max(dim=2)    gcn3d.py:214-216, :236-240
 * feat (B,Nsrc,C); idx (B,Nidx,kstride) of which the first k columns are used; qsel (Nq) optional
 * row selector shared by the batch (Pool_layer's randperm slice, gcn3d.py:243-245; NULL = identity,
 * then Nq must equal Nidx).  out (B,Nq,C) = max_{n<k} feat[b, idx[b, q', n], :], q' = qsel ? qsel[q] : q;
 * argmax (B,Nq,C) uint8.
 */
int hsp_gather_max_fwd(const float *feat, const int32_t *idx, const int32_t *qsel, int B, int Nsrc,
                       int Nidx, int Nq, int k, int kstride, int C, float *out, uint8_t *argmax,
                       hspStream_t stream);
/* grad_feat (B,Nsrc,C) is OVERWRITTEN.  grad_out is (B,Nq,C), or (B,C) broadcast over q when
 * grad_bcast != 0 (the ORL mean-over-points branch; integer counts in LDS => exactly reproducible).
 * Column-tile LDS scatter when a (Nsrc x 16-column) tile fits LDS, else memset + global atomics. */
/* Pool_layer (gcn3d.py:220-246) in ONE launch: out (B,Nq,C) = max over the first k listed neighbours of the kept rows qsel
 * (Nq ints, shared by the batch) + argmax, and xyz_sel (B,Nq,3) = xyz[:, qsel] (the reference's vertices[:, sample_idx]). */
int hsp_pool_fwd(const float *feat, const float *xyz, const int32_t *idx, const int32_t *qsel, int B, int N, int Nq, int k,
                 int kstride, int C, float *out, uint8_t *argmax, float *xyz_sel, hspStream_t stream);
/* The plan of the column-tile LDS scatter behind hsp_gather_max_bwd* and hsp_gather_rows_bwd (their dispatch decides by the same functions):
 * returns the tile width (16, 8 or 4 columns: the widest that divides C with Nsrc * width * 4 bytes <= 144 KiB) or 0 where no
 * tile fits (then fp32 falls back to memset + global atomics, without `extra`; bf16 declines); *threads (may be NULL) = the
 * workgroup size, 1024 / 512 / 256 by the grid (C / width) * B against the 256 CUs. */
int hsp_scatter_tile_plan(int B, int Nsrc, int C, int *threads);
/* grad_bcast == 2 (hsp_gather_max_bwd and _bf16): `argmax` points at the winner counts (B,Nsrc,C) uint16 that hsp_orl_global_fwd
 * left in its workspace (hsp_orl_counts_offset; 8-byte aligned) instead of the arg-max bytes; grad_out is the (B,C) fp32 row as for
 * grad_bcast == 1.  idx and qsel are ignored and may be NULL, Nidx / Nq / kstride are ignored.  One streaming launch, no LDS, no
 * atomics: grad_feat = grad_out[b] * count (+ grad_feat if accumulate) (+ extra), the same expression in the same order as the
 * flush of the LDS scatter, hence the same bits as grad_bcast == 1 on the arg-max bytes of the same forward call. */
int hsp_gather_max_bwd(const float *grad_out, int grad_bcast, const int32_t *idx, const int32_t *qsel,
                       const uint8_t *argmax, int B, int Nsrc, int Nidx, int Nq, int kstride, int C,
                       float *grad_feat, int accumulate /* !=0: add into grad_feat instead of overwriting */,
                       const float *extra /* optional (B,Nsrc,C) tensor added in the same pass, or NULL */,
                       hspStream_t stream);
/* The pooling entry points with a row selector PER CLOUD (gcn3d.Pool_layer(sampler="fps"): every cloud keeps the rows its own
 * farthest-point sampling picks).  Same arguments, semantics and kernels as hsp_gather_max_fwd / hsp_pool_fwd / hsp_gather_max_bwd
 * and their bf16 twins, plus qsel_stride: 0 -- qsel (Nq) is one list shared by the batch (the entry points above forward here with
 * 0); >= Nq -- cloud b keeps the rows qsel[b * qsel_stride + q] (a dense (B,Nq) selector has qsel_stride == Nq).  Any other
 * stride, or a non-zero stride with qsel == NULL: HSP_ERR_BAD_ARG.  A list may name a source row more than once (a tiled cloud):
 * each listing is one output row of its own and one more contribution to the backward's sum.  The entries are device data and
 * are not range-checked: every entry must lie in [0, Nidx). */
int hsp_gather_max_fwd_sel(const float *feat, const int32_t *idx, const int32_t *qsel, int qsel_stride, int B, int Nsrc,
                           int Nidx, int Nq, int k, int kstride, int C, float *out, uint8_t *argmax, hspStream_t stream);
int hsp_pool_fwd_sel(const float *feat, const float *xyz, const int32_t *idx, const int32_t *qsel, int qsel_stride, int B, int N,
                     int Nq, int k, int kstride, int C, float *out, uint8_t *argmax, float *xyz_sel, hspStream_t stream);
int hsp_gather_max_bwd_sel(const float *grad_out, int grad_bcast, const int32_t *idx, const int32_t *qsel, int qsel_stride,
                           const uint8_t *argmax, int B, int Nsrc, int Nidx, int Nq, int kstride, int C, float *grad_feat,
                           int accumulate, const float *extra, hspStream_t stream);
/* the same result in GATHER form over hsp_rev_build(idx, k) (qsel == NULL case, Nq rows of idx):
 * each grad_feat row written once, no atomics. */
int hsp_gather_max_bwd_csr(const float *grad_out, int grad_bcast, const uint8_t *argmax, const int32_t *rev_off,
                           const int32_t *rev_edge, int B, int Nsrc, int Nq, int k, int C, float *grad_feat,
                           hspStream_t stream);
/* The ORDERED pooling backward (config.FLAGS.reproducible): hsp_gather_max_bwd_csr and its storage-type twin over
 * (rev_off, rev_edge) = hsp_rev_build_sel(idx, qsel, ...), k the k of that call, argmax / grad_out the (B,Nq,C) of the forward
 * over the same kept rows.  For every cloud b, source row m and column c, in fp32:
 *   s = +0;  for q = 0 .. Nq-1 ascending:  if idx[b, r_q, argmax[b,q,c]] == m:  s = fl32(s + float(grad_out[b,q,c]))
 *   grad_feat[b,m,c] = s        (bf16 storage: rounded once, to nearest even)
 * with r_q = qsel ? qsel[b * qsel_stride + q] : q.  No atomics; every grad_feat row is written exactly once (no memset, a row no
 * query won is zeros); any Nsrc the reverse index takes, no LDS tile.  A row listed in several slots of one list counts once per
 * query (the slot argmax names).  One thread per (source row, 4 columns) walks the row's edge list: written for the pool graphs'
 * mean in-degree k Nq / Nsrc ~ 1, no hub handling (a long list is walked serially).  grad_bcast != 0: grad_out is the fp32 (B,C)
 * row of hsp_gather_max_bwd and grad_feat = grad_out[b] * (number of winning queries), one rounding.  _bf16: grad_out (B,Nq,C) and
 * grad_feat bf16, the broadcast row fp32.  C % 4 != 0: HSP_ERR_UNSUPPORTED; a NULL pointer or a size <= 0: HSP_ERR_BAD_ARG. */
int hsp_gather_max_bwd_csr_bf16(const void *grad_out, int grad_bcast, const uint8_t *argmax, const int32_t *rev_off,
                                const int32_t *rev_edge, int B, int Nsrc, int Nq, int k, int C, hsp_bf16_t *grad_feat,
                                hspStream_t stream);

/* ---- max over the points of a cloud (the heads' global feature) ------------------------------
 * replaces torch.max(x, 2, keepdim=True)[0]    PoseR.py:30 / :61, PoseTs.py:35, FaceRecon.py:98
 * x (B,N,C) point-major; out (B,C) = max_n x[b,n,c]; argrow (B,C) int32 = the FIRST row attaining
 * it (NaN counts as the maximum, as in ATen).  bwd: grad_x (B,N,C) is OVERWRITTEN with grad_out on
 * the winning row and 0 elsewhere (C % 4 == 0). */
int hsp_points_max_fwd(const float *x, int B, int N, int C, float *out, int32_t *argrow, hspStream_t stream);
int hsp_points_max_bwd(const float *grad_out, const int32_t *argrow, int B, int N, int C, float *grad_x,
                       hspStream_t stream);

/* ORL global feature in one pass (get_ORL_global, gcn3d.py:211-218, before the repeat):
 * fg (B,C) = mean_i max_{n<k} feat[b, idx[b,i,n], :], argmax (B,N,C) uint8; the (B,N,C) max tensor is never
 * written.  idx (B,N,kstride).  ws: hsp_orl_workspace_bytes(B,N,C).  Backward: hsp_gather_max_bwd(grad_bcast=1).
 *
 * Winner counts (fp32 rows): a LARGER workspace asks hsp_orl_global_fwd to also leave counts (B,N,C) uint16,
 * counts[b][m][c] = #{i : idx[b][i][argmax[b][i][c]] == m} -- all the backward needs of this call -- at byte offset
 * hsp_orl_counts_offset(B, N, k, kstride, C, ws_bytes) of ws.  The offset is hsp_orl_workspace_bytes rounded up to 256, and
 * ws_bytes must cover B*N*C*2 bytes after it; the query returns -1, and the call writes no counts, when ws_bytes is smaller
 * or the call does not take the LDS slab kernel: k != 20, kstride != k, C % 8, a cloud whose slab is past the LDS limit
 * (N > 2858), or a C the forward itself declines (C / 4 must divide 256, as without counts: HSP_ERR_UNSUPPORTED).
 * ws must be 16-BYTE ALIGNED for counts (the query does not see the pointer): a call whose ws is large enough but not so
 * aligned is the plain call -- it succeeds and writes NO counts -- so a caller that wants them aligns ws, and a caller that
 * passes some larger scratch buffer without wanting them loses nothing but, when aligned, has B*N*C*2 bytes written there.
 * fg and argmax are bit for bit those of the call with the plain workspace size.
 * Clouds under 128 points (k = 20): the plain call is the chunked form (two launches); with counts the slab kernel runs AFTER
 * it as a third launch, only to count: fg stays the chunked form's (its fold order), the arg-max bytes are rewritten by the
 * slab kernel so that they are the winners the counts count.  The two kernels pick the same winner for ordinary numbers and
 * differ only where the comment at max3_raw (csrc/gather.hip) says they do, on NaN activations -- there argmax/counts follow
 * the slab kernel and fg the chunked one.  Whether the extra launch pays is the caller's choice: hs_pose_amd.ops asks for
 * counts only from 128 points on.
 * Backward from the counts: hsp_gather_max_bwd(grad_bcast=2).  hsp_orl_global_fwd_bf16 never writes counts (its slab rows
 * have no room for them) and ignores the extra bytes. */
size_t hsp_orl_workspace_bytes(int B, int N, int C);
long long hsp_orl_counts_offset(int B, int N, int k, int kstride, int C, size_t ws_bytes);
int hsp_orl_global_fwd(const float *feat, const int32_t *idx, int B, int N, int k, int kstride, int C,
                       float *fg, uint8_t *argmax, void *ws, size_t ws_bytes, hspStream_t stream);
/* The same feature with the REFERENCE's summation order: ATen's cascade sum over the points (16-row level-0 chunks, levels dumped
 * every 16 / 256 / 4096 rows, remainder last) then a division by N -- torch.mean(dim=1) of gcn3d.py:217 bit for bit
 * (tests/golden/exact_*.npz).  ws: hsp_orl_exact_workspace_bytes(B,N,C).  argmax as above. */
size_t hsp_orl_exact_workspace_bytes(int B, int N, int C);
int hsp_orl_global_exact_f32(const float *feat, const int32_t *idx, int B, int N, int k, int kstride, int C, float *fg,
                             uint8_t *argmax, void *ws, size_t ws_bytes, hspStream_t stream);
/* eval-mode BatchNorm1d of FaceRecon.py:90-95 on point rows x (R,C) in ATen's own operation order (the reference applies it to
 * a transposed view: the generic TensorIterator path): y = ((x - running_mean) * invstd) * weight + bias, every operation
 * rounded to fp32, optionally followed by relu.  invstd (C) = 1 / sqrt(running_var + eps) as the HOST's ATen evaluates it
 * (its sqrt is MKL VML's, not correctly rounded: one channel in ~180 differs), or NULL: the correctly rounded value from
 * running_var.  C % 4 == 0. */
int hsp_bn_eval_f32(const float *x, long long R, int C, const float *running_mean, const float *running_var,
                    const float *invstd, const float *weight, const float *bias, float eps, int relu, float *y,
                    hspStream_t stream);
/* The HS layer's out product in the reference's order of operations (gcn3d.py:111-112 / :185-186 then :90 / :156): every product a
 * k-ordered fp32 fma chain from 0 (what the reference's CPU GEMM runs for K <= 256; K = 512 is two such chains added), additions
 * in the reference's order.  two_chain == 0 (2C <= 256): out = ((chain(F Wa^T) continued by chain(fg[cloud] Wb^T)) + F) + tail;
 * two_chain == 1: out = (((chain(F Wa^T)) + cloud_t[cloud]) + F) + tail with cloud_t (B,C) = chain(fg Wb^T) from
 * hsp_gemm_wave_f32.  tail = ste (M,C) (the STE product) or the K = 3 chain xyz3 . w3 (surface layer; relu allowed).
 * C % 32 == 0, 16-byte aligned rows, rows_per_cloud >= 32. */
/* 1 where the reference-order entry points of one HS layer -- hsp_gemm_wave_f32 for the fm and STE products (Cin != 3),
 * hsp_orl_global_exact_f32, hsp_layer_out_exact_f32 with two_chain = (2 C > 256) -- all take a cloud of N points with Cin input and C
 * output channels: the function hsp_layer_out_exact_f32 itself declines by for its own part (its plan, C <= 256 in one or two
 * chains, rows_per_cloud >= 32), with the other two entry points' shape rules */
int hsp_exact_layer_takes(int N, int Cin, int C);
int hsp_layer_out_exact_f32(const float *F, int ldf, const float *Wa, int ldwa, const float *fg, int ldfg, const float *Wb,
                            int ldwb, const float *cloud_t, int two_chain, const float *ste, int ldste, const float *xyz3,
                            const float *w3, int relu, int M, int C, int rows_per_cloud, float *out, int ldo,
                            hspStream_t stream);
/* out (B,C) = sum_i x[b,i,:]  (the per-cloud column sum autograd takes of a gradient that was
 * broadcast over the points, e.g. d/d(fg Wb^T)); deterministic two-stage.  ws as above. */
/* 1 where hsp_colsum_rows (elem_bytes 4) / hsp_colsum_rows_bf16 (2) take rows of C columns: C a multiple of 4 with C/4 | 256, fp32
 * rows also any C <= 256 -- the function those entry points themselves decline by */
int hsp_colsum_rows_takes(int C, int elem_bytes);
/* The chunking of the per-cloud column sums -- hsp_colsum_rows (elem_bytes 4), hsp_colsum_rows_bf16 (2), hsp_colsum_rows_xyz(_bf16)
 * and hsp_colsum_cloud_f32 where they take the shape -- from the functions the launches use.  A cloud's N rows are cut into
 * *nchunk chunks of *rows rows (the last may be shorter); a workgroup sums a chunk with *row_lanes row lanes, lane l adding rows
 * l, l + row_lanes, ... of the chunk one by one from +0; the lanes are folded in ascending order from lane 0; the chunk sums are
 * folded as eight running sums over chunk (chunk ch into sum ch % 8, ascending) combined pairwise
 * ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)): at most ceil(rows / row_lanes) + (row_lanes - 1) + ceil(nchunk / 8) + 3
 * additions on the path of any row.  *form: 0 -- four columns per lane (C a multiple of 4 with C/4 | 256), 1 -- one column per
 * lane (fp32 rows of any other C <= 256), -1 -- hsp_colsum_rows_takes(C, elem_bytes) is 0 (then the other three are 0).
 * Returns HSP_OK, or HSP_ERR_BAD_ARG (nothing written) for a size <= 0, elem_bytes other than 2 / 4 or a NULL pointer. */
int hsp_colsum_rows_plan(int B, int N, int C, int elem_bytes, int *rows, int *nchunk, int *row_lanes, int *form);
int hsp_colsum_rows(const float *x, int B, int N, int C, float *out, void *ws, size_t ws_bytes,
                    hspStream_t stream);

/* out (B,N,C) += f (B,N,C) + t (B,C) broadcast over the points: the "+ feature" residual and the per-cloud
 * half of conv2 of an HS layer (gcn3d.py:112,186) in one pass.  Association: out = fl(out + fl(f + t[b])), both additions
 * rounded to fp32.  C % 4 != 0: HSP_ERR_UNSUPPORTED. */
/* out (R, C) = (ga + gb) * [y > 0]: the backward of relu(conv_0(...)) (FaceRecon.py:88) fused with the sum of the two gradients
 * that reach fm_0 (conv_1 and the concat); ga / gb rows of an even pitch lda / ldb (8-byte aligned), gb may be NULL; C even
 * (an odd C, lda or ldb: HSP_ERR_UNSUPPORTED).  The mask is the fp32 comparison y > 0: a positive subnormal passes the gradient,
 * +0 and -0 give 0 -- as ATen's threshold_backward -- and y = NaN gives 0 (the comparison is false), where threshold_backward
 * passes the gradient: a NaN activation is an upstream fault, not a case the two promise to agree on. */
int hsp_add_relu_bwd(const float *ga, int lda, const float *gb, int ldb, const float *y, int R, int C, float *out,
                     hspStream_t stream);
int hsp_residual_bias(float *out, const float *f, const float *t, int B, int N, int C, hspStream_t stream);

/* ---- feature assembly ---------------------------------------------------------------------------
 * replaces the nearest-up-sampling gathers + one-hot repeat + torch.cat     FaceRecon.py:100-107
 * out (B,N,sum width): column segment s of row (b,i) is
 *   kind 0: src[s][(b*N+i)*w .. ]   kind 1: src[s][(b*nsrc[s] + idx[s][b*N+i])*w ..]   kind 2: src[s][b*w ..]
 *   kind 3: (long) src[s][b] == c ? 1 : 0  -- one-hot columns from the (B) float category ids (FaceRecon.py:80-85)
 * (host arrays of nseg <= 8 entries; device pointers inside).  The backward of kind-1 segments is
 * hsp_gather_rows_bwd with grad_stride = total width.
 */
int hsp_concat_rows(int nseg, const float *const *src, const int32_t *const *idx, const int *width,
                    const int *kind, const int *nsrc, int B, int N, float *out, hspStream_t stream);

/* ---- row gather (nearest up-sample, vertex select) -------------------------------------------
 * replaces indexing_neighbor_new(t, nearest).squeeze(2)    FaceRecon.py:102-104 ; vertices[:, sample_idx]
 * feat (B,Nsrc,C); idx (B,Nq) or, when idx_shared != 0, (Nq) shared by the batch.
 * out rows are written at out + (b*Nq+q)*out_stride (out_stride >= C lets the caller write straight
 * into a slice of the concatenated feature tensor, FaceRecon.py:107).
 */
int hsp_gather_rows_fwd(const float *feat, const int32_t *idx, int idx_shared, int B, int Nsrc, int Nq,
                        int C, float *out, int out_stride, hspStream_t stream);
/* grad_feat (B,Nsrc,C) OVERWRITTEN; grad_out rows at grad_out + (b*Nq+q)*grad_stride. */
int hsp_gather_rows_bwd(const float *grad_out, int grad_stride, const int32_t *idx, int idx_shared, int B,
                        int Nsrc, int Nq, int C, float *grad_feat, hspStream_t stream);
/* the same backward in gather form over (rev_off, rev_edge) = hsp_rev_build(idx as (B,Nq,1), k = 1): every source row
 * sums its queries' gradient rows in ascending query order (no atomics, bit-reproducible), whole row segments at
 * a time -- the faster form when grad_out is a column block of a much wider tensor (the 1286-wide feature). */
/* 1 where hsp_gather_rows_bwd_csr(_bf16) takes a gradient of C columns of elem_bytes each at row stride grad_stride (elements)
 * whose address is grad_align modulo 16: even C and stride, a 2-element-aligned address, C/2 >= 256 or C/2 | 256 -- the function
 * those entry points themselves decline by; hsp_gather_rows_bwd_csr_multi(_bf16) asks it once per segment */
int hsp_gather_rows_bwd_csr_takes(int elem_bytes, int C, int grad_stride, int grad_align);
int hsp_gather_rows_bwd_csr(const float *grad_out, int grad_stride, const int32_t *rev_off, const int32_t *rev_edge,
                            int B, int Nsrc, int Nq, int C, float *grad_feat, hspStream_t stream);
/* nseg <= 4 such gathers out of ONE gradient tensor (row pitch grad_stride, Nq rows per cloud; segment s: grad_out[s] = the
 * tensor's base + the segment's column offset, rev_off[s] / rev_edge[s], Nsrc[s], C[s] -> grad_feat[s]) in ONE launch, the
 * bits of hsp_gather_rows_bwd_csr segment by segment: the backward of the feat concat's gathered segments.  A thread moves
 * 16 bytes where the segment's width, pitch and addresses allow, else two elements.  HSP_ERR_UNSUPPORTED where
 * hsp_gather_rows_bwd_csr declines one of the segments (nothing is launched). */
int hsp_gather_rows_bwd_csr_multi(int nseg, const float *const *grad_out, int grad_stride, const int32_t *const *rev_off,
                                  const int32_t *const *rev_edge, int B, const int *Nsrc, int Nq, const int *C,
                                  float *const *grad_feat, hspStream_t stream);

/* ---- dense per-point products (forward / input-gradient GEMMs with fused tails) ----------------
 * replaces the matmuls / Conv1d(k=1) of an HS layer and of the heads and the element-wise tail around them:
 *   feature_map @ self.weights + self.bias                                  gcn3d.py:171   ("nn" B, bias)
 *   STE_layer(x) + conv2(cat[feature, f_global]) + feature                  gcn3d.py:149,156,186 (two sources,
 *                                                  resid = feature, cloud_bias = f_global Wb^T per cloud)
 *   their input gradients (g Wa ; g Wste + gfm W^T)                          autograd of the above
 *   Conv1d(Cin, Cout, 1) of the heads                                       PoseR.py:16-39, PoseTs.py:18-45, FaceRecon.py:37-68
 * C (M,N) = alpha * (A1 (M,K1) op(B1) [+ A2 (M,K2) op(B2)]) [+ bias (N)] [+ resid (M,N)] [+ cloud_bias[row / rows_per_cloud] (N)]
 *           [+ xyz3[row] . w3[col]]     (xyz3 (M,3), w3 (N,3) fp32: the K = 3 STE of HSlayer_surface on raw coordinates,
 *                                        gcn3d.py:85 -- coordinates never pass through bf16, gcn3d.py:57,59)
 * b?_layout 0 = "nt": B is (N,K), k contiguous (a Linear / Conv1d weight);  1 = "nn": B is (K,N) (HS_layer.weights).
 * A2 == NULL: single source.  Leading dimensions in elements; any K, any alignment (aligned operands stage 16 bytes
 * per load).  fp32: v_mfma_f32_32x32x2_f32 (exact fp32).  bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulate, "nt"
 * operands only, bias / cloud_bias fp32, resid bf16, C bf16 (round to nearest even) or fp32.
 */
int hsp_gemm_rows_f32(const float *A1, int lda1, const float *B1, int ldb1, int b1_layout, int K1,
                      const float *A2, int lda2, const float *B2, int ldb2, int b2_layout, int K2, int M, int N,
                      const float *bias, const float *resid, int ldr, const float *cloud_bias, int rows_per_cloud,
                      float alpha, const float *xyz3, const float *w3, float *C, int ldc, void *ws, size_t ws_bytes,
                      hspStream_t stream);
/* ws: hsp_gemm_rows_workspace_bytes(M,N,K1,K2, 4 | 2) -- 0 unless few output tiles meet a deep K (the input-gradient
 * products), which then split K over up to 16 workgroups per tile and fold the partial tiles in a second launch; with
 * ws == NULL (or too small) the product runs unsplit */
size_t hsp_gemm_rows_workspace_bytes(int M, int N, int K1, int K2, int elem_bytes);
/* host-only: what hsp_gemm_rows_f32 (elem_bytes 4) / hsp_gemm_rows_*bf16 (2) run for a shape (the dispatch decides by the same
 * functions): out[4] = tile edge (64 | 128), staging mode (1: 16-byte, 2: 8-byte, 0: 4-byte pieces), K splits with a workspace
 * of hsp_gemm_rows_workspace_bytes (1 = unsplit), k-blocks of 128 bytes over both sources.  align: the smallest of 16 | 8 | 4
 * that every operand's base pointer and row pitch in bytes is a multiple of.  K2 = 0: one source; the split of a dual-source
 * call does not depend on the order of its sources.  HSP_ERR_UNSUPPORTED: bf16 operands off a 16-byte alignment. */
int hsp_gemm_rows_plan(int M, int N, int K1, int K2, int elem_bytes, int align, int *out);
int hsp_gemm_rows_bf16(const hsp_bf16_t *A1, int lda1, const hsp_bf16_t *B1, int ldb1, int K1,
                       const hsp_bf16_t *A2, int lda2, const hsp_bf16_t *B2, int ldb2, int K2, int M, int N,
                       const float *bias, const hsp_bf16_t *resid, int ldr, const float *cloud_bias,
                       int rows_per_cloud, float alpha, const float *xyz3, const float *w3, void *C, int ldc,
                       int c_is_f32 /* != 0: C is fp32 (an output that feeds BatchNorm keeps its mantissa) */,
                       void *ws, size_t ws_bytes, hspStream_t stream);

/* The same product (same arguments, same result contract; reference gcn3d.py:149,171,186 and their input gradients) by the
 * LDS-free wave-level kernel of csrc/gemm_wave.hip: every wave is an independent worker that streams both operands from
 * L2 / L1 straight into MFMA operand layout (16-byte buffer loads, a ring of 4 steps of 8 k in flight that does not drain
 * between the sources of a product nor between the tiles of a wave), no LDS, no barriers; the work is cut per WAVE -- a
 * contiguous run of (32|64) x (32|64|128) tiles each, the tiles that do not divide by the wave count dealt out as 32 x 32
 * blocks -- so there are no partial sums and the result does not depend on the cut.  Covers K1, K2 multiples of 32, N a
 * multiple of 32, 16-byte aligned rows (hsp_gemm_wave_supported; anything else: hsp_gemm_rows_f32); fp32 on
 * v_mfma_f32_32x32x2_f32.  cfg: 0 = automatic tile / cut; otherwise RB | NCB << 4 | waves_per_simd << 16 | order << 28
 * (tuning: rows / 32 and columns / 32 of the wave tile, occupancy, 1 = row panels fastest in the tile order); bit 29 of cfg:
 * relu on the result (the xyz3 + residual + per-cloud-bias form only: relu(conv_0(...)) of FaceRecon.py:88 in the epilogue). */
int hsp_gemm_wave_supported(int M, int N, int K1, int K2, int cfg);
/* host-only: out[10] = rows / 32 and columns / 32 of the wave tile, waves per SIMD, tiles along M and N, whole tiles per wave,
 * waves, first leftover tile, 32 x 32 blocks of the leftover tiles, 0; returns 0 when the shape is not covered */
int hsp_gemm_wave_plan_info(int M, int N, int K1, int K2, int cfg, int *out);
int hsp_gemm_wave_f32(const float *A1, int lda1, const float *B1, int ldb1, int b1_layout, int K1,
                      const float *A2, int lda2, const float *B2, int ldb2, int b2_layout, int K2, int M, int N,
                      const float *bias, const float *resid, int ldr, const float *cloud_bias, int rows_per_cloud,
                      float alpha, const float *xyz3, const float *w3, float *C, int ldc, int cfg, hspStream_t stream);

/* ---- fp32 dense products on the bf16 matrix cores, fp32-accurate (csrc/gemm_x3.hip) ---------------------------------------
 * replaces the same reference lines as hsp_gemm_rows_f32 (gcn3d.py:149,171,186 and their input gradients; the Conv1d(k=1)
 * layers of PoseR.py:16-39, PoseTs.py:18-45, FaceRecon.py:37-68):
 *   C = alpha * (A1 W1^T (+ A2 W2^T)) (+ bias) (+ resid) (+ cloud_bias[row / rows_per_cloud])        A*: fp32 rows (M, K*)
 * Every fp32 operand is split EXACTLY into three bf16 slices (x = hi + mid + lo, truncations) and six slice products per k
 * -- each exact in fp32 -- are accumulated in fp32 by v_mfma_f32_32x32x16_bf16; the dropped terms are below 2^-23 |a||b| per
 * product (the rounding an fp32 fma chain commits per step).  The weight-side operand comes ALREADY SPLIT in (N, K) form:
 * three bf16 planes (N, ldp), plane p at P + p * ps elements, columns k >= K zero, ldp >= K rounded up to 32 -- written once
 * per step for every weight by hsp_split_params_x3 (HspSplitDesc: src (rows, cols) fp32 with pitch ld; transpose = 0: src is
 * (N, K); 1: src is (K, N), i.e. the product wants src^T; kp = plane row pitch, ps = plane stride, both in elements and even; tile0 =
 * number of 32 (n) x 64 (k) output pieces, ceil(N / 32) * ceil(K / 64) each, of the entries before; table in DEVICE memory;
 * transpose = 2: not a weight but the raw (3, cols) direction parameter of a receptive-field layer, cols % 4 == 0: dst = its
 * column-normalised fp32 copy (3, cols) for hsp_rf_dirs_hat_bind, ceil(cols / 1024) pieces, kp and ps unused).  Covers N >= 64 and 16-byte aligned
 * activation rows (hsp_gemm_x3_supported; anything else: hsp_gemm_rows_f32); epilogues: none, bias, resid + cloud_bias.
 * Deep-K products with few tiles split K over workgroups (ws: hsp_gemm_x3_workspace_bytes) and fold in a fixed order. */
typedef struct HspSplitDesc { const float *src; void *dst; int rows, cols, ld, transpose, kp, tile0; long long ps; } HspSplitDesc;
int hsp_split_params_x3(const HspSplitDesc *table_dev, int n, int total_tiles, hspStream_t stream);
int hsp_gemm_x3_supported(int M, int N, int K1, int K2);
size_t hsp_gemm_x3_workspace_bytes(int M, int N, int K1, int K2);
/* host-only: what hsp_gemm_x3_f32 runs for a shape (the dispatch decides by the same functions).  epi: bias 1 | resid 2 |
 * cloud_bias 4; K2 = 0: one source.  out[4] = 1 for the panel kernel (K1 = 128, N in whole 128-column panels, 32-row tiles,
 * >= 3 rounds filled to >= 0.75) else 0 for the tile kernel; the tile height in 64-row units (1 | 2; 0 with the panel kernel);
 * K splits with a workspace of hsp_gemm_x3_workspace_bytes (1 = unsplit: any epilogue, or too few k-blocks); the fold's path,
 * 4 = float4 (N and ldc multiples of 4), 1 = scalar, 0 = no fold.  HSP_ERR_UNSUPPORTED where hsp_gemm_x3_supported is 0. */
int hsp_gemm_x3_plan(int M, int N, int K1, int K2, int epi, int ldc, int *out);
int hsp_gemm_x3_f32(const float *A1, int lda1, const hsp_bf16_t *P1, int ldp1, long long ps1, int K1,
                    const float *A2, int lda2, const hsp_bf16_t *P2, int ldp2, long long ps2, int K2, int M, int N,
                    const float *bias, const float *resid, int ldr, const float *cloud_bias, int rows_per_cloud,
                    float alpha, float *C, int ldc, void *ws, size_t ws_bytes, hspStream_t stream);
/* the layer's out product (residual + per-cloud bias) that also leaves the FIRST PASS of the train-mode BatchNorm that follows it
 * (FaceRecon.py:90-95): bn_part[(M + 63) / 64][2][N] = per 64-row tile, sum (c - s[n]) and sum (c - s[n])^2 over the tile's rows
 * of the result, with the shift s[n] = resid[0][n] + cloud_bias[0][n] (this step's data only, so a replayed graph and an eager
 * step agree bit for bit) written to bn_shift (N floats); hsp_bn_relu_fwd_partials folds them (nblk = (M + 63) / 64 <= 512) */
int hsp_gemm_x3_bn_f32(const float *A1, int lda1, const hsp_bf16_t *P1, int ldp1, long long ps1, int K1,
                       const float *A2, int lda2, const hsp_bf16_t *P2, int ldp2, long long ps2, int K2, int M, int N,
                       const float *resid, int ldr, const float *cloud_bias, int rows_per_cloud, float *C, int ldc,
                       float *bn_shift, float *bn_part, hspStream_t stream);
/* the same for a Linear / Conv1d(k=1) WITH BIAS that a train-mode BatchNorm follows (the heads: PoseR.py:27-30, PoseTs.py:32-36,
 * FaceRecon.py:37-47): C = A W^T + bias plus bn_part[tiles][2][N], tiles = hsp_gemm_x3_bn_tiles(M, N) (64- or 128-row tiles by
 * shape, <= 512), shift = bias (written to bn_shift) */
int hsp_gemm_x3_bn_tiles(int M, int N);
int hsp_gemm_x3_bias_bn_f32(const float *A1, int lda1, const hsp_bf16_t *P1, int ldp1, long long ps1, int K1, int M, int N,
                            const float *bias, float *C, int ldc, float *bn_shift, float *bn_part, hspStream_t stream);

/* the per-CLOUD products of the ORL branch (gcn3d.py:186: the f_global half of conv2, one row per cloud of the batch), one
 * launch each, fp32 fma chains in a fixed order:
 *   hsp_small_rows_f32:  out (M, N) = alpha * A (M, K) op(W), M <= 64 (<= 16 unless K is a multiple of 128); w_layout 0: W is (N, K) (t = fg Wb^T), 1: W is (K, N)
 *                        (gfg = gt Wb / N); K <= 2048
 *   hsp_small_outer_f32: out (Ma, Nb) = a^T c over the B <= 64 rows of a (B, Ma), c (B, Nb) (gWb = gt^T fg) */
int hsp_small_rows_f32(const float *A, int lda, const float *W, int ldw, int w_layout, int M, int N, int K, float alpha,
                       float *out, int ldo, hspStream_t stream);
/* 1 where hsp_small_outer_f32 takes B per-cloud rows (one row per lane: B <= 64) -- the function that entry point itself declines by */
int hsp_small_outer_takes(int B);
int hsp_small_outer_f32(const float *a, int lda, const float *c, int ldc, int B, int Ma, int Nb, float *out, int ldo,
                        const float *mom, int ldm, int Cm, float *gste, hspStream_t stream);
/* (mom != NULL: the same launch also writes gste (Cm, 3) = sum over the B rows of mom (B, >= 3 Cm) [j * Cm + c] -- the STE weight
 * gradient of HSlayer_surface, g^T xyz (gcn3d.py:85), from the per-cloud coordinate moments of hsp_colsum_rows_xyz:
 * out4 (B, 4, C), slot 0 = sum_i g[b][i][:], slots 1..3 = sum_i g[b][i][:] * xyz[b][i][0..2]; ws >= 4 * hsp_orl_workspace_bytes) */
/* 1 where hsp_colsum_rows_xyz(_bf16) takes rows of C columns (C a multiple of 4 with C/4 | 256) -- the function those entry points
 * themselves decline by */
int hsp_colsum_rows_xyz_takes(int C);
int hsp_colsum_rows_xyz(const float *x, const float *xyz, int B, int N, int C, float *out4, void *ws, size_t ws_bytes,
                        hspStream_t stream);
int hsp_colsum_rows_xyz_bf16(const hsp_bf16_t *x, const float *xyz, int B, int N, int C, float *out4, void *ws, size_t ws_bytes,
                             hspStream_t stream);

/* The per-cloud chain of an HS layer's backward in two launches instead of four (fp32 training path), bit for bit what the
 * entry points above compute -- a dependent launch of this size costs 4-6 us whatever it does:
 *   hsp_colsum_cloud_f32: hsp_colsum_rows (xyz == NULL: out (B, C)) or hsp_colsum_rows_xyz (out (B, 4, C)) with both stages in
 *                         one launch and no workspace: a workgroup per (cloud, C/8 columns) sums the same chunks in the same
 *                         order and folds them itself.  hsp_colsum_cloud_ok: 1 where it takes the shape (C a multiple of 32
 *                         with C/4 | 256, at most 65535 clouds, the chunk sums of a column tile fit in LDS), else 0
 *   hsp_small_pair_f32:   hsp_small_rows_f32 with w_layout 1 (out_nn (B, Nn) = alpha * gt (B, Ma) W (Ma, Nn)) and
 *                         hsp_small_outer_f32 (out_o (Ma, Nb) = gt^T c; mom / ldm / Cm / gste as there) as two block ranges of
 *                         one launch.  Ma a multiple of 128 and <= 2048, B <= 64; other shapes: HSP_ERR_UNSUPPORTED */
int hsp_colsum_cloud_ok(int B, int N, int C, int with_xyz);
int hsp_colsum_cloud_f32(const float *x, const float *xyz, int B, int N, int C, float *out, hspStream_t stream);
/* 1 where hsp_small_pair_f32 takes B per-cloud rows of Ma columns (B <= 64, Ma a multiple of 128 up to 2048) -- the function that
 * entry point itself declines by */
int hsp_small_pair_takes(int B, int Ma);
int hsp_small_pair_f32(const float *gt, int ldgt, int B, int Ma, const float *W, int ldw, int Nn, float alpha, float *out_nn,
                       int ldnn, const float *c, int ldc, int Nb, float *out_o, int ldo, const float *mom, int ldm, int Cm,
                       float *gste, hspStream_t stream);

/* ---- which of the kernels above takes a product call (host-only: no HIP call, no operand is dereferenced) ------------------
 * HspGemmCall (a HOST struct) describes a call of the hsp_gemm_rows_f32 contract: extents, layouts and pitches as there;
 * A2 == NULL: one source (K2 is ignored); resid == NULL: no residual; C == NULL: the caller allocates the result dense (ldc = N,
 * on 16 bytes); elem_bytes 4 | 2; bias / cloud_bias / xyz3 / relu: != 0 where the call has that rider; alpha_one: alpha == 1;
 * bn: the BatchNorm-partials form asked for (HSP_GEMM_BN_OUT: hsp_gemm_x3_bn_f32, HSP_GEMM_BN_LINEAR:
 * hsp_gemm_x3_bias_bn_f32); allow_x3 == 0 keeps the product off csrc/gemm_x3.hip's matrix-core kernels.
 *   hsp_gemm_takes(call, route): 1 where the entry point of that family runs the call -- the function that entry point itself
 *       returns HSP_ERR_UNSUPPORTED by (hsp_gemm_x3_supported / hsp_gemm_wave_supported are its shape-only clause) -- else 0
 *   hsp_gemm_route(call): the family the call goes to: the first of small rows, x3 (with the partials where bn asks for them
 *       and the kernel leaves them; else the route of the same call without), wave, tile that takes it AND is the faster
 *       choice for the shape (x3: M >= 256 and, with an epilogue, >= 128 tiles; wave: K1 + K2 <= 512, M N >= 512 K, clouds of
 *       >= 64 rows); HSP_GEMM_ROUTE_NONE where no kernel takes it */
#define HSP_GEMM_ROUTE_NONE 0
#define HSP_GEMM_ROUTE_SMALL_ROWS 1   /* hsp_small_rows_f32 */
#define HSP_GEMM_ROUTE_X3 2           /* hsp_gemm_x3_f32 */
#define HSP_GEMM_ROUTE_X3_BN 3        /* hsp_gemm_x3_bn_f32 / hsp_gemm_x3_bias_bn_f32, by HspGemmCall.bn */
#define HSP_GEMM_ROUTE_WAVE 4         /* hsp_gemm_wave_f32 (relu: cfg bit 29) */
#define HSP_GEMM_ROUTE_TILE 5         /* hsp_gemm_rows_f32 / hsp_gemm_rows_bf16 */
#define HSP_GEMM_BN_NONE 0
#define HSP_GEMM_BN_OUT 1
#define HSP_GEMM_BN_LINEAR 2
typedef struct HspGemmCall {
    const void *A1, *B1, *A2, *B2, *resid, *C;
    int M, N, K1, K2, b1_layout, b2_layout, elem_bytes;
    int lda1, ldb1, lda2, ldb2, ldr, ldc;
    int bias, cloud_bias, xyz3, relu, alpha_one, rows_per_cloud, bn, allow_x3;
} HspGemmCall;
int hsp_gemm_takes(const HspGemmCall *call, int route);
int hsp_gemm_route(const HspGemmCall *call);

/* fp32 master parameters -> bf16 working copies for the *_bf16 entry points, every tensor of a step in one launch:
 * entry e copies src (rows, cols; row pitch ld) to dst (rows, cols) and / or dstT (cols, rows) -- either may be NULL --
 * rounding to nearest even.  tile0 = number of 32 x 32 tiles of the entries before e; table_dev lives in DEVICE memory. */
typedef struct HspCastDesc { const float *src; void *dst; void *dstT; int rows, cols, ld, tile0; } HspCastDesc;
int hsp_cast_params_bf16(const HspCastDesc *table_dev, int n, int total_tiles, hspStream_t stream);
/* the same with row pitches for the copies (ldd for dst, lddT for dstT, in elements): 16-byte aligned rows for a K = 1286
 * weight (the heads' first layers on feat) */
typedef struct HspCastPitchedDesc {
    const float *src; void *dst; void *dstT; int rows, cols, ld, tile0, ldd, lddT;
} HspCastPitchedDesc;
int hsp_cast_params_pitched_bf16(const HspCastPitchedDesc *table_dev, int n, int total_tiles, hspStream_t stream);

/* ---- weight-gradient GEMM ---------------------------------------------------------------------
 * replaces the parameter-gradient matmuls autograd runs for `feature_map @ self.weights + self.bias`
 * (gcn3d.py:171) and the 1x1 Conv1d layers (gcn3d.py:85,149,186):
 *   C[m][n] = sum_k A[k][m]*B[k][n],  A (K,M) row stride lda, B (K,N) row stride ldb, C row stride ldc;
 *   colsum_B (N) = sum_k B[k][n] when non-NULL (the bias gradient).  K is the point-row count (deep),
 * M and N multiples of 64; split-K over independent waves on v_mfma_f32_32x32x2_f32, partials folded in
 * a fixed order (deterministic).  ws: hsp_wgrad_workspace_bytes(M,N,K).
 */
size_t hsp_wgrad_workspace_bytes(int M, int N, int K);
/* host-only: the form and the K cut of a weight-gradient call (every hsp_wgrad_* entry decides by the same function).
 * elem_bytes: 4 (the *_f32 entries) | 2 (*_bf16); aligned16: A and B both start on 16 bytes; lda / ldb in elements;
 * ragged_entry != 0: the hsp_wgrad_ragged_* entries.  out[4] = form, K slices, rows per slice (a multiple of 16; of 64 on the
 * matrix-core forms), partial sums in the workspace (slices / 4 on HSP_WGRAD_FORM_F32_KB4, else the slices);
 * partials * (M*N + N) * 4 <= hsp_wgrad_workspace_bytes(M, N, K).  Returns the HSP_ERR_UNSUPPORTED of the entry where it declines. */
#define HSP_WGRAD_FORM_F32_KB1 0   /* fp32 MFMA, a wave per (tile, slice) */
#define HSP_WGRAD_FORM_F32_KB4 1   /* fp32 MFMA, the 4 waves of a workgroup on 4 consecutive slices of one tile, folded in LDS */
#define HSP_WGRAD_FORM_BF16 2      /* bf16 rows on the bf16 MFMA (128 x 128 tiles) */
#define HSP_WGRAD_FORM_X3 3        /* fp32 rows as three bf16 slices on the bf16 MFMA */
int hsp_wgrad_plan(int M, int N, int K, int elem_bytes, int aligned16, int lda, int ldb, int ragged_entry, int *out);
/* host-only: the cut of hsp_wgrad_partial_pair_(colsum_)f32 for dense operands: out[7] = 1 where both problems share one launch
 * (both on HSP_WGRAD_FORM_F32_KB4; else 0, two hsp_wgrad_partial_f32 launches, see hsp_wgrad_plan, and the rest is 0), K slices and
 * rows per slice of problem 0, of problem 1 -- as launched, after the slices were lengthened to keep the pair inside one round of
 * 2 workgroups per CU --, workgroups of problem 0, of problem 1.  HSP_ERR_UNSUPPORTED: M or N off a multiple of 64. */
int hsp_wgrad_pair_plan(int M0, int N0, int K0, int M1, int N1, int K1, int *out);
/* split forms for a backward that computes several parameter gradients (an HS layer has three): hsp_wgrad_partial_* runs the
 * split-K launch only and describes the pending fold in *pending (a HOST struct; the workspace must stay alive and untouched
 * until the fold); hsp_wgrad_fold folds up to HSP_FOLD_MAX_WGRAD pending problems in ONE launch (same fixed order, same
 * results). */
#define HSP_FOLD_MAX_WGRAD 24
#define HSP_FOLD_MAX_DIRS 8
typedef struct HspWgradPending {
    const void *part, *cs_part;   /* split-K partials in the problem's workspace */
    void *C, *colsum;             /* outputs (colsum may be NULL) */
    int nparts, M, N, ldc;
} HspWgradPending;
int hsp_wgrad_fold(const HspWgradPending *pending, int n, hspStream_t stream);
/* the pending fold of a receptive-field layer's support-direction gradient (hsp_rf_*_bwd*_partial below): nparts per-cloud
 * partials (3, SC) in the call's workspace -> grad_dirs (3, SC) through the Jacobian of F.normalize(directions, dim=0)
 * (gcn3d.py:100,166).  A HOST struct; the workspace must stay alive and untouched until the fold. */
typedef struct HspDirsPending {
    const void *part, *dirs;      /* partials; the layer's RAW directions parameter (3, SC) */
    void *grad_dirs;              /* output (3, SC) */
    int nparts, SC;
} HspDirsPending;
/* every fold a backward pass left pending in ONE launch: nw <= HSP_FOLD_MAX_WGRAD parameter-gradient folds and
 * nd <= HSP_FOLD_MAX_DIRS direction-gradient folds (autograd of gcn3d.py:149,171,186 and :166 produce them; nothing before the
 * optimizer reads them).  Same summation order as the stand-alone folds: same bits. */
int hsp_step_fold(const HspWgradPending *wgrads, int nw, const HspDirsPending *dirs, int nd, hspStream_t stream);
/* hsp_rf_surface_bwd / hsp_rf_conv_bwd_scatter (and their bf16-storage twins) WITHOUT the direction-gradient fold: the tile
 * launch only; *pending describes the fold that hsp_step_fold runs later (grad_dirs is not valid until then). */
int hsp_rf_surface_bwd_partial(const float *xyz, const float *dirs, const uint16_t *argrow, const float *grad_out, int B, int N,
                               int S, int K, float *grad_dirs, void *ws, size_t ws_bytes, HspDirsPending *pending,
                               hspStream_t stream);
int hsp_rf_conv_bwd_scatter_partial(const float *xyz, const float *dirs, const float *fm, const float *fwin,
                                    const uint16_t *argrow, const float *grad_out, int B, int N, int S, int C, float *grad_fm,
                                    float *grad_dirs, void *ws, size_t ws_bytes, HspDirsPending *pending, hspStream_t stream);
int hsp_rf_surface_bwd_partial_bf16(const float *xyz, const float *dirs, const uint16_t *argrow, const hsp_bf16_t *grad_out,
                                    int B, int N, int S, int K, float *grad_dirs, void *ws, size_t ws_bytes,
                                    HspDirsPending *pending, hspStream_t stream);
int hsp_rf_conv_bwd_scatter_partial_bf16(const float *xyz, const float *dirs, const hsp_bf16_t *fm, const hsp_bf16_t *fwin,
                                         const uint16_t *argrow, const hsp_bf16_t *grad_out, int B, int N, int S, int C,
                                         hsp_bf16_t *grad_fm, float *grad_dirs, void *ws, size_t ws_bytes,
                                         HspDirsPending *pending, hspStream_t stream);
/* two pending weight gradients from ONE split-K launch (an HS layer's backward has two that depend only on the incoming
 * gradient and are each too small to fill the chip: g^T F and g^T X -- autograd of gcn3d.py:186 and :149); pending[2] */
int hsp_wgrad_partial_pair_f32(const float *A0, int lda0, const float *B0, int ldb0, int M0, int N0, int K0, float *C0, int ldc0,
                               void *ws0, size_t ws_bytes0, const float *A1, int lda1, const float *B1, int ldb1, int M1, int N1,
                               int K1, float *C1, int ldc1, void *ws1, size_t ws_bytes1, HspWgradPending *pending,
                               hspStream_t stream);
/* the same launch with out (B, C) = hsp_colsum_cloud_f32(x (B,N,C), NULL) riding in it, bit for bit: the head of the layer's
 * per-cloud backward chain depends on nothing the two products write.  The rider takes the resident workgroup slots the pair
 * leaves free.  HSP_ERR_UNSUPPORTED, with nothing launched, where the pair is not a single launch, hsp_colsum_cloud_ok(B, N, C, 0)
 * is 0 or the rider does not fit beside the pair: issue hsp_colsum_cloud_f32 and hsp_wgrad_partial_pair_f32 then. */
int hsp_wgrad_partial_pair_colsum_f32(const float *A0, int lda0, const float *B0, int ldb0, int M0, int N0, int K0, float *C0,
                                      int ldc0, void *ws0, size_t ws_bytes0, const float *A1, int lda1, const float *B1, int ldb1,
                                      int M1, int N1, int K1, float *C1, int ldc1, void *ws1, size_t ws_bytes1,
                                      HspWgradPending *pending, const float *x, int B, int N, int C, float *out,
                                      hspStream_t stream);
int hsp_wgrad_f32(const float *A, int lda, const float *B, int ldb, int M, int N, int K, float *C, int ldc,
                  float *colsum_B, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_wgrad_partial_f32(const float *A, int lda, const float *B, int ldb, int M, int N, int K, float *C, int ldc,
                          float *colsum_B, void *ws, size_t ws_bytes, HspWgradPending *pending, hspStream_t stream);

/* ---- BatchNorm1d (train mode) + ReLU over point rows -------------------------------------------
 * replaces F.relu(bn(x.transpose(1,2)).transpose(1,2))          FaceRecon.py:27-29, :90-95
 * x (R,C) point rows (R = B*N), batch statistics over R (biased variance for the normalisation, eps),
 * running_mean/var updated in place with `momentum` (unbiased variance) and *num_batches_tracked += 1
 * when the pointers are non-NULL -- nn.BatchNorm1d semantics.  y = relu ? max(0, bn(x)) : bn(x).
 * save_mean / save_invstd (C) feed the backward.  ws: hsp_bn_workspace_bytes(R, C) = [chunks][2][C] floats, chunks =
 * ceil(R / max(32, ceil(R / 512))) <= 512 row chunks.  The forward's statistics: every chunk sums (x - s) and (x - s)^2 with
 * s its OWN first row (read again from x by the fold, so the workspace holds no third row) and the chunks are merged as
 * (n, mean, M2) in a fixed order -- deterministic, and a row far from its column's mean costs no digits of the variance.
 */
/* 1 where the BatchNorm entry points below (hsp_bn_relu_fwd*, _apply*, _bwd*) take R rows of C channels: C a multiple of 4 with
 * C/4 | 256 -- the function those entry points themselves decline by */
int hsp_bn_takes(int R, int C);
size_t hsp_bn_workspace_bytes(int R, int C);
int hsp_bn_relu_fwd(const float *x, int R, int C, const float *gamma, const float *beta, float eps,
                    float momentum, int relu, float *y, float *save_mean, float *save_invstd,
                    float *running_mean, float *running_var, long long *num_batches_tracked, void *ws,
                    size_t ws_bytes, hspStream_t stream);
/* the affine + ReLU part alone with given statistics (eval mode: mean = running_mean,
 * invstd = 1/sqrt(running_var + eps)) */
int hsp_bn_relu_apply(const float *x, int R, int C, const float *mean, const float *invstd,
                      const float *gamma, const float *beta, int relu, float *y, hspStream_t stream);
/* dx (R,C), dgamma (C), dbeta (C) OVERWRITTEN; x is the forward INPUT (the ReLU mask is recomputed). */
int hsp_bn_relu_bwd(const float *x, const float *dy, int R, int C, const float *gamma, const float *beta,
                    const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma,
                    float *dbeta, void *ws, size_t ws_bytes, hspStream_t stream);
/* the same for a tensor with TWO consumers: dy rows of pitch ldy (>= C, even -- 8-byte aligned rows: a column block of a wider gradient
 * tensor, e.g. of a dense (B, N, 1286) one, is consumed in place) plus an optional second incoming gradient dy2 (pitch ldy2, NULL: none), added as they are read */
int hsp_bn_relu_fwd_partials(const float *x, int R, int C, const float *gamma, const float *beta, float eps, float momentum,
                             int relu, float *y, float *save_mean, float *save_invstd, float *running_mean, float *running_var,
                             long long *num_batches_tracked, const float *partial, int nblk, const float *shift,
                             hspStream_t stream);
int hsp_bn_relu_bwd2(const float *x, const float *dy, int ldy, const float *dy2, int ldy2, int R, int C, const float *gamma,
                     const float *beta, const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma,
                     float *dbeta, void *ws, size_t ws_bytes, hspStream_t stream);

/* ---- depth -> point cloud front end -------------------------------------------------------------
 * replaces the device work of PC_sample(obj_mask, Depth, camK, coor2d)    network/point_sample/pc_sample.py:8-77
 * mask (B,HW) fp32 (object mask, already arg-maxed if it was a 2-channel prediction), depth (B,HW).
 * hsp_pc_compact: pix (B,HW) int32 = ids of the pixels with mask*(depth>0) > 0 in row-major order (the order
 * of torch boolean indexing), count (B) int32.  The HOST then draws np.random.choice(count[b], S, replace =
 * count[b] < S) per image exactly like the reference (pc_sample.py:57-66) and
 * hsp_pc_gather back-projects the chosen pixels: pc (B,S,3) = ((u-cx)*d/fx, (v-cy)*d/fy, d) / 1000,
 * coor2d (B,2,HW), camK (B,3,3), choose (B,S) int32.
 */
size_t hsp_pc_compact_workspace_bytes(int B, int HW);   /* per-chunk counts of the two-launch compaction */
int hsp_pc_compact(const float *mask, const float *depth, int B, int HW, int32_t *pix, int32_t *count,
                   void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_pc_gather(const float *depth, const float *coor2d, const float *camK, const int32_t *pix,
                  const int32_t *choose, int B, int HW, int S, float *pc, hspStream_t stream);

/* dataset-side variant: replaces PoseDataset._depth_to_pcl(depth, K, xymap, mask) / 1000.0
 * datasets/load_data.py:322-333, :275 (numpy float64 arithmetic, fp32 result).  camK (B,9) DOUBLE, as the
 * loader holds it; mask/compaction via hsp_pc_compact; choose = the loader's _sample_points ids (:308-320). */
int hsp_depth_to_pcl(const float *depth, const float *xymap, const double *camK, const int32_t *pix,
                     const int32_t *choose, int B, int HW, int S, float *pc, hspStream_t stream);

/* ---- detections of a depth frame -> instance clouds -------------------------------------------------
 * replaces the crop chain of the evaluation loader, evaluation/load_data_eval.py:215-254: get_2d_coord_np (:215), three
 * crop_resize_by_warp_affine(..., INTER_NEAREST) over the frame (:231-243, tools/dataset_utils.py:80-93 with rot = 0), the two
 * validity sums (:246-252) and the boolean compaction inside _depth_to_pcl (:309-320); with inst_id also the training
 * loader's `mask == inst_id` (datasets/load_data.py:239-240).  The crops are never built: a nearest-neighbour warp of the coordinate
 * grid returns the coordinates of the pixel it sampled, so the three crops are views of one integer map from crop pixel
 * (u, v) (column, row) to frame pixel (X, Y), warpAffine's fixed-point form
 *     X = (rint(b1 * 1024) + 512 + rint(m0 * u * 1024)) >> 10,   Y = (rint(b2 * 1024) + 512 + rint(m0 * v * 1024)) >> 10
 * (rint: float64, half to even; >>: arithmetic; each rint term clamped to +-2^52), where xf (n,3) DOUBLE = (m0, b1, b2) is the
 * inverse of the forward matrix a = O / scale, tx = O/2 - a * cx, ty = O/2 - a * cy: D = 1 / (a * a), m0 = a * D, b1 = -m0 * tx,
 * b2 = -m0 * ty, computed by the host in float64.  (X, Y) outside the frame reads the constant border 0: never valid.
 * depth (H,W) fp32 (_f32) or 16-bit unsigned (_u16, what the PNG loader yields), H * W < 2^31; mask uint8 with an ELEMENT
 * stride per instance: H * W = one mask per instance (n,H,W), 0 = one label image shared by all.  inst_id (n) int32 or NULL:
 * a pixel belongs to instance j if mask == inst_id[j], with NULL if mask != 0.
 * src (n, O*O) int32 = frame pixel id Y * W + X of every crop pixel with depth > 0 and the mask set, in crop row-major order
 * (v, u); entries past the count are undefined; a source pixel sampled by several crop pixels (scale < O) appears once per crop
 * pixel, like in the reference.  count (n,2) int32 = [mask-and-depth valid, depth valid] (the loader's two rejection tests).
 * n <= 65535, O <= 46340. */
size_t hsp_roi_compact_workspace_bytes(int n, int O);   /* per-chunk count pairs of the two-launch compaction */
int hsp_roi_compact_f32(const float *depth, const uint8_t *mask, long long mask_stride, const int32_t *inst_id,
                        const double *xf, int n, int H, int W, int O, int32_t *src, int32_t *count, void *ws,
                        size_t ws_bytes, hspStream_t stream);
int hsp_roi_compact_u16(const uint16_t *depth, const uint8_t *mask, long long mask_stride, const int32_t *inst_id,
                        const double *xf, int n, int H, int W, int O, int32_t *src, int32_t *count, void *ws,
                        size_t ws_bytes, hspStream_t stream);
/* replaces _depth_to_pcl(roi_depth, out_camK, roi_coord_2d, roi_mask) / 1000.0 and the gather of _sample_points,
 * evaluation/load_data_eval.py:253-254, :294-320, on the frame itself: for p = src[j, choose[j,s]] the pixel coordinates are
 * u = float(p % W), v = float(p / W) (the float32 grid values the reference warps, exact), then hsp_depth_to_pcl's arithmetic.
 * camK (camK_rows, 9) DOUBLE with camK_rows = 1 (one camera for all) or n; src rows of pitch src_stride; choose (n,S) int32
 * -> pc (n,S,3) fp32 metres.  An index outside its src row or outside the frame gives NaN. */
int hsp_frame_to_pcl_f32(const float *depth, int H, int W, const double *camK, int camK_rows, const int32_t *src,
                         long long src_stride, const int32_t *choose, int n, int S, float *pc, hspStream_t stream);
int hsp_frame_to_pcl_u16(const uint16_t *depth, int H, int W, const double *camK, int camK_rows, const int32_t *src,
                         long long src_stride, const int32_t *choose, int n, int S, float *pc, hspStream_t stream);

/* ---- the rows each instance keeps, drawn on the device ----------------------------------------------
 * The opt-in counterpart of the host draws the three front ends above are fed by default (np.random.permutation /
 * np.random.choice on numpy's global generator, the reference's generator consumption): the same DISTRIBUTION from a keyed,
 * counter-based generator, not the same draws.  One launch, integer arithmetic only, no workspace, no atomics; the
 * back-projection entry points above consume its choose as they consume the host's.
 *
 * count: the counts of hsp_pc_compact (count_stride 1) or the pairs of hsp_roi_compact (count_stride 2), on the device.
 * key: DEVICE pointer to two uint64 {seed, call}; read by the kernel, so a captured launch sees the values of each replay.
 * choose (n,S) int32, status (n) int32.  n <= 65535, S >= 1, n * S < 2^31, count_stride 1 or 2, short_mode 0 or 1; anything
 * else is HSP_ERR_BAD_ARG before any launch.
 *
 * Per instance j, with c = count[j * count_stride]:
 *   status[j] = (c < min_pts ? 1 : 0) | (count_stride == 2 && count[j * 2 + 1] < min_depth_pts ? 2 : 0)
 *   status[j] != 0 or c <= 0:      choose[j,s] = -1 for every s (hsp_frame_to_pcl_* then writes NaN; hsp_pc_gather and
 *                                  hsp_depth_to_pcl must not be given such a row)
 *   short_mode 0 and c <= S:       choose[j,s] = s % c          (_sample_points: tiling when short, identity at c == S)
 *   short_mode 1 and c <  S:       choose[j,s] = (uint64(absorb(absorb(kj, 0xffffffff), s)) * c) >> 32     (with replacement)
 *   otherwise (c > S; c == S under short_mode 1):   choose[j,s] = P(s), the first S values of a permutation P of [0, c)
 *
 * All arithmetic below is on uint32 and wraps modulo 2^32.
 *   fmix32(h):     h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16       (murmur3's finaliser)
 *   absorb(h, w) = fmix32((h ^ w) + 0x9e3779b9)
 *   instance key:  kj = absorb(absorb(absorb(absorb(absorb(0, seed & 0xffffffff), seed >> 32), call & 0xffffffff), call >> 32), j)
 *   round keys:    k[r] = absorb(kj, r), r = 0..3
 *   width:         bits = 0 for c <= 1, else the number of bits of c - 1 (smallest with 2^bits >= c);
 *                  half = max(1, (bits + 1) / 2) (integer division), mask = 2^half - 1: a balanced Feistel network over
 *                  2 * half <= 32 bits, a domain of less than 4 c values for c >= 2
 *   one pass E(x): L = x >> half, R = x & mask;  for r = 0, 1, 2, 3 in this order:  t = L ^ (fmix32(R ^ k[r]) & mask), L = R, R = t;
 *                  E(x) = (L << half) | R
 *   P(s):          x = E(s);  while x >= c:  x = E(x)      (cycle walking: E is a bijection of [0, 2^(2 half)), so P is one of
 *                  [0, c) and the walk returns below c)
 * For c of a few units the 4 rounds reach only some of the c! orders; the sampler is meant for counts of tens to hundreds of
 * thousands of which about a thousand are kept. */
int hsp_sample_ids(const int32_t *count, int count_stride, int n, int S, int min_pts, int min_depth_pts, int short_mode,
                   const unsigned long long *key, int32_t *choose, int32_t *status, hspStream_t stream);

/* ---- the rows each instance keeps, picked by farthest-point sampling: no draw -------------------------
 * The third, opt-in way to fill choose / status between hsp_roi_compact_* and hsp_frame_to_pcl_*: a pure function of the frame,
 * the candidates and K -- no key, no generator.  (The loader's own docstring asks for it: evaluation/load_data_eval.py
 * _sample_points, "Down sample the point cloud using farthest point sampling", above a random permutation.)  One launch, one
 * workgroup per instance, plain C++ and vector stores, no atomics, no workspace, nothing read back; it can be captured.
 *
 * depth, H, W, camK (camK_rows, 9) DOUBLE, src rows of pitch src_stride: as hsp_frame_to_pcl_* takes them; count (n,2) int32: the
 * pairs of hsp_roi_compact_*, on the device; choose (n,S) int32, status (n) int32.  n <= 65535, S >= 1, n * S < 2^31,
 * H * W < 2^31, camK_rows 1 or n, src_stride >= 1, no NULL pointer; anything else is HSP_ERR_BAD_ARG before any launch.  Nothing
 * is declined by shape: there is no HSP_ERR_UNSUPPORTED.
 *
 * Per instance j, with c = count[2 j]:
 *   status[j] = (c < min_pts ? 1 : 0) | (count[2 j + 1] < min_depth_pts ? 2 : 0)            (hsp_sample_ids's at count_stride 2)
 *   status[j] != 0 or c <= 0:   choose[j,s] = -1 for every s
 *   c <= S:                     choose[j,s] = s % c                                          (the tiling of short_mode 0)
 *   otherwise:                  choose[j,s] = g(pick_s), with
 *     candidates   CAP = hsp_fps_ids_cap() = 12288, m = min(c, CAP); candidate t in [0, m) is the src entry g(t):
 *                  g(t) = t for c <= CAP, g(t) = (uint64(t) * c) / CAP (integer division) for c > CAP -- a strided thinning in
 *                  crop raster order, strictly increasing, g(0) = 0, g(CAP - 1) < c.  (A c beyond src_stride is the caller's
 *                  error; it is read as src_stride, so nothing past the row is touched.)
 *     coordinates  of candidate t: the three fp32 values hsp_frame_to_pcl_* writes for src[j, g(t)], bit for bit (one device
 *                  function serves both)
 *     picks        hsp_fps_levels_f32's rule on those coordinates: pick_0 = 0; every candidate keeps the running minimum of its
 *                  distance to the picked ones, fp32 (dx*dx + dy*dy) + dz*dz under a correctly rounded sqrt; the largest wins,
 *                  the lowest index among equals; A PICKED CANDIDATE IS NEVER PICKED AGAIN (it ranks below every unpicked one,
 *                  a zero distance included).  Exact ties are the normal case here -- whole millimetres on a pixel grid -- and
 *                  with fewer distinct points than S (a crop window smaller than the crop is up-sampled, so src names a source
 *                  pixel several times) the tail of the row is the lowest-index unpicked candidates.
 *                  (S > CAP with c > S leaves nothing unpicked after CAP picks: every later pick is candidate 0.)
 * A src entry outside the frame has NaN coordinates (hsp_frame_to_pcl_*'s rule) and a NaN distance never replaces a minimum;
 * hsp_roi_compact_* writes no such entry. */
int hsp_fps_ids_cap(void);     /* 12288: the most candidates one instance's pick chain ranks */
int hsp_fps_ids_f32(const float *depth, int H, int W, const double *camK, int camK_rows, const int32_t *src,
                    long long src_stride, const int32_t *count, int n, int S, int min_pts, int min_depth_pts, int32_t *choose,
                    int32_t *status, hspStream_t stream);
int hsp_fps_ids_u16(const uint16_t *depth, int H, int W, const double *camK, int camK_rows, const int32_t *src,
                    long long src_stride, const int32_t *count, int n, int S, int min_pts, int min_depth_pts, int32_t *choose,
                    int32_t *status, hspStream_t stream);

/* ---- instances followed from frame to frame: the crop decided by the last pose, no mask ---------------------
 * The opt-in front end of a video stream: where hsp_roi_compact_* cuts instance j out of the frame by a detector's mask and a
 * window the host made of the detector's box, these cut it by the pose and size the previous frame's replay left on the
 * device.  The oriented box of half extents h = (0.5 * pad) * size about the pose, projected with K, gives the window; the
 * same box in metres is the mask.  Nothing is read back: windows, flags and the tracked state live on the device.
 *
 * Arithmetic, all three entry points: float64, every operation named below is ONE rounding, in the order written (the
 * kernels spell them __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn, so no contraction moves a bit); a float32 input enters
 * by its exact conversion.  RT (n,16) fp32 row-major is a rigid pose in metres, what hsp_generate_rt writes: R = RT[0..2][0..2],
 * t = (RT[3], RT[7], RT[11]); the fourth row is not read.  size (n,3) fp32 metres.  camK (camK_rows, 9) DOUBLE with camK_rows
 * 1 (one camera for all) or n; K0, K2, K4, K5 are read.  pad finite and > 0.
 *
 * hsp_pose_windows: one launch, one lane per instance.  boxes (n,4) int32 = (x1, y1, x2, y2), xf (n,3) DOUBLE (the transform
 * rows hsp_roi_compact_* reads), wstatus (n) int32.  Per instance:
 *   half extents  h_i = (0.5 * pad) * double(size_i), i = 0, 1, 2
 *   corner k      k = 0..7, e_i = +h_i where bit i of k is set, -h_i where it is clear
 *                 X = ((R00 * e0 + R01 * e1) + R02 * e2) + t_x, Y and Z likewise with R's second and third row
 *                 u = (K0 * X) / Z + K2,   v = (K4 * Y) / Z + K5
 *   box           x1 = max(0, floor(min u)), y1 = max(0, floor(min v)), x2 = min(W - 1, ceil(max u)), y2 = min(H - 1, ceil(max v))
 *                 over the eight corners, clamped in float64 before the conversion to integer
 *   wstatus       4 ("no window") when any of R, t, size, K0, K2, K4, K5 or any u, v is not finite, any h_i <= 0, any corner
 *                 has Z <= 0, or x2 <= x1 or y2 <= y1 (a box off the frame ends here); boxes and xf of the instance are then
 *                 zeros.  0 otherwise.
 *   window        centre (cx, cy) = ((x1 + x2) / 2, (y1 + y2) / 2), scale s = max(x2 - x1, y2 - y1): the evaluation loader's rule
 *                 (evaluation/load_data_eval.py:221-228) without get_bbox's snapping to multiples of 40
 *   xf            a = O / s, tx = O / 2 - a * cx, ty = O / 2 - a * cy, D = 1 / (a * a), m0 = a * D, xf = (m0, -m0 * tx, -m0 * ty):
 *                 pc_sample.roi_transform's order, as hsp_dzi_windows has it on the device
 * n <= 65535, H, W >= 1, H * W < 2^31, 0 < O <= 46340.
 *
 * hsp_roi_compact_box_*: hsp_roi_compact_* with a geometric mask -- the same crop map, the same src (n, O*O) order, the same
 * count (n,2) = [inside-and-depth valid, depth valid], the same workspace (hsp_roi_compact_workspace_bytes), the same limits.
 * A crop pixel that maps to frame pixel p with depth > 0 is depth valid; it is inside iff, with (px, py, pz) the three fp32
 * values hsp_frame_to_pcl_* writes for p (one device function serves both: these are the values the network will see),
 *   q_i = ((R0i * px + R1i * py) + R2i * pz) - ((R0i * tx + R1i * ty) + R2i * tz)          (every product of two fp32 is exact)
 *   |q_i| <= h_i for i = 0, 1, 2, h as above; a NaN is never inside.
 * xf and wstatus are hsp_pose_windows's; wstatus may be NULL (no instance is flagged).  An instance with wstatus != 0 lists
 * nothing and counts (0, 0).
 *
 * hsp_track_update: the state a stream carries from one replay to the next, one launch.  Where status[j] == 0 the state takes
 * the new pose and size (words copied, not computed on) and lost[j] = 0; elsewhere the state stays as it is and lost[j] += 1.
 * rt_new (n,16) / size_new (n,3) / rt_state / size_state fp32, status / lost (n) int32; new and state must not overlap.
 *
 * Status bits of the chain: 1 and 2 are hsp_sample_ids's (hsp_fps_ids_*'s), 4 is wstatus's; the caller ORs them.
 * A NULL pointer (wstatus of hsp_roi_compact_box_* apart), a size out of range or a bad pad is HSP_ERR_BAD_ARG before any
 * launch; O > 46340 or n > 65535 in hsp_roi_compact_box_* is HSP_ERR_UNSUPPORTED and a short workspace HSP_ERR_WORKSPACE, as
 * in hsp_roi_compact_*. */
int hsp_pose_windows(const float *rt, const float *size, const double *camK, int camK_rows, int n, int H, int W, int O,
                     double pad, int32_t *boxes, double *xf, int32_t *wstatus, hspStream_t stream);
int hsp_roi_compact_box_f32(const float *depth, const float *rt, const float *size, double pad, const double *camK,
                            int camK_rows, const int32_t *wstatus, const double *xf, int n, int H, int W, int O, int32_t *src,
                            int32_t *count, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_roi_compact_box_u16(const uint16_t *depth, const float *rt, const float *size, double pad, const double *camK,
                            int camK_rows, const int32_t *wstatus, const double *xf, int n, int H, int W, int O, int32_t *src,
                            int32_t *count, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_track_update(const float *rt_new, const float *size_new, const int32_t *status, int n, float *rt_state,
                     float *size_state, int32_t *lost, hspStream_t stream);

/* ---- the training loader's front end: a batch of frames, the mask perturbed before the cloud is cut -------
 * replaces datasets/load_data.py:234-278 behind aug_bbox_DZI: the three nearest-neighbour crops, defor_2D
 * (datasets/data_augmentation.py:9-32) on the cropped mask, the three rejection tests (:254, :257, :276), _depth_to_pcl and the
 * gather of _sample_points.  Instance j of the batch has its own window xf[j] (the map and the transform of hsp_roi_compact),
 * its own mask and, with an element stride of H * W, its own frame; the crops are never built.  Four calls, queued in order:
 *   hsp_roi_defor -> hsp_crop_compact_* -> hsp_sample_ids(count, 2, ...) -> hsp_frames_to_pcl_*
 * Plain C++, vector stores, no atomics.  Every call: n <= 65535, O <= 46340, H * W < 2^31, a stride 0 or H * W; anything else
 * is HSP_ERR_BAD_ARG before any launch.
 *
 * THE MASK RULE (the definition; cv2 was never run against it).  m(u, v), u the column and v the row of the O x O crop, is 1
 * where the frame pixel the map gives for (u, v) carries the instance (mask == inst_id[j], with inst_id NULL mask != 0), and 0
 * where that pixel lies outside the frame (the warp's constant border).  With r = iters (1..8) and the footprint
 * T_r = {(i, j) : i, j >= 0, i + j <= r}:
 *   E(u, v) = AND of m(u - i, v - j) over T_r,   D(u, v) = OR of the same pixels,
 * both over the positions INSIDE THE CROP only (u - i >= 0, v - j >= 0): a position outside the crop is left out (erode's
 * +inf and dilate's -inf border), unlike a crop pixel whose source is outside the frame, which is there and reads 0.
 * band = (E != D); l = the number of band pixels.  T_1 is getStructuringElement(MORPH_ELLIPSE, (2, 2)) = [[0,1],[1,1]] with the
 * default anchor (1, 1), T_r its r-fold iteration.  The reference passes rand_r in cv2.erode's third positional argument, which
 * is dst, not iterations: it runs ONE iteration whatever FLAGS.roi_mask_r says, so iters = 1 is the reference's behaviour.
 * The draws are hsp_sample_ids's: key {seed, call} on the device, kj its instance key of j, absorb and P as defined there.
 *   gate:    the instance is deformed iff l >= 1 and uint64(absorb(absorb(kj, 0xfffffffe), 0)) < gate, gate in [0, 2^32]
 *            (= floor(rand_pro * 2^32) clipped; the reference deforms unless np.random.rand() > rand_pro)
 *   subset:  kd = absorb(kj, 0xfffffffd); P = the cycle-walked 4-round Feistel permutation of [0, l) with round keys
 *            absorb(kd, r), r = 0..3 (hsp_sample_ids's P with kd in place of kj and c = l).  The band pixel of row-major rank t
 *            among the band pixels becomes 0 iff P(t) < l / 2 (integer division), else 1; off the band the mask is unchanged.
 *            Exactly l / 2 zeros on a uniformly drawn subset: np.random.choice(l, l // 2, replace=False)'s DISTRIBUTION, not
 *            its draws.  (0xfffffffe / 0xfffffffd keep these apart from the row draws under absorb(kj, 0..3 | 0xffffffff).)
 * An instance that is not deformed keeps m.
 *
 * hsp_roi_defor: mask uint8 with an element stride per instance and inst_id as in hsp_roi_compact (H * W without ids: a mask
 * per instance; 0 with ids: one label image for all; H * W with ids: a label image per instance); xf (n,3) DOUBLE.
 * crop_mask (n, O*O) uint8: bit 0 = the mask after the rule, bit 1 = m.  band (n,2) int32 = [l, deformed ? 1 : 0].
 * iters outside 1..8 or gate > 2^32: HSP_ERR_BAD_ARG. */
size_t hsp_roi_defor_workspace_bytes(int n, int O);     /* per-chunk band counts of the two-launch form */
int hsp_roi_defor(const uint8_t *mask, long long mask_stride, const int32_t *inst_id, const double *xf, int n, int H, int W,
                  int O, int iters, unsigned long long gate, const unsigned long long *key, uint8_t *crop_mask,
                  int32_t *band, void *ws, size_t ws_bytes, hspStream_t stream);
/* hsp_roi_compact_* with the mask taken from crop_mask (crop space) and a depth_stride in ELEMENTS per instance: 0 = one frame
 * for all, H * W = a frame per instance (n,H,W).  src (n, O*O) and count (n,2) as hsp_roi_compact defines them with bit 0 as the
 * mask; src ids are relative to the instance's own frame.  pre (n) int32 = crop pixels with depth > 0 and bit 1: the loader's
 * roi_m_d_valid sum (:256-258), taken before the deformation. */
size_t hsp_crop_compact_workspace_bytes(int n, int O);  /* per-chunk count triples of the two-launch compaction */
int hsp_crop_compact_f32(const float *depth, long long depth_stride, const uint8_t *crop_mask, const double *xf, int n, int H,
                         int W, int O, int32_t *src, int32_t *count, int32_t *pre, void *ws, size_t ws_bytes,
                         hspStream_t stream);
int hsp_crop_compact_u16(const uint16_t *depth, long long depth_stride, const uint8_t *crop_mask, const double *xf, int n, int H,
                         int W, int O, int32_t *src, int32_t *count, int32_t *pre, void *ws, size_t ws_bytes,
                         hspStream_t stream);
/* hsp_frame_to_pcl_* with the same depth_stride: src[j, .] indexes the frame at depth + j * depth_stride. */
int hsp_frames_to_pcl_f32(const float *depth, long long depth_stride, int H, int W, const double *camK, int camK_rows,
                          const int32_t *src, long long src_stride, const int32_t *choose, int n, int S, float *pc,
                          hspStream_t stream);
int hsp_frames_to_pcl_u16(const uint16_t *depth, long long depth_stride, int H, int W, const double *camK, int camK_rows,
                          const int32_t *src, long long src_stride, const int32_t *choose, int n, int S, float *pc,
                          hspStream_t stream);

/* The kept items of a training batch: the loader answers a rejected item by moving on to the next index
 * (datasets/load_data.py:254-278), so a batch always holds its full number of good items.  Here the batch arrives with spares,
 * M >= keep items with the status of the chain above, and ONE launch picks the kept ones and gathers every per-item tensor:
 * no device->host copy, no counter shared between workgroups, plain vector stores, no arithmetic on the data.
 *
 * status (M) int32 on the device: non-zero = rejected (any bit counts, negative values included).  segs: a HOST array of nseg
 * segments, copied into the launch's arguments: src (M, row_bytes) and dst (keep, row_bytes) dense device rows that do not
 * overlap, fill NULL or one device row of row_bytes.  sel (keep) int32, info (2) int32.
 * 1 <= keep <= M <= HSP_BATCH_SELECT_MAX_ITEMS, 0 <= nseg <= HSP_BATCH_SELECT_MAX_SEGS (0: sel and info only), row_bytes a
 * positive multiple of 4, src / dst / fill 4-byte aligned; anything else -- also a NULL status, sel or info, a NULL src or dst in
 * a listed segment, a src that overlaps its dst -- is HSP_ERR_BAD_ARG before any launch.
 *
 * THE RULE.  V = the number of items with status 0, v_0 < v_1 < ... < v_{V-1} those items in ascending order.
 *   info = {V, min(V, keep)}
 *   V >= 1:  sel[j] = v_{j mod V}, j = 0 .. keep-1: the first keep good items in loader order; when the spares run out the good
 *            ones repeat in order.  No row of a rejected item is read into a dst.
 *   V == 0:  sel[j] = j.  A segment with a fill row gets that row in every dst row (the clouds: the network is never given the
 *            NaN rows of a rejected item); a segment without copies rows 0 .. keep-1.
 *   dst[j] = src[sel[j]] byte for byte (NaN payloads and integer rows pass unchanged).
 * Rows move 16 bytes at a time where row_bytes and both rows' addresses allow, else 4. */
#define HSP_BATCH_SELECT_MAX_SEGS 16
#define HSP_BATCH_SELECT_MAX_ITEMS 1024
typedef struct HspSelectSeg {
    const void *src;              /* (M, row_bytes) */
    void *dst;                    /* (keep, row_bytes) */
    const void *fill;             /* NULL, or the row every dst row gets when no item is good */
    long long row_bytes;
} HspSelectSeg;
int hsp_batch_select(const int32_t *status, int M, int keep, const HspSelectSeg *segs, int nseg, int32_t *sel, int32_t *info,
                     hspStream_t stream);

/* ---- pose matrix assembly -----------------------------------------------------------------------
 * replaces generate_RT([p_green,p_red],[f_green,f_red], T, 'vec', sym)     tools/geom_utils.py:232-244
 * (with to_R_matrices / get_vertical_rot_vec_in_batch / get_rot_mat_y_first, tools/rot_utils.py:39-100)
 * p_green, p_red (B,3) unit axes, f_green, f_red (B) confidences, T (B,3), sym (B, sym_stride) (column 0 == 1
 * zeroes the red confidence) -> out (B,4,4).
 */
int hsp_generate_rt(const float *p_green, const float *p_red, const float *f_green, const float *f_red,
                    const float *T, const float *sym, int sym_stride, int B, float *out, hspStream_t stream);

/* ---- optimizer step (training driver) ---------------------------------------------------------------
 * All parameters / gradients / optimizer state of a parameter group live in flat fp32 buffers; `rows` (device)
 * lists the dim-0 slices of every >= 2-D tensor (gc = 1: gradient centralisation applies) and chunks of the
 * 1-D tensors (gc = 0).
 * hsp_sumsq_f32: out[0] = sum x^2 (the squared total norm of torch.nn.utils.clip_grad_norm_, engine/train.py:99).
 * hsp_ranger_step replaces Ranger.step() tools/torch_utils/solver/ranger2020.py:135-246 for the whole group:
 *   clip (coef = min(1, max_norm / (sqrt(*gnorm_sq) + 1e-6)); gnorm_sq NULL = no clipping), gradient
 *   centralisation (before the moments, or with gc_after on the generalised gradient), RAdam moments,
 *   adaptive (N_sma > threshold, decided by the host from the step count) or plain momentum step with
 *   step_lr = step_size * lr, weight decay, and on lookahead steps slow += la_alpha * (p - slow); p = slow.
 */
typedef struct HspRowDesc { long long offset; int len; int gc; } HspRowDesc;
size_t hsp_sumsq_workspace_bytes(long long n);
int hsp_sumsq_f32(const float *x, long long n, float *out, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_ranger_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, float *slow,
                    const HspRowDesc *rows, int nrows, float beta1, float beta2, float eps, float weight_decay,
                    float step_lr, int adaptive, int lookahead, float la_alpha, int gc_after,
                    const float *gnorm_sq, float max_norm, hspStream_t stream);

/* ---- the step applied on the device's own decision (training step as one replay) --------------------
 * The two scalars hsp_ranger_step takes from the host per step -- step_lr and the adaptive / Lookahead switches -- come from
 * a device TABLE the host fills once, one HspStepEntry per applied step to come (Ranger's own doubles, rounded to fp32 once:
 * the bits the host path would have passed), and the decision whether a step is applied at all is made on the device by
 * hsp_step_gate.  Both launches take only pointers and constants, so they can be captured in a graph.
 *
 * HspStepEntry.flags: HSP_STEP_ADAPTIVE (N_sma > threshold), HSP_STEP_LOOKAHEAD (step % k == 0), HSP_STEP_FILL_SLOW (slow :=
 * the weights as they are BEFORE this step's update: the reference creates slow_buffer as a copy of the weights at the first
 * step, ranger2020.py:168-170).
 *
 * The control block `ctl`: HSP_STEP_CTL_SLOTS int32 on the device.
 *   slot 0  HSP_STEP_CTL_ARMED            written by the host only.  0: the gate answers "do not apply" and counts nothing
 *   slot 1  HSP_STEP_CTL_APPLY            the gate's answer for this replay, written by every gate launch
 *   slot 2  HSP_STEP_CTL_INDEX            the table entry of the step being applied (valid while apply == 1)
 *   slot 3  HSP_STEP_CTL_APPLIED          steps applied since the table was built
 *   slot 4  HSP_STEP_CTL_REPLAYS          armed gate launches
 *   slot 5  HSP_STEP_CTL_SKIPPED_NAN      of those, skipped for a NaN loss
 *   slot 6  HSP_STEP_CTL_SKIPPED_NO_ITEM  of those, skipped because no item of the batch was good
 *   slot 7  HSP_STEP_CTL_EXHAUSTED        1 once a step was refused because the table had no entry left
 *   slots 8-15: hsp_step_gate and hsp_ranger_step_gated never touch them.  Slots 8-11 belong to hsp_step_gate_accum (below),
 *   slots 12-15 are reserved: no launch writes them
 *
 * hsp_step_gate: one launch of one wave, one lane decides, rules in this order:
 *   1. armed == 0: apply = 0, nothing else changes
 *   2. replays += 1
 *   3. isnan(*total): apply = 0, skipped_nan += 1      (NaN only, like math.isnan in engine/train.py:91-95: +-inf is applied)
 *   4. else info != NULL and info[0] == 0: apply = 0, skipped_no_item += 1      (info: hsp_batch_select's [good items, ...])
 *   5. else applied >= horizon: apply = 0, exhausted = 1
 *   6. else apply = 1, index = applied, applied += 1
 * HSP_ERR_BAD_ARG: total or ctl NULL, horizon <= 0.
 *
 * hsp_ranger_step_gated: hsp_ranger_step whose every wave first reads ctl[HSP_STEP_CTL_APPLY]: 0 (or an index outside
 * [0, horizon)) and the wave returns having touched nothing; otherwise step_lr, adaptive and lookahead are those of
 * table[ctl[HSP_STEP_CTL_INDEX]], a HSP_STEP_FILL_SLOW entry copies each row's weights into slow first, and the update is
 * the very code of hsp_ranger_step (one kernel, built without fused multiply-adds: equal inputs give equal bits).
 * HSP_ERR_BAD_ARG: what hsp_ranger_step declines, table or ctl NULL, horizon <= 0.
 */
#define HSP_STEP_ADAPTIVE 1
#define HSP_STEP_LOOKAHEAD 2
#define HSP_STEP_FILL_SLOW 4
#define HSP_STEP_CTL_SLOTS 16
#define HSP_STEP_CTL_ARMED 0
#define HSP_STEP_CTL_APPLY 1
#define HSP_STEP_CTL_INDEX 2
#define HSP_STEP_CTL_APPLIED 3
#define HSP_STEP_CTL_REPLAYS 4
#define HSP_STEP_CTL_SKIPPED_NAN 5
#define HSP_STEP_CTL_SKIPPED_NO_ITEM 6
#define HSP_STEP_CTL_EXHAUSTED 7
typedef struct HspStepEntry { float step_lr; int32_t flags; } HspStepEntry;
int hsp_step_gate(const float *total, const int32_t *info, int32_t *ctl, int horizon, hspStream_t stream);
int hsp_ranger_step_gated(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, float *slow,
                          const HspRowDesc *rows, int nrows, float beta1, float beta2, float eps, float weight_decay,
                          float la_alpha, int gc_after, const float *gnorm_sq, float max_norm,
                          const HspStepEntry *table, const int32_t *ctl, int horizon, hspStream_t stream);

/* ---- gradient accumulation under the device's decision (FLAGS.accumulate, engine/train.py:99-114) ----
 * The reference steps when global_step % accumulate == 0 and otherwise only adds the batch's gradient to .grad; it runs
 * clip_grad_norm_ on the ACCUMULATED gradient after every backward, and a NaN loss skips the batch before its backward while
 * global_step still advances.  Here the fresh gradient of a replay lands in a buffer of its own and is added to the accumulator --
 * the `grads` buffer hsp_ranger_step_gated reads -- only when the gate took the slot.
 *
 * Further control slots (same block, same sixteen int32):
 *   slot 8   HSP_STEP_CTL_MICRO    the reference's global_step: set by the host when the block is built, += 1 by EVERY armed
 *                                  hsp_step_gate_accum launch, skipped and refused slots included
 *   slot 9   HSP_STEP_CTL_TAKE     this replay's fresh gradient enters the accumulator, written by every gate launch
 *   slot 10  HSP_STEP_CTL_FIRST    this take starts a fresh accumulator (valid while take == 1)
 *   slot 11  HSP_STEP_CTL_PENDING  micro-batches in the accumulator after this replay
 * While pending == 0 the contents of the accumulator and of the norm scalar mean nothing: no launch clears them after a step,
 * the next take has first == 1 and neither reads the accumulator nor the scalar.
 *
 * hsp_step_gate_accum: hsp_step_gate for accumulate >= 1 micro-batches per step.  One launch of one wave, one lane decides and
 * makes ALL state transitions; hsp_grad_accumulate and hsp_ranger_step_gated only read the block.  Rules in this order:
 *   1. armed == 0: take = 0, apply = 0, nothing else changes
 *   2. replays += 1; take = first = apply = 0
 *   3. isnan(*total): skipped_nan += 1                      (NaN only: +-inf is taken)
 *   4. else info != NULL and info[0] == 0: skipped_no_item += 1
 *   5. else applied >= horizon: exhausted = 1               (nothing taken, nothing applied)
 *   6. else take = 1, first = (pending == 0), pending += 1; and when micro % accumulate == 0: apply = 1, index = applied,
 *      applied += 1, pending = 0                            (micro = 0 steps on its own gradient alone: the reference's quirk)
 *   7. micro += 1                                           (after rules 3-6, whichever held)
 * A skipped stepping slot applies nothing, so the accumulator keeps growing until the next micro % accumulate == 0.
 * HSP_ERR_BAD_ARG: total or ctl NULL, horizon <= 0, accumulate <= 0.
 *
 * hsp_grad_accumulate: acc (n floats) takes in fresh (n floats), and norm_sq[0] becomes the squared norm of the result.
 *   - Every element: acc[i] = first ? 0.0f + fresh[i] : fl(fl(acc[i] * c) + fresh[i]).  Two roundings, multiply then add: the
 *     library is built with contraction off and no fused multiply-add may form here; the bits are those of scaling the
 *     accumulator in place and then adding to it.
 *   - c = min(1, max_norm / (sqrt(norm_sq[0]) + 1e-6)) (a NaN norm gives a NaN c), from the value norm_sq[0] holds when the call
 *     begins: the squared norm of the accumulator as the previous take left it.  This is the reference's in-place clip of an
 *     accumulate-only iteration, DEFERRED: the accumulator is not swept a second time to scale it, the coefficient stays pending
 *     in norm_sq beside it and is folded into the next take.  The stepping slot's hsp_ranger_step(_gated) applies the
 *     coefficient of the final norm itself, as it always has.  With first != 0 neither acc nor norm_sq is read.
 *   - norm_sq[0] is overwritten at the end of the call with the sum of squares of the new acc, accumulated in the same pass and
 *     by the same element -> lane -> partial -> fold mapping as hsp_sumsq_f32 (one device function instantiated by both): it is
 *     bit-equal to hsp_sumsq_f32 run over acc afterwards.
 *   - ctl NULL: `first` is the argument and the call always takes.  ctl given (the block hsp_step_gate_accum wrote): every
 *     workgroup reads take and first from it and the argument is ignored; with take == 0 acc and norm_sq are left untouched.
 *   - acc and fresh must not overlap and both need 16-byte alignment (else HSP_ERR_UNSUPPORTED); ws / ws_bytes as for
 *     hsp_sumsq_f32 (hsp_sumsq_workspace_bytes(n), else HSP_ERR_WORKSPACE).  Ordinary vector loads and stores, no atomics.
 *   - 12 B per element (8 B with first).  HSP_ERR_BAD_ARG: acc, fresh or norm_sq NULL, n <= 0.
 */
#define HSP_STEP_CTL_MICRO 8
#define HSP_STEP_CTL_TAKE 9
#define HSP_STEP_CTL_FIRST 10
#define HSP_STEP_CTL_PENDING 11
int hsp_step_gate_accum(const float *total, const int32_t *info, int32_t *ctl, int horizon, int accumulate,
                        hspStream_t stream);
int hsp_grad_accumulate(float *acc, const float *fresh, long long n, float *norm_sq, float max_norm, int first,
                        const int32_t *ctl, void *ws, size_t ws_bytes, hspStream_t stream);

/* ---- Chamfer distance -------------------------------------------------------------------------
 * replaces cd.forward_cuda / cd.backward_cuda    tools/pyTorchChamferDistance/chamfer_distance.cpp:27-56
 * xyz1 (B,n,3), xyz2 (B,m,3) -> dist1 (B,n), dist2 (B,m) squared NN distances, idx1/idx2 int32 arg-min
 * (first minimum wins, chamfer_distance.cpp:78).  bwd: gx1/gx2 OVERWRITTEN with +-2g(p-q) sums
 * (chamfer_distance.cpp:141-175).
 */
int hsp_chamfer_fwd(const float *xyz1, const float *xyz2, int B, int n, int m, float *dist1, float *dist2,
                    int32_t *idx1, int32_t *idx2, hspStream_t stream);
int hsp_chamfer_bwd(const float *xyz1, const float *xyz2, const int32_t *idx1, const int32_t *idx2,
                    const float *gd1, const float *gd2, int B, int n, int m, float *gx1, float *gx2,
                    hspStream_t stream);

/* ---- Chamfer distance: ordered backward, and the reconstruction term of the training step ----------------------
 * (not in the reference.)  hsp_chamfer_bwd sums with float atomics into pre-zeroed outputs; the forms below write every
 * output row once, from one fp32 sum in a stated order, so two runs give equal bits.
 *
 * hsp_chamfer_bwd_ordered: hsp_chamfer_bwd's contract (any n, m; per-point gd1 (B,n), gd2 (B,m)) and its arithmetic term by
 * term -- g = 2 gd, v = g * (p - q), each operation rounded once --, summed per output row as
 *     gx1[b,i] = 2 gd1[i] (x1_i - x2_idx1[i])  -  2 gd2[j] (x2_j - x1_i)   for the j with idx2[j] == i, j ASCENDING,
 * own term first, one subtraction per j; gx2 likewise over idx1.  The lists of the rows that chose a row are
 * hsp_rev_build(idx, k = 1) -- one launch for both maps -- and one more launch writes the rows; no memset.  gx1 or gx2
 * (not both) may be NULL: not wanted.  idx1 / idx2 are device data in [0, m) / [0, n) and are not range-checked.
 * ws: hsp_chamfer_bwd_ordered_workspace_bytes(B, n, m) (the two reverse maps).
 * hsp_chamfer_bwd_ordered_ok(B, n, m): 1 where the entry takes the call -- clouds the reverse build holds
 * (hsp_rev_build_takes(n) and (m): n, m <= 35 839) and B <= 65 535 --, the function the entry itself declines by; it is the
 * limit of hsp_recon_chamfer_bwd as well, at n = m = N.
 * A NULL pointer (but one of gx1 / gx2), B, n, m <= 0, ws NULL or short: HSP_ERR_BAD_ARG; a call beyond _ok:
 * HSP_ERR_UNSUPPORTED; nothing is launched in either case.
 *
 * hsp_recon_chamfer_fwd: the term 'Prop_sym_cd' (config.FLAGS.prop_sym_cd_w) between the reconstruction P = recon (B,N,3) and
 * the target G (B,N,3) of the loss kernels' Prop_sym_recon -- the observed cloud PC (B,N,3) turned 180 degrees about the
 * object's y axis (sym[b] = [1, *] with a mirror flag set), mirrored in z ([0, 1, *]) or taken as is ([0, != 1, *]) under the
 * ground-truth pose gt_R (B,3,3), gt_t (B,3); the rule is csrc/sym_target.h's, one copy for both -- as SETS:
 *     d1[b,i] = min_j |G[b,j] - P[b,i]|^2,   d2[b,j] = min_i |P[b,i] - G[b,j]|^2,
 *     term[0] = (w * S) / (float)(B N),      S = sum of d1 and d2 over the batch.
 * Distances are hsp_chamfer_fwd's expression: candidate minus query, (dx dx + dy dy) + dz dz, each operation rounded once,
 * strict '<', so idx1 / idx2 (B,N) are the FIRST minima (defined on the exact ties of a tiled cloud).  A cloud with
 * sym[b] = [1, 0, 0, 0] ("skip") is left out: G[b] = 0, its distances 0, its arg-mins 0, nothing searched.
 * Two launches for any (B, N): the first searches both directions (G is made while the candidates are staged through LDS in
 * chunks of 2048 points, and written out by the workgroups that hold it as queries) and leaves d1 (B,N) | d2 (B,N) in ws, in
 * that order; the second is one workgroup of 1024 threads that sums the 2 B N floats of ws in the order
 *     acc_t = ((0 + ws[t]) + ws[t + 1024]) + ...            for thread t,
 *     acc_t += acc_(t + h)   for t < h,   h = 512, 256, ..., 1,        S = acc_0,
 * fixed by (B, N) alone.  G, idx1, idx2 are outputs the backward (and a test) reads; term is a device scalar.
 * ws: hsp_recon_chamfer_fwd_workspace_bytes(B, N) = 8 B N.  Any N >= 1; B <= 65 535 (HSP_ERR_UNSUPPORTED beyond).
 *
 * hsp_recon_chamfer_bwd: d term / d recon of that call, hsp_chamfer_bwd_ordered specialised to it: gd = (g[0] * w) / (B N)
 * for every point, g the device scalar arriving at the term, gx (B,N,3) only (G is a constant):
 *     gx[b,i] = (2 gd) * [ (P_i - G_idx1[i]) + (P_i - G_j) for the j with idx2[j] == i, j ASCENDING ],
 * the bracket summed in fp32 in that order, scaled once at the end; the rows of a skip cloud are written as zeros.  One
 * hsp_rev_build launch and one more.  ws: hsp_recon_chamfer_bwd_workspace_bytes(B, N).
 * Both: a NULL pointer, B, N <= 0, w not finite, ws NULL or short: HSP_ERR_BAD_ARG, nothing launched.
 */
int hsp_chamfer_bwd_ordered_ok(int B, int n, int m);
size_t hsp_chamfer_bwd_ordered_workspace_bytes(int B, int n, int m);
int hsp_chamfer_bwd_ordered(const float *xyz1, const float *xyz2, const int32_t *idx1, const int32_t *idx2,
                            const float *gd1, const float *gd2, int B, int n, int m, float *gx1, float *gx2, void *ws,
                            size_t ws_bytes, hspStream_t stream);
size_t hsp_recon_chamfer_fwd_workspace_bytes(int B, int N);
int hsp_recon_chamfer_fwd(const float *PC, const float *gt_R, const float *gt_t, const float *sym, const float *recon, int B,
                          int N, float w, float *term, float *G, int32_t *idx1, int32_t *idx2, void *ws, size_t ws_bytes,
                          hspStream_t stream);
size_t hsp_recon_chamfer_bwd_workspace_bytes(int B, int N);
int hsp_recon_chamfer_bwd(const float *recon, const float *G, const int32_t *idx1, const int32_t *idx2, const float *sym,
                          const float *g, int B, int N, float w, float *gx, void *ws, size_t ws_bytes, hspStream_t stream);

/* ---- farthest point sampling -----------------------------------------------------------------
 * replaces farthest_point_sampling(points, n)         tools/eval_utils.py:107-119 (per cloud)
 * xyz (B,N,3) -> sel (B,n_samples): start at 0, running min of the Euclidean distances, first maximum wins.
 * The arithmetic follows the dtype the numpy helper is called with (eval_utils.py:73-84):
 *   hsp_fps_f32 -- a float32 cloud: (x*x + y*y) + z*z and a correctly rounded sqrt, all in fp32;
 *   hsp_fps_f64 -- a float64 cloud (what tools/eval_utils.py:122-140 passes): the same in fp64.
 * The sqrt is part of the contract: it creates exact ties that the first-maximum rule resolves by index.
 * ws: hsp_fps_workspace_bytes(B,N) for f32, twice that for f64.
 */
size_t hsp_fps_workspace_bytes(int B, int N);
int hsp_fps_f32(const float *xyz, int B, int N, int n_samples, int32_t *sel, void *ws, size_t ws_bytes,
                hspStream_t stream);
int hsp_fps_f64(const double *xyz, int B, int N, int n_samples, int32_t *sel, void *ws, size_t ws_bytes,
                hspStream_t stream);
/* The LEVELS form: the sampler of gcn3d.Pool_layer(sampler="fps") for both Pool_layers of the stack in one launch.
 * xyz (B,N0,3) -> sel1 (B,N1) int32, the rows hsp_fps_f32's rule picks (fp32, (x*x + y*y) + z*z, correctly rounded sqrt, running
 * minimum of the distance to the picked set, start at row 0, first maximum wins) with ONE rule added: A PICKED ROW IS NEVER PICKED
 * AGAIN -- its distance-to-set ranks below every unpicked row's, a zero included.  On a cloud whose picks are all distinct under
 * hsp_fps_f32 the picks are hsp_fps_f32's, bit for bit; on a cloud with fewer distinct points than picks (a short crop tiled up to
 * N0 rows), where hsp_fps_f32 returns row 0 over and over, the remaining picks are the lowest-index unpicked rows, so sel1 always
 * names N1 different rows.  v1 (B,N1,3) = xyz[b, sel1[b]] in pick order.  Farthest-point picks are nested: the same sampler run on
 * v1 returns 0 .. N2-1, so the second level is a prefix, and v2 (B,N2,3) = v1[:, :N2] is written here as well (N2 == 0: v2 may be
 * NULL).  0 < N1 <= N0, 0 <= N2 <= N1.  N0 > 12288 (beyond the register-resident kernel): HSP_ERR_UNSUPPORTED, nothing launched. */
/* 1 where hsp_fps_levels_f32 takes a cloud of N0 points (the register-resident kernel: N0 <= 12 288) -- the function that entry
 * point itself declines by */
int hsp_fps_levels_takes(int N0);
int hsp_fps_levels_f32(const float *xyz, int B, int N0, int N1, int N2, int32_t *sel1, float *v1, float *v2,
                       hspStream_t stream);

/* ---- bf16 feature storage (BASELINE configs[3]: dense clouds, bf16 features / weights / fm / gradients) -----------
 * Twins of the entry points above for feature tensors stored as bfloat16 (hsp_bf16_t = the upper 16 bits of an fp32).
 * Same argument roles and semantics; every kernel still computes in fp32 (loads widen, stores round to nearest even).
 * What stays fp32: xyz, support directions and theta (the reference hard-casts them with .float(), gcn3d.py:57,59),
 * arg-max / index tensors, BatchNorm statistics and affine parameters, every parameter gradient, per-cloud (B,C) rows
 * (ORL global feature and its gradient).  The fp32 master parameters are rounded once per step by hsp_cast_params_bf16.
 * hsp_knn_bf16: inner products on v_mfma_f32_32x32x16_bf16 (exact products, fp32 accumulation), |x|^2 in fp32, the fp32
 * path's distance expression and selection rule; C % 32 == 0.  ws: B*N*4 bytes.
 */
int hsp_knn_bf16(const hsp_bf16_t *x, int B, int N, int C, int k, int drop_first, int32_t *idx, void *ws,
                 size_t ws_bytes, hspStream_t stream);
int hsp_rf_surface_fwd_bf16(const float *xyz, const int32_t *idx, const float *dirs, int B, int N, int k, int S, int K,
                            hsp_bf16_t *out, uint16_t *argrow, hspStream_t stream);
int hsp_rf_surface_bwd_bf16(const float *xyz, const float *dirs, const uint16_t *argrow, const hsp_bf16_t *grad_out, int B,
                            int N, int S, int K, float *grad_dirs, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_rf_conv_wants_fwin_bf16(int N, int S, int C);
int hsp_rf_conv_fwd_bf16(const float *xyz, const int32_t *idx, const float *dirs, const hsp_bf16_t *fm, int B, int N, int k,
                         int S, int C, hsp_bf16_t *out, uint16_t *argrow, hsp_bf16_t *fwin, hspStream_t stream);
int hsp_rf_conv_bwd_scatter_bf16(const float *xyz, const float *dirs, const hsp_bf16_t *fm, const hsp_bf16_t *fwin,
                                 const uint16_t *argrow, const hsp_bf16_t *grad_out, int B, int N, int S, int C,
                                 hsp_bf16_t *grad_fm, float *grad_dirs, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_gather_max_fwd_bf16(const hsp_bf16_t *feat, const int32_t *idx, const int32_t *qsel, int B, int Nsrc, int Nidx,
                            int Nq, int k, int kstride, int C, hsp_bf16_t *out, uint8_t *argmax, hspStream_t stream);
/* grad_out: (B,Nq,C) bf16, or with grad_bcast != 0 the fp32 (B,C) per-cloud row; LDS tile form only */
int hsp_gather_max_bwd_bf16(const void *grad_out, int grad_bcast, const int32_t *idx, const int32_t *qsel,
                            const uint8_t *argmax, int B, int Nsrc, int Nidx, int Nq, int kstride, int C,
                            hsp_bf16_t *grad_feat, int accumulate, const hsp_bf16_t *extra, hspStream_t stream);
int hsp_gather_max_fwd_sel_bf16(const hsp_bf16_t *feat, const int32_t *idx, const int32_t *qsel, int qsel_stride, int B, int Nsrc,
                                int Nidx, int Nq, int k, int kstride, int C, hsp_bf16_t *out, uint8_t *argmax, hspStream_t stream);
int hsp_gather_max_bwd_sel_bf16(const void *grad_out, int grad_bcast, const int32_t *idx, const int32_t *qsel, int qsel_stride,
                                const uint8_t *argmax, int B, int Nsrc, int Nidx, int Nq, int kstride, int C,
                                hsp_bf16_t *grad_feat, int accumulate, const hsp_bf16_t *extra, hspStream_t stream);
int hsp_orl_global_fwd_bf16(const hsp_bf16_t *feat, const int32_t *idx, int B, int N, int k, int kstride, int C, float *fg,
                            uint8_t *argmax, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_colsum_rows_bf16(const hsp_bf16_t *x, int B, int N, int C, float *out, void *ws, size_t ws_bytes,
                         hspStream_t stream);
/* out_pitch: row pitch of out in elements (>= sum of widths; padding columns are zeroed when every segment is 16-byte
 * aligned -- the feat assembly -- and left untouched otherwise).  Three forms, the same copy in each: 16-BYTE chunks where
 * out_pitch, the address of out and every kind 0 / 1 segment's width, first column and source address are multiples of 16 bytes
 * (kind 2 / 3 segments of any width: they only move the columns after them) -- the one form that writes the padding, ALL
 * out_pitch - sum of widths columns of every row, with zeros; element PAIRS where the same holds for two elements; SCALARS
 * otherwise.  nseg outside 1 .. 8, a NULL source, a width <= 0, a kind outside 0 .. 3, a kind 1 segment without idx, or
 * out_pitch below the sum of the widths: HSP_ERR_BAD_ARG.  A kind 3 id is truncated toward zero ((long) id == column); an id
 * outside [0, width) gives an all-zero segment.  bf16 form: kind 0 / 1
 * sources are bf16, kind 2 (per-cloud rows) and kind 3 (the (B) float
 * category ids, expanded to one-hot columns in place) fp32 */
int hsp_concat_rows_pitched(int nseg, const float *const *src, const int32_t *const *idx, const int *width, const int *kind,
                            const int *nsrc, int B, int N, float *out, int out_pitch, hspStream_t stream);
int hsp_concat_rows_bf16(int nseg, const void *const *src, const int32_t *const *idx, const int *width, const int *kind,
                         const int *nsrc, int B, int N, hsp_bf16_t *out, int out_pitch, hspStream_t stream);
int hsp_gather_rows_bwd_csr_bf16(const hsp_bf16_t *grad_out, int grad_stride, const int32_t *rev_off,
                                 const int32_t *rev_edge, int B, int Nsrc, int Nq, int C, hsp_bf16_t *grad_feat,
                                 hspStream_t stream);
int hsp_gather_rows_bwd_csr_multi_bf16(int nseg, const hsp_bf16_t *const *grad_out, int grad_stride,
                                       const int32_t *const *rev_off, const int32_t *const *rev_edge, int B, const int *Nsrc,
                                       int Nq, const int *C, hsp_bf16_t *const *grad_feat, hspStream_t stream);
int hsp_wgrad_bf16(const hsp_bf16_t *A, int lda, const hsp_bf16_t *B, int ldb, int M, int N, int K, float *C, int ldc,
                   float *colsum_B, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_wgrad_partial_bf16(const hsp_bf16_t *A, int lda, const hsp_bf16_t *B, int ldb, int M, int N, int K, float *C, int ldc,
                           float *colsum_B, void *ws, size_t ws_bytes, HspWgradPending *pending, hspStream_t stream);
/* ragged M (not a multiple of 64; N a multiple of 128): A's rows on a 16-byte pitch >= ceil8(M), e.g. the 1286 columns of feat
 * on its 1288 pitch.  Other shapes as hsp_wgrad_bf16; same workspace rule (hsp_wgrad_workspace_bytes) and fold */
int hsp_wgrad_ragged_bf16(const hsp_bf16_t *A, int lda, const hsp_bf16_t *B, int ldb, int M, int N, int K, float *C, int ldc,
                          float *colsum_B, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_wgrad_ragged_partial_bf16(const hsp_bf16_t *A, int lda, const hsp_bf16_t *B, int ldb, int M, int N, int K, float *C,
                                  int ldc, float *colsum_B, void *ws, size_t ws_bytes, HspWgradPending *pending,
                                  hspStream_t stream);
/* hsp_gemm_rows_bf16 with an fp32 residual (no bias / cloud bias / xyz3): C = A1 B1^T (+ A2 B2^T) + resid, C fp32 (c_is_f32)
 * or bf16 -- a sum over more than two products carried in fp32 and rounded once */
int hsp_gemm_rows_acc_bf16(const hsp_bf16_t *A1, int lda1, const hsp_bf16_t *B1, int ldb1, int K1, const hsp_bf16_t *A2,
                           int lda2, const hsp_bf16_t *B2, int ldb2, int K2, int M, int N, const float *resid, int ldr, void *C,
                           int ldc, int c_is_f32, void *ws, size_t ws_bytes, hspStream_t stream);
/* bf16 product with the BatchNorm first pass in its epilogue: C (fp32) = A B^T + bias (+ cloud_bias[row / rows_per_cloud])
 * (+ xyz3 . w3), bn_shift[n] = bias[n] + cloud_bias[0][n], bn_part[tiles][2][N] = per row tile sum (c - shift), sum (c - shift)^2
 * (the layout of hsp_gemm_x3_bias_bn_f32), tiles = hsp_gemm_rows_bn_tiles_bf16(M, N, K), which is 0 where the fold cannot take
 * that many (more than 512) and the entry point declines; fold with
 * hsp_bn_relu_fwd_partials_mixed (bf16 rows out) or hsp_bn_relu_fwd_partials */
int hsp_gemm_rows_bn_tiles_bf16(int M, int N, int K);
int hsp_gemm_rows_bn_bf16(const hsp_bf16_t *A, int lda, const hsp_bf16_t *B, int ldb, int K, int M, int N, const float *bias,
                          const float *cloud_bias, int rows_per_cloud, const float *xyz3, const float *w3, float *C, int ldc,
                          float *bn_shift, float *bn_part, hspStream_t stream);
int hsp_bn_relu_fwd_partials_mixed(const float *x, int R, int C, const float *gamma, const float *beta, float eps, float momentum,
                                   int relu, hsp_bf16_t *y, float *save_mean, float *save_invstd, float *running_mean,
                                   float *running_var, long long *num_batches_tracked, const float *partial, int nblk,
                                   const float *shift, hspStream_t stream);
/* (B,N,C) bf16 rows -> fp32 (B,C) max and winning row (the fp32 kernel's rule on the widened values); backward: bf16 (B,N,C) */
int hsp_points_max_fwd_bf16(const hsp_bf16_t *x, int B, int N, int C, float *out, int32_t *argrow, hspStream_t stream);
int hsp_points_max_bwd_bf16(const float *grad_out, const int32_t *argrow, int B, int N, int C, hsp_bf16_t *grad_x,
                            hspStream_t stream);
/* "mixed": x fp32 (the pre-BatchNorm layer output is kept in fp32: with |mean| >> std per channel a bf16 x would leave
 * the normalised value only a few significant bits), y / dy / dx bf16 */
int hsp_bn_relu_fwd_mixed(const float *x, int R, int C, const float *gamma, const float *beta, float eps, float momentum,
                          int relu, hsp_bf16_t *y, float *save_mean, float *save_invstd, float *running_mean,
                          float *running_var, long long *num_batches_tracked, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_bn_relu_apply_mixed(const float *x, int R, int C, const float *mean, const float *invstd, const float *gamma,
                            const float *beta, int relu, hsp_bf16_t *y, hspStream_t stream);
int hsp_bn_relu_bwd_mixed(const float *x, const hsp_bf16_t *dy, int R, int C, const float *gamma, const float *beta,
                          const float *save_mean, const float *save_invstd, int relu, hsp_bf16_t *dx, float *dgamma,
                          float *dbeta, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_bn_relu_fwd_bf16(const hsp_bf16_t *x, int R, int C, const float *gamma, const float *beta, float eps, float momentum,
                         int relu, hsp_bf16_t *y, float *save_mean, float *save_invstd, float *running_mean,
                         float *running_var, long long *num_batches_tracked, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_bn_relu_apply_bf16(const hsp_bf16_t *x, int R, int C, const float *mean, const float *invstd, const float *gamma,
                           const float *beta, int relu, hsp_bf16_t *y, hspStream_t stream);
int hsp_bn_relu_bwd_bf16(const hsp_bf16_t *x, const hsp_bf16_t *dy, int R, int C, const float *gamma, const float *beta,
                         const float *save_mean, const float *save_invstd, int relu, hsp_bf16_t *dx, float *dgamma,
                         float *dbeta, void *ws, size_t ws_bytes, hspStream_t stream);

/* ---- training losses of the PoseNet_only stage -----------------------------------------------------------
 * replaces, for one batch, the four loss modules as network/HSPose.py:84-160 wires them:
 *   fs_net_loss          losses/fs_net_loss.py:95-235      Rot1 Rot1_cos Rot2 Rot2_cos Rot_r_a Tran Size R_con
 *   recon_6face_loss     losses/recon_loss.py:464-649      recon_per_p recon_p_f recon_point_{vote,r,t,s,self}
 *   geo_transform_loss   losses/geometry_loss.py:123-150   geo_point
 *   prop_rot_loss        losses/prop_loss.py:156-276       Prop_pm Prop_sym_recon Prop_sym_rt
 * terms (19) in that order, each already multiplied by its FLAGS weight.  PC (B,N,3), gt_R (B,3,3), gt_t / gt_s /
 * mean_shape (B,3), sym (B,4), obj_id (B) fp32; network outputs recon (B,N,3), face_normal (B,N,6,3), face_dis / face_f
 * (B,N,6) in the network's face order (y+ x+ z+ x- z- y-), p_green / p_red / pred_T / pred_s (B,3), f_green / f_red (B).
 * The axis confidences are variables only in R_con and the face confidences only in recon_p_f (HSPose.py detaches them
 * elsewhere).  `cfg` is a HOST struct.  The workspace written by _fwd is read by _bwd (keep it until then).
 * _bwd: grad_terms (19) = d(objective)/d(term); every d_* buffer is OVERWRITTEN with the gradient w.r.t. that network output;
 * d_mom_scratch: B*54 doubles.  Five launches in all; sums in a fixed order (bit-reproducible). */
#define HSP_LOSS_TERMS 19
typedef struct HspLossCfg {       /* config/config.py:64-93 */
    float rot_1_w, rot_2_w, rot_regular, tran_w, size_w, r_con_w;
    float recon_n_w, recon_d_w, recon_f_w, recon_v_w, recon_bb_r_w, recon_bb_t_w, recon_bb_s_w, recon_bb_self_w;
    float geo_p_w, prop_pm_w, prop_sym_w;
    int smooth_l1;                /* fsnet_loss_type: 0 = 'l1', 1 = 'smoothl1' (beta 0.5) */
} HspLossCfg;
size_t hsp_pose_losses_workspace_bytes(int B);
int hsp_pose_losses_fwd(const float *PC, const float *gt_R, const float *gt_t, const float *gt_s, const float *mean_shape,
                        const float *sym, const float *obj_id, const float *recon, const float *face_normal,
                        const float *face_dis, const float *face_f, const float *p_green, const float *p_red,
                        const float *f_green, const float *f_red, const float *pred_T, const float *pred_s, int B, int N,
                        const HspLossCfg *cfg, float *terms, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_pose_losses_bwd(const float *PC, const float *gt_R, const float *gt_t, const float *gt_s, const float *mean_shape,
                        const float *sym, const float *obj_id, const float *recon, const float *face_normal,
                        const float *face_dis, const float *face_f, const float *p_green, const float *p_red,
                        const float *f_green, const float *f_red, const float *pred_T, const float *pred_s, int B, int N,
                        const HspLossCfg *cfg, const float *grad_terms, const void *ws, size_t ws_bytes,
                        double *d_mom_scratch, float *d_recon, float *d_face_normal, float *d_face_dis, float *d_face_f,
                        float *d_green, float *d_red, float *d_f_green, float *d_f_red, float *d_T, float *d_s,
                        hspStream_t stream);

/* replaces HSPose.data_augment                          network/HSPose.py:185-256 over
 *          defor_3D_bb_in_batch / _rt_in_batch / _bc_in_batch / defor_3D_pc   datasets/data_augmentation.py:70-190
 * one launch for a training batch: box scaling in the object frame (aug_bb; x and z share the mean factor under rotational
 * symmetry), rigid perturbation (aug_rt_t, aug_rt_r), box-cage taper for bowls (1) / mugs (5) with the size taken from the
 * tapered model's extent * nocs_scale, per-point radial jitter noise * (p - t).  Each applies to the clouds whose draw is
 * below its probability.  draws (6,B): u_bb, u_rt, u_bc, ey_up, ey_down (uniforms in [0,1), mapped to [0.8,1.2)), u_pc -- the
 * caller draws them in the reference's order; noise (B,N,3) = rand * FLAGS.aug_pc_r (the reference's CPU draw, uploaded).
 * PC (B,N,3), model_point (B,M,3); gt_s / s_out are size residuals to mean_shape.  Outputs may not alias the inputs. */
int hsp_pose_augment(const float *PC, const float *gt_R, const float *gt_t, const float *gt_s, const float *mean_shape,
                     const float *sym, const float *aug_bb, const float *aug_rt_t, const float *aug_rt_r,
                     const float *model_point, const float *nocs_scale, const float *obj_id, const float *draws,
                     const float *noise, int B, int N, int M, float p_bb, float p_rt, float p_bc, float p_pc, float *PC_out,
                     float *R_out, float *t_out, float *s_out, hspStream_t stream);

/* ---- keyed draws of a step: every random choice of a forward or a replay, made on the device ----------------------------
 * The opt-in counterpart (config.FLAGS.step_draws = 'device') of what the host draws before a forward or a replay: the rows the
 * two Pool_layers keep (torch.randperm on the CPU generator, gcn3d.py:243), the augmentation's six per-item uniforms and its
 * jitter factors (torch.rand), the training loader's DZI windows (numpy's generator).  The same DISTRIBUTIONS from the keyed
 * generator of the hsp_sample_ids section, not the same draws.  Plain C++, vector stores, integer arithmetic for the draws, no
 * atomics, no workspace.  key: the DEVICE pointer to two uint64 {seed, call} that hsp_sample_ids reads, so a captured launch
 * sees each replay's values; one {seed, call} pair keys every draw of one forward or replay.
 *
 * fmix32, absorb, the instance key kj of an index j and the cycle-walked Feistel permutation P of [0, c) under a key are those
 * of the hsp_sample_ids section, unchanged.  Each purpose has instance indices j >= 2^31 of its own, so no stream coincides with
 * a row draw (there j < 65536) or with another purpose:
 *   Pool rows of level l (0 or 1):     j = 0x80000000 | l
 *   augmentation of cloud b:           j = 0x81000000 | b        (b < 2^24)
 *   DZI window of item i:              j = 0x82000000 | i        (i < 65535)
 *   Dropout of site s:                 j = 0x83000000 | s        (s < 2^24)
 *   scene of item i:                   j = 0x84000000 | i        (i < 2^24; section "scenes drawn under a step's key")
 *   model points of item i:            j = 0x85000000 | i        (i < 2^24; the same section)
 * A stream of words under kj and a tag T is  word(i) = absorb(absorb(kj, T), i), i = 0, 1, ... (uint32).
 * A word w becomes an fp32 uniform as  float(w >> 8) * 2^-24  and a float64 uniform as  double(w) * 2^-32: both conversions are
 * exact and give values in [0, 1).
 *
 * hsp_pool_rows_draw: the kept rows of `levels` (1 or 2) consecutive Pool_layers of pooling rate `rate`, ONE launch.  n_0 = n0,
 * level l keeps m_l = n_l / rate rows (integer division: the reference's int(n / rate)) of n_l, and n_1 = m_0.  With
 * kl = the instance key of j = 0x80000000 | l and P_l = P over [0, n_l) under kl (round keys absorb(kl, r), c = n_l):
 *   rows[off_l + s] = P_l(s),  s = 0 .. m_l - 1,   off_0 = 0, off_1 = m_0
 * -- the first m_l values of a permutation: an ordered subset drawn uniformly, shared by the batch like the reference's single
 * randperm.  rows (m_0 [+ m_1]) int32, back to back.  n0 <= 0, rate <= 0, levels outside {1, 2} or an m_l of 0: HSP_ERR_BAD_ARG. */
int hsp_pool_rows_draw(const unsigned long long *key, int n0, int rate, int levels, int32_t *rows, hspStream_t stream);

/* hsp_pose_augment with its draws made in the kernel (the same kernel body): `draws` and `noise` give way to key and aug_pc_r.
 * For cloud b, kb = the instance key of j = 0x81000000 | b and word(i) = absorb(absorb(kb, 0xfffffffc), i):
 *   draws[q, b]     = the fp32 uniform of word(q), q = 0 .. 5        (u_bb, u_rt, u_bc, ey_up, ey_down, u_pc in this order)
 *   noise[b, n, i]  = the fp32 uniform of word(6 + 3 n + i), times aug_pc_r in fp32 (one rounding, as the host's rand * r)
 * and everything else is hsp_pose_augment's, operation for operation: given these draws and this noise hsp_pose_augment returns
 * the same bits.  B <= 2^24, N <= 2^29; beyond, a NULL pointer or a size <= 0: HSP_ERR_BAD_ARG. */
int hsp_pose_augment_keyed(const float *PC, const float *gt_R, const float *gt_t, const float *gt_s, const float *mean_shape,
                           const float *sym, const float *aug_bb, const float *aug_rt_t, const float *aug_rt_r,
                           const float *model_point, const float *nocs_scale, const float *obj_id,
                           const unsigned long long *key, float aug_pc_r, int B, int N, int M, float p_bb, float p_rt,
                           float p_bc, float p_pc, float *PC_out, float *R_out, float *t_out, float *s_out, hspStream_t stream);

/* replaces aug_bbox_DZI with DZI_TYPE 'uniform' (tools/dataset_utils.py:24-61) and the crop transform behind it for the M items
 * of a training batch: bboxes (M,4) int32 = (x1, y1, x2, y2) on the device -> xf (M,3) DOUBLE = (m0, b1, b2), the rows
 * hsp_roi_compact / hsp_roi_defor / hsp_crop_compact read.  For item i, ki = the instance key of j = 0x82000000 | i,
 * word(q) = absorb(absorb(ki, 0xfffffffb), q), and u0, u1, u2 = the float64 uniforms of word(0), word(1), word(2) (the
 * reference's random_sample(), then random_sample(2)).  All in float64, every operation rounded once (nothing contracted into a
 * fused multiply-add), in this order; integers convert exactly:
 *   cx = 0.5 * (x1 + x2),  cy = 0.5 * (y1 + y2),  bw = x2 - x1,  bh = y2 - y1
 *   sr = 1 + scale_ratio * (2 * u0 - 1),   sx = shift_ratio * (2 * u1 - 1),   sy = shift_ratio * (2 * u2 - 1)
 *   cx' = cx + bw * sx,   cy' = cy + bh * sy
 *   scale = min((max(bh, bw) * sr) * pad_scale, max(H, W))
 *   O = out_size;  a = O / scale;  tx = O / 2 - a * cx';  ty = O / 2 - a * cy';  D = 1 / (a * a);  m0 = a * D
 *   xf[i] = (m0, (-m0) * tx, (-m0) * ty)
 * A box with max(bh, bw) <= 0 gives a row that is not finite (the host form refuses it); the caller keeps such boxes out.
 * 'roi10d' / 'truncnorm' are not built.  M outside 1..65535, H, W <= 0, out_size outside 1..46340, pad_scale <= 0, scale_ratio
 * outside [0, 1), shift_ratio < 0 or a value that is not finite: HSP_ERR_BAD_ARG. */
int hsp_dzi_windows(const int32_t *bboxes, const unsigned long long *key, int M, int H, int W, int out_size, double pad_scale,
                    double scale_ratio, double shift_ratio, double *xf, hspStream_t stream);

/* Keyed Dropout (config.FLAGS.reproducible under device draws): the heads' nn.Dropout (PoseR.py:27, PoseTs.py) with its mask drawn
 * from the step's key instead of torch's device generator, whose Philox offset is part of neither the key nor the checkpoint.
 * x, out (R,C) fp32, keep (R,C) uint8.  For site s (Rot_green 0, Rot_red 1, Pose_Ts 2), ks = the instance key of
 * j = 0x83000000 | s, word(i) = absorb(absorb(ks, 0xfffffffa), i) with i = r * C + c, u = the fp32 uniform of word(i):
 *   keep[r,c] = u >= p;   out[r,c] = keep ? x[r,c] * scale : 0,   scale = 1.0f / (1.0f - p) computed once on the host in fp32
 * -- the same distribution as nn.Dropout(p) in training mode (P(keep) = 1 - p to 2^-24), not the same draws.  p outside [0, 1),
 * site outside [0, 2^24), R * C >= 2^32, a NULL pointer or a size <= 0: HSP_ERR_BAD_ARG.
 * hsp_dropout_bwd: grad_x = grad_out * keep * scale from the SAVED mask (scale from p as above); it never re-derives the mask
 * from the key, so an eager caller may run two forwards before a backward. */
int hsp_dropout_keyed_fwd(const float *x, const unsigned long long *key, int site, float p, int R, int C, float *out,
                          uint8_t *keep, hspStream_t stream);
int hsp_dropout_bwd(const float *grad_out, const uint8_t *keep, float p, int R, int C, float *grad_x, hspStream_t stream);

/* the face head's output split (PoseNet9D.py:31-35) in one launch each way: face (R, 30) -> unit normals (R, 6, 3) =
 * face[:, :18] / its per-face 3-norm (no epsilon, as the reference), distances (R, 6) = face[:, 18:24], confidences (R, 6) =
 * sigmoid(face[:, 24:]); backward: g_face (R, 30) from the three incoming gradients (each may be NULL = zero). */
int hsp_face_split_fwd(const float *face, long long R, float *normals, float *dis, float *conf, hspStream_t stream);
int hsp_face_split_bwd(const float *face, const float *g_normals, const float *g_dis, const float *g_conf, long long R,
                       float *g_face, hspStream_t stream);

/* a rotation head's output split (PoseNet9D.py:40-46): h (B, 4) -> axis (B, 3) = h[:, 1:] / (||h[:, 1:]|| + 1e-6), confidence (B) =
 * sigmoid(h[:, 0]); backward: g_h (B, 4) from g_axis / g_conf (each may be NULL = zero). */
int hsp_axis_conf_fwd(const float *h, int B, float *axis, float *conf, hspStream_t stream);
int hsp_axis_conf_bwd(const float *h, const float *g_axis, const float *g_conf, int B, float *g_h, hspStream_t stream);

/* ---- evaluation metrics: 3D IoU, degree / cm matching, average precision ---------------------------------------------------
 * replaces compute_degree_cm_mAP (evaluation/eval_utils_v1.py:430-621) and what it calls, quirks included, in three stages.
 *
 * A GROUP is the predictions and the ground truths of one class in one image.  The caller lays the instances out so that a group's
 * predictions are consecutive rows of pred_RT (.,4,4) / pred_scale (.,3) / scores, its ground truths consecutive rows of gt_RT /
 * gt_scale / gt_handle, both in the image's own order, and the groups of one class follow each other in image order: a class's
 * rows are then its concatenation across images.  groups (n_groups, 6) int32 on the device, one row per group:
 *   {p_off, np, g_off, ng, pair_off, kind}
 * p_off / g_off: first prediction / ground-truth row; np, ng <= hsp_eval_group_cap() (32: the pair table of a group is then 20 KB
 * of LDS); pair_off: where the group's np * ng pair values start ([i * ng + j], i and j in the image's order); kind: 0 no
 * symmetry, 1 bottle / bowl / can, 2 mug, 3 phone / eggbox / glue.  Images with neither predictions nor ground truths have no
 * group (:485-486).  max_group is the caller's statement of the largest np or ng in the table, which lives on the device: above the
 * cap every entry point returns HSP_ERR_UNSUPPORTED before any launch.  pred_bboxes is not an input (the reference only asserts
 * on it).  All arithmetic is fp64 unless stated; no atomics; every output slot has one writer.
 *
 * hsp_eval_pairs: compute_3d_iou_new (:35-91) and compute_RT_degree_cm_symmetry (:94-167), one pair per lane.
 *   iou: the eight corners of get_3d_bbox(scale) through RT, divided by the homogeneous row; then the reference's extremes, which
 *   are np.amax / np.amin(axis=0) of a (3, 8) array (:47-50): the largest and smallest COORDINATE of each corner, eight intervals
 *   in get_3d_bbox's corner order, not a box per axis -- kept, because that is the number everyone quotes.  Overlap interval c =
 *   [max of the two minima, min of the two maxima]; intersection = the product of the eight overlap lengths, 0 where one is
 *   negative; volumes = the products of the eight lengths; intersection / union.  For kind 1, and kind 2 where gt_handle == 0 (kinds other than 2
 *   never read gt_handle: the reference forces it to 1, :509-513): the largest of that over pred_RT . Ry(2 pi i / 20), i = 0..19,
 *   starting from 0.  Stored rounded to fp32 (the reference's float32 overlap table); a disjoint pair is exactly 0.
 *   degree: both rotations divided by cbrt(det); for the symmetric pairs above the angle between the two y axes, otherwise
 *   arccos((trace(R1 R2^T) - 1) / 2), for kind 3 the smaller of that and the same with R1 diag(-1, 1, -1); times 180 / pi.  The
 *   arccos argument is NOT clamped: above 1 it gives NaN, as numpy does.  shift: |T1 - T2| * 100.
 *
 * hsp_eval_match: compute_3d_matches (:252-327) and compute_match_from_degree_cm (:385-427), one workgroup per group, one lane per
 * threshold running the sequential greedy loop.
 *   order (slots) int8: a group's predictions in the reference's argsort(scores)[::-1] -- descending score, equal scores by the
 *   HIGHER original index first (numpy's stable ascending order, reversed; what its argsort gives for groups this small) --,
 *   order[p_off + pos] = the group-local index of the prediction at position pos; score_sorted: its score.
 *   IoU stage, for each of the T_iou thresholds (iou_thres holds them rounded to fp32, numpy >= 2's comparison of a float32 with
 *   a Python float): predictions by position; each one's ground truths by argsort(iou_row)[::-1] (equal values by the higher index
 *   first); matched ones skipped; STOP at the first iou < thres; match only on iou > thres.  iou_pred_match (slots, T_iou) int8:
 *   [p_off + pos][t] = the matched ground truth's group-local index or -1; iou_gt_match (gt rows, T_iou): [g_off + j][t] = the
 *   position of the matched prediction or -1.  (The tables are slot-major so that the lanes of a group store side by side.)
 *   Pose stage: with pose_iou_index >= 0 (use_matches_for_pose) only the predictions and ground truths matched at that IoU
 *   threshold take part, in their kept order; with -1 all do.  kept (n_groups, 2) int32 = how many of each.  For each of the
 *   D1 x S1 thresholds (the lists with 360 and 100 appended by the caller; t = d * S1 + s): kept predictions by position, each
 *   one's kept ground truths by ascending degree + shift (equal sums by the lower index, NaN last), matched ones skipped, pairs
 *   with degree > deg_thres[d] or shift > shift_thres[s] skipped (`continue`: a NaN compares false and passes), the first one left
 *   is taken.  pose_pred_match (slots, D1 * S1), pose_gt_match (gt rows, D1 * S1): as above with positions in the KEPT lists; a
 *   group's slots past its kept count hold -1.  pose_score (slots): the kept predictions' scores, 0 past the kept count.
 *
 * hsp_eval_ap: compute_ap_from_matches_scores (:330-356), one workgroup per (class, threshold), and the mean row.
 *   match (slots, T) int8 as written above; order (.) int32: slot numbers, class c's in [seg_off[c], seg_off[c + 1]) (seg_off
 *   (C + 1) int32 on the device) by DESCENDING score, equal scores by ascending slot (the reference's order among equal scores of
 *   different images is unspecified); the sort is the caller's (a stable device sort).  gt_count (C) int32 on the device: the
 *   class's ground-truth entries -- for the pose table those the IoU filter kept.  Per class and threshold: matched > -1, running
 *   count, precision count / (i + 1) in fp64, recall count / G in FP32, the sentinels, the running maximum of the precision from
 *   the right, and the sum of (recall step) * precision over the points where the recall moves, added in numpy's pairwise order
 *   (np.sum's: eight interleaved partial sums per block of up to 128 terms, blocks joined by halves, pieces of 8192 terms added
 *   up in order), so the result is the
 *   reference's bit for bit.  No predictions: 0.  Predictions but G == 0: NaN (numpy's 0 / 0).  aps (C + 2, T) fp64: row 0 (BG)
 *   = 0, row c + 1 = class c, the last row = np.mean(aps[1:-1], axis=0) (a NaN class makes it NaN): for T > 1 the class rows added
 *   in row order, for T == 1 -- one contiguous run -- in np.sum's order above.  The row order is
 *   np.mean's order for fewer than 8 classes; from 8 classes on the reference's pose mean, taken over a strided 1-D slice, adds
 *   pairwise and may differ from this row in the last bit (its IoU mean, taken along axis 0, never does).
 *   ws: hsp_eval_ap_workspace_bytes(slots, T, C) = 8 T (slots + C), the terms of every (class, threshold).
 *   slots >= 2^23: HSP_ERR_UNSUPPORTED (fp32 recalls of neighbouring counts must differ).
 *
 * All three: a NULL pointer, a size <= 0, pose_iou_index >= T_iou: HSP_ERR_BAD_ARG; nothing is launched on any refusal. */
int hsp_eval_group_cap(void);
int hsp_eval_pairs(const double *pred_RT, const double *pred_scale, const double *gt_RT, const double *gt_scale,
                   const int32_t *gt_handle, const int32_t *groups, int n_groups, int max_group, float *iou, double *degree,
                   double *shift, hspStream_t stream);
int hsp_eval_match(const int32_t *groups, int n_groups, int max_group, const double *scores, const float *iou,
                   const double *degree, const double *shift, const float *iou_thres, int T_iou, const double *deg_thres, int D1,
                   const double *shift_thres, int S1, int pose_iou_index, int8_t *order, double *score_sorted,
                   int8_t *iou_pred_match, int8_t *iou_gt_match, int8_t *pose_pred_match, int8_t *pose_gt_match,
                   double *pose_score, int32_t *kept, hspStream_t stream);
size_t hsp_eval_ap_workspace_bytes(int slots, int T, int C);
int hsp_eval_ap(const int8_t *match, int slots, int T, const int32_t *order, const int32_t *seg_off, const int32_t *gt_count,
                int C, double *aps, void *ws, size_t ws_bytes, hspStream_t stream);

/* ---- depth frames rendered from meshes and poses ------------------------------------------------------------
 * A z-buffered triangle rasteriser: n instances of triangle meshes, each under its own pose and per-axis scale, drawn into F
 * frames in the formats the front ends above read -- depth in millimetres (uint16, or fp32) and a uint8 label image.  The
 * reference has no counterpart: its synthetic frames are rendered off line and read from files.  Nothing is uploaded and
 * nothing is read back; every call can be captured.
 *
 * Data.  verts (V,3) fp32 in model units; tris (T,3) int32, indices relative to the first vertex of their mesh;
 * mesh (n_mesh,4) int32 = (first vertex, vertex count, first triangle, triangle count), every row inside verts and tris.
 * Instance j of n draws mesh mesh_id[j] into frame frame_id[j] in [0, F) under label label[j] in [1, 255]; its pose is rt[j]
 * (16 fp32 row-major, what hsp_generate_rt writes; the fourth row is not read), its scale[j] 3 fp32, the metres per model
 * unit along each axis.  camK (camK_rows, 9) DOUBLE with camK_rows 1 (one camera for all) or F (one per frame); K0, K2, K4, K5
 * are read.  depth (F,H,W), labels (F,H,W).
 *
 * Arithmetic: float64, every operation named below is ONE rounding, in the order written (the kernels spell them
 * __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn); a float32 input enters by its exact conversion.
 *   vertex      m_i = double(scale_i) * double(v_i), i = 0, 1, 2
 *               X = ((R00 * m0 + R01 * m1) + R02 * m2) + t_x, Y and Z likewise with R's second and third row
 *               u = (K0 * X) / Z + K2,   v = (K4 * Y) / Z + K5
 *               a vertex is recomputed for every triangle that names it: the same operations on the same inputs, the same bits
 *   drop        a triangle is dropped if a vertex has Z <= 0 or a u, v or Z that is not finite.  THERE IS NO CLIPPING: a
 *               triangle that crosses the camera plane is not drawn at all.
 *   samples     the integer pixel coordinates (px, py): the grid hsp_frame_to_pcl_* back-projects, so a rendered pixel's
 *               point lies on the ray it was sampled on
 *   edges       for k = 0, 1, 2: c = vertex k of the row, a and b the other two with index a < index b (a repeated index
 *               drops the triangle);  e_k(q) = (u_b - u_a) * (q_y - v_a) - (v_b - v_a) * (q_x - u_a),  A_k = e_k(P_c);
 *               A_k == 0 or not finite drops the triangle.  Two triangles that share an edge evaluate the same e there.
 *   candidates  the pixels of the frame with floor(min u) <= px <= ceil(max u) and floor(min v) <= py <= ceil(max v) over the
 *               three vertices (min, max, floor and ceil are exact; in exact arithmetic no pixel outside them is inside)
 *   inside      a candidate with, for all three k, e_k(p) >= 0 where A_k > 0 and e_k(p) <= 0 where A_k < 0: edges are
 *               inclusive and both facings are drawn
 *   depth       l_k = e_k(p) / A_k,  inv = (l0 / Z0 + l1 / Z1) + l2 / Z2,  Z = ((l0 + l1) + l2) / inv,  zmm = Z * 1000
 *   word        _u16: q = rint(zmm), half to even; the fragment is kept iff 1 <= q <= 65535, its word is q
 *               _f32: f = (float) zmm; kept iff f is finite and > 0, its word is the bit pattern of f
 *   visibility  per pixel the smallest 64-bit key (word << 32) | j over the kept fragments of its frame wins: the nearest
 *               surface, and among equal depth words the lower instance index.  over == 0: a pixel no fragment reaches gets
 *               depth 0 and label 0.  over == 1: an existing pixel with depth > 0 (fp32: finite and > 0) enters with the key
 *               (its word << 32) | 0xFFFFFFFF and keeps its label where it wins -- a rendered surface at the same word goes in
 *               front of it --, any other existing pixel counts as empty and is written as depth 0, label 0.
 * The frames are a pure function of the inputs: a minimum does not depend on the order the fragments arrive in.
 *
 * hsp_label_boxes: boxes[j] = (x1, y1, x2, y2) int32 with x1, y1 the least column and row of frame frame_id[j] whose label is
 * label[j] and x2, y2 the greatest column and row PLUS ONE (the exclusive convention of the annotations the training loader
 * reads, what hsp_dzi_windows takes; get_bbox's snapping to multiples of 40 is not applied); count[j] (n) int32 the number of
 * such pixels.  No such pixel, or a frame_id / label out of range: zeros and a count of 0.  Integer min, max and add only.
 *
 * Limits: 0 <= n <= 65535 (hsp_label_boxes: n >= 1), F, H, W >= 1, H * W < 2^31, over 0 or 1, camK_rows 1 or F, V, T, n_mesh
 * >= 1; with n == 0 the instance and mesh pointers are not read (they may be NULL) and the frames are cleared, or with over
 * left as they are (empty pixels written as zeros).  A NULL pointer or a size out of range is HSP_ERR_BAD_ARG before any launch;
 * ws NULL, off a 16-byte boundary or below hsp_render_workspace_bytes(F, H, W, n) (0 for sizes out of range) is
 * HSP_ERR_WORKSPACE.  On the device a mesh_id, frame_id or label out of range, or a mesh row that leaves verts or tris, makes
 * that instance draw nothing and a vertex index outside its mesh drops the triangle: nothing is read out of bounds.  (The
 * host checks the indices of a mesh set once, when it is built.) */
size_t hsp_render_workspace_bytes(int F, int H, int W, int n);
int hsp_render_depth_u16(const float *verts, int V, const int32_t *tris, int T, const int32_t *mesh, int n_mesh,
                         const int32_t *mesh_id, const int32_t *frame_id, const int32_t *label, const float *rt,
                         const float *scale, const double *camK, int camK_rows, int n, int F, int H, int W, int over,
                         uint16_t *depth, uint8_t *labels, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_render_depth_f32(const float *verts, int V, const int32_t *tris, int T, const int32_t *mesh, int n_mesh,
                         const int32_t *mesh_id, const int32_t *frame_id, const int32_t *label, const float *rt,
                         const float *scale, const double *camK, int camK_rows, int n, int F, int H, int W, int over,
                         float *depth, uint8_t *labels, void *ws, size_t ws_bytes, hspStream_t stream);
int hsp_label_boxes(const uint8_t *labels, const int32_t *frame_id, const int32_t *label, int n, int F, int H, int W,
                    int32_t *boxes, int32_t *count, hspStream_t stream);

/* ---- scenes drawn under a step's key --------------------------------------------------------------------------------------
 * The last host draw of a synthetic training step, made on the device: the poses, sizes, ground truth and augmentation rows of M
 * items and of D distractors per item (hsp_scene_draw) and the items' model points (hsp_mesh_sample), as keyed draws of the
 * step -- the rules of that section hold: plain C++, vector stores, uint32 arithmetic for the draws, no atomics, no workspace,
 * every output slot has one writer, key the DEVICE pointer to {seed, call}.  The same DISTRIBUTIONS as render.SyntheticItems
 * draws on numpy's generator, not the same draws.  Two purposes join the table of that section:
 *   scene of item i:                   j = 0x84000000 | i        (i < 2^24), tag 0xfffffff9
 *   model points of item i:            j = 0x85000000 | i        (i < 2^24), tag 0xfffffff8
 * All real arithmetic is float64, every operation named below ONE rounding in the order written, nothing contracted; an fp32
 * input enters by its exact conversion; u_q = the float64 uniform of word(q) of the item's stream.
 *
 * hsp_scene_draw.  Tables on the device, one row per mesh: ext (n_mesh,3) DOUBLE the extent of the mesh along each axis in
 * model units, cls (n_mesh) fp32 its category, mean_shape (n_mesh,3), sym (n_mesh,4) fp32.  params: 13 doubles ON THE HOST, read
 * when the call is made (a captured launch keeps them): size lo, hi (metres, of the LARGEST side), distance lo, hi (metres),
 * elev lo, hi, roll (degrees), W, H (pixels), fx, fy, cx0, cy0 (the camera's K0, K4, K2, K5).  distractors (D,8) DOUBLE on the
 * device = (mesh, sx, sy, sz, ox, oy, oz, rest): the mesh index as a double, the size in metres, the offset in metres in the
 * item's frame, rest != 0 "lies under the item"; not read when D == 0 (it may be NULL).  For item i:
 *   mesh        k = (uint64(word(0)) * n_mesh) >> 32
 *   scale       side = lo + (hi - lo) * u1;  s = (float)(side / max(ext_k)), max over the three extents; all three scale
 *               components equal s
 *   size        dims = ext_k * (double)s
 *   depth       z = dlo + (dhi - dlo) * u2
 *   centre      px = (W - 1) * u3,  py = (H - 1) * u4: the pixel the centre projects to, inside the frame
 *   t           ((z * (px - cx0)) / fx, (z * (py - cy0)) / fy, z), rounded to fp32
 *   angles      degrees: yaw = 360 * u5, elev = elo + (ehi - elo) * u6, roll = (-r) + (2 * r) * u7
 *   R           Rz(roll) Rx(180 + elev) Ry(yaw), with Rx(a) = [1 0 0; 0 c -s; 0 s c], Ry(a) = [c 0 s; 0 1 0; -s 0 c],
 *               Rz(a) = [c -s 0; s c 0; 0 0 1], c and s the float64 cosine and sine of a * (pi / 180) (the constant pi / 180
 *               rounded once); the two products left to right, an entry of a product (a0 * b0 + a1 * b1) + a2 * b2 with the
 *               zeros and ones multiplied like any other entry; the result rounded to fp32
 *   aug_bb      0.8 + 0.4 * u8, u9, u10, rounded to fp32
 *   aug_rt_r    Rz(az) Ry(ay) Rx(ax) of ax, ay, az = -15 + 30 * u11, u12, u13 degrees, products as above, rounded to fp32
 *   aug_rt_t    (-50 + 100 * u14, u15, u16) / 1000, rounded to fp32
 * Everything else comes from the ROUNDED fp32 R, t and s (the ground truth is the rendered pose exactly): gt_R = R, gt_t = t,
 * nocs_scale = (float) sqrt((d0 * d0 + d1 * d1) + d2 * d2) over dims, gt_s = (float)(dims - (double) mean_shape_k), obj_id,
 * mean_shape and sym the rows of mesh k.  Distractor d of item i, with m its mesh and size its (sx, sy, sz):
 *   scale = (float)(size / ext_m) component by component;  off = (ox, oy, oz), with rest  off_y = off_y - (0.5 * dims_y +
 *   0.5 * size_y);  t_d = (float)(((R_r0 * off_0 + R_r1 * off_1) + R_r2 * off_2) + t_r), r = 0, 1, 2;  its rotation is R.
 *   A mesh entry outside [0, n_mesh) or not finite: mesh_id -1 and scale 0 -- the renderer draws nothing for it.
 * Outputs, n = M * (1 + D) instance rows with the items first, then distractor 0's M rows, then distractor 1's, ...: mesh_id,
 * frame_id (= i), label (1 for an item, 2 + d for distractor d) (n) int32, rt (n,16) fp32 row-major with the fourth row
 * (0, 0, 0, 1), scale (n,3) fp32: what hsp_render_depth_u16 reads.  Item rows (M rows each) fp32: obj_id (M), gt_R (M,9),
 * gt_t, gt_s, mean_shape_out (M,3), sym_out (M,4), nocs_scale (M), aug_bb, aug_rt_t (M,3), aug_rt_r (M,9); angles (M,6) DOUBLE
 * = (yaw, elev, roll, ax, ay, az) in degrees -- the draws themselves, because sine and cosine may differ in the last place
 * between two libraries: two implementations agree on angles bit for bit and on R and aug_rt_r to one fp32 rounding.
 * A NULL pointer, M outside 1..65535, n_mesh < 1, D outside 0..254, a parameter that is not finite, lo > hi or lo <= 0 for size
 * or distance: HSP_ERR_BAD_ARG before any launch.
 *
 * hsp_mesh_sample: model_point (M, n_model, 3) fp32, n_model surface points of each item's mesh in units of the object's
 * diagonal, one lane per point.  verts, tris, mesh: the packed mesh set of the renderer's section; cum (T) DOUBLE: per mesh the
 * running sum of its triangles' areas 0.5 * |(b - a) x (c - a)|, restarting at each mesh's first triangle (made once on the
 * host in float64; a mesh without area is refused there); ext as above; mesh_id (M) int32 and scale (M,3) fp32: the first M
 * rows hsp_scene_draw wrote, or the caller's own.  For point n of item i, with k = mesh_id[i], u0, u1, u2 the float64 uniforms
 * of word(3 n), word(3 n + 1), word(3 n + 2) of the model-point stream of item i:
 *   triangle    x = u0 * cum_last (the mesh's last entry); the first triangle of mesh k with cum > x, found by bisection, the
 *               last one where there is none -- searchsorted on the right side, so a triangle without area is never picked
 *   point       if u1 + u2 > 1: u1 = 1 - u1, u2 = 1 - u2 (reflection: no square root, no transcendental);
 *               p = (a + u1 * (b - a)) + u2 * (c - a) per component, a, b, c the triangle's vertices in its row's order
 *   output      dims_c = ext_k,c * (double) scale_c;  diag = sqrt((d0 * d0 + d1 * d1) + d2 * d2) -- the float64 value whose
 *               rounding is hsp_scene_draw's nocs_scale, made again by the same operations, not passed through memory;
 *               model_point[i,n,c] = (float)((p_c * (double) scale_c) / diag)
 * A mesh_id outside [0, n_mesh), a mesh row that leaves verts or tris, or a vertex index outside its mesh gives a zero point:
 * nothing is read out of bounds.  A NULL pointer, V, T, n_mesh < 1, M outside 1..65535, n_model outside 1..2^20:
 * HSP_ERR_BAD_ARG.
 *
 * hsp_label_boxes_guarded: hsp_label_boxes with one clause added -- where the count is 0 the box is (0, 0, 1, 1), not zeros;
 * the same kernel body, the same bits where the count is positive, the same limits.  For boxes that never visit the host:
 * hsp_dzi_windows gives a row that is not finite for a box without a positive side, and a host caller keeps such boxes out.
 * The guarded box gives a finite window that holds no pixel of the label; hsp_crop_compact then counts 0 valid pixels, the
 * training front end rejects the item by that count (status bit 1), and hsp_batch_select moves on to a spare. */
int hsp_scene_draw(const unsigned long long *key, const double *ext, const float *cls, const float *mean_shape, const float *sym,
                   const double *params, const double *distractors, int M, int n_mesh, int D, int32_t *mesh_id,
                   int32_t *frame_id, int32_t *label, float *rt, float *scale, float *obj_id, float *gt_R, float *gt_t,
                   float *gt_s, float *mean_shape_out, float *sym_out, float *nocs_scale, float *aug_bb, float *aug_rt_t,
                   float *aug_rt_r, double *angles, hspStream_t stream);
int hsp_mesh_sample(const float *verts, int V, const int32_t *tris, int T, const int32_t *mesh, int n_mesh, const double *cum,
                    const double *ext, const int32_t *mesh_id, const float *scale, const unsigned long long *key, int M,
                    int n_model, float *model_point, hspStream_t stream);
int hsp_label_boxes_guarded(const uint8_t *labels, const int32_t *frame_id, const int32_t *label, int n, int F, int H, int W,
                            int32_t *boxes, int32_t *count, hspStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HSP_H_ */
