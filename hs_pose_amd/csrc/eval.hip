// eval.hip -- scoring a run on the device: the reference's compute_degree_cm_mAP (evaluation/eval_utils_v1.py:430-621) as three
// stages.  A GROUP is the predictions and ground truths of one class in one image; a group row of the table the entry points read
// is six int32: {p_off, np, g_off, ng, pair_off, kind}.  include/hsp.h ("evaluation metrics") states the contract; this file follows
// it operation for operation.  Small, latency-bound fp64 work: plain launches, no atomics, every output slot has one writer.
#include "common.h"

namespace hsp {

#define EVAL_L 32                // most predictions, and most ground truths, of one group (hsp_eval_group_cap)
#define EVAL_GCOLS 6
#define EVAL_MATCH_THREADS 256
#define EVAL_AP_THREADS 256

// kind of a group's class: how compute_3d_iou_new / compute_RT_degree_cm_symmetry treat it
#define EVAL_KIND_NONE 0         // camera, laptop, ...
#define EVAL_KIND_YSYM 1         // bottle, bowl, can: symmetric about y
#define EVAL_KIND_MUG 2          // symmetric about y where the ground truth's handle is not visible
#define EVAL_KIND_FLIP 3         // phone, eggbox, glue: the degree also against a half turn about y; the IoU as NONE

// The reference takes its "axis-aligned" extremes with np.amax(bbox, axis=0) on a (3, 8) array: per CORNER over its three
// coordinates, not per axis over the corners (eval_utils_v1.py:47-50).  What it calls a box is therefore eight [min, max] intervals,
// one per corner in get_3d_bbox's order, and intersection and volumes are products of eight lengths.  That is the metric everyone
// quotes, so it is the contract.
struct Box { double lo[8], hi[8]; };

// get_3d_bbox + transform_coordinates_3d + those extremes: M row-major 4x4, s the three extents
__device__ static Box box_of(const double* M, const double* s) {
    Box b;
    const double hx = s[0] / 2, hy = s[1] / 2, hz = s[2] / 2;
    for (int c = 0; c < 8; ++c) {                                // (+,+,+) (+,+,-) (-,+,+) (-,+,-) (+,-,+) (+,-,-) (-,-,+) (-,-,-)
        const double x = (c & 2) ? -hx : hx, y = (c & 4) ? -hy : hy, z = (c & 1) ? -hz : hz;
        const double w = ((M[12] * x + M[13] * y) + M[14] * z) + M[15];
        double v[3];
        for (int k = 0; k < 3; ++k) v[k] = (((M[4 * k] * x + M[4 * k + 1] * y) + M[4 * k + 2] * z) + M[4 * k + 3]) / w;
        b.lo[c] = fmin(fmin(v[0], v[1]), v[2]);
        b.hi[c] = fmax(fmax(v[0], v[1]), v[2]);
    }
    return b;
}

__device__ static double iou_of(const Box& a, const Box& b) {
    double mn = INFINITY, inter = 1.0, va = 1.0, vb = 1.0;     // np.prod: the running product in index order, from 1
    for (int c = 0; c < 8; ++c) {
        const double e = fmin(a.hi[c], b.hi[c]) - fmax(a.lo[c], b.lo[c]);
        mn = fmin(mn, e);
        inter *= e;
        va *= a.hi[c] - a.lo[c];
        vb *= b.hi[c] - b.lo[c];
    }
    if (mn < 0) inter = 0.0;
    return inter / ((va + vb) - inter);
}

__device__ static double det3(const double* M) {         // of the upper-left 3x3 of a row-major 4x4
    return (M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8])) + M[2] * (M[4] * M[9] - M[5] * M[8]);
}

// one (prediction, ground truth) pair per lane and turn of the loop; a workgroup of one wave per group
__global__ __launch_bounds__(HSP_WAVE) void eval_pairs_kernel(const double* __restrict__ pred_RT, const double* __restrict__ pred_s,
                                                              const double* __restrict__ gt_RT, const double* __restrict__ gt_s,
                                                              const int32_t* __restrict__ gt_hv, const int32_t* __restrict__ groups,
                                                              float* __restrict__ iou_out, double* __restrict__ deg_out,
                                                              double* __restrict__ shift_out) {
    const int32_t* gr = groups + (size_t)blockIdx.x * EVAL_GCOLS;
    const int p_off = gr[0], np = gr[1], g_off = gr[2], ng = gr[3], pair_off = gr[4], kind = gr[5];
    for (int q = threadIdx.x; q < np * ng; q += HSP_WAVE) {
        const int i = q / ng, j = q - i * ng;
        double A[16], Bm[16];
        for (int k = 0; k < 16; ++k) { A[k] = pred_RT[(size_t)(p_off + i) * 16 + k]; Bm[k] = gt_RT[(size_t)(g_off + j) * 16 + k]; }
        const double* sa = pred_s + (size_t)(p_off + i) * 3;
        const double* sb = gt_s + (size_t)(g_off + j) * 3;
        const bool sym = kind == EVAL_KIND_YSYM || (kind == EVAL_KIND_MUG && gt_hv[g_off + j] == 0);

        // ---- IoU (compute_3d_iou_new) ----
        const Box bb = box_of(Bm, sb);
        double iou;
        if (sym) {
            iou = 0.0;
            for (int r = 0; r < 20; ++r) {
                const double th = (2.0 * M_PI * (double)r) / 20.0;
                const double c = cos(th), s = sin(th);
                double R[16];
                for (int k = 0; k < 4; ++k) {                   // A . Ry(th)
                    R[4 * k] = A[4 * k] * c + A[4 * k + 2] * (-s);
                    R[4 * k + 1] = A[4 * k + 1];
                    R[4 * k + 2] = A[4 * k] * s + A[4 * k + 2] * c;
                    R[4 * k + 3] = A[4 * k + 3];
                }
                const double v = iou_of(box_of(R, sa), bb);
                if (v > iou) iou = v;                            // Python's max(max_iou, v): a NaN never replaces
            }
        } else {
            iou = iou_of(box_of(A, sa), bb);
        }
        iou_out[pair_off + q] = (float)iou;                      // the reference's float32 overlap table

        // ---- degree and shift (compute_RT_degree_cm_symmetry) ----
        const double ca = cbrt(det3(A)), cb = cbrt(det3(Bm));
        double R1[9], R2[9];
        for (int k = 0; k < 3; ++k)
            for (int m = 0; m < 3; ++m) { R1[3 * k + m] = A[4 * k + m] / ca; R2[3 * k + m] = Bm[4 * k + m] / cb; }
        double theta;
        if (sym) {
            const double dot = (R1[1] * R2[1] + R1[4] * R2[4]) + R1[7] * R2[7];
            const double n1 = sqrt((R1[1] * R1[1] + R1[4] * R1[4]) + R1[7] * R1[7]);
            const double n2 = sqrt((R2[1] * R2[1] + R2[4] * R2[4]) + R2[7] * R2[7]);
            theta = acos(dot / (n1 * n2));
        } else {
            double d[3];                                         // the diagonal of R1 R2^T
            for (int k = 0; k < 3; ++k) d[k] = (R1[3 * k] * R2[3 * k] + R1[3 * k + 1] * R2[3 * k + 1]) + R1[3 * k + 2] * R2[3 * k + 2];
            theta = acos((((d[0] + d[1]) + d[2]) - 1.0) / 2.0);  // not clamped: an argument above 1 is NaN, as in numpy
            if (kind == EVAL_KIND_FLIP) {                        // R1 diag(-1, 1, -1) R2^T
                for (int k = 0; k < 3; ++k)
                    d[k] = ((-R1[3 * k]) * R2[3 * k] + R1[3 * k + 1] * R2[3 * k + 1]) + (-R1[3 * k + 2]) * R2[3 * k + 2];
                const double t2 = acos((((d[0] + d[1]) + d[2]) - 1.0) / 2.0);
                if (t2 < theta) theta = t2;                      // Python's min(theta, t2)
            }
        }
        deg_out[pair_off + q] = theta * (180.0 / M_PI);
        const double dx = A[3] - Bm[3], dy = A[7] - Bm[7], dz = A[11] - Bm[11];
        shift_out[pair_off + q] = sqrt((dx * dx + dy * dy) + dz * dz) * 100.0;
    }
}

// ascending, NaN last, equal keys by ascending index: numpy's stable argsort
template <typename T> __device__ __forceinline__ bool key_before(T va, int ia, T vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na == nb ? ia < ib : nb;
    return va < vb || (va == vb && ia < ib);
}

// one workgroup per group: the pair table in LDS, the three orders made once, then one lane per threshold runs the greedy loops
__global__ __launch_bounds__(EVAL_MATCH_THREADS) void eval_match_kernel(
    const int32_t* __restrict__ groups, const double* __restrict__ scores, const float* __restrict__ iou_tab,
    const double* __restrict__ deg_tab, const double* __restrict__ shift_tab, const float* __restrict__ iou_thres, int T_iou,
    const double* __restrict__ deg_thres, int D1, const double* __restrict__ shift_thres, int S1, int pose_iou_index,
    int8_t* __restrict__ order_out, double* __restrict__ score_sorted, int8_t* __restrict__ iou_pm, int8_t* __restrict__ iou_gm,
    int8_t* __restrict__ pose_pm, int8_t* __restrict__ pose_gm, double* __restrict__ pose_score, int32_t* __restrict__ kept_out) {
    __shared__ double s_deg[EVAL_L * EVAL_L], s_shift[EVAL_L * EVAL_L];
    __shared__ float s_iou[EVAL_L * EVAL_L];
    __shared__ uint8_t s_isort[EVAL_L * EVAL_L], s_psort[EVAL_L * EVAL_L];    // per prediction: its ground truths in visiting order
    __shared__ uint8_t s_order[EVAL_L], s_kp[EVAL_L], s_kg[EVAL_L];
    __shared__ int8_t s_selp[EVAL_L], s_selg[EVAL_L];
    __shared__ int s_knp, s_kng;

    const int32_t* gr = groups + (size_t)blockIdx.x * EVAL_GCOLS;
    const int p_off = gr[0], np = gr[1], g_off = gr[2], ng = gr[3], pair_off = gr[4];
    const int tid = threadIdx.x, TP = D1 * S1;
    if (np > EVAL_L || ng > EVAL_L) return;         // (the entry point refuses such a table; a row that lies about it writes nothing)

    for (int q = tid; q < np * ng; q += EVAL_MATCH_THREADS) {
        s_iou[q] = iou_tab[pair_off + q];
        s_deg[q] = deg_tab[pair_off + q];
        s_shift[q] = shift_tab[pair_off + q];
    }
    if (tid == 0) {                                 // argsort(scores)[::-1]: the stable ascending order, reversed
        for (int i = 0; i < np; ++i) {
            const double v = scores[p_off + i];
            int r = i;                              // insertion into the ascending list s_order[0 .. i)
            while (r > 0 && key_before(v, i, scores[p_off + s_order[r - 1]], (int)s_order[r - 1])) { s_order[r] = s_order[r - 1]; --r; }
            s_order[r] = (uint8_t)i;
        }
        for (int a = 0, b = np - 1; a < b; ++a, --b) { const uint8_t t = s_order[a]; s_order[a] = s_order[b]; s_order[b] = t; }
        for (int pos = 0; pos < np; ++pos) {
            order_out[p_off + pos] = (int8_t)s_order[pos];
            score_sorted[p_off + pos] = scores[p_off + s_order[pos]];
        }
    }
    __syncthreads();
    if (tid < np) {                                 // argsort(iou_row)[::-1] of prediction tid (its index in the class's order)
        uint8_t* row = s_isort + tid * EVAL_L;
        for (int j = 0; j < ng; ++j) {
            const float v = s_iou[tid * ng + j];
            int r = j;
            while (r > 0 && key_before(v, j, s_iou[tid * ng + row[r - 1]], (int)row[r - 1])) { row[r] = row[r - 1]; --r; }
            row[r] = (uint8_t)j;
        }
        for (int a = 0, b = ng - 1; a < b; ++a, --b) { const uint8_t t = row[a]; row[a] = row[b]; row[b] = t; }
    }
    __syncthreads();

    // ---- IoU stage (compute_3d_matches): rows of the tables are group slots, columns thresholds ----
    for (int t = tid; t < T_iou; t += EVAL_MATCH_THREADS) {
        const float thr = iou_thres[t];
        for (int j = 0; j < ng; ++j) iou_gm[(size_t)(g_off + j) * T_iou + t] = -1;
        uint32_t taken = 0;
        for (int pos = 0; pos < np; ++pos) {
            const int i = s_order[pos];
            int m = -1;
            for (int r = 0; r < ng; ++r) {
                const int j = s_isort[i * EVAL_L + r];
                if (taken >> j & 1u) continue;
                const float v = s_iou[i * ng + j];
                if (v < thr) break;
                if (v > thr) { m = j; break; }
            }
            if (m >= 0) {
                taken |= 1u << m;
                iou_gm[(size_t)(g_off + m) * T_iou + t] = (int8_t)pos;      // (this lane wrote the -1 above: program order)
            }
            iou_pm[(size_t)(p_off + pos) * T_iou + t] = (int8_t)m;
            if (t == pose_iou_index) s_selp[pos] = (int8_t)m;
        }
        if (t == pose_iou_index)
            for (int j = 0; j < ng; ++j) s_selg[j] = (taken >> j & 1u) ? 1 : -1;
    }
    __syncthreads();

    // ---- what the pose stage sees: everything (pose_iou_index < 0), or what matched at that IoU threshold, in kept order ----
    if (tid == 0) {
        int knp = 0, kng = 0;
        for (int pos = 0; pos < np; ++pos)
            if (pose_iou_index < 0 || s_selp[pos] > -1) s_kp[knp++] = s_order[pos];
        for (int j = 0; j < ng; ++j)
            if (pose_iou_index < 0 || s_selg[j] > -1) s_kg[kng++] = (uint8_t)j;
        s_knp = knp;
        s_kng = kng;
        kept_out[2 * blockIdx.x] = knp;
        kept_out[2 * blockIdx.x + 1] = kng;
        for (int pos = 0; pos < np; ++pos) pose_score[p_off + pos] = pos < knp ? scores[p_off + s_kp[pos]] : 0.0;
    }
    __syncthreads();
    const int knp = s_knp, kng = s_kng;
    if (tid < knp) {                                // argsort(degree + shift) of kept prediction tid over the kept ground truths
        uint8_t* row = s_psort + tid * EVAL_L;
        const int i = s_kp[tid];
        for (int jj = 0; jj < kng; ++jj) {
            const double v = s_deg[i * ng + s_kg[jj]] + s_shift[i * ng + s_kg[jj]];
            int r = jj;
            while (r > 0) {
                const int o = row[r - 1];
                if (!key_before(v, jj, s_deg[i * ng + s_kg[o]] + s_shift[i * ng + s_kg[o]], o)) break;
                row[r] = row[r - 1];
                --r;
            }
            row[r] = (uint8_t)jj;
        }
    }
    __syncthreads();

    // ---- pose stage (compute_match_from_degree_cm): indices are positions in the kept lists ----
    for (int t = tid; t < TP; t += EVAL_MATCH_THREADS) {
        const double dthr = deg_thres[t / S1], sthr = shift_thres[t % S1];
        for (int j = 0; j < ng; ++j) pose_gm[(size_t)(g_off + j) * TP + t] = -1;
        uint32_t taken = 0;
        for (int pos = 0; pos < np; ++pos) {
            int m = -1;
            if (pos < knp) {
                const int i = s_kp[pos];
                for (int r = 0; r < kng; ++r) {
                    const int jj = s_psort[pos * EVAL_L + r];
                    if (taken >> jj & 1u) continue;
                    const int q = i * ng + s_kg[jj];
                    if (s_deg[q] > dthr || s_shift[q] > sthr) continue;      // a NaN compares false: it passes
                    m = jj;
                    break;
                }
            }
            if (m >= 0) {
                taken |= 1u << m;
                pose_gm[(size_t)(g_off + m) * TP + t] = (int8_t)pos;
            }
            pose_pm[(size_t)(p_off + pos) * TP + t] = (int8_t)m;
        }
    }
}

// numpy's pairwise sum of a[0 .. n) (the add loop np.sum runs over a contiguous piece of up to 8192 elements): below 8 terms in index order, up to 128
// eight interleaved partial sums folded as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the tail in index order, beyond that halves, the
// left one a multiple of 8 long
__device__ static double pairwise_block(const double* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

__device__ static double pairwise_sum(const double* a, int n) {
    // the recursion without a call stack: segments are visited left to right, a finished segment of depth d folds into the
    // pending left sibling of the same depth
    int lo[32], len[32];
    double left[32];
    bool has_left[32];
    int sp = 0;
    lo[0] = 0; len[0] = n; has_left[0] = false;
    double ret = 0.0;
    while (true) {
        if (len[sp] > 128) {                        // split: descend into the left half
            int n2 = len[sp] / 2;
            n2 -= n2 % 8;
            lo[sp + 1] = lo[sp]; len[sp + 1] = n2; has_left[sp + 1] = false;
            ++sp;
            continue;
        }
        ret = pairwise_block(a + lo[sp], len[sp]);
        while (true) {                              // hand the value up
            if (sp == 0) return ret;
            if (!has_left[sp]) {                    // a left half is done: keep it, run the right half of the parent in this slot
                left[sp] = ret;
                has_left[sp] = true;
                const int n2 = len[sp];
                lo[sp] = lo[sp - 1] + n2;
                len[sp] = len[sp - 1] - n2;
                break;
            }
            ret = left[sp] + ret;
            --sp;
        }
    }
}

// np.sum of a contiguous a[0 .. n): it hands its add loop at most 8192 elements at a time and adds the pieces up in order
__device__ static double numpy_sum(const double* a, int n) {
    double acc = 0.0;
    for (int k = 0; k < n; k += 8192) acc += pairwise_sum(a + k, min(8192, n - k));
    return acc;
}

// one workgroup per (threshold, class): compute_ap_from_matches_scores over the class's slots in score order
__global__ __launch_bounds__(EVAL_AP_THREADS) void eval_ap_kernel(const int8_t* __restrict__ match, int T, const int32_t* __restrict__ order,
                                                                  const int32_t* __restrict__ seg_off, const int32_t* __restrict__ gt_cnt,
                                                                  int slots, int C, double* __restrict__ ws, double* __restrict__ aps) {
    __shared__ int s_cnt[EVAL_AP_THREADS];
    __shared__ double s_max[EVAL_AP_THREADS];
    const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int off = seg_off[c], n = seg_off[c + 1] - off, G = gt_cnt[c];
    double* out = aps + (size_t)(c + 1) * T + t;
    if (n <= 0) { if (tid == 0) *out = 0.0; return; }                     // recalls [0, 1], precisions [0, 0]
    if (G <= 0) { if (tid == 0) *out = NAN; return; }                     // recalls 0 / 0: every term is NaN
    double* terms = ws + ((size_t)t * (size_t)(slots + C) + (size_t)(off + c));
    const int chunk = (n + EVAL_AP_THREADS - 1) / EVAL_AP_THREADS;
    const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);

    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += match[(size_t)order[off + i] * T + t] > -1;
    s_cnt[tid] = mine;
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < EVAL_AP_THREADS; ++k) { const int v = s_cnt[k]; total += v; if (k < tid) before += v; }

    // precisions of the chunk, its largest, then the running maximum from the right (the sentinel 0 at the end changes nothing)
    double mx = 0.0;
    {
        int cnt = before;
        for (int i = lo; i < hi; ++i) {
            cnt += match[(size_t)order[off + i] * T + t] > -1;
            mx = fmax(mx, (double)cnt / (double)(i + 1));
        }
    }
    s_max[tid] = mx;
    __syncthreads();
    double env = 0.0;
    for (int k = tid + 1; k < EVAL_AP_THREADS; ++k) env = fmax(env, s_max[k]);
    {
        int cnt = before + mine;                                          // the count at position hi - 1
        const float Gf = (float)G;
        for (int i = hi - 1; i >= lo; --i) {
            env = fmax(env, (double)cnt / (double)(i + 1));
            const bool hit = match[(size_t)order[off + i] * T + t] > -1;
            if (hit) {                                                    // the recall moves exactly where a match is counted
                const double r1 = (double)__fdiv_rn((float)cnt, Gf), r0 = (double)__fdiv_rn((float)(cnt - 1), Gf);
                terms[cnt - 1] = (r1 - r0) * env;
                --cnt;
            }
        }
    }
    if (tid == 0 && total != G) terms[total] = (1.0 - (double)__fdiv_rn((float)total, (float)G)) * 0.0;   // the step up to the sentinel 1
    __syncthreads();
    if (tid == 0) *out = numpy_sum(terms, total + (total != G));
}

// row 0 (BG) = 0, the last row = np.mean(aps[1:-1], axis=0): with more than one column numpy adds row after row, a running sum per
// column; a single column is one contiguous run, which it adds as np.sum does (from 8 classes on that is not the running sum)
__global__ void eval_ap_mean_kernel(double* __restrict__ aps, int T, int C) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double s = 0.0;
    if (T == 1) s = numpy_sum(aps + 1, C);
    else for (int c = 1; c <= C; ++c) s += aps[(size_t)c * T + t];
    aps[t] = 0.0;
    aps[(size_t)(C + 1) * T + t] = s / (double)C;
}

}  // namespace hsp

using namespace hsp;

extern "C" int hsp_eval_group_cap(void) { return EVAL_L; }

// the table of groups lives on the device, so the entry points check what the host can see: extents and pointers
extern "C" int hsp_eval_pairs(const double* pred_RT, const double* pred_scale, const double* gt_RT, const double* gt_scale,
                              const int32_t* gt_handle, const int32_t* groups, int n_groups, int max_group, float* iou, double* degree,
                              double* shift, hspStream_t stream) {
    if (!pred_RT || !pred_scale || !gt_RT || !gt_scale || !gt_handle || !groups || !iou || !degree || !shift || n_groups <= 0 ||
        max_group <= 0)
        return HSP_ERR_BAD_ARG;
    if (max_group > EVAL_L) return HSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(eval_pairs_kernel, dim3(n_groups), dim3(HSP_WAVE), 0, as_stream(stream), pred_RT, pred_scale, gt_RT, gt_scale,
                       gt_handle, groups, iou, degree, shift);
    return check_launch();
}

extern "C" int hsp_eval_match(const int32_t* groups, int n_groups, int max_group, const double* scores, const float* iou,
                              const double* degree, const double* shift, const float* iou_thres, int T_iou, const double* deg_thres,
                              int D1, const double* shift_thres, int S1, int pose_iou_index, int8_t* order, double* score_sorted,
                              int8_t* iou_pred_match, int8_t* iou_gt_match, int8_t* pose_pred_match, int8_t* pose_gt_match,
                              double* pose_score, int32_t* kept, hspStream_t stream) {
    if (!groups || !scores || !iou || !degree || !shift || !iou_thres || !deg_thres || !shift_thres || !order || !score_sorted ||
        !iou_pred_match || !iou_gt_match || !pose_pred_match || !pose_gt_match || !pose_score || !kept || n_groups <= 0 ||
        max_group <= 0 || T_iou <= 0 || D1 <= 0 || S1 <= 0 || pose_iou_index >= T_iou || (long long)D1 * S1 > 2147483647LL)
        return HSP_ERR_BAD_ARG;
    if (max_group > EVAL_L) return HSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(eval_match_kernel, dim3(n_groups), dim3(EVAL_MATCH_THREADS), 0, as_stream(stream), groups, scores, iou, degree,
                       shift, iou_thres, T_iou, deg_thres, D1, shift_thres, S1, pose_iou_index < 0 ? -1 : pose_iou_index, order,
                       score_sorted, iou_pred_match, iou_gt_match, pose_pred_match, pose_gt_match, pose_score, kept);
    return check_launch();
}

extern "C" size_t hsp_eval_ap_workspace_bytes(int slots, int T, int C) {
    if (slots < 0 || T <= 0 || C <= 0) return 0;
    return (size_t)T * ((size_t)slots + (size_t)C) * sizeof(double);
}

extern "C" int hsp_eval_ap(const int8_t* match, int slots, int T, const int32_t* order, const int32_t* seg_off, const int32_t* gt_count,
                           int C, double* aps, void* ws, size_t ws_bytes, hspStream_t stream) {
    if (!match || !order || !seg_off || !gt_count || !aps || slots <= 0 || T <= 0 || C <= 0 || C > 65535) return HSP_ERR_BAD_ARG;
    if (slots >= (1 << 23)) return HSP_ERR_UNSUPPORTED;               // fp32 recalls of neighbouring counts stay apart below 2^23
    if (!ws || ws_bytes < hsp_eval_ap_workspace_bytes(slots, T, C)) return HSP_ERR_WORKSPACE;
    hipLaunchKernelGGL(eval_ap_kernel, dim3(T, C), dim3(EVAL_AP_THREADS), 0, as_stream(stream), match, T, order, seg_off, gt_count, slots,
                       C, static_cast<double*>(ws), aps);
    int rc = check_launch();
    if (rc != HSP_OK) return rc;
    hipLaunchKernelGGL(eval_ap_mean_kernel, dim3((T + 255) / 256), dim3(256), 0, as_stream(stream), aps, T, C);
    return check_launch();
}
