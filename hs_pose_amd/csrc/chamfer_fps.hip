// chamfer_fps.hip -- Chamfer distance (fwd/bwd) and farthest point sampling for gfx950.
//
// Chamfer: replaces the reference's CUDA extension tools/pyTorchChamferDistance/chamfer_distance.cu
// (:6-137 forward, :158-187 backward) / its CPU twin chamfer_distance.cpp:59-177.  Same results:
// squared distance from coordinate differences in fp32, FIRST minimum wins (strict '<').
// Design differs from the reference kernel: one lane per query point, the other cloud staged in
// LDS as float4 in chunks of 2048 points (broadcast ds_read_b128, no bank conflicts), grid sized
// from the problem instead of a fixed dim3(32,16).
// FPS: replaces tools/eval_utils.py:107-119 (per cloud): start at 0, running min, first max wins.
#include "common.h"
#include "fps_pick.h"
#include "sym_target.h"

namespace hsp {

#define CH_CHUNK 2048

// 64 queries per workgroup (lane = query); the 4 waves scan the 4 quarters of every staged chunk and the partial
// (distance, index) pairs meet in LDS -- lexicographic minimum == the first minimum of a serial scan.  With one wave per
// 64 queries a 1028-point cloud pair gives 272 waves for 1024 SIMDs; this form gives 1088.
// The scan itself, shared by chamfer_nn_kernel and recon_chamfer_nn_kernel: cand(j) is candidate j of the cloud (a float4, .w unused),
// (x1, y1, z1) the lane's query.  Returns true on the lanes of wave 0, which then hold the query's (distance, first arg-min).
template <class Cand>
__device__ __forceinline__ bool chamfer_scan(float4* pts, float (*sd)[64], int (*si)[64], const Cand& cand, int m, float x1,
                                             float y1, float z1, float& bd, int& bi) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float best = INFINITY;
    int besti = INT_MAX;
    for (int c0 = 0; c0 < m; c0 += CH_CHUNK) {
        const int cn = min(CH_CHUNK, m - c0);
        __syncthreads();
        for (int j = threadIdx.x; j < cn; j += 256) pts[j] = cand(c0 + j);
        __syncthreads();
        const int q = (cn + 3) >> 2;
        const int j0 = wv * q, j1 = min(cn, j0 + q);
        int j = j0;
        for (; j + 7 < j1; j += 8) {                         // 8 broadcast LDS reads in flight per round trip
            float4 p[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u] = pts[j + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float dx = sub_rn(p[u].x, x1), dy = sub_rn(p[u].y, y1), dz = sub_rn(p[u].z, z1);
                const float d = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
                if (d < best) { best = d; besti = c0 + j + u; }
            }
        }
        for (; j < j1; ++j) {
            const float4 p = pts[j];
            const float dx = sub_rn(p.x, x1), dy = sub_rn(p.y, y1), dz = sub_rn(p.z, z1);
            const float d = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
            if (d < best) { best = d; besti = c0 + j; }
        }
    }
    sd[wv][lane] = best;
    si[wv][lane] = besti;
    __syncthreads();
    if (wv != 0) return false;
    // lexicographic minimum of the partial (distance, index) pairs == the serial scan's first minimum
    bd = sd[0][lane];
    bi = si[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float d = sd[w][lane];
        const int k = si[w][lane];
        if (d < bd || (d == bd && k < bi)) { bd = d; bi = k; }
    }
    if (bi == INT_MAX) {        // nothing compared below +inf (NaN / overflowing input): the reference keeps candidate 0
        const float4 p = cand(0);
        const float dx = sub_rn(p.x, x1), dy = sub_rn(p.y, y1), dz = sub_rn(p.z, z1);
        bd = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
        bi = 0;
    }
    return true;
}

struct CandRows {                  // the candidates of a cloud as they lie in memory
    const float* cb;
    __device__ __forceinline__ float4 operator()(int j) const { return make_float4(cb[j * 3], cb[j * 3 + 1], cb[j * 3 + 2], 0.f); }
};

__global__ __launch_bounds__(256) void chamfer_nn_kernel(const float* __restrict__ a, int n,
                                                         const float* __restrict__ c, int m,
                                                         float* __restrict__ dist, int32_t* __restrict__ idx) {
    __shared__ float4 pts[CH_CHUNK];
    __shared__ float sd[4][64];
    __shared__ int si[4][64];
    const int b = blockIdx.y;
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const float* ab = a + (size_t)b * n * 3;
    float x1 = 0.f, y1 = 0.f, z1 = 0.f;
    if (i < n) { x1 = ab[i * 3]; y1 = ab[i * 3 + 1]; z1 = ab[i * 3 + 2]; }
    float bd;
    int bi;
    if (chamfer_scan(pts, sd, si, CandRows{c + (size_t)b * m * 3}, m, x1, y1, z1, bd, bi) && i < n) {
        dist[(size_t)b * n + i] = bd;
        idx[(size_t)b * n + i] = bi;
    }
}

// ---- the Chamfer reconstruction term (hsp_recon_chamfer_fwd / _bwd; include/hsp.h) ---------------------------------------------
// One launch searches both directions: workgroup x < nb of cloud b holds 64 rows of the reconstruction P = recon[b] as queries and
// scans the target G[b], which it makes from PC[b] while it stages a chunk (sym_target.h: the rule of the loss kernels'
// Prop_sym_recon; ~30 flops per candidate against 64 distances); workgroup x >= nb holds 64 rows of G as queries -- made by the same
// function, so the same bits -- writes them out and scans P.  A skip cloud is not searched: G = 0, distances 0, arg-mins 0.
struct ReconCloud {
    SymClass k;
    float R[9], t[3];
};
struct CandTarget {                // candidate j = the target of observed point j
    const float* pc;
    const ReconCloud* c;
    __device__ __forceinline__ float4 operator()(int j) const {
        const float P[3] = {pc[j * 3], pc[j * 3 + 1], pc[j * 3 + 2]};
        float canon[3], T[3];
        sym_canon(c->R, c->t, P, canon);
        sym_recon_target(c->k, c->R, c->t, P, canon, T);
        return make_float4(T[0], T[1], T[2], 0.f);
    }
};

__global__ __launch_bounds__(256) void recon_chamfer_nn_kernel(const float* __restrict__ PC, const float* __restrict__ gt_R,
                                                               const float* __restrict__ gt_t, const float* __restrict__ sym,
                                                               const float* __restrict__ recon, int N, int nb,
                                                               float* __restrict__ G, int32_t* __restrict__ idx1,
                                                               int32_t* __restrict__ idx2, float* __restrict__ d1,
                                                               float* __restrict__ d2) {
    __shared__ float4 pts[CH_CHUNK];
    __shared__ float sd[4][64];
    __shared__ int si[4][64];
    const int b = blockIdx.y;
    const bool dir2 = (int)blockIdx.x >= nb;                  // workgroup-uniform
    const int i = ((int)blockIdx.x - (dir2 ? nb : 0)) * 64 + (threadIdx.x & 63);
    const size_t row = (size_t)b * N + i;
    ReconCloud c;
    c.k = sym_class(sym + b * 4);
    for (int e = 0; e < 9; ++e) c.R[e] = gt_R[b * 9 + e];
    for (int e = 0; e < 3; ++e) c.t[e] = gt_t[b * 3 + e];
    const float* pc = PC + (size_t)b * N * 3;
    const float* re = recon + (size_t)b * N * 3;
    float* dist = dir2 ? d2 : d1;
    int32_t* idx = dir2 ? idx2 : idx1;
    if (c.k.skip) {                                           // (the whole workgroup: no barrier is left waiting)
        if (threadIdx.x < 64 && i < N) {
            dist[row] = 0.f;
            idx[row] = 0;
            if (dir2) { G[row * 3] = 0.f; G[row * 3 + 1] = 0.f; G[row * 3 + 2] = 0.f; }
        }
        return;
    }
    const CandTarget target{pc, &c};
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < N) q = dir2 ? target(i) : CandRows{re}(i);
    float bd;
    int bi;
    const bool mine = dir2 ? chamfer_scan(pts, sd, si, CandRows{re}, N, q.x, q.y, q.z, bd, bi)
                           : chamfer_scan(pts, sd, si, target, N, q.x, q.y, q.z, bd, bi);
    if (mine && i < N) {
        dist[row] = bd;
        idx[row] = bi;
        if (dir2) { G[row * 3] = q.x; G[row * 3 + 1] = q.y; G[row * 3 + 2] = q.z; }
    }
}

// term = (w * S) / (B N), S the sum of the E = 2 B N distances d[0 .. E) (d1 then d2, row-major) in ONE order: thread t of the
// 1024 adds d[t], d[t + 1024], ... in that order starting from d[t] + 0; the 1024 partials then fold pairwise, s[t] += s[t + h]
// for h = 512, 256, ..., 1.  Every operation rounded once.
#define RC_SUM_THREADS 1024
__global__ __launch_bounds__(RC_SUM_THREADS) void recon_chamfer_sum_kernel(const float* __restrict__ d, long long E, float w,
                                                                           float bn, float* __restrict__ term) {
    __shared__ float s[RC_SUM_THREADS];
    const int t = threadIdx.x;
    float acc = 0.f;
    for (long long e = t; e < E; e += RC_SUM_THREADS) acc = add_rn(acc, d[e]);
    s[t] = acc;
    __syncthreads();
    for (int h = RC_SUM_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) s[t] = add_rn(s[t], s[t + h]);
        __syncthreads();
    }
    if (t == 0) term[0] = __fdiv_rn(mul_rn(w, s[0]), bn);
}

// ---- ordered backward: one output row per WAVE, its own term first, then the terms of the points that chose it in ascending
// order of their index (the lists of hsp_rev_build, k = 1: edge id == the choosing point's index).  No atomics, no pre-zeroing.
// The lanes fetch 64 of the row's terms at a time (the loads of a long list -- a hub row that a whole cloud chose -- are in
// flight together instead of one dependent round trip each); every lane then adds them to the same accumulator in list order,
// lane by lane, so the sum is the serial one whatever the list's length.
#define CH_ROWS_PER_WG 4           // 256 threads

template <class Term>              // term(j): the three addends that choosing point j contributes
__device__ __forceinline__ void ordered_row_sum(float& ax, float& ay, float& az, const int32_t* __restrict__ off,
                                                const int32_t* __restrict__ edge, int row, const Term& term) {
    const int lane = threadIdx.x & 63;
    const int e0 = __builtin_amdgcn_readfirstlane(off[row]), e1 = __builtin_amdgcn_readfirstlane(off[row + 1]);
    for (int base = e0; base < e1; base += 64) {
        float tx = 0.f, ty = 0.f, tz = 0.f;
        if (base + lane < e1) term(edge[base + lane], tx, ty, tz);
        const int cnt = min(64, e1 - base);                  // wave-uniform
        for (int l = 0; l < cnt; ++l) {
            ax = add_rn(ax, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tx), l)));
            ay = add_rn(ay, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ty), l)));
            az = add_rn(az, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tz), l)));
        }
    }
}

// hsp_chamfer_bwd's arithmetic term by term: g = 2 gd, v = g (p - q); the chosen row receives -v (a - v == a + (-v) bit for bit)
struct TermScatter {
    const float* other;
    const float* gd_other;
    float px, py, pz;
    __device__ __forceinline__ void operator()(int j, float& tx, float& ty, float& tz) const {
        const float gj = mul_rn(gd_other[j], 2.0f);
        tx = -mul_rn(gj, sub_rn(other[j * 3], px));
        ty = -mul_rn(gj, sub_rn(other[j * 3 + 1], py));
        tz = -mul_rn(gj, sub_rn(other[j * 3 + 2], pz));
    }
};
__device__ __forceinline__ void chamfer_row_ordered(const float* __restrict__ own, const float* __restrict__ other, int i, int j0,
                                                    float gd_own, const float* __restrict__ gd_other,
                                                    const int32_t* __restrict__ off, const int32_t* __restrict__ edge,
                                                    float* __restrict__ out) {
    const float px = own[i * 3], py = own[i * 3 + 1], pz = own[i * 3 + 2];
    const float g = mul_rn(gd_own, 2.0f);
    float ax = mul_rn(g, sub_rn(px, other[j0 * 3])), ay = mul_rn(g, sub_rn(py, other[j0 * 3 + 1])),
          az = mul_rn(g, sub_rn(pz, other[j0 * 3 + 2]));
    ordered_row_sum(ax, ay, az, off, edge, i, TermScatter{other, gd_other, px, py, pz});
    if ((threadIdx.x & 63) == 0) { out[i * 3] = ax; out[i * 3 + 1] = ay; out[i * 3 + 2] = az; }
}

// workgroups x < nb1: rows of gx1 over (off1, edge1) = the reverse of idx2 (n source rows); the others: rows of gx2 over
// (off2, edge2) = the reverse of idx1 (m source rows)
__global__ __launch_bounds__(256) void chamfer_grad_ordered_kernel(const float* __restrict__ x1, int n, const float* __restrict__ x2,
                                                                   int m, const int32_t* __restrict__ idx1,
                                                                   const int32_t* __restrict__ idx2, const float* __restrict__ gd1,
                                                                   const float* __restrict__ gd2, const int32_t* __restrict__ off1,
                                                                   const int32_t* __restrict__ edge1,
                                                                   const int32_t* __restrict__ off2,
                                                                   const int32_t* __restrict__ edge2, int nb1,
                                                                   float* __restrict__ gx1, float* __restrict__ gx2) {
    const int b = blockIdx.y;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* a = x1 + (size_t)b * n * 3;
    const float* c = x2 + (size_t)b * m * 3;
    if ((int)blockIdx.x < nb1) {
        const int i = blockIdx.x * CH_ROWS_PER_WG + wv;
        if (i >= n) return;
        chamfer_row_ordered(a, c, i, idx1[(size_t)b * n + i], gd1[(size_t)b * n + i], gd2 + (size_t)b * m,
                            off1 + (size_t)b * (n + 1), edge1 + (size_t)b * m, gx1 + (size_t)b * n * 3);
    } else {
        const int j = ((int)blockIdx.x - nb1) * CH_ROWS_PER_WG + wv;
        if (j >= m) return;
        chamfer_row_ordered(c, a, j, idx2[(size_t)b * m + j], gd2[(size_t)b * m + j], gd1 + (size_t)b * n,
                            off2 + (size_t)b * (m + 1), edge2 + (size_t)b * n, gx2 + (size_t)b * m * 3);
    }
}

// the term's own backward: gx[b,i] = s * [ (P_i - G_idx1[i]) + sum over the j that chose i, ascending, of (P_i - G_j) ],
// s = 2 * ((g * w) / (B N)) applied once at the end; a skip cloud's rows are zeros
struct TermRecon {
    const float* Gb;
    float px, py, pz;
    __device__ __forceinline__ void operator()(int j, float& tx, float& ty, float& tz) const {
        tx = sub_rn(px, Gb[j * 3]);
        ty = sub_rn(py, Gb[j * 3 + 1]);
        tz = sub_rn(pz, Gb[j * 3 + 2]);
    }
};
__global__ __launch_bounds__(256) void recon_chamfer_grad_kernel(const float* __restrict__ recon, const float* __restrict__ G,
                                                                 const int32_t* __restrict__ idx1, const float* __restrict__ sym,
                                                                 const int32_t* __restrict__ off, const int32_t* __restrict__ edge,
                                                                 const float* __restrict__ g, float w, float bn, int N,
                                                                 float* __restrict__ gx) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * CH_ROWS_PER_WG + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= N) return;
    const bool writer = (threadIdx.x & 63) == 0;
    float* out = gx + ((size_t)b * N + i) * 3;
    if (sym_class(sym + b * 4).skip) {
        if (writer) { out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; }
        return;
    }
    const float* P = recon + (size_t)b * N * 3;
    const float* Gb = G + (size_t)b * N * 3;
    const float px = P[i * 3], py = P[i * 3 + 1], pz = P[i * 3 + 2];
    const int j0 = idx1[(size_t)b * N + i];
    float ax = sub_rn(px, Gb[j0 * 3]), ay = sub_rn(py, Gb[j0 * 3 + 1]), az = sub_rn(pz, Gb[j0 * 3 + 2]);
    ordered_row_sum(ax, ay, az, off + (size_t)b * (N + 1), edge + (size_t)b * N, i, TermRecon{Gb, px, py, pz});
    const float s = mul_rn(2.0f, __fdiv_rn(mul_rn(g[0], w), bn));
    if (writer) { out[0] = mul_rn(s, ax); out[1] = mul_rn(s, ay); out[2] = mul_rn(s, az); }
}

// one direction of the backward: ga += g*(p-q), gc[idx] -= g*(p-q), g = 2*gd   (both pre-zeroed)
__global__ __launch_bounds__(256) void chamfer_grad_kernel(const float* __restrict__ a, int n,
                                                           const float* __restrict__ c, int m,
                                                           const int32_t* __restrict__ idx,
                                                           const float* __restrict__ gd, float* __restrict__ ga,
                                                           float* __restrict__ gc) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t pi = (size_t)b * n + i;
    const int j2 = idx[pi];
    const size_t pj = (size_t)b * m + j2;
    const float g = mul_rn(gd[pi], 2.0f);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float v = mul_rn(g, sub_rn(a[pi * 3 + d], c[pj * 3 + d]));
        atomicAdd(ga + pi * 3 + d, v);
        atomicAdd(gc + pj * 3 + d, -v);
    }
}

// ------------------------------------------------------------------------------------------------
// FPS.  A pick is a dependent chain (distance update -> arg-max over the cloud -> next centre), so the kernel is
// built around the length of that chain: one workgroup per cloud, the cloud's coordinates AND the running
// distance-to-set in registers (PPT points per thread, point j = tid + k * THREADS so indices ascend per lane),
// a copy of the coordinates in LDS for the centre look-up, and per pick
//   registers: update + per-lane best  ->  one 64-bit key (value bits | ~index: max = largest value, lowest index)
//   wave:      4 DPP steps inside the 16-lane rows + 4 v_readlane across the rows
//   workgroup: one LDS slot per wave, ONE barrier (slots double-buffered by pick parity), every thread folds
//              the <= 16 slots itself and reads the winner's coordinates from LDS (broadcast).
// No global memory inside the loop except the 4-byte result store.  (fps_generic_kernel below: any N, distances
// in a global workspace.)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long k, const int ctrl_sel) {
    unsigned lo = (unsigned)k, hi = (unsigned)(k >> 32), olo, ohi;
    switch (ctrl_sel) {                                     // dpp_ctrl must be an immediate
        case 0: olo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xF, 0xF, false);      // quad_perm [1,0,3,2]
                ohi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xF, 0xF, false); break;
        case 1: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xF, 0xF, false);      // quad_perm [2,3,0,1]
                ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xF, 0xF, false); break;
        case 2: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xF, 0xF, false);     // row_half_mirror
                ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xF, 0xF, false); break;
        default: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xF, 0xF, false);    // row_mirror
                 ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xF, 0xF, false); break;
    }
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    return o > k ? o : k;
}

template <int THREADS, int PPT>
__global__ __launch_bounds__(THREADS) void fps_reg_kernel(const float* __restrict__ xyz, int N, int n_samples,
                                                          int32_t* __restrict__ sel) {
    constexpr int W = THREADS / HSP_WAVE;
    extern __shared__ __attribute__((aligned(16))) float s_xyz[];          // N * 3
    __shared__ unsigned long long slot[2][W];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* p = xyz + (size_t)b * N * 3;
    for (int e = tid; e < N * 3; e += THREADS) s_xyz[e] = p[e];
    float px[PPT], py[PPT], pz[PPT], dt[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int j = tid + k * THREADS;
        const bool in = j < N;
        px[k] = in ? p[j * 3] : 0.f;
        py[k] = in ? p[j * 3 + 1] : 0.f;
        pz[k] = in ? p[j * 3 + 2] : 0.f;
        dt[k] = INFINITY;
    }
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < n_samples; ++s) {
        if (tid == 0) sel[(size_t)b * n_samples + s] = cur;
        const float cx = s_xyz[cur * 3], cy = s_xyz[cur * 3 + 1], cz = s_xyz[cur * 3 + 2];
        unsigned long long key = 0;                         // (value bits << 32) | ~index; values are >= 0
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int j = tid + k * THREADS;
            const float dx = sub_rn(px[k], cx), dy = sub_rn(py[k], cy), dz = sub_rn(pz[k], cz);
            // numpy on a float32 cloud: fp32 (x*x + y*y) + z*z, then a correctly rounded fp32 sqrt (eval_utils.py:73-84);
            // the sqrt folds neighbouring d^2 values into exact ties that argmax breaks by index, so it cannot be skipped
            const float d = sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));   // (__fsqrt_rn is the 1-ulp native sqrt)
            const float v = fminf(dt[k], d);
            dt[k] = v;
            const unsigned long long kk = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(~j);
            if (j < N && kk > key) key = kk;
        }
        key = dpp_max_u64(key, 0);
        key = dpp_max_u64(key, 1);
        key = dpp_max_u64(key, 2);
        key = dpp_max_u64(key, 3);                          // every lane holds its 16-lane row's best
        unsigned long long wk = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned lo = __builtin_amdgcn_readlane((unsigned)key, r * 16);
            const unsigned hi = __builtin_amdgcn_readlane((unsigned)(key >> 32), r * 16);
            const unsigned long long rk = ((unsigned long long)hi << 32) | lo;
            wk = rk > wk ? rk : wk;
        }
        if (W > 1) {
            if (lane == 0) slot[s & 1][wv] = wk;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const unsigned long long o = slot[s & 1][w];
                wk = o > wk ? o : wk;
            }
        }
        cur = (int)(~(unsigned)wk);
    }
}

// ---- the levels form: Pool_layer's farthest-point sampler (gcn3d.Pool_layer(sampler="fps")) -------------------------------------
// The pick chain of fps_reg_kernel with ONE rule added: a picked row is never picked again.  A picked row's distance-to-set is set
// to -1 and the key's value word is compared SIGNED, so such a row ranks below every unpicked row (whose distance is >= +0) in the
// same single 64-bit compare; among unpicked rows the order is fps_reg_kernel's (largest value, then lowest index).  On a cloud
// whose plain picks are all distinct the picks are therefore the plain kernel's, bit for bit; on a tiled cloud with fewer distinct
// points than picks the remaining picks are the lowest-index unpicked rows.  The picked coordinates -- in LDS already -- are written
// as the level-1 cloud v1 (B,N1,3) in pick order and its first N2 rows as v2 (B,N2,3): farthest-point picks are nested, so the
// sampler run on v1 returns 0 .. N2-1.  (The key and its wave fold: fps_pick.h.)
template <int THREADS, int PPT>
__global__ __launch_bounds__(THREADS) void fps_levels_kernel(const float* __restrict__ xyz, int N, int N1, int N2,
                                                             int32_t* __restrict__ sel1, float* __restrict__ v1,
                                                             float* __restrict__ v2) {
    constexpr int W = THREADS / HSP_WAVE;
    extern __shared__ __attribute__((aligned(16))) float s_xyz[];          // N * 3
    __shared__ long long slot[2][W];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* p = xyz + (size_t)b * N * 3;
    for (int e = tid; e < N * 3; e += THREADS) s_xyz[e] = p[e];
    float px[PPT], py[PPT], pz[PPT], dt[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int j = tid + k * THREADS;
        const bool in = j < N;
        px[k] = in ? p[j * 3] : 0.f;
        py[k] = in ? p[j * 3 + 1] : 0.f;
        pz[k] = in ? p[j * 3 + 2] : 0.f;
        dt[k] = INFINITY;
    }
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < N1; ++s) {
        const float cx = s_xyz[cur * 3], cy = s_xyz[cur * 3 + 1], cz = s_xyz[cur * 3 + 2];
        if (tid < 3) {                                      // the pick and its coordinates (lane e: coordinate e)
            const float c = tid == 0 ? cx : tid == 1 ? cy : cz;
            if (tid == 0) sel1[(size_t)b * N1 + s] = cur;
            v1[((size_t)b * N1 + s) * 3 + tid] = c;
            if (s < N2) v2[((size_t)b * N2 + s) * 3 + tid] = c;
        }
        long long key = LLONG_MIN;                          // (value bits, signed) << 32 | ~index
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int j = tid + k * THREADS;
            const float dx = sub_rn(px[k], cx), dy = sub_rn(py[k], cy), dz = sub_rn(pz[k], cz);
            const float d = sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));   // as fps_reg_kernel
            const float v = j == cur ? -1.f : fminf(dt[k], d);           // picked: -1 for good (fminf(-1, d) == -1)
            dt[k] = v;
            const long long kk = (long long)(((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(~j));
            if (j < N && kk > key) key = kk;
        }
        long long wk = wave_max_i64(key);                   // (fps_pick.h)
        if (W > 1) {
            if (lane == 0) slot[s & 1][wv] = wk;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const long long o = slot[s & 1][w];
                wk = o > wk ? o : wk;
            }
        }
        cur = (int)(~(unsigned)wk);
    }
}

// any N: one 1024-thread workgroup per cloud; dist-to-set lives in a global workspace (L2 resident);
// each round = distance update + workgroup arg-max (max value, then lowest index).
#define FPS_THREADS 1024

template <typename T> __device__ __forceinline__ T fps_dist(T dx, T dy, T dz);
template <> __device__ __forceinline__ float fps_dist<float>(float dx, float dy, float dz) {
    return sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));      // correctly rounded (ocml)
}
template <> __device__ __forceinline__ double fps_dist<double>(double dx, double dy, double dz) {
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

// T = float: any N (distances in a global workspace); T = double: the reference helper's own dtype (it is called on
// float64 mesh vertices, tools/eval_utils.py:122-140) -- numpy's float64 arithmetic step for step.
template <typename T>
__global__ __launch_bounds__(FPS_THREADS) void fps_generic_kernel(const T* __restrict__ xyz, int N, int n_samples,
                                                                  int32_t* __restrict__ sel, T* __restrict__ dts) {
    __shared__ T sv[FPS_THREADS / HSP_WAVE];
    __shared__ int si[FPS_THREADS / HSP_WAVE];
    __shared__ int scur;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const T* p = xyz + (size_t)b * N * 3;
    T* dt = dts + (size_t)b * N;
    for (int j = tid; j < N; j += FPS_THREADS) dt[j] = (T)INFINITY;
    int cur = 0;
    for (int s = 0; s < n_samples; ++s) {
        if (tid == 0) sel[(size_t)b * n_samples + s] = cur;
        const T cx = p[cur * 3], cy = p[cur * 3 + 1], cz = p[cur * 3 + 2];
        T bv = (T)-1.0;
        int bi = INT_MAX;
        for (int j = tid; j < N; j += FPS_THREADS) {
            const T d = fps_dist<T>(p[j * 3] - cx, p[j * 3 + 1] - cy, p[j * 3 + 2] - cz);
            T v = dt[j];
            if (d < v) { v = d; dt[j] = d; }
            if (v > bv) { bv = v; bi = j; }          // j ascends per lane: strict '>' keeps the first max
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const T ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { sv[tid >> 6] = bv; si[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            T fv = sv[0];
            int fi = si[0];
            for (int w = 1; w < FPS_THREADS / HSP_WAVE; ++w)
                if (sv[w] > fv || (sv[w] == fv && si[w] < fi)) { fv = sv[w]; fi = si[w]; }
            scur = fi;
        }
        __syncthreads();
        cur = scur;
    }
}

}  // namespace hsp

using namespace hsp;

extern "C" int hsp_chamfer_fwd(const float* xyz1, const float* xyz2, int B, int n, int m, float* dist1, float* dist2,
                               int32_t* idx1, int32_t* idx2, hspStream_t stream) {
    if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2 || B <= 0 || n <= 0 || m <= 0) return HSP_ERR_BAD_ARG;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(chamfer_nn_kernel, dim3((n + 63) / 64, B), dim3(256), 0, st, xyz1, n, xyz2, m, dist1, idx1);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(chamfer_nn_kernel, dim3((m + 63) / 64, B), dim3(256), 0, st, xyz2, m, xyz1, n, dist2, idx2);
    return check_launch();
}

extern "C" int hsp_chamfer_bwd(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2,
                               const float* gd1, const float* gd2, int B, int n, int m, float* gx1, float* gx2,
                               hspStream_t stream) {
    if (!xyz1 || !xyz2 || !idx1 || !idx2 || !gd1 || !gd2 || !gx1 || !gx2 || B <= 0 || n <= 0 || m <= 0)
        return HSP_ERR_BAD_ARG;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(gx1, 0, (size_t)B * n * 3 * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(gx2, 0, (size_t)B * m * 3 * sizeof(float), st);
    if (e != hipSuccess) { set_last_hip_error(e); return HSP_ERR_LAUNCH; }
    hipLaunchKernelGGL(chamfer_grad_kernel, dim3((n + 255) / 256, B), dim3(256), 0, st, xyz1, n, xyz2, m, idx1, gd1, gx1, gx2);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(chamfer_grad_kernel, dim3((m + 255) / 256, B), dim3(256), 0, st, xyz2, m, xyz1, n, idx2, gd2, gx2, gx1);
    return check_launch();
}

// ---- ordered backward (no float atomics) ----------------------------------------------------------------------------------------
// the grids put a cloud on blockIdx.y
#define CH_MAX_CLOUDS 65535

extern "C" int hsp_chamfer_bwd_ordered_ok(int B, int n, int m) {
    return B > 0 && B <= CH_MAX_CLOUDS && hsp_rev_build_takes(n) && hsp_rev_build_takes(m) ? 1 : 0;
}

extern "C" size_t hsp_chamfer_bwd_ordered_workspace_bytes(int B, int n, int m) {
    if (B <= 0 || n <= 0 || m <= 0) return 0;
    return (size_t)B * (2 * ((size_t)n + m) + 2) * sizeof(int32_t);
}

extern "C" int hsp_chamfer_bwd_ordered(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2,
                                       const float* gd1, const float* gd2, int B, int n, int m, float* gx1, float* gx2, void* ws,
                                       size_t ws_bytes, hspStream_t stream) {
    if (!xyz1 || !xyz2 || !idx1 || !idx2 || !gd1 || !gd2 || (!gx1 && !gx2) || B <= 0 || n <= 0 || m <= 0 || !ws ||
        ws_bytes < hsp_chamfer_bwd_ordered_workspace_bytes(B, n, m))
        return HSP_ERR_BAD_ARG;
    if (!hsp_chamfer_bwd_ordered_ok(B, n, m)) return HSP_ERR_UNSUPPORTED;      // (nothing launched)
    // ws: off1 (B,n+1) | edge1 (B,m) -- the reverse of idx2, the lists of gx1's rows -- | off2 (B,m+1) | edge2 (B,n) -- of idx1
    int32_t* off1 = reinterpret_cast<int32_t*>(ws);
    int32_t* edge1 = off1 + (size_t)B * (n + 1);
    int32_t* off2 = edge1 + (size_t)B * m;
    int32_t* edge2 = off2 + (size_t)B * (m + 1);
    int rc;
    if (gx1 && gx2) {
        const int32_t* idx[2] = {idx2, idx1};
        const int nq[2] = {m, n}, ns[2] = {n, m}, one[2] = {1, 1};
        int32_t* off[2] = {off1, off2};
        int32_t* edge[2] = {edge1, edge2};
        rc = hsp_rev_build_multi(2, idx, B, nq, ns, one, one, off, edge, stream);
    } else if (gx1) {
        rc = hsp_rev_build(idx2, B, m, n, 1, 1, off1, edge1, stream);
    } else {
        rc = hsp_rev_build(idx1, B, n, m, 1, 1, off2, edge2, stream);
    }
    if (rc) return rc;
    const int nb1 = gx1 ? (n + CH_ROWS_PER_WG - 1) / CH_ROWS_PER_WG : 0, nb2 = gx2 ? (m + CH_ROWS_PER_WG - 1) / CH_ROWS_PER_WG : 0;
    hipLaunchKernelGGL(chamfer_grad_ordered_kernel, dim3(nb1 + nb2, B), dim3(256), 0, as_stream(stream), xyz1, n, xyz2, m, idx1,
                       idx2, gd1, gd2, off1, edge1, off2, edge2, nb1, gx1, gx2);
    return check_launch();
}

// ---- the Chamfer reconstruction term ------------------------------------------------------------------------------------------
extern "C" size_t hsp_recon_chamfer_fwd_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return 2 * (size_t)B * N * sizeof(float);
}

extern "C" int hsp_recon_chamfer_fwd(const float* PC, const float* gt_R, const float* gt_t, const float* sym, const float* recon,
                                     int B, int N, float w, float* term, float* G, int32_t* idx1, int32_t* idx2, void* ws,
                                     size_t ws_bytes, hspStream_t stream) {
    if (!PC || !gt_R || !gt_t || !sym || !recon || !term || !G || !idx1 || !idx2 || B <= 0 || N <= 0 || !isfinite(w) || !ws ||
        ws_bytes < hsp_recon_chamfer_fwd_workspace_bytes(B, N))
        return HSP_ERR_BAD_ARG;
    if (B > CH_MAX_CLOUDS) return HSP_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    float* d1 = reinterpret_cast<float*>(ws);                  // ws: d1 (B,N) | d2 (B,N)
    float* d2 = d1 + (size_t)B * N;
    const int nb = (N + 63) / 64;
    hipLaunchKernelGGL(recon_chamfer_nn_kernel, dim3(2 * nb, B), dim3(256), 0, st, PC, gt_R, gt_t, sym, recon, N, nb, G, idx1, idx2,
                       d1, d2);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(recon_chamfer_sum_kernel, dim3(1), dim3(RC_SUM_THREADS), 0, st, d1, 2LL * B * N, w, (float)((long long)B * N),
                       term);
    return check_launch();
}

extern "C" size_t hsp_recon_chamfer_bwd_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (size_t)B * (2 * (size_t)N + 1) * sizeof(int32_t);
}

extern "C" int hsp_recon_chamfer_bwd(const float* recon, const float* G, const int32_t* idx1, const int32_t* idx2, const float* sym,
                                     const float* g, int B, int N, float w, float* gx, void* ws, size_t ws_bytes,
                                     hspStream_t stream) {
    if (!recon || !G || !idx1 || !idx2 || !sym || !g || !gx || B <= 0 || N <= 0 || !isfinite(w) || !ws ||
        ws_bytes < hsp_recon_chamfer_bwd_workspace_bytes(B, N))
        return HSP_ERR_BAD_ARG;
    if (!hsp_chamfer_bwd_ordered_ok(B, N, N)) return HSP_ERR_UNSUPPORTED;      // (nothing launched)
    int32_t* off = reinterpret_cast<int32_t*>(ws);             // ws: off (B,N+1) | edge (B,N): the reverse of idx2
    int32_t* edge = off + (size_t)B * (N + 1);
    int rc = hsp_rev_build(idx2, B, N, N, 1, 1, off, edge, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(recon_chamfer_grad_kernel, dim3((N + CH_ROWS_PER_WG - 1) / CH_ROWS_PER_WG, B), dim3(256), 0, as_stream(stream), recon, G, idx1, sym,
                       off, edge, g, w, (float)((long long)B * N), N, gx);
    return check_launch();
}

extern "C" size_t hsp_fps_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (size_t)B * N * sizeof(float);
}

extern "C" int hsp_fps_f32(const float* xyz, int B, int N, int n_samples, int32_t* sel, void* ws, size_t ws_bytes,
                           hspStream_t stream) {
    if (!xyz || !sel || B <= 0 || N <= 0 || n_samples <= 0 || n_samples > N) return HSP_ERR_BAD_ARG;
    if (!ws || ws_bytes < hsp_fps_workspace_bytes(B, N)) return HSP_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    const size_t lds = (size_t)N * 3 * sizeof(float);
#define FPS_REG(THREADS, PPT) return launch_lds(fps_reg_kernel<THREADS, PPT>, dim3(B), dim3(THREADS), lds, st, xyz, N, n_samples, sel)
    if (N <= 12288) {                                          // coordinates fit LDS (144 KB) and a few dozen registers
        if (N <= 64 * 2) FPS_REG(64, 2);
        if (N <= 256 * 2) FPS_REG(256, 2);
        if (N <= 256 * 5) FPS_REG(256, 5);                     // N = 1028 (128 x 10 and 512 x 3: 15 % slower)
        if (N <= 256 * 8) FPS_REG(256, 8);
        if (N <= 256 * 16) FPS_REG(256, 16);                   // N = 4096 (512 x 8 is as fast, 1024 x 4 is 40 % slower)
        if (N <= 1024 * 8) FPS_REG(1024, 8);
        FPS_REG(1024, 12);
    }
#undef FPS_REG
    hipLaunchKernelGGL(fps_generic_kernel<float>, dim3(B), dim3(FPS_THREADS), 0, st, xyz, N, n_samples, sel,
                       reinterpret_cast<float*>(ws));
    return check_launch();
}

extern "C" int hsp_fps_f64(const double* xyz, int B, int N, int n_samples, int32_t* sel, void* ws, size_t ws_bytes,
                           hspStream_t stream) {
    if (!xyz || !sel || B <= 0 || N <= 0 || n_samples <= 0 || n_samples > N) return HSP_ERR_BAD_ARG;
    if (!ws || ws_bytes < 2 * hsp_fps_workspace_bytes(B, N)) return HSP_ERR_WORKSPACE;
    hipLaunchKernelGGL(fps_generic_kernel<double>, dim3(B), dim3(FPS_THREADS), 0, as_stream(stream), xyz, N, n_samples,
                       sel, reinterpret_cast<double*>(ws));
    return check_launch();
}

// the register-resident kernel: a cloud's points in the registers of one workgroup, 1024 threads x 12 at the most
extern "C" int hsp_fps_levels_takes(int N0) { return N0 > 0 && N0 <= 12288 ? 1 : 0; }

extern "C" int hsp_fps_levels_f32(const float* xyz, int B, int N0, int N1, int N2, int32_t* sel1, float* v1, float* v2,
                                  hspStream_t stream) {
    if (!xyz || !sel1 || !v1 || B <= 0 || N0 <= 0 || N1 <= 0 || N1 > N0 || N2 < 0 || N2 > N1 || (N2 > 0 && !v2))
        return HSP_ERR_BAD_ARG;
    if (!hsp_fps_levels_takes(N0)) return HSP_ERR_UNSUPPORTED;   // (nothing launched)
    hipStream_t st = as_stream(stream);
    const size_t lds = (size_t)N0 * 3 * sizeof(float);
#define FPS_LV(THREADS, PPT) \
    return launch_lds(fps_levels_kernel<THREADS, PPT>, dim3(B), dim3(THREADS), lds, st, xyz, N0, N1, N2, sel1, v1, v2)
    if (N0 <= 64 * 2) FPS_LV(64, 2);                           // (the shapes of hsp_fps_f32's register kernel)
    if (N0 <= 256 * 2) FPS_LV(256, 2);
    if (N0 <= 256 * 5) FPS_LV(256, 5);
    if (N0 <= 256 * 8) FPS_LV(256, 8);
    if (N0 <= 256 * 16) FPS_LV(256, 16);
    if (N0 <= 1024 * 8) FPS_LV(1024, 8);
    FPS_LV(1024, 12);
#undef FPS_LV
}
