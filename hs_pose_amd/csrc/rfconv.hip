// rfconv.hip -- fused receptive-field graph convolution (3D-GCN style) for gfx950.
//
// Replaces HSlayer_surface.graph_conv / HS_layer.graph_conv of the reference
// (network/fs_net_repo/gcn3d.py:92-107, :158-181) together with the neighbour gather
// (gcn3d.py:39-47) and direction normalisation (gcn3d.py:49-59).  The reference materialises three
// (B,N,k,S*C) tensors per layer (1.18 GB each at B=16,N=1028,C=128); here a workgroup owns one
// point at a time, streams its k neighbour rows of the support tensor with 16-byte loads (the only
// large traffic, served from the XCD's L2: all workgroups of an XCD work on the same cloud), keeps
// the running max/arg-max in registers and writes only out (N,C) + arg-max bytes (N,S*C).
//
// Layout: column j of the S*C axis <-> (s = j / C, c = j % C)  (gcn3d.py:104,177).
// HBM-bound kernels: algorithmic bytes/point (fwd) = k*S*C*4 (gather, L2) + (S+1)*C*4/own row ... see DESIGN.md.
#include "common.h"
#include "folds.h"
#include "rf_dirs.h"
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

namespace hsp {

#define RF_THREADS 256
// forward workgroups per CU below 2048 / below 8192 points (rf_fwd, where the measurements stand; -D for the A/B)
#ifndef RF_FWD_WGS_TINY
#define RF_FWD_WGS_TINY 4
#endif
#ifndef RF_FWD_WGS_SMALL
#define RF_FWD_WGS_SMALL 4
#endif

// F.normalize(directions, dim=0) of the raw (3, S*C) parameter (rf_dirs.h: normalise_dirs, load_dirs_normed) is part of every
// kernel here, and its Jacobian is applied by rf_dirs_reduce_kernel.  Where the caller has bound a normalised table to the
// parameter (hsp_rf_dirs_hat_bind: a network's registry refreshes it once per forward, in the launch that splits its weights)
// the kernels load the table -- the same bits -- and a workgroup's prologue has no square root and no division left; with no
// table they normalise in the prologue.  `hat` below is that table or null.

// relu(theta) of the forward kernels.  theta = R^ . D^ is the cosine of two unit vectors, so relu == clamp to [0, 1] up to the
// rounding of the three-term chain: fmed3(x, 0, 1) is folded by the compiler into the LAST FMA as its clamp modifier
// (v_fma_f32 ... clamp) -- the 4 v_max of the 41 VALU instructions per (neighbour, float4) unit disappear (the kernel is
// VALU-issue-bound: measured 1.875 -> 1.852 ms per step at B=16 N=1028, 15.92 -> 15.68 ms on the bf16 dense clouds).  The one
// difference from max(x, 0): a theta that rounding pushed an ulp or two ABOVE 1 (a neighbour exactly along a support
// direction) reads 1.0 instead of 1.0000001 (2.4e-7 relative, inside every tolerance of section 2; NaN -> 0 either way).
// -DRF_RELU_MAX restores the plain max.
#ifdef RF_RELU_MAX
#define RF_RELU(X) fmaxf((X), 0.f)
#else
#define RF_RELU(X) __builtin_amdgcn_fmed3f((X), 0.f, 1.f)
#endif

// point schedule shared by all rf kernels: blocks of XCD x handle clouds x, x+8, ... one cloud at a
// time (keeps that cloud's fm rows resident in the XCD-private 4 MiB L2); purely a speed choice.
struct PointIter {
    int b0, bstep, i0, istep;
    __device__ __forceinline__ PointIter(int B) {
        const int xcd = blockIdx.x % HSP_NUM_XCD;
        const int local = blockIdx.x / HSP_NUM_XCD;
        const int per_xcd = gridDim.x / HSP_NUM_XCD;
        if (B >= HSP_NUM_XCD) {            // several clouds per XCD, visited one after the other
            b0 = xcd; bstep = HSP_NUM_XCD; i0 = local; istep = per_xcd;
        } else {                           // fewer clouds than XCDs: XCDs x, x+B, ... share cloud x % B
            b0 = xcd % B; bstep = B * HSP_NUM_XCD;   // (visited once)
            const int share = xcd / B;
            const int nshare = (HSP_NUM_XCD - b0 + B - 1) / B;
            i0 = local + per_xcd * share; istep = per_xcd * nshare;
        }
    }
};

// theta / z of one column: common.h's dot3_chain (the k-ordered fma chain of the reference's matmul, where the chain is spelled)
// on a neighbour direction and one column of the three direction rows.  Every rf kernel takes theta / z through here: the
// backward kernels' mask z > 0 has to reproduce the forward's relu(theta) bit for bit.
template <class R3>
__device__ __forceinline__ float rf_dot3(const R3 r, float d0, float d1, float d2) { return dot3_chain(r.x, r.y, r.z, d0, d1, d2); }

// the normalised directions of a thread's NCH column groups tid, tid + 256, ... (a slot past the last group reads group 0)
template <int NCH>
__device__ __forceinline__ void rf_load_dirs(const float* dirs, const float* hat, int SC, int tid, float4 (&d0)[NCH],
                                             float4 (&d1)[NCH], float4 (&d2)[NCH]) {
    const int nq = SC >> 2;
    const float* src = hat ? hat : dirs;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        const int cq = tid + u * RF_THREADS;
        load_dirs_raw(src, SC, (cq < nq ? cq : 0) << 2, d0[u], d1[u], d2[u]);
    }
    if (!hat) {
#pragma unroll
        for (int u = 0; u < NCH; ++u) normalise_dirs(d0[u], d1[u], d2[u]);
    }
}

// ------------------------------------------------------------------------------------------------
// forward.  SURFACE=true: out = mean_s max_n relu(z);  false: out = fm_c + mean_s max_n relu(z)*fm_support
// WF: also record the winners' support values (fwin)
// FT: storage type of fm / out / fwin (float, or bf16_t: arithmetic stays fp32, common.h Feat<>)
// Two schedules (rf_fwd_kernel, rf_fwd_pipe_kernel) around ONE arithmetic: rf_group_body and rf_mean_phase.
// ------------------------------------------------------------------------------------------------
// One (point, float4 column group): the running max / arg-max over the k neighbours in sR / sIdx, then the group's maxima to
// smax_j, the winning SOURCE ROWS m* = idx[b,i,n*] (uint16: the backward needs neither idx nor n) to arg_pj and, WF, the winners'
// support values to fwin_pj (the backward's direction gradient reads them as a stream instead of gathering 4-byte values from N
// rows: 4x the HBM traffic, measured).  fetch(n): the four support values fm[b, idx[n], C + j ..] -- the one thing the two
// schedules do differently.
template <bool SURFACE, bool WF, typename FT, class Fetch>
__device__ __forceinline__ void rf_group_body(const float4 d0, const float4 d1, const float4 d2, const float4* sR, const int* sIdx,
                                              int k, Fetch fetch, float* smax_j, uint16_t* arg_pj, FT* fwin_pj) {
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    float4 wf = make_float4(1.f, 1.f, 1.f, 1.f);          // the support value behind each winner
#pragma unroll 4
    for (int n = 0; n < k; ++n) {
        const float4 r = sR[n];
        float4 th;
        th.x = RF_RELU(rf_dot3(r, d0.x, d1.x, d2.x));
        th.y = RF_RELU(rf_dot3(r, d0.y, d1.y, d2.y));
        th.z = RF_RELU(rf_dot3(r, d0.z, d1.z, d2.z));
        th.w = RF_RELU(rf_dot3(r, d0.w, d1.w, d2.w));
        if (!SURFACE) {
            const float4 f = fetch(n);
            th.x = mul_rn(th.x, f.x); th.y = mul_rn(th.y, f.y);
            th.z = mul_rn(th.z, f.z); th.w = mul_rn(th.w, f.w);
            if (WF) {
                if (th.x > best.x) wf.x = f.x;
                if (th.y > best.y) wf.y = f.y;
                if (th.z > best.z) wf.z = f.z;
                if (th.w > best.w) wf.w = f.w;
            }
        }
        if (th.x > best.x) { best.x = th.x; a0 = n; }
        if (th.y > best.y) { best.y = th.y; a1 = n; }
        if (th.z > best.z) { best.z = th.z; a2 = n; }
        if (th.w > best.w) { best.w = th.w; a3 = n; }
    }
    *reinterpret_cast<float4*>(smax_j) = best;
    // fwin / argrow / out are write-once streams read again only by the backward: non-temporal stores keep them from evicting
    // the cloud's fm rows (the gather's working set) from the XCD's L2
    {
        const unsigned lo = (unsigned)sIdx[a0] | ((unsigned)sIdx[a1] << 16);
        const unsigned hi = (unsigned)sIdx[a2] | ((unsigned)sIdx[a3] << 16);
        unsigned* ap = reinterpret_cast<unsigned*>(arg_pj);
        __builtin_nontemporal_store(lo, ap); __builtin_nontemporal_store(hi, ap + 1);
    }
    if (WF) Feat<FT>::st4_nt(fwin_pj, wf);
}

// out[pt] = (fm_c[pt] +) the mean over the S supports of the point's maxima
template <bool SURFACE, typename FT>
__device__ __forceinline__ void rf_mean_phase(const float* smax, const FT* fm, FT* out, size_t pt, int S,
                                              int C, float invS_div, int tid) {      // invS_div = (float)S
    const int fstride = (S + 1) * C;
    for (int c = tid; c < C; c += RF_THREADS) {
        float s = smax[c];
        for (int sp = 1; sp < S; ++sp) s = add_rn(s, smax[sp * C + c]);
        float v = __fdiv_rn(s, invS_div);
        if (!SURFACE) v = add_rn(Feat<FT>::ld(fm + pt * fstride + c), v);
        Feat<FT>::st_nt(out + pt * C + c, v);
    }
}

// The plain schedule: a point in three phases separated by barriers.  dynamic LDS: (S*C + 4*k + k) floats
template <bool SURFACE, int NCH, bool WF, typename FT>
__global__ __launch_bounds__(RF_THREADS) void rf_fwd_kernel(const float* __restrict__ xyz,
                                                            const int32_t* __restrict__ idx,
                                                            const float* __restrict__ dirs,
                                                            const float* __restrict__ hat,
                                                            const FT* __restrict__ fm, int B, int N, int k,
                                                            int S, int C, FT* __restrict__ out,
                                                            uint16_t* __restrict__ argrow,
                                                            FT* __restrict__ fwin) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int SC = S * C;
    float* smax = reinterpret_cast<float*>(smem);             // SC
    float4* sR = reinterpret_cast<float4*>(smax + SC);        // k  (unit direction, w unused)
    int* sIdx = reinterpret_cast<int*>(sR + k);               // k
    const int tid = threadIdx.x;
    const int nq = SC >> 2;                                   // float4 columns
    const int fstride = (S + 1) * C;
    const float invS_div = (float)S;
    float4 d0[NCH], d1[NCH], d2[NCH];
    rf_load_dirs<NCH>(dirs, hat, SC, tid, d0, d1, d2);
    const PointIter it(B);
    for (int b = it.b0; b < B; b += it.bstep) {
        const float* xb = xyz + (size_t)b * N * 3;
        for (int i = it.i0; i < N; i += it.istep) {
            const size_t pt = (size_t)b * N + i;
            __syncthreads();                                   // previous point's LDS reads are done
            for (int t = tid; t < k; t += RF_THREADS) {         // (k may exceed the workgroup: the host bounds only the LDS)
                const int m = idx[pt * k + t];
                sIdx[t] = m;
                const float3 r = unit_dir(xb[i * 3], xb[i * 3 + 1], xb[i * 3 + 2], xb[m * 3], xb[m * 3 + 1], xb[m * 3 + 2]);
                sR[t] = make_float4(r.x, r.y, r.z, 0.f);
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NCH; ++u) {
                const int cq = tid + u * RF_THREADS;
                if (cq < nq) {
                    const int j = cq << 2;
                    const FT* fsup = SURFACE ? nullptr : fm + (size_t)b * N * fstride + C + j;
                    auto fetch = [=](int n) { return Feat<FT>::ld4(fsup + (size_t)sIdx[n] * fstride); };     // a pointer gather
                    rf_group_body<SURFACE, WF, FT>(d0[u], d1[u], d2[u], sR, sIdx, k, fetch, smax + j, argrow + pt * SC + j,
                                                   WF ? fwin + pt * SC + j : nullptr);
                }
            }
            __syncthreads();
            rf_mean_phase<SURFACE, FT>(smax, fm, out, pt, S, C, invS_div, tid);
        }
    }
}


// ------------------------------------------------------------------------------------------------
// forward, PIPELINED over the points of a workgroup (the default schedule).  rf_fwd_kernel spends a point in three phases
// separated by barriers: k threads fetch the neighbour list and build the unit directions (two dependent global round
// trips while 236 threads wait), everybody gathers, C threads average the S maxima.  Here the three phases of three
// consecutive points share ONE barrier interval: the threads that have no column group in the last of the NCH slots
// (S*C/4 = 224 groups on 256 threads at C = 128) build the directions of point i+1 into the other half of a double
// buffer while the gather of point i runs, and the average of point i-1 is taken from the other maxima buffer at the
// start of the interval.  The arithmetic is rf_fwd_kernel's by construction; no shape runs under both schedules (hsp_rf_fwd_plan
// picks one per (k, S, C)), so tests/test_gpu_rf_reference.py holds each of them to the same fp64 reference and asserts the plan
// it entered.
// dynamic LDS: 2 * (S*C + 6 k) floats.  Needs S*C/4 - (NCH-1)*256 + k <= 256.
// ------------------------------------------------------------------------------------------------
template <bool SURFACE, int NCH, bool WF, typename FT>
__global__ __launch_bounds__(RF_THREADS) void rf_fwd_pipe_kernel(const float* __restrict__ xyz,
                                                                 const int32_t* __restrict__ idx,
                                                                 const float* __restrict__ dirs,
                                                                 const float* __restrict__ hat,
                                                                 const FT* __restrict__ fm, int B, int N, int k,
                                                                 int S, int C, FT* __restrict__ out,
                                                                 uint16_t* __restrict__ argrow,
                                                                 FT* __restrict__ fwin) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int SC = S * C;
    float* smax2 = reinterpret_cast<float*>(smem);            // 2 x SC
    float4* sR2 = reinterpret_cast<float4*>(smax2 + 2 * SC);  // 2 x k
    int* sIdx2 = reinterpret_cast<int*>(sR2 + 2 * k);         // 2 x k
    unsigned* sOff2 = reinterpret_cast<unsigned*>(sIdx2 + 2 * k);   // 2 x k: the neighbour row's byte offset in the cloud's fm
    const int tid = threadIdx.x;
    const int nq = SC >> 2;
    const int fstride = (S + 1) * C;
    const int spare0 = nq - (NCH - 1) * RF_THREADS;           // first thread without a group in the last slot
    const float invS_div = (float)S;
    float4 d0[NCH], d1[NCH], d2[NCH];
    rf_load_dirs<NCH>(dirs, hat, SC, tid, d0, d1, d2);
    const PointIter it(B);
    auto dirs_phase = [&](int b, int i, int buf) {
        const int t = tid - spare0;
        if (t >= 0 && t < k) {
            const float* xb = xyz + (size_t)b * N * 3;
            const int m = idx[((size_t)b * N + i) * k + t];
            sIdx2[buf * k + t] = m;
            sOff2[buf * k + t] = (unsigned)m * (unsigned)fstride * (unsigned)sizeof(FT);
            const float3 r = unit_dir(xb[i * 3], xb[i * 3 + 1], xb[i * 3 + 2], xb[m * 3], xb[m * 3 + 1], xb[m * 3 + 2]);
            sR2[buf * k + t] = make_float4(r.x, r.y, r.z, 0.f);
        }
    };
    int b = it.b0, i = it.i0;
    bool have = b < B && i < N;
    if (have) dirs_phase(b, i, 0);
    int cur = 0;
    bool have_prev = false;
    size_t prev_pt = 0;
    while (have) {
        int nb = b, ni = i + it.istep;
        if (ni >= N) { nb = b + it.bstep; ni = it.i0; }
        const bool have_next = nb < B;
        const size_t pt = (size_t)b * N + i;
        __syncthreads();        // directions of this point are in place; the previous point's maxima are complete
        if (have_prev) rf_mean_phase<SURFACE, FT>(smax2 + (cur ^ 1) * SC, fm, out, prev_pt, S, C, invS_div, tid);
        if (have_next) dirs_phase(nb, ni, cur ^ 1);
        float* smax = smax2 + cur * SC;
        const float4* sR = sR2 + cur * k;
        const int* sIdx = sIdx2 + cur * k;
        const unsigned* sOff = sOff2 + cur * k;
#pragma unroll
        for (int u = 0; u < NCH; ++u) {
            const int cq = tid + u * RF_THREADS;
            if (cq < nq) {
                const int j = cq << 2;
                // gathers through a buffer descriptor over the cloud's fm: address = base + 32-bit (column + row) byte offset, one
                // v_add per gather instead of a 64-bit multiply-add
                // (the base goes through v_readfirstlane: hipcc does not see that the cloud index is wave-uniform and would wrap
                // every load in a waterfall loop over the descriptor)
                const unsigned long long fbase = reinterpret_cast<unsigned long long>(SURFACE ? out : fm + (size_t)b * N * fstride);
                FT* ubase = reinterpret_cast<FT*>(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(fbase >> 32)) << 32) |
                                                  (unsigned)__builtin_amdgcn_readfirstlane((unsigned)fbase));
                const __amdgpu_buffer_rsrc_t frs =
                    __builtin_amdgcn_make_buffer_rsrc(ubase, 0, (int)((size_t)N * fstride * sizeof(FT)), 0x00020000);
                const unsigned voff = (unsigned)(C + j) * (unsigned)sizeof(FT);
                auto fetch = [=](int n) {
                    if constexpr (sizeof(FT) == 4) {
                        const auto v = __builtin_amdgcn_raw_buffer_load_b128(frs, (int)(voff + sOff[n]), 0, 0);
                        return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
                    } else {
                        const auto v = __builtin_amdgcn_raw_buffer_load_b64(frs, (int)(voff + sOff[n]), 0, 0);
                        return bf16x4_to_f32(make_uint2(v[0], v[1]));
                    }
                };
                rf_group_body<SURFACE, WF, FT>(d0[u], d1[u], d2[u], sR, sIdx, k, fetch, smax + j,
                                               argrow + pt * SC + j, WF ? fwin + pt * SC + j : nullptr);
            }
        }
        have_prev = true; prev_pt = pt;
        cur ^= 1;
        b = nb; i = ni; have = have_next;
    }
    __syncthreads();
    if (have_prev) rf_mean_phase<SURFACE, FT>(smax2 + (cur ^ 1) * SC, fm, out, prev_pt, S, C, invS_div, tid);
}

// ------------------------------------------------------------------------------------------------
// backward of HS_layer.graph_conv, GATHER form (no atomics, fixed summation order).
// A workgroup owns one SOURCE row m at a time and walks the reverse-edge list of m (csr.hip):
// for every edge e = i*k + n with idx[b,i,n] == m and every column j
//     hit = (argrow[b,i,j] == m);  z = R(i->m) . dirs[:,j];  ga = g[b,i,j%C] / S
//     grad_fm[b,m,C+j] += hit ? ga * relu(z) : 0
//     gD[d][j]         += hit && z>0 ? ga * fm[b,m,C+j] * R[d] : 0        (registers -> ws partials)
// grad_fm[b,m,c] = g[b,m,c] (centre).  Edges are staged EB at a time in LDS (unit direction, slot n,
// the query's g row pre-scaled by 1/S) so the EB arg-max loads of a thread are independent.
// dynamic LDS: EB*(C + 8) floats
// ------------------------------------------------------------------------------------------------
#define RF_EB 8

template <int NCH>
__global__ __launch_bounds__(RF_THREADS) void rf_conv_bwd_csr_kernel(
    const float* __restrict__ xyz, const float* __restrict__ dirs, const float* __restrict__ hat, const float* __restrict__ fm,
    const uint16_t* __restrict__ argrow, const float* __restrict__ gout, const int32_t* __restrict__ rev_off,
    const int32_t* __restrict__ rev_edge, int B, int N, int k, int S, int C, float* __restrict__ gfm,
    float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int SC = S * C;
    float* sg = reinterpret_cast<float*>(smem);                       // RF_EB x C   (g[i] / S)
    float4* sR = reinterpret_cast<float4*>(sg + RF_EB * C);           // RF_EB       (R.xyz, w = slot n as int bits)
    int* sI = reinterpret_cast<int*>(sR + RF_EB);                     // RF_EB       query row i
    const int tid = threadIdx.x;
    const int nq = SC >> 2;
    const int fstride = (S + 1) * C;
    const float invS = 1.0f / (float)S;
    const int cq4 = C >> 2;

    float4 d0[NCH], d1[NCH], d2[NCH], gd0[NCH], gd1[NCH], gd2[NCH];
    rf_load_dirs<NCH>(dirs, hat, SC, tid, d0, d1, d2);
#pragma unroll
    for (int u = 0; u < NCH; ++u) gd0[u] = gd1[u] = gd2[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    const PointIter it(B);
    for (int b = it.b0; b < B; b += it.bstep) {
        const float* xb = xyz + (size_t)b * N * 3;
        const int32_t* offb = rev_off + (size_t)b * (N + 1);
        const int32_t* edgeb = rev_edge + (size_t)b * N * k;
        for (int m = it.i0; m < N; m += it.istep) {
            const size_t pm = (size_t)b * N + m;
            const int o0 = offb[m], o1 = offb[m + 1];
            const float mx = xb[m * 3], my = xb[m * 3 + 1], mz = xb[m * 3 + 2];
            float4 fv[NCH], acc[NCH];
#pragma unroll
            for (int u = 0; u < NCH; ++u) {
                const int cq = tid + u * RF_THREADS;
                acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                fv[u] = cq < nq ? *reinterpret_cast<const float4*>(fm + pm * fstride + C + (cq << 2)) : acc[u];
            }
            for (int c = tid; c < C; c += RF_THREADS) gfm[pm * fstride + c] = gout[pm * C + c];   // centre
            for (int e0 = o0; e0 < o1; e0 += RF_EB) {
                const int ne = min(RF_EB, o1 - e0);
                __syncthreads();                                   // previous batch consumed
                if (tid < ne) {
                    const int e = edgeb[e0 + tid];
                    const int i = e / k, n = e - i * k;
                    const float3 r = unit_dir(xb[i * 3], xb[i * 3 + 1], xb[i * 3 + 2], mx, my, mz);
                    sR[tid] = make_float4(r.x, r.y, r.z, __int_as_float(n));
                    sI[tid] = i;
                }
                __syncthreads();
                for (int q = tid; q < ne * cq4; q += RF_THREADS) {   // stage the g rows, scaled by 1/S
                    const int t = q / cq4, c4 = q - t * cq4;
                    float4 g = *reinterpret_cast<const float4*>(gout + ((size_t)b * N + sI[t]) * C + (c4 << 2));
                    g.x *= invS; g.y *= invS; g.z *= invS; g.w *= invS;
                    *reinterpret_cast<float4*>(sg + t * C + (c4 << 2)) = g;
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    const int cq = tid + u * RF_THREADS;
                    if (cq < nq) {
                        const int j = cq << 2;
                        const int c = j % C;
                        ushort4 am[RF_EB];
#pragma unroll
                        for (int t = 0; t < RF_EB; ++t)     // clamped slot instead of a branch around the load
                            am[t] = *reinterpret_cast<const ushort4*>(argrow + ((size_t)b * N + sI[t < ne ? t : 0]) * SC + j);
#pragma unroll
                        for (int t = 0; t < RF_EB; ++t) {
                            if (t < ne) {
                                const float4 r = sR[t];
                                const int n = m;                    // a hit is "the winner of (i,j) is this row"
                                const float4 ga = *reinterpret_cast<const float4*>(sg + t * C + c);
#define RF_ONE(X)                                                                                         \
    if (am[t].X == n) {                                                                                   \
        const float z = rf_dot3(r, d0[u].X, d1[u].X, d2[u].X);                                            \
        if (z > 0.f) {                                                                                    \
            acc[u].X += ga.X * z;                                                                         \
            const float w = ga.X * fv[u].X;                                                               \
            gd0[u].X += w * r.x; gd1[u].X += w * r.y; gd2[u].X += w * r.z;                                \
        }                                                                                                 \
    }
                                RF_ONE(x) RF_ONE(y) RF_ONE(z) RF_ONE(w)
#undef RF_ONE
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < NCH; ++u) {
                const int cq = tid + u * RF_THREADS;
                if (cq < nq) *reinterpret_cast<float4*>(gfm + pm * fstride + C + (cq << 2)) = acc[u];
            }
        }
    }
    float* wsb = ws + (size_t)blockIdx.x * 3 * SC;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        const int cq = tid + u * RF_THREADS;
        if (cq < nq) {
            const int j = cq << 2;
            *reinterpret_cast<float4*>(wsb + j) = gd0[u];
            *reinterpret_cast<float4*>(wsb + SC + j) = gd1[u];
            *reinterpret_cast<float4*>(wsb + 2 * SC + j) = gd2[u];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward, COLUMN-TILE LDS-SCATTER form (default for HS_layer.graph_conv; SURFACE = the surface layer,
// which has only the direction gradient).
// One workgroup per (cloud b, tile of TC support columns).  The tile of grad_fm, acc[N][TC] fp32, and the
// cloud's xyz live in LDS (66 KB + 12 KB at N=1028, TC=16); the workgroup sweeps the cloud's points i and,
// for each column j of the tile, reads the winning source row m = argrow[b,i,j] (coalesced), rebuilds
// R(i->m) from the LDS copy of xyz, and routes  ga*relu(z)  to acc[m] with an LDS atomic add
// (ds_add_f32: no L2 round trip; hub rows of feature-space KNN graphs only serialise inside one wave);
// every grad_fm row segment is then written once with 16-byte stores.  The fm[b,m,C+j] value per element
// that the direction gradient needs comes from fwin[b,i,j], stored by the forward next to argrow (a stream,
// where gathering it from fm fetched a 64-byte sector per 4-byte value).  That gradient is
// accumulated in registers, folded across the workgroup's point lanes in LDS in a fixed order and written
// to gd_part[b][3][SC] (one writer per element); rf_dirs_reduce_kernel sums the B clouds.
// (hsp_rf_conv_bwd, the CSR form, is the gather twin; both are bit-reproducible now that the tile adds integers.)
// grid (SC/TC, B), block 512, dynamic LDS = max(N*TC (acc) + 3N (xyz), 512*12) floats
// ------------------------------------------------------------------------------------------------
#ifndef RF_BWD_CLOUD_PER_XCD
#define RF_BWD_CLOUD_PER_XCD 1     // 0: only groups of 4 adjacent tiles share an XCD (measured 65.3 vs 60.7 us at N = 1028)
#endif
#define RF_TILE_THREADS 512   // 8 waves: with one 78 KB tile per workgroup this doubles the waves per CU
// The tile accumulates in 32-bit FIXED POINT: ds_add_u32 retires ~24x the lanes per clock of ds_add_f32 on gfx950
// (tools/ubench/lds_atomic.hip), and with the winners' support values streamed (fwin) the float adds were what the
// cache-resident layers waited on (measured: 52.7 -> 28.1 us at N = 257, C = 256; 83 -> 72 us at N = 1028).  The scale is
// private to the workgroup -- a power of two chosen from the largest |grad_out| / S of the columns this tile reads, with
// ceil(log2 N) bits of headroom: a (row, column) cell receives at most one term per point and every term is bounded by that
// maximum (|theta| <= 1), so the sum cannot overflow; a term is rounded to 2^-(30 - log2 N) of the tile's largest one (1.2e-7
// at N = 257, 1e-6 at N = 1028 -- the fp32 adds it replaces carried the same order) and the integer sum is exact and
// order-independent: the scatter form is now bit-reproducible as well.
#define RF_ACC_ADD(P, V) atomicAdd(reinterpret_cast<int*>(P), __float2int_rn((V) * fx_scale))

// The tile's fixed-point scale from a thread's max |grad_out| over the rows it visits: folded over the workgroup (fmaxf drops a
// NaN, so the fold's order cannot matter), / S, then the power of two that leaves ceil(log2 N) bits of headroom.
// Holds one __syncthreads.
__device__ __forceinline__ void rf_tile_scale(float vm, float invS, int N, float* wmax, int tid, float& fx_scale, float& fx_inv) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vm = fmaxf(vm, __shfl_xor(vm, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = vm;
    __syncthreads();
    vm = wmax[0];
#pragma unroll
    for (int w = 1; w < RF_TILE_THREADS / 64; ++w) vm = fmaxf(vm, wmax[w]);
    vm *= invS;
    if (vm > 0.f && vm < 3.0e38f) {            // (0 / inf / NaN gradients: scale 1 -- nothing sensible to preserve)
        int ex;
        frexpf(vm, &ex);                        // vm < 2^ex
        int lg = 0;
        while ((1 << lg) < N) ++lg;
        int e = 30 - ex - lg;
        e = e > 126 ? 126 : (e < -126 ? -126 : e);      // (2^e and 2^-e both normal floats; |grad| / S down to ~2^-96 keeps the full quantum)
        fx_scale = ldexpf(1.f, e);
        fx_inv = ldexpf(1.f, -e);
    }
}

__device__ __forceinline__ float absmax4(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

// four values of a row AS LOADED: the batched schedule keeps these in its register batches and widens a bf16 piece where it is
// used, so that no conversion stands between a load and the loads issued after it
template <typename FT> struct Raw4;
template <> struct Raw4<float> {
    typedef float4 T;
    static __device__ __forceinline__ T ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ float4 wide(T v) { return v; }
    static __device__ __forceinline__ void st(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
};
template <> struct Raw4<bf16_t> {
    typedef uint2 T;
    static __device__ __forceinline__ T ld(const bf16_t* p) { return *reinterpret_cast<const uint2*>(p); }
    static __device__ __forceinline__ float4 wide(T u) { return bf16x4_to_f32(u); }
    static __device__ __forceinline__ void st(bf16_t* p, T v) { *reinterpret_cast<uint2*>(p) = v; }
};
typedef float rf_v4f __attribute__((ext_vector_type(4)));

// (cloud, column tile) of a workgroup of rf_bwd_tile_kernel's grid (T column tiles, B clouds[, row ranges]).  Neighbouring column
// tiles read neighbouring 32- / 64-byte pieces of the same argrow / fwin / grad_out lines; dispatched round-robin over the 8 XCDs
// each piece was fetched into another L2 (measured: 340 MB of HBM traffic for 164 MB algorithmic at N = 1028).  So: every tile of a
// cloud on ONE XCD where B % 8 == 0 (grad_out is shared by its S tiles too), else groups of 4 adjacent tiles per XCD where they
// divide evenly, as consecutive workgroups of it (block id = XCD + 8 k, observed placement), else the plain order.  A speed choice
// only; tests/test_gpu_rf_reference.py restates which of the three a shape takes as _wg_map.
__device__ __forceinline__ void rf_bwd_wg_map(int& b, int& tile) {
    b = blockIdx.y; tile = blockIdx.x;
    const int T = gridDim.x, ngrp = (T >> 2) * (int)gridDim.y;
    if (RF_BWD_CLOUD_PER_XCD && ((int)gridDim.y & 7) == 0) {
        const int L = blockIdx.x + T * blockIdx.y;
        const int xcd = L & 7, k = L >> 3;
        b = xcd + 8 * (k / T);
        tile = k - (k / T) * T;
    } else if ((T & 3) == 0 && (ngrp & 7) == 0) {
        const int L = blockIdx.x + T * blockIdx.y;
        const int xcd = L & 7, k = L >> 3;
        const int gid = xcd + 8 * (k >> 2);
        b = gid / (T >> 2);
        tile = 4 * (gid - b * (T >> 2)) + (k & 3);
    }
}

// one point's four columns: route ga * relu(theta) to the winning rows' cells, add to the direction gradient
#define RF_T1(X, E, FV)                                                                              \
        {                                                                                            \
            const int m = (int)am.X - r0;                                                            \
            if (RS == 1 || (unsigned)m < (unsigned)(r1 - r0)) {                                      \
                const float3 r = unit_dir_fast(px, py, pz, sx[m * 3], sx[m * 3 + 1], sx[m * 3 + 2]); \
                const float z = rf_dot3(r, d0.X, d1.X, d2.X);                                        \
                if (z > 0.f) {                                                                       \
                    if (!SURFACE) RF_ACC_ADD(accg + m * TC + E, ga.X * z);                           \
                    const float w = ga.X * FV;                                                       \
                    g0.X += w * r.x; g1.X += w * r.y; g2.X += w * r.z;                               \
                }                                                                                    \
            }                                                                                        \
        }

// FWIN: the support values come from the forward's fwin stream; else they are gathered from fm (fine while a
// cloud's fm stays L2-resident: small N)
// RS > 1 (dense clouds: N = 4096): the tile holds only the source rows [r0, r0 + N/RS) of the cloud -- RS workgroups (grid z)
// sweep the same points and each keeps the elements whose winning row falls in its range.  What LDS buys is bytes of
// accumulator: lines touched per launch = N * SC * RS / TC, and acc = (N / RS) * TC * 4 bytes, so two 128 KB half-cloud
// tiles of 16 columns touch half the lines of one 64 KB whole-cloud tile of 4 (the only whole-cloud width that fits).
// D, RG: the SCHEDULE (what is computed, and in which order each thread adds, is the same under every value):
//   D = 0   the first form ("legacy", hsp_rf_bwd_set_schedule(1)): every phase a loop of one load and its wait -- staging xyz,
//           the scale's pass over grad_out, a sweep that prefetches one point ahead and reads grad_out a second time, and the
//           centre columns copied by the first C / TC tiles of a cloud after their flush.
//   D > 0   the batched form: every independent load of the set-up -- directions, xyz, the centre columns' share, the scale
//           pass's grad_out rows, the sweep's first D stages -- is issued as fixed-size register batches with clamped addresses
//           BEFORE anything waits (the tile is zeroed under that one round trip); the sweep runs
//           a D-deep register ring of (argrow, fwin[, grad_out][, the point]) stages, unrolled by D so that it rotates by
//           renaming; the centre columns are spread over all tiles of the cloud.
//   RG > 0  (D > 0, not SURFACE, RS == 1, ceil(N / PL) <= RG): the scale pass's grad_out rows ARE the sweep's -- same thread,
//           same rows, same columns -- so they stay in registers and the sweep, fully unrolled, has no grad_out stream.
//   RG = 0  grad_out travels in the ring; the scale pass is batched rf_max_batch rows deep.
// rows per batch of the scale pass where grad_out is not resident (the half-cloud form: N = 4096, 32 rows per thread)
__host__ __device__ constexpr int rf_max_batch(int tc) { return tc >= 32 ? 4 : 8; }
// xyz floats per thread and batch (16 columns at N = 1028: 3084 floats over 512 threads, one batch; a 32- / 64-column tile holds
// at most 585 / 305 points and has fewer registers to spend), centre-column pieces per thread and batch (N = 1028, C = 128: 588
// per tile; N = 257, C = 256: 294)
__host__ __device__ constexpr int rf_xyz_batch(int tc) { return tc == 64 ? 2 : (tc == 32 ? 4 : 8); }
__host__ __device__ constexpr int rf_centre_batch(int tc) { return tc >= 32 ? 1 : 2; }
// waves per SIMD the batched form must keep (it has more in flight than the legacy form, and hipcc spends registers freely up
// to the launch bound): 4 = two workgroups per CU where the LDS tile allows no more (16 columns at N = 1028: 128 VGPRs); 6 = the
// three workgroups per CU of the 32- / 64-column tiles (80 VGPRs); 8 = four for the surface kernel, which has no tile (64 VGPRs)
__host__ __device__ constexpr int rf_tile_waves(int tc, bool surface, int rs, int d) {
    return d == 0 || rs > 1 ? 1 : (surface ? 8 : (tc >= 32 ? 6 : 4));
}
template <int TC, bool SURFACE, bool FWIN, typename FT, int RS = 1, int D = 0, int RG = 0>
__global__ __launch_bounds__(RF_TILE_THREADS, rf_tile_waves(TC, SURFACE, RS, D)) void rf_bwd_tile_kernel(
    const float* __restrict__ xyz, const float* __restrict__ dirs, const float* __restrict__ hat, const FT* __restrict__ fwin,
    const uint16_t* __restrict__ argrow, const FT* __restrict__ gout, int B, int N, int S, int C,
    FT* __restrict__ gfm, float* __restrict__ gd_part) {
    static_assert(RG == 0 || (D > 0 && !SURFACE && RS == 1), "resident grad_out rows: batched whole-cloud conv tiles only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wmax[RF_TILE_THREADS / 64];
    const int NR = RS > 1 ? (N + RS - 1) / RS : N;                     // source rows of this tile
    const int r0 = RS > 1 ? (int)blockIdx.z * NR : 0;
    const int r1 = min(N, r0 + NR);
    float* acc = reinterpret_cast<float*>(smem);                       // NR*TC   (unused when SURFACE)
    float* sx = acc + (SURFACE ? 0 : (size_t)NR * TC);                 // 3*NR: xyz of the source rows (RS == 1: of all points)
    constexpr int G = TC / 4;                 // float4 groups per tile
    constexpr int PL = RF_TILE_THREADS / G;        // point lanes
    const int SC = S * C;
    const int fstride = (S + 1) * C;
    const int tid = threadIdx.x;
    int b, tile;
    rf_bwd_wg_map(b, tile);
    const int j0 = tile * TC;
    const int cg = tid % G, pl = tid / G;
    const int j = j0 + cg * 4;
    const int c = j % C;
    const float invS = 1.0f / (float)S;
    const float* xb = xyz + (size_t)b * N * 3;
    float fx_scale = 1.f, fx_inv = 1.f;
    float4 d0, d1, d2;
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, g2 = g0;
    const FT* fsup = (SURFACE || FWIN) ? nullptr : fwin + (size_t)b * N * fstride + C + j;   // (fwin is fm then)
    // One point p of the sweep, under either schedule: am = its four winning rows, gq = its grad_out values, fw = their support
    // values from the fwin stream (FWIN), ps = the point's coordinates as streamed by the schedule (RS > 1; the whole-cloud tile
    // has them in sx).  accg = acc + cg * 4, this thread's columns of the tile, handed in by the caller: written inside this
    // body the sum moved the legacy kernels' address code; operands by reference for the same reason.
    auto point = [&](float* accg, const ushort4& am, const float4& gq, const float4& fw, const float3& ps, int p) {
        float4 ga = gq;
        float f0 = 1.f, f1 = 1.f, f2 = 1.f, f3 = 1.f;              // (SURFACE: no support value)
        if (!SURFACE && FWIN) { f0 = fw.x; f1 = fw.y; f2 = fw.z; f3 = fw.w; }
        if (!SURFACE && !FWIN) {
            f0 = Feat<FT>::ld(fsup + (size_t)am.x * fstride + 0);
            f1 = Feat<FT>::ld(fsup + (size_t)am.y * fstride + 1);
            f2 = Feat<FT>::ld(fsup + (size_t)am.z * fstride + 2);
            f3 = Feat<FT>::ld(fsup + (size_t)am.w * fstride + 3);
        }
        ga.x *= invS; ga.y *= invS; ga.z *= invS; ga.w *= invS;
        float px, py, pz;
        if (RS > 1) { px = ps.x; py = ps.y; pz = ps.z; }
        else { px = sx[p * 3]; py = sx[p * 3 + 1]; pz = sx[p * 3 + 2]; }
        RF_T1(x, 0, f0) RF_T1(y, 1, f1) RF_T1(z, 2, f2) RF_T1(w, 3, f3)
    };
#undef RF_T1
    if constexpr (D > 0) {
        typedef typename Raw4<FT>::T RawT;
        constexpr int RF_XB = rf_xyz_batch(TC), RF_CB = rf_centre_batch(TC);
        constexpr bool RES = RG > 0;
        constexpr int NG = RES ? RG : rf_max_batch(TC);          // grad_out rows of the set-up batch
        constexpr int NST = RES ? RG : D;               // stage registers (RES: one per sweep iteration, D of them in flight)
        const size_t row0 = (size_t)b * N;
        const int nlast = N - 1;
        struct Stage { ushort4 am; RawT fw, ga; float px, py, pz; };
        auto load_stage = [&](int p) {                  // clamped: no branch around the loads
            Stage s;
            p = p < nlast ? p : nlast;
            s.am = *reinterpret_cast<const ushort4*>(argrow + (row0 + p) * SC + j);
            s.fw = RawT(); s.ga = RawT(); s.px = s.py = s.pz = 0.f;
            if (!SURFACE && FWIN) s.fw = Raw4<FT>::ld(fwin + (row0 + p) * SC + j);
            if (!RES) s.ga = Raw4<FT>::ld(gout + (row0 + p) * C + c);
            if (RS > 1) { s.px = xb[p * 3]; s.py = xb[p * 3 + 1]; s.pz = xb[p * 3 + 2]; }   // the point itself: a coalesced stream
            return s;
        };
        // ---- 1. issue: nothing below waits before the last of these loads is out
        load_dirs_raw(hat ? hat : dirs, SC, j, d0, d1, d2);
        const int n3 = 3 * (r1 - r0);
        const float* xsrc = xb + r0 * 3;
        float xv[RF_XB];
#pragma unroll
        for (int u = 0; u < RF_XB; ++u) {
            const int q = tid + u * RF_TILE_THREADS;
            xv[u] = xsrc[q < n3 ? q : n3 - 1];
        }
        // the centre columns grad_fm[b,m,c] = g[b,m,c] of this tile's rows, in 4-value pieces: every tile of the cloud copies an
        // equal, contiguous share of them
        const int C4 = C >> 2, Q = (r1 - r0) * C4, per = (Q + (int)gridDim.x - 1) / (int)gridDim.x;
        const int q_lo = tile * per, q_hi = min(Q, q_lo + per);
        RawT cv[RF_CB];
        size_t cdst[RF_CB];
        auto centre_load = [&](int qb) {
#pragma unroll
            for (int u = 0; u < RF_CB; ++u) {
                int q = qb + tid + u * RF_TILE_THREADS;
                q = q < Q ? q : Q - 1;
                const int m = q / C4, c4 = q - m * C4;
                cv[u] = Raw4<FT>::ld(gout + (row0 + r0 + m) * C + c4 * 4);
                cdst[u] = (row0 + r0 + m) * fstride + c4 * 4;
            }
        };
        auto centre_store = [&](int qb) {
#pragma unroll
            for (int u = 0; u < RF_CB; ++u)
                if (qb + tid + u * RF_TILE_THREADS < q_hi) Raw4<FT>::st(gfm + cdst[u], cv[u]);
        };
        RawT gres[NG];
        if (!SURFACE) {
            centre_load(q_lo);
#pragma unroll
            for (int t = 0; t < NG; ++t) {
                const int p = pl + t * PL;
                gres[t] = Raw4<FT>::ld(gout + (row0 + (p < nlast ? p : nlast)) * C + c);
            }
        }
        Stage st[NST];
#pragma unroll
        for (int u = 0; u < (D < NST ? D : NST); ++u) st[u] = load_stage(pl + u * PL);
        // ---- 2. under that round trip: zero the tile (one 128-bit LDS store per piece)
        if (!SURFACE)
            for (int q = tid; q < NR * G; q += RF_TILE_THREADS) *reinterpret_cast<rf_v4f*>(acc + q * 4) = rf_v4f{0.f, 0.f, 0.f, 0.f};
        // ---- 3. consume
#pragma unroll
        for (int u = 0; u < RF_XB; ++u) {
            const int q = tid + u * RF_TILE_THREADS;
            if (q < n3) sx[q] = xv[u];
        }
        for (int q0 = tid + RF_XB * RF_TILE_THREADS; q0 < n3; q0 += RF_XB * RF_TILE_THREADS) {      // (N > 1365)
#pragma unroll
            for (int u = 0; u < RF_XB; ++u) {
                const int q = q0 + u * RF_TILE_THREADS;
                xv[u] = xsrc[q < n3 ? q : n3 - 1];
            }
#pragma unroll
            for (int u = 0; u < RF_XB; ++u) {
                const int q = q0 + u * RF_TILE_THREADS;
                if (q < n3) sx[q] = xv[u];
            }
        }
        if (!SURFACE) {
            centre_store(q_lo);
            for (int qb = q_lo + RF_CB * RF_TILE_THREADS; qb < q_hi; qb += RF_CB * RF_TILE_THREADS) {
                centre_load(qb);
                centre_store(qb);
            }
            // fixed-point scale of this tile: max |grad_out| / S over the (point, channel) values it is going to route (a clamped
            // row is one of them)
            float vm = 0.f;
#pragma unroll
            for (int t = 0; t < NG; ++t) vm = fmaxf(vm, absmax4(Raw4<FT>::wide(gres[t])));
            if (!RES)
                for (int p0 = pl + NG * PL; p0 < N; p0 += NG * PL) {
                    RawT mv[NG];
#pragma unroll
                    for (int t = 0; t < NG; ++t) {
                        const int p = p0 + t * PL;
                        mv[t] = Raw4<FT>::ld(gout + (row0 + (p < nlast ? p : nlast)) * C + c);
                    }
#pragma unroll
                    for (int t = 0; t < NG; ++t) vm = fmaxf(vm, absmax4(Raw4<FT>::wide(mv[t])));
                }
            rf_tile_scale(vm, invS, N, wmax, tid, fx_scale, fx_inv);
        }
        // no table bound to the parameter: normalise here.  (As a branch in step 2, where the unconditional normalisation used to
        // hide under the round trip, it cost the 16-column resident instance 5 spilled registers at its 128-VGPR bound; here, with
        // the set-up batches consumed, every instance keeps the registers and the occupancy it had.)
        if (!hat) normalise_dirs(d0, d1, d2);
        __syncthreads();
        // ---- 4. sweep: each thread takes its points pl, pl + PL, ... in that order (the direction gradient's rounding)
        auto stage_point = [&](const Stage& s, RawT graw, int p) {   // (a bf16 piece is widened here, where it is used)
            point(acc + cg * 4, s.am, Raw4<FT>::wide(graw), Raw4<FT>::wide(s.fw), make_float3(s.px, s.py, s.pz), p);
        };
        if constexpr (RES) {
#pragma unroll
            for (int t = 0; t < RG; ++t) {
                if (t * PL >= N) break;
                if (t + D < RG) st[t + D] = load_stage(pl + (t + D) * PL);
                const int p = pl + t * PL;
                if (p < N) stage_point(st[t], gres[t], p);
            }
        } else {
            for (int p0 = pl; p0 < N; p0 += D * PL) {
#pragma unroll
                for (int u = 0; u < D; ++u) {
                    const int p = p0 + u * PL;
                    const Stage cur = st[u];
                    st[u] = load_stage(p + D * PL);
                    if (p < N) stage_point(cur, cur.ga, p);
                }
            }
        }
    } else {
    if (!SURFACE)
        for (int q = tid; q < NR * G; q += RF_TILE_THREADS) *reinterpret_cast<float4*>(acc + q * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = tid; q < 3 * (r1 - r0); q += RF_TILE_THREADS) sx[q] = xb[r0 * 3 + q];
    // fixed-point scale of this tile: max |grad_out| / S over the (point, channel) values it is going to route
    if (!SURFACE) {
        float vm = 0.f;
        for (int p = pl; p < N; p += PL) {
            const float4 gq = Feat<FT>::ld4(gout + ((size_t)b * N + p) * C + c);
            vm = fmaxf(vm, fmaxf(fmaxf(fabsf(gq.x), fabsf(gq.y)), fmaxf(fabsf(gq.z), fabsf(gq.w))));
        }
        rf_tile_scale(vm, invS, N, wmax, tid, fx_scale, fx_inv);
    }
    load_dirs_normed(dirs, hat, SC, j, d0, d1, d2);
    __syncthreads();
    // software pipeline: the next point's winning rows / their support values / gradient are in flight while
    // this one is processed; with FWIN every global read of the loop is a coalesced stream
    ushort4 am_n = make_ushort4(0, 0, 0, 0);
    float4 ga_n = make_float4(0.f, 0.f, 0.f, 0.f), fw_n = make_float4(1.f, 1.f, 1.f, 1.f);
    if (pl < N) {
        am_n = *reinterpret_cast<const ushort4*>(argrow + ((size_t)b * N + pl) * SC + j);
        ga_n = Feat<FT>::ld4(gout + ((size_t)b * N + pl) * C + c);
        if (!SURFACE && FWIN) fw_n = Feat<FT>::ld4(fwin + ((size_t)b * N + pl) * SC + j);
    }
    for (int p = pl; p < N; p += PL) {
        const ushort4 am = am_n;
        const float4 ga = ga_n, fw = fw_n;
        const int pn = p + PL < N ? p + PL : p;                      // clamped: no branch around the loads
        am_n = *reinterpret_cast<const ushort4*>(argrow + ((size_t)b * N + pn) * SC + j);
        ga_n = Feat<FT>::ld4(gout + ((size_t)b * N + pn) * C + c);
        if (!SURFACE && FWIN) fw_n = Feat<FT>::ld4(fwin + ((size_t)b * N + pn) * SC + j);
        float3 ps = make_float3(0.f, 0.f, 0.f);
        if (RS > 1) ps = make_float3(xb[p * 3], xb[p * 3 + 1], xb[p * 3 + 2]);      // the point itself: a coalesced stream
        point(acc + cg * 4, am, ga, fw, ps, p);
    }
    }
    __syncthreads();
    if (!SURFACE) {
        // flush the tile: one 16-byte store per (row, group)
        for (int q = tid; q < (r1 - r0) * G; q += RF_TILE_THREADS) {
            const int m = q / G, g4 = q - m * G;
            const int4 iv = *reinterpret_cast<const int4*>(acc + m * TC + g4 * 4);
            Feat<FT>::st4(gfm + ((size_t)b * N + r0 + m) * fstride + C + j0 + g4 * 4,
                          make_float4((float)iv.x * fx_inv, (float)iv.y * fx_inv, (float)iv.z * fx_inv, (float)iv.w * fx_inv));
        }
        if (D == 0 && j0 < C) {   // legacy: the first C/TC tiles also copy the centre columns grad_fm[b,m,c] = g[b,m,c]
            for (int q = tid; q < (r1 - r0) * G; q += RF_TILE_THREADS) {
                const int m = q / G, g4 = q - m * G;
                Feat<FT>::st4(gfm + ((size_t)b * N + r0 + m) * fstride + j0 + g4 * 4,
                              Feat<FT>::ld4(gout + ((size_t)b * N + r0 + m) * C + j0 + g4 * 4));
            }
        }
        __syncthreads();
    }
    // fold the direction gradient across the PL point lanes (fixed order) -> gd_part[b][d][j]
    float* red = reinterpret_cast<float*>(smem);       // RF_TILE_THREADS x 12 floats
    float* mine = red + tid * 12;
    mine[0] = g0.x; mine[1] = g0.y; mine[2] = g0.z; mine[3] = g0.w;
    mine[4] = g1.x; mine[5] = g1.y; mine[6] = g1.z; mine[7] = g1.w;
    mine[8] = g2.x; mine[9] = g2.y; mine[10] = g2.z; mine[11] = g2.w;
    __syncthreads();
    if (tid < G * 12) {
        const int gg = tid / 12, w = tid - gg * 12;    // group, (d*4 + e)
        float sacc = 0.f;
        for (int l = 0; l < PL; ++l) sacc += red[(l * G + gg) * 12 + w];
        const int d = w >> 2, e = w & 3;
        gd_part[((size_t)(b * RS + (RS > 1 ? (int)blockIdx.z : 0)) * 3 + d) * SC + j0 + gg * 4 + e] = sacc;
    }
}

// Direction-gradient epilogue.  ws[blk][3][SC] holds per-workgroup partials of d(loss)/d(D^) (D^ = the
// column-normalised directions).  Workgroup = 64 columns x 16 block-slices: every thread sums its slice
// for the 3 rows of its column (independent accumulators keep loads in flight), the 16 slices are folded
// through LDS in a fixed order (deterministic), then the Jacobian of F.normalize(dim=0) is applied:
//   n = max(||D||, 1e-12);  ||D|| > 1e-12:  gD = (gD^ - D^ (D^ . gD^)) / n ;  else gD = gD^ / 1e-12
__global__ __launch_bounds__(1024) void rf_dirs_reduce_kernel(const float* __restrict__ ws, int nblk, int SC,
                                                              const float* __restrict__ dirs,
                                                              float* __restrict__ out) {
    __shared__ float red[16][3][64];
    dirs_fold_body<1024>(ws, nblk, SC, dirs, out, (int)blockIdx.x, red);          // (folds.h; also inside hsp_step_fold)
}

// the end of every direction-gradient backward, once its partials launch is out: the fold of the nparts partials is left to
// the caller (*pending, the *_partial entries) or launched here
static int rf_dirs_finish(const float* part, int nparts, int SC, const float* dirs, float* gdirs, hipStream_t st,
                          HspDirsPending* pending) {
    if (pending) { *pending = HspDirsPending{part, dirs, gdirs, nparts, SC}; return HSP_OK; }
    hipLaunchKernelGGL(rf_dirs_reduce_kernel, dim3((SC + 63) / 64), dim3(1024), 0, st, part, nparts, SC, dirs, gdirs);
    return check_launch();
}

// backward grid: persistent, capped so that the per-block direction-gradient partials stay <= 8 MiB
static int rf_bwd_grid_max(int SC) {
    long long g = (8ll << 20) / (12ll * SC);
    g &= ~7ll;
    if (g < 8) g = 8;
    if (g > 1024) g = 1024;
    return (int)g;
}

static int rf_bwd_grid(long long points, int SC) {
    const int g = persistent_blocks(points, 4), gm = rf_bwd_grid_max(SC);
    return g < gm ? g : gm;
}

}  // namespace hsp

using namespace hsp;

// The normalised tables bound to direction parameters, keyed by the parameter's device address: host state of the process, like
// the tile schedule below.  Every launcher here looks its `dirs` argument up when the call is issued (a captured graph keeps what
// it was captured with); the binder keeps parameter and table alive while bound and answers for the table holding
// normalise_dirs of the parameter's current values when a kernel that was handed it runs.
namespace {
struct RfDirsHat { const float* dirs; int SC; const float* hat; };
std::mutex g_rf_hat_mutex;
std::vector<RfDirsHat> g_rf_hat;
}  // namespace

static const float* rf_dirs_hat_find(const float* dirs, int SC) {
    std::lock_guard<std::mutex> lock(g_rf_hat_mutex);
    for (const RfDirsHat& e : g_rf_hat)
        if (e.dirs == dirs) return e.SC == SC ? e.hat : nullptr;     // (another shape under this address: not this parameter)
    return nullptr;
}

extern "C" int hsp_rf_dirs_hat_bind(const float* dirs, int SC, const float* hat) {
    if (!dirs || SC <= 0 || (SC & 3)) return HSP_ERR_BAD_ARG;
    if (hat && (((uintptr_t)hat & 15) || hat == dirs)) return HSP_ERR_BAD_ARG;     // read with 16-byte loads
    std::lock_guard<std::mutex> lock(g_rf_hat_mutex);
    for (size_t i = 0; i < g_rf_hat.size(); ++i)
        if (g_rf_hat[i].dirs == dirs) {
            if (hat) g_rf_hat[i] = RfDirsHat{dirs, SC, hat};
            else g_rf_hat.erase(g_rf_hat.begin() + (long)i);
            return HSP_OK;
        }
    if (hat) g_rf_hat.push_back(RfDirsHat{dirs, SC, hat});
    return HSP_OK;
}

extern "C" const float* hsp_rf_dirs_hat_lookup(const float* dirs, int SC) {
    return dirs && SC > 0 ? rf_dirs_hat_find(dirs, SC) : nullptr;
}

static int rf_check(const void* a, const void* b, const void* c, int B, int N, int k, int S, int C) {
    if (!a || !b || !c || B <= 0 || N <= 0 || k <= 0 || S <= 0 || C <= 0) return HSP_ERR_BAD_ARG;
    if (N > 65535 || (C & 3)) return HSP_ERR_UNSUPPORTED;   // winning rows are stored as uint16; float4 column groups
    return HSP_OK;
}

// which forward kernel a (k, S, C) runs: column slots per thread (0: declined) and the schedule.  The one source of truth of
// rf_fwd and of hsp_rf_fwd_plan.
struct RfFwdPlan { int nch; bool pipe; size_t lds; };
static RfFwdPlan rf_fwd_plan(int k, int S, int C) {
    RfFwdPlan p{0, false, 0};
    if (k <= 0 || S <= 0 || C <= 0 || (C & 3) || (long long)S * C > 4096 || k > 16384) return p;   // S*C <= 4096: 4 slots
    const size_t lds = (size_t)(S * C + 5 * k) * 4;
    if (lds > 64 * 1024) return p;
    p.nch = ((S * C >> 2) + RF_THREADS - 1) / RF_THREADS;
    p.lds = lds;
    // the pipelined schedule (three points' phases per barrier interval) wherever the last slot leaves k threads free
    const int spare0 = (S * C >> 2) - (p.nch - 1) * RF_THREADS;
    const size_t lds_pipe = 2 * (size_t)(S * C + 6 * k) * 4;
    if (spare0 + k <= RF_THREADS && lds_pipe <= 64 * 1024) { p.pipe = true; p.lds = lds_pipe; }
    return p;
}

extern "C" int hsp_rf_fwd_plan(int k, int S, int C, int* pipelined) {
    const RfFwdPlan p = rf_fwd_plan(k, S, C);
    if (pipelined) *pipelined = p.pipe ? 1 : 0;
    return p.nch;
}

// the run-time column slots per thread (1..4) and WF as template arguments: launch(integral_constant<int, NCH>, bool_constant<WF>)
template <class F>
static void rf_dispatch_nch(int nch, bool wf, F launch) {
    with_int<1, 2, 3, 4>(nch, [&](auto n) {
        if (wf) launch(n, std::true_type{});
        else launch(n, std::false_type{});
    });
}

template <bool SURFACE, typename FT>
static int rf_fwd(const float* xyz, const int32_t* idx, const float* dirs, const FT* fm, int B, int N, int k,
                  int S, int C, FT* out, uint16_t* argrow, FT* fwin, hspStream_t stream) {
    int rc = rf_check(xyz, idx, dirs, B, N, k, S, C);
    if (rc) return rc;
    if (!out || !argrow || (!SURFACE && !fm)) return HSP_ERR_BAD_ARG;
    // (A channel-split schedule -- C / 2 channels per pass so that a cloud's fm slice stays in the XCD's L2 -- halves the fabric
    // reads (FETCH_SIZE 252 -> 121 MB at B=16 N=1028) but the kernel is VALU-issue-bound: 121 vs 101 us in round 2, and again
    // slower inside the matrix-core form of round 4, tools/experiments/.  Removed.)
    const RfFwdPlan plan = rf_fwd_plan(k, S, C);
    if (!plan.nch) return HSP_ERR_UNSUPPORTED;            // S*C <= 4096, (S*C + 5 k) floats of LDS
    const float* hat = rf_dirs_hat_find(dirs, S * C);
    // workgroups per CU: 8 for the large layers, 4 below 8192 points.  Measured at B = 16 with the normalised table bound (no
    // normalisation left in the prologue; event-timed launches, three alternations):
    //   N = 257, C = 256 (4112 points):  4: 40.2 - 40.6 us   5: 40.8 - 41.2   6 (the setting until then): 41.4 - 41.6   8: 41.4 - 41.6
    //   N = 64,  C = 512 (1024 points):  4: 19.19 - 19.28 us  6: 19.24 - 19.29  8: 19.25 - 19.27  2: 18.82 - 18.95
    // At N = 64 the point schedule gives an XCD's workgroups the indices 0 .. 63 of its two clouds: from 2 per CU (64 per XCD) on,
    // the same 512 workgroups work and the rest leave at once, so 4 / 6 / 8 are one setting.  2 per CU measured 0.3 us less but is
    // not taken: below 2048 points lie the single-cloud inference shapes too, where it halves the workgroups and was not measured.
    const long long npts = (long long)B * N;
    const int grid = persistent_blocks(npts, npts < 2048 ? RF_FWD_WGS_TINY : npts < 8192 ? RF_FWD_WGS_SMALL : 8);
    rf_dispatch_nch(plan.nch, !SURFACE && fwin, [&](auto nch, auto wf) {
        constexpr int NCH = decltype(nch)::value;
        constexpr bool WF = !SURFACE && decltype(wf)::value;
        auto kern = plan.pipe ? rf_fwd_pipe_kernel<SURFACE, NCH, WF, FT> : rf_fwd_kernel<SURFACE, NCH, WF, FT>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(RF_THREADS), plan.lds, as_stream(stream), xyz, idx, dirs, hat, fm, B, N, k, S, C, out,
                           argrow, fwin);
    });
    return check_launch();
}

extern "C" int hsp_rf_surface_fwd(const float* xyz, const int32_t* idx, const float* dirs_n, int B, int N, int k,
                                  int S, int K, float* out, uint16_t* argrow, hspStream_t stream) {
    return rf_fwd<true, float>(xyz, idx, dirs_n, nullptr, B, N, k, S, K, out, argrow, nullptr, stream);
}
extern "C" int hsp_rf_surface_fwd_bf16(const float* xyz, const int32_t* idx, const float* dirs_n, int B, int N, int k,
                                       int S, int K, hsp_bf16_t* out, uint16_t* argrow, hspStream_t stream) {
    return rf_fwd<true, bf16_t>(xyz, idx, dirs_n, nullptr, B, N, k, S, K, out, argrow, nullptr, stream);
}

// the forward's fwin stream pays off once a cloud's fm no longer stays in its XCD's L2 next to the other streams
// (round 3: always.  With the tile kernel's adds in fixed point the 4-byte gathers of the winners' support values were what
// the small clouds' backward waited on: 52.7 -> 28.1 us at N = 257, C = 256 for +5 us in the forward.)
extern "C" int hsp_rf_conv_wants_fwin(int N, int S, int C) {
    (void)N; (void)S; (void)C;
    return 1;
}

extern "C" int hsp_rf_conv_fwd(const float* xyz, const int32_t* idx, const float* dirs_n, const float* fm, int B,
                               int N, int k, int S, int C, float* out, uint16_t* argrow, float* fwin,
                               hspStream_t stream) {
    return rf_fwd<false, float>(xyz, idx, dirs_n, fm, B, N, k, S, C, out, argrow, fwin, stream);
}
extern "C" int hsp_rf_conv_fwd_bf16(const float* xyz, const int32_t* idx, const float* dirs_n, const hsp_bf16_t* fm, int B,
                                    int N, int k, int S, int C, hsp_bf16_t* out, uint16_t* argrow, hsp_bf16_t* fwin,
                                    hspStream_t stream) {
    return rf_fwd<false, bf16_t>(xyz, idx, dirs_n, fm, B, N, k, S, C, out, argrow, fwin, stream);
}
extern "C" int hsp_rf_conv_wants_fwin_bf16(int N, int S, int C) {
    return (size_t)N * (S + 1) * C * sizeof(bf16_t) >= ((size_t)3 << 20) ? 1 : 0;
}

extern "C" size_t hsp_rf_bwd_workspace_bytes(int SC) {
    if (SC <= 0) return 0;
    return (size_t)rf_bwd_grid_max(SC) * 3 * (size_t)SC * sizeof(float);
}

extern "C" int hsp_rf_conv_bwd(const float* xyz, const float* dirs_n, const float* fm, const uint16_t* argrow,
                               const float* grad_out, const int32_t* rev_off, const int32_t* rev_edge, int B, int N,
                               int k, int S, int C, float* grad_fm, float* grad_dirs_n, void* ws, size_t ws_bytes,
                               hspStream_t stream) {
    int rc = rf_check(xyz, dirs_n, fm, B, N, k, S, C);
    if (rc) return rc;
    if (!argrow || !grad_out || !rev_off || !rev_edge || !grad_fm || !grad_dirs_n) return HSP_ERR_BAD_ARG;
    const int SC = S * C;
    if (!ws || ws_bytes < hsp_rf_bwd_workspace_bytes(SC)) return HSP_ERR_WORKSPACE;
    const int nq = SC >> 2;
    const int nch = (nq + RF_THREADS - 1) / RF_THREADS;
    if (nch > 4) return HSP_ERR_UNSUPPORTED;              // S*C <= 4096
    hipStream_t st = as_stream(stream);
    const int grid = rf_bwd_grid((long long)B * N, SC);
    const size_t lds = (size_t)(RF_EB * (C + 8)) * 4;
    if (lds > 64 * 1024) return HSP_ERR_UNSUPPORTED;
    float* wsf = reinterpret_cast<float*>(ws);
    const float* hat = rf_dirs_hat_find(dirs_n, SC);
    rf_dispatch_nch(nch, false, [&](auto n, auto) {
        hipLaunchKernelGGL((rf_conv_bwd_csr_kernel<decltype(n)::value>), dim3(grid), dim3(RF_THREADS), lds, st, xyz, dirs_n, hat, fm, argrow,
                           grad_out, rev_off, rev_edge, B, N, k, S, C, grad_fm, wsf);
    });
    rc = check_launch();
    if (rc) return rc;
    return rf_dirs_finish(wsf, grid, SC, dirs_n, grad_dirs_n, st, nullptr);
}

// dynamic LDS of a tile launch over `rows` rows: acc[rows][tc] (the surface kernel keeps none) + xyz[rows][3], and never less
// than the RF_TILE_THREADS x 12 floats of the kernel's direction fold.  The plan's fit tests and the launch both ask here.
static size_t rf_tile_lds(int rows, int tc, bool surface) {
    const size_t lds = ((surface ? 0 : (size_t)rows * tc) + 3 * (size_t)rows) * 4;
    return lds < RF_TILE_THREADS * 12 * 4 ? RF_TILE_THREADS * 12 * 4 : lds;
}

// column-tile scatter: the widest tile whose acc[N][TC] + xyz[N][3] fits two workgroups per CU, else one
static int pick_tile_cols(int N, int C, bool surface, int B = 0, int SC = 0) {
    if (surface) return (C % 16 == 0) ? 16 : ((C % 8 == 0) ? 8 : 4);
    // small clouds take wider tiles (up to 64 columns): the per-workgroup set-up (direction normalisation, tile
    // zeroing / flush, gradient fold) is then amortised over 4x the elements and the row segments read are longer
    for (int pass = 0; pass < 2; ++pass)
        for (int tc = 64; tc >= 4; tc >>= 1) {
            if (tc > 16 && (long long)(SC / tc) * B < 2 * HSP_NUM_CU) continue;   // ... while the grid still fills the chip
            if (C % tc == 0 && rf_tile_lds(N, tc, false) <= (pass == 0 ? 80u : 156u) * 1024) return tc;
        }
    return 0;
}

extern "C" size_t hsp_rf_bwd_scatter_workspace_bytes(int B, int SC) {
    if (B <= 0 || SC <= 0) return 0;
    return (size_t)B * 2 * 3 * SC * sizeof(float);             // (x2: the two half-cloud tiles of the dense-cloud form)
}

// dense clouds: two half-cloud tiles of 16 columns instead of one whole-cloud tile of <= 8 (see rf_bwd_tile_kernel)
static bool rf_use_row_split(int half_rows, int C, bool surface, int tc_whole) {
    return !surface && tc_whole < 16 && C % 16 == 0 && rf_tile_lds(half_rows, 16, false) <= 156u * 1024;
}

// which tile kernel a shape runs and what its launch needs: tile width (0: declined), the number of row ranges (2: the
// half-cloud form), the rows of one tile and the launch's dynamic LDS.  The one source of truth of rf_bwd_scatter and of
// hsp_rf_bwd_scatter_plan.
struct RfBwdPlan { int tc, rs, rows; size_t lds; };
static RfBwdPlan rf_bwd_plan(int B, int N, int S, int C, bool surface) {
    const int tc = pick_tile_cols(N, C, surface, B, S * C), nr = (N + 1) / 2;   // nr: the rows of a cloud's larger half
    if (rf_use_row_split(nr, C, surface, tc)) return RfBwdPlan{16, 2, nr, rf_tile_lds(nr, 16, false)};
    return RfBwdPlan{tc, tc ? 1 : 0, N, tc ? rf_tile_lds(N, tc, surface) : 0};
}

extern "C" int hsp_rf_bwd_scatter_plan(int B, int N, int S, int C, int surface, int* row_split) {
    RfBwdPlan p{0, 0, 0, 0};
    if (B > 0 && N > 0 && N <= 65535 && S > 0 && C > 0 && !(C & 3) && (long long)S * C <= (1 << 24))
        p = rf_bwd_plan(B, N, S, C, surface != 0);
    if (row_split) *row_split = p.rs;
    return p.tc;
}

// The tile kernel's schedule (rf_bwd_tile_kernel: D, RG).  Ring depth and resident rows per instance, from the VGPR count of
// each: the 16-column whole-cloud tile is LDS-bound at two workgroups per CU and has 128 VGPRs to spend;
// the 32- and 64-column tiles stay inside the 80 VGPRs that keep three workgroups per CU; the half-cloud form (one workgroup per
// CU) and the surface kernel (no tile in LDS) carry grad_out in the ring.
static std::atomic<int> g_rf_bwd_legacy{0};

extern "C" int hsp_rf_bwd_set_schedule(int legacy) {
    if (legacy != 0 && legacy != 1) return HSP_ERR_BAD_ARG;
    return g_rf_bwd_legacy.exchange(legacy);
}

template <int TC, bool SURFACE, int RS> struct RfSched {
    // (the 32-column tile: depth 1 is what fits 80 VGPRs beside five resident rows; depth 2 at two workgroups per CU measured slower)
    static constexpr int depth = RS > 1 ? 4 : (SURFACE ? 2 : (TC == 32 ? 1 : (TC == 64 ? 2 : 3)));
    static constexpr int depth_stream = (!SURFACE && RS == 1 && TC >= 32) ? 1 : depth;      // (grad_out in the ring: four more registers a stage)
    static constexpr int resident = (SURFACE || RS > 1) ? 0 : (TC == 16 ? 9 : (TC == 32 ? 5 : (TC == 64 ? 2 : 0)));   // rows per thread
};

// one (tile width, row ranges) under the schedule in force when the call is issued (a captured graph keeps what it was captured with)
template <int TC, bool SURFACE, bool FWIN, typename FT, int RS, typename... A>
static int rf_tile_launch(bool legacy, int N, dim3 grid, size_t lds, hipStream_t st, A... args) {
    typedef RfSched<TC, SURFACE, RS> Sch;
    const dim3 block(RF_TILE_THREADS);
    if (legacy) return launch_lds(rf_bwd_tile_kernel<TC, SURFACE, FWIN, FT, RS, 0, 0>, grid, block, lds, st, args...);
    constexpr int PL = RF_TILE_THREADS / (TC / 4);
    if constexpr (Sch::resident > 0) {
        if ((N + PL - 1) / PL <= Sch::resident)
            return launch_lds(rf_bwd_tile_kernel<TC, SURFACE, FWIN, FT, RS, Sch::depth, Sch::resident>, grid, block, lds, st, args...);
    }
    if constexpr (Sch::resident > 0 && TC == 16) {
        // pick_tile_cols gives a whole cloud 16 columns only while (16 + 3) N floats fit 80 KB: N <= 1077, nine rows per thread.
        // No streamed instance is built for it; a plan that widened would be declined here, loudly, until one is.
        static_assert(80 * 1024 / ((16 + 3) * 4) <= Sch::resident * PL, "the 16-column whole-cloud tile must always be resident");
        return HSP_ERR_UNSUPPORTED;
    } else {
        return launch_lds(rf_bwd_tile_kernel<TC, SURFACE, FWIN, FT, RS, Sch::depth_stream, 0>, grid, block, lds, st, args...);
    }
}

template <bool SURFACE, bool FWIN, typename FT>
static int rf_bwd_scatter(const float* xyz, const float* dirs, const FT* fm, const uint16_t* argrow,
                          const FT* gout, int B, int N, int S, int C, FT* gfm, float* gdirs, void* ws,
                          size_t ws_bytes, hspStream_t stream, HspDirsPending* pending) {
    int rc = rf_check(xyz, dirs, argrow, B, N, 1, S, C);
    if (rc) return rc;
    if (!gout || !gdirs || (!SURFACE && (!fm || !gfm))) return HSP_ERR_BAD_ARG;
    const int SC = S * C;
    if (!ws || ws_bytes < hsp_rf_bwd_scatter_workspace_bytes(B, SC)) return HSP_ERR_WORKSPACE;
    const RfBwdPlan plan = rf_bwd_plan(B, N, S, C, SURFACE);
    if (!plan.tc) return HSP_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    float* part = reinterpret_cast<float*>(ws);
    const bool legacy = g_rf_bwd_legacy.load() != 0;
    const float* hat = rf_dirs_hat_find(dirs, SC);
    auto tile = [&](auto tc, auto rs) {
        return rf_tile_launch<decltype(tc)::value, SURFACE, FWIN, FT, decltype(rs)::value>(
            legacy, N, dim3(SC / plan.tc, B, plan.rs), plan.lds, st, xyz, dirs, hat, fm, argrow, gout, B, N, S, C, gfm, part);
    };
    // (the half-cloud form is built at 16 columns only; a whole cloud takes 64 ... 4)
    rc = plan.rs == 2 ? tile(int_c<16>{}, int_c<2>{}) : with_int<64, 32, 16, 8, 4>(plan.tc, [&](auto tc) { return tile(tc, int_c<1>{}); });
    if (rc) return rc;
    return rf_dirs_finish(part, plan.rs * B, SC, dirs, gdirs, st, pending);   // one partial per cloud and row range
}

// every scatter-backward entry point: pending_required = the *_partial entries, which leave the direction-gradient fold pending
// (hsp_step_fold runs it with the step's other folds); the support values come from the fwin stream where the caller has one,
// else they are gathered from fm
template <bool SURFACE, typename FT>
static int rf_bwd_entry(const float* xyz, const float* dirs_n, const FT* fm, const FT* fwin, const uint16_t* argrow,
                        const FT* grad_out, int B, int N, int S, int C, FT* grad_fm, float* grad_dirs_n, void* ws, size_t ws_bytes,
                        hspStream_t stream, HspDirsPending* pending, bool pending_required) {
    if (pending_required && !pending) return HSP_ERR_BAD_ARG;
    if (!SURFACE && fwin)
        return rf_bwd_scatter<SURFACE, !SURFACE, FT>(xyz, dirs_n, fwin, argrow, grad_out, B, N, S, C, grad_fm, grad_dirs_n, ws, ws_bytes,
                                                     stream, pending);
    return rf_bwd_scatter<SURFACE, false, FT>(xyz, dirs_n, fm, argrow, grad_out, B, N, S, C, grad_fm, grad_dirs_n, ws, ws_bytes, stream,
                                              pending);
}

extern "C" int hsp_rf_surface_bwd(const float* xyz, const float* dirs_n, const uint16_t* argrow, const float* grad_out,
                                  int B, int N, int S, int K, float* grad_dirs_n, void* ws, size_t ws_bytes,
                                  hspStream_t stream) {
    return rf_bwd_entry<true, float>(xyz, dirs_n, nullptr, nullptr, argrow, grad_out, B, N, S, K, nullptr, grad_dirs_n, ws,
                        ws_bytes, stream, nullptr, false);
}
extern "C" int hsp_rf_surface_bwd_bf16(const float* xyz, const float* dirs_n, const uint16_t* argrow,
                                       const hsp_bf16_t* grad_out, int B, int N, int S, int K, float* grad_dirs_n, void* ws,
                                       size_t ws_bytes, hspStream_t stream) {
    return rf_bwd_entry<true, bf16_t>(xyz, dirs_n, nullptr, nullptr, argrow, grad_out, B, N, S, K, nullptr, grad_dirs_n, ws,
                        ws_bytes, stream, nullptr, false);
}
extern "C" int hsp_rf_conv_bwd_scatter(const float* xyz, const float* dirs_n, const float* fm, const float* fwin,
                                       const uint16_t* argrow, const float* grad_out, int B, int N, int S, int C,
                                       float* grad_fm, float* grad_dirs_n, void* ws, size_t ws_bytes,
                                       hspStream_t stream) {
    return rf_bwd_entry<false, float>(xyz, dirs_n, fm, fwin, argrow, grad_out, B, N, S, C, grad_fm, grad_dirs_n, ws,
                        ws_bytes, stream, nullptr, false);
}
extern "C" int hsp_rf_conv_bwd_scatter_bf16(const float* xyz, const float* dirs_n, const hsp_bf16_t* fm,
                                            const hsp_bf16_t* fwin, const uint16_t* argrow, const hsp_bf16_t* grad_out,
                                            int B, int N, int S, int C, hsp_bf16_t* grad_fm, float* grad_dirs_n, void* ws,
                                            size_t ws_bytes, hspStream_t stream) {
    return rf_bwd_entry<false, bf16_t>(xyz, dirs_n, fm, fwin, argrow, grad_out, B, N, S, C, grad_fm, grad_dirs_n, ws,
                        ws_bytes, stream, nullptr, false);
}
extern "C" int hsp_rf_surface_bwd_partial(const float* xyz, const float* dirs_n, const uint16_t* argrow, const float* grad_out,
                                          int B, int N, int S, int K, float* grad_dirs_n, void* ws, size_t ws_bytes,
                                          HspDirsPending* pending, hspStream_t stream) {
    return rf_bwd_entry<true, float>(xyz, dirs_n, nullptr, nullptr, argrow, grad_out, B, N, S, K, nullptr, grad_dirs_n, ws,
                        ws_bytes, stream, pending, true);
}
extern "C" int hsp_rf_surface_bwd_partial_bf16(const float* xyz, const float* dirs_n, const uint16_t* argrow,
                                               const hsp_bf16_t* grad_out, int B, int N, int S, int K, float* grad_dirs_n,
                                               void* ws, size_t ws_bytes, HspDirsPending* pending, hspStream_t stream) {
    return rf_bwd_entry<true, bf16_t>(xyz, dirs_n, nullptr, nullptr, argrow, grad_out, B, N, S, K, nullptr, grad_dirs_n, ws,
                        ws_bytes, stream, pending, true);
}
extern "C" int hsp_rf_conv_bwd_scatter_partial(const float* xyz, const float* dirs_n, const float* fm, const float* fwin,
                                               const uint16_t* argrow, const float* grad_out, int B, int N, int S, int C,
                                               float* grad_fm, float* grad_dirs_n, void* ws, size_t ws_bytes,
                                               HspDirsPending* pending, hspStream_t stream) {
    return rf_bwd_entry<false, float>(xyz, dirs_n, fm, fwin, argrow, grad_out, B, N, S, C, grad_fm, grad_dirs_n, ws,
                        ws_bytes, stream, pending, true);
}
extern "C" int hsp_rf_conv_bwd_scatter_partial_bf16(const float* xyz, const float* dirs_n, const hsp_bf16_t* fm,
                                                    const hsp_bf16_t* fwin, const uint16_t* argrow, const hsp_bf16_t* grad_out,
                                                    int B, int N, int S, int C, hsp_bf16_t* grad_fm, float* grad_dirs_n,
                                                    void* ws, size_t ws_bytes, HspDirsPending* pending, hspStream_t stream) {
    return rf_bwd_entry<false, bf16_t>(xyz, dirs_n, fm, fwin, argrow, grad_out, B, N, S, C, grad_fm, grad_dirs_n, ws,
                        ws_bytes, stream, pending, true);
}
