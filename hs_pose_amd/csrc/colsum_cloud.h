// colsum_cloud.h -- device body of the one-launch per-cloud column sum (gather.hip: colsum_cloud_kernel, 1024 threads; gemm.hip:
// the same sum as a rider of the weight-gradient pair launch, 256 threads).  Every form walks the same chunks, sums a chunk's
// rows in the same order, folds the row lanes and the chunks in the same order: same bits.
#pragma once
#include "common.h"

namespace hsp {

// sum over the chunks of p[chunk * stride]: THE order of every per-cloud column sum's second stage (chunk_fold_kernel, and
// colsum_cloud_kernel, which folds its own chunks out of LDS) -- eight running sums over chunk, combined pairwise.
// 8 independent partial sums: 8 loads in flight per round trip (the fold is a latency chain, not bandwidth)
__device__ __forceinline__ float chunk_fold8(const float* __restrict__ p, int nchunk, int stride) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int ch = 0;
    for (; ch + 7 < nchunk; ch += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] += p[(size_t)(ch + u) * stride];
    }
    for (; ch < nchunk; ++ch) s[ch & 7] += p[(size_t)ch * stride];
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

__device__ __forceinline__ float fma_plain(float a, float b, float c) {
    float r;
    asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// One row lane's share of a chunk: rows i0, i0 + RL, ... < r1 of cloud rows [row0, ...) added one by one into s[0] for the four
// columns from 4 g on; XYZ: and their three coordinate moments into s[1..3].  THE row order of every float4 form.
template <bool XYZ, typename FT>
__device__ __forceinline__ void colsum_chunk_rows(const FT* __restrict__ x, const float* __restrict__ xyz, size_t row0, int C, int g,
                                                  int i0, int r1, int RL, float4* s) {
    for (int i = i0; i < r1; i += RL) {
        const float4 v = Feat<FT>::ld4(x + (row0 + i) * C + (g << 2));
        s[0].x += v.x; s[0].y += v.y; s[0].z += v.z; s[0].w += v.w;
        if constexpr (XYZ) {
            const float* p3 = xyz + (row0 + i) * 3;
            const float w[3] = {p3[0], p3[1], p3[2]};
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                // plain v_fma_f32, spelled out: hipcc packs these into v_pk_fma_f32 with op_sel picking the coordinate out of the
                // loaded (x, y, z) register run, and that form returned wrong LOW halves (the .x / .z sums of the y moment, lanes 16-31
                // of each half-wave) whenever another process's MFMA kernels shared the GPU -- 3-8 % of the replays, 1-3 % off
                // (tools/dbg_ste2.py, tests/test_gpu_dp_shared.py); never alone on the GPU.  The scalar form has not deviated once.
                s[q + 1].x = fma_plain(v.x, w[q], s[q + 1].x); s[q + 1].y = fma_plain(v.y, w[q], s[q + 1].y);
                s[q + 1].z = fma_plain(v.z, w[q], s[q + 1].z); s[q + 1].w = fma_plain(v.w, w[q], s[q + 1].w);
            }
        }
    }
}

// The row-lane fold: row lane 0 adds the sums that lanes 1 .. RL - 1 left in LDS, in that order, to its own.  red[(lane + l) * G + col]
// is where row lane l of this thread's chunk stands (G float4 columns per lane); the caller has put a barrier after the stores.
__device__ __forceinline__ float4 colsum_lane_fold(float4 a, const float4* red, int lane, int G, int col, int RL) {
    for (int l = 1; l < RL; ++l) {
        const float4 v = red[(lane + l) * G + col];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    return a;
}

// Both stages of the per-cloud column sum (XYZ: and of its three coordinate moments) with the bits of the two-launch form
// (colsum_partial_kernel + chunk_fold_kernel): NT threads own (cloud b, column tile ``tile`` of C/8
// columns) and walk the SAME chunks, NT/32 * R of them per round.  A chunk is 32 threads = the RL = 256 / (C/4) row lanes x the
// tile's C/32 float4 columns, so every thread does exactly the work of one thread of the partial kernel (colsum_chunk_rows and
// colsum_lane_fold, above, are the code of both); the chunk sums stay in LDS and chunk_fold8 sums them in chunk_fold_kernel's
// order.  No partial workspace, no second dependent launch (a fold is a 4-5 us launch for a fraction of a microsecond of adds).
// R > 1 (no XYZ): a thread works on R chunks of a round at once, two rows of each in flight -- a small workgroup then has as
// many loads in the air as the 1024-thread form; each chunk's rows are still added one by one in ascending order.
// cc_smem: (R * NT + (XYZ ? 4 : 1) * nchunk * C/32) float4
template <bool XYZ, int NT, int R>
__device__ __forceinline__ void colsum_cloud_body(float4* __restrict__ cc_smem, const int tile, const int b,
                                                  const float* __restrict__ x, const float* __restrict__ xyz, int N, int C,
                                                  int nchunk, int rows, float* __restrict__ out) {
    static_assert(!XYZ || R == 1, "the coordinate moments are summed one chunk at a time");
    constexpr int NS = XYZ ? 4 : 1;
    constexpr int CPR = NT / 32;                                           // chunks a workgroup covers at once
    const int cq = C >> 2, RL = 256 / cq, G = cq >> 3;
    const int tid = threadIdx.x;
    const int gl = tid % G, rl = (tid / G) % RL, cs = tid / (G * RL);      // tid = (cs * RL + rl) * G + gl
    const int g = tile * G + gl;
    float4* red = cc_smem;                                                 // [R][NT]
    float4* cp = cc_smem + R * NT;                                         // [NS][nchunk][G]
    for (int c0 = 0; c0 < nchunk; c0 += CPR * R) {
        float4 s[R][NS];
#pragma unroll
        for (int u = 0; u < R; ++u)
#pragma unroll
            for (int q = 0; q < NS; ++q) s[u][q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (R == 1) {
            const int chunk = c0 + cs;
            const int r0 = chunk * rows, r1 = chunk < nchunk ? min(N, r0 + rows) : 0;
            colsum_chunk_rows<XYZ, float>(x, xyz, (size_t)b * N, C, g, r0 + rl, r1, RL, s[0]);
        } else {
            int r0[R], r1[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int chunk = c0 + u * CPR + cs;
                r0[u] = chunk * rows + rl;
                r1[u] = chunk < nchunk ? min(N, chunk * rows + rows) : 0;
            }
            for (int j = 0; j < rows; j += 2 * RL) {           // rows past a chunk's end: loaded from row N - 1, not added
                float4 v[R][2];
#pragma unroll
                for (int u = 0; u < R; ++u)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        v[u][h] = *reinterpret_cast<const float4*>(x + ((size_t)b * N + min(r0[u] + j + h * RL, N - 1)) * C + (g << 2));
#pragma unroll
                for (int u = 0; u < R; ++u)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (r0[u] + j + h * RL < r1[u]) {
                            s[u][0].x += v[u][h].x; s[u][0].y += v[u][h].y; s[u][0].z += v[u][h].z; s[u][0].w += v[u][h].w;
                        }
            }
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
#pragma unroll
            for (int u = 0; u < R; ++u) red[u * NT + tid] = s[u][q];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int chunk = c0 + u * CPR + cs;
                if (rl == 0 && chunk < nchunk) {
                    cp[((size_t)q * nchunk + chunk) * G + gl] = colsum_lane_fold(s[u][q], red + u * NT, cs * RL, G, gl, RL);
                }
            }
            __syncthreads();                                   // red is reused by the next slot / round; cp complete after the last
        }
    }
    const int TC = G << 2;
    if (tid < NS * TC) {
        const int q = tid / TC, c = tid - q * TC;
        out[(size_t)b * NS * C + (size_t)q * C + tile * TC + c] =
            chunk_fold8(reinterpret_cast<const float*>(cp) + (size_t)q * nchunk * TC + c, nchunk, TC);
    }
}

}  // namespace hsp
