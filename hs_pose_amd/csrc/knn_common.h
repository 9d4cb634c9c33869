// knn_common.h -- the steps of the neighbour search that knn.hip, knn_exact.hip and tie_pass.h must spell identically.
#pragma once
#include "common.h"

namespace hsp {

// the expanded distance of gcn3d.py:21 in its association: ((inner * -2) + first) + second.  A search adds the CANDIDATE's |c|^2
// first and the query's |q|^2 second; the symmetric tail's dtail store swaps the roles (knn_feat_kernel).
__device__ __forceinline__ float dist_expand(float inner, float first, float second) {
    return add_rn(add_rn(mul_rn(inner, -2.0f), first), second);
}

// four candidate rows r[0..3] per lane against the query row sq (LDS): acc[u] continues torch.bmm's k-ordered fma chain over the
// C columns, independent chains.  Columns below Cv (a multiple of 4) go as 16-byte segments -- the caller vouches that they are
// aligned -- the rest one by one.
__device__ __forceinline__ void chain4_rows(const float* sq, const float* const (&r)[4], int Cv, int C, float (&acc)[4]) {
    int c = 0;
    for (; c < Cv; c += 4) {
        const float4 a = *reinterpret_cast<const float4*>(sq + c);
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(r[u] + c);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            acc[u] = __fmaf_rn(a.w, v[u].w, __fmaf_rn(a.z, v[u].z, __fmaf_rn(a.y, v[u].y, __fmaf_rn(a.x, v[u].x, acc[u]))));
    }
    for (; c < C; ++c) {
        const float a = sq[c];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __fmaf_rn(a, r[u][c], acc[u]);
    }
}

// what every search entry point refuses first (k_max: HSP_MAX_K, or INT_MAX where the entry point has no such bound)
inline bool knn_args_ok(const void* x, const void* idx, int B, int N, int C, int k, int drop, int k_max) {
    return x && idx && B > 0 && N > 0 && C > 0 && k > 0 && k + drop <= N && k <= k_max;
}

}  // namespace hsp
