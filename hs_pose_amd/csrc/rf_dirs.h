// rf_dirs.h -- F.normalize(directions, dim=0) of a receptive-field layer's raw (3, S*C) parameter: the ONE copy of its arithmetic.
// Two readers: the prologue of every rf kernel (rfconv.hip) and split_params_x3_kernel (gemm_x3.hip), which writes the normalised
// table once per forward (HspSplitDesc.transpose == 2) so that the rf kernels of a registered parameter load it instead.  Both
// must produce the same bits: a kernel that finds a table and one that does not are the same function of the parameter.
#pragma once
#include "common.h"

namespace hsp {

// the 4 columns j..j+3 (reference gcn3d.py:100,166): D / max(||D||_col, 1e-12).
// A column whose squared norm overflows fp32 (entries beyond 1e19) is first scaled by 2^-96 -- exact, and a unit vector does not
// depend on the scale -- so it normalises to its direction instead of to the 0 that x / inf gives; every column whose squared
// norm is finite, zero, denormal and NaN columns included, takes the plain chain and keeps its bits.  (An infinite entry stays
// what it was: inf / inf = NaN, finite / inf = 0.)
__device__ __forceinline__ void normalise_dirs(float4& d0, float4& d1, float4& d2) {
#define RF_NRM(X)                                                                                    \
    {                                                                                                \
        float n2 = norm2_chain(d0.X, d1.X, d2.X);                                                    \
        if (__builtin_expect(n2 == INFINITY, 0)) {                                                   \
            d0.X *= 0x1p-96f; d1.X *= 0x1p-96f; d2.X *= 0x1p-96f;                                    \
            n2 = norm2_chain(d0.X, d1.X, d2.X);                                                      \
        }                                                                                            \
        const float nr = fmaxf(sqrtf(n2), 1e-12f);           /* correctly rounded, as ATen's */          \
        d0.X = __fdiv_rn(d0.X, nr); d1.X = __fdiv_rn(d1.X, nr); d2.X = __fdiv_rn(d2.X, nr);          \
    }
    RF_NRM(x) RF_NRM(y) RF_NRM(z) RF_NRM(w)
#undef RF_NRM
}

// the three rows of columns j..j+3 of a (3, SC) matrix with row pitch ld
__device__ __forceinline__ void load_dirs_raw(const float* __restrict__ dirs, int ld, int j, float4& d0, float4& d1, float4& d2) {
    d0 = *reinterpret_cast<const float4*>(dirs + j);
    d1 = *reinterpret_cast<const float4*>(dirs + ld + j);
    d2 = *reinterpret_cast<const float4*>(dirs + 2 * ld + j);
}

// hat: the normalised table of this parameter where one is bound (hsp_rf_dirs_hat_bind), else null -- a kernel argument, so the
// branch is uniform over the launch
__device__ __forceinline__ void load_dirs_normed(const float* __restrict__ dirs, const float* __restrict__ hat, int SC, int j,
                                                 float4& d0, float4& d1, float4& d2) {
    if (hat) {
        load_dirs_raw(hat, SC, j, d0, d1, d2);
    } else {
        load_dirs_raw(dirs, SC, j, d0, d1, d2);
        normalise_dirs(d0, d1, d2);
    }
}

}  // namespace hsp
