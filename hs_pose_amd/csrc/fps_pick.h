// fps_pick.h -- the per-pick arg-max of the never-repick farthest-point samplers (chamfer_fps.hip: fps_levels_kernel,
// frontend.hip: fps_ids_kernel), inside one wave.
// A candidate's key is (distance-to-set bits, SIGNED) << 32 | ~index: the largest value wins, the lowest index among equals, and
// a picked candidate -- distance -1 -- ranks below every unpicked one (>= +0) in the same single 64-bit compare.
#pragma once
#include <climits>

#include "common.h"

namespace hsp {

__device__ __forceinline__ long long dpp_max_i64(long long k, const int ctrl_sel) {
    unsigned lo = (unsigned)k, hi = (unsigned)((unsigned long long)k >> 32), olo, ohi;
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
    const long long o = (long long)(((unsigned long long)ohi << 32) | olo);
    return o > k ? o : k;
}

// every lane's key -> the wave's best, uniform: 4 DPP steps inside the 16-lane rows, 4 v_readlane across the rows
__device__ __forceinline__ long long wave_max_i64(long long key) {
    key = dpp_max_i64(key, 0);
    key = dpp_max_i64(key, 1);
    key = dpp_max_i64(key, 2);
    key = dpp_max_i64(key, 3);                              // every lane holds its 16-lane row's best
    long long wk = LLONG_MIN;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)key, r * 16);
        const unsigned hi = __builtin_amdgcn_readlane((unsigned)((unsigned long long)key >> 32), r * 16);
        const long long rk = (long long)(((unsigned long long)hi << 32) | lo);
        wk = rk > wk ? rk : wk;
    }
    return wk;
}

}  // namespace hsp
