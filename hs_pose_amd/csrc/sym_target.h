// sym_target.h -- the symmetry classes of a cloud and the target of its reconstruction (prop_loss.py:218-229, 258-276), stated
// once: the loss kernels' Prop_sym_recon (losses.hip) and the Chamfer reconstruction term (chamfer_fps.hip) both read the rule here.
#pragma once
#include "common.h"

namespace hsp {

// sym (4 floats of a cloud): rotational symmetry with a mirror plane (can, bowl, bottle) | x-y mirror plane only (laptop, mug
// with handle) | none (camera) | a handle-less mug (sym = [1,0,0,0]), which is left out of the reconstruction terms
struct SymClass {
    bool rot_sym;                  // sym[0] == 1
    bool cls_y, cls_yx, cls_none, skip;
};
__device__ __forceinline__ SymClass sym_class(const float* s) {
    SymClass k;
    k.rot_sym = s[0] == 1.f;
    const float mirrors = s[1] + s[2] + s[3];
    k.cls_y = k.rot_sym && mirrors > 0.f;
    k.cls_yx = !k.rot_sym && s[1] == 1.f;
    k.cls_none = !k.rot_sym && s[1] != 1.f;
    k.skip = k.rot_sym && mirrors == 0.f;
    return k;
}

// canon = R^T (P - t): the point in the object frame of the ground-truth pose (R row-major (3,3))
__device__ __forceinline__ void sym_canon(const float* R, const float* t, const float* P, float canon[3]) {
    const float d0 = P[0] - t[0], d1 = P[1] - t[1], d2 = P[2] - t[2];
    for (int j = 0; j < 3; ++j) canon[j] = d0 * R[j] + d1 * R[3 + j] + d2 * R[6 + j];
}

// the reconstruction's target for the point P with object-frame coordinates canon: mirrored in z (cls_yx) or turned 180 degrees
// about y (cls_y) in the object frame and taken back under the ground-truth pose, P itself (cls_none), 0 (skip)
__device__ __forceinline__ void sym_recon_target(const SymClass& k, const float* R, const float* t, const float* P,
                                                 const float* canon, float target[3]) {
    if (k.cls_yx || k.cls_y) {
        float m[3] = {k.cls_yx ? canon[0] : -canon[0], canon[1], -canon[2]};      // (x, y, -z) | (-x, y, -z)
        for (int i = 0; i < 3; ++i) target[i] = (m[0] * R[3 * i] + m[1] * R[3 * i + 1] + m[2] * R[3 * i + 2]) + t[i];
    } else if (k.cls_none) {
        for (int i = 0; i < 3; ++i) target[i] = P[i];
    } else {
        for (int i = 0; i < 3; ++i) target[i] = 0.f;
    }
}

}  // namespace hsp
