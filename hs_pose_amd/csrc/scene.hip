// scene.hip -- scenes drawn under a step's key (include/hsp.h states the contract, sentence by sentence): the poses, sizes and
// augmentation rows of a batch of synthetic items and their distractors, and the items' model points, from the keyed generator of
// keyed_draws.h.  Plain HIP C++, vector stores, uint32 arithmetic for the draws, no atomics, no workspace; every output slot
// has one writer.
//
//   scene_draw_kernel    one lane per item: its 17 uniforms, pose, ground truth and augmentation rows, then its D distractors
//   mesh_sample_kernel   one lane per (item, model point): area-weighted triangle by bisection, a point inside by reflection
//
// Every float64 operation of the contract is spelled with its _rn form -- one rounding each, in the header's order.  Two
// launches, not one: the draw has M lanes of work and the sampling M * n_model, and the sampling reads nothing of the draw
// but the mesh and the scale, which it takes from the instance rows -- so it also serves instances the caller made itself.
#include "common.h"
#include "keyed_draws.h"

namespace hsp {
namespace {

constexpr double DEG = 3.141592653589793 / 180.0;        // radians per degree, rounded once
constexpr int SCENE_WORDS = 17;

struct SceneParams {       // the parameter row, in the header's order
    double size_lo, size_hi, dist_lo, dist_hi, elev_lo, elev_hi, roll, W, H, fx, fy, cx0, cy0;
};

__device__ __forceinline__ double lerp_rn(double lo, double hi, double u) { return __dadd_rn(lo, __dmul_rn(__dsub_rn(hi, lo), u)); }

// C = A B of 3 x 3 row-major matrices: every entry (a0 b0 + a1 b1) + a2 b2
__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            C[r * 3 + c] = __dadd_rn(__dadd_rn(__dmul_rn(A[r * 3], B[c]), __dmul_rn(A[r * 3 + 1], B[3 + c])),
                                     __dmul_rn(A[r * 3 + 2], B[6 + c]));
}

// render.euler_zyx's three matrices of an angle in degrees
__device__ __forceinline__ void rot_x(double deg, double* R) {
    const double a = __dmul_rn(deg, DEG), c = cos(a), s = sin(a);
    R[0] = 1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = c; R[5] = -s; R[6] = 0.0; R[7] = s; R[8] = c;
}
__device__ __forceinline__ void rot_y(double deg, double* R) {
    const double a = __dmul_rn(deg, DEG), c = cos(a), s = sin(a);
    R[0] = c; R[1] = 0.0; R[2] = s; R[3] = 0.0; R[4] = 1.0; R[5] = 0.0; R[6] = -s; R[7] = 0.0; R[8] = c;
}
__device__ __forceinline__ void rot_z(double deg, double* R) {
    const double a = __dmul_rn(deg, DEG), c = cos(a), s = sin(a);
    R[0] = c; R[1] = -s; R[2] = 0.0; R[3] = s; R[4] = c; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
}

// the pose of an instance: rt row-major, the fourth row (0, 0, 0, 1)
__device__ __forceinline__ void store_rt(float* __restrict__ rt, const float* R, float tx, float ty, float tz) {
    const float t[3] = {tx, ty, tz};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rt[r * 4] = R[r * 3]; rt[r * 4 + 1] = R[r * 3 + 1]; rt[r * 4 + 2] = R[r * 3 + 2]; rt[r * 4 + 3] = t[r];
    }
    rt[12] = 0.0f; rt[13] = 0.0f; rt[14] = 0.0f; rt[15] = 1.0f;
}

struct SceneOut {
    int32_t *mesh_id, *frame_id, *label;
    float *rt, *scale;
    float *obj_id, *gt_R, *gt_t, *gt_s, *mean_shape, *sym, *nocs_scale, *aug_bb, *aug_rt_t, *aug_rt_r;
    double* angles;
};

__global__ __launch_bounds__(64) void scene_draw_kernel(const unsigned long long* __restrict__ key, const double* __restrict__ ext,
                                                        const float* __restrict__ cls, const float* __restrict__ mean_shape,
                                                        const float* __restrict__ sym, SceneParams p,
                                                        const double* __restrict__ distractors, int M, int n_mesh, int D,
                                                        SceneOut o) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M) return;
    const uint32_t ks = absorb(instance_key(key, (int)(0x84000000u | (uint32_t)i)), 0xfffffff9u);
    double u[SCENE_WORDS];
#pragma unroll
    for (int q = 1; q < SCENE_WORDS; ++q) u[q] = word_to_f64(absorb(ks, (uint32_t)q));
    const int k = (int)(((unsigned long long)absorb(ks, 0u) * (unsigned long long)n_mesh) >> 32);
    const double e0 = ext[k * 3], e1 = ext[k * 3 + 1], e2 = ext[k * 3 + 2];
    const float s = (float)__ddiv_rn(lerp_rn(p.size_lo, p.size_hi, u[1]), fmax(fmax(e0, e1), e2));
    const double sd = (double)s;
    const double dims[3] = {__dmul_rn(e0, sd), __dmul_rn(e1, sd), __dmul_rn(e2, sd)};
    const double z = lerp_rn(p.dist_lo, p.dist_hi, u[2]);
    const double px = __dmul_rn(__dsub_rn(p.W, 1.0), u[3]), py = __dmul_rn(__dsub_rn(p.H, 1.0), u[4]);
    const float t[3] = {(float)__ddiv_rn(__dmul_rn(z, __dsub_rn(px, p.cx0)), p.fx),
                        (float)__ddiv_rn(__dmul_rn(z, __dsub_rn(py, p.cy0)), p.fy), (float)z};
    const double yaw = __dmul_rn(360.0, u[5]), elev = lerp_rn(p.elev_lo, p.elev_hi, u[6]);
    const double roll = __dadd_rn(-p.roll, __dmul_rn(__dmul_rn(2.0, p.roll), u[7]));
    double A[9], B[9], C[9], R64[9];
    rot_z(roll, A); rot_x(__dadd_rn(180.0, elev), B); mat3_mul(A, B, C);
    rot_y(yaw, B); mat3_mul(C, B, R64);
    float R[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = (float)R64[q];
    const double ax = __dadd_rn(-15.0, __dmul_rn(30.0, u[11])), ay = __dadd_rn(-15.0, __dmul_rn(30.0, u[12])),
                 az = __dadd_rn(-15.0, __dmul_rn(30.0, u[13]));
    rot_z(az, A); rot_y(ay, B); mat3_mul(A, B, C);
    rot_x(ax, B); mat3_mul(C, B, R64);

    // the item: instance row i and the item rows
    o.mesh_id[i] = k; o.frame_id[i] = i; o.label[i] = 1;
    store_rt(o.rt + (size_t)i * 16, R, t[0], t[1], t[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.scale[i * 3 + c] = s;
        o.gt_t[i * 3 + c] = t[c];
        o.gt_s[i * 3 + c] = (float)__dsub_rn(dims[c], (double)mean_shape[k * 3 + c]);
        o.mean_shape[i * 3 + c] = mean_shape[k * 3 + c];
        o.aug_bb[i * 3 + c] = (float)__dadd_rn(0.8, __dmul_rn(0.4, u[8 + c]));
        o.aug_rt_t[i * 3 + c] = (float)__ddiv_rn(__dadd_rn(-50.0, __dmul_rn(100.0, u[14 + c])), 1000.0);
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        o.gt_R[i * 9 + q] = R[q];
        o.aug_rt_r[i * 9 + q] = (float)R64[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) o.sym[i * 4 + q] = sym[k * 4 + q];
    o.obj_id[i] = cls[k];
    o.nocs_scale[i] = (float)__dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dims[0], dims[0]), __dmul_rn(dims[1], dims[1])),
                                                  __dmul_rn(dims[2], dims[2])));
    double* __restrict__ ang = o.angles + (size_t)i * 6;
    ang[0] = yaw; ang[1] = elev; ang[2] = roll; ang[3] = ax; ang[4] = ay; ang[5] = az;

    // its distractors: the item's rotation at t + R off, everything from the ROUNDED R, t and s
    for (int d = 0; d < D; ++d) {
        const double* __restrict__ row = distractors + (size_t)d * 8;
        const size_t j = (size_t)(1 + d) * M + i;
        const double md = row[0];
        const bool known = md >= 0.0 && md < (double)n_mesh;              // (false for NaN)
        const int m = known ? (int)md : 0;
        double off[3] = {row[4], row[5], row[6]};
        if (row[7] != 0.0) off[1] = __dsub_rn(off[1], __dadd_rn(__dmul_rn(0.5, dims[1]), __dmul_rn(0.5, row[2])));
        float td[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            td[r] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)R[r * 3], off[0]), __dmul_rn((double)R[r * 3 + 1], off[1])),
                                               __dmul_rn((double)R[r * 3 + 2], off[2])), (double)t[r]);
        o.mesh_id[j] = known ? m : -1;                                    // (the renderer draws nothing for -1)
        o.frame_id[j] = i;
        o.label[j] = 2 + d;
        store_rt(o.rt + j * 16, R, td[0], td[1], td[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) o.scale[j * 3 + c] = known ? (float)__ddiv_rn(row[1 + c], ext[m * 3 + c]) : 0.0f;
    }
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris,
                                                          int T, const int32_t* __restrict__ mesh, int n_mesh,
                                                          const double* __restrict__ cum, const double* __restrict__ ext,
                                                          const int32_t* __restrict__ mesh_id, const float* __restrict__ scale,
                                                          const unsigned long long* __restrict__ key, int n_model,
                                                          float* __restrict__ model_point) {
    const int i = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= n_model) return;
    float* __restrict__ out = model_point + ((size_t)i * n_model + n) * 3;
    out[0] = out[1] = out[2] = 0.0f;                                      // what a mesh that cannot be read gives
    const int k = mesh_id[i];                                             // (wave-uniform from here to the words)
    if (k < 0 || k >= n_mesh) return;
    const int v0 = mesh[k * 4], nv = mesh[k * 4 + 1], t0 = mesh[k * 4 + 2], nt = mesh[k * 4 + 3];
    if (v0 < 0 || nv <= 0 || t0 < 0 || nt <= 0 || (long long)v0 + nv > V || (long long)t0 + nt > T) return;
    const uint32_t km = absorb(instance_key(key, (int)(0x85000000u | (uint32_t)i)), 0xfffffff8u);
    const double u0 = word_to_f64(absorb(km, 3u * (uint32_t)n));
    double u1 = word_to_f64(absorb(km, 3u * (uint32_t)n + 1u)), u2 = word_to_f64(absorb(km, 3u * (uint32_t)n + 2u));
    // the first triangle of the mesh with cum > x, the last one where there is none
    const double* __restrict__ mc = cum + t0;
    const double x = __dmul_rn(u0, mc[nt - 1]);
    int lo = 0, hi = nt - 1;                                              // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (mc[mid] > x) hi = mid; else lo = mid + 1;
    }
    const int32_t* __restrict__ row = tris + ((size_t)t0 + lo) * 3;
    const int ia = row[0], ib = row[1], ic = row[2];
    if (ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) return;
    if (__dadd_rn(u1, u2) > 1.0) { u1 = __dsub_rn(1.0, u1); u2 = __dsub_rn(1.0, u2); }
    const float* __restrict__ a = verts + ((size_t)v0 + ia) * 3;
    const float* __restrict__ b = verts + ((size_t)v0 + ib) * 3;
    const float* __restrict__ c = verts + ((size_t)v0 + ic) * 3;
    double dims[3], ps[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double sq = (double)scale[i * 3 + q], aq = (double)a[q];
        dims[q] = __dmul_rn(ext[k * 3 + q], sq);
        const double pq = __dadd_rn(__dadd_rn(aq, __dmul_rn(u1, __dsub_rn((double)b[q], aq))), __dmul_rn(u2, __dsub_rn((double)c[q], aq)));
        ps[q] = __dmul_rn(pq, sq);
    }
    const double diag = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dims[0], dims[0]), __dmul_rn(dims[1], dims[1])),
                                             __dmul_rn(dims[2], dims[2])));
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q] = (float)__ddiv_rn(ps[q], diag);
}

bool fin(double x) { return fabs(x) < INFINITY; }

}  // namespace
}  // namespace hsp

using namespace hsp;

extern "C" int hsp_scene_draw(const unsigned long long* key, const double* ext, const float* cls, const float* mean_shape,
                              const float* sym, const double* params, const double* distractors, int M, int n_mesh, int D,
                              int32_t* mesh_id, int32_t* frame_id, int32_t* label, float* rt, float* scale, float* obj_id,
                              float* gt_R, float* gt_t, float* gt_s, float* mean_shape_out, float* sym_out, float* nocs_scale,
                              float* aug_bb, float* aug_rt_t, float* aug_rt_r, double* angles, hspStream_t stream) {
    if (!key || !ext || !cls || !mean_shape || !sym || !params || !mesh_id || !frame_id || !label || !rt || !scale || !obj_id ||
        !gt_R || !gt_t || !gt_s || !mean_shape_out || !sym_out || !nocs_scale || !aug_bb || !aug_rt_t || !aug_rt_r || !angles)
        return HSP_ERR_BAD_ARG;
    if (M < 1 || M > 65535 || n_mesh < 1 || D < 0 || D > 254 || (D > 0 && !distractors)) return HSP_ERR_BAD_ARG;
    for (int q = 0; q < 13; ++q)
        if (!fin(params[q])) return HSP_ERR_BAD_ARG;
    const SceneParams p = {params[0], params[1], params[2], params[3], params[4], params[5], params[6], params[7], params[8],
                           params[9], params[10], params[11], params[12]};
    if (!(p.size_lo > 0.0 && p.size_lo <= p.size_hi && p.dist_lo > 0.0 && p.dist_lo <= p.dist_hi)) return HSP_ERR_BAD_ARG;
    const SceneOut o = {mesh_id, frame_id, label, rt, scale, obj_id, gt_R, gt_t, gt_s, mean_shape_out, sym_out, nocs_scale,
                        aug_bb, aug_rt_t, aug_rt_r, angles};
    hipLaunchKernelGGL(scene_draw_kernel, dim3((M + 63) / 64), dim3(64), 0, as_stream(stream), key, ext, cls, mean_shape, sym, p,
                       distractors, M, n_mesh, D, o);
    return check_launch();
}

extern "C" int hsp_mesh_sample(const float* verts, int V, const int32_t* tris, int T, const int32_t* mesh, int n_mesh,
                               const double* cum, const double* ext, const int32_t* mesh_id, const float* scale,
                               const unsigned long long* key, int M, int n_model, float* model_point, hspStream_t stream) {
    if (!verts || !tris || !mesh || !cum || !ext || !mesh_id || !scale || !key || !model_point) return HSP_ERR_BAD_ARG;
    if (V < 1 || T < 1 || n_mesh < 1 || M < 1 || M > 65535 || n_model < 1 || n_model > (1 << 20)) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((n_model + 255) / 256, M), dim3(256), 0, as_stream(stream), verts, V, tris, T, mesh,
                       n_mesh, cum, ext, mesh_id, scale, key, n_model, model_point);
    return check_launch();
}
