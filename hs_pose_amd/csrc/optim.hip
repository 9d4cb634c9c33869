// optim.hip -- fused multi-tensor optimizer step for gfx950.
//
// Replaces, for every parameter tensor at once:
//   torch.nn.utils.clip_grad_norm_(params, max_norm)                    engine/train.py:99,104
//   Ranger.step(): gradient centralisation -> RAdam -> Lookahead        tools/torch_utils/solver/ranger2020.py:135-246
// The reference walks 103 parameter tensors in Python and issues ~10 small elementwise kernels for each
// (~1000 launches per step, more than the whole forward + backward here).  All parameters, gradients and
// the three state tensors live in flat fp32 buffers; a table of ROWS (a dim-0 slice of a >= 2-D tensor,
// or a chunk of a 1-D tensor) drives one kernel in which a wave owns a row: it sums the row's gradient
// (the centralisation mean of ranger2020.py:31-41), then streams the update over the row.  The clip
// coefficient is read from device memory (hsp_sumsq_f32 -> no host round trip).
// HBM-bound: 28 B read + 16 B written per parameter (+4 B / 4 B on a Lookahead step).
//
// Gradient accumulation (FLAGS.accumulate, engine/train.py:99-114): hsp_step_gate_accum decides per replay whether the fresh
// gradient is taken and whether the step is applied, hsp_grad_accumulate adds it to the accumulator -- the `grads` buffer of the
// Ranger kernel -- in one 12 B per parameter pass that also leaves the accumulator's squared norm for the clip.
#include "common.h"

namespace hsp {

// The sweep of a squared norm, stated once: element -> lane -> partial.  `quad(i)` yields the i-th float4 of the swept
// buffer, `one(i)` element i of its tail (block 0 only); four accumulators per lane, a wave fold, four waves through LDS,
// part[blockIdx.x].  sumsq_partial_kernel reads its values, grad_accumulate_kernel makes (and stores) them on the way: equal
// values give equal partials, bit for bit, whichever of the two produced them.
template <class Quad, class One>
__device__ __forceinline__ void sumsq_sweep(long long n, float* __restrict__ part, Quad quad, One one) {
    __shared__ float red[4];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = quad(i);
        a0 += v.x * v.x; a1 += v.y * v.y; a2 += v.z * v.z; a3 += v.w * v.w;
    }
    if (blockIdx.x == 0)
        for (long long i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            const float x = one(i);
            a0 += x * x;
        }
    float s = wave_sum((a0 + a1) + (a2 + a3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// partials -> the scalar: one workgroup
__device__ __forceinline__ void sumsq_fold(const float* __restrict__ part, int nblk, float* __restrict__ out) {
    __shared__ float red[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) a += part[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long long n,
                                                            float* __restrict__ part) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    sumsq_sweep(n, part, [=](long long i) { return x4[i]; }, [=](long long i) { return x[i]; });
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ part, int nblk,
                                                          float* __restrict__ out) {
    sumsq_fold(part, nblk, out);
}

// clip_grad_norm_: coef = max_norm / (norm + 1e-6), capped at 1 (torch.clamp(max=1): a NaN norm stays a NaN coefficient).
// The one statement of it: the Ranger step and the accumulate pass scale by the same bits.
__device__ __forceinline__ float clip_coef(float norm_sq, float max_norm) {
    const float c = max_norm / (sqrtf(norm_sq) + 1e-6f);
    return c > 1.0f ? 1.0f : c;
}

// hsp_grad_accumulate (include/hsp.h): acc = first ? 0 + fresh : acc * c + fresh, and the partials of the squared norm of the
// RESULT by sumsq_sweep.  c is the coefficient of the norm the previous take left in norm_sq[0]; the fold behind this launch
// overwrites that scalar, every workgroup here has read it before (stream order).  ctl given: take and first are the gate's.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ fresh,
                                                              long long n, const float* __restrict__ norm_sq, float max_norm,
                                                              int first, const int* __restrict__ ctl,
                                                              float* __restrict__ part) {
    if (ctl) {
        if (ctl[HSP_STEP_CTL_TAKE] == 0) return;
        first = ctl[HSP_STEP_CTL_FIRST];
    }
    float4* a4 = reinterpret_cast<float4*>(acc);
    const float4* f4 = reinterpret_cast<const float4*>(fresh);
    if (first) {                                           // a fresh accumulator: neither acc nor the scalar is read
        sumsq_sweep(n, part,
                    [=](long long i) {
                        const float4 f = f4[i];
                        const float4 r = make_float4(0.0f + f.x, 0.0f + f.y, 0.0f + f.z, 0.0f + f.w);
                        a4[i] = r;
                        return r;
                    },
                    [=](long long i) { const float r = 0.0f + fresh[i]; acc[i] = r; return r; });
        return;
    }
    const float c = clip_coef(norm_sq[0], max_norm);
    sumsq_sweep(n, part,
                [=](long long i) {
                    const float4 a = a4[i], f = f4[i];
                    const float4 r = make_float4(a.x * c + f.x, a.y * c + f.y, a.z * c + f.z, a.w * c + f.w);
                    a4[i] = r;
                    return r;
                },
                [=](long long i) { const float r = acc[i] * c + fresh[i]; acc[i] = r; return r; });
}

// the fold behind grad_accumulate_kernel: a slot the gate did not take leaves the scalar as it was
__global__ __launch_bounds__(256) void sumsq_final_gated_kernel(const float* __restrict__ part, int nblk,
                                                                float* __restrict__ out, const int* __restrict__ ctl) {
    if (ctl && ctl[HSP_STEP_CTL_TAKE] == 0) return;
    sumsq_fold(part, nblk, out);
}

struct RangerArgs {
    float beta1, beta2, eps, weight_decay, step_lr, la_alpha, max_norm;
    int adaptive, lookahead, gc_after;
};

// The device's decision on one replay of the training step (include/hsp.h: the control block).  One wave, one lane, ordinary
// loads and stores: the launches behind it on the stream read what it wrote.
__global__ __launch_bounds__(64) void step_gate_kernel(const float* __restrict__ total, const int* __restrict__ info,
                                                       int* __restrict__ ctl, int horizon) {
    if (threadIdx.x != 0) return;
    if (ctl[HSP_STEP_CTL_ARMED] == 0) {                    // warm-up runs of a capture: no step, no count
        ctl[HSP_STEP_CTL_APPLY] = 0;
        return;
    }
    ctl[HSP_STEP_CTL_REPLAYS] += 1;
    int apply = 0;
    const int applied = ctl[HSP_STEP_CTL_APPLIED];
    if (isnan(total[0])) {                                 // NaN only (math.isnan, engine/train.py:91-95): +-inf is no skip
        ctl[HSP_STEP_CTL_SKIPPED_NAN] += 1;
    } else if (info && info[0] == 0) {                     // no good item: the network ran on the stand-in cloud
        ctl[HSP_STEP_CTL_SKIPPED_NO_ITEM] += 1;
    } else if (applied >= horizon) {                       // the table has no entry for this step
        ctl[HSP_STEP_CTL_EXHAUSTED] = 1;
    } else {
        apply = 1;
        ctl[HSP_STEP_CTL_INDEX] = applied;
        ctl[HSP_STEP_CTL_APPLIED] = applied + 1;
    }
    ctl[HSP_STEP_CTL_APPLY] = apply;
}

// hsp_step_gate_accum (include/hsp.h, rules 1-7): the gate for `accumulate` micro-batches per step.  The one place where micro,
// pending and the counters move.
__global__ __launch_bounds__(64) void step_gate_accum_kernel(const float* __restrict__ total, const int* __restrict__ info,
                                                             int* __restrict__ ctl, int horizon, int accumulate) {
    if (threadIdx.x != 0) return;
    if (ctl[HSP_STEP_CTL_ARMED] == 0) {
        ctl[HSP_STEP_CTL_TAKE] = 0;
        ctl[HSP_STEP_CTL_APPLY] = 0;
        return;
    }
    ctl[HSP_STEP_CTL_REPLAYS] += 1;
    int take = 0, first = 0, apply = 0;
    const int applied = ctl[HSP_STEP_CTL_APPLIED];
    const int micro = ctl[HSP_STEP_CTL_MICRO];
    int pending = ctl[HSP_STEP_CTL_PENDING];
    if (isnan(total[0])) {
        ctl[HSP_STEP_CTL_SKIPPED_NAN] += 1;
    } else if (info && info[0] == 0) {
        ctl[HSP_STEP_CTL_SKIPPED_NO_ITEM] += 1;
    } else if (applied >= horizon) {
        ctl[HSP_STEP_CTL_EXHAUSTED] = 1;
    } else {
        take = 1;
        first = pending == 0;
        pending += 1;
        if (micro % accumulate == 0) {                     // optimizer, scheduler, zero_grad (engine/train.py:105-110)
            apply = 1;
            ctl[HSP_STEP_CTL_INDEX] = applied;
            ctl[HSP_STEP_CTL_APPLIED] = applied + 1;
            pending = 0;
        }
    }
    ctl[HSP_STEP_CTL_MICRO] = micro + 1;
    ctl[HSP_STEP_CTL_TAKE] = take;
    ctl[HSP_STEP_CTL_FIRST] = first;
    ctl[HSP_STEP_CTL_PENDING] = pending;
    ctl[HSP_STEP_CTL_APPLY] = apply;
}

// one wave per row.  ctl == nullptr (hsp_ranger_step): step_lr / adaptive / lookahead are the host's, in `a`.  Otherwise
// (hsp_ranger_step_gated) the wave leaves unless the gate said apply, and takes the three from the table entry the gate named;
// everything below the head is the same code for both.
__global__ __launch_bounds__(256) void ranger_rows_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          float* __restrict__ slow,
                                                          const HspRowDesc* __restrict__ rows, int nrows,
                                                          const float* __restrict__ gnorm_sq,
                                                          const HspStepEntry* __restrict__ table, const int* __restrict__ ctl,
                                                          int horizon, RangerArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nrows) return;
    bool fill_slow = false;
    if (ctl) {
        if (ctl[HSP_STEP_CTL_APPLY] == 0) return;
        const int idx = ctl[HSP_STEP_CTL_INDEX];
        if (idx < 0 || idx >= horizon) return;             // (the gate never names such an entry)
        const HspStepEntry en = table[idx];
        a.step_lr = en.step_lr;
        a.adaptive = (en.flags & HSP_STEP_ADAPTIVE) != 0;
        a.lookahead = (en.flags & HSP_STEP_LOOKAHEAD) != 0;
        fill_slow = (en.flags & HSP_STEP_FILL_SLOW) != 0;
    }
    const HspRowDesc rd = rows[r];
    float clip = 1.0f;
    if (gnorm_sq) {
        clip = clip_coef(gnorm_sq[0], a.max_norm);
    }
    float* pp = p + rd.offset;
    const float* gp = g + rd.offset;
    float* mp = m + rd.offset;
    float* vp = v + rd.offset;
    float* sp = slow + rd.offset;
    if (fill_slow)                                         // first step: slow weights = the weights now (ranger2020.py:168-170);
        for (int e = lane; e < rd.len; e += 64) sp[e] = pp[e];     // each lane reads back below only what it stored itself
    // gradient centralisation (ranger2020.py:31-41, gc_loc=True): g -= mean over all dims but the first
    float mean = 0.f;
    if (rd.gc && !a.gc_after) {
        float s = 0.f;
        for (int e = lane; e < rd.len; e += 64) s += gp[e] * clip;
        mean = wave_sum(s) / (float)rd.len;
    }
    const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
    if (!(rd.gc && a.gc_after)) {
        for (int e = lane; e < rd.len; e += 64) {
            const float gr = gp[e] * clip - mean;
            const float vn = vp[e] * a.beta2 + omb2 * gr * gr;      // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
            const float mn = mp[e] * a.beta1 + omb1 * gr;           // exp_avg.mul_(beta1).add_(g, alpha=1-beta1)
            vp[e] = vn;
            float G = a.adaptive ? mn / (sqrtf(vn) + a.eps) : mn;   // ranger2020.py:215-219
            float w = pp[e];
            if (a.weight_decay != 0.f) G += a.weight_decay * w;
            // on the non-adaptive steps the reference's G_grad IS exp_avg (:219), so its in-place weight-decay
            // term also lands in the stored moment: reproduced
            mp[e] = a.adaptive ? mn : G;
            w -= a.step_lr * G;                                     // p.add_(G, alpha=-step_size*lr)
            if (a.lookahead) {                                      // ranger2020.py:232-238
                const float sl = sp[e] + a.la_alpha * (w - sp[e]);
                sp[e] = sl;
                w = sl;
            }
            pp[e] = w;
        }
        return;
    }
    // gc_loc=False: the centralisation acts on the generalised gradient G (ranger2020.py:223-225): two sweeps.
    // (non-adaptive steps: G aliases exp_avg in the reference, so the stored moment ends up centralised too)
    float s = 0.f;
    for (int e = lane; e < rd.len; e += 64) {
        const float gr = gp[e] * clip;
        const float vn = vp[e] * a.beta2 + omb2 * gr * gr;
        const float mn = mp[e] * a.beta1 + omb1 * gr;
        vp[e] = vn;
        float G = a.adaptive ? mn / (sqrtf(vn) + a.eps) : mn;
        if (a.weight_decay != 0.f) G += a.weight_decay * pp[e];
        mp[e] = a.adaptive ? mn : G;
        s += G;
    }
    const float gmean = wave_sum(s) / (float)rd.len;
    for (int e = lane; e < rd.len; e += 64) {
        float w = pp[e];
        float G;
        if (a.adaptive) {
            G = mp[e] / (sqrtf(vp[e]) + a.eps);
            if (a.weight_decay != 0.f) G += a.weight_decay * w;
            G -= gmean;
        } else {
            G = mp[e] - gmean;
            mp[e] = G;
        }
        w -= a.step_lr * G;
        if (a.lookahead) {
            const float sl = sp[e] + a.la_alpha * (w - sp[e]);
            sp[e] = sl;
            w = sl;
        }
        pp[e] = w;
    }
}

static int sumsq_blocks(long long n) {
    long long b = (n / 4 + 255) / 256;
    if (b < 1) b = 1;
    if (b > 1024) b = 1024;
    return (int)b;
}

}  // namespace hsp

using namespace hsp;

extern "C" size_t hsp_sumsq_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    return (size_t)sumsq_blocks(n) * sizeof(float);
}

extern "C" int hsp_sumsq_f32(const float* x, long long n, float* out, void* ws, size_t ws_bytes, hspStream_t stream) {
    if (!x || !out || n <= 0) return HSP_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) return HSP_ERR_UNSUPPORTED;     // float4 sweeps
    if (!ws || ws_bytes < hsp_sumsq_workspace_bytes(n)) return HSP_ERR_WORKSPACE;
    const int nb = sumsq_blocks(n);
    float* part = reinterpret_cast<float*>(ws);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, st, x, n, part);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, part, nb, out);
    return check_launch();
}

extern "C" int hsp_grad_accumulate(float* acc, const float* fresh, long long n, float* norm_sq, float max_norm, int first,
                                   const int32_t* ctl, void* ws, size_t ws_bytes, hspStream_t stream) {
    if (!acc || !fresh || !norm_sq || n <= 0) return HSP_ERR_BAD_ARG;
    if (((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(fresh)) & 15) != 0) return HSP_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < hsp_sumsq_workspace_bytes(n)) return HSP_ERR_WORKSPACE;
    const int nb = sumsq_blocks(n);
    float* part = reinterpret_cast<float*>(ws);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(nb), dim3(256), 0, st, acc, fresh, n, norm_sq, max_norm, first, ctl, part);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(sumsq_final_gated_kernel, dim3(1), dim3(256), 0, st, part, nb, norm_sq, ctl);
    return check_launch();
}

extern "C" int hsp_step_gate_accum(const float* total, const int32_t* info, int32_t* ctl, int horizon, int accumulate,
                                   hspStream_t stream) {
    if (!total || !ctl || horizon <= 0 || accumulate <= 0) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(step_gate_accum_kernel, dim3(1), dim3(64), 0, as_stream(stream), total, info, ctl, horizon, accumulate);
    return check_launch();
}

extern "C" int hsp_ranger_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* slow,
                               const HspRowDesc* rows, int nrows, float beta1, float beta2, float eps,
                               float weight_decay, float step_lr, int adaptive, int lookahead, float la_alpha,
                               int gc_after, const float* gnorm_sq, float max_norm, hspStream_t stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !slow || !rows || nrows <= 0) return HSP_ERR_BAD_ARG;
    RangerArgs a;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.step_lr = step_lr;
    a.la_alpha = la_alpha; a.max_norm = max_norm; a.adaptive = adaptive; a.lookahead = lookahead; a.gc_after = gc_after;
    hipLaunchKernelGGL(ranger_rows_kernel, dim3((nrows + 3) / 4), dim3(256), 0, as_stream(stream), params, grads, exp_avg,
                       exp_avg_sq, slow, rows, nrows, gnorm_sq,
                       static_cast<const HspStepEntry*>(nullptr), static_cast<const int*>(nullptr), 0, a);
    return check_launch();
}

extern "C" int hsp_step_gate(const float* total, const int32_t* info, int32_t* ctl, int horizon, hspStream_t stream) {
    if (!total || !ctl || horizon <= 0) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(step_gate_kernel, dim3(1), dim3(64), 0, as_stream(stream), total, info, ctl, horizon);
    return check_launch();
}

extern "C" int hsp_ranger_step_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* slow,
                                     const HspRowDesc* rows, int nrows, float beta1, float beta2, float eps,
                                     float weight_decay, float la_alpha, int gc_after, const float* gnorm_sq, float max_norm,
                                     const HspStepEntry* table, const int32_t* ctl, int horizon, hspStream_t stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !slow || !rows || nrows <= 0) return HSP_ERR_BAD_ARG;
    if (!table || !ctl || horizon <= 0) return HSP_ERR_BAD_ARG;
    RangerArgs a;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.step_lr = 0.f;
    a.la_alpha = la_alpha; a.max_norm = max_norm; a.adaptive = 0; a.lookahead = 0; a.gc_after = gc_after;
    hipLaunchKernelGGL(ranger_rows_kernel, dim3((nrows + 3) / 4), dim3(256), 0, as_stream(stream), params, grads, exp_avg,
                       exp_avg_sq, slow, rows, nrows, gnorm_sq,
                       table, ctl, horizon, a);
    return check_launch();
}
