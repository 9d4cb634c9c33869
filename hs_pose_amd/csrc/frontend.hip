// frontend.hip -- the steps either side of the network for gfx950.
//
// In front of it, a set of pixels is listed in row-major order and the chosen ones are back-projected:
//  * depth -> point cloud: the device work of PC_sample (reference network/point_sample/pc_sample.py:8-77):
//    fuse = mask * (depth > 0), the masked pixels back-projected with the intrinsics, `samplenum` of them kept, / 1000.
//    hsp_pc_compact lists the masked pixel ids of every image (the order of torch's boolean indexing) with their counts;
//    hsp_pc_gather / hsp_depth_to_pcl back-project only the chosen ones.  One sync per batch where the reference has one per image.
//  * frame -> instance clouds: the evaluation loader's crop chain in front of that (evaluation/load_data_eval.py:207-254):
//    get_bbox window, three cv2.warpAffine(INTER_NEAREST) over the frame, boolean compaction.  hsp_roi_compact walks the crop
//    pixels of every instance through the warp's integer map and lists the source ids of the valid ones; hsp_frame_to_pcl
//    back-projects the chosen ones straight from the frame.
//  * a training batch -> instance clouds: that chain for B frames with one instance each and the loader's defor_2D on the
//    cropped mask in between (datasets/load_data.py:234-278): hsp_roi_defor, hsp_crop_compact, hsp_frames_to_pcl; and the
//    loader's "move on to the next index" for a rejected item (:254-278): hsp_batch_select picks the first good items of a
//    batch with spares and gathers every per-item tensor, one launch.
//  * the chosen rows themselves, optionally: a keyed counter-based draw on the device between the two stages (hsp_sample_ids)
//    in place of the host's, so that no front end has to bring its counts to the host.
// Behind it:
//  * (R|t) assembly: replaces generate_RT(..., mode='vec') (tools/geom_utils.py:232-244 with
//    tools/rot_utils.py:39-100): confidence-weighted orthogonalisation of the two predicted axes and
//    the 4x4 pose matrix, one lane per object instead of ~40 tiny launches.
//  * a video stream, optionally: the crop decided by the pose the previous frame left on the device instead of a detector's
//    mask and box (hsp_pose_windows, hsp_roi_compact_box, hsp_track_update), so that a tracked frame is one replay.
// The listing is ONE skeleton (chunk_count, prefix_sums, chunk_rank, store_ids) under five per-pixel predicates -- hsp_pc_compact,
// hsp_roi_compact, hsp_roi_compact_box, hsp_crop_compact, hsp_roi_defor --; each form's section says what it adds.
#include <tuple>

#include "common.h"
#include "fps_pick.h"
#include "keyed_draws.h"

namespace hsp {

// ---- the skeleton: row-major stream compaction in two launches --------------------------------------------------------------
// The pixels of item blockIdx.y (an image, an instance's crop) are cut into chunks of PC_CHUNK, one workgroup each: 256 threads
// x 16 consecutive pixels, so thread order is pixel order.  A form's predicate turns a thread's 16 pixels into NC bit masks, bit
// i for pixel i; the set bits of mask 0 are what gets listed, the others are only counted.
//   count launch  grid (nchunk, n): cnt[(j * nchunk + chunk) * NC + t] = set bits of mask t in the chunk
//   write launch  grid (nchunk, n): evaluates the predicate again; a thread's rank = mask-0 counts of the earlier chunks + of the
//                                   earlier waves of the workgroup + of the earlier lanes of the wave; the set pixels' ids are
//                                   stored from that rank on; the last chunk's workgroup writes the item's totals
// No atomics, nothing indexed dynamically.  (One workgroup per image moved 75 GB/s: 16 workgroups on 256 CUs.)
#define PC_CHUNK 4096

// every lane gets the wave's sums; the N butterflies go step by step side by side, so their exchanges overlap
template <int N>
__device__ __forceinline__ void wave_sum(int (&v)[N]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int t = 0; t < N; ++t) v[t] += __shfl_xor(v[t], m);
    }
}

template <int NC>
__device__ __forceinline__ void chunk_count(const unsigned (&bits)[NC], int nchunk, int32_t* __restrict__ cnt) {
    __shared__ int wsum[4][NC];
    const int tid = threadIdx.x;
    int c[NC];
#pragma unroll
    for (int t = 0; t < NC; ++t) c[t] = __popc(bits[t]);
    wave_sum(c);
#pragma unroll
    for (int t = 0; t < NC; ++t)
        if ((tid & 63) == 0) wsum[tid >> 6][t] = c[t];
    __syncthreads();
    if (tid < NC)
        cnt[((size_t)blockIdx.y * nchunk + blockIdx.x) * NC + tid] = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
}

// the write launch's LDS: NS sums over the chunk counts (one partial per wave) and the waves' mask-0 counts
template <int NS>
struct ChunkLds {
    int red[4][NS];
    int wpre[4];
    __device__ __forceinline__ int sum(int s) const { return (red[0][s] + red[1][s]) + (red[2][s] + red[3][s]); }
};

// First half of a write kernel, BEFORE the thread evaluates its predicate (these loads go out first).  Sum 0 is always the
// mask-0 counts of the item's earlier chunks.  With SELF, sum 1 is the mask-0 counts of all chunks, in every workgroup; without,
// sums 1 .. NC-1 are the totals of masks 1 .. NC-1, in the last chunk's workgroup only (0 elsewhere).
template <int NC, bool SELF>
__device__ __forceinline__ void prefix_sums(const int32_t* __restrict__ cnt, int nchunk, ChunkLds<(SELF ? NC + 1 : NC)>& sh) {
    constexpr int NS = SELF ? NC + 1 : NC;
    const int chunk = blockIdx.x, tid = threadIdx.x;
    const int32_t* row = cnt + (size_t)blockIdx.y * nchunk * NC;
    int part[NS] = {};
    if (SELF) {
        for (int c = tid; c < nchunk; c += 256) {
            const int v = row[(size_t)c * NC];
            part[1] += v;
            if (c < chunk) part[0] += v;
        }
    } else {
        for (int c = tid; c < chunk; c += 256) part[0] += row[(size_t)c * NC];
        if (NC > 1 && chunk == nchunk - 1)
            for (int c = tid; c < nchunk; c += 256) {
#pragma unroll
                for (int t = 1; t < NC; ++t) part[t] += row[(size_t)c * NC + t];
            }
    }
    wave_sum(part);
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if ((tid & 63) == 0) sh.red[tid >> 6][s] = part[s];
}

// Second half, after the predicate: the exclusive row-major rank of the thread's first set pixel among the item's; `end` is the
// rank past its last (thread 255 of the last chunk: the item's mask-0 total).  Holds the kernel's one __syncthreads();
// sh.sum(s) may be read after it.
template <int NS>
__device__ __forceinline__ int chunk_rank(unsigned bits, ChunkLds<NS>& sh, int& end) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = __popc(bits);
    int incl = c;                                            // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    if (lane == 63) sh.wpre[wv] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wv; ++w) woff += sh.wpre[w];
    end = sh.sum(0) + woff + incl;
    return end - c;
}

// the ids of the thread's set pixels, in order, from rank off on
__device__ __forceinline__ void store_ids(int32_t* __restrict__ out, int off, unsigned bits, const int (&src)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if ((bits >> i) & 1u) out[off++] = src[i];
}

// ---- depth -> point cloud: the pixels of image b with mask * (depth > 0) > 0, listed by their own ids -------------------------
__device__ __forceinline__ bool pc_valid(float m, float d) { return m * (d > 0.f ? 1.f : 0.f) > 0.f; }

__device__ __forceinline__ unsigned pc_scan16(const float* __restrict__ mb, const float* __restrict__ db, int lo, int hi) {
    unsigned bits = 0;
    for (int p = lo; p < hi; ++p) bits |= (pc_valid(mb[p], db[p]) ? 1u : 0u) << (p - lo);
    return bits;
}

__global__ __launch_bounds__(256) void pc_count_kernel(const float* __restrict__ mask, const float* __restrict__ depth,
                                                       int HW, int nchunk, int32_t* __restrict__ cnt) {
    const int b = blockIdx.y;
    const int lo = min(blockIdx.x * PC_CHUNK + threadIdx.x * 16, HW), hi = min(lo + 16, HW);
    const unsigned bits[1] = {pc_scan16(mask + (size_t)b * HW, depth + (size_t)b * HW, lo, hi)};
    chunk_count(bits, nchunk, cnt);
}

__global__ __launch_bounds__(256) void pc_write_kernel(const float* __restrict__ mask, const float* __restrict__ depth,
                                                       int HW, int nchunk, const int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ pix, int32_t* __restrict__ count) {
    __shared__ ChunkLds<1> sh;
    const int b = blockIdx.y;
    prefix_sums<1, false>(cnt, nchunk, sh);
    const int lo = min(blockIdx.x * PC_CHUNK + threadIdx.x * 16, HW), hi = min(lo + 16, HW);
    const unsigned bits = pc_scan16(mask + (size_t)b * HW, depth + (size_t)b * HW, lo, hi);
    int end;
    const int off = chunk_rank(bits, sh, end);
    int src[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) src[i] = lo + i;
    store_ids(pix + (size_t)b * HW, off, bits, src);
    if (blockIdx.x == nchunk - 1 && threadIdx.x == 255) count[b] = end;
}

// PC[b,s,:] = ( (u - cx) * d / fx, (v - cy) * d / fy, d ) / 1000   for pixel pix[b, choose[b,s]]
__global__ __launch_bounds__(256) void pc_gather_kernel(const float* __restrict__ depth,
                                                        const float* __restrict__ coor2d,
                                                        const float* __restrict__ camK,
                                                        const int32_t* __restrict__ pix,
                                                        const int32_t* __restrict__ choose, int B, int HW, int S,
                                                        float* __restrict__ pc) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * S) return;
    const int b = e / S;
    const int p = pix[(size_t)b * HW + choose[e]];
    const float d = depth[(size_t)b * HW + p];
    const float u = coor2d[((size_t)b * 2 + 0) * HW + p], v = coor2d[((size_t)b * 2 + 1) * HW + p];
    const float* K = camK + (size_t)b * 9;
    const float fx = K[0], fy = K[4], ux = K[2], uy = K[5];
    const float x = __fdiv_rn(mul_rn(sub_rn(u, ux), d), fx);
    const float y = __fdiv_rn(mul_rn(sub_rn(v, uy), d), fy);
    pc[(size_t)e * 3 + 0] = __fdiv_rn(x, 1000.0f);
    pc[(size_t)e * 3 + 1] = __fdiv_rn(y, 1000.0f);
    pc[(size_t)e * 3 + 2] = __fdiv_rn(d, 1000.0f);
}

// dataset-side arithmetic (datasets/load_data.py:322-333 then :275): numpy promotes to float64 --
// ((u - cx) * d / fx evaluated in double with a double K), rounds to fp32, then / 1000 in fp32.
__device__ __forceinline__ void backproject_f64(double u, double v, double d, const double* __restrict__ K,
                                                float* __restrict__ o) {
    const double x = __ddiv_rn(__dmul_rn(__dsub_rn(u, K[2]), d), K[0]);
    const double y = __ddiv_rn(__dmul_rn(__dsub_rn(v, K[5]), d), K[4]);
    o[0] = __fdiv_rn((float)x, 1000.0f);
    o[1] = __fdiv_rn((float)y, 1000.0f);
    o[2] = __fdiv_rn((float)d, 1000.0f);
}

__global__ __launch_bounds__(256) void depth_to_pcl_kernel(const float* __restrict__ depth,
                                                           const float* __restrict__ xymap,
                                                           const double* __restrict__ camK,
                                                           const int32_t* __restrict__ pix,
                                                           const int32_t* __restrict__ choose, int B, int HW, int S,
                                                           float* __restrict__ pc) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * S) return;
    const int b = e / S;
    const int p = pix[(size_t)b * HW + choose[e]];
    backproject_f64((double)xymap[((size_t)b * 2 + 0) * HW + p], (double)xymap[((size_t)b * 2 + 1) * HW + p],
                    (double)depth[(size_t)b * HW + p], camK + (size_t)b * 9, pc + (size_t)e * 3);
}

// ---- detections of one frame -> instance clouds (evaluation/load_data_eval.py:207-254) --------------------------------
// The loader warps the coordinate grid, the mask and the depth of the frame into an O x O crop per instance with
// cv2.warpAffine(INTER_NEAREST).  A nearest-neighbour warp of the coordinate grid returns the coordinates of the pixel it
// sampled, so the three crops are three views of ONE integer map crop pixel -> frame pixel; it is evaluated here and the crops
// never exist.  The map, in warpAffine's fixed-point form (10 fractional bits), for xf = (m0, b1, b2) of the inverse transform:
//     X = (rint(b1 * 1024) + 512 + rint(m0 * u * 1024)) >> 10,   Y = (rint(b2 * 1024) + 512 + rint(m0 * v * 1024)) >> 10
// rint in float64 (half to even), arithmetic shift; outside the frame the warp's constant border reads 0: never valid.
// The terms are clamped to +-2^52 so that the sums stay inside int64 whatever the host passes (a clamped term is far outside
// any frame with H * W < 2^31 unless the other term is as absurd).
__device__ __forceinline__ long long roi_fix(double x) {
    return (long long)fmin(fmax(rint(x * 1024.0), -4503599627370496.0), 4503599627370496.0);
}

// the map of instance j and which mask values are its own: m == inst_id[j], or without inst_id m != 0
struct CropMap {
    double m0;
    long long bx, by;
    bool by_id;
    int want;
    __device__ __forceinline__ long long X(int u) const { return (bx + roi_fix(m0 * (double)u)) >> 10; }
    __device__ __forceinline__ long long Y(int v) const { return (by + roi_fix(m0 * (double)v)) >> 10; }
    __device__ __forceinline__ bool owns(int m) const { return by_id ? m == want : m != 0; }
};

__device__ __forceinline__ CropMap crop_map(const double* __restrict__ xf, const int32_t* __restrict__ inst_id, int j) {
    CropMap cm;
    cm.m0 = xf[(size_t)j * 3];
    cm.bx = roi_fix(xf[(size_t)j * 3 + 1]) + 512;
    cm.by = roi_fix(xf[(size_t)j * 3 + 2]) + 512;
    cm.by_id = inst_id != nullptr;
    cm.want = inst_id ? inst_id[j] : 0;
    return cm;
}

// frame pixel id Y * W + X that crop pixel q = v * O + u reads, or -1 outside the frame
__device__ __forceinline__ int roi_source(const CropMap& cm, int q, int O, int H, int W) {
    const int v = q / O, u = q - v * O;
    const long long X = cm.X(u), Y = cm.Y(v);
    if (X < 0 || X >= W || Y < 0 || Y >= H) return -1;
    return (int)Y * W + (int)X;
}

// hsp_roi_compact: the skeleton over the O * O crop pixels of instance blockIdx.y, NC = 2, source ids listed.
// The 16 consecutive crop pixels of one thread: source ids, bits[1] = depth > 0, bits[0] = depth > 0 and own(p) -- the form's
// test of frame pixel p, asked only where the depth is valid: the mask value owned (MaskOwn), or the point inside the tracked
// box (BoxOwn, below)
template <typename D, typename Own>
__device__ __forceinline__ void roi_scan16(const D* __restrict__ depth, const Own& own, const CropMap& cm, int lo, int OO, int O,
                                           int H, int W, int (&src)[16], unsigned (&bits)[2]) {
    bits[0] = 0;
    bits[1] = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int q = lo + i;
        int p = -1;
        if (q < OO) p = roi_source(cm, q, O, H, W);
        src[i] = p;
        if (p >= 0 && depth[p] > (D)0) {
            bits[1] |= 1u << i;
            if (own(p)) bits[0] |= 1u << i;
        }
    }
}

struct MaskOwn {
    const uint8_t* __restrict__ mask;
    const CropMap& cm;
    __device__ __forceinline__ bool operator()(int p) const { return cm.owns(mask[p]); }
};

template <typename D>
__global__ __launch_bounds__(256) void roi_count_kernel(const D* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                        long long mask_stride, const int32_t* __restrict__ inst_id,
                                                        const double* __restrict__ xf, int H, int W, int O, int nchunk,
                                                        int32_t* __restrict__ cnt) {
    const int j = blockIdx.y;
    int src[16];
    unsigned bits[2];
    const CropMap cm = crop_map(xf, inst_id, j);
    roi_scan16(depth, MaskOwn{mask + (size_t)j * mask_stride, cm}, cm, blockIdx.x * PC_CHUNK + threadIdx.x * 16, O * O, O, H, W,
               src, bits);
    chunk_count(bits, nchunk, cnt);
}

template <typename D>
__global__ __launch_bounds__(256) void roi_write_kernel(const D* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                        long long mask_stride, const int32_t* __restrict__ inst_id,
                                                        const double* __restrict__ xf, int H, int W, int O, int nchunk,
                                                        const int32_t* __restrict__ cnt, int32_t* __restrict__ out_src,
                                                        int32_t* __restrict__ count) {
    __shared__ ChunkLds<2> sh;
    const int j = blockIdx.y;
    const int OO = O * O;
    prefix_sums<2, false>(cnt, nchunk, sh);
    int src[16];
    unsigned bits[2];
    const CropMap cm = crop_map(xf, inst_id, j);
    roi_scan16(depth, MaskOwn{mask + (size_t)j * mask_stride, cm}, cm, blockIdx.x * PC_CHUNK + threadIdx.x * 16, OO, O, H, W, src,
               bits);
    int end;
    const int off = chunk_rank(bits[0], sh, end);
    store_ids(out_src + (size_t)j * OO, off, bits[0], src);
    if (blockIdx.x == nchunk - 1 && threadIdx.x == 255) {
        count[j * 2 + 0] = end;
        count[j * 2 + 1] = sh.sum(1);
    }
}

// The fp32 metres of frame pixel p -- THE coordinates of a crop pixel, for the back-projection below and for the farthest-point
// sampler that ranks candidates by them (fps_ids_kernel): the grid values the reference warps are u = float(p % W),
// v = float(p / W) (exact), then the loader's arithmetic.  p outside the frame gives NaN.
template <typename D>
__device__ __forceinline__ void frame_pixel_xyz(const D* __restrict__ depth, int H, int W, const double* __restrict__ K, int p,
                                                float* __restrict__ o) {
    if (p < 0 || p >= H * W) {
        o[0] = o[1] = o[2] = __builtin_nanf("");
        return;
    }
    const int v = p / W, u = p - v * W;
    backproject_f64((double)(float)u, (double)(float)v, (double)depth[p], K, o);
}

// pc[j,s,:] for pixel p = src[j, choose[j,s]] of the frame of instance j, depth + j * depth_stride (0: one frame for all).  An
// index outside its row or frame (a choose beyond the instance's count) gives NaN.
template <typename D>
__global__ __launch_bounds__(256) void frames_to_pcl_kernel(const D* __restrict__ depth, long long depth_stride, int H, int W,
                                                            const double* __restrict__ camK, int camK_rows,
                                                            const int32_t* __restrict__ src, long long src_stride,
                                                            const int32_t* __restrict__ choose, int n, int S,
                                                            float* __restrict__ pc) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * S) return;
    const int j = e / S;
    float* o = pc + (size_t)e * 3;
    const int c = choose[e];
    const int p = (c >= 0 && c < src_stride) ? src[(size_t)j * src_stride + c] : -1;
    frame_pixel_xyz(depth + (size_t)j * depth_stride, H, W, camK + (camK_rows > 1 ? (size_t)j * 9 : 0), p, o);
}

// ---- instances followed from frame to frame (include/hsp.h states the contract, sentence by sentence) -----------------------
// The crop of instance j is decided by the pose and size the last replay left on the device: hsp_pose_windows turns them into
// the window (the transform rows the crop map reads), hsp_roi_compact_box is hsp_roi_compact with the mask replaced by "the
// pixel's point lies inside the padded oriented box", hsp_track_update keeps the state.  Every float64 operation is spelled
// with its _rn form: one rounding each, in the header's order.

// R (row-major, [r * 3 + c]) and t of a pose as doubles; the fourth row of RT is not read
struct PoseF64 {
    double R[9], t[3];
};

__device__ __forceinline__ PoseF64 load_pose(const float* __restrict__ rt) {
    PoseF64 P;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P.R[r * 3 + c] = (double)rt[r * 4 + c];
        P.t[r] = (double)rt[r * 4 + 3];
    }
    return P;
}

// h_i = (0.5 * pad) * double(size_i)
__device__ __forceinline__ void half_extents(const float* __restrict__ size, double pad, double (&h)[3]) {
    const double hp = __dmul_rn(0.5, pad);
#pragma unroll
    for (int i = 0; i < 3; ++i) h[i] = __dmul_rn(hp, (double)size[i]);
}

__device__ __forceinline__ bool finite_f64(double x) { return fabs(x) < INFINITY; }      // (false for NaN)

__global__ __launch_bounds__(64) void pose_windows_kernel(const float* __restrict__ rt, const float* __restrict__ size,
                                                          const double* __restrict__ camK, int camK_rows, int n, double Wm1,
                                                          double Hm1, double O, double pad, int32_t* __restrict__ boxes,
                                                          double* __restrict__ xf, int32_t* __restrict__ wstatus) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    const PoseF64 P = load_pose(rt + (size_t)j * 16);
    const double* __restrict__ K = camK + (camK_rows > 1 ? (size_t)j * 9 : 0);
    const double K0 = K[0], K2 = K[2], K4 = K[4], K5 = K[5];
    double h[3];
    half_extents(size + (size_t)j * 3, pad, h);
    bool ok = finite_f64(K0) && finite_f64(K2) && finite_f64(K4) && finite_f64(K5);
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && finite_f64(P.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && finite_f64(P.t[i]) && finite_f64(h[i]) && h[i] > 0.0;   // (pad is finite: a finite h is a finite size)
    double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double e0 = (k & 1) ? h[0] : -h[0], e1 = (k & 2) ? h[1] : -h[1], e2 = (k & 4) ? h[2] : -h[2];
        double c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            c[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P.R[r * 3], e0), __dmul_rn(P.R[r * 3 + 1], e1)),
                                       __dmul_rn(P.R[r * 3 + 2], e2)), P.t[r]);
        const double u = __dadd_rn(__ddiv_rn(__dmul_rn(K0, c[0]), c[2]), K2);
        const double v = __dadd_rn(__ddiv_rn(__dmul_rn(K4, c[1]), c[2]), K5);
        ok = ok && c[2] > 0.0 && finite_f64(u) && finite_f64(v);
        ulo = fmin(ulo, u); uhi = fmax(uhi, u);
        vlo = fmin(vlo, v); vhi = fmax(vhi, v);
    }
    // clamped as doubles: whatever the extremes, the four values that reach the conversion lie inside the frame
    const double x1 = fmax(0.0, floor(ulo)), y1 = fmax(0.0, floor(vlo));
    const double x2 = fmin(Wm1, ceil(uhi)), y2 = fmin(Hm1, ceil(vhi));
    ok = ok && x2 > x1 && y2 > y1;
    int32_t* __restrict__ b = boxes + (size_t)j * 4;
    double* __restrict__ o = xf + (size_t)j * 3;
    wstatus[j] = ok ? 0 : 4;
    if (!ok) {
        b[0] = b[1] = b[2] = b[3] = 0;
        o[0] = o[1] = o[2] = 0.0;
        return;
    }
    b[0] = (int)x1; b[1] = (int)y1; b[2] = (int)x2; b[3] = (int)y2;
    // integers below 2^31: the sums, the halves and the differences are exact
    const double cx = __dmul_rn(0.5, __dadd_rn(x1, x2)), cy = __dmul_rn(0.5, __dadd_rn(y1, y2));
    const double scale = fmax(__dsub_rn(x2, x1), __dsub_rn(y2, y1));
    // roi_transform, as dzi_windows_kernel has it
    const double a = __ddiv_rn(O, scale), half_O = __ddiv_rn(O, 2.0);
    const double tx = __dsub_rn(half_O, __dmul_rn(a, cx)), ty = __dsub_rn(half_O, __dmul_rn(a, cy));
    const double D = __ddiv_rn(1.0, __dmul_rn(a, a));
    const double m0 = __dmul_rn(a, D), nm0 = -m0;
    o[0] = m0;
    o[1] = __dmul_rn(nm0, tx);
    o[2] = __dmul_rn(nm0, ty);
}

// hsp_roi_compact_box's predicate: frame pixel p (depth valid) -> its fp32 point, as the back-projection writes it -> inside the box
template <typename D>
struct BoxOwn {
    const D* __restrict__ depth;
    const double* __restrict__ K;
    int H, W;
    double Rc[9];      // Rc[i * 3 + r] = R[r][i]: column i of R
    double c[3], h[3];   // c_i = (R0i * tx + R1i * ty) + R2i * tz
    __device__ __forceinline__ bool operator()(int p) const {
        float o[3];
        frame_pixel_xyz(depth, H, W, K, p, o);
        const double px = (double)o[0], py = (double)o[1], pz = (double)o[2];
        bool in = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double q = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(Rc[i * 3], px), __dmul_rn(Rc[i * 3 + 1], py)),
                                                 __dmul_rn(Rc[i * 3 + 2], pz)), c[i]);
            in = in && fabs(q) <= h[i];                         // (false for a NaN on either side)
        }
        return in;
    }
};

template <typename D>
__device__ __forceinline__ BoxOwn<D> box_own(const D* __restrict__ depth, const float* __restrict__ rt,
                                             const float* __restrict__ size, double pad, const double* __restrict__ camK,
                                             int camK_rows, int H, int W, int j) {
    BoxOwn<D> b;
    b.depth = depth;
    b.K = camK + (camK_rows > 1 ? (size_t)j * 9 : 0);
    b.H = H;
    b.W = W;
    const PoseF64 P = load_pose(rt + (size_t)j * 16);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int r = 0; r < 3; ++r) b.Rc[i * 3 + r] = P.R[r * 3 + i];
        b.c[i] = __dadd_rn(__dadd_rn(__dmul_rn(b.Rc[i * 3], P.t[0]), __dmul_rn(b.Rc[i * 3 + 1], P.t[1])),
                           __dmul_rn(b.Rc[i * 3 + 2], P.t[2]));
    }
    half_extents(size + (size_t)j * 3, pad, b.h);
    return b;
}

// the scan of a tracked instance: a flagged one (wstatus != 0, the whole workgroup alike) lists and counts nothing
template <typename D>
__device__ __forceinline__ void box_scan16(const D* __restrict__ depth, const float* __restrict__ rt,
                                           const float* __restrict__ size, double pad, const double* __restrict__ camK,
                                           int camK_rows, const int32_t* __restrict__ wstatus, const double* __restrict__ xf,
                                           int H, int W, int O, int (&src)[16], unsigned (&bits)[2]) {
    const int j = blockIdx.y;
    if (wstatus != nullptr && wstatus[j] != 0) {
        bits[0] = 0;
        bits[1] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) src[i] = -1;
        return;
    }
    roi_scan16(depth, box_own(depth, rt, size, pad, camK, camK_rows, H, W, j), crop_map(xf, nullptr, j),
               blockIdx.x * PC_CHUNK + threadIdx.x * 16, O * O, O, H, W, src, bits);
}

template <typename D>
__global__ __launch_bounds__(256) void box_count_kernel(const D* __restrict__ depth, const float* __restrict__ rt,
                                                        const float* __restrict__ size, double pad,
                                                        const double* __restrict__ camK, int camK_rows,
                                                        const int32_t* __restrict__ wstatus, const double* __restrict__ xf, int H,
                                                        int W, int O, int nchunk, int32_t* __restrict__ cnt) {
    int src[16];
    unsigned bits[2];
    box_scan16(depth, rt, size, pad, camK, camK_rows, wstatus, xf, H, W, O, src, bits);
    chunk_count(bits, nchunk, cnt);
}

template <typename D>
__global__ __launch_bounds__(256) void box_write_kernel(const D* __restrict__ depth, const float* __restrict__ rt,
                                                        const float* __restrict__ size, double pad,
                                                        const double* __restrict__ camK, int camK_rows,
                                                        const int32_t* __restrict__ wstatus, const double* __restrict__ xf, int H,
                                                        int W, int O, int nchunk, const int32_t* __restrict__ cnt,
                                                        int32_t* __restrict__ out_src, int32_t* __restrict__ count) {
    __shared__ ChunkLds<2> sh;
    const int j = blockIdx.y;
    prefix_sums<2, false>(cnt, nchunk, sh);
    int src[16];
    unsigned bits[2];
    box_scan16(depth, rt, size, pad, camK, camK_rows, wstatus, xf, H, W, O, src, bits);
    int end;
    const int off = chunk_rank(bits[0], sh, end);
    store_ids(out_src + (size_t)j * O * O, off, bits[0], src);
    if (blockIdx.x == nchunk - 1 && threadIdx.x == 255) {
        count[j * 2 + 0] = end;
        count[j * 2 + 1] = sh.sum(1);
    }
}

// one lane per word of the state: 16 of the pose, 3 of the size, the lost counter; the words are moved, never computed on
__global__ __launch_bounds__(256) void track_update_kernel(const uint32_t* __restrict__ rt_new, const uint32_t* __restrict__ size_new,
                                                           const int32_t* __restrict__ status, int n, uint32_t* __restrict__ rt_state,
                                                           uint32_t* __restrict__ size_state, int32_t* __restrict__ lost) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * 20) return;
    const int j = e / 20, w = e - j * 20;
    const bool good = status[j] == 0;
    if (w == 19) {
        lost[j] = good ? 0 : lost[j] + 1;
    } else if (good) {
        if (w < 16) rt_state[j * 16 + w] = rt_new[j * 16 + w];
        else size_state[j * 3 + (w - 16)] = size_new[j * 3 + (w - 16)];
    }
}

// ---- the rows each instance keeps, drawn on the device (include/hsp.h: hsp_sample_ids states the construction) ------------
// A stand-alone launch between the compaction and the back-projection: one lane per (instance, kept row), uint32 arithmetic
// only.  The permutation is a 4-round balanced Feistel network over the smallest even width that holds the count, cycle-walked
// into [0, c): O(S) work per instance whatever c, no selection pass, no scratch.
__global__ __launch_bounds__(256) void sample_ids_kernel(const int32_t* __restrict__ count, int stride, int n, int S,
                                                         int min_pts, int min_depth_pts, int short_mode,
                                                         const unsigned long long* __restrict__ key,
                                                         int32_t* __restrict__ choose, int32_t* __restrict__ status) {
    const unsigned eu = blockIdx.x * 256u + threadIdx.x;      // (n * S < 2^31: the last block's tail stays below 2^32)
    if (eu >= (unsigned)(n * S)) return;
    const int e = (int)eu;
    const int j = e / S, s = e - j * S;
    const int c = count[(size_t)j * stride];
    int st = c < min_pts ? 1 : 0;
    if (stride == 2 && count[(size_t)j * 2 + 1] < min_depth_pts) st |= 2;
    if (s == 0) status[j] = st;
    int out;
    if (st != 0 || c <= 0) {
        out = -1;
    } else if (short_mode == 0 && c <= S) {
        out = s % c;
    } else {
        const uint32_t kj = instance_key(key, j);
        if (c < S)
            out = (int)(((unsigned long long)absorb(absorb(kj, 0xffffffffu), (uint32_t)s) * (unsigned long long)c) >> 32);
        else
            out = (int)feistel_permute((uint32_t)s, (uint32_t)c, kj);
    }
    choose[e] = out;
}

// ---- the rows each instance keeps, picked by farthest-point sampling (include/hsp.h: hsp_fps_ids_* states the contract) -----
// The same place in the chain and the same outputs as sample_ids_kernel, with no draw: ONE workgroup per instance ranks the
// instance's candidates -- at most FPS_IDS_CAP entries of its src row, thinned by a stride in crop raster order beyond that -- by
// the coordinates hsp_frame_to_pcl_* would write for them (frame_pixel_xyz), with the pick chain of fps_levels_kernel
// (chamfer_fps.hip): coordinates and distance-to-set in registers, FPS_IDS_THREADS x FPS_IDS_PPT, per pick one 64-bit key
// (fps_pick.h), DPP + v_readlane inside the wave, one LDS slot per wave (double-buffered by pick parity), ONE barrier, and the 16
// slots folded by DPP again.
// The winner's coordinates come from an LDS copy of the candidates (not published beside the key: that would cost every lane a
// select chain over its FPS_IDS_PPT points per pick to save a broadcast read).  The count is a run-time value: the launch is
// shaped for the cap, and a wave updates only the slots that hold a candidate of its own (a wave-uniform switch per pick).
// Every exit before the pick loop is taken by the whole workgroup: the two counts are read once, by two lanes, and broadcast
// through LDS, and the branches test only those.
// Budget: 12 x 4 registers of state + the update's temporaries = 113 VGPRs, no scratch, under the 128 a 1024-thread workgroup
// leaves each lane; LDS 12 bytes per candidate (147 456 at the cap; the launch asks for min(cap, src_stride) of them) + 272
// static, of 160 KB.
// Plain C++, vector stores, no atomics, no workspace, nothing read back.
#define FPS_IDS_THREADS 1024
#define FPS_IDS_PPT 12
#define FPS_IDS_CAP (FPS_IDS_THREADS * FPS_IDS_PPT)

// one pick's update of a lane's first NK slots -> the lane's best key.  NK is the wave's count of slots that hold a candidate:
// one straight-line body per count, no test per slot, so that the NK distance chains are scheduled together (a wave-uniform
// test in front of every slot instead: 3.37 against 2.86 us a pick at the cap, measured)
template <int NK>
__device__ __forceinline__ long long fps_ids_update(const float (&px)[FPS_IDS_PPT], const float (&py)[FPS_IDS_PPT],
                                                    const float (&pz)[FPS_IDS_PPT], float (&dt)[FPS_IDS_PPT], float cx, float cy,
                                                    float cz, int cur, int tid) {
    long long key = LLONG_MIN;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int t = tid + k * FPS_IDS_THREADS;
        const float dx = sub_rn(px[k], cx), dy = sub_rn(py[k], cy), dz = sub_rn(pz[k], cz);
        const float d = sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));   // as fps_levels_kernel
        // picked: -1 for good (fminf(-1, d) == -1).  The select stands in FRONT of the minimum, on operands that cost nothing:
        // behind it the compiler moves the whole distance under a branch on t != cur, a basic block per slot again
        const float v = fminf(t == cur ? -1.f : dt[k], d);
        dt[k] = v;
        const long long kk = (long long)(((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(~t));
        if (kk > key) key = kk;                                      // (no test of t against the count: see dt's start values)
    }
    return key;
}

template <typename D>
__global__ __launch_bounds__(FPS_IDS_THREADS) void fps_ids_kernel(const D* __restrict__ depth, int H, int W,
                                                                  const double* __restrict__ camK, int camK_rows,
                                                                  const int32_t* __restrict__ src, long long src_stride,
                                                                  const int32_t* __restrict__ count, int S, int min_pts,
                                                                  int min_depth_pts, int32_t* __restrict__ choose,
                                                                  int32_t* __restrict__ status) {
    constexpr int T = FPS_IDS_THREADS, PPT = FPS_IDS_PPT, NW = T / HSP_WAVE, CAP = FPS_IDS_CAP;
    extern __shared__ __attribute__((aligned(16))) float s_xyz[];          // min(CAP, src_stride) * 3
    __shared__ long long slot[2][NW];
    __shared__ int s_cnt[2];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 2) s_cnt[tid] = count[(size_t)j * 2 + tid];
    __syncthreads();
    const int c = __builtin_amdgcn_readfirstlane(s_cnt[0]), cd = __builtin_amdgcn_readfirstlane(s_cnt[1]);
    const int st = (c < min_pts ? 1 : 0) | (cd < min_depth_pts ? 2 : 0);
    if (tid == 0) status[j] = st;
    int32_t* __restrict__ out = choose + (size_t)j * S;
    if (st != 0 || c <= 0) {                                    // (whole workgroup)
        for (int s = tid; s < S; s += T) out[s] = -1;
        return;
    }
    if (c <= S) {                                               // (whole workgroup)
        for (int s = tid; s < S; s += T) out[s] = s % c;
        return;
    }
    // a count beyond the row's pitch is the caller's error; no entry past the row is read
    const unsigned cc = (unsigned)(c < src_stride ? c : (int)src_stride);
    const bool thin = cc > (unsigned)CAP;
    const int m = thin ? CAP : (int)cc;
    const int32_t* __restrict__ row = src + (size_t)j * src_stride;
    const double* __restrict__ K = camK + (camK_rows > 1 ? (size_t)j * 9 : 0);
    for (int t = tid; t < m; t += T) {
        const unsigned g = thin ? (unsigned)(((unsigned long long)t * cc) / (unsigned)CAP) : (unsigned)t;
        frame_pixel_xyz(depth, H, W, K, row[g], s_xyz + t * 3);
    }
    __syncthreads();
    float px[PPT], py[PPT], pz[PPT], dt[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int t = tid + k * T;
        const bool in = t < m;
        px[k] = in ? s_xyz[t * 3] : 0.f;
        py[k] = in ? s_xyz[t * 3 + 1] : 0.f;
        pz[k] = in ? s_xyz[t * 3 + 2] : 0.f;
        dt[k] = in ? INFINITY : -1.f;                           // past the candidates: "picked" from the start -- it ranks with the
    }                                                           // picked ones and below them all by its index, so it never wins
    // slot k of this wave holds candidates wv * 64 + k * T ..: the first nk slots reach below m
    const int left = m - wv * HSP_WAVE;
    const int nk = left <= 0 ? 0 : (left + T - 1) / T;         // (<= PPT: m <= CAP)
    int cur = 0;
    for (int s = 0; s < S; ++s) {
        const float cx = s_xyz[cur * 3], cy = s_xyz[cur * 3 + 1], cz = s_xyz[cur * 3 + 2];
        if (tid == 0) out[s] = thin ? (int)(((unsigned long long)cur * cc) / (unsigned)CAP) : cur;
        long long key;                                          // (value bits, signed) << 32 | ~index
        switch (nk) {                                           // wave-uniform: the wave's slots that hold a candidate
            case 0: key = LLONG_MIN; break;
            case 1: key = fps_ids_update<1>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 2: key = fps_ids_update<2>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 3: key = fps_ids_update<3>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 4: key = fps_ids_update<4>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 5: key = fps_ids_update<5>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 6: key = fps_ids_update<6>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 7: key = fps_ids_update<7>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 8: key = fps_ids_update<8>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 9: key = fps_ids_update<9>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 10: key = fps_ids_update<10>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            case 11: key = fps_ids_update<11>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
            default: key = fps_ids_update<12>(px, py, pz, dt, cx, cy, cz, cur, tid); break;
        }
        long long wk = wave_max_i64(key);
        if (lane == 0) slot[s & 1][wv] = wk;
        __syncthreads();
        // the fold of the NW = 16 slots: lane l reads slot l % 16, so every 16-lane row holds them all and 4 DPP steps leave the
        // workgroup's best in every lane (16 reads folded one after the other compile to a serial chain of scalar selects here:
        // 3.34 against 2.86 us a pick at the cap, measured)
        static_assert(NW == 16, "one slot per lane of a DPP row");
        wk = slot[s & 1][lane & 15];
        wk = dpp_max_i64(wk, 0);
        wk = dpp_max_i64(wk, 1);
        wk = dpp_max_i64(wk, 2);
        wk = dpp_max_i64(wk, 3);
        cur = __builtin_amdgcn_readfirstlane((int)(~(unsigned)wk));   // (wave 0 always holds candidate 0: some key is a candidate's)
    }
}

// ---- the keyed draws of a step (include/hsp.h: "keyed draws of a step" states each stream) -----------------------------------
// What a forward or a replay used to be handed by the host: the rows the Pool_layers keep and the training loader's DZI windows
// (the augmentation's share lives with its kernel, losses.hip).  Streams j >= 2^31, apart from every row draw (j < 65536).

// rows[off_l + s] = P_l(s), s < m_l: level l keeps m_l = n_l / rate of n_l rows, n_1 = m_0; one lane per kept row of either level
__global__ __launch_bounds__(256) void pool_rows_kernel(const unsigned long long* __restrict__ key, int n0, int m0, int m1,
                                                        int32_t* __restrict__ rows) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m0 + m1) return;
    const int level = e >= m0 ? 1 : 0;
    const uint32_t s = (uint32_t)(level ? e - m0 : e), c = (uint32_t)(level ? m0 : n0);
    rows[e] = (int)feistel_permute(s, c, instance_key(key, (int)(0x80000000u | (uint32_t)level)));
}

// aug_bbox_DZI ('uniform', tools/dataset_utils.py:24-61) and roi_transform of item k in float64, one rounding per operation in
// the order pc_sample.dzi_windows / pc_sample.roi_transform perform them; one lane per item
__global__ __launch_bounds__(64) void dzi_windows_kernel(const int32_t* __restrict__ bboxes, const unsigned long long* __restrict__ key,
                                                         int M, double frame_max, double O, double pad_scale, double scale_ratio,
                                                         double shift_ratio, double* __restrict__ xf) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= M) return;
    const uint32_t kz = absorb(instance_key(key, (int)(0x82000000u | (uint32_t)k)), 0xfffffffbu);
    const double u0 = word_to_f64(absorb(kz, 0u)), u1 = word_to_f64(absorb(kz, 1u)), u2 = word_to_f64(absorb(kz, 2u));
    const int x1 = bboxes[k * 4], y1 = bboxes[k * 4 + 1], x2 = bboxes[k * 4 + 2], y2 = bboxes[k * 4 + 3];
    const double cx = __dmul_rn(0.5, (double)((long long)x1 + x2)), cy = __dmul_rn(0.5, (double)((long long)y1 + y2));
    const long long bh = (long long)y2 - y1, bw = (long long)x2 - x1;
    const double sr = __dadd_rn(1.0, __dmul_rn(scale_ratio, __dsub_rn(__dmul_rn(2.0, u0), 1.0)));
    const double sx = __dmul_rn(shift_ratio, __dsub_rn(__dmul_rn(2.0, u1), 1.0));
    const double sy = __dmul_rn(shift_ratio, __dsub_rn(__dmul_rn(2.0, u2), 1.0));
    const double ccx = __dadd_rn(cx, __dmul_rn((double)bw, sx)), ccy = __dadd_rn(cy, __dmul_rn((double)bh, sy));
    const double side = (double)(bh > bw ? bh : bw);
    const double scale = fmin(__dmul_rn(__dmul_rn(side, sr), pad_scale), frame_max);
    // roi_transform: the inverse of the forward matrix a = O / scale, tx = O/2 - a * cx, ty = O/2 - a * cy
    const double a = __ddiv_rn(O, scale), half_O = __ddiv_rn(O, 2.0);
    const double tx = __dsub_rn(half_O, __dmul_rn(a, ccx)), ty = __dsub_rn(half_O, __dmul_rn(a, ccy));
    const double D = __ddiv_rn(1.0, __dmul_rn(a, a));
    const double m0 = __dmul_rn(a, D), nm0 = -m0;
    xf[k * 3] = m0;
    xf[k * 3 + 1] = __dmul_rn(nm0, tx);
    xf[k * 3 + 2] = __dmul_rn(nm0, ty);
}

// ---- the training loader's chain (datasets/load_data.py:228-278): a batch of frames, the mask perturbed before the cut ------
// include/hsp.h ("the training loader's front end") states the mask rule.  hsp_roi_defor writes the crop-space masks, before
// and after defor_2D, as one byte per crop pixel; hsp_crop_compact lists the valid crop pixels under that byte; the clouds come
// from the back-projection above with a frame per instance.

// 16 consecutive bytes of a row of (n, O*O) uint8 as four words, byte i in bits 8 * (i & 3) of word i >> 2: one 16-byte access
// where the address allows it and all 16 lie inside the row, single bytes (inside the row only) otherwise
__device__ __forceinline__ void load16(const uint8_t* __restrict__ p, int left, uint32_t w[4]) {
    if (left >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < left) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
}

__device__ __forceinline__ void store16(uint8_t* __restrict__ p, int left, const uint32_t w[4]) {
    if (left >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < left) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// hsp_roi_defor: the skeleton with NC = 1 over the band pixels, but what it writes is a byte per crop pixel, not ids: every
// workgroup needs the band's size l, so every workgroup totals its counter (SELF), and a band pixel's rank decides its bit.
// The 16 consecutive crop pixels of one thread: bit i of mbits = m, of bbits = on the band (E != D over the triangle i + j <= r
// up and to the left, positions outside the crop left out).  Every footprint pixel is walked through the map again: at most
// (r + 1)(r + 2) / 2 mask reads per pixel (3 at r = 1), neighbours' reads meet in the cache.
__device__ __forceinline__ void defor_scan16(const uint8_t* __restrict__ mask, const CropMap& cm, int lo, int OO, int O, int H,
                                             int W, int r, unsigned& mbits, unsigned& bbits) {
    mbits = 0;
    bbits = 0;
    int v = lo / O, u = lo - v * O;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (lo + i < OO) {
            unsigned e = 1u, d = 0u;
            const int rb = min(r, v);
            for (int b = 0; b <= rb; ++b) {
                const long long Y = cm.Y(v - b);
                const bool yin = Y >= 0 && Y < H;
                const int ra = min(r - b, u);
                for (int a = 0; a <= ra; ++a) {
                    const long long X = cm.X(u - a);
                    unsigned val = 0u;
                    if (yin && X >= 0 && X < W) val = cm.owns(mask[(size_t)Y * W + (size_t)X]) ? 1u : 0u;
                    e &= val;
                    d |= val;
                    if ((a | b) == 0) mbits |= val << i;
                }
            }
            bbits |= (e ^ d) << i;
            if (++u == O) {
                u = 0;
                ++v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void defor_count_kernel(const uint8_t* __restrict__ mask, long long mask_stride,
                                                          const int32_t* __restrict__ inst_id, const double* __restrict__ xf,
                                                          int H, int W, int O, int r, int nchunk, int32_t* __restrict__ cnt) {
    const int j = blockIdx.y;
    unsigned mbits, bits[1];
    defor_scan16(mask + (size_t)j * mask_stride, crop_map(xf, inst_id, j), blockIdx.x * PC_CHUNK + threadIdx.x * 16, O * O, O, H,
                 W, r, mbits, bits[0]);
    chunk_count(bits, nchunk, cnt);
}

// its own epilogue: the gate, the subset of the band that becomes 0, the bytes; the last chunk's workgroup writes band[j]
__global__ __launch_bounds__(256) void defor_write_kernel(const uint8_t* __restrict__ mask, long long mask_stride,
                                                          const int32_t* __restrict__ inst_id, const double* __restrict__ xf,
                                                          int H, int W, int O, int r, int nchunk,
                                                          const int32_t* __restrict__ cnt, unsigned long long gate,
                                                          const unsigned long long* __restrict__ key,
                                                          uint8_t* __restrict__ crop_mask, int32_t* __restrict__ band) {
    __shared__ ChunkLds<2> sh;
    const int j = blockIdx.y;
    const int OO = O * O;
    prefix_sums<1, true>(cnt, nchunk, sh);
    const int lo = blockIdx.x * PC_CHUNK + threadIdx.x * 16;
    unsigned mbits, bbits;
    defor_scan16(mask + (size_t)j * mask_stride, crop_map(xf, inst_id, j), lo, OO, O, H, W, r, mbits, bbits);
    int end;
    uint32_t t = (uint32_t)chunk_rank(bbits, sh, end);   // row-major rank of this thread's first band pixel
    const int l = sh.sum(1);
    const uint32_t kj = instance_key(key, j);
    const bool deformed = l >= 1 && (unsigned long long)absorb(absorb(kj, 0xfffffffeu), 0u) < gate;
    unsigned one = mbits;                                    // bit 0 of the 16 bytes
    if (deformed) {
        const uint32_t kd = absorb(kj, 0xfffffffdu), zeros = (uint32_t)l / 2u;
        one |= bbits;
        for (unsigned rest = bbits; rest; rest &= rest - 1u, ++t)
            if (feistel_permute(t, (uint32_t)l, kd) < zeros) one &= ~(rest & (0u - rest));
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i >> 2] |= (((one >> i) & 1u) | (((mbits >> i) & 1u) << 1)) << (8 * (i & 3));
    store16(crop_mask + (size_t)j * OO + min(lo, OO), OO - min(lo, OO), w);
    if (blockIdx.x == nchunk - 1 && threadIdx.x == 255) {
        band[j * 2 + 0] = l;
        band[j * 2 + 1] = deformed ? 1 : 0;
    }
}

// hsp_crop_compact: hsp_roi_compact's predicate with the mask taken from the crop-space byte and a third mask counted, NC = 3:
// bits[1] = depth > 0, bits[0] = depth > 0 and bit 0 (the deformed mask), bits[2] = depth > 0 and bit 1 (the mask before)
template <typename D>
__device__ __forceinline__ void crop_scan16(const D* __restrict__ depth, const uint8_t* __restrict__ cmask, const CropMap& cm,
                                            int lo, int OO, int O, int H, int W, int (&src)[16], unsigned (&bits)[3]) {
    uint32_t w[4];
    load16(cmask + min(lo, OO), OO - min(lo, OO), w);
    bits[0] = 0;
    bits[1] = 0;
    bits[2] = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int q = lo + i;
        int p = -1;
        if (q < OO) p = roi_source(cm, q, O, H, W);
        src[i] = p;
        if (p >= 0 && depth[p] > (D)0) {
            const uint32_t c = w[i >> 2] >> (8 * (i & 3));
            bits[1] |= 1u << i;
            bits[0] |= (c & 1u) << i;
            bits[2] |= ((c >> 1) & 1u) << i;
        }
    }
}

template <typename D>
__global__ __launch_bounds__(256) void crop_count_kernel(const D* __restrict__ depth, long long depth_stride,
                                                         const uint8_t* __restrict__ crop_mask, const double* __restrict__ xf,
                                                         int H, int W, int O, int nchunk, int32_t* __restrict__ cnt) {
    const int j = blockIdx.y;
    const int OO = O * O;
    int src[16];
    unsigned bits[3];
    crop_scan16(depth + (size_t)j * depth_stride, crop_mask + (size_t)j * OO, crop_map(xf, nullptr, j),
                blockIdx.x * PC_CHUNK + threadIdx.x * 16, OO, O, H, W, src, bits);
    chunk_count(bits, nchunk, cnt);
}

template <typename D>
__global__ __launch_bounds__(256) void crop_write_kernel(const D* __restrict__ depth, long long depth_stride,
                                                         const uint8_t* __restrict__ crop_mask, const double* __restrict__ xf,
                                                         int H, int W, int O, int nchunk, const int32_t* __restrict__ cnt,
                                                         int32_t* __restrict__ out_src, int32_t* __restrict__ count,
                                                         int32_t* __restrict__ pre) {
    __shared__ ChunkLds<3> sh;
    const int j = blockIdx.y;
    const int OO = O * O;
    prefix_sums<3, false>(cnt, nchunk, sh);
    int src[16];
    unsigned bits[3];
    crop_scan16(depth + (size_t)j * depth_stride, crop_mask + (size_t)j * OO, crop_map(xf, nullptr, j),
                blockIdx.x * PC_CHUNK + threadIdx.x * 16, OO, O, H, W, src, bits);
    int end;
    const int off = chunk_rank(bits[0], sh, end);
    store_ids(out_src + (size_t)j * OO, off, bits[0], src);
    if (blockIdx.x == nchunk - 1 && threadIdx.x == 255) {
        count[j * 2 + 0] = end;
        count[j * 2 + 1] = sh.sum(1);
        pre[j] = sh.sum(2);
    }
}

// ---- the kept items of a training batch (include/hsp.h: hsp_batch_select states the rule) ---------------------------------------
// One launch over grid (keep, max(nseg, 1)): workgroup (j, s) copies row sel[j] of segment s into its row j.  status is at most
// 4 KB, so every workgroup derives its own sel[j] from it and nothing is handed from one workgroup to another: item i belongs to
// lane i & 63 of slot i >> 6 (16 slots of 64 items, four rounds of the workgroup's four waves); a slot's good items are one
// __ballot, their ranks the set bits below the lane plus the counts of the earlier slots.  The rows are moved as words, never
// computed on.
struct BatchSelectDesc { HspSelectSeg seg[HSP_BATCH_SELECT_MAX_SEGS]; };

__global__ __launch_bounds__(256) void batch_select_kernel(const int32_t* __restrict__ status, int M, int keep, int nseg,
                                                           const BatchSelectDesc d, int32_t* __restrict__ sel,
                                                           int32_t* __restrict__ info) {
    __shared__ int slot_cnt[16];
    __shared__ int picked;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = blockIdx.x;                                   // (< keep by the grid)
    unsigned long long good[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = q * 256 + tid;
        good[q] = __ballot(i < M && status[i] == 0);
        if (lane == 0) slot_cnt[q * 4 + wv] = __popcll(good[q]);
    }
    __syncthreads();
    int V = 0, before[4] = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        if ((s & 3) == wv) before[s >> 2] = V;                  // slot q * 4 + wv is this wave's in round q
        V += slot_cnt[s];
    }
    if (V > 0) {
        const int t = j % V;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (((good[q] >> lane) & 1ull) && before[q] + __popcll(good[q] & ((1ull << lane) - 1ull)) == t) picked = q * 256 + tid;
    } else if (tid == 0) {
        picked = j;
    }
    __syncthreads();
    const int from = picked;
    if (blockIdx.y == 0 && tid == 0) {
        sel[j] = from;
        if (j == 0) {
            info[0] = V;
            info[1] = min(V, keep);
        }
    }
    if ((int)blockIdx.y >= nseg) return;
    const HspSelectSeg sg = d.seg[blockIdx.y];
    const size_t rb = (size_t)sg.row_bytes;
    const char* s = (V == 0 && sg.fill) ? reinterpret_cast<const char*>(sg.fill)
                                        : reinterpret_cast<const char*>(sg.src) + (size_t)from * rb;
    char* o = reinterpret_cast<char*>(sg.dst) + (size_t)j * rb;
    if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(o) | rb) & 15) == 0) {
        for (size_t b = (size_t)tid * 16; b < rb; b += 256 * 16)
            *reinterpret_cast<uint4*>(o + b) = *reinterpret_cast<const uint4*>(s + b);
    } else {
        for (size_t b = (size_t)tid * 4; b < rb; b += 256 * 4)
            *reinterpret_cast<uint32_t*>(o + b) = *reinterpret_cast<const uint32_t*>(s + b);
    }
}

__device__ __forceinline__ void rodrigues_apply(const float rx[3], float s, float c, const float v[3], float o[3]) {
    // rows of to_rot_matrix_in_batch (rot_utils.py:67-75) times v
    const float t = 1.f - c;
    o[0] = (rx[0] * rx[0] * t + c) * v[0] + (rx[0] * rx[1] * t - rx[2] * s) * v[1] + (rx[0] * rx[2] * t + rx[1] * s) * v[2];
    o[1] = (rx[1] * rx[0] * t + rx[2] * s) * v[0] + (rx[1] * rx[1] * t + c) * v[1] + (rx[1] * rx[2] * t - rx[0] * s) * v[2];
    o[2] = (rx[0] * rx[2] * t - rx[1] * s) * v[0] + (rx[2] * rx[1] * t + rx[0] * s) * v[1] + (rx[2] * rx[2] * t + c) * v[2];
}

__device__ __forceinline__ void normalize3(float v[3]) {     // F.normalize: v / max(|v|, 1e-12)
    const float n = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-12f);
    v[0] /= n; v[1] /= n; v[2] /= n;
}

// generate_RT(mode='vec'): f_red := 0 where sym[:,0]==1; (new_y,new_x) = get_vertical_rot_vec_in_batch;
// R = get_rot_mat_y_first(new_y,new_x) = stack(x,y,z) as columns; res = [[R, T],[0,1]]
__global__ __launch_bounds__(64) void generate_rt_kernel(const float* __restrict__ p_green,
                                                         const float* __restrict__ p_red,
                                                         const float* __restrict__ f_green,
                                                         const float* __restrict__ f_red,
                                                         const float* __restrict__ T,
                                                         const float* __restrict__ sym, int sym_stride, int B,
                                                         float* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    const float c1 = f_green[i];
    const float c2 = (sym[(size_t)i * sym_stride] == 1.0f) ? 0.f : f_red[i];
    float y[3] = {p_green[i * 3], p_green[i * 3 + 1], p_green[i * 3 + 2]};
    float z[3] = {p_red[i * 3], p_red[i * 3 + 1], p_red[i * 3 + 2]};
    float rx[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
    const float rn = sqrtf(rx[0] * rx[0] + rx[1] * rx[1] + rx[2] * rx[2]) + 1e-8f;
    rx[0] /= rn; rx[1] /= rn; rx[2] /= rn;
    float cs = y[0] * z[0] + y[1] * z[1] + y[2] * z[2];
    cs = fminf(fmaxf(cs, -1.f + 1e-6f), 1.f - 1e-6f);
    const float theta = acosf(cs);
    const float half_pi = 1.57079632679489661923f;
    const float th2 = c1 / (c1 + c2) * (theta - half_pi);
    const float th1 = c2 / (c1 + c2) * (theta - half_pi);
    float ny[3], nz[3];
    rodrigues_apply(rx, sinf(th1), cosf(th1), y, ny);
    rodrigues_apply(rx, sinf(-th2), cosf(-th2), z, nz);
    // get_rot_mat_y_first(y = ny, x = nz)
    normalize3(ny);
    float zz[3] = {nz[1] * ny[2] - nz[2] * ny[1], nz[2] * ny[0] - nz[0] * ny[2], nz[0] * ny[1] - nz[1] * ny[0]};   // cross(x, y)
    normalize3(zz);
    const float xx[3] = {ny[1] * zz[2] - ny[2] * zz[1], ny[2] * zz[0] - ny[0] * zz[2], ny[0] * zz[1] - ny[1] * zz[0]};   // cross(y, z)
    float* o = out + (size_t)i * 16;
    for (int r = 0; r < 3; ++r) {
        o[r * 4 + 0] = xx[r]; o[r * 4 + 1] = ny[r]; o[r * 4 + 2] = zz[r]; o[r * 4 + 3] = T[i * 3 + r];
    }
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
}

}  // namespace hsp

using namespace hsp;

static int chunks_of(int pixels) { return (pixels + PC_CHUNK - 1) / PC_CHUNK; }

// the two launches of a compaction over grid (nchunk, n): count_k(in..., nchunk, cnt), then write_k(in..., nchunk, cnt, out...)
template <typename CountK, typename WriteK, typename... In, typename... Out>
static int compact_launch(CountK count_k, WriteK write_k, int n, int pixels, void* ws, hspStream_t stream,
                          const std::tuple<In...>& in, Out... out) {
    const int nchunk = chunks_of(pixels);
    const dim3 grid(nchunk, n);
    hipStream_t st = as_stream(stream);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws);
    std::apply([&](In... a) { hipLaunchKernelGGL(count_k, grid, dim3(256), 0, st, a..., nchunk, cnt); }, in);
    int rc = check_launch();
    if (rc) return rc;
    std::apply([&](In... a) { hipLaunchKernelGGL(write_k, grid, dim3(256), 0, st, a..., nchunk, cnt, out...); }, in);
    return check_launch();
}

// NC counters per chunk of each of n crops of O x O pixels
static size_t crop_workspace_bytes(int n, int O, int NC) {
    if (n <= 0 || O <= 0 || O > 46340) return 0;
    return (size_t)n * chunks_of(O * O) * NC * sizeof(int32_t);
}

extern "C" size_t hsp_pc_compact_workspace_bytes(int B, int HW) {
    if (B <= 0 || HW <= 0) return 0;
    return (size_t)B * chunks_of(HW) * sizeof(int32_t);
}

extern "C" int hsp_pc_compact(const float* mask, const float* depth, int B, int HW, int32_t* pix, int32_t* count,
                              void* ws, size_t ws_bytes, hspStream_t stream) {
    if (!mask || !depth || !pix || !count || B <= 0 || HW <= 0) return HSP_ERR_BAD_ARG;
    if (!ws || ws_bytes < hsp_pc_compact_workspace_bytes(B, HW)) return HSP_ERR_WORKSPACE;
    if (chunks_of(HW) > 65535) return HSP_ERR_UNSUPPORTED;
    return compact_launch(pc_count_kernel, pc_write_kernel, B, HW, ws, stream, std::make_tuple(mask, depth, HW), pix, count);
}

extern "C" int hsp_pc_gather(const float* depth, const float* coor2d, const float* camK, const int32_t* pix,
                             const int32_t* choose, int B, int HW, int S, float* pc, hspStream_t stream) {
    if (!depth || !coor2d || !camK || !pix || !choose || !pc || B <= 0 || HW <= 0 || S <= 0) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(pc_gather_kernel, dim3((B * S + 255) / 256), dim3(256), 0, as_stream(stream), depth, coor2d, camK,
                       pix, choose, B, HW, S, pc);
    return check_launch();
}

extern "C" int hsp_depth_to_pcl(const float* depth, const float* xymap, const double* camK, const int32_t* pix,
                                const int32_t* choose, int B, int HW, int S, float* pc, hspStream_t stream) {
    if (!depth || !xymap || !camK || !pix || !choose || !pc || B <= 0 || HW <= 0 || S <= 0) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(depth_to_pcl_kernel, dim3((B * S + 255) / 256), dim3(256), 0, as_stream(stream), depth, xymap,
                       camK, pix, choose, B, HW, S, pc);
    return check_launch();
}

extern "C" size_t hsp_roi_compact_workspace_bytes(int n, int O) { return crop_workspace_bytes(n, O, 2); }

template <typename D>
static int roi_compact(const D* depth, const uint8_t* mask, long long mask_stride, const int32_t* inst_id, const double* xf,
                       int n, int H, int W, int O, int32_t* src, int32_t* count, void* ws, size_t ws_bytes,
                       hspStream_t stream) {
    if (!depth || !mask || !xf || !src || !count || n <= 0 || H <= 0 || W <= 0 || O <= 0) return HSP_ERR_BAD_ARG;
    if ((long long)H * W > 2147483647LL || (mask_stride != 0 && mask_stride != (long long)H * W)) return HSP_ERR_BAD_ARG;
    if (O > 46340 || n > 65535) return HSP_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < hsp_roi_compact_workspace_bytes(n, O)) return HSP_ERR_WORKSPACE;
    return compact_launch(roi_count_kernel<D>, roi_write_kernel<D>, n, O * O, ws, stream,
                          std::make_tuple(depth, mask, mask_stride, inst_id, xf, H, W, O), src, count);
}

extern "C" int hsp_roi_compact_f32(const float* depth, const uint8_t* mask, long long mask_stride, const int32_t* inst_id,
                                   const double* xf, int n, int H, int W, int O, int32_t* src, int32_t* count, void* ws,
                                   size_t ws_bytes, hspStream_t stream) {
    return roi_compact(depth, mask, mask_stride, inst_id, xf, n, H, W, O, src, count, ws, ws_bytes, stream);
}

extern "C" int hsp_roi_compact_u16(const uint16_t* depth, const uint8_t* mask, long long mask_stride, const int32_t* inst_id,
                                   const double* xf, int n, int H, int W, int O, int32_t* src, int32_t* count, void* ws,
                                   size_t ws_bytes, hspStream_t stream) {
    return roi_compact(depth, mask, mask_stride, inst_id, xf, n, H, W, O, src, count, ws, ws_bytes, stream);
}

// what the tracked entry points refuse alike: the pose, the size, K and its row count, a finite pad > 0
static bool track_args_ok(const float* rt, const float* size, const double* camK, int camK_rows, int n, double pad) {
    return rt && size && camK && n > 0 && (camK_rows == 1 || camK_rows == n) && pad > 0.0 && pad < INFINITY;
}

extern "C" int hsp_pose_windows(const float* rt, const float* size, const double* camK, int camK_rows, int n, int H, int W,
                                int O, double pad, int32_t* boxes, double* xf, int32_t* wstatus, hspStream_t stream) {
    if (!track_args_ok(rt, size, camK, camK_rows, n, pad) || !boxes || !xf || !wstatus) return HSP_ERR_BAD_ARG;
    if (n > 65535 || H <= 0 || W <= 0 || (long long)H * W > 2147483647LL || O <= 0 || O > 46340) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(pose_windows_kernel, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), rt, size, camK, camK_rows, n,
                       (double)(W - 1), (double)(H - 1), (double)O, pad, boxes, xf, wstatus);
    return check_launch();
}

template <typename D>
static int roi_compact_box(const D* depth, const float* rt, const float* size, double pad, const double* camK, int camK_rows,
                           const int32_t* wstatus, const double* xf, int n, int H, int W, int O, int32_t* src, int32_t* count,
                           void* ws, size_t ws_bytes, hspStream_t stream) {
    if (!depth || !xf || !src || !count || n <= 0 || H <= 0 || W <= 0 || O <= 0) return HSP_ERR_BAD_ARG;
    if ((long long)H * W > 2147483647LL || !track_args_ok(rt, size, camK, camK_rows, n, pad)) return HSP_ERR_BAD_ARG;
    if (O > 46340 || n > 65535) return HSP_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < hsp_roi_compact_workspace_bytes(n, O)) return HSP_ERR_WORKSPACE;
    return compact_launch(box_count_kernel<D>, box_write_kernel<D>, n, O * O, ws, stream,
                          std::make_tuple(depth, rt, size, pad, camK, camK_rows, wstatus, xf, H, W, O), src, count);
}

extern "C" int hsp_roi_compact_box_f32(const float* depth, const float* rt, const float* size, double pad, const double* camK,
                                       int camK_rows, const int32_t* wstatus, const double* xf, int n, int H, int W, int O,
                                       int32_t* src, int32_t* count, void* ws, size_t ws_bytes, hspStream_t stream) {
    return roi_compact_box(depth, rt, size, pad, camK, camK_rows, wstatus, xf, n, H, W, O, src, count, ws, ws_bytes, stream);
}

extern "C" int hsp_roi_compact_box_u16(const uint16_t* depth, const float* rt, const float* size, double pad,
                                       const double* camK, int camK_rows, const int32_t* wstatus, const double* xf, int n, int H,
                                       int W, int O, int32_t* src, int32_t* count, void* ws, size_t ws_bytes, hspStream_t stream) {
    return roi_compact_box(depth, rt, size, pad, camK, camK_rows, wstatus, xf, n, H, W, O, src, count, ws, ws_bytes, stream);
}

extern "C" int hsp_track_update(const float* rt_new, const float* size_new, const int32_t* status, int n, float* rt_state,
                                float* size_state, int32_t* lost, hspStream_t stream) {
    if (!rt_new || !size_new || !status || !rt_state || !size_state || !lost || n <= 0 || n > 65535) return HSP_ERR_BAD_ARG;
    const uintptr_t a = reinterpret_cast<uintptr_t>(rt_new), b = reinterpret_cast<uintptr_t>(rt_state);
    const uintptr_t c = reinterpret_cast<uintptr_t>(size_new), d = reinterpret_cast<uintptr_t>(size_state);
    if ((a < b + (uintptr_t)n * 64 && b < a + (uintptr_t)n * 64) || (c < d + (uintptr_t)n * 12 && d < c + (uintptr_t)n * 12))
        return HSP_ERR_BAD_ARG;                                  // new and state overlap
    hipLaunchKernelGGL(track_update_kernel, dim3((n * 20 + 255) / 256), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint32_t*>(rt_new), reinterpret_cast<const uint32_t*>(size_new), status, n,
                       reinterpret_cast<uint32_t*>(rt_state), reinterpret_cast<uint32_t*>(size_state), lost);
    return check_launch();
}

// hsp_frame_to_pcl's refusals and the launch: one frame for all instances with depth_stride 0, and no bound on n beyond
// n * S < 2^31
template <typename D>
static int frame_to_pcl(const D* depth, long long depth_stride, int H, int W, const double* camK, int camK_rows,
                        const int32_t* src, long long src_stride, const int32_t* choose, int n, int S, float* pc,
                        hspStream_t stream) {
    if (!depth || !camK || !src || !choose || !pc || n <= 0 || S <= 0 || H <= 0 || W <= 0 || src_stride <= 0)
        return HSP_ERR_BAD_ARG;
    if ((long long)H * W > 2147483647LL || (camK_rows != 1 && camK_rows != n) || (long long)n * S > 2147483647LL)
        return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(frames_to_pcl_kernel<D>, dim3((n * S + 255) / 256), dim3(256), 0, as_stream(stream), depth, depth_stride,
                       H, W, camK, camK_rows, src, src_stride, choose, n, S, pc);
    return check_launch();
}

extern "C" int hsp_frame_to_pcl_f32(const float* depth, int H, int W, const double* camK, int camK_rows, const int32_t* src,
                                    long long src_stride, const int32_t* choose, int n, int S, float* pc,
                                    hspStream_t stream) {
    return frame_to_pcl(depth, 0, H, W, camK, camK_rows, src, src_stride, choose, n, S, pc, stream);
}

extern "C" int hsp_frame_to_pcl_u16(const uint16_t* depth, int H, int W, const double* camK, int camK_rows,
                                    const int32_t* src, long long src_stride, const int32_t* choose, int n, int S, float* pc,
                                    hspStream_t stream) {
    return frame_to_pcl(depth, 0, H, W, camK, camK_rows, src, src_stride, choose, n, S, pc, stream);
}

extern "C" int hsp_sample_ids(const int32_t* count, int count_stride, int n, int S, int min_pts, int min_depth_pts,
                              int short_mode, const unsigned long long* key, int32_t* choose, int32_t* status,
                              hspStream_t stream) {
    if (!count || !key || !choose || !status || n <= 0 || n > 65535 || S <= 0) return HSP_ERR_BAD_ARG;
    if ((count_stride != 1 && count_stride != 2) || (short_mode != 0 && short_mode != 1)) return HSP_ERR_BAD_ARG;
    if ((long long)n * S > 2147483647LL) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(sample_ids_kernel, dim3((unsigned)(((long long)n * S + 255) / 256)), dim3(256), 0, as_stream(stream), count, count_stride, n,
                       S, min_pts, min_depth_pts, short_mode, key, choose, status);
    return check_launch();
}

extern "C" int hsp_fps_ids_cap(void) { return FPS_IDS_CAP; }

// hsp_fps_ids's refusals -- hsp_sample_ids's and hsp_frame_to_pcl's -- and the launch: nothing is declined by shape
template <typename D>
static int fps_ids(const D* depth, int H, int W, const double* camK, int camK_rows, const int32_t* src, long long src_stride,
                   const int32_t* count, int n, int S, int min_pts, int min_depth_pts, int32_t* choose, int32_t* status,
                   hspStream_t stream) {
    if (!depth || !camK || !src || !count || !choose || !status || n <= 0 || n > 65535 || S <= 0 || H <= 0 || W <= 0 ||
        src_stride <= 0)
        return HSP_ERR_BAD_ARG;
    if ((long long)H * W > 2147483647LL || (camK_rows != 1 && camK_rows != n) || (long long)n * S > 2147483647LL)
        return HSP_ERR_BAD_ARG;
    const size_t lds = (size_t)(src_stride < FPS_IDS_CAP ? src_stride : FPS_IDS_CAP) * 3 * sizeof(float);
    return launch_lds(fps_ids_kernel<D>, dim3(n), dim3(FPS_IDS_THREADS), lds, as_stream(stream), depth, H, W, camK, camK_rows, src,
                      src_stride, count, S, min_pts, min_depth_pts, choose, status);
}

extern "C" int hsp_fps_ids_f32(const float* depth, int H, int W, const double* camK, int camK_rows, const int32_t* src,
                               long long src_stride, const int32_t* count, int n, int S, int min_pts, int min_depth_pts,
                               int32_t* choose, int32_t* status, hspStream_t stream) {
    return fps_ids(depth, H, W, camK, camK_rows, src, src_stride, count, n, S, min_pts, min_depth_pts, choose, status, stream);
}

extern "C" int hsp_fps_ids_u16(const uint16_t* depth, int H, int W, const double* camK, int camK_rows, const int32_t* src,
                               long long src_stride, const int32_t* count, int n, int S, int min_pts, int min_depth_pts,
                               int32_t* choose, int32_t* status, hspStream_t stream) {
    return fps_ids(depth, H, W, camK, camK_rows, src, src_stride, count, n, S, min_pts, min_depth_pts, choose, status, stream);
}

extern "C" int hsp_pool_rows_draw(const unsigned long long* key, int n0, int rate, int levels, int32_t* rows,
                                  hspStream_t stream) {
    if (!key || !rows || n0 <= 0 || rate <= 0 || (levels != 1 && levels != 2)) return HSP_ERR_BAD_ARG;
    const int m0 = n0 / rate, m1 = levels == 2 ? m0 / rate : 0;
    if (m0 == 0 || (levels == 2 && m1 == 0)) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(pool_rows_kernel, dim3((unsigned)(((long long)m0 + m1 + 255) / 256)), dim3(256), 0, as_stream(stream), key,
                       n0, m0, m1, rows);
    return check_launch();
}

extern "C" int hsp_dzi_windows(const int32_t* bboxes, const unsigned long long* key, int M, int H, int W, int out_size,
                               double pad_scale, double scale_ratio, double shift_ratio, double* xf, hspStream_t stream) {
    if (!bboxes || !key || !xf || M <= 0 || M > 65535 || H <= 0 || W <= 0 || out_size <= 0 || out_size > 46340)
        return HSP_ERR_BAD_ARG;
    if (!(pad_scale > 0.0) || !(scale_ratio >= 0.0 && scale_ratio < 1.0) || !(shift_ratio >= 0.0) || !(pad_scale < INFINITY) ||
        !(shift_ratio < INFINITY))
        return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(dzi_windows_kernel, dim3((M + 63) / 64), dim3(64), 0, as_stream(stream), bboxes, key, M,
                       (double)(H > W ? H : W), (double)out_size, pad_scale, scale_ratio, shift_ratio, xf);
    return check_launch();
}

// what the three entry points of the training chain refuse alike: n, O, the frame size and an element stride per instance
static bool train_shape_ok(int n, int H, int W, int O, long long stride) {
    if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || O <= 0 || O > 46340) return false;
    if ((long long)H * W > 2147483647LL) return false;
    return stride == 0 || stride == (long long)H * W;
}

extern "C" size_t hsp_roi_defor_workspace_bytes(int n, int O) { return crop_workspace_bytes(n, O, 1); }

extern "C" int hsp_roi_defor(const uint8_t* mask, long long mask_stride, const int32_t* inst_id, const double* xf, int n, int H,
                             int W, int O, int iters, unsigned long long gate, const unsigned long long* key,
                             uint8_t* crop_mask, int32_t* band, void* ws, size_t ws_bytes, hspStream_t stream) {
    if (!mask || !xf || !key || !crop_mask || !band || !train_shape_ok(n, H, W, O, mask_stride)) return HSP_ERR_BAD_ARG;
    if (iters < 1 || iters > 8 || gate > (1ULL << 32)) return HSP_ERR_BAD_ARG;
    if (!ws || ws_bytes < hsp_roi_defor_workspace_bytes(n, O)) return HSP_ERR_WORKSPACE;
    return compact_launch(defor_count_kernel, defor_write_kernel, n, O * O, ws, stream,
                          std::make_tuple(mask, mask_stride, inst_id, xf, H, W, O, iters), gate, key, crop_mask, band);
}

extern "C" size_t hsp_crop_compact_workspace_bytes(int n, int O) { return crop_workspace_bytes(n, O, 3); }

template <typename D>
static int crop_compact(const D* depth, long long depth_stride, const uint8_t* crop_mask, const double* xf, int n, int H, int W,
                        int O, int32_t* src, int32_t* count, int32_t* pre, void* ws, size_t ws_bytes, hspStream_t stream) {
    if (!depth || !crop_mask || !xf || !src || !count || !pre || !train_shape_ok(n, H, W, O, depth_stride))
        return HSP_ERR_BAD_ARG;
    if (!ws || ws_bytes < hsp_crop_compact_workspace_bytes(n, O)) return HSP_ERR_WORKSPACE;
    return compact_launch(crop_count_kernel<D>, crop_write_kernel<D>, n, O * O, ws, stream,
                          std::make_tuple(depth, depth_stride, crop_mask, xf, H, W, O), src, count, pre);
}

extern "C" int hsp_crop_compact_f32(const float* depth, long long depth_stride, const uint8_t* crop_mask, const double* xf,
                                    int n, int H, int W, int O, int32_t* src, int32_t* count, int32_t* pre, void* ws,
                                    size_t ws_bytes, hspStream_t stream) {
    return crop_compact(depth, depth_stride, crop_mask, xf, n, H, W, O, src, count, pre, ws, ws_bytes, stream);
}

extern "C" int hsp_crop_compact_u16(const uint16_t* depth, long long depth_stride, const uint8_t* crop_mask, const double* xf,
                                    int n, int H, int W, int O, int32_t* src, int32_t* count, int32_t* pre, void* ws,
                                    size_t ws_bytes, hspStream_t stream) {
    return crop_compact(depth, depth_stride, crop_mask, xf, n, H, W, O, src, count, pre, ws, ws_bytes, stream);
}

// a frame per instance (or one for all) under the training chain's bounds
template <typename D>
static int frames_to_pcl(const D* depth, long long depth_stride, int H, int W, const double* camK, int camK_rows,
                         const int32_t* src, long long src_stride, const int32_t* choose, int n, int S, float* pc,
                         hspStream_t stream) {
    if (!train_shape_ok(n, H, W, 1, depth_stride)) return HSP_ERR_BAD_ARG;
    return frame_to_pcl(depth, depth_stride, H, W, camK, camK_rows, src, src_stride, choose, n, S, pc, stream);
}

extern "C" int hsp_frames_to_pcl_f32(const float* depth, long long depth_stride, int H, int W, const double* camK,
                                     int camK_rows, const int32_t* src, long long src_stride, const int32_t* choose, int n, int S,
                                     float* pc, hspStream_t stream) {
    return frames_to_pcl(depth, depth_stride, H, W, camK, camK_rows, src, src_stride, choose, n, S, pc, stream);
}

extern "C" int hsp_frames_to_pcl_u16(const uint16_t* depth, long long depth_stride, int H, int W, const double* camK,
                                     int camK_rows, const int32_t* src, long long src_stride, const int32_t* choose, int n,
                                     int S, float* pc, hspStream_t stream) {
    return frames_to_pcl(depth, depth_stride, H, W, camK, camK_rows, src, src_stride, choose, n, S, pc, stream);
}

extern "C" int hsp_batch_select(const int32_t* status, int M, int keep, const HspSelectSeg* segs, int nseg, int32_t* sel,
                                int32_t* info, hspStream_t stream) {
    if (!status || !sel || !info || keep < 1 || keep > M || M > HSP_BATCH_SELECT_MAX_ITEMS) return HSP_ERR_BAD_ARG;
    if (nseg < 0 || nseg > HSP_BATCH_SELECT_MAX_SEGS || (nseg > 0 && !segs)) return HSP_ERR_BAD_ARG;
    BatchSelectDesc d = {};
    for (int s = 0; s < nseg; ++s) {
        const HspSelectSeg& g = segs[s];
        if (!g.src || !g.dst || g.row_bytes <= 0 || (g.row_bytes & 3) != 0) return HSP_ERR_BAD_ARG;
        const uintptr_t a = reinterpret_cast<uintptr_t>(g.src), b = reinterpret_cast<uintptr_t>(g.dst);
        if (((a | b | reinterpret_cast<uintptr_t>(g.fill)) & 3) != 0) return HSP_ERR_BAD_ARG;
        if (a < b + (uintptr_t)keep * g.row_bytes && b < a + (uintptr_t)M * g.row_bytes) return HSP_ERR_BAD_ARG;   // src and dst overlap
        d.seg[s] = g;
    }
    hipLaunchKernelGGL(batch_select_kernel, dim3(keep, nseg > 0 ? nseg : 1), dim3(256), 0, as_stream(stream), status, M, keep, nseg,
                       d, sel, info);
    return check_launch();
}

extern "C" int hsp_generate_rt(const float* p_green, const float* p_red, const float* f_green, const float* f_red,
                               const float* T, const float* sym, int sym_stride, int B, float* out,
                               hspStream_t stream) {
    if (!p_green || !p_red || !f_green || !f_red || !T || !sym || !out || B <= 0 || sym_stride <= 0) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(generate_rt_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), p_green, p_red, f_green,
                       f_red, T, sym, sym_stride, B, out);
    return check_launch();
}
