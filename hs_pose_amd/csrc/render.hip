// render.hip -- depth frames and label images rendered from meshes and poses (include/hsp.h states the contract, sentence by
// sentence): a z-buffered triangle rasteriser in the key-buffer form.  Plain HIP C++, vector stores, no inline assembly.
//
//   render_init_kernel     a 64-bit key per pixel in the workspace: all ones (empty), or with `over` the existing depth word
//                          over 0xFFFFFFFF; zeroes the chunk queue's counter
//   render_prefix_kernel   one workgroup: the running sum of the instances' triangle counts (an instance that names a mesh, a
//                          frame or a label out of range counts 0 triangles: it draws nothing and reads nothing)
//   render_small_kernel    one lane per (instance, triangle), balanced over the running sum: a triangle whose pixel box holds
//                          at most RENDER_SMALL pixels is drawn by its lane; a larger one is cut into RENDER_CW x RENDER_CH
//                          pixel chunks that go to the queue (a chunk the queue has no room for is drawn by the lane)
//   render_chunk_kernel    one wave per queued chunk, the 64 lanes along the chunk's rows
//   render_resolve_kernel  key -> depth word and label, four pixels per lane where the addresses allow
//
// A fragment is one no-return 64-bit unsigned atomicMin ((word << 32) | instance) on the pixel's key: the minimum does not
// depend on the order of arrival, so neither does the frame.  Every float64 operation of the contract is spelled with its _rn
// form -- one rounding each, in the header's order -- and both raster kernels run the SAME device functions (tri_setup,
// fragment), so which of them draws a pixel does not change a bit.
#include "common.h"

namespace hsp {
namespace {

constexpr int RENDER_SMALL = 64;                 // pixel boxes up to this many pixels stay with their lane
constexpr int RENDER_CW = 64, RENDER_CH = 16;    // a queued chunk: one wave, 16 steps
constexpr unsigned long long KEY_EMPTY = ~0ull;
constexpr unsigned KEEP = 0xFFFFFFFFu;           // low word of a key made of the existing frame

__device__ __forceinline__ bool fin64(double x) { return fabs(x) < INFINITY; }      // (false for NaN)

struct RenderArgs {
    const float* verts;
    const int32_t* tris;
    const int32_t* mesh;
    const int32_t* mesh_id;
    const int32_t* frame_id;
    const int32_t* label;
    const float* rt;
    const float* scale;
    const double* camK;
    int camK_rows, n, n_mesh, V, T, F, H, W;
};

// the valid triangle count of instance j: 0 where it draws nothing
__device__ __forceinline__ int instance_tris(const RenderArgs& a, int j) {
    const int m = a.mesh_id[j], f = a.frame_id[j], l = a.label[j];
    if (m < 0 || m >= a.n_mesh || f < 0 || f >= a.F || l < 1 || l > 255) return 0;
    const int v0 = a.mesh[m * 4 + 0], nv = a.mesh[m * 4 + 1], t0 = a.mesh[m * 4 + 2], nt = a.mesh[m * 4 + 3];
    if (v0 < 0 || nv <= 0 || t0 < 0 || nt <= 0 || (long long)v0 + nv > a.V || (long long)t0 + nt > a.T) return 0;
    return nt;
}

// prefix[j] = triangles of the instances before j, prefix[n] = all of them.  One workgroup of 256: a run of consecutive
// instances per thread, the runs' sums scanned in LDS.
__global__ __launch_bounds__(256) void render_prefix_kernel(RenderArgs a, long long* __restrict__ prefix) {
    __shared__ long long s_sum[256];
    const int t = threadIdx.x, per = (a.n + 255) / 256;
    const int lo = min(t * per, a.n), hi = min(lo + per, a.n);
    long long sum = 0;
    for (int j = lo; j < hi; ++j) sum += instance_tris(a, j);
    s_sum[t] = sum;
    __syncthreads();
    long long before = 0;
    for (int i = 0; i < t; ++i) before += s_sum[i];
    for (int j = lo; j < hi; ++j) {
        prefix[j] = before;
        before += instance_tris(a, j);
    }
    if (t == 255) prefix[a.n] = before;
}

// the instance whose run of triangles holds g: the last j with prefix[j] <= g (instances without triangles are skipped)
__device__ __forceinline__ int find_instance(const long long* __restrict__ prefix, int n, long long g) {
    int lo = 0, hi = n;                     // prefix[lo] <= g < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// what a triangle's pixels need: the three canonical edges (a < b by vertex index, c the row's vertex k), the vertices' Z and
// the candidate pixel box
struct TriSetup {
    double ua[3], va[3], dx[3], dy[3], A[3], Z[3];
    int x0, x1, y0, y1;
};

// e_k(q) = (u_b - u_a) * (q_y - v_a) - (v_b - v_a) * (q_x - u_a)
__device__ __forceinline__ double edge(const TriSetup& s, int k, double qx, double qy) {
    return __dsub_rn(__dmul_rn(s.dx[k], __dsub_rn(qy, s.va[k])), __dmul_rn(s.dy[k], __dsub_rn(qx, s.ua[k])));
}

// triangle `tri` of instance j -> its setup; false where the contract drops it or no pixel of the frame is a candidate
__device__ __forceinline__ bool tri_setup(const RenderArgs& a, int j, int tri, TriSetup& s) {
    const int m = a.mesh_id[j];
    const int v0 = a.mesh[m * 4 + 0], nv = a.mesh[m * 4 + 1], t0 = a.mesh[m * 4 + 2];
    const int32_t* __restrict__ row = a.tris + ((size_t)t0 + tri) * 3;
    const int id[3] = {row[0], row[1], row[2]};
    if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (id[k] < 0 || id[k] >= nv) return false;          // (the host checks a mesh set once; this keeps the loads in bounds)
    const float* __restrict__ rt = a.rt + (size_t)j * 16;
    const float* __restrict__ sc = a.scale + (size_t)j * 3;
    const double* __restrict__ K = a.camK + (a.camK_rows > 1 ? (size_t)a.frame_id[j] * 9 : 0);
    const double K0 = K[0], K2 = K[2], K4 = K[4], K5 = K[5];
    const double s0 = (double)sc[0], s1 = (double)sc[1], s2 = (double)sc[2];
    double u[3], v[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* __restrict__ p = a.verts + ((size_t)v0 + id[k]) * 3;
        const double m0 = __dmul_rn(s0, (double)p[0]), m1 = __dmul_rn(s1, (double)p[1]), m2 = __dmul_rn(s2, (double)p[2]);
        double c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            c[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)rt[r * 4], m0), __dmul_rn((double)rt[r * 4 + 1], m1)),
                                       __dmul_rn((double)rt[r * 4 + 2], m2)), (double)rt[r * 4 + 3]);
        u[k] = __dadd_rn(__ddiv_rn(__dmul_rn(K0, c[0]), c[2]), K2);
        v[k] = __dadd_rn(__ddiv_rn(__dmul_rn(K4, c[1]), c[2]), K5);
        s.Z[k] = c[2];
        ok = ok && c[2] > 0.0 && fin64(c[2]) && fin64(u[k]) && fin64(v[k]);
    }
    if (!ok) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const int ia = id[k1] < id[k2] ? k1 : k2, ib = id[k1] < id[k2] ? k2 : k1;
        s.ua[k] = u[ia]; s.va[k] = v[ia];
        s.dx[k] = __dsub_rn(u[ib], u[ia]);
        s.dy[k] = __dsub_rn(v[ib], v[ia]);
        s.A[k] = edge(s, k, u[k], v[k]);
        if (s.A[k] == 0.0 || !fin64(s.A[k])) return false;
    }
    // candidates: floor(min u) <= px <= ceil(max u), floor(min v) <= py <= ceil(max v), inside the frame.  Compared as doubles:
    // whatever the extremes, the four values that reach the conversion lie inside the frame
    const double xlo = fmax(0.0, floor(fmin(fmin(u[0], u[1]), u[2]))), xhi = fmin((double)(a.W - 1), ceil(fmax(fmax(u[0], u[1]), u[2])));
    const double ylo = fmax(0.0, floor(fmin(fmin(v[0], v[1]), v[2]))), yhi = fmin((double)(a.H - 1), ceil(fmax(fmax(v[0], v[1]), v[2])));
    if (!(xlo <= xhi && ylo <= yhi)) return false;
    s.x0 = (int)xlo; s.x1 = (int)xhi; s.y0 = (int)ylo; s.y1 = (int)yhi;
    return true;
}

// the fragment of pixel (px, py), if the triangle has one there, into the pixel's key
template <bool F32>
__device__ __forceinline__ void fragment(const TriSetup& s, int px, int py, unsigned j, unsigned long long* __restrict__ key) {
    const double qx = (double)px, qy = (double)py;
    double e[3];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e[k] = edge(s, k, qx, qy);
        in = in && (s.A[k] > 0.0 ? e[k] >= 0.0 : e[k] <= 0.0);
    }
    if (!in) return;
    const double l0 = __ddiv_rn(e[0], s.A[0]), l1 = __ddiv_rn(e[1], s.A[1]), l2 = __ddiv_rn(e[2], s.A[2]);
    const double inv = __dadd_rn(__dadd_rn(__ddiv_rn(l0, s.Z[0]), __ddiv_rn(l1, s.Z[1])), __ddiv_rn(l2, s.Z[2]));
    const double zmm = __dmul_rn(__ddiv_rn(__dadd_rn(__dadd_rn(l0, l1), l2), inv), 1000.0);
    unsigned word;
    if (F32) {
        const float f = (float)zmm;
        if (!(f > 0.0f && f < INFINITY)) return;
        word = __float_as_uint(f);
    } else {
        const double q = rint(zmm);
        if (!(q >= 1.0 && q <= 65535.0)) return;
        word = (unsigned)q;
    }
    atomicMin(key, ((unsigned long long)word << 32) | j);
}

// chunk c of the pixel box: lanes `first`, `first + step`, ... of its RENDER_CW x RENDER_CH pixels
template <bool F32>
__device__ __forceinline__ void raster_chunk(const TriSetup& s, int c, int first, int step, unsigned j,
                                             unsigned long long* __restrict__ keys, int W) {
    const int ncx = (s.x1 - s.x0) / RENDER_CW + 1;
    const int cy = c / ncx, cx = c - cy * ncx;
    const int bx = s.x0 + cx * RENDER_CW, by = s.y0 + cy * RENDER_CH;
    for (int i = first; i < RENDER_CW * RENDER_CH; i += step) {
        const int px = bx + (i % RENDER_CW), py = by + (i / RENDER_CW);
        if (px <= s.x1 && py <= s.y1) fragment<F32>(s, px, py, j, keys + (size_t)py * W + px);
    }
}

struct ChunkQueue {
    unsigned long long* count;      // chunks asked for, may pass cap
    int4* entry;                    // (instance, triangle, chunk, 0)
    long long cap;
};

template <bool F32>
__global__ __launch_bounds__(256) void render_small_kernel(RenderArgs a, const long long* __restrict__ prefix,
                                                           unsigned long long* __restrict__ keys, ChunkQueue q) {
    const long long total = prefix[a.n], stride = (long long)gridDim.x * 256;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += stride) {
        const int j = find_instance(prefix, a.n, g);
        const int tri = (int)(g - prefix[j]);
        TriSetup s;
        if (!tri_setup(a, j, tri, s)) continue;
        unsigned long long* __restrict__ fkeys = keys + (size_t)a.frame_id[j] * a.H * a.W;
        const int w = s.x1 - s.x0 + 1, h = s.y1 - s.y0 + 1;
        if ((long long)w * h <= RENDER_SMALL) {
            for (int py = s.y0; py <= s.y1; ++py)
                for (int px = s.x0; px <= s.x1; ++px) fragment<F32>(s, px, py, (unsigned)j, fkeys + (size_t)py * a.W + px);
            continue;
        }
        const int nchunk = ((w - 1) / RENDER_CW + 1) * ((h - 1) / RENDER_CH + 1);
        const unsigned long long base = atomicAdd(q.count, (unsigned long long)nchunk);
        for (int c = 0; c < nchunk; ++c) {
            if (base + c < (unsigned long long)q.cap) q.entry[base + c] = make_int4(j, tri, c, 0);
            else raster_chunk<F32>(s, c, 0, 1, (unsigned)j, fkeys, a.W);         // no room: the lane draws the chunk itself
        }
    }
}

template <bool F32>
__global__ __launch_bounds__(256) void render_chunk_kernel(RenderArgs a, unsigned long long* __restrict__ keys, ChunkQueue q) {
    const unsigned long long asked = *q.count;
    const long long count = asked < (unsigned long long)q.cap ? (long long)asked : q.cap;
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < count; e += waves) {
        const int4 w = q.entry[e];
        TriSetup s;                                       // every lane makes the same setup: the same bits the queueing lane had
        if (!tri_setup(a, w.x, w.y, s)) continue;
        raster_chunk<F32>(s, w.z, lane, 64, (unsigned)w.x, keys + (size_t)a.frame_id[w.x] * a.H * a.W, a.W);
    }
}

template <typename D> __device__ __forceinline__ bool depth_counts(D d, unsigned& word);
template <> __device__ __forceinline__ bool depth_counts<uint16_t>(uint16_t d, unsigned& word) { word = d; return d > 0; }
template <> __device__ __forceinline__ bool depth_counts<float>(float d, unsigned& word) {
    word = __float_as_uint(d);
    return d > 0.0f && d < INFINITY;
}

template <typename D>
__global__ __launch_bounds__(256) void render_init_kernel(const D* __restrict__ depth, int over, long long npix,
                                                          unsigned long long* __restrict__ keys,
                                                          unsigned long long* __restrict__ qcount) {
    const long long stride = (long long)gridDim.x * 256;
    if (blockIdx.x == 0 && threadIdx.x == 0) *qcount = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += stride) {
        unsigned word;
        keys[p] = (over && depth_counts<D>(depth[p], word)) ? (((unsigned long long)word << 32) | KEEP) : KEY_EMPTY;
    }
}

template <typename D> struct Vec4;
template <> struct Vec4<uint16_t> { typedef ushort4 type; };
template <> struct Vec4<float> { typedef float4 type; };
template <typename D> __device__ __forceinline__ D word_depth(unsigned word);
template <> __device__ __forceinline__ uint16_t word_depth<uint16_t>(unsigned word) { return (uint16_t)word; }
template <> __device__ __forceinline__ float word_depth<float>(unsigned word) { return __uint_as_float(word); }

// V pixels per lane (4 where depth and labels allow whole-vector stores, else 1).  An empty pixel gets depth 0 and label 0, a
// pixel the existing frame won keeps its label and is given its own depth word again.
template <typename D, int V>
__global__ __launch_bounds__(256) void render_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                             const int32_t* __restrict__ label, int n, long long npix,
                                                             D* __restrict__ depth, uint8_t* __restrict__ labels) {
    const long long stride = (long long)gridDim.x * 256 * V;
    for (long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * V; p < npix; p += stride) {
        D d[V];
        uint8_t l[V];
        if (V == 4 && p + 4 <= npix) {
            const uchar4 old = *reinterpret_cast<const uchar4*>(labels + p);
            l[0] = old.x; l[1 % V] = old.y; l[2 % V] = old.z; l[3 % V] = old.w;
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) l[i] = p + i < npix ? labels[p + i] : 0;
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const unsigned long long k = p + i < npix ? keys[p + i] : KEY_EMPTY;
            const unsigned lo = (unsigned)k;
            d[i] = k == KEY_EMPTY ? word_depth<D>(0) : word_depth<D>((unsigned)(k >> 32));
            if (k == KEY_EMPTY) l[i] = 0;
            else if (lo != KEEP) l[i] = lo < (unsigned)n ? (uint8_t)label[lo] : 0;
        }
        if (V == 4 && p + 4 <= npix) {
            typename Vec4<D>::type dv;
            dv.x = d[0]; dv.y = d[1 % V]; dv.z = d[2 % V]; dv.w = d[3 % V];
            *reinterpret_cast<typename Vec4<D>::type*>(depth + p) = dv;
            *reinterpret_cast<uchar4*>(labels + p) = make_uchar4(l[0], l[1 % V], l[2 % V], l[3 % V]);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (p + i < npix) { depth[p + i] = d[i]; labels[p + i] = l[i]; }
        }
    }
}

// ---- hsp_label_boxes: one workgroup per instance over its frame, integer min / max / add only -------------------------------
struct BoxAcc {
    int x1, y1, x2, y2, cnt;
    __device__ __forceinline__ void take(int x, int y) {
        x1 = min(x1, x); y1 = min(y1, y); x2 = max(x2, x); y2 = max(y2, y); ++cnt;
    }
    __device__ __forceinline__ void join(const BoxAcc& o) {
        x1 = min(x1, o.x1); y1 = min(y1, o.y1); x2 = max(x2, o.x2); y2 = max(y2, o.y2); cnt += o.cnt;
    }
};

// GUARD: a label without a pixel gets the box (0, 0, 1, 1) -- a positive side for hsp_dzi_windows -- instead of zeros; the
// count stays 0.  One body for hsp_label_boxes and hsp_label_boxes_guarded: where the count is positive they write the same bits.
template <bool GUARD>
__global__ __launch_bounds__(1024) void label_boxes_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ frame_id,
                                                           const int32_t* __restrict__ label, int F, int H, int W,
                                                           int32_t* __restrict__ boxes, int32_t* __restrict__ count) {
    __shared__ BoxAcc s_acc[16];
    const int j = blockIdx.x, t = threadIdx.x, f = frame_id[j], want = label[j];
    BoxAcc acc = {INT_MAX, INT_MAX, -1, -1, 0};
    if (f >= 0 && f < F && want >= 1 && want <= 255) {               // (wave-uniform: one instance per workgroup)
        const int HW = H * W;
        const uint8_t* __restrict__ img = labels + (size_t)f * HW;
        // scalar up to the first 16-byte boundary, 16 bytes per lane from there, scalar again for the rest
        const int head = min(HW, (int)((16 - (reinterpret_cast<uintptr_t>(img) & 15)) & 15));
        const int nvec = (HW - head) / 16, tail = head + nvec * 16;
        const unsigned rep = (unsigned)want * 0x01010101u;
        for (int p = t; p < head; p += 1024)
            if (img[p] == want) acc.take(p % W, p / W);
        for (int p = tail + t; p < HW; p += 1024)
            if (img[p] == want) acc.take(p % W, p / W);
        const uint4* __restrict__ vec = reinterpret_cast<const uint4*>(img + head);
        for (int i = t; i < nvec; i += 1024) {
            const uint4 q = vec[i];
            const unsigned w4[4] = {q.x ^ rep, q.y ^ rep, q.z ^ rep, q.w ^ rep};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (((w4[k] - 0x01010101u) & ~w4[k] & 0x80808080u) == 0) continue;       // no byte of the word is zero
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (((w4[k] >> (8 * b)) & 0xffu) == 0) {
                        const int p = head + i * 16 + k * 4 + b;
                        acc.take(p % W, p / W);
                    }
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        BoxAcc other = {__shfl_xor(acc.x1, o), __shfl_xor(acc.y1, o), __shfl_xor(acc.x2, o), __shfl_xor(acc.y2, o),
                        __shfl_xor(acc.cnt, o)};
        acc.join(other);
    }
    if ((t & 63) == 0) s_acc[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 16; ++w) acc.join(s_acc[w]);
        int32_t* __restrict__ b = boxes + (size_t)j * 4;
        const bool any = acc.cnt > 0;
        b[0] = any ? acc.x1 : 0; b[1] = any ? acc.y1 : 0; b[2] = any ? acc.x2 + 1 : (GUARD ? 1 : 0);
        b[3] = any ? acc.y2 + 1 : (GUARD ? 1 : 0);
        count[j] = acc.cnt;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

struct RenderLayout {
    size_t keys, prefix, qcount, queue, total;
    long long cap;
};

bool frame_sizes_ok(int F, int H, int W) { return F >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 2147483647LL; }

// keys (F*H*W) | prefix (n + 1) | the queue's counter | the queue: room for 16 frames' worth of chunks per frame, at most 2^22
RenderLayout render_layout(int F, int H, int W, int n) {
    RenderLayout L;
    const long long chunks = (long long)((W - 1) / RENDER_CW + 1) * ((H - 1) / RENDER_CH + 1);
    L.cap = 16LL * F * chunks < (1LL << 22) ? 16LL * F * chunks : (1LL << 22);
    L.keys = 0;
    L.prefix = up16((size_t)F * H * W * 8);
    L.qcount = L.prefix + up16(((size_t)n + 1) * 8);
    L.queue = L.qcount + 16;
    L.total = L.queue + (size_t)L.cap * 16;
    return L;
}

template <typename D>
int render_depth(const float* verts, int V, const int32_t* tris, int T, const int32_t* mesh, int n_mesh, const int32_t* mesh_id,
                 const int32_t* frame_id, const int32_t* label, const float* rt, const float* scale, const double* camK,
                 int camK_rows, int n, int F, int H, int W, int over, D* depth, uint8_t* labels, void* ws, size_t ws_bytes,
                 hspStream_t stream) {
    if (!depth || !labels || !frame_sizes_ok(F, H, W) || n < 0 || n > 65535 || (over != 0 && over != 1)) return HSP_ERR_BAD_ARG;
    if (n > 0 && (!verts || !tris || !mesh || !mesh_id || !frame_id || !label || !rt || !scale || !camK || V < 1 || T < 1 ||
                  n_mesh < 1 || (camK_rows != 1 && camK_rows != F)))
        return HSP_ERR_BAD_ARG;
    const RenderLayout L = render_layout(F, H, W, n);
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < L.total) return HSP_ERR_WORKSPACE;
    char* base = static_cast<char*>(ws);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + L.keys);
    long long* prefix = reinterpret_cast<long long*>(base + L.prefix);
    const ChunkQueue q = {reinterpret_cast<unsigned long long*>(base + L.qcount), reinterpret_cast<int4*>(base + L.queue), L.cap};
    const long long npix = (long long)F * H * W;
    const hipStream_t st = as_stream(stream);
    constexpr bool F32 = sizeof(D) == 4;
    hipLaunchKernelGGL(render_init_kernel<D>, dim3(persistent_blocks((npix + 255) / 256, 8)), dim3(256), 0, st, depth, over, npix,
                       keys, q.count);
    if (n > 0) {
        const RenderArgs a = {verts, tris, mesh, mesh_id, frame_id, label, rt, scale, camK, camK_rows, n, n_mesh, V, T, F, H, W};
        hipLaunchKernelGGL(render_prefix_kernel, dim3(1), dim3(256), 0, st, a, prefix);
        hipLaunchKernelGGL(render_small_kernel<F32>, dim3(persistent_blocks(((long long)n * T + 255) / 256, 8)), dim3(256), 0, st, a,
                           prefix, keys, q);
        hipLaunchKernelGGL(render_chunk_kernel<F32>, dim3(persistent_blocks((L.cap + 3) / 4, 4)), dim3(256), 0, st, a, keys, q);
    }
    const bool vec = ((reinterpret_cast<uintptr_t>(depth) & (4 * sizeof(D) - 1)) | (reinterpret_cast<uintptr_t>(labels) & 3)) == 0;
    if (vec)
        hipLaunchKernelGGL((render_resolve_kernel<D, 4>), dim3(persistent_blocks((npix + 1023) / 1024, 8)), dim3(256), 0, st, keys,
                           label, n, npix, depth, labels);
    else
        hipLaunchKernelGGL((render_resolve_kernel<D, 1>), dim3(persistent_blocks((npix + 255) / 256, 8)), dim3(256), 0, st, keys,
                           label, n, npix, depth, labels);
    return check_launch();
}

}  // namespace
}  // namespace hsp

using namespace hsp;

extern "C" size_t hsp_render_workspace_bytes(int F, int H, int W, int n) {
    if (!frame_sizes_ok(F, H, W) || n < 0 || n > 65535) return 0;
    return render_layout(F, H, W, n).total;
}

extern "C" int hsp_render_depth_u16(const float* verts, int V, const int32_t* tris, int T, const int32_t* mesh, int n_mesh,
                                    const int32_t* mesh_id, const int32_t* frame_id, const int32_t* label, const float* rt,
                                    const float* scale, const double* camK, int camK_rows, int n, int F, int H, int W, int over,
                                    uint16_t* depth, uint8_t* labels, void* ws, size_t ws_bytes, hspStream_t stream) {
    return render_depth(verts, V, tris, T, mesh, n_mesh, mesh_id, frame_id, label, rt, scale, camK, camK_rows, n, F, H, W, over,
                        depth, labels, ws, ws_bytes, stream);
}

extern "C" int hsp_render_depth_f32(const float* verts, int V, const int32_t* tris, int T, const int32_t* mesh, int n_mesh,
                                    const int32_t* mesh_id, const int32_t* frame_id, const int32_t* label, const float* rt,
                                    const float* scale, const double* camK, int camK_rows, int n, int F, int H, int W, int over,
                                    float* depth, uint8_t* labels, void* ws, size_t ws_bytes, hspStream_t stream) {
    return render_depth(verts, V, tris, T, mesh, n_mesh, mesh_id, frame_id, label, rt, scale, camK, camK_rows, n, F, H, W, over,
                        depth, labels, ws, ws_bytes, stream);
}

template <bool GUARD>
static int label_boxes(const uint8_t* labels, const int32_t* frame_id, const int32_t* label, int n, int F, int H, int W,
                       int32_t* boxes, int32_t* count, hspStream_t stream) {
    if (!labels || !frame_id || !label || !boxes || !count || n < 1 || n > 65535 || !frame_sizes_ok(F, H, W)) return HSP_ERR_BAD_ARG;
    hipLaunchKernelGGL(label_boxes_kernel<GUARD>, dim3(n), dim3(1024), 0, as_stream(stream), labels, frame_id, label, F, H, W, boxes,
                       count);
    return check_launch();
}

extern "C" int hsp_label_boxes(const uint8_t* labels, const int32_t* frame_id, const int32_t* label, int n, int F, int H, int W,
                               int32_t* boxes, int32_t* count, hspStream_t stream) {
    return label_boxes<false>(labels, frame_id, label, n, F, H, W, boxes, count, stream);
}

extern "C" int hsp_label_boxes_guarded(const uint8_t* labels, const int32_t* frame_id, const int32_t* label, int n, int F, int H,
                                       int W, int32_t* boxes, int32_t* count, hspStream_t stream) {
    return label_boxes<true>(labels, frame_id, label, n, F, H, W, boxes, count, stream);
}
