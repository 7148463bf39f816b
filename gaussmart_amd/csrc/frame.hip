// Frame kernels (gfx950): the maps of a render package, already in HBM, become 8-bit pictures and video frames next to them
// (include/gsr.h, FRAME_*; Python: gaussmart_amd/frames.py).
//
//   frame_to_u8_kernel       fp32 [B,C,H,W] -> u8 [B,H,W,C]; W % 4 == 0: four pixels of a row per thread, one 16-byte load per
//                            channel plane and the 4 C output bytes as whole dwords; otherwise one pixel per thread
//   frame_keys_kernel        nan_to_num(values) as order-preserving u32 keys (then gsr_sort_pairs_u32)
//   frame_pick_kernel        the keys at the k asked ranks, back as floats
//   frame_depth_vis_kernel   depth -> cleaned fp32 depth and the turbo video frame; the 768-byte table staged once per workgroup
//   frame_sobel_kernel       gradient_map: both Sobel responses per channel, magnitude, L2 norm over the channels; C looped
//   frame_minmax_kernel      min and max of a map: 16-byte loads, wave_reduce.h, one integer atomic per wave and bound
//   frame_colormap_kernel    (x - min) / (max - min) * 255, rint, 256 x 3 fp32 table staged once per workgroup
//
// This file is compiled with -ffp-contract=off: every sum, product and quotient below rounds on its own, which is what makes
// the Sobel sums, the colormap index and the fp64 normalisation of the depth frame the bits of their host twins.
// Every kernel is a grid-stride loop over 64-bit element offsets; no kernel uses floating-point atomics.
#include "gsr_common.h"
#include "wave_reduce.h"

#define FRAME_THREADS 256
#define FRAME_MAX_BLOCKS (1 << 16)
#define FRAME_MAX_RANKS 8

static inline unsigned frame_blocks(int64_t items) {
    int64_t b = (items + FRAME_THREADS - 1) / FRAME_THREADS;
    if (b > FRAME_MAX_BLOCKS) b = FRAME_MAX_BLOCKS;
    return (unsigned)(b > 0 ? b : 1);
}
static inline bool frame_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// numpy's nan_to_num on fp32: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float frame_nan_to_num(float x) {
    if (x != x) return 0.0f;
    return fminf(fmaxf(x, -FLT_MAX), FLT_MAX);
}
// FRAME_U8: uint8(clip(nan_to_num(x), 0, 1) * 255.0f), one fp32 multiply, truncation
__device__ __forceinline__ uint32_t frame_u8(float x) {
    const float c = (x != x) ? 0.0f : fminf(fmaxf(x, 0.0f), 1.0f);
    return (uint32_t)(int)(c * 255.0f);
}
// u(a) < u(b) exactly when a < b (-0 below +0), and back
__device__ __forceinline__ uint32_t frame_f2ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float frame_ord2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// ------------------------------------------------------------------------------- to_u8
template <int C>
__global__ void __launch_bounds__(FRAME_THREADS) frame_to_u8_vec_kernel(const float* __restrict__ in, int64_t images,
                                                                        int64_t plane, uint8_t* __restrict__ out) {
    // one thread: pixels [4 q, 4 q + 4) of one image (plane % 4 == 0, so a group never straddles two images)
    const int64_t qpi = plane / 4, total = images * qpi, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t b = i / qpi, p = (i - b * qpi) * 4;
        uint32_t v[C][4];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float4 f = *reinterpret_cast<const float4*>(in + (b * C + c) * plane + p);
            v[c][0] = frame_u8(f.x); v[c][1] = frame_u8(f.y); v[c][2] = frame_u8(f.z); v[c][3] = frame_u8(f.w);
        }
        uint32_t w[C];    // the 4 C bytes in output order (pixel-major, channel fastest)
#pragma unroll
        for (int d = 0; d < C; ++d) {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int byte = 4 * d + k;
                word |= v[byte % C][byte / C] << (8 * k);
            }
            w[d] = word;
        }
        uint32_t* o = reinterpret_cast<uint32_t*>(out + (b * plane + p) * C);
#pragma unroll
        for (int d = 0; d < C; ++d) o[d] = w[d];
    }
}
__global__ void __launch_bounds__(FRAME_THREADS) frame_to_u8_scalar_kernel(const float* __restrict__ in, int64_t images, int C,
                                                                           int64_t plane, uint8_t* __restrict__ out) {
    const int64_t total = images * plane, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t b = i / plane, p = i - b * plane;
        for (int c = 0; c < C; ++c) out[i * C + c] = (uint8_t)frame_u8(in[(b * C + c) * plane + p]);
    }
}

extern "C" int32_t gsr_frame_to_u8(const float* in, int32_t B, int32_t C, int32_t H, int32_t W, uint8_t* out,
                                   gsr_stream_t stream_) {
    if (B < 0 || H < 0 || W < 0) { gsr_set_error("frame_to_u8: negative size (%d, %d, %d)", B, H, W); return GSR_E_INVALID; }
    if (C != 1 && C != 3 && C != 4) { gsr_set_error("frame_to_u8: channels must be 1, 3 or 4 (got %d)", C); return GSR_E_UNSUPPORTED; }
    const int64_t plane = (int64_t)H * W;
    if (B == 0 || plane == 0) return GSR_OK;
    if (!in || !out) { gsr_set_error("frame_to_u8: in and out are required"); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (W % 4 == 0 && frame_aligned16(in) && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
        const dim3 grid(frame_blocks((int64_t)B * (plane / 4))), block(FRAME_THREADS);
        if (C == 1) hipLaunchKernelGGL(frame_to_u8_vec_kernel<1>, grid, block, 0, s, in, (int64_t)B, plane, out);
        else if (C == 3) hipLaunchKernelGGL(frame_to_u8_vec_kernel<3>, grid, block, 0, s, in, (int64_t)B, plane, out);
        else hipLaunchKernelGGL(frame_to_u8_vec_kernel<4>, grid, block, 0, s, in, (int64_t)B, plane, out);
    } else {
        hipLaunchKernelGGL(frame_to_u8_scalar_kernel, dim3(frame_blocks((int64_t)B * plane)), dim3(FRAME_THREADS), 0, s, in,
                           (int64_t)B, C, plane, out);
    }
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ------------------------------------------------------------------------------- order statistics
struct FrameRanks { int64_t r[FRAME_MAX_RANKS]; };

__global__ void __launch_bounds__(FRAME_THREADS) frame_keys_kernel(const float* __restrict__ v, int64_t n,
                                                                   uint32_t* __restrict__ keys) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        keys[i] = frame_f2ord(frame_nan_to_num(v[i]));
}
__global__ void frame_pick_kernel(const uint32_t* __restrict__ sorted, FrameRanks ranks, int k, float* __restrict__ out) {
    const int j = threadIdx.x;
    if (j < k) out[j] = frame_ord2f(sorted[ranks.r[j]]);
}

struct FrameStatsWs {
    uint32_t *keys, *sorted, *vals;
    float* picked;
    void* sort_ws;
    size_t sort_bytes, total;
    FrameStatsWs(void* base, int64_t n) {
        GsrWsCursor c(base);
        const size_t nb = size_t(n > 0 ? n : 1) * 4;
        keys = c.take<uint32_t>(nb);
        sorted = c.take<uint32_t>(nb);
        vals = c.take<uint32_t>(nb);
        picked = c.take<float>(FRAME_MAX_RANKS * 4);
        sort_bytes = gsr_sort_workspace_bytes((int32_t)(n > 0 ? n : 1));
        sort_ws = c.take<void>(sort_bytes);
        total = c.off;
    }
};

extern "C" size_t gsr_frame_order_stats_workspace_bytes(int64_t n) {
    if (n < 0 || n > 0x7fffffffLL) return 0;
    return FrameStatsWs(nullptr, n).total;
}

extern "C" int32_t gsr_frame_order_stats(const float* values, int64_t n, const int64_t* ranks_host, int32_t k, float* out_host,
                                         void* ws_, size_t ws_bytes, gsr_stream_t stream_) {
    if (n < 1) { gsr_set_error("frame_order_stats: n must be >= 1 (got %lld)", (long long)n); return GSR_E_INVALID; }
    if (n > 0x7fffffffLL) { gsr_set_error("frame_order_stats: n %lld exceeds the sort's 2^31 - 1 elements", (long long)n); return GSR_E_UNSUPPORTED; }
    if (k < 1 || k > FRAME_MAX_RANKS) { gsr_set_error("frame_order_stats: k must be in 1..%d (got %d)", FRAME_MAX_RANKS, k); return GSR_E_INVALID; }
    if (!values || !ranks_host || !out_host || !ws_) { gsr_set_error("frame_order_stats: null argument"); return GSR_E_INVALID; }
    FrameRanks ranks = {};
    for (int j = 0; j < k; ++j) {
        if (ranks_host[j] < 0 || ranks_host[j] >= n) {
            gsr_set_error("frame_order_stats: rank %lld outside [0, %lld)", (long long)ranks_host[j], (long long)n);
            return GSR_E_INVALID;
        }
        ranks.r[j] = ranks_host[j];
    }
    const FrameStatsWs ws(ws_, n);
    if (ws_bytes < ws.total) { gsr_set_error("frame_order_stats: workspace too small (%zu < %zu)", ws_bytes, ws.total); return GSR_E_INVALID; }
    unsigned long long* host = gsr_pinned_words(FRAME_MAX_RANKS / 2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(frame_keys_kernel, dim3(frame_blocks(n)), dim3(FRAME_THREADS), 0, s, values, n, ws.keys);
    GSR_LAUNCH_CHECK();
    // values: the element indices (vals_in == NULL), not used afterwards
    const int rc = gsr_sort_pairs_u32(ws.keys, nullptr, ws.sorted, ws.vals, (int32_t)n, 0, 32, ws.sort_ws, ws.sort_bytes, stream_);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(frame_pick_kernel, dim3(1), dim3(64), 0, s, ws.sorted, ranks, (int)k, ws.picked);
    GSR_LAUNCH_CHECK();
    // the one read-back: the k floats
    GSR_HIP_CHECK(hipMemcpyAsync(host, ws.picked, size_t(k) * 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    const float* h = reinterpret_cast<const float*>(host);
    for (int j = 0; j < k; ++j) out_host[j] = h[j];
    return GSR_OK;
}

// ------------------------------------------------------------------------------- depth frame
// FRAME_DEPTH of one pixel: the packed (r | g << 8 | b << 16) of the cleaned depth d
__device__ __forceinline__ uint32_t frame_depth_rgb(float d, double lo, double den, const uint8_t* tab) {
    const double t = ((double)logf(d) - lo) / den;
    if (t != t) return 0u;
    const double tc = fmin(fmax(t, 0.0), 1.0);
    int idx = (int)(tc * 256.0);
    if (idx > 255) idx = 255;
    return (uint32_t)tab[3 * idx] | ((uint32_t)tab[3 * idx + 1] << 8) | ((uint32_t)tab[3 * idx + 2] << 16);
}

__global__ void __launch_bounds__(FRAME_THREADS) frame_depth_vis_kernel(const float* __restrict__ depth, int64_t n, double lo,
                                                                        double den, const uint8_t* __restrict__ table,
                                                                        float* __restrict__ clean, uint8_t* __restrict__ frame,
                                                                        int vec) {
    __shared__ uint8_t tab[768];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) tab[i] = table[i];
    __syncthreads();
    const int64_t groups = (n + 3) / 4, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
        const int64_t p = q * 4;
        if (vec && p + 4 <= n) {
            float4 d = *reinterpret_cast<const float4*>(depth + p);
            d.x = frame_nan_to_num(d.x); d.y = frame_nan_to_num(d.y); d.z = frame_nan_to_num(d.z); d.w = frame_nan_to_num(d.w);
            if (clean) *reinterpret_cast<float4*>(clean + p) = d;
            if (!frame) continue;
            const uint32_t c0 = frame_depth_rgb(d.x, lo, den, tab), c1 = frame_depth_rgb(d.y, lo, den, tab);
            const uint32_t c2 = frame_depth_rgb(d.z, lo, den, tab), c3 = frame_depth_rgb(d.w, lo, den, tab);
            uint32_t* o = reinterpret_cast<uint32_t*>(frame + p * 3);      // 12 bytes: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            o[0] = c0 | (c1 << 24);
            o[1] = (c1 >> 8) | (c2 << 16);
            o[2] = (c2 >> 16) | (c3 << 8);
        } else {
            const int64_t end = p + 4 < n ? p + 4 : n;
            for (int64_t i = p; i < end; ++i) {
                const float d = frame_nan_to_num(depth[i]);
                if (clean) clean[i] = d;
                if (!frame) continue;
                const uint32_t c = frame_depth_rgb(d, lo, den, tab);
                frame[3 * i] = (uint8_t)c; frame[3 * i + 1] = (uint8_t)(c >> 8); frame[3 * i + 2] = (uint8_t)(c >> 16);
            }
        }
    }
}

extern "C" int32_t gsr_frame_depth_vis(const float* depth, int32_t B, int32_t H, int32_t W, double lo, double hi,
                                       const uint8_t* table, float* clean, uint8_t* frame, gsr_stream_t stream_) {
    if (B < 0 || H < 0 || W < 0) { gsr_set_error("frame_depth_vis: negative size (%d, %d, %d)", B, H, W); return GSR_E_INVALID; }
    const int64_t n = (int64_t)B * H * W;
    if (n == 0) return GSR_OK;
    if (!depth || !table || (!frame && !clean)) { gsr_set_error("frame_depth_vis: depth, table and one of clean / frame are required"); return GSR_E_INVALID; }
    const int vec = frame_aligned16(depth) && (!clean || frame_aligned16(clean)) && (reinterpret_cast<uintptr_t>(frame) & 3u) == 0;   // a NULL frame is aligned
    hipLaunchKernelGGL(frame_depth_vis_kernel, dim3(frame_blocks((n + 3) / 4)), dim3(FRAME_THREADS), 0,
                       static_cast<hipStream_t>(stream_), depth, n, lo < hi ? lo : hi, fabs(hi - lo), table, clean, frame, vec);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ------------------------------------------------------------------------------- Sobel
// r[0..5] = row[x0 - 1 .. x0 + 4], zero outside the image (row == NULL: a row above or below it)
__device__ __forceinline__ void frame_sobel_row(const float* __restrict__ row, int x0, int W, bool vec, float (&r)[6]) {
    if (!row) {
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = 0.0f;
        return;
    }
    if (vec) {     // W % 4 == 0 and a 16-byte aligned row: the four centre columns exist
        const float4 m = *reinterpret_cast<const float4*>(row + x0);
        r[1] = m.x; r[2] = m.y; r[3] = m.z; r[4] = m.w;
        r[0] = x0 > 0 ? row[x0 - 1] : 0.0f;
        r[5] = x0 + 4 < W ? row[x0 + 4] : 0.0f;
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int x = x0 - 1 + k;
            r[k] = (x >= 0 && x < W) ? row[x] : 0.0f;
        }
    }
}

__global__ void __launch_bounds__(FRAME_THREADS) frame_sobel_kernel(const float* __restrict__ img, int C, int H, int W,
                                                                    float* __restrict__ out, int vec) {
    const int gw = (W + 3) / 4;
    const int64_t plane = (int64_t)H * W, groups = (int64_t)H * gw, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const int y = (int)(g / gw), x0 = (int)(g - (int64_t)y * gw) * 4;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < C; ++c) {
            const float* base = img + c * plane;
            float a[6], m[6], b[6];    // the rows above, of and below the pixel
            frame_sobel_row(y > 0 ? base + (int64_t)(y - 1) * W : nullptr, x0, W, vec, a);
            frame_sobel_row(base + (int64_t)y * W, x0, W, vec, m);
            frame_sobel_row(y + 1 < H ? base + (int64_t)(y + 1) * W : nullptr, x0, W, vec, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // FRAME_SOBEL: the six terms in row-major order of the kernel's non-zero weights, added left to right
                const float gx = ((((-0.25f * a[k] + 0.25f * a[k + 2]) + -0.5f * m[k]) + 0.5f * m[k + 2]) + -0.25f * b[k]) +
                                 0.25f * b[k + 2];
                const float gy = ((((-0.25f * a[k] + -0.5f * a[k + 1]) + -0.25f * a[k + 2]) + 0.25f * b[k]) + 0.5f * b[k + 1]) +
                                 0.25f * b[k + 2];
                const float mag = sqrtf(gx * gx + gy * gy);
                acc[k] = acc[k] + mag * mag;
            }
        }
        float* o = out + (int64_t)y * W + x0;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(sqrtf(acc[0]), sqrtf(acc[1]), sqrtf(acc[2]), sqrtf(acc[3]));
        } else {
            for (int k = 0; k < 4 && x0 + k < W; ++k) o[k] = sqrtf(acc[k]);
        }
    }
}

extern "C" int32_t gsr_frame_sobel(const float* image, int32_t C, int32_t H, int32_t W, float* out, gsr_stream_t stream_) {
    if (C < 1 || H < 0 || W < 0) { gsr_set_error("frame_sobel: bad size (%d, %d, %d)", C, H, W); return GSR_E_INVALID; }
    if (H == 0 || W == 0) return GSR_OK;
    if (!image || !out) { gsr_set_error("frame_sobel: image and out are required"); return GSR_E_INVALID; }
    const int vec = W % 4 == 0 && frame_aligned16(image) && frame_aligned16(out);
    hipLaunchKernelGGL(frame_sobel_kernel, dim3(frame_blocks((int64_t)H * ((W + 3) / 4))), dim3(FRAME_THREADS), 0,
                       static_cast<hipStream_t>(stream_), image, C, H, W, out, vec);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ------------------------------------------------------------------------------- min / max and the colour table
#define FRAME_MINMAX_MAX_BLOCKS 1024    // grid-stride beyond: a lane folds several groups before its wave's two atomics

__global__ void __launch_bounds__(FRAME_THREADS) frame_minmax_kernel(const float* __restrict__ x, int64_t n, int vec,
                                                                     uint32_t* __restrict__ bounds) {
    const int64_t groups = (n + 3) / 4, stride = (int64_t)gridDim.x * blockDim.x;
    float lo = INFINITY, hi = -INFINITY;
    bool any = false;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
        const int64_t p = q * 4;
        if (vec && p + 4 <= n) {
            const float4 v = *reinterpret_cast<const float4*>(x + p);
            lo = fminf(fminf(lo, fminf(v.x, v.y)), fminf(v.z, v.w));
            hi = fmaxf(fmaxf(hi, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        } else {
            const int64_t end = p + 4 < n ? p + 4 : n;
            for (int64_t i = p; i < end; ++i) { lo = fminf(lo, x[i]); hi = fmaxf(hi, x[i]); }
        }
        any = true;
    }
    if (!__ballot(any)) return;
    const float l = wave_min_f32(lo), h = wave_max_f32(hi);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(bounds, frame_f2ord(l));
        atomicMax(bounds + 1, frame_f2ord(h));
    }
}

extern "C" int32_t gsr_frame_minmax(const float* x, int64_t n, uint32_t* bounds, gsr_stream_t stream_) {
    if (n < 1) { gsr_set_error("frame_minmax: n must be >= 1 (got %lld)", (long long)n); return GSR_E_INVALID; }
    if (!x || !bounds) { gsr_set_error("frame_minmax: x and bounds are required"); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GSR_HIP_CHECK(hipMemsetAsync(bounds, 0xff, 4, s));
    GSR_HIP_CHECK(hipMemsetAsync(bounds + 1, 0, 4, s));
    int64_t blocks = ((n + 3) / 4 + FRAME_THREADS - 1) / FRAME_THREADS;
    if (blocks > FRAME_MINMAX_MAX_BLOCKS) blocks = FRAME_MINMAX_MAX_BLOCKS;
    hipLaunchKernelGGL(frame_minmax_kernel, dim3((unsigned)blocks), dim3(FRAME_THREADS), 0, s, x, n, (int)frame_aligned16(x),
                       bounds);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

__global__ void __launch_bounds__(FRAME_THREADS) frame_colormap_kernel(const float* __restrict__ x, int64_t n,
                                                                       const uint32_t* __restrict__ bounds,
                                                                       const float* __restrict__ table, float* __restrict__ out,
                                                                       int vec) {
    __shared__ float tab[768];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) tab[i] = table[i];
    __syncthreads();
    const float mn = frame_ord2f(bounds[0]), mx = frame_ord2f(bounds[1]);
    const float range = mx - mn;
    const bool flat = mx == mn;
    const int64_t groups = (n + 3) / 4, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
        const int64_t p = q * 4;
        const bool full = vec && p + 4 <= n;
        const int cnt = full ? 4 : (int)((p + 4 < n ? p + 4 : n) - p);
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (full) {
            const float4 f = *reinterpret_cast<const float4*>(x + p);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
            for (int k = 0; k < cnt; ++k) v[k] = x[p + k];
        }
        int idx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // FRAME_COLORMAP: subtract, divide, multiply, round half to even: four fp32 operations
            const float r = rintf((v[k] - mn) / range * 255.0f);
            int i = flat ? 0 : (int)r;
            idx[k] = i < 0 ? 0 : (i > 255 ? 255 : i);     // a NaN or an overflow never indexes outside the table
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = out + c * n + p;
            if (full) {
                *reinterpret_cast<float4*>(o) = make_float4(tab[3 * idx[0] + c], tab[3 * idx[1] + c], tab[3 * idx[2] + c],
                                                            tab[3 * idx[3] + c]);
            } else {
                for (int k = 0; k < cnt; ++k) o[k] = tab[3 * idx[k] + c];
            }
        }
    }
}

extern "C" int32_t gsr_frame_colormap(const float* x, int32_t H, int32_t W, const uint32_t* bounds, const float* table,
                                      float* out, gsr_stream_t stream_) {
    if (H < 0 || W < 0) { gsr_set_error("frame_colormap: negative size (%d, %d)", H, W); return GSR_E_INVALID; }
    const int64_t n = (int64_t)H * W;
    if (n == 0) return GSR_OK;
    if (!x || !bounds || !table || !out) { gsr_set_error("frame_colormap: x, bounds, table and out are required"); return GSR_E_INVALID; }
    // the three output planes start at out + c n: all 16-byte aligned only when n % 4 == 0
    const int vec = n % 4 == 0 && frame_aligned16(x) && frame_aligned16(out);
    hipLaunchKernelGGL(frame_colormap_kernel, dim3(frame_blocks((n + 3) / 4)), dim3(FRAME_THREADS), 0,
                       static_cast<hipStream_t>(stream_), x, n, bounds, table, out, vec);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
