// Segment-aware initialisation of the point cloud on the device (include/gsr.h, "segment-aware initialisation"): what the
// reference does in numpy in a subprocess (filter/hull_removal.py, identification/pc_projection.py, identification/main.py)
// and in a Python loop over segments (scene/gaussian_model.py:132-258), restated as the rules SEG_HULL ... SEG_EMIT of the
// header.  This object is compiled with -ffp-contract=off: every fp64 expression below rounds operation by operation, like
// numpy's.  No floating-point atomic anywhere: integer atomics carry counts, areas and the (exact) minimum / maximum.
//
//   seg_hull_kernel        SEG_HULL: one thread per point, facet records (normal, offset, norm) staged through LDS in chunks
//   seg_sum_partial / seg_sum_final kernels   SEG_MEANSTD: two passes, each a fixed-order tree
//   seg_label_kernel       SEG_LABEL: one thread per 16 consecutive pixels of a row, 16-byte loads of the M planes
//   seg_box_kernel         SEG_PROJ_TYT's bounds over the points without a NaN
//   seg_dtu_count_kernel   SEG_PROJ_DTU's in-bounds count per view
//   seg_project_kernel, seg_assign_kernel   SEG_PROJ_*, SEG_ASSIGN: one thread per point
//   seg_stats_kernel       SEG_STATS: one workgroup per label over the label-sorted order
//   seg_emit_kernel        SEG_EMIT: one thread per new point
#include "cloud_common.h"
#include <cmath>

#define SEG_FACET_CHUNK 512          // facet records per LDS chunk (5 doubles each: 20 KB)
#define SEG_MAX_MASKS 32767
#define SEG_MAX_VIEWS 4096
// the reference's hard-coded DTU image size and fallback focal terms (pc_projection.py:48-63)
#define SEG_DTU_W 1554.0
#define SEG_DTU_H 1162.0
#define SEG_DTU_MIN_FRACTION 0.1
#define SEG_EPS 1e-10
#define SEG_TYT_PADDING 0.1

static int seg_check_dtype(int32_t point_f64) {
    if (point_f64 != 0 && point_f64 != 1) { gsr_set_error("point_f64 must be 0 (f32) or 1 (f64), got %d", point_f64); return GSR_E_INVALID; }
    return GSR_OK;
}

// a coordinate of point i, widened on load
__device__ __forceinline__ double seg_ld(const void* __restrict__ pts, int f64, int64_t i, int a) {
    return f64 ? static_cast<const double*>(pts)[3 * i + a] : (double)static_cast<const float*>(pts)[3 * i + a];
}

// ---------------------------------------------------------------- SEG_HULL
__global__ void __launch_bounds__(256) seg_hull_kernel(const void* __restrict__ pts, int f64, int64_t n,
                                                       const double* __restrict__ eq, int n_facets, double* __restrict__ out) {
    __shared__ double s_f[SEG_FACET_CHUNK * 5];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (live) { px = seg_ld(pts, f64, i, 0); py = seg_ld(pts, f64, i, 1); pz = seg_ld(pts, f64, i, 2); }
    double best = INFINITY;
    for (int base = 0; base < n_facets; base += SEG_FACET_CHUNK) {
        const int cnt = min(SEG_FACET_CHUNK, n_facets - base);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt; k += 256) {
            const double* e = eq + 4 * (int64_t)(base + k);
            const double a = e[0], b = e[1], c = e[2];
            s_f[5 * k] = a; s_f[5 * k + 1] = b; s_f[5 * k + 2] = c; s_f[5 * k + 3] = e[3];
            s_f[5 * k + 4] = sqrt((a * a + b * b) + c * c);                 // once per facet
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < cnt; ++k) {                                 // facets in index order
                const double* f = s_f + 5 * k;
                const double d = fabs(((f[0] * px + f[1] * py) + f[2] * pz) + f[3]) / f[4];
                if (d < best || d != d) best = d;                           // a NaN stays, as in np.min
            }
        }
    }
    if (live) out[i] = best;
}

extern "C" int32_t gsr_seg_hull_distance(const void* points, int32_t point_f64, int64_t n, const double* equations,
                                         int32_t n_facets, double* out, gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    rc = seg_check_dtype(point_f64);
    if (rc != GSR_OK) return rc;
    if (n_facets < 1) { gsr_set_error("n_facets must be >= 1 (got %d)", n_facets); return GSR_E_INVALID; }
    if (!equations) { gsr_set_error("equations is null"); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!points || !out) { gsr_set_error("points / out are null with n %lld", (long long)n); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(seg_hull_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, point_f64, n, equations,
                       n_facets, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- SEG_MEANSTD
// The fixed order of gsr_block_sum_256 (cloud_common.h), twice: the mean, then the centred squares.
// centre == NULL: sum of d; else: sum of (d - *centre)^2
__global__ void __launch_bounds__(256) seg_sum_partial_kernel(const double* __restrict__ d, int64_t n, const double* centre,
                                                              double* __restrict__ partial) {
    __shared__ double s_sum[256];
    const double c = centre ? *centre : 0.0;
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = d[i];
        if (centre) { const double e = v - c; sum += e * e; } else sum += v;
    }
    sum = gsr_block_sum_256(sum, s_sum);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// root == 0: *out = sum / n; root == 1: *out = sqrt(sum / n).  n == 0 gives NaN, like numpy.
__global__ void __launch_bounds__(256) seg_sum_final_kernel(const double* __restrict__ partial, int blocks, int64_t n, int root,
                                                            double* __restrict__ out) {
    __shared__ double s_sum[256];
    double sum = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256) sum += partial[b];
    sum = gsr_block_sum_256(sum, s_sum);
    if (threadIdx.x == 0) {
        const double m = sum / (double)n;
        *out = root ? sqrt(m) : m;
    }
}

extern "C" size_t gsr_seg_mean_std_workspace_bytes(int64_t n) { (void)n; return gsr_align(GSR_PARTIAL_BLOCKS * 8); }

extern "C" int32_t gsr_seg_mean_std(const double* d, int64_t n, double* out, void* ws, size_t ws_bytes, gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (!out) { gsr_set_error("out (mean, std) is required"); return GSR_E_INVALID; }
    if (n > 0 && !d) { gsr_set_error("d is null with n %lld", (long long)n); return GSR_E_INVALID; }
    if (!ws || ws_bytes < gsr_seg_mean_std_workspace_bytes(n)) {
        gsr_set_error("ws_bytes: mean / std workspace too small (%zu < %zu bytes)", ws_bytes, gsr_seg_mean_std_workspace_bytes(n));
        return GSR_E_INVALID;
    }
    double* partial = static_cast<double*>(ws);
    const unsigned blocks = gsr_partial_blocks(n);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    for (int pass = 0; pass < 2; ++pass) {
        if (blocks > 0) {
            hipLaunchKernelGGL(seg_sum_partial_kernel, dim3(blocks), dim3(256), 0, s, d, n,
                               pass ? out : static_cast<const double*>(nullptr), partial);
            GSR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(seg_sum_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)blocks, n, pass, out + pass);
        GSR_LAUNCH_CHECK();
    }
    return GSR_OK;
}

// ---------------------------------------------------------------- SEG_LABEL
// bit 7 of every non-zero byte of w
__device__ __forceinline__ uint32_t seg_nonzero_bytes(uint32_t w) { return (w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u; }

__global__ void __launch_bounds__(256) seg_label_kernel(const uint8_t* __restrict__ masks, int n_masks, int H, int W,
                                                        int16_t* __restrict__ label, unsigned long long* __restrict__ area) {
    const int segs = (W + 15) / 16;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < (int64_t)H * segs;
    const int y = live ? (int)(t / segs) : 0;
    const int x0 = live ? (int)(t - (int64_t)y * segs) * 16 : 0;
    const int cnt = live ? min(16, W - x0) : 0;                             // pixels this thread owns
    const int64_t plane = (int64_t)H * W, pix = (int64_t)y * W + x0;
    uint32_t lab[8];                                                        // 16 int16 labels, two per word
#pragma unroll
    for (int k = 0; k < 8; ++k) lab[k] = 0xffffffffu;
    for (int m = 0; m < n_masks; ++m) {
        const uint8_t* src = masks + (int64_t)m * plane + pix;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        // a 16-byte load needs 16 pixels and an address that is a multiple of 16 (row length and base decide that per plane)
        if (cnt == 16 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
            const uint4 q = *reinterpret_cast<const uint4*>(src);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            for (int k = 0; k < cnt; ++k) w[k >> 2] |= (uint32_t)src[k] << (8 * (k & 3));
        }
        uint32_t set_px = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t nz = seg_nonzero_bytes(w[q]);
            set_px += (uint32_t)__popc(nz);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (nz >> (8 * b + 7) & 1u) {
                    const int k = 4 * q + b;
                    const uint32_t sh = 16u * (k & 1);
                    lab[k >> 1] = (lab[k >> 1] & ~(0xffffu << sh)) | ((uint32_t)m << sh);
                }
            }
        }
        // one integer atomic per wave and mask
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) set_px += __shfl_xor(set_px, d, 64);
        if ((threadIdx.x & 63) == 0 && set_px) atomicAdd(&area[m], (unsigned long long)set_px);
    }
    if (!live) return;
    int16_t* dst = label + pix;
    if (cnt == 16 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        reinterpret_cast<uint4*>(dst)[0] = make_uint4(lab[0], lab[1], lab[2], lab[3]);
        reinterpret_cast<uint4*>(dst)[1] = make_uint4(lab[4], lab[5], lab[6], lab[7]);
    } else {
        for (int k = 0; k < cnt; ++k) dst[k] = (int16_t)(lab[k >> 1] >> (16 * (k & 1)) & 0xffffu);
    }
}

extern "C" int32_t gsr_seg_label_map(const uint8_t* masks, int32_t n_masks, int32_t H, int32_t W, int16_t* label,
                                     int64_t* area, gsr_stream_t stream_) {
    if (n_masks < 0 || H < 0 || W < 0) { gsr_set_error("n_masks, H, W must be >= 0 (got %d, %d, %d)", n_masks, H, W); return GSR_E_INVALID; }
    if (n_masks > SEG_MAX_MASKS) {
        gsr_set_error("n_masks %d exceeds %d (labels are int16)", n_masks, SEG_MAX_MASKS);
        return GSR_E_UNSUPPORTED;
    }
    if ((int64_t)H * W > 0x7fffffffLL) { gsr_set_error("H * W %lld exceeds int32 indices", (long long)H * W); return GSR_E_UNSUPPORTED; }
    if (n_masks > 0 && !area) { gsr_set_error("area is null with n_masks %d", n_masks); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (n_masks > 0) GSR_HIP_CHECK(hipMemsetAsync(area, 0, size_t(n_masks) * 8, s));
    if ((int64_t)H * W == 0) return GSR_OK;
    if (!label) { gsr_set_error("label is null with H * W %lld", (long long)H * W); return GSR_E_INVALID; }
    if (n_masks > 0 && !masks) { gsr_set_error("masks is null with n_masks %d", n_masks); return GSR_E_INVALID; }
    const int64_t threads = (int64_t)H * ((W + 15) / 16);
    hipLaunchKernelGGL(seg_label_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, masks, n_masks, H, W, label,
                       reinterpret_cast<unsigned long long*>(area));
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- SEG_PROJ_*
// workspace of the view calls: [box: lo.xyz hi.xyz as ordered words, count of points without a NaN, pad][in-bounds count per
// view][the views]
struct SegViewWs {
    unsigned long long* box;     // [8]
    unsigned long long* counts;  // [n_views]
    GsrSegView* views;           // [n_views]
    size_t bytes;
};

static SegViewWs seg_view_layout(void* base, int32_t n_views) {
    SegViewWs w{};
    GsrWsCursor c(base);
    const size_t v = size_t(n_views > 0 ? n_views : 1);
    w.box = c.take<unsigned long long>(64);
    w.counts = c.take<unsigned long long>(v * 8);
    w.views = c.take<GsrSegView>(v * sizeof(GsrSegView));
    w.bytes = c.off;
    return w;
}

__global__ void __launch_bounds__(256) seg_box_kernel(const void* __restrict__ pts, int f64, int64_t n,
                                                      unsigned long long* __restrict__ box) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned long long valid = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = seg_ld(pts, f64, i, 0), y = seg_ld(pts, f64, i, 1), z = seg_ld(pts, f64, i, 2);
        if (x != x || y != y || z != z) continue;
        ++valid;
        lo[0] = fmin(lo[0], x); hi[0] = fmax(hi[0], x);
        lo[1] = fmin(lo[1], y); hi[1] = fmax(hi[1], y);
        lo[2] = fmin(lo[2], z); hi[2] = fmax(hi[2], z);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        valid += __shfl_xor(valid, d, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], __shfl_xor(lo[a], d, 64));
            hi[a] = fmax(hi[a], __shfl_xor(hi[a], d, 64));
        }
    }
    if ((threadIdx.x & 63) == 0 && valid) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&box[a], gsr_d2ord(lo[a]));
            atomicMax(&box[3 + a], gsr_d2ord(hi[a]));
        }
        atomicAdd(&box[6], valid);
    }
}

struct SegProj { double u, v, z; };

// SEG_PROJ_DTU without the fallback decision: the pinhole projection through scale_mat and world_mat
__device__ __forceinline__ SegProj seg_project_dtu_main(const GsrSegView& V, double px, double py, double pz) {
    double sc[4], c[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double* S = V.scale_mat + 4 * r;
        sc[r] = ((S[0] * px + S[1] * py) + S[2] * pz) + S[3];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double* M = V.world_mat + 4 * r;
        c[r] = ((M[0] * sc[0] + M[1] * sc[1]) + M[2] * sc[2]) + M[3] * sc[3];
    }
    const double x = c[0] / c[3], y = c[1] / c[3];
    return SegProj{V.camera_mat[0] * x + V.camera_mat[2], V.camera_mat[4] * y + V.camera_mat[5], c[2]};
}

__device__ __forceinline__ bool seg_in_bounds(double u, double v, double w, double h) {
    return u >= 0.0 && u < w && v >= 0.0 && v < h;                          // false for NaN
}

__device__ __forceinline__ double seg_nan_to_num(double v) {
    if (v != v) return 0.0;
    return fmin(fmax(v, -DBL_MAX), DBL_MAX);
}

__device__ __forceinline__ SegProj seg_project(const GsrSegView& V, double px, double py, double pz, int64_t n,
                                               unsigned long long dtu_count, const unsigned long long* __restrict__ box) {
    if (V.kind == GSR_SEG_DTU) {
        SegProj p = seg_project_dtu_main(V, px, py, pz);
        if ((double)dtu_count < SEG_DTU_MIN_FRACTION * (double)n) {         // the view's fallback: normalised rays
            const double vx = px - V.cam_pos[0], vy = py - V.cam_pos[1], vz = pz - V.cam_pos[2];
            const double len = sqrt((vx * vx + vy * vy) + vz * vz);
            const double nx = vx / len, ny = vy / len, nz = vz / len;
            p.u = (nx / (nz + SEG_EPS)) * (SEG_DTU_W / 3.0) + SEG_DTU_W / 2.0;
            p.v = (ny / (nz + SEG_EPS)) * (SEG_DTU_H / 3.0) + SEG_DTU_H / 2.0;
        }
        return p;
    }
    if (V.kind == GSR_SEG_NERF) {
        double pc[3], q[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double* M = V.world_mat + 4 * r;
            pc[r] = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double* K = V.camera_mat + 3 * r;
            q[r] = (K[0] * pc[0] + K[1] * pc[1]) + K[2] * pc[2];
        }
        return SegProj{q[0] / q[2], q[1] / q[2], pc[2]};
    }
    // GSR_SEG_TYT
    if (box[6] == 0) return SegProj{0.0, 0.0, 0.0};
    const double lox = gsr_ord2d(box[0]), loy = gsr_ord2d(box[1]), hix = gsr_ord2d(box[3]), hiy = gsr_ord2d(box[4]);
    const double span = 1.0 - 2.0 * SEG_TYT_PADDING;
    const double nx = SEG_TYT_PADDING + span * (px - lox) / ((hix - lox) + SEG_EPS);
    const double ny = SEG_TYT_PADDING + span * (py - loy) / ((hiy - loy) + SEG_EPS);
    const double vx = px - V.cam_pos[0], vy = py - V.cam_pos[1], vz = pz - V.cam_pos[2];
    return SegProj{seg_nan_to_num(nx * V.img_w), seg_nan_to_num(ny * V.img_h),
                   (vx * V.world_mat[8] + vy * V.world_mat[9]) + vz * V.world_mat[10]};
}

// blockIdx.y: the view; views that are not DTU leave at once
__global__ void __launch_bounds__(256) seg_dtu_count_kernel(const void* __restrict__ pts, int f64, int64_t n,
                                                            const GsrSegView* __restrict__ views,
                                                            unsigned long long* __restrict__ counts) {
    const GsrSegView& V = views[blockIdx.y];
    if (V.kind != GSR_SEG_DTU) return;
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const SegProj p = seg_project_dtu_main(V, seg_ld(pts, f64, i, 0), seg_ld(pts, f64, i, 1), seg_ld(pts, f64, i, 2));
        c += seg_in_bounds(p.u, p.v, SEG_DTU_W, SEG_DTU_H) ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[blockIdx.y], c);
}

__global__ void __launch_bounds__(256) seg_project_kernel(const void* __restrict__ pts, int f64, int64_t n,
                                                          const GsrSegView* __restrict__ views, int view,
                                                          const unsigned long long* __restrict__ counts,
                                                          const unsigned long long* __restrict__ box, double* __restrict__ uv,
                                                          double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const SegProj p = seg_project(views[view], seg_ld(pts, f64, i, 0), seg_ld(pts, f64, i, 1), seg_ld(pts, f64, i, 2), n,
                                  counts[view], box);
    uv[2 * i] = p.u; uv[2 * i + 1] = p.v; z[i] = p.z;
}

__global__ void __launch_bounds__(256) seg_assign_kernel(const void* __restrict__ pts, int f64, int64_t n,
                                                         const GsrSegView* __restrict__ views, int n_views,
                                                         const unsigned long long* __restrict__ counts,
                                                         const unsigned long long* __restrict__ box,
                                                         const int16_t* __restrict__ label_maps, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = seg_ld(pts, f64, i, 0), py = seg_ld(pts, f64, i, 1), pz = seg_ld(pts, f64, i, 2);
    int32_t lab = -1;
    for (int v = 0; v < n_views && lab < 0; ++v) {
        const GsrSegView& V = views[v];
        if (V.n_masks <= 0 || V.width <= 0 || V.height <= 0) continue;     // (a)
        const SegProj p = seg_project(V, px, py, pz, n, counts[v], box);
        const double w = (double)V.width, h = (double)V.height;
        if (!seg_in_bounds(p.u, p.v, w, h) || !(p.z > 0.0)) continue;       // (b), (c)
        const int x = (int)rint(fmin(fmax(p.u, 0.0), w - 1.0)), y = (int)rint(fmin(fmax(p.v, 0.0), h - 1.0));
        lab = (int32_t)label_maps[V.label_offset + (int64_t)y * V.width + x];    // (d)
    }
    out[i] = lab;
}

extern "C" size_t gsr_seg_views_workspace_bytes(int32_t n_views) { return seg_view_layout(nullptr, n_views).bytes; }

extern "C" int32_t gsr_seg_views_prepare(const void* points, int32_t point_f64, int64_t n, const GsrSegView* views_host,
                                         int32_t n_views, int64_t label_elems, void* ws, size_t ws_bytes, gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    rc = seg_check_dtype(point_f64);
    if (rc != GSR_OK) return rc;
    if (n_views < 0 || n_views > SEG_MAX_VIEWS) {
        gsr_set_error("n_views must be in [0, %d] (got %d)", SEG_MAX_VIEWS, n_views);
        return n_views < 0 ? GSR_E_INVALID : GSR_E_UNSUPPORTED;
    }
    if (label_elems < 0) { gsr_set_error("label_elems must be >= 0 (got %lld)", (long long)label_elems); return GSR_E_INVALID; }
    if (n_views > 0 && !views_host) { gsr_set_error("views_host is null with n_views %d", n_views); return GSR_E_INVALID; }
    if (n > 0 && !points) { gsr_set_error("points is null with n %lld", (long long)n); return GSR_E_INVALID; }
    bool any_dtu = false, any_tyt = false;
    for (int v = 0; v < n_views; ++v) {
        const GsrSegView& V = views_host[v];
        if (V.kind != GSR_SEG_DTU && V.kind != GSR_SEG_NERF && V.kind != GSR_SEG_TYT) {
            gsr_set_error("views_host[%d].kind must be GSR_SEG_DTU, _NERF or _TYT (got %d)", v, V.kind);
            return GSR_E_INVALID;
        }
        if (V.width < 0 || V.height < 0 || V.n_masks < 0 || V.n_masks > SEG_MAX_MASKS) {
            gsr_set_error("views_host[%d]: width, height >= 0 and 0 <= n_masks <= %d (got %d, %d, %d)", v, SEG_MAX_MASKS, V.width,
                          V.height, V.n_masks);
            return GSR_E_INVALID;
        }
        // a view with masks reads its whole label map: it must lie inside label_maps
        if (V.n_masks > 0 && (V.label_offset < 0 || V.label_offset > label_elems ||
                              (int64_t)V.width * V.height > label_elems - V.label_offset)) {
            gsr_set_error("views_host[%d]: label_offset %lld + %d x %d lies outside label_maps (%lld elements)", v,
                          (long long)V.label_offset, V.width, V.height, (long long)label_elems);
            return GSR_E_INVALID;
        }
        any_dtu = any_dtu || V.kind == GSR_SEG_DTU;
        any_tyt = any_tyt || V.kind == GSR_SEG_TYT;
    }
    const SegViewWs w = seg_view_layout(ws, n_views);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: view workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GSR_HIP_CHECK(hipMemsetAsync(w.box, 0xFF, 24, s));
    GSR_HIP_CHECK(hipMemsetAsync(w.box + 3, 0x00, 40, s));
    if (n_views == 0) return GSR_OK;
    GSR_HIP_CHECK(hipMemsetAsync(w.counts, 0, size_t(n_views) * 8, s));
    // (pageable source: the copy has left views_host when the call returns)
    GSR_HIP_CHECK(hipMemcpyAsync(w.views, views_host, size_t(n_views) * sizeof(GsrSegView), hipMemcpyHostToDevice, s));
    if (n == 0) return GSR_OK;
    const unsigned blocks = gsr_partial_blocks(n);
    if (any_tyt) {
        hipLaunchKernelGGL(seg_box_kernel, dim3(blocks), dim3(256), 0, s, points, point_f64, n, w.box);
        GSR_LAUNCH_CHECK();
    }
    if (any_dtu) {
        hipLaunchKernelGGL(seg_dtu_count_kernel, dim3(blocks, (unsigned)n_views), dim3(256), 0, s, points, point_f64, n,
                           w.views, w.counts);
        GSR_LAUNCH_CHECK();
    }
    return GSR_OK;
}

static int seg_check_view_call(const void* points, int32_t point_f64, int64_t n, int32_t n_views, void* ws, size_t ws_bytes,
                               SegViewWs& w) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    rc = seg_check_dtype(point_f64);
    if (rc != GSR_OK) return rc;
    if (n_views < 0 || n_views > SEG_MAX_VIEWS) { gsr_set_error("n_views must be in [0, %d] (got %d)", SEG_MAX_VIEWS, n_views); return GSR_E_INVALID; }
    if (n > 0 && !points) { gsr_set_error("points is null with n %lld", (long long)n); return GSR_E_INVALID; }
    w = seg_view_layout(ws, n_views);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: view workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

extern "C" int32_t gsr_seg_project(const void* points, int32_t point_f64, int64_t n, void* ws, size_t ws_bytes, int32_t n_views,
                                   int32_t view, double* uv_out, double* z_out, gsr_stream_t stream_) {
    SegViewWs w;
    int rc = seg_check_view_call(points, point_f64, n, n_views, ws, ws_bytes, w);
    if (rc != GSR_OK) return rc;
    if (view < 0 || view >= n_views) { gsr_set_error("view %d is outside [0, %d)", view, n_views); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!uv_out || !z_out) { gsr_set_error("uv_out / z_out are null with n %lld", (long long)n); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(seg_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, point_f64, n, w.views, view,
                       w.counts, w.box, uv_out, z_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_seg_assign(const void* points, int32_t point_f64, int64_t n, void* ws, size_t ws_bytes, int32_t n_views,
                                  const int16_t* label_maps, int32_t* out, gsr_stream_t stream_) {
    SegViewWs w;
    int rc = seg_check_view_call(points, point_f64, n, n_views, ws, ws_bytes, w);
    if (rc != GSR_OK) return rc;
    if (n == 0) return GSR_OK;
    if (!out) { gsr_set_error("out is null with n %lld", (long long)n); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(seg_assign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, point_f64, n, w.views,
                       n_views, w.counts, w.box, label_maps, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- SEG_STATS
// One workgroup per label.  order: the point indices sorted by label (stable); seg_off[l] .. seg_off[l + 1]: label l's run.
// Thread t adds the run's elements t, t + 256, ... in that order, the 256 sums go through gsr_block_sum_256's tree: mean first,
// then the centred moments.  out row: mean.xyz, cov (row-major 3x3), std.xyz, mean colour.rgb
__global__ void __launch_bounds__(256) seg_stats_kernel(const float* __restrict__ pts, const float* __restrict__ col,
                                                        const int64_t* __restrict__ order, const int64_t* __restrict__ seg_off,
                                                        int64_t n, int64_t* __restrict__ count_out, double* __restrict__ out) {
    __shared__ double s_sum[256];
    const int l = blockIdx.x;
    int64_t b = seg_off[l], e = seg_off[l + 1];
    b = b < 0 ? 0 : (b > n ? n : b);
    e = e < b ? b : (e > n ? n : e);
    const double cnt = (double)(e - b);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t k = b + threadIdx.x; k < e; k += 256) {
        const int64_t i = order[k];
        if ((uint64_t)i >= (uint64_t)n) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) { acc[a] += (double)pts[3 * i + a]; acc[3 + a] += (double)col[3 * i + a]; }
    }
    double mean[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) { mean[a] = gsr_block_sum_256(acc[a], s_sum) / cnt; __syncthreads(); }     // s_sum is written again
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                           // xx xy xz yy yz zz
    for (int64_t k = b + threadIdx.x; k < e; k += 256) {
        const int64_t i = order[k];
        if ((uint64_t)i >= (uint64_t)n) continue;
        const double dx = (double)pts[3 * i] - mean[0], dy = (double)pts[3 * i + 1] - mean[1], dz = (double)pts[3 * i + 2] - mean[2];
        m[0] += dx * dx; m[1] += dx * dy; m[2] += dx * dz; m[3] += dy * dy; m[4] += dy * dz; m[5] += dz * dz;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        m[a] = gsr_block_sum_256(m[a], s_sum) / (cnt > 1.0 ? cnt - 1.0 : 0.0);      // fewer than two points: NaN
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        count_out[l] = e - b;
        double* o = out + 18 * (int64_t)l;
        o[0] = mean[0]; o[1] = mean[1]; o[2] = mean[2];
        o[3] = m[0]; o[4] = m[1]; o[5] = m[2];
        o[6] = m[1]; o[7] = m[3]; o[8] = m[4];
        o[9] = m[2]; o[10] = m[4]; o[11] = m[5];
        o[12] = sqrt(m[0]); o[13] = sqrt(m[3]); o[14] = sqrt(m[5]);
        o[15] = mean[3]; o[16] = mean[4]; o[17] = mean[5];
    }
}

extern "C" int32_t gsr_seg_stats(const float* points, const float* colors, const int64_t* order, const int64_t* seg_off, int64_t n,
                                 int32_t n_labels, int64_t* count_out, double* stats_out, gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (n_labels < 0) { gsr_set_error("n_labels must be >= 0 (got %d)", n_labels); return GSR_E_INVALID; }
    if (n_labels == 0) return GSR_OK;
    if (!seg_off || !count_out || !stats_out) { gsr_set_error("seg_off / count_out / stats_out are null with n_labels %d", n_labels); return GSR_E_INVALID; }
    if (n > 0 && (!points || !colors || !order)) { gsr_set_error("points / colors / order are null with n %lld", (long long)n); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(seg_stats_kernel, dim3((unsigned)n_labels), dim3(256), 0, s, points, colors, order, seg_off, n, count_out,
                       stats_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- SEG_EMIT
__global__ void __launch_bounds__(256) seg_emit_kernel(const float* __restrict__ eps, const int64_t* __restrict__ offsets, int n_segs,
                                                       const float* __restrict__ mean, const float* __restrict__ tril,
                                                       const float* __restrict__ mean_color, const int64_t* __restrict__ labels,
                                                       int64_t total, float* __restrict__ out_xyz, float* __restrict__ out_color,
                                                       int64_t* __restrict__ out_label) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    // the segment s with offsets[s] <= i < offsets[s + 1] (empty segments are passed over)
    int lo = 0, hi = n_segs;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const int sgm = lo;
    const double e0 = (double)eps[3 * i], e1 = (double)eps[3 * i + 1], e2 = (double)eps[3 * i + 2];
    const float* L = tril + 9 * (int64_t)sgm;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double le = ((double)L[3 * r] * e0 + (double)L[3 * r + 1] * e1) + (double)L[3 * r + 2] * e2;
        out_xyz[3 * i + r] = (float)((double)mean[3 * (int64_t)sgm + r] + le);
        out_color[3 * i + r] = mean_color[3 * (int64_t)sgm + r];
    }
    out_label[i] = labels[sgm];
}

extern "C" int32_t gsr_seg_augment_emit(const float* eps, const int64_t* offsets, int32_t n_segs, const float* mean,
                                        const float* tril, const float* mean_color, const int64_t* labels, int64_t total,
                                        float* out_xyz, float* out_color, int64_t* out_label, gsr_stream_t stream_) {
    int rc = gsr_check_count("total", total);
    if (rc != GSR_OK) return rc;
    if (n_segs < 0) { gsr_set_error("n_segs must be >= 0 (got %d)", n_segs); return GSR_E_INVALID; }
    if (total == 0) return GSR_OK;
    if (n_segs == 0) { gsr_set_error("total %lld new points need at least one segment", (long long)total); return GSR_E_INVALID; }
    if (!eps || !offsets || !mean || !tril || !mean_color || !labels || !out_xyz || !out_color || !out_label) {
        gsr_set_error("an array is null with total %lld", (long long)total);
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(seg_emit_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, eps, offsets, n_segs, mean, tril,
                       mean_color, labels, total, out_xyz, out_color, out_label);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
