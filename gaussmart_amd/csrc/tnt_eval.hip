// Tanks-and-Temples mesh evaluation on the device (include/gsr.h, "mesh evaluation: Tanks-and-Temples F-score"): what the
// reference's scripts/eval_tnt/run.py does with Open3D and trimesh, restated as the rules TNT_CLOUD ... TNT_SCORE of the
// header.  The nearest-neighbour searches are mesh_eval.hip's gsr_points_nearest; this object holds what sits around them.
// Compiled with -ffp-contract=off: every fp64 expression below rounds operation by operation, like numpy's.
//
//   te_centres_kernel      TNT_CLOUD: one thread per face
//   te_transform_kernel    TNT_TRANSFORM: one thread per point, the matrix by value
//   te_crop_kernel         TNT_CROP: the polygon's (u, v) in LDS, one thread per point walks the m edges
//   cloud_bounds<false> (cloud_common.h), te_cell_kernel, te_head_kernel, te_voxel_emit_kernel   TNT_VOXEL: minimum, 63-bit cell keys as two words,
//                          (stable two-word sort by gsr_radix_sort_pairs), run heads, (scan), one thread per cell adds its run
//   te_sums_kernel, te_sums_final_kernel   TNT_ICP_SUMS in EVAL_MEAN's fixed order
//   te_score_kernel        TNT_SCORE: edges and int32 bins in LDS, integer atomics only
// No floating-point atomic anywhere: every result has the same bits on every run.
#include "cloud_common.h"
#include <cmath>

#define TE_MAX_POLY 256
#define TE_MAX_BINS 4096
#define TE_CELL_LIMIT 2097152.0      // 2^21 cells per axis: three indices share a 63-bit key
#define TE_SUM_VALUES 10

// ---------------------------------------------------------------- TNT_CLOUD
// An index outside [0, V) gives a NaN row, never a wild read; the caller checks the range and raises.
__global__ void __launch_bounds__(256) te_centres_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                         int64_t F, int64_t V, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    const bool in = (uint64_t)i0 < (uint64_t)V && (uint64_t)i1 < (uint64_t)V && (uint64_t)i2 < (uint64_t)V;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float r = __uint_as_float(0x7fc00000u);
        if (in) {
            const double p0 = (double)verts[3 * (int64_t)i0 + a], p1 = (double)verts[3 * (int64_t)i1 + a],
                         p2 = (double)verts[3 * (int64_t)i2 + a];
            r = (float)(((p0 + p1) + p2) / 3.0);
        }
        out[3 * t + a] = r;
    }
}

extern "C" int32_t gsr_mesh_face_centres(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts,
                                         float* centres_out, gsr_stream_t stream_) {
    int rc = gsr_check_count("n_tris", n_tris);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_count("n_verts", n_verts);
    if (rc != GSR_OK) return rc;
    if (n_tris + n_verts > 0x7fffffffLL) {
        gsr_set_error("n_verts %lld + n_tris %lld exceed int32 indices", (long long)n_verts, (long long)n_tris);
        return GSR_E_UNSUPPORTED;
    }
    if (n_tris == 0) return GSR_OK;
    if (!tris || !centres_out) { gsr_set_error("tris / centres_out are null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    if (n_verts > 0 && !verts) { gsr_set_error("verts is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(te_centres_kernel, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, s, verts, tris, n_tris, n_verts,
                       centres_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- TNT_TRANSFORM
struct TeMat { double m[12]; };

__global__ void __launch_bounds__(256) te_transform_kernel(const float* __restrict__ points, int64_t n, TeMat T,
                                                           float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)points[3 * i], y = (double)points[3 * i + 1], z = (double)points[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        out[3 * i + r] = (float)(((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3]);   // TNT_POINT_F32
}

extern "C" int32_t gsr_points_transform(const float* points, int64_t n, const double* transform_host, float* out,
                                        gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (!transform_host) { gsr_set_error("transform_host (4x4, row-major) is required"); return GSR_E_INVALID; }
    if (!(transform_host[12] == 0.0 && transform_host[13] == 0.0 && transform_host[14] == 0.0 && transform_host[15] == 1.0)) {
        gsr_set_error("transform_host: the last row must be (0, 0, 0, 1) (got %g %g %g %g)", transform_host[12], transform_host[13],
                      transform_host[14], transform_host[15]);
        return GSR_E_INVALID;
    }
    if (n == 0) return GSR_OK;
    if (!points || !out) { gsr_set_error("points / out are null with n %lld", (long long)n); return GSR_E_INVALID; }
    TeMat T;
    for (int k = 0; k < 12; ++k) T.m[k] = transform_host[k];
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(te_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, T, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- TNT_CROP
__global__ void __launch_bounds__(256) te_crop_kernel(const float* __restrict__ points, int64_t n, const double* __restrict__ poly,
                                                      int m, int a, int ua, int va, double lo, double hi,
                                                      uint8_t* __restrict__ keep) {
    __shared__ double s_u[TE_MAX_POLY], s_v[TE_MAX_POLY];
    for (int k = threadIdx.x; k < m; k += 256) { s_u[k] = poly[3 * k + ua]; s_v[k] = poly[3 * k + va]; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double pa = (double)points[3 * i + a], pu = (double)points[3 * i + ua], pv = (double)points[3 * i + va];
    bool in = pa >= lo && pa <= hi;
    if (in) {
        int nodes = 0;
        double iu = s_u[m - 1], iv = s_v[m - 1];            // edge (m - 1, 0) first: the count does not depend on the order
        for (int k = 0; k < m; ++k) {
            const double ju = s_u[k], jv = s_v[k];
            if ((iv < pv && jv >= pv) || (jv < pv && iv >= pv)) {
                const double node = iu + (pv - iv) / (jv - iv) * (ju - iu);
                nodes += node < pu;
            }
            iu = ju; iv = jv;
        }
        in = (nodes & 1) != 0;
    }
    keep[i] = in;
}

extern "C" int32_t gsr_points_crop_polygon(const float* points, int64_t n, int32_t orthogonal_axis, double axis_min, double axis_max,
                                           const double* polygon, int32_t n_polygon, uint8_t* keep_out, gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (orthogonal_axis < 0 || orthogonal_axis > 2) {
        gsr_set_error("orthogonal_axis must be 0 (X), 1 (Y) or 2 (Z) (got %d)", orthogonal_axis);
        return GSR_E_INVALID;
    }
    if (axis_min != axis_min || axis_max != axis_max) { gsr_set_error("axis_min / axis_max must not be NaN"); return GSR_E_INVALID; }
    if (n_polygon < 1) { gsr_set_error("n_polygon must be >= 1 (got %d)", n_polygon); return GSR_E_INVALID; }
    if (n_polygon > TE_MAX_POLY) {
        gsr_set_error("n_polygon %d exceeds the %d vertices a crop polygon may have", n_polygon, TE_MAX_POLY);
        return GSR_E_UNSUPPORTED;
    }
    if (!polygon) { gsr_set_error("polygon is null with n_polygon %d", n_polygon); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!points || !keep_out) { gsr_set_error("points / keep_out are null with n %lld", (long long)n); return GSR_E_INVALID; }
    const int a = orthogonal_axis, ua = a == 0 ? 1 : 0, va = a == 2 ? 1 : 2;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(te_crop_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, polygon, n_polygon, a, ua, va,
                       fmin(axis_min, axis_max), fmax(axis_min, axis_max), keep_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- TNT_VOXEL
// info[0..2]: the per-axis minimum as ordered words, by cloud_bounds<false> (integer atomicMin: the same word whatever the
// order of arrival)
// key = ix << 42 | iy << 21 | iz as two words; info[1] != 0: some index is not in [0, 2^21) (NaN and inf included)
__global__ void __launch_bounds__(256) te_cell_kernel(const float* __restrict__ xyz, int64_t n, const uint32_t* __restrict__ mm,
                                                      double voxel, uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi,
                                                      uint32_t* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long key = 0;
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)gsr_ord2f(mm[a]) - 0.5 * voxel;
        const double c = floor(((double)xyz[3 * i + a] - lo) / voxel);
        const bool ok = c >= 0.0 && c < TE_CELL_LIMIT;
        bad = bad || !ok;
        key = (key << 21) | (ok ? (unsigned long long)c : 0ull);
    }
    key_lo[i] = (uint32_t)key;
    key_hi[i] = (uint32_t)(key >> 32);
    if (bad) atomicOr(&info[1], 1u);
}

// head[k]: sorted position k starts a cell
__global__ void __launch_bounds__(256) te_head_kernel(const uint32_t* __restrict__ order, int64_t n, const uint32_t* __restrict__ key_lo,
                                                      const uint32_t* __restrict__ key_hi, uint8_t* __restrict__ head) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    bool h = true;
    if (k > 0) {
        const uint32_t a = order[k], b = order[k - 1];
        h = key_lo[a] != key_lo[b] || key_hi[a] != key_hi[b];
    }
    head[k] = h;
}

// off: exclusive scan of head.  The thread at a cell's head walks the cell's run: ascending input index (the sort is stable),
// added sequentially -- that order is the rule.
__global__ void __launch_bounds__(256) te_voxel_emit_kernel(const float* __restrict__ xyz, int64_t n, const uint32_t* __restrict__ order,
                                                            const uint8_t* __restrict__ head, const uint32_t* __restrict__ off,
                                                            float* __restrict__ out, int32_t* __restrict__ cell_of) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const bool h = head[k] != 0;
    const int64_t cell = (int64_t)off[k] + (h ? 1 : 0) - 1;
    if (cell_of) cell_of[order[k]] = (int32_t)cell;
    if (!h) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, cnt = 0.0;
    int64_t j = k;
    do {
        const int64_t src = order[j];
        sx += (double)xyz[3 * src]; sy += (double)xyz[3 * src + 1]; sz += (double)xyz[3 * src + 2];
        cnt += 1.0;
        ++j;
    } while (j < n && !head[j]);
    out[3 * cell] = (float)(sx / cnt); out[3 * cell + 1] = (float)(sy / cnt); out[3 * cell + 2] = (float)(sz / cnt);
}

struct TeVoxelWs {
    uint32_t *info;                                     // [0..2] minimum words, [3] unused; info + 4: [0] cells, [1] refused
    uint32_t *key_lo, *key_hi, *k1, *o1, *h1, *kt, *vt, *v2t, *k2, *order;      // [n] each
    uint8_t* head;                                      // [n]
    uint32_t* off;                                      // [n + 1]
    void *scan_ws, *sort_ws;
    size_t bytes;
};

static TeVoxelWs te_voxel_layout(void* base, int64_t n_) {
    TeVoxelWs w{};
    GsrWsCursor c(base);
    const size_t n = size_t(n_ > 0 ? n_ : 1);
    auto words = [&]() { return c.take<uint32_t>(n * 4); };
    w.info = c.take<uint32_t>(32);
    w.key_lo = words(); w.key_hi = words(); w.k1 = words(); w.o1 = words(); w.h1 = words(); w.kt = words(); w.vt = words();
    w.v2t = words(); w.k2 = words(); w.order = words();
    w.head = c.take<uint8_t>(n);
    w.off = c.take<uint32_t>((n + 1) * 4);
    w.scan_ws = c.take(gsr_scan_workspace_bytes((int64_t)n));
    w.sort_ws = c.take(gsr_sort_ws_bytes((int64_t)n));
    w.bytes = c.off;
    return w;
}

static int te_check_voxel(const float* points, int64_t n, double voxel_size, void* ws, size_t ws_bytes, TeVoxelWs& w) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_positive("voxel_size", voxel_size);
    if (rc != GSR_OK) return rc;
    if (n > 0 && !points) { gsr_set_error("points is null with n %lld", (long long)n); return GSR_E_INVALID; }
    w = te_voxel_layout(ws, n);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: voxel down-sampling workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

extern "C" size_t gsr_points_voxel_workspace_bytes(int64_t n) { return te_voxel_layout(nullptr, n).bytes; }

extern "C" int32_t gsr_points_voxel_count(const float* points, int64_t n, double voxel_size, void* ws, size_t ws_bytes,
                                          int64_t* n_cells_out, gsr_stream_t stream_) {
    if (!n_cells_out) { gsr_set_error("n_cells_out is required"); return GSR_E_INVALID; }
    *n_cells_out = 0;
    TeVoxelWs w;
    int rc = te_check_voxel(points, n, voxel_size, ws, ws_bytes, w);
    if (rc != GSR_OK) return rc;
    if (n == 0) return GSR_OK;
    unsigned long long* host = gsr_pinned_words(1);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const dim3 grid((unsigned)((n + 255) / 256));
    rc = cloud_bounds<false>(points, n, w.info, s);
    if (rc != GSR_OK) return rc;
    GSR_HIP_CHECK(hipMemsetAsync(w.info + 4, 0, 16, s));
    hipLaunchKernelGGL(te_cell_kernel, grid, dim3(256), 0, s, points, n, w.info, voxel_size, w.key_lo, w.key_hi, w.info + 4);
    GSR_LAUNCH_CHECK();
    // stable sort on the 63-bit key, low word first; the high word rides along as the second value of the first sort
    rc = gsr_radix_sort_pairs(w.key_lo, nullptr, w.k1, w.o1, w.kt, w.vt, n, 0, 32, w.sort_ws, s, w.key_hi, w.h1, w.v2t);
    if (rc != GSR_OK) return rc;
    rc = gsr_radix_sort_pairs(w.h1, w.o1, w.k2, w.order, w.kt, w.vt, n, 0, 31, w.sort_ws, s);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(te_head_kernel, grid, dim3(256), 0, s, w.order, n, w.key_lo, w.key_hi, w.head);
    GSR_LAUNCH_CHECK();
    rc = gsr_exclusive_scan_u8(w.head, w.off, n, w.scan_ws, s);
    if (rc != GSR_OK) return rc;
    // the one read-back: the number of cells and whether an index was refused
    GSR_HIP_CHECK(hipMemcpyAsync(w.info + 4, w.off + n, 4, hipMemcpyDeviceToDevice, s));
    uint32_t* h = reinterpret_cast<uint32_t*>(host);
    GSR_HIP_CHECK(hipMemcpyAsync(h, w.info + 4, 8, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    if (h[1]) {
        gsr_set_error("voxel_size %g gives 2^21 or more cells on an axis (or a coordinate is not finite): raise voxel_size", voxel_size);
        return GSR_E_UNSUPPORTED;
    }
    *n_cells_out = (int64_t)h[0];
    return GSR_OK;
}

extern "C" int32_t gsr_points_voxel_emit(const float* points, int64_t n, double voxel_size, void* ws, size_t ws_bytes,
                                         float* points_out, int32_t* cell_of_point_out, gsr_stream_t stream_) {
    TeVoxelWs w;
    int rc = te_check_voxel(points, n, voxel_size, ws, ws_bytes, w);
    if (rc != GSR_OK) return rc;
    if (n == 0) return GSR_OK;
    if (!points_out) { gsr_set_error("points_out is null with n %lld", (long long)n); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(te_voxel_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, w.order, w.head, w.off,
                       points_out, cell_of_point_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- TNT_ICP_SUMS
// The fixed order of gsr_block_sum_256 (cloud_common.h) for TE_SUM_VALUES sums at once.
struct TeMeans { double s[3], t[3]; };

// PASS2 false: v = (count, sum s.xyz, sum t.xyz, sum d^2, 0, 0); true: v = (sum (t - tm)(s - sm)^T row-major, sum |s - sm|^2)
template <bool PASS2>
__global__ void __launch_bounds__(256) te_sums_kernel(const float* __restrict__ src, const float* __restrict__ tgt, int64_t n,
                                                      int64_t n_tgt, const double* __restrict__ dist, const int32_t* __restrict__ idx,
                                                      TeMeans mu, double* __restrict__ partial) {
    __shared__ double s_val[TE_SUM_VALUES * 256];
    double v[TE_SUM_VALUES];
#pragma unroll
    for (int q = 0; q < TE_SUM_VALUES; ++q) v[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t j = idx[i];
        if ((uint64_t)j >= (uint64_t)n_tgt) continue;          // -1: no correspondence (anything else outside: never read)
        const double sx = (double)src[3 * i], sy = (double)src[3 * i + 1], sz = (double)src[3 * i + 2];
        const double tx = (double)tgt[3 * (int64_t)j], ty = (double)tgt[3 * (int64_t)j + 1], tz = (double)tgt[3 * (int64_t)j + 2];
        if (!PASS2) {
            const double d = dist[i];
            v[0] += 1.0;
            v[1] += sx; v[2] += sy; v[3] += sz;
            v[4] += tx; v[5] += ty; v[6] += tz;
            v[7] += d * d;
        } else {
            const double ds[3] = {sx - mu.s[0], sy - mu.s[1], sz - mu.s[2]};
            const double dt[3] = {tx - mu.t[0], ty - mu.t[1], tz - mu.t[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[3 * r + c] += dt[r] * ds[c];
            }
            v[9] += (ds[0] * ds[0] + ds[1] * ds[1]) + ds[2] * ds[2];
        }
    }
    gsr_block_sum_256(v, s_val);
    if (threadIdx.x < TE_SUM_VALUES) partial[(int64_t)blockIdx.x * TE_SUM_VALUES + threadIdx.x] = s_val[threadIdx.x * 256];
}

__global__ void __launch_bounds__(256) te_sums_final_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
    __shared__ double s_val[TE_SUM_VALUES * 256];
    double v[TE_SUM_VALUES];
#pragma unroll
    for (int q = 0; q < TE_SUM_VALUES; ++q) v[q] = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256) {
#pragma unroll
        for (int q = 0; q < TE_SUM_VALUES; ++q) v[q] += partial[(int64_t)b * TE_SUM_VALUES + q];
    }
    gsr_block_sum_256(v, s_val);
    if (threadIdx.x < TE_SUM_VALUES) out[threadIdx.x] = s_val[threadIdx.x * 256];
}

extern "C" size_t gsr_icp_sums_workspace_bytes(int64_t n) { (void)n; return gsr_align(size_t(GSR_PARTIAL_BLOCKS) * TE_SUM_VALUES * 8); }

extern "C" int32_t gsr_icp_sums(const float* source, int64_t n_source, const float* target, int64_t n_target, const double* dist,
                                const int32_t* idx, const double* means_host, void* ws, size_t ws_bytes, double* out,
                                gsr_stream_t stream_) {
    int rc = gsr_check_count("n_source", n_source);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_count("n_target", n_target);
    if (rc != GSR_OK) return rc;
    if (!out) { gsr_set_error("out (device f64 [10]) is required"); return GSR_E_INVALID; }
    if (n_source > 0 && (!source || !dist || !idx)) {
        gsr_set_error("source / dist / idx are null with n_source %lld", (long long)n_source);
        return GSR_E_INVALID;
    }
    if (n_source > 0 && n_target > 0 && !target) { gsr_set_error("target is null with n_target %lld", (long long)n_target); return GSR_E_INVALID; }
    if (!ws || ws_bytes < gsr_icp_sums_workspace_bytes(n_source)) {
        gsr_set_error("ws_bytes: ICP sums workspace too small (%zu < %zu bytes)", ws_bytes, gsr_icp_sums_workspace_bytes(n_source));
        return GSR_E_INVALID;
    }
    TeMeans mu{};
    if (means_host) {
        for (int a = 0; a < 3; ++a) { mu.s[a] = means_host[a]; mu.t[a] = means_host[3 + a]; }
    }
    double* partial = static_cast<double*>(ws);
    const unsigned blocks = gsr_partial_blocks(n_source);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (blocks > 0) {
        if (means_host)
            hipLaunchKernelGGL(te_sums_kernel<true>, dim3(blocks), dim3(256), 0, s, source, target, n_source, n_target, dist,
                               idx, mu, partial);
        else
            hipLaunchKernelGGL(te_sums_kernel<false>, dim3(blocks), dim3(256), 0, s, source, target, n_source, n_target,
                               dist, idx, mu, partial);
        GSR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(te_sums_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)blocks, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- TNT_SCORE
// LDS: the B + 1 edges, then B int32 bins.  A value's bin is (number of edges <= d) - 1, the last edge belonging to the last
// bin; values outside [e_0, e_B] (NaN and +inf included) fall in no bin.
__global__ void __launch_bounds__(256) te_score_kernel(const double* __restrict__ dist, int64_t n, const double* __restrict__ edges,
                                                       int B, double tau, unsigned long long* __restrict__ count,
                                                       unsigned long long* __restrict__ hist) {
    extern __shared__ double s_mem[];
    double* s_edge = s_mem;
    int* s_bin = reinterpret_cast<int*>(s_mem + (B + 1));
    for (int k = threadIdx.x; k <= B; k += 256) s_edge[k] = edges[k];
    for (int k = threadIdx.x; k < B; k += 256) s_bin[k] = 0;
    __syncthreads();
    const double e0 = s_edge[0], eB = s_edge[B];
    unsigned long long below = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double d = dist[i];
        below += d < tau;
        if (d >= e0 && d <= eB) {
            int lo = 0, hi = B + 1;                     // first edge > d
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_edge[mid] <= d) lo = mid + 1; else hi = mid;
            }
            int b = lo - 1;
            if (b >= B) b = B - 1;
            atomicAdd(&s_bin[b], 1);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) below += __shfl_xor(below, d, 64);
    if ((threadIdx.x & 63) == 0 && below) atomicAdd(count, below);
    __syncthreads();
    for (int k = threadIdx.x; k < B; k += 256) {
        const int c = s_bin[k];
        if (c) atomicAdd(&hist[k], (unsigned long long)c);
    }
}

extern "C" size_t gsr_dist_score_workspace_bytes(int32_t n_bins) {
    return gsr_align(size_t(n_bins > 0 ? n_bins : 1) * 8 + 8);
}

extern "C" int32_t gsr_dist_score(const double* dist, int64_t n, const double* edges_host, int32_t n_bins, double tau, void* ws,
                                  size_t ws_bytes, int64_t* count_out, int64_t* hist_out, gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_positive("tau", tau);
    if (rc != GSR_OK) return rc;
    if (n_bins < 1) { gsr_set_error("n_bins must be >= 1 (got %d)", n_bins); return GSR_E_INVALID; }
    if (n_bins > TE_MAX_BINS) { gsr_set_error("n_bins %d exceeds %d", n_bins, TE_MAX_BINS); return GSR_E_UNSUPPORTED; }
    if (!edges_host) { gsr_set_error("edges_host (n_bins + 1 values) is required"); return GSR_E_INVALID; }
    for (int k = 0; k <= n_bins; ++k) {
        const bool finite = edges_host[k] >= -DBL_MAX && edges_host[k] <= DBL_MAX;
        if (!finite || (k > 0 && edges_host[k] < edges_host[k - 1])) {
            gsr_set_error("edges_host must be finite and must not decrease (entry %d)", k);
            return GSR_E_INVALID;
        }
    }
    if (!count_out || !hist_out) { gsr_set_error("count_out / hist_out are required"); return GSR_E_INVALID; }
    if (n > 0 && !dist) { gsr_set_error("dist is null with n %lld", (long long)n); return GSR_E_INVALID; }
    if (!ws || ws_bytes < gsr_dist_score_workspace_bytes(n_bins)) {
        gsr_set_error("ws_bytes: score workspace too small (%zu < %zu bytes)", ws_bytes, gsr_dist_score_workspace_bytes(n_bins));
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GSR_HIP_CHECK(hipMemsetAsync(count_out, 0, 8, s));
    GSR_HIP_CHECK(hipMemsetAsync(hist_out, 0, size_t(n_bins) * 8, s));
    if (n == 0) return GSR_OK;
    double* edges = static_cast<double*>(ws);
    // (pageable source: the copy has left edges_host when the call returns)
    GSR_HIP_CHECK(hipMemcpyAsync(edges, edges_host, size_t(n_bins + 1) * 8, hipMemcpyHostToDevice, s));
    const size_t lds = size_t(n_bins + 1) * 8 + size_t(n_bins) * 4;
    hipLaunchKernelGGL(te_score_kernel, dim3(gsr_partial_blocks(n)), dim3(256), lds, s, dist, n, edges, n_bins, tau,
                       reinterpret_cast<unsigned long long*>(count_out), reinterpret_cast<unsigned long long*>(hist_out));
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
