// TSDF fusion of depth / colour views into a block-sparse voxel volume (include/gsr.h, "mesh export"): the bounded mesh path
// of the reference (utils/mesh_utils.py:125-170), which calls Open3D's ScalableTSDFVolume there.
//
//   tsdf_touch_kernel     stride-4 pixel lattice: marks the blocks around each valid back-projected depth sample
//   tsdf_flags_kernel     per grid block: touched by this view? new?
//   tsdf_scan_*           two exclusive scans of those flags (scan_bodies.h), one launch each half
//   tsdf_assign_kernel    new blocks get pool slots in grid order, the touched list is compacted
//   tsdf_integrate_kernel one workgroup per touched block, one thread per voxel column (16 voxels)
//   tsdf_depth_aabb_kernel running AABB of a view's back-projected valid depth (places the grid before the first touch)
#include "tsdf_common.h"
#include "wave_reduce.h"

#include <math.h>

// ---------------------------------------------------------------- recalled Open3D rules (include/gsr.h lists them)
#define TSDF_TOUCH_STRIDE 4          // allocation samples the depth image on a stride-4 pixel lattice
#define TSDF_PIXEL_ROUND 0.5f        // projected pixel coordinate + 0.5, truncated
#define TSDF_BORDER 1e-4f            // projected coordinates within 1e-4 of the image border are rejected
// distance along the pixel's ray per unit of depth difference
__device__ __forceinline__ float tsdf_ray_multiplier(int u, int v, float fx, float fy, float cx, float cy) {
    const float a = (u - cx) / fx, b = (v - cy) / fy;
    return sqrtf(1.f + a * a + b * b);
}

struct TsdfCam {
    float fx, fy, cx, cy;
    float m[12];   // row-major 3x4: world -> camera (integrate) or camera -> world (touch)
};

__device__ __forceinline__ bool tsdf_pixel_valid(float d, float depth_trunc) { return d > 0.f && d <= depth_trunc; }

__global__ void __launch_bounds__(256) tsdf_touch_kernel(TsdfGrid g, TsdfCam cam, const float* __restrict__ depth,
                                                         const uint8_t* __restrict__ mask, int H, int W, float depth_trunc,
                                                         float sdf_trunc, int stamp_val, int* __restrict__ stamp,
                                                         uint32_t* __restrict__ header) {
    const int lw = (W + TSDF_TOUCH_STRIDE - 1) / TSDF_TOUCH_STRIDE, lh = (H + TSDF_TOUCH_STRIDE - 1) / TSDF_TOUCH_STRIDE;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)lw * lh) return;
    const int u = (int)(i % lw) * TSDF_TOUCH_STRIDE, v = (int)(i / lw) * TSDF_TOUCH_STRIDE;
    const int64_t pix = (int64_t)v * W + u;
    const float d = depth[pix];
    if (!tsdf_pixel_valid(d, depth_trunc) || (mask && !mask[pix])) return;
    const float xc = (u - cam.cx) * d / cam.fx, yc = (v - cam.cy) * d / cam.fy;
    float p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = cam.m[4 * r] * xc + cam.m[4 * r + 1] * yc + cam.m[4 * r + 2] * d + cam.m[4 * r + 3];
    const float bl = TSDF_B * g.vs;
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int)floorf((p[a] - sdf_trunc) / bl) - g.lo[a];
        hi[a] = (int)floorf((p[a] + sdf_trunc) / bl) - g.lo[a];
        if (lo[a] < 0 || hi[a] >= g.dim[a]) {   // outside the AABB: the call fails, nothing is written
            atomicOr(header, 1u);
            return;
        }
    }
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x)
                stamp[x + (int64_t)g.dim[0] * (y + (int64_t)g.dim[1] * z)] = stamp_val;
}

// Running AABB of the back-projected valid depth (gsr_depth_aabb): floats as order-preserving u32, so that the six running
// bounds are integer atomics -- exact, and the same whatever the order
__device__ __forceinline__ uint32_t tsdf_float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

#define TSDF_AABB_MAX_BLOCKS 1024    // grid-stride beyond: a wave folds several pixels per lane before its six atomics

__global__ void __launch_bounds__(256) tsdf_depth_aabb_kernel(TsdfCam cam, const float* __restrict__ depth,
                                                              const uint8_t* __restrict__ mask, int H, int W,
                                                              float depth_trunc, uint32_t* __restrict__ bounds) {
    const int64_t n = (int64_t)H * W, stride = (int64_t)gridDim.x * blockDim.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float d = depth[i];
        if (!tsdf_pixel_valid(d, depth_trunc) || (mask && !mask[i])) continue;
        const int u = (int)(i % W), v = (int)(i / W);
        const float xc = (u - cam.cx) * d / cam.fx, yc = (v - cam.cy) * d / cam.fy;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float p = cam.m[4 * r] * xc + cam.m[4 * r + 1] * yc + cam.m[4 * r + 2] * d + cam.m[4 * r + 3];
            lo[r] = fminf(lo[r], p);
            hi[r] = fmaxf(hi[r], p);
        }
        any = true;
    }
    if (!__ballot(any)) return;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float l = wave_min_f32(lo[r]), h = wave_max_f32(hi[r]);
        if ((threadIdx.x & 63) == 0) {
            atomicMin(bounds + r, tsdf_float_key(l));
            atomicMax(bounds + 3 + r, tsdf_float_key(h));
        }
    }
}

__global__ void __launch_bounds__(256) tsdf_flags_kernel(int64_t n, int stamp_val, const int* __restrict__ stamp,
                                                         const int* __restrict__ block_index, uint8_t* __restrict__ flags) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const bool touched = stamp[b] == stamp_val;
    flags[b] = touched;
    flags[n + b] = touched && block_index[b] < 0;
}

// the two scans (blockIdx.y: 0 touched, 1 new) of the flags
__global__ void __launch_bounds__(SCAN_BLOCK) tsdf_scan_reduce_kernel(const uint8_t* __restrict__ flags,
                                                                      uint32_t* __restrict__ partial, int64_t n) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    const int64_t tiles = scan_tiles(n);
    scan_reduce_body<uint8_t>(flags + blockIdx.y * n, nullptr, partial + blockIdx.y * tiles, n, blockIdx.x, wt);
}

__global__ void __launch_bounds__(SCAN_BLOCK) tsdf_scan_apply_kernel(const uint8_t* __restrict__ flags,
                                                                     const uint32_t* __restrict__ partial,
                                                                     uint32_t* __restrict__ scans, int64_t n) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    const int64_t tiles = scan_tiles(n);
    scan_apply_body<uint8_t>(flags + blockIdx.y * n, nullptr, partial + blockIdx.y * tiles, scans + blockIdx.y * (n + 1), n,
                             blockIdx.x, wt);
}

__global__ void __launch_bounds__(256) tsdf_assign_kernel(int64_t n, int64_t n_alloc, const uint8_t* __restrict__ flags,
                                                          const uint32_t* __restrict__ scans, int* __restrict__ block_index,
                                                          int* __restrict__ slot_block, int* __restrict__ touched,
                                                          uint32_t* __restrict__ header) {
    if (header[0]) return;   // a sample fell outside the AABB: the view is rejected as a whole
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) {
        header[1] = scans[n];
        header[2] = scans[(n + 1) + n];
    }
    if (b >= n) return;
    if (flags[b]) touched[scans[b]] = (int)b;
    if (flags[n + b]) {
        const int64_t slot = n_alloc + scans[(n + 1) + b];
        block_index[b] = (int)slot;
        slot_block[slot] = (int)b;
    }
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_integrate_kernel(TsdfGrid g, TsdfCam cam, const int* __restrict__ touched,
                                                                      const int* __restrict__ block_index,
                                                                      float* __restrict__ pool, int64_t pool_blocks,
                                                                      const float* __restrict__ depth,
                                                                      const uint8_t* __restrict__ mask,
                                                                      const float* __restrict__ rgb, int H, int W,
                                                                      float depth_trunc, float sdf_trunc) {
    const int b = touched[blockIdx.x];
    const int64_t slot = block_index[b];
    int bx, by, bz;
    tsdf_block_coords(g, b, bx, by, bz);
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const float wx = ((float)((g.lo[0] + bx) * TSDF_B + lx) + 0.5f) * g.vs;
    const float wy = ((float)((g.lo[1] + by) * TSDF_B + ly) + 0.5f) * g.vs;
    const int64_t plane = pool_blocks * TSDF_BV;
    float* tsdf = pool + slot * TSDF_BV;
    float* wgt = tsdf + plane;
    float* col = tsdf + 2 * plane;
    const int64_t HW = (int64_t)H * W;
    for (int lz = 0; lz < TSDF_B; ++lz) {
        const float wz = ((float)((g.lo[2] + bz) * TSDF_B + lz) + 0.5f) * g.vs;
        const float x = cam.m[0] * wx + cam.m[1] * wy + cam.m[2] * wz + cam.m[3];
        const float y = cam.m[4] * wx + cam.m[5] * wy + cam.m[6] * wz + cam.m[7];
        const float z = cam.m[8] * wx + cam.m[9] * wy + cam.m[10] * wz + cam.m[11];
        if (z <= 0.f) continue;
        const float uf = cam.fx * x / z + cam.cx + TSDF_PIXEL_ROUND;
        const float vf = cam.fy * y / z + cam.cy + TSDF_PIXEL_ROUND;
        if (!(uf >= TSDF_BORDER && uf < W - TSDF_BORDER && vf >= TSDF_BORDER && vf < H - TSDF_BORDER)) continue;
        const int u = (int)uf, v = (int)vf;
        const int64_t pix = (int64_t)v * W + u;
        const float d = depth[pix];
        if (!tsdf_pixel_valid(d, depth_trunc) || (mask && !mask[pix])) continue;
        const float sdf = (d - z) * tsdf_ray_multiplier(u, v, cam.fx, cam.fy, cam.cx, cam.cy);
        if (!(sdf > -sdf_trunc)) continue;
        const float t = fminf(1.f, sdf / sdf_trunc);
        const int l = threadIdx.x + TSDF_THREADS * lz;
        const float w = wgt[l], w1 = w + 1.f;
        tsdf[l] = (tsdf[l] * w + t) / w1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float rc = fminf(fmaxf(rgb[c * HW + pix], 0.f), 1.f);
            const float c8 = (float)(int)(rc * 255.f);   // (uint8)(clip(rgb, 0, 1) * 255), truncated (mesh_utils.py:158)
            col[c * plane + l] = (col[c * plane + l] * w + c8) / w1;
        }
        wgt[l] = w1;
    }
}

// ---------------------------------------------------------------- host side
int tsdf_check_volume(const GsrTsdfVolume* vol, TsdfGrid& g, int64_t& n_blocks) {
    if (!vol) { gsr_set_error("null volume"); return GSR_E_INVALID; }
    if (!(vol->voxel_size > 0.f) || !isfinite(vol->voxel_size)) {
        gsr_set_error("voxel_size must be > 0 (got %g)", (double)vol->voxel_size);
        return GSR_E_INVALID;
    }
    if (!(vol->sdf_trunc > 0.f) || !isfinite(vol->sdf_trunc)) {
        gsr_set_error("sdf_trunc must be > 0 (got %g)", (double)vol->sdf_trunc);
        return GSR_E_INVALID;
    }
    n_blocks = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t d = (int64_t)vol->block_hi[a] - vol->block_lo[a];
        if (d < 0) {
            gsr_set_error("block AABB is inverted on axis %d (lo %d > hi %d)", a, vol->block_lo[a], vol->block_hi[a]);
            return GSR_E_INVALID;
        }
        g.lo[a] = vol->block_lo[a];
        g.dim[a] = (int)(d < (int64_t)INT32_MAX ? d : INT32_MAX);
        n_blocks *= d;
        if (n_blocks > GSR_TSDF_BLOCK_CAP) break;
    }
    if (n_blocks > GSR_TSDF_BLOCK_CAP) {
        gsr_set_error("TSDF block grid of %d x %d x %d blocks exceeds the cap of %lld blocks: raise voxel_size or lower "
                      "depth_trunc (voxel_size %g)", vol->block_hi[0] - vol->block_lo[0], vol->block_hi[1] - vol->block_lo[1],
                      vol->block_hi[2] - vol->block_lo[2], (long long)GSR_TSDF_BLOCK_CAP, (double)vol->voxel_size);
        return GSR_E_UNSUPPORTED;
    }
    // voxel coordinates of the grid must stay in int32
    for (int a = 0; a < 3; ++a) {
        if (llabs((int64_t)vol->block_lo[a]) * TSDF_B > (1LL << 30) || llabs((int64_t)vol->block_hi[a]) * TSDF_B > (1LL << 30)) {
            gsr_set_error("block AABB too far from the origin for voxel_size %g", (double)vol->voxel_size);
            return GSR_E_INVALID;
        }
    }
    g.vs = vol->voxel_size;
    return GSR_OK;
}

extern "C" int32_t gsr_tsdf_sizes(const GsrTsdfVolume* vol, int64_t* n_blocks, size_t* workspace_bytes,
                                  size_t* slot_block_offset) {
    TsdfGrid g;
    int64_t n = 0;
    const int rc = tsdf_check_volume(vol, g, n);
    if (rc != GSR_OK) return rc;
    if (n_blocks) *n_blocks = n;
    const TsdfWs w = tsdf_ws_layout(nullptr, n);
    if (workspace_bytes) *workspace_bytes = w.bytes;
    if (slot_block_offset) *slot_block_offset = w.slot_block_offset;
    return GSR_OK;
}

static int tsdf_check_view(const GsrTsdfVolume* vol, const float* depth, int H, int W, const float* intr, const float* w2c,
                           float depth_trunc, TsdfGrid& g, int64_t& n, TsdfWs& ws) {
    int rc = tsdf_check_volume(vol, g, n);
    if (rc != GSR_OK) return rc;
    if (H <= 0 || W <= 0) { gsr_set_error("empty image (%d x %d)", H, W); return GSR_E_INVALID; }
    if (!depth || !intr || !w2c) { gsr_set_error("depth, intrinsics and w2c are required"); return GSR_E_INVALID; }
    if (!(intr[0] > 0.f) || !(intr[1] > 0.f)) { gsr_set_error("focal lengths must be > 0"); return GSR_E_INVALID; }
    if (!(depth_trunc > 0.f)) { gsr_set_error("depth_trunc must be > 0 (got %g)", (double)depth_trunc); return GSR_E_INVALID; }
    if (n > 0 && (!vol->block_index || !vol->workspace)) { gsr_set_error("block_index / workspace missing"); return GSR_E_INVALID; }
    ws = tsdf_ws_layout(vol->workspace, n);
    if (n > 0 && vol->workspace_bytes < ws.bytes) {
        gsr_set_error("workspace too small (%zu < %zu bytes)", vol->workspace_bytes, ws.bytes);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

static TsdfCam tsdf_cam(const float* intr, const double m[12]) {
    TsdfCam c;
    c.fx = intr[0]; c.fy = intr[1]; c.cx = intr[2]; c.cy = intr[3];
    for (int i = 0; i < 12; ++i) c.m[i] = (float)m[i];
    return c;
}

extern "C" int32_t gsr_tsdf_touch(GsrTsdfVolume* vol, const float* depth, const uint8_t* mask, int32_t H, int32_t W,
                                  const float* intr, const float* w2c, float depth_trunc, int64_t* n_touched,
                                  gsr_stream_t stream_) {
    TsdfGrid g;
    int64_t n = 0;
    TsdfWs ws;
    int rc = tsdf_check_view(vol, depth, H, W, intr, w2c, depth_trunc, g, n, ws);
    if (rc != GSR_OK) return rc;
    if (!n_touched) { gsr_set_error("n_touched is required"); return GSR_E_INVALID; }
    *n_touched = 0;
    if (n == 0) return GSR_OK;   // empty grid: nothing to touch, nothing launched
    // camera -> world: inverse of the affine w2c (in double)
    double R[9], t[3], inv[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = w2c[4 * r + c];
        t[r] = w2c[4 * r + 3];
    }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(fabs(det) > 1e-12)) { gsr_set_error("w2c is singular"); return GSR_E_INVALID; }
    const double Ri[9] = {(R[4] * R[8] - R[5] * R[7]) / det, (R[2] * R[7] - R[1] * R[8]) / det, (R[1] * R[5] - R[2] * R[4]) / det,
                          (R[5] * R[6] - R[3] * R[8]) / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[2] * R[3] - R[0] * R[5]) / det,
                          (R[3] * R[7] - R[4] * R[6]) / det, (R[1] * R[6] - R[0] * R[7]) / det, (R[0] * R[4] - R[1] * R[3]) / det};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) inv[4 * r + c] = Ri[3 * r + c];
        inv[4 * r + 3] = -(Ri[3 * r] * t[0] + Ri[3 * r + 1] * t[1] + Ri[3 * r + 2] * t[2]);
    }
    unsigned long long* host = gsr_pinned_words(2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int stamp_val = vol->n_views + 1;
    const TsdfCam cam = tsdf_cam(intr, inv);
    GSR_HIP_CHECK(hipMemsetAsync(ws.header, 0, 16, s));
    const int64_t lattice = (int64_t)((W + TSDF_TOUCH_STRIDE - 1) / TSDF_TOUCH_STRIDE) * ((H + TSDF_TOUCH_STRIDE - 1) / TSDF_TOUCH_STRIDE);
    hipLaunchKernelGGL(tsdf_touch_kernel, dim3((unsigned)((lattice + 255) / 256)), dim3(256), 0, s, g, cam, depth, mask, H, W,
                       depth_trunc, vol->sdf_trunc, stamp_val, ws.stamp, ws.header);
    GSR_LAUNCH_CHECK();
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(tsdf_flags_kernel, dim3(nb), dim3(256), 0, s, n, stamp_val, ws.stamp, vol->block_index, ws.flags);
    GSR_LAUNCH_CHECK();
    const dim3 sg((unsigned)scan_tiles(n), 2);
    hipLaunchKernelGGL(tsdf_scan_reduce_kernel, sg, dim3(SCAN_BLOCK), 0, s, ws.flags, ws.partial, n);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsdf_scan_apply_kernel, sg, dim3(SCAN_BLOCK), 0, s, ws.flags, ws.partial, ws.scans, n);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsdf_assign_kernel, dim3(nb), dim3(256), 0, s, n, vol->n_alloc, ws.flags, ws.scans, vol->block_index,
                       ws.slot_block, ws.touched, ws.header);
    GSR_LAUNCH_CHECK();
    // the one synchronisation of a view: the caller sizes the pool from the new-block count before integrating
    GSR_HIP_CHECK(hipMemcpyAsync(host, ws.header, 12, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    const uint32_t* h = reinterpret_cast<const uint32_t*>(host);
    vol->n_views += 1;
    if (h[0]) {
        gsr_set_error("view %d touches TSDF blocks outside the block AABB [%d,%d,%d]..[%d,%d,%d): enlarge the AABB "
                      "(or lower depth_trunc)", vol->n_views - 1, vol->block_lo[0], vol->block_lo[1], vol->block_lo[2],
                      vol->block_hi[0], vol->block_hi[1], vol->block_hi[2]);
        return GSR_E_INVALID;
    }
    *n_touched = h[1];
    vol->n_alloc += h[2];
    return GSR_OK;
}

extern "C" int32_t gsr_tsdf_integrate(const GsrTsdfVolume* vol, const float* depth, const uint8_t* mask, const float* rgb,
                                      int32_t H, int32_t W, const float* intr, const float* w2c, float depth_trunc,
                                      int64_t n_touched, gsr_stream_t stream_) {
    TsdfGrid g;
    int64_t n = 0;
    TsdfWs ws;
    int rc = tsdf_check_view(vol, depth, H, W, intr, w2c, depth_trunc, g, n, ws);
    if (rc != GSR_OK) return rc;
    if (!rgb) { gsr_set_error("rgb is required"); return GSR_E_INVALID; }
    if (n_touched < 0 || n_touched > n || n_touched > vol->n_alloc) {
        gsr_set_error("n_touched %lld out of range (grid %lld blocks, %lld allocated)", (long long)n_touched, (long long)n,
                      (long long)vol->n_alloc);
        return GSR_E_INVALID;
    }
    if (n_touched == 0) return GSR_OK;
    if (!vol->pool || vol->pool_blocks < vol->n_alloc) {
        gsr_set_error("pool of %lld blocks cannot hold the %lld allocated ones", (long long)vol->pool_blocks,
                      (long long)vol->n_alloc);
        return GSR_E_INVALID;
    }
    double m[12];
    for (int i = 0; i < 12; ++i) m[i] = w2c[i];
    const TsdfCam cam = tsdf_cam(intr, m);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)n_touched), dim3(TSDF_THREADS), 0, s, g, cam, ws.touched,
                       vol->block_index, vol->pool, vol->pool_blocks, depth, mask, rgb, H, W, depth_trunc, vol->sdf_trunc);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_depth_aabb(const float* depth, const uint8_t* mask, int32_t H, int32_t W, const float* intr,
                                  const float* c2w, float depth_trunc, uint32_t* bounds, gsr_stream_t stream_) {
    if (H <= 0 || W <= 0) { gsr_set_error("empty image (%d x %d)", H, W); return GSR_E_INVALID; }
    if (!depth || !intr || !c2w || !bounds) { gsr_set_error("depth, intrinsics, c2w and bounds are required"); return GSR_E_INVALID; }
    if (!(intr[0] > 0.f) || !(intr[1] > 0.f)) { gsr_set_error("focal lengths must be > 0"); return GSR_E_INVALID; }
    if (!(depth_trunc > 0.f)) { gsr_set_error("depth_trunc must be > 0 (got %g)", (double)depth_trunc); return GSR_E_INVALID; }
    double m[12];
    for (int i = 0; i < 12; ++i) m[i] = c2w[i];
    const TsdfCam cam = tsdf_cam(intr, m);
    const int64_t n = (int64_t)H * W;
    int64_t blocks = (n + 255) / 256;
    if (blocks > TSDF_AABB_MAX_BLOCKS) blocks = TSDF_AABB_MAX_BLOCKS;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(tsdf_depth_aabb_kernel, dim3((unsigned)blocks), dim3(256), 0, s, cam, depth, mask, H, W, depth_trunc,
                       bounds);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
