// Unbounded mesh export (include/gsr.h, "unbounded mesh export"): the contracted-space TSDF field of the reference's
// extract_mesh_unbounded, with every view fused inside one launch.  The view table (GsrUnbView records) is read uniformly,
// so the compiler keeps a record in scalar registers; a thread keeps tsdf, w (and rgb) of its points in vector registers
// across the view loop and stores once.
//
//   unb_points_kernel      [n,3] points, grid-stride, 64-bit indexing                     -> tsdf [n] (, rgb [n,3])
//   unb_box_kernel         a sub-box of the lattice, coordinates by UNB_LATTICE           -> dense f32 [dx,dy,dz]
//   unb_flags_kernel       pass 1: one workgroup per 16^3 block of the lattice            -> sign flags u8 per block
//   unb_select_kernel      UNB_ALLOC: anchors dilated by +{0,1}^3                         -> allocated u8 per block
//   unb_scan_* / unb_assign_kernel   slots in grid order (scan_bodies.h)                  -> block_index, slot_block
//   unb_fill_kernel        pass 2: one workgroup per allocated block                      -> pool tsdf / weight
//   unb_finish_kernel      UNB_VERTEX: index-space vertices -> world                      -> vertices in place
//
// The three evaluating kernels run ONE device body (unb_eval) and this object is built with -ffp-contract=off (Makefile):
// the compiler may not fuse a multiply and an add differently in each of them, so pass 1, pass 2 and the dense box give the
// same bits for the same lattice point.
#include "tsdf_common.h"
#include "wave_reduce.h"

#include <math.h>

#define UNB_PPT 4   // lattice points a thread carries through the view loop: 4 x 4 independent taps in flight per view

struct UnbFrame {
    float center[3];
    float radius;
    float trunc0;    // UNB_TRUNC's constant 5 voxel_size, rounded once to f32 by the host
};

struct UnbLattice {
    double R, step;  // UNB_LATTICE: s = -R + g step, step = 2R / (G - 1)
    int G;
};

// UNB_LATTICE: lattice coordinate of index g, formed in fp64 and rounded to fp32
__device__ __forceinline__ float unb_coord(const UnbLattice& L, int g) { return (float)(-L.R + (double)g * L.step); }

// UNB_CONTRACT: contracted -> normalised coordinates, torch's operations in torch's order (1 / (2 - m)) * (s / m); whatever
// that arithmetic gives for m >= 2 is the rule
__device__ __forceinline__ void unb_uncontract(const float (&s)[3], float m, float (&y)[3]) {
    const float a = 1.f / (2.f - m);
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = m < 1.f ? s[k] : a * (s[k] / m);
}

__device__ __forceinline__ float unb_norm(const float (&s)[3]) { return sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]); }

// UNB_TRUNC: the truncation of a contracted sample
__device__ __forceinline__ float unb_trunc(float trunc0, float m) {
    return m > 1.f ? trunc0 * (1.f / (2.f - fminf(m, 1.9f))) : trunc0;
}

// contracted sample -> world point and truncation
__device__ __forceinline__ void unb_world(const UnbFrame& f, const float (&s)[3], float (&x)[3], float& trunc) {
    const float m = unb_norm(s);
    float y[3];
    unb_uncontract(s, m, y);
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = y[k] * f.radius + f.center[k];
    trunc = unb_trunc(f.trunc0, m);
}

// UNB_SAMPLE: grid_sample, bilinear, border padding, align_corners: four taps with clamped indices
struct UnbTaps {
    int64_t i[4];
    float w[4];
};
__device__ __forceinline__ UnbTaps unb_taps(float u, float v, int H, int W) {
    float ix = (u + 1.f) / 2.f * (float)(W - 1);
    float iy = (v + 1.f) / 2.f * (float)(H - 1);
    ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
    iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float ax = ix - fx, ay = iy - fy, bx = (fx + 1.f) - ix, by = (fy + 1.f) - iy;
    UnbTaps t;
    t.i[0] = (int64_t)y0 * W + x0; t.w[0] = bx * by;   // nw
    t.i[1] = (int64_t)y0 * W + x1; t.w[1] = ax * by;   // ne
    t.i[2] = (int64_t)y1 * W + x0; t.w[2] = bx * ay;   // sw
    t.i[3] = (int64_t)y1 * W + x1; t.w[3] = ax * ay;   // se
    return t;
}
__device__ __forceinline__ float unb_sample(const float* __restrict__ map, const UnbTaps& t) {
    float r = map[t.i[0]] * t.w[0];
    r = r + map[t.i[1]] * t.w[1];
    r = r + map[t.i[2]] * t.w[2];
    r = r + map[t.i[3]] * t.w[3];
    return r;
}

// The shared device body: fuses every view into P points held in registers.  x: world points, trunc: their truncations.
// UNB_FUSE starts at tsdf = 1, rgb = 0 and w = 1 (the reference's start).
template <int P, bool RGB>
__device__ __forceinline__ void unb_eval(const GsrUnbView* __restrict__ views, int n_views, const float (&x)[P][3],
                                         const float (&trunc)[P], float (&tsdf)[P], float (&rgb)[P][3]) {
    float w[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        tsdf[p] = 1.f;
        w[p] = 1.f;
        rgb[p][0] = rgb[p][1] = rgb[p][2] = 0.f;
    }
    for (int v = 0; v < n_views; ++v) {
        const GsrUnbView& V = views[v];   // uniform address: scalar loads
        const int H = V.height, W = V.width;
        const int64_t HW = (int64_t)H * W;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            // UNB_PROJECT: p = [x, 1] @ full_proj_transform; only columns x, y and w are needed
            const float px = x[p][0] * V.col_x[0] + x[p][1] * V.col_x[1] + x[p][2] * V.col_x[2] + V.col_x[3];
            const float py = x[p][0] * V.col_y[0] + x[p][1] * V.col_y[1] + x[p][2] * V.col_y[2] + V.col_y[3];
            const float z = x[p][0] * V.col_w[0] + x[p][1] * V.col_w[1] + x[p][2] * V.col_w[2] + V.col_w[3];
            const float pu = px / z, pv = py / z;
            if (!(pu > -1.f && pu < 1.f && pv > -1.f && pv < 1.f && z > 0.f)) continue;
            const UnbTaps t = unb_taps(pu, pv, H, W);
            const float sdf = unb_sample(V.depth, t) - z;
            // UNB_FUSE
            if (!(sdf > -trunc[p])) continue;
            const float tv = fminf(fmaxf(sdf / trunc[p], -1.f), 1.f);
            const float w1 = w[p] + 1.f;
            tsdf[p] = (tsdf[p] * w[p] + tv) / w1;
            if (RGB) {
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[p][c] = (rgb[p][c] * w[p] + unb_sample(V.rgb + c * HW, t)) / w1;
            }
            w[p] = w1;
        }
    }
}

// ---------------------------------------------------------------- entry 1: points
template <bool RGB>
__global__ void __launch_bounds__(256) unb_points_kernel(const GsrUnbView* __restrict__ views, int n_views, UnbFrame f,
                                                         const float* __restrict__ points, int64_t n, int contracted,
                                                         float* __restrict__ tsdf_out, float* __restrict__ rgb_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float s[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        float x[1][3], trunc[1], tsdf[1], rgb[1][3];
        if (contracted) {
            unb_world(f, s, x[0], trunc[0]);
        } else {
            x[0][0] = s[0]; x[0][1] = s[1]; x[0][2] = s[2];
            trunc[0] = f.trunc0;
        }
        unb_eval<1, RGB>(views, n_views, x, trunc, tsdf, rgb);
        tsdf_out[i] = tsdf[0];
        if (RGB) {
            rgb_out[3 * i] = rgb[0][0];
            rgb_out[3 * i + 1] = rgb[0][1];
            rgb_out[3 * i + 2] = rgb[0][2];
        }
    }
}

// ---------------------------------------------------------------- entry 2: lattice sub-box -> dense
struct UnbBox {
    int lo[3], dim[3];
};
__global__ void __launch_bounds__(256) unb_box_kernel(const GsrUnbView* __restrict__ views, int n_views, UnbFrame f,
                                                      UnbLattice L, UnbBox b, float* __restrict__ out) {
    const int64_t n = (int64_t)b.dim[0] * b.dim[1] * b.dim[2];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        // out is [dx, dy, dz], z fastest (torch.meshgrid(indexing="ij") flattened)
        const int gz = b.lo[2] + (int)(i % b.dim[2]);
        const int64_t r = i / b.dim[2];
        const int gy = b.lo[1] + (int)(r % b.dim[1]);
        const int gx = b.lo[0] + (int)(r / b.dim[1]);
        const float s[3] = {unb_coord(L, gx), unb_coord(L, gy), unb_coord(L, gz)};
        float x[1][3], trunc[1], tsdf[1], rgb[1][3];
        unb_world(f, s, x[0], trunc[0]);
        unb_eval<1, false>(views, n_views, x, trunc, tsdf, rgb);
        out[i] = tsdf[0];
    }
}

// ---------------------------------------------------------------- entry 3: block passes
// The field of lattice block (bx, by, bz): thread t owns voxel entries t + 256 z, z = 0..15 (the pool layout of
// tsdf_common.h), evaluated UNB_PPT z slices at a time.  val[z] = the field, inside[z] = the point lies on the lattice.
__device__ __forceinline__ void unb_block_field(const GsrUnbView* __restrict__ views, int n_views, const UnbFrame& f,
                                                const UnbLattice& L, int bx, int by, int bz, float (&val)[TSDF_B],
                                                bool& inside_xy) {
    const int gx = bx * TSDF_B + (threadIdx.x & 15), gy = by * TSDF_B + (threadIdx.x >> 4);
    inside_xy = gx < L.G && gy < L.G;
    const float sx = unb_coord(L, gx), sy = unb_coord(L, gy);
#pragma unroll
    for (int z0 = 0; z0 < TSDF_B; z0 += UNB_PPT) {
        float x[UNB_PPT][3], trunc[UNB_PPT], tsdf[UNB_PPT], rgb[UNB_PPT][3];
#pragma unroll
        for (int p = 0; p < UNB_PPT; ++p) {
            const float s[3] = {sx, sy, unb_coord(L, bz * TSDF_B + z0 + p)};
            unb_world(f, s, x[p], trunc[p]);
        }
        unb_eval<UNB_PPT, false>(views, n_views, x, trunc, tsdf, rgb);
#pragma unroll
        for (int p = 0; p < UNB_PPT; ++p) val[z0 + p] = tsdf[p];
    }
}

// pass 1: flags bit 0 = the block holds a negative value, bit 1 = a non-negative one (lattice points beyond G - 1 ignored)
__global__ void __launch_bounds__(TSDF_THREADS) unb_flags_kernel(const GsrUnbView* __restrict__ views, int n_views, UnbFrame f,
                                                                 UnbLattice L, TsdfGrid g, uint8_t* __restrict__ flags) {
    __shared__ float red[2][TSDF_THREADS / 64];
    int bx, by, bz;
    tsdf_block_coords(g, blockIdx.x, bx, by, bz);
    float val[TSDF_B];
    bool inside_xy;
    unb_block_field(views, n_views, f, L, bx, by, bz, val, inside_xy);
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int z = 0; z < TSDF_B; ++z) {
        if (inside_xy && bz * TSDF_B + z < L.G) {
            mn = fminf(mn, val[z]);
            mx = fmaxf(mx, val[z]);
        }
    }
    mn = wave_min_f32(mn);
    mx = wave_max_f32(mx);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mn;
        red[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TSDF_THREADS / 64; ++w) {
            mn = fminf(mn, red[0][w]);
            mx = fmaxf(mx, red[1][w]);
        }
        flags[blockIdx.x] = (uint8_t)((mn < 0.f ? 1 : 0) | (mx >= 0.f ? 2 : 0));
    }
}

// UNB_ALLOC: block a is an anchor when the union of the flags over a + {0,1}^3 has both signs; block b is allocated when one
// of b - {0,1}^3 is an anchor
__device__ __forceinline__ uint32_t unb_flag_at(const TsdfGrid& g, const uint8_t* __restrict__ flags, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= g.dim[0] || y >= g.dim[1] || z >= g.dim[2]) return 0;
    return flags[x + (int64_t)g.dim[0] * (y + (int64_t)g.dim[1] * z)];
}
__global__ void __launch_bounds__(256) unb_select_kernel(TsdfGrid g, int64_t n, const uint8_t* __restrict__ flags,
                                                         uint8_t* __restrict__ alloc) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    int bx, by, bz;
    tsdf_block_coords(g, (int)b, bx, by, bz);
    bool sel = false;
    for (int o = 0; o < 8 && !sel; ++o) {
        const int ax = bx - (o & 1), ay = by - ((o >> 1) & 1), az = bz - (o >> 2);
        if (ax < 0 || ay < 0 || az < 0) continue;
        uint32_t u = 0;
        for (int c = 0; c < 8; ++c) u |= unb_flag_at(g, flags, ax + (c & 1), ay + ((c >> 1) & 1), az + (c >> 2));
        sel = u == 3u;
    }
    alloc[b] = sel ? 1 : 0;
}

__global__ void __launch_bounds__(SCAN_BLOCK) unb_scan_reduce_kernel(const uint8_t* __restrict__ alloc,
                                                                     uint32_t* __restrict__ partial, int64_t n) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    scan_reduce_body<uint8_t>(alloc, nullptr, partial, n, blockIdx.x, wt);
}
__global__ void __launch_bounds__(SCAN_BLOCK) unb_scan_apply_kernel(const uint8_t* __restrict__ alloc,
                                                                    const uint32_t* __restrict__ partial,
                                                                    uint32_t* __restrict__ scans, int64_t n) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    scan_apply_body<uint8_t>(alloc, nullptr, partial, scans, n, blockIdx.x, wt);
}
__global__ void __launch_bounds__(256) unb_assign_kernel(int64_t n, const uint8_t* __restrict__ alloc,
                                                         const uint32_t* __restrict__ scans, int* __restrict__ block_index,
                                                         int* __restrict__ slot_block) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    if (alloc[b]) {
        block_index[b] = (int)scans[b];
        slot_block[scans[b]] = (int)b;
    } else {
        block_index[b] = -1;
    }
}

// pass 2: the allocated blocks straight into the pool, weight 1 inside the lattice and 0 beyond it
__global__ void __launch_bounds__(TSDF_THREADS) unb_fill_kernel(const GsrUnbView* __restrict__ views, int n_views, UnbFrame f,
                                                                UnbLattice L, TsdfGrid g, const int* __restrict__ slot_block,
                                                                float* __restrict__ pool, int64_t plane) {
    const int64_t slot = blockIdx.x;
    int bx, by, bz;
    tsdf_block_coords(g, slot_block[slot], bx, by, bz);
    float val[TSDF_B];
    bool inside_xy;
    unb_block_field(views, n_views, f, L, bx, by, bz, val, inside_xy);
    float* tsdf = pool + slot * TSDF_BV;
    float* wgt = tsdf + plane;
#pragma unroll
    for (int z = 0; z < TSDF_B; ++z) {
        const bool in = inside_xy && bz * TSDF_B + z < L.G;
        tsdf[threadIdx.x + TSDF_THREADS * z] = in ? val[z] : 1.f;
        wgt[threadIdx.x + TSDF_THREADS * z] = in ? 1.f : 0.f;
    }
}

// UNB_VERTEX: marching cubes with voxel_size 1 puts lattice index g at g + 0.5; back to the lattice coordinate (fp64, rounded
// once), then uncontract, un-normalise and clip in fp32
__global__ void __launch_bounds__(256) unb_finish_kernel(float* __restrict__ verts, int64_t n, UnbFrame f, UnbLattice L,
                                                         float max_range) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float s[3], y[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = (float)(-L.R + ((double)verts[3 * i + k] - 0.5) * L.step);
        unb_uncontract(s, unb_norm(s), y);
#pragma unroll
        for (int k = 0; k < 3; ++k) verts[3 * i + k] = fminf(fmaxf(y[k] * f.radius + f.center[k], -max_range), max_range);
    }
}

// ---------------------------------------------------------------- host side
#define UNB_MAX_GRID 65536   // workgroups of a grid-stride launch

static int unb_check_frame(const void* views, int32_t n_views, const float* center_host, float radius, float trunc0,
                           UnbFrame& f) {
    if (!views) { gsr_set_error("the view table is required"); return GSR_E_INVALID; }
    if (n_views <= 0) { gsr_set_error("no views (n_views = %d)", n_views); return GSR_E_INVALID; }
    if (!center_host) { gsr_set_error("center is required"); return GSR_E_INVALID; }
    if (!(radius > 0.f) || !isfinite(radius)) { gsr_set_error("radius must be > 0 (got %g)", (double)radius); return GSR_E_INVALID; }
    if (!(trunc0 > 0.f) || !isfinite(trunc0)) { gsr_set_error("trunc must be > 0 (got %g)", (double)trunc0); return GSR_E_INVALID; }
    for (int k = 0; k < 3; ++k) f.center[k] = center_host[k];
    f.radius = radius;
    f.trunc0 = trunc0;
    return GSR_OK;
}

static int unb_check_lattice(double R, int32_t resolution, int32_t crop, UnbLattice& L) {
    if (!(R > 0.0) || !isfinite(R)) { gsr_set_error("R must be > 0 (got %g)", R); return GSR_E_INVALID; }
    if (crop < 2 || resolution < crop || resolution % crop != 0) {
        gsr_set_error("resolution %d must be a positive multiple of crop %d (crop >= 2)", resolution, crop);
        return GSR_E_INVALID;
    }
    const int64_t G = (int64_t)(resolution / crop) * (crop - 1) + 1;
    if (G > (1 << 20)) { gsr_set_error("lattice of %lld points per axis is too large", (long long)G); return GSR_E_INVALID; }
    L.R = R;
    L.G = (int)G;
    L.step = 2.0 * R / (double)(G - 1);
    return GSR_OK;
}

static unsigned unb_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < UNB_MAX_GRID ? b : UNB_MAX_GRID);
}

extern "C" int32_t gsr_unb_lattice_size(int32_t resolution, int32_t crop, int32_t* G, int32_t* blocks_per_axis) {
    UnbLattice L;
    const int rc = unb_check_lattice(1.0, resolution, crop, L);
    if (rc != GSR_OK) return rc;
    if (G) *G = L.G;
    if (blocks_per_axis) *blocks_per_axis = (L.G + TSDF_B - 1) / TSDF_B;
    return GSR_OK;
}

extern "C" int32_t gsr_unb_points(const GsrUnbView* views, int32_t n_views, const float* points, int64_t n,
                                  const float* center_host, float radius, float trunc, int32_t contracted, float* tsdf_out,
                                  float* rgb_out, gsr_stream_t stream_) {
    UnbFrame f;
    const int rc = unb_check_frame(views, n_views, center_host, radius, trunc, f);
    if (rc != GSR_OK) return rc;
    if (n < 0) { gsr_set_error("negative point count"); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!points || !tsdf_out) { gsr_set_error("points and tsdf_out are required"); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (rgb_out)
        hipLaunchKernelGGL(unb_points_kernel<true>, dim3(unb_grid(n)), dim3(256), 0, s, views, n_views, f, points, n, contracted,
                           tsdf_out, rgb_out);
    else
        hipLaunchKernelGGL(unb_points_kernel<false>, dim3(unb_grid(n)), dim3(256), 0, s, views, n_views, f, points, n, contracted,
                           tsdf_out, rgb_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_unb_lattice_box(const GsrUnbView* views, int32_t n_views, double R, int32_t resolution, int32_t crop,
                                       const int32_t* lo_host, const int32_t* dims_host, const float* center_host, float radius,
                                       float trunc, float* out, gsr_stream_t stream_) {
    UnbFrame f;
    UnbLattice L;
    int rc = unb_check_frame(views, n_views, center_host, radius, trunc, f);
    if (rc != GSR_OK) return rc;
    rc = unb_check_lattice(R, resolution, crop, L);
    if (rc != GSR_OK) return rc;
    if (!lo_host || !dims_host || !out) { gsr_set_error("lo, dims and out are required"); return GSR_E_INVALID; }
    UnbBox b;
    for (int k = 0; k < 3; ++k) {
        if (dims_host[k] <= 0) { gsr_set_error("empty box (dims[%d] = %d)", k, dims_host[k]); return GSR_E_INVALID; }
        if (lo_host[k] < 0 || (int64_t)lo_host[k] + dims_host[k] > L.G) {
            gsr_set_error("box [%d, %lld) leaves the lattice of %d points on axis %d", lo_host[k],
                          (long long)lo_host[k] + dims_host[k], L.G, k);
            return GSR_E_INVALID;
        }
        b.lo[k] = lo_host[k];
        b.dim[k] = dims_host[k];
    }
    const int64_t n = (int64_t)b.dim[0] * b.dim[1] * b.dim[2];
    hipLaunchKernelGGL(unb_box_kernel, dim3(unb_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream_), views, n_views, f, L, b,
                       out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// the volume of the block passes: block AABB [0, ceil(G / 16))^3
static int unb_check_volume(const GsrTsdfVolume* vol, const UnbLattice& L, TsdfGrid& g, int64_t& n, TsdfWs& ws) {
    int rc = tsdf_check_volume(vol, g, n);
    if (rc != GSR_OK) return rc;
    const int nb = (L.G + TSDF_B - 1) / TSDF_B;
    for (int k = 0; k < 3; ++k) {
        if (g.lo[k] != 0 || g.dim[k] != nb) {
            gsr_set_error("the volume's block AABB must be [0, %d)^3 for a lattice of %d points", nb, L.G);
            return GSR_E_INVALID;
        }
    }
    if (!vol->block_index || !vol->workspace) { gsr_set_error("block_index / workspace missing"); return GSR_E_INVALID; }
    ws = tsdf_ws_layout(vol->workspace, n);
    if (vol->workspace_bytes < ws.bytes) {
        gsr_set_error("workspace too small (%zu < %zu bytes)", vol->workspace_bytes, ws.bytes);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

extern "C" int32_t gsr_unb_block_flags(const GsrUnbView* views, int32_t n_views, double R, int32_t resolution, int32_t crop,
                                       const float* center_host, float radius, float trunc, uint8_t* flags,
                                       gsr_stream_t stream_) {
    UnbFrame f;
    UnbLattice L;
    int rc = unb_check_frame(views, n_views, center_host, radius, trunc, f);
    if (rc != GSR_OK) return rc;
    rc = unb_check_lattice(R, resolution, crop, L);
    if (rc != GSR_OK) return rc;
    if (!flags) { gsr_set_error("flags is required"); return GSR_E_INVALID; }
    TsdfGrid g{};
    const int nb = (L.G + TSDF_B - 1) / TSDF_B;
    g.dim[0] = g.dim[1] = g.dim[2] = nb;
    g.vs = 1.f;
    const int64_t n = (int64_t)nb * nb * nb;
    if (n > GSR_TSDF_BLOCK_CAP) { gsr_set_error("lattice of %d^3 blocks exceeds the block cap", nb); return GSR_E_UNSUPPORTED; }
    hipLaunchKernelGGL(unb_flags_kernel, dim3((unsigned)n), dim3(TSDF_THREADS), 0, static_cast<hipStream_t>(stream_), views,
                       n_views, f, L, g, flags);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_unb_alloc(GsrTsdfVolume* vol, int32_t resolution, int32_t crop, const uint8_t* flags,
                                 gsr_stream_t stream_) {
    UnbLattice L;
    int rc = unb_check_lattice(1.0, resolution, crop, L);
    if (rc != GSR_OK) return rc;
    TsdfGrid g;
    int64_t n = 0;
    TsdfWs ws;
    rc = unb_check_volume(vol, L, g, n, ws);
    if (rc != GSR_OK) return rc;
    if (!flags) { gsr_set_error("flags is required"); return GSR_E_INVALID; }
    unsigned long long* host = gsr_pinned_words(1);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const unsigned nbk = (unsigned)((n + 255) / 256);
    const unsigned tiles = (unsigned)scan_tiles(n);
    hipLaunchKernelGGL(unb_select_kernel, dim3(nbk), dim3(256), 0, s, g, n, flags, ws.flags);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(unb_scan_reduce_kernel, dim3(tiles), dim3(SCAN_BLOCK), 0, s, ws.flags, ws.partial, n);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(unb_scan_apply_kernel, dim3(tiles), dim3(SCAN_BLOCK), 0, s, ws.flags, ws.partial, ws.scans, n);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(unb_assign_kernel, dim3(nbk), dim3(256), 0, s, n, ws.flags, ws.scans, vol->block_index, ws.slot_block);
    GSR_LAUNCH_CHECK();
    // the one read-back of the extraction's allocation: the caller sizes the pool from it
    GSR_HIP_CHECK(hipMemcpyAsync(host, ws.scans + n, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    vol->n_alloc = *reinterpret_cast<const uint32_t*>(host);
    return GSR_OK;
}

extern "C" int32_t gsr_unb_fill(const GsrTsdfVolume* vol, const GsrUnbView* views, int32_t n_views, double R, int32_t resolution,
                                int32_t crop, const float* center_host, float radius, float trunc, gsr_stream_t stream_) {
    UnbFrame f;
    UnbLattice L;
    int rc = unb_check_frame(views, n_views, center_host, radius, trunc, f);
    if (rc != GSR_OK) return rc;
    rc = unb_check_lattice(R, resolution, crop, L);
    if (rc != GSR_OK) return rc;
    TsdfGrid g;
    int64_t n = 0;
    TsdfWs ws;
    rc = unb_check_volume(vol, L, g, n, ws);
    if (rc != GSR_OK) return rc;
    if (vol->n_alloc < 0 || vol->n_alloc > n) { gsr_set_error("n_alloc %lld out of range", (long long)vol->n_alloc); return GSR_E_INVALID; }
    if (vol->n_alloc == 0) return GSR_OK;
    if (!vol->pool || vol->pool_blocks < vol->n_alloc) {
        gsr_set_error("pool of %lld blocks cannot hold the %lld allocated ones", (long long)vol->pool_blocks,
                      (long long)vol->n_alloc);
        return GSR_E_INVALID;
    }
    hipLaunchKernelGGL(unb_fill_kernel, dim3((unsigned)vol->n_alloc), dim3(TSDF_THREADS), 0, static_cast<hipStream_t>(stream_),
                       views, n_views, f, L, g, ws.slot_block, vol->pool, vol->pool_blocks * TSDF_BV);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_unb_finish(float* verts, int64_t n, double R, int32_t resolution, int32_t crop, const float* center_host,
                                  float radius, float max_range, gsr_stream_t stream_) {
    UnbLattice L;
    const int rc = unb_check_lattice(R, resolution, crop, L);
    if (rc != GSR_OK) return rc;
    if (!center_host) { gsr_set_error("center is required"); return GSR_E_INVALID; }
    if (!(radius > 0.f) || !isfinite(radius)) { gsr_set_error("radius must be > 0 (got %g)", (double)radius); return GSR_E_INVALID; }
    if (!(max_range > 0.f)) { gsr_set_error("max_range must be > 0 (got %g)", (double)max_range); return GSR_E_INVALID; }
    if (n < 0) { gsr_set_error("negative vertex count"); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!verts) { gsr_set_error("verts is required"); return GSR_E_INVALID; }
    UnbFrame f;
    for (int k = 0; k < 3; ++k) f.center[k] = center_host[k];
    f.radius = radius;
    f.trunc0 = 0.f;
    hipLaunchKernelGGL(unb_finish_kernel, dim3(unb_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream_), verts, n, f, L,
                       max_range);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
