// Mesh culling by visibility on the device (include/gsr.h, "mesh evaluation: culling by visibility"): what the reference's
// scripts/eval_tnt/cull_mesh.py does with pyrender (the mesh's own depth from every camera), grid_sample and trimesh,
// restated as the rules VIS_CAMERA ... VIS_COMPACT of the header.
//
//   mv_raster_small_kernel  one thread per (triangle, view of the call).  Transforms its three vertices (VIS_CAMERA; the
//                           same expression for a vertex whichever triangle asks, so no camera-space copy of the mesh is
//                           kept: it would cost 12 bytes written and 36 gathered per pair where the world-space rows are
//                           36 gathered bytes shared by all views), drops what is wholly nearer than `near`, non-finite or
//                           has an empty pixel box, loops over a box of at most MV_SMALL x MV_SMALL pixels itself and
//                           appends the other pairs to a work list with ONE atomic per wave
//   mv_raster_large_kernel  a fixed grid of workgroups strides over the work list (its length is read on the device);
//                           the 256 lanes of a workgroup cover the pixels of one pair's box
//   mv_resolve_kernel       the images start as 0xffffffff; what no triangle lowered becomes 0.0
//   mv_vote_kernel          one thread per vertex over the views in index order (VIS_PROJECT, VIS_SAMPLE, VIS_VOTE); the
//                           matrices are kernel arguments, i.e. wave-uniform loads; stops at min_views
//   mv_keep_kernel, mv_mark_kernel   keep[v] = count >= min_views; emit[t] = three kept vertices, used[v] for those
//   (scans, emission)       as the cluster filter: binning.hip's scan twice, ONE synchronisation for the two totals,
//                           rows through compact.hip, triangles through mesh_emit.h
//
// Depth is stored with atomicMin on the bit pattern of a positive float: the minimum does not depend on the order, so the
// images are the same bits on every run, whichever path drew a triangle and in whatever order the triangles come.
#include "gsr_common.h"
#include "mesh_emit.h"

#define MV_SMALL 8                  // boxes up to 8 x 8 pixels are looped over by the thread that found them
#define MV_LARGE_BLOCKS 2048        // fixed grid of the large path: 8 workgroups per CU
#define MV_EMPTY 0xffffffffu        // above every float's bit pattern that VIS_RANGE lets through
#define MV_VOTE_VIEWS 64            // matrices per vote launch (3 KB of kernel arguments)

struct MvIntr { float fx, fy, cx, cy; };
struct MvCams { float m[MV_VOTE_VIEWS * 12]; };

// One triangle as a view sees it: the three edge vectors of VIS_COVER (sign folded in), the plane of VIS_DEPTH, the box.
struct MvTri {
    float c0[3], c1[3], c2[3];
    float n[3], np0;
    int x0, x1, y0, y1;             // inclusive pixel box; x0 > x1: nothing to draw
};

// VIS_CAMERA
__device__ __forceinline__ void mv_to_camera(const float* __restrict__ m, const float* __restrict__ v, float* p) {
    const float x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = fmaf(m[4 * k + 2], z, fmaf(m[4 * k + 1], y, fmaf(m[4 * k], x, m[4 * k + 3])));
}

// a x b with every product and difference rounded on its own (never contracted): exactly antisymmetric, exactly 0 for a == b
__device__ __forceinline__ void mv_cross(const float* a, const float* b, float* c) {
    c[0] = __fsub_rn(__fmul_rn(a[1], b[2]), __fmul_rn(a[2], b[1]));
    c[1] = __fsub_rn(__fmul_rn(a[2], b[0]), __fmul_rn(a[0], b[2]));
    c[2] = __fsub_rn(__fmul_rn(a[0], b[1]), __fmul_rn(a[1], b[0]));
}

// VIS_COVER's edge vector of the directed edge a -> b: the cross product is formed from the endpoint with the smaller vertex
// index to the other one and negated when that reverses the edge, so the two triangles of an edge see e and -e exactly
__device__ __forceinline__ void mv_edge(const float* pa, int ia, const float* pb, int ib, float* c) {
    if (ia <= ib) {
        mv_cross(pa, pb, c);
    } else {
        mv_cross(pb, pa, c);
        c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2];
    }
}

__device__ __forceinline__ float mv_dot_ray(const float* c, float dx, float dy) { return fmaf(c[0], dx, fmaf(c[1], dy, c[2])); }

// Sets up triangle t for the view with matrix m.  False: the triangle draws nothing in this view.
__device__ __forceinline__ bool mv_setup(const float* __restrict__ verts, const int32_t* __restrict__ tris, int64_t t, int64_t V,
                                         const float* __restrict__ m, MvIntr k, int H, int W, float near, MvTri& T) {
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if ((uint64_t)i0 >= (uint64_t)V || (uint64_t)i1 >= (uint64_t)V || (uint64_t)i2 >= (uint64_t)V) return false;
    float p0[3], p1[3], p2[3];
    mv_to_camera(m, verts + 3 * (int64_t)i0, p0);
    mv_to_camera(m, verts + 3 * (int64_t)i1, p1);
    mv_to_camera(m, verts + 3 * (int64_t)i2, p2);
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) sum += (fabsf(p0[j]) + fabsf(p1[j]) + fabsf(p2[j])) * 0.0625f;   // finite inputs cannot overflow it
    if (!(sum <= 3.0e38f)) return false;                            // VIS_COVER: a non-finite vertex draws nothing
    if (p0[2] < near && p1[2] < near && p2[2] < near) return false;  // a hit lies between the vertices' depths
    if (p0[2] >= near && p1[2] >= near && p2[2] >= near) {
        // VIS_COVER's guard: pixel centres within one pixel of the projected bounding box
        const float u0 = fmaf(k.fx, p0[0] / p0[2], k.cx), u1 = fmaf(k.fx, p1[0] / p1[2], k.cx), u2 = fmaf(k.fx, p2[0] / p2[2], k.cx);
        const float v0 = fmaf(k.fy, p0[1] / p0[2], k.cy), v1 = fmaf(k.fy, p1[1] / p1[2], k.cy), v2 = fmaf(k.fy, p2[1] / p2[2], k.cy);
        const float ulo = fminf(u0, fminf(u1, u2)), uhi = fmaxf(u0, fmaxf(u1, u2));
        const float vlo = fminf(v0, fminf(v1, v2)), vhi = fmaxf(v0, fmaxf(v1, v2));
        // umin - 1 <= i + 0.5 <= umax + 1, clamped to the image while still a float (the projections may overflow an int)
        T.x0 = (int)fminf(fmaxf(ceilf(ulo - 1.5f), 0.0f), (float)W);
        T.x1 = (int)fminf(fmaxf(floorf(uhi + 0.5f), -1.0f), (float)(W - 1));
        T.y0 = (int)fminf(fmaxf(ceilf(vlo - 1.5f), 0.0f), (float)H);
        T.y1 = (int)fminf(fmaxf(floorf(vhi + 0.5f), -1.0f), (float)(H - 1));
        if (T.x0 > T.x1 || T.y0 > T.y1) return false;
    } else {                                                        // crosses the near plane: no box, every pixel is asked
        T.x0 = 0; T.x1 = W - 1; T.y0 = 0; T.y1 = H - 1;
    }
    mv_edge(p1, i1, p2, i2, T.c0);
    mv_edge(p2, i2, p0, i0, T.c1);
    mv_edge(p0, i0, p1, i1, T.c2);
    float e1[3], e2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { e1[j] = __fsub_rn(p1[j], p0[j]); e2[j] = __fsub_rn(p2[j], p0[j]); }
    mv_cross(e1, e2, T.n);
    T.np0 = fmaf(T.n[0], p0[0], fmaf(T.n[1], p0[1], __fmul_rn(T.n[2], p0[2])));
    return true;
}

// VIS_RAY (one axis)
__device__ __forceinline__ float mv_ray(int i, float c, float f) { return ((float)i + 0.5f - c) / f; }

// VIS_COVER, VIS_DEPTH, VIS_RANGE at one pixel: lowers the pixel's word when the ray hits inside the range
__device__ __forceinline__ void mv_pixel(const MvTri& T, float dx, float dy, float near, float far, uint32_t* px) {
    const float b0 = mv_dot_ray(T.c0, dx, dy), b1 = mv_dot_ray(T.c1, dx, dy), b2 = mv_dot_ray(T.c2, dx, dy);
    const bool pos = b0 >= 0.0f && b1 >= 0.0f && b2 >= 0.0f, neg = b0 <= 0.0f && b1 <= 0.0f && b2 <= 0.0f;
    if (!(pos || neg) || (pos && neg)) return;                      // pos && neg: all three are zero
    const float nd = mv_dot_ray(T.n, dx, dy);
    if (nd == 0.0f) return;
    const float z = T.np0 / nd;
    if (!(z >= near && z <= far)) return;                           // false for NaN
    const uint32_t bits = __float_as_uint(z);
    // a stale word is never below the true one (words only go down): skipping on it is safe
    if (bits < *px) atomicMin(px, bits);
}

__global__ void __launch_bounds__(256) mv_raster_small_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                              int64_t F, int64_t V, const float* __restrict__ w2c, int n_views,
                                                              int H, int W, MvIntr k, float near, float far,
                                                              uint32_t* depth, uint32_t* __restrict__ list,
                                                              uint32_t* __restrict__ list_count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool large = false;
    if (i < F * n_views) {
        const int view = (int)((uint32_t)i / (uint32_t)F);             // F * n_views < 2^32
        const int64_t t = i - (int64_t)view * F;
        MvTri T;
        if (mv_setup(verts, tris, t, V, w2c + 12 * view, k, H, W, near, T)) {
            if (T.x1 - T.x0 >= MV_SMALL || T.y1 - T.y0 >= MV_SMALL) {
                large = true;
            } else {
                uint32_t* img = depth + (int64_t)view * H * W;
                for (int y = T.y0; y <= T.y1; ++y) {
                    const float dy = mv_ray(y, k.cy, k.fy);
                    for (int x = T.x0; x <= T.x1; ++x) mv_pixel(T, mv_ray(x, k.cx, k.fx), dy, near, far, img + (int64_t)y * W + x);
                }
            }
        }
    }
    // every lane of the wave is back here: one atomic per wave reserves the list slots of its large pairs
    const unsigned long long m = __ballot(large);
    if (m) {
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(list_count, (uint32_t)__popcll(m));
        base = __shfl(base, leader, 64);
        if (large) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;       // F * n_views < 2^32
    }
}

__global__ void __launch_bounds__(256) mv_raster_large_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                              int64_t F, int64_t V, const float* __restrict__ w2c, int H, int W,
                                                              MvIntr k, float near, float far, uint32_t* depth,
                                                              const uint32_t* __restrict__ list,
                                                              const uint32_t* __restrict__ list_count) {
    const uint32_t n = *list_count;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const uint32_t i = list[e];
        const int view = (int)(i / (uint32_t)F);
        const int64_t t = (int64_t)i - (int64_t)view * F;
        MvTri T;
        if (!mv_setup(verts, tris, t, V, w2c + 12 * view, k, H, W, near, T)) continue;     // (it was set up once already)
        uint32_t* img = depth + (int64_t)view * H * W;
        const int bw = T.x1 - T.x0 + 1;
        const int64_t px = (int64_t)bw * (T.y1 - T.y0 + 1);
        for (int64_t q = threadIdx.x; q < px; q += blockDim.x) {
            const int y = T.y0 + (int)(q / bw), x = T.x0 + (int)(q % bw);
            mv_pixel(T, mv_ray(x, k.cx, k.fx), mv_ray(y, k.cy, k.fy), near, far, img + (int64_t)y * W + x);
        }
    }
}

__global__ void __launch_bounds__(256) mv_resolve_kernel(uint32_t* __restrict__ depth, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && depth[i] == MV_EMPTY) depth[i] = 0u;
}

struct MvDepthWs {
    uint32_t* count;     // [1] length of the list
    float* w2c;          // [n_views, 12]
    uint32_t* list;      // [F * n_views] pair ids view * F + t
    size_t bytes;
};

static MvDepthWs mv_depth_layout(void* base, int64_t F, int32_t n_views) {
    MvDepthWs w{};
    GsrWsCursor c(base);
    const size_t f = size_t(F > 0 ? F : 0), n = size_t(n_views > 0 ? n_views : 0);
    w.count = c.take<uint32_t>(4);
    w.w2c = c.take<float>((n ? n : 1) * 48);
    w.list = c.take<uint32_t>((f * n ? f * n : 1) * 4);
    w.bytes = c.off;
    return w;
}

static int mv_check_image(int32_t n_views, int32_t H, int32_t W) {
    if (n_views < 0) { gsr_set_error("n_views must be >= 0 (got %d)", n_views); return GSR_E_INVALID; }
    if (H < 1) { gsr_set_error("H must be >= 1 (got %d)", H); return GSR_E_INVALID; }
    if (W < 1) { gsr_set_error("W must be >= 1 (got %d)", W); return GSR_E_INVALID; }
    if (H > (1 << 24) || W > (1 << 24)) {
        gsr_set_error("H, W = %d, %d exceed 2^24 (pixel indices are converted to float)", H, W);
        return GSR_E_UNSUPPORTED;
    }
    return GSR_OK;
}

extern "C" size_t gsr_mesh_depth_workspace_bytes(int64_t n_tris, int32_t n_views) {
    return mv_depth_layout(nullptr, n_tris, n_views).bytes;
}

extern "C" int32_t gsr_mesh_depth_render(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts,
                                         const float* w2c_host, int32_t n_views, int32_t H, int32_t W, float fx, float fy,
                                         float cx, float cy, float near, float far, float* depth_out, void* ws, size_t ws_bytes,
                                         gsr_stream_t stream_) {
    int rc = gsr_check_mesh_counts(n_tris, n_verts);
    if (rc != GSR_OK) return rc;
    rc = mv_check_image(n_views, H, W);
    if (rc != GSR_OK) return rc;
    if (!(near > 0.0f)) { gsr_set_error("near must be > 0 (got %g): depths are compared as bit patterns", near); return GSR_E_INVALID; }
    if (!(near < far)) { gsr_set_error("near %g must be below far %g", near, far); return GSR_E_INVALID; }
    if (!(far <= 3.0e38f)) { gsr_set_error("far must be finite (got %g)", far); return GSR_E_INVALID; }
    if (!(fx != 0.0f && fy != 0.0f)) { gsr_set_error("fx, fy must not be 0 (got %g, %g)", fx, fy); return GSR_E_INVALID; }
    if (n_views == 0) return GSR_OK;
    if (!depth_out) { gsr_set_error("depth_out is null with n_views %d", n_views); return GSR_E_INVALID; }
    if (!w2c_host) { gsr_set_error("w2c_host is null with n_views %d", n_views); return GSR_E_INVALID; }
    if (n_tris > 0 && (!verts || !tris)) { gsr_set_error("verts / tris are null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    if (n_tris > 0 && n_verts == 0) { gsr_set_error("n_verts is 0 with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    const int64_t pairs = n_tris * n_views, pixels = (int64_t)n_views * H * W;
    if (pairs > 0xffffffffLL) {
        gsr_set_error("n_tris * n_views = %lld pairs exceed 2^32 - 1: pass fewer views per call", (long long)pairs);
        return GSR_E_UNSUPPORTED;
    }
    if ((pixels + 255) / 256 > 0x7fffffffLL) {
        gsr_set_error("n_views * H * W = %lld pixels exceed one launch: pass fewer views per call", (long long)pixels);
        return GSR_E_UNSUPPORTED;
    }
    const MvDepthWs w = mv_depth_layout(ws, n_tris, n_views);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh depth workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    uint32_t* depth = reinterpret_cast<uint32_t*>(depth_out);
    const MvIntr k{fx, fy, cx, cy};
    GSR_HIP_CHECK(hipMemsetAsync(depth, 0xff, size_t(pixels) * 4, s));
    if (pairs > 0) {
        GSR_HIP_CHECK(hipMemsetAsync(w.count, 0, 4, s));
        GSR_HIP_CHECK(hipMemcpyAsync(w.w2c, w2c_host, size_t(n_views) * 48, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(mv_raster_small_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, verts, tris, n_tris,
                           n_verts, w.w2c, n_views, H, W, k, near, far, depth, w.list, w.count);
        GSR_LAUNCH_CHECK();
        hipLaunchKernelGGL(mv_raster_large_kernel, dim3(MV_LARGE_BLOCKS), dim3(256), 0, s, verts, tris, n_tris, n_verts, w.w2c,
                           H, W, k, near, far, depth, w.list, w.count);
        GSR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mv_resolve_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, depth, pixels);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- vote
// VIS_PROJECT, VIS_SAMPLE, VIS_VOTE.  `cams.m + 12 * i` is a kernel argument at a wave-uniform index: scalar loads.
__global__ void __launch_bounds__(256) mv_vote_kernel(const float* __restrict__ verts, int64_t V, const float* __restrict__ depths,
                                                      int n_views, int H, int W, MvCams cams, MvIntr k, float eps, int min_views,
                                                      int32_t* __restrict__ counts) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    int cnt = counts[v];
    if (cnt >= min_views) return;
    const float w1 = (float)(W - 1), h1 = (float)(H - 1);
    for (int i = 0; i < n_views && cnt < min_views; ++i) {
        float p[3];
        mv_to_camera(cams.m + 12 * i, verts + 3 * v, p);
        const float z = p[2] + 1e-8f;
        const float pu = fmaf(k.fx, p[0], __fmul_rn(k.cx, p[2])) / z, pv = fmaf(k.fy, p[1], __fmul_rn(k.cy, p[2])) / z;
        if (!(pu >= 0.0f && pu <= w1 && pv >= 0.0f && pv <= h1 && z > 0.0f)) continue;      // false for NaN
        const float xf = floorf(pu), yf = floorf(pv);
        const int x0 = (int)xf, y0 = (int)yf;                                                // in [0, W - 1], [0, H - 1]
        const float ax = pu - xf, ay = pv - yf, bx = (xf + 1.0f) - pu, by = (yf + 1.0f) - pv;
        const float* img = depths + ((int64_t)i * H + y0) * W + x0;
        const bool right = x0 + 1 < W, down = y0 + 1 < H;        // a tap outside the image has weight 0 here: left out
        float ds = __fmul_rn(img[0], __fmul_rn(bx, by));
        if (right) ds = fmaf(img[1], __fmul_rn(ax, by), ds);
        if (down) ds = fmaf(img[W], __fmul_rn(bx, ay), ds);
        if (right && down) ds = fmaf(img[(int64_t)W + 1], __fmul_rn(ax, ay), ds);
        cnt += ds > 0.0f ? (z < ds + eps) : 1;
    }
    counts[v] = cnt;
}

extern "C" int32_t gsr_mesh_vis_count(const float* verts, int64_t n_verts, const float* depths, int32_t n_views, int32_t H,
                                      int32_t W, const float* w2c_host, const float* intrinsics, float eps, int32_t min_views,
                                      int32_t* counts_inout, gsr_stream_t stream_) {
    int rc = gsr_check_mesh_counts(0, n_verts);
    if (rc != GSR_OK) return rc;
    rc = mv_check_image(n_views, H, W);
    if (rc != GSR_OK) return rc;
    if (!intrinsics) { gsr_set_error("intrinsics (fx, fy, cx, cy) are required"); return GSR_E_INVALID; }
    if (n_verts == 0 || n_views == 0) return GSR_OK;
    if (!verts) { gsr_set_error("verts is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    if (!counts_inout) { gsr_set_error("counts_inout is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    if (!depths) { gsr_set_error("depths is null with n_views %d", n_views); return GSR_E_INVALID; }
    if (!w2c_host) { gsr_set_error("w2c_host is null with n_views %d", n_views); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const MvIntr k{intrinsics[0], intrinsics[1], intrinsics[2], intrinsics[3]};
    for (int32_t a = 0; a < n_views; a += MV_VOTE_VIEWS) {
        const int32_t nb = n_views - a < MV_VOTE_VIEWS ? n_views - a : MV_VOTE_VIEWS;
        MvCams cams;
        for (int32_t j = 0; j < nb * 12; ++j) cams.m[j] = w2c_host[(size_t)a * 12 + j];
        for (int32_t j = nb * 12; j < MV_VOTE_VIEWS * 12; ++j) cams.m[j] = 0.0f;
        hipLaunchKernelGGL(mv_vote_kernel, dim3((unsigned)((n_verts + 255) / 256)), dim3(256), 0, s, verts, n_verts,
                           depths + (size_t)a * H * W, nb, H, W, cams, k, eps, min_views, counts_inout);
        GSR_LAUNCH_CHECK();
    }
    return GSR_OK;
}

// ---------------------------------------------------------------- marks, scans, emission (VIS_COMPACT)
struct MvWs {
    uint8_t* keep;       // [V] count >= min_views
    uint8_t* used;       // [V] a kept triangle uses the vertex
    uint8_t* emit;       // [F]
    uint32_t* vert_off;  // [V + 1]
    uint32_t* tri_off;   // [F + 1]
    void* scan_ws;
    size_t bytes;
};

static MvWs mv_layout(void* base, int64_t F, int64_t V) {
    MvWs w{};
    GsrWsCursor c(base);
    const size_t f = size_t(F > 0 ? F : 1), v = size_t(V > 0 ? V : 1);
    w.keep = c.take<uint8_t>(v);
    w.used = c.take<uint8_t>(v);
    w.emit = c.take<uint8_t>(f);
    w.vert_off = c.take<uint32_t>((v + 1) * 4);
    w.tri_off = c.take<uint32_t>((f + 1) * 4);
    w.scan_ws = c.take(gsr_scan_workspace_bytes((int64_t)(v > f ? v : f)));
    w.bytes = c.off;
    return w;
}

__global__ void __launch_bounds__(256) mv_keep_kernel(const int32_t* __restrict__ counts, int64_t V, int min_views,
                                                      uint8_t* __restrict__ keep, uint8_t* keep_out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const uint8_t k = counts[v] >= min_views;
    keep[v] = k;
    if (keep_out) keep_out[v] = k;
}

// a triangle with an index outside [0, V) is not emitted (and marks nothing)
__global__ void __launch_bounds__(256) mv_mark_kernel(const int32_t* __restrict__ tris, int64_t F, int64_t V,
                                                      const uint8_t* __restrict__ keep, uint8_t* __restrict__ used,
                                                      uint8_t* __restrict__ emit) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F) return;
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    const bool in = (uint64_t)a < (uint64_t)V && (uint64_t)b < (uint64_t)V && (uint64_t)c < (uint64_t)V;
    const bool e = in && keep[a] && keep[b] && keep[c];
    if (e) used[a] = used[b] = used[c] = 1;         // racing stores of the same byte
    emit[t] = e;
}

extern "C" size_t gsr_mesh_vis_workspace_bytes(int64_t n_tris, int64_t n_verts) { return mv_layout(nullptr, n_tris, n_verts).bytes; }

extern "C" int32_t gsr_mesh_vis_compact_count(const int32_t* tris, int64_t n_tris, int64_t n_verts, const int32_t* counts,
                                              int32_t min_views, void* ws, size_t ws_bytes, uint8_t* vertex_keep,
                                              int64_t* n_verts_out, int64_t* n_tris_out, gsr_stream_t stream_) {
    if (!n_verts_out || !n_tris_out) { gsr_set_error("n_verts_out / n_tris_out are required"); return GSR_E_INVALID; }
    *n_verts_out = *n_tris_out = 0;
    int rc = gsr_check_mesh_counts(n_tris, n_verts);
    if (rc != GSR_OK) return rc;
    if (n_verts == 0) {
        if (n_tris > 0) { gsr_set_error("n_verts is 0 with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
        return GSR_OK;
    }
    if (!counts) { gsr_set_error("counts is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    if (n_tris > 0 && !tris) { gsr_set_error("tris is null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    const MvWs w = mv_layout(ws, n_tris, n_verts);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh visibility workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    unsigned long long* host = gsr_pinned_words(2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int64_t F = n_tris, V = n_verts;
    hipLaunchKernelGGL(mv_keep_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, counts, V, min_views, w.keep, vertex_keep);
    GSR_LAUNCH_CHECK();
    if (F == 0) return GSR_OK;                      // no triangle, so no used vertex: both totals are 0, nothing to read back
    GSR_HIP_CHECK(hipMemsetAsync(w.used, 0, size_t(V), s));
    hipLaunchKernelGGL(mv_mark_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, tris, F, V, w.keep, w.used, w.emit);
    GSR_LAUNCH_CHECK();
    rc = gsr_exclusive_scan_u8(w.used, w.vert_off, V, w.scan_ws, s);
    if (rc != GSR_OK) return rc;
    rc = gsr_exclusive_scan_u8(w.emit, w.tri_off, F, w.scan_ws, s);   // (same stream: the first scan is done with scan_ws)
    if (rc != GSR_OK) return rc;
    // the one synchronisation (as gsr_mesh_filter_count's): the two totals size the caller's output buffers
    uint32_t* h = reinterpret_cast<uint32_t*>(host);
    GSR_HIP_CHECK(hipMemcpyAsync(h, w.vert_off + V, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipMemcpyAsync(h + 1, w.tri_off + F, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    *n_verts_out = (int64_t)h[0];
    *n_tris_out = (int64_t)h[1];
    return GSR_OK;
}

extern "C" int32_t gsr_mesh_vis_emit(const float* verts, const float* colors, const int32_t* tris, int64_t n_tris,
                                     int64_t n_verts, void* ws, size_t ws_bytes, float* verts_out, float* colors_out,
                                     int32_t* tris_out, gsr_stream_t stream_) {
    int rc = gsr_check_mesh_counts(n_tris, n_verts);
    if (rc != GSR_OK) return rc;
    if (n_tris == 0) return GSR_OK;
    if (n_verts == 0) { gsr_set_error("n_verts is 0 with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    if (!verts || !tris) { gsr_set_error("verts and tris are required"); return GSR_E_INVALID; }
    if (!verts_out || !tris_out) { gsr_set_error("verts_out and tris_out are required"); return GSR_E_INVALID; }
    if (colors && !colors_out) { gsr_set_error("colors_out is null with colors given"); return GSR_E_INVALID; }
    const MvWs w = mv_layout(ws, n_tris, n_verts);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh visibility workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    const void* src[2] = {verts, colors};
    void* dst[2] = {verts_out, colors_out};
    const int32_t row_bytes[2] = {12, 12};
    rc = gsr_compact_apply(colors ? 2 : 1, src, dst, row_bytes, n_verts, w.used, w.vert_off, stream_);
    if (rc != GSR_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(mesh_emit_tris_kernel, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, s, tris, n_tris, w.emit,
                       w.tri_off, w.vert_off, tris_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
