// Mesh culling by view masks on the device (include/gsr.h, "mesh evaluation: culling by view masks"): what the reference's
// scripts/eval_dtu/evaluate_single_scene.py: cull_scan does with skimage, grid_sample and trimesh, restated as the rules
// CULL_MASK_BINARISE ... CULL_TO_WORLD of the header.
//
//   mc_hdist_kernel      (dilation, pass 1) one workgroup per image row: per pixel the horizontal distance to the nearest set
//                        pixel of that row, capped at r + 1, one byte.  Every thread scans its own piece of the row; the
//                        "last set pixel before my piece" / "first set pixel after it" travel through LDS (max / min scan)
//   mc_dilate_kernel     (dilation, pass 2) per pixel: is there a row dy in [-r, r] with hdist[y + dy][x] <= w(dy), w(dy) =
//                        floor(sqrt(r^2 - dy^2)) from an integer host table: exactly the disk dx^2 + dy^2 <= r^2.  One byte or,
//                        where the row pitch allows, four bytes per lane
//   mc_vote_kernel       one thread per vertex over the views in index order, out at the first view that removes it; the
//                        matrices are read with wave-uniform loads; each thread owns its vertex's mark
//   mc_mark_tris_kernel  emit[t] = all three vertices kept (degenerate triangles stay)
//   (scans)              vertex and triangle offsets (binning.hip's scan); ONE synchronisation reads the two totals
//   (emission)           vertex rows through compact.hip (or mc_emit_verts_kernel with v s + t), colours through compact.hip,
//                        triangles through mesh_emit.h, the kernel the cluster filter uses
//
// The dilation is integer work and the vote one fixed fp32 expression per (vertex, view): the same bytes on every run,
// whatever the launch shape.
#include "gsr_common.h"
#include "mesh_emit.h"

#define MC_MAX_RADIUS 127            // hdist is a byte capped at r + 1

struct McSpans { uint8_t w[2 * MC_MAX_RADIUS + 2]; };     // w[dy + r], dy in [-r, r]

// ---------------------------------------------------------------- dilation
__global__ void __launch_bounds__(256) mc_hdist_kernel(const uint8_t* __restrict__ masks, int W, int cap,
                                                       uint8_t* __restrict__ hdist) {
    __shared__ int s_last[256], s_next[256];            // pixel positions; -1 / INT_MAX: no set pixel on that side
    const long long NONE_L = -(1LL << 40), NONE_R = 1LL << 40;
    const int t = threadIdx.x;
    const uint8_t* src = masks + (long long)blockIdx.x * W;
    uint8_t* dst = hdist + (long long)blockIdx.x * W;
    const long long S = ((long long)W + 255) / 256;
    const long long x0 = min(t * S, (long long)W), x1 = min(x0 + S, (long long)W);
    long long last = NONE_L, first = NONE_R;
    for (long long x = x0; x < x1; ++x)
        if (src[x]) {                                   // CULL_MASK_BINARISE: non-zero is set
            if (first == NONE_R) first = x;
            last = x;
        }
    s_last[t] = last == NONE_L ? -1 : (int)last;
    s_next[t] = first == NONE_R ? 0x7fffffff : (int)first;          // x <= W - 1 <= 2^31 - 2: never a position
    __syncthreads();
    // inclusive max scan of `last` towards higher threads, inclusive min scan of `first` towards lower threads
    for (int d = 1; d < 256; d <<= 1) {
        const int a = t >= d ? s_last[t - d] : -1;
        const int b = t + d < 256 ? s_next[t + d] : 0x7fffffff;
        __syncthreads();
        s_last[t] = max(s_last[t], a);
        s_next[t] = min(s_next[t], b);
        __syncthreads();
    }
    long long cur = t > 0 && s_last[t - 1] >= 0 ? s_last[t - 1] : NONE_L;
    for (long long x = x0; x < x1; ++x) {
        if (src[x]) cur = x;
        dst[x] = (uint8_t)min(x - cur, (long long)cap);
    }
    cur = t < 255 && s_next[t + 1] != 0x7fffffff ? s_next[t + 1] : NONE_R;
    for (long long x = x1 - 1; x >= x0; --x) {
        if (src[x]) cur = x;
        const int d = (int)min(cur - x, (long long)cap);
        if (d < (int)dst[x]) dst[x] = (uint8_t)d;      // this thread wrote dst[x] itself
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) mc_dilate_kernel(const uint8_t* __restrict__ hdist, long long n_rows, int H, int W,
                                                        int r, McSpans sp, uint8_t* __restrict__ out) {
    const int wq = W / VEC;                             // VEC == 4 only when W % 4 == 0
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * wq) return;
    const long long row = i / wq;                       // image * H + y
    const int x = (int)(i - row * wq) * VEC;
    const int y = (int)(row % H);
    const int lo = max(-r, -y), hi = min(r, H - 1 - y); // rows outside the image count as unset
    const uint8_t* p = hdist + row * W + x;
    if (VEC == 1) {
        uint8_t hit = 0;
        for (int dy = lo; dy <= hi && !hit; ++dy) hit = p[(long long)dy * W] <= sp.w[dy + r];
        out[row * W + x] = hit;
    } else {
        uint32_t hit = 0;
        for (int dy = lo; dy <= hi && hit != 0x01010101u; ++dy) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(p + (long long)dy * W);
            const uint32_t w = sp.w[dy + r];
#pragma unroll
            for (int k = 0; k < 4; ++k) hit |= (uint32_t)(((v >> (8 * k)) & 0xffu) <= w) << (8 * k);
        }
        *reinterpret_cast<uint32_t*>(out + row * W + x) = hit;
    }
}

extern "C" size_t gsr_mask_dilate_workspace_bytes(int32_t n, int32_t H, int32_t W) {
    const size_t px = size_t(n > 0 ? n : 0) * size_t(H > 0 ? H : 0) * size_t(W > 0 ? W : 0);
    return gsr_align(px > 0 ? px : 1);
}

extern "C" int32_t gsr_mask_dilate_disk(const uint8_t* masks, int32_t n, int32_t H, int32_t W, int32_t radius, uint8_t* out,
                                        void* ws, size_t ws_bytes, gsr_stream_t stream_) {
    if (n < 0) { gsr_set_error("n must be >= 0 (got %d)", n); return GSR_E_INVALID; }
    if (H < 1) { gsr_set_error("H must be >= 1 (got %d)", H); return GSR_E_INVALID; }
    if (W < 1) { gsr_set_error("W must be >= 1 (got %d)", W); return GSR_E_INVALID; }
    if (radius < 0) { gsr_set_error("radius must be >= 0 (got %d)", radius); return GSR_E_INVALID; }
    if (radius > MC_MAX_RADIUS) {
        gsr_set_error("radius %d exceeds %d (the row distances are bytes)", radius, MC_MAX_RADIUS);
        return GSR_E_UNSUPPORTED;
    }
    const long long n_rows = (long long)n * H;
    if (n_rows > 0x7fffffffLL) {
        gsr_set_error("n * H = %lld image rows exceed the 2^31 - 1 workgroups of one launch", n_rows);
        return GSR_E_UNSUPPORTED;
    }
    if ((n_rows * W + 255) / 256 > 0x7fffffffLL) {          // pass 2 at one pixel per thread; four per thread needs fewer
        gsr_set_error("n * H * W = %lld pixels exceed one launch", n_rows * W);
        return GSR_E_UNSUPPORTED;
    }
    if (n == 0) return GSR_OK;
    if (!masks) { gsr_set_error("masks is null with n %d", n); return GSR_E_INVALID; }
    if (!out) { gsr_set_error("out is null with n %d", n); return GSR_E_INVALID; }
    const size_t need = gsr_mask_dilate_workspace_bytes(n, H, W);
    if (!ws || ws_bytes < need) {
        gsr_set_error("ws_bytes: mask dilation workspace too small (%zu < %zu bytes)", ws_bytes, need);
        return GSR_E_INVALID;
    }
    // CULL_DISK: w(dy) is the largest integer with w^2 <= r^2 - dy^2, found with integers only
    McSpans sp{};
    for (int dy = -radius; dy <= radius; ++dy) {
        const int rest = radius * radius - dy * dy;
        int w = 0;
        while ((w + 1) * (w + 1) <= rest) ++w;
        sp.w[dy + radius] = (uint8_t)w;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    uint8_t* hdist = static_cast<uint8_t*>(ws);
    hipLaunchKernelGGL(mc_hdist_kernel, dim3((unsigned)n_rows), dim3(256), 0, s, masks, W, radius + 1, hdist);
    GSR_LAUNCH_CHECK();
    const bool wide = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(hdist) | reinterpret_cast<uintptr_t>(out)) & 3) == 0;
    const long long blocks = (n_rows * (wide ? W / 4 : W) + 255) / 256;
    if (wide)
        hipLaunchKernelGGL(mc_dilate_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, hdist, n_rows, H, W, radius, sp, out);
    else
        hipLaunchKernelGGL(mc_dilate_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, hdist, n_rows, H, W, radius, sp, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- vote, marks, scans
struct McWs {
    uint8_t* keep;       // [V]
    uint8_t* emit;       // [F]
    uint32_t* vert_off;  // [V + 1]
    uint32_t* tri_off;   // [F + 1]
    void* scan_ws;
    float* proj;         // [n_views, 12]: last, so that the emit call (which knows no view count) sees the same layout
    size_t bytes_emit;   // up to and without proj
    size_t bytes;
};

static McWs mc_layout(void* base, int64_t F, int64_t V, int32_t n_views) {
    McWs w{};
    GsrWsCursor c(base);
    const size_t f = size_t(F > 0 ? F : 1), v = size_t(V > 0 ? V : 1);
    w.keep = c.take<uint8_t>(v);
    w.emit = c.take<uint8_t>(f);
    w.vert_off = c.take<uint32_t>((v + 1) * 4);
    w.tri_off = c.take<uint32_t>((f + 1) * 4);
    w.scan_ws = c.take(gsr_scan_workspace_bytes((int64_t)(v > f ? v : f)));
    w.bytes_emit = c.off;
    w.proj = c.take<float>(size_t(n_views > 0 ? n_views : 1) * 12 * 4);
    w.bytes = c.off;
    return w;
}

// CULL_PROJECT, CULL_SAMPLE, CULL_VOTE.  `proj + 12 * i` is the same address in every lane: scalar loads.
__global__ void __launch_bounds__(256) mc_vote_kernel(const float* __restrict__ verts, int64_t V,
                                                      const uint8_t* __restrict__ dilated, int n_views, int H, int W,
                                                      float wn1, float hn1, const float* __restrict__ proj,
                                                      const uint8_t* prior, uint8_t* __restrict__ keep, uint8_t* keep_out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    bool kept = prior ? prior[v] != 0 : true;
    const float x = verts[3 * v], y = verts[3 * v + 1], z = verts[3 * v + 2];
    const float w1 = (float)(W - 1), h1 = (float)(H - 1);
    for (int i = 0; i < n_views && kept; ++i) {
        const float* m = proj + 12 * i;
        const float px = fmaf(m[2], z, fmaf(m[1], y, fmaf(m[0], x, m[3])));
        const float py = fmaf(m[6], z, fmaf(m[5], y, fmaf(m[4], x, m[7])));
        const float pz = fmaf(m[10], z, fmaf(m[9], y, fmaf(m[8], x, m[11])));
        const float den = pz + 1e-6f;
        const float gx = (px / den / wn1 - 0.5f) * 2.0f;
        const float gy = (py / den / hn1 - 0.5f) * 2.0f;
        const bool valid = gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f;      // false for NaN
        if (!valid) continue;                                                       // kept by this view
        const float fx = nearbyintf((gx + 1.0f) / 2.0f * w1), fy = nearbyintf((gy + 1.0f) / 2.0f * h1);
        uint8_t sample = 0;
        if (fx >= 0.0f && fx <= w1 && fy >= 0.0f && fy <= h1)
            sample = dilated[((int64_t)i * H + (int64_t)fy) * W + (int64_t)fx];
        kept = sample != 0;
    }
    keep[v] = kept;
    if (keep_out) keep_out[v] = kept;
}

// CULL_COMPACT: a triangle stays when its three vertices stay; a degenerate one is a triangle like any other
__global__ void __launch_bounds__(256) mc_mark_tris_kernel(const int32_t* __restrict__ tris, int64_t F,
                                                           const uint8_t* __restrict__ keep, uint8_t* __restrict__ emit) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F) return;
    emit[t] = keep[tris[3 * t]] && keep[tris[3 * t + 1]] && keep[tris[3 * t + 2]];
}

// CULL_TO_WORLD: one fmaf per component
__global__ void __launch_bounds__(256) mc_emit_verts_kernel(const float* __restrict__ verts, int64_t V,
                                                            const uint8_t* __restrict__ keep, const uint32_t* __restrict__ off,
                                                            float s, float tx, float ty, float tz, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * V) return;
    const int64_t v = i / 3;
    if (!keep[v]) return;
    const int k = (int)(i - 3 * v);
    out[3 * (int64_t)off[v] + k] = fmaf(verts[i], s, k == 0 ? tx : k == 1 ? ty : tz);
}

extern "C" size_t gsr_mesh_cull_workspace_bytes(int64_t n_tris, int64_t n_verts, int32_t n_views) {
    return mc_layout(nullptr, n_tris, n_verts, n_views).bytes;
}

extern "C" int32_t gsr_mesh_cull_count(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts,
                                       const uint8_t* dilated, int32_t n_views, int32_t H, int32_t W, int32_t Wn, int32_t Hn,
                                       const float* proj_host, void* ws, size_t ws_bytes, uint8_t* vertex_keep,
                                       int64_t* n_verts_out, int64_t* n_tris_out, gsr_stream_t stream_) {
    if (!n_verts_out || !n_tris_out) { gsr_set_error("n_verts_out / n_tris_out are required"); return GSR_E_INVALID; }
    *n_verts_out = *n_tris_out = 0;
    int rc = gsr_check_mesh_counts(n_tris, n_verts);
    if (rc != GSR_OK) return rc;
    if (n_views < 0) { gsr_set_error("n_views must be >= 0 (got %d)", n_views); return GSR_E_INVALID; }
    if (H < 1) { gsr_set_error("H must be >= 1 (got %d)", H); return GSR_E_INVALID; }
    if (W < 1) { gsr_set_error("W must be >= 1 (got %d)", W); return GSR_E_INVALID; }
    if (Wn < 1) { gsr_set_error("Wn must be >= 1 (got %d)", Wn); return GSR_E_INVALID; }
    if (Hn < 1) { gsr_set_error("Hn must be >= 1 (got %d)", Hn); return GSR_E_INVALID; }
    if (n_verts == 0) {
        if (n_tris > 0) { gsr_set_error("n_verts is 0 with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
        return GSR_OK;
    }
    if (!verts) { gsr_set_error("verts is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    if (n_tris > 0 && !tris) { gsr_set_error("tris is null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    if (n_views > 0 && !dilated) { gsr_set_error("dilated is null with n_views %d", n_views); return GSR_E_INVALID; }
    if (n_views > 0 && !proj_host) { gsr_set_error("proj_host is null with n_views %d", n_views); return GSR_E_INVALID; }
    const McWs w = mc_layout(ws, n_tris, n_verts, n_views);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh cull workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    unsigned long long* host = gsr_pinned_words(2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int64_t F = n_tris, V = n_verts;
    if (n_views > 0) GSR_HIP_CHECK(hipMemcpyAsync(w.proj, proj_host, size_t(n_views) * 48, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(mc_vote_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, verts, V, dilated, n_views, H, W,
                       (float)(Wn - 1), (float)(Hn - 1), w.proj, vertex_keep, w.keep, vertex_keep);
    GSR_LAUNCH_CHECK();
    rc = gsr_exclusive_scan_u8(w.keep, w.vert_off, V, w.scan_ws, s);
    if (rc != GSR_OK) return rc;
    uint32_t* h = reinterpret_cast<uint32_t*>(host);
    h[1] = 0;
    if (F > 0) {
        hipLaunchKernelGGL(mc_mark_tris_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, tris, F, w.keep, w.emit);
        GSR_LAUNCH_CHECK();
        rc = gsr_exclusive_scan_u8(w.emit, w.tri_off, F, w.scan_ws, s);   // (same stream: the first scan is done with scan_ws)
        if (rc != GSR_OK) return rc;
        GSR_HIP_CHECK(hipMemcpyAsync(h + 1, w.tri_off + F, 4, hipMemcpyDeviceToHost, s));
    }
    // the one synchronisation (as gsr_mesh_filter_count's): the two totals size the caller's output buffers
    GSR_HIP_CHECK(hipMemcpyAsync(h, w.vert_off + V, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    *n_verts_out = (int64_t)h[0];
    *n_tris_out = (int64_t)h[1];
    return GSR_OK;
}

extern "C" int32_t gsr_mesh_cull_emit(const float* verts, const float* colors, const int32_t* tris, int64_t n_tris,
                                      int64_t n_verts, const float* scale_offset_host, void* ws, size_t ws_bytes,
                                      float* verts_out, float* colors_out, int32_t* tris_out, gsr_stream_t stream_) {
    int rc = gsr_check_mesh_counts(n_tris, n_verts);
    if (rc != GSR_OK) return rc;
    if (n_verts == 0) {
        if (n_tris > 0) { gsr_set_error("n_verts is 0 with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
        return GSR_OK;
    }
    if (!verts) { gsr_set_error("verts is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    if (!verts_out) { gsr_set_error("verts_out is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    if (colors && !colors_out) { gsr_set_error("colors_out is null with colors given"); return GSR_E_INVALID; }
    if (n_tris > 0 && !tris) { gsr_set_error("tris is null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    if (n_tris > 0 && !tris_out) { gsr_set_error("tris_out is null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    const McWs w = mc_layout(ws, n_tris, n_verts, 0);
    if (!ws || ws_bytes < w.bytes_emit) {
        gsr_set_error("ws_bytes: mesh cull workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes_emit);
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const void* src[2];
    void* dst[2];
    const int32_t row_bytes[2] = {12, 12};
    int count = 0;
    if (scale_offset_host) {
        hipLaunchKernelGGL(mc_emit_verts_kernel, dim3((unsigned)((3 * n_verts + 255) / 256)), dim3(256), 0, s, verts, n_verts,
                           w.keep, w.vert_off, scale_offset_host[0], scale_offset_host[1], scale_offset_host[2],
                           scale_offset_host[3], verts_out);
        GSR_LAUNCH_CHECK();
    } else {
        src[count] = verts; dst[count++] = verts_out;
    }
    if (colors) { src[count] = colors; dst[count++] = colors_out; }
    rc = gsr_compact_apply(count, src, dst, row_bytes, n_verts, w.keep, w.vert_off, stream_);
    if (rc != GSR_OK) return rc;
    if (n_tris > 0) {
        hipLaunchKernelGGL(mesh_emit_tris_kernel, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, s, tris, n_tris, w.emit,
                           w.tri_off, w.vert_off, tris_out);
        GSR_LAUNCH_CHECK();
    }
    return GSR_OK;
}
