// Mesh post-processing on the device (include/gsr.h, "mesh export: triangle clusters and the cluster filter"): what
// gaussmart_amd/mesh.py: post_process_mesh does with numpy + scipy, bit for bit.
//
//   mp_edges_kernel      per (triangle, edge): lo = min, hi = max of the two vertex ids; parent[t] = t
//   (radix sort x 2)     the 3F edge ids ordered by (lo, hi): stable by hi, gather lo, stable by lo (binning.hip's sort)
//   mp_union_kernel      per sorted position with the same (lo, hi) as its successor: lock-free union of the two triangles
//   mp_flatten_kernel    (own launch: the kernel boundary publishes every parent) label[t] = root = smallest triangle of the cluster
//   mp_count_kernel      count[root] += 1, one integer atomic per (wave, distinct root)
//   mp_size_kernel       cluster_size[t] = count[label[t]]
//   mp_rootkey_kernel    sort key count[t] (roots) / 0 (others), number of roots; sorted ascending by the same radix sort
//   mp_threshold_kernel  one thread: max(sorted[F - min(k, n_clusters)], 50) -> a device word
//   mp_mark_kernel       keep_tri, used[v] (before the degenerate test), emit flag keep && !degenerate
//   (scans)              vertex and triangle offsets (binning.hip's scan); ONE synchronisation reads the two totals
//   (compact rows)       vertices and colours in one launch (compact.hip);  mesh_emit_tris_kernel (mesh_emit.h) writes the remapped triangles
//
// Everything is integer work: labels, counts and the output are the same on every run, whatever the schedule.
#include "gsr_common.h"
#include "mesh_emit.h"

#define MP_MIN_CLUSTER 50u            // utils/mesh_utils.py:36: never keep a cluster below 50 triangles
#define MP_MAX_EDGES 0x7fffffffLL     // the sort's element count is an int32
#define MP_TRIS_EXCEED_SORT "n_tris %lld: the 3 n_tris edge records exceed the sort's 2^31 - 1 elements"

static inline int mp_bits(uint64_t max_value) {
    int b = 0;
    while (b < 32 && (max_value >> b)) ++b;
    return b;
}

struct MpWs {
    uint32_t* header;    // [0] clusters, [1] threshold
    uint32_t *lo, *hi;   // [E] per edge id
    uint32_t *ka, *va, *kb, *vb, *kt, *vt;   // [E] sort buffers
    void* sort_ws;
    int32_t* parent;     // [F]
    uint32_t* count;     // [F] triangles per root
    // the filter's part
    int32_t* labels;     // [F]
    int32_t* csize;      // [F]
    uint8_t* emit;       // [F] kept and not degenerate
    uint8_t* used;       // [V]
    uint32_t* vert_off;  // [V + 1]
    uint32_t* tri_off;   // [F + 1]
    void* scan_ws;
    size_t bytes;
};

// V < 0: the clustering part only
static MpWs mp_layout(void* base, int64_t F, int64_t V) {
    MpWs w{};
    GsrWsCursor c(base);
    const size_t f = size_t(F > 0 ? F : 1), e = 3 * f;
    w.header = c.take<uint32_t>(64 * 4);
    uint32_t** eb[] = {&w.lo, &w.hi, &w.ka, &w.va, &w.kb, &w.vb, &w.kt, &w.vt};
    for (uint32_t** q : eb) *q = c.take<uint32_t>(e * 4);
    w.sort_ws = c.take(gsr_sort_ws_bytes((int64_t)e));
    w.parent = c.take<int32_t>(f * 4);
    w.count = c.take<uint32_t>(f * 4);
    if (V >= 0) {
        const size_t v = size_t(V > 0 ? V : 1);
        w.labels = c.take<int32_t>(f * 4);
        w.csize = c.take<int32_t>(f * 4);
        w.emit = c.take<uint8_t>(f);
        w.used = c.take<uint8_t>(v);
        w.vert_off = c.take<uint32_t>((v + 1) * 4);
        w.tri_off = c.take<uint32_t>((f + 1) * 4);
        w.scan_ws = c.take(gsr_scan_workspace_bytes((int64_t)(v > f ? v : f)));
    }
    w.bytes = c.off;
    return w;
}

// ---------------------------------------------------------------- clusters
__global__ void __launch_bounds__(256) mp_edges_kernel(const int32_t* __restrict__ tris, int64_t F, uint32_t* __restrict__ lo,
                                                       uint32_t* __restrict__ hi, int32_t* __restrict__ parent) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * F) return;
    const int64_t t = e / 3;
    const int j = (int)(e - 3 * t);
    const uint32_t a = (uint32_t)tris[3 * t + j], b = (uint32_t)tris[3 * t + (j == 2 ? 0 : j + 1)];
    lo[e] = a < b ? a : b;
    hi[e] = a < b ? b : a;
    if (j == 0) parent[t] = (int32_t)t;
}

__global__ void __launch_bounds__(256) mp_gather_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx,
                                                        int64_t n, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}

// Other workgroups (other XCDs, other L2s) change `parent` during the launch: every read of it is an agent-scope atomic load
__device__ __forceinline__ int mp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Invariant of `parent`: parent[x] <= x, and parent[x] < x once x is not a root (hooks go larger -> smaller, the halving
// below only lowers an entry further, to an ancestor).  A walk therefore visits strictly decreasing ids: at most x steps,
// whatever the other threads do meanwhile.
__device__ __forceinline__ int mp_find(int32_t* parent, int x) {
    int p = mp_load(parent + x);
    while (p != x) {
        const int gp = mp_load(parent + p);
        if (gp != p) atomicMin(parent + x, gp);   // path halving: x is not a root and never becomes one again
        x = p;
        p = gp;
    }
    return x;
}

// No loop here waits for another thread's store.  The CAS hooks `a` under `b` only while a is still a root; when it fails,
// somebody else has hooked a, i.e. the number of roots went down -- and it never goes up -- so over the whole launch at
// most F CAS attempts fail.  A stale find costs one such retry, continued from the value the CAS returned; b may have stopped
// being a root meanwhile, which is harmless: b < a is in the same cluster as its root, and the walks stay decreasing.
__device__ __forceinline__ void mp_unite(int32_t* parent, int a, int b) {
    a = mp_find(parent, a);
    b = mp_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = mp_find(parent, old);
    }
}

__global__ void __launch_bounds__(256) mp_union_kernel(const uint32_t* __restrict__ lo_sorted, const uint32_t* __restrict__ e_sorted,
                                                       const uint32_t* __restrict__ hi, int64_t E, int32_t* parent) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= E) return;
    if (lo_sorted[i] != lo_sorted[i + 1]) return;
    const uint32_t e0 = e_sorted[i], e1 = e_sorted[i + 1];
    if (hi[e0] != hi[e1]) return;
    const int t0 = (int)(e0 / 3u), t1 = (int)(e1 / 3u);
    if (t0 != t1) mp_unite(parent, t0, t1);
}

// behind the kernel boundary every parent is visible to plain loads, and nothing changes any more
__global__ void __launch_bounds__(256) mp_flatten_kernel(const int32_t* __restrict__ parent, int64_t F, int32_t* __restrict__ labels) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F) return;
    int x = (int)t, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    labels[t] = x;
}

// count[root] += 1.  Nearly every triangle of a wave shares one root in a real mesh: the lanes with the root of the first
// pending lane add their popcount with ONE atomic, then the loop goes on over the remaining distinct roots.
__global__ void __launch_bounds__(256) mp_count_kernel(const int32_t* __restrict__ labels, int64_t F, uint32_t* __restrict__ count) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool pending = t < F;
    const int root = pending ? labels[t] : 0;
    for (;;) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, leader, 64);
        const bool same = pending && root == r0;
        const unsigned long long m = __ballot(same);
        if (lane == leader) atomicAdd(count + r0, (uint32_t)__popcll(m));
        if (same) pending = false;
    }
}

__global__ void __launch_bounds__(256) mp_size_kernel(const int32_t* __restrict__ labels, const uint32_t* __restrict__ count,
                                                      int64_t F, int32_t* __restrict__ csize) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < F) csize[t] = (int32_t)count[labels[t]];
}

static int mp_run_clusters(const int32_t* tris, int64_t F, int64_t V, int32_t* labels, int32_t* csize, const MpWs& w,
                           hipStream_t s) {
    const int64_t E = 3 * F;
    const unsigned eb = (unsigned)((E + 255) / 256), fb = (unsigned)((F + 255) / 256);
    const int bits = mp_bits((uint64_t)(V > 0 ? V - 1 : 0));   // the bits a vertex id can use
    hipLaunchKernelGGL(mp_edges_kernel, dim3(eb), dim3(256), 0, s, tris, F, w.lo, w.hi, w.parent);
    GSR_LAUNCH_CHECK();
    // (lo, hi) order = the host's stable argsort of lo * V + hi: stable by hi, then stable by lo; no 64-bit key
    int rc = gsr_radix_sort_pairs(w.hi, nullptr, w.ka, w.va, w.kt, w.vt, E, 0, bits, w.sort_ws, s);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(mp_gather_kernel, dim3(eb), dim3(256), 0, s, w.lo, w.va, E, w.kb);
    GSR_LAUNCH_CHECK();
    rc = gsr_radix_sort_pairs(w.kb, w.va, w.ka, w.vb, w.kt, w.vt, E, 0, bits, w.sort_ws, s);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(mp_union_kernel, dim3(eb), dim3(256), 0, s, w.ka, w.vb, w.hi, E, w.parent);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(mp_flatten_kernel, dim3(fb), dim3(256), 0, s, w.parent, F, labels);
    GSR_LAUNCH_CHECK();
    GSR_HIP_CHECK(hipMemsetAsync(w.count, 0, size_t(F) * 4, s));
    hipLaunchKernelGGL(mp_count_kernel, dim3(fb), dim3(256), 0, s, labels, F, w.count);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(mp_size_kernel, dim3(fb), dim3(256), 0, s, labels, w.count, F, csize);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" size_t gsr_mesh_clusters_workspace_bytes(int64_t n_tris) { return mp_layout(nullptr, n_tris, -1).bytes; }

extern "C" size_t gsr_mesh_filter_workspace_bytes(int64_t n_tris, int64_t n_verts) {
    return mp_layout(nullptr, n_tris, n_verts < 0 ? 0 : n_verts).bytes;
}

extern "C" int32_t gsr_mesh_clusters(const int32_t* tris, int64_t n_tris, int64_t n_verts, int32_t* labels,
                                     int32_t* cluster_size, void* ws, size_t ws_bytes, gsr_stream_t stream_) {
    int rc = gsr_check_mesh_counts(n_tris, n_verts, MP_MAX_EDGES / 3, MP_TRIS_EXCEED_SORT);
    if (rc != GSR_OK) return rc;
    if (n_tris == 0) return GSR_OK;
    if (!tris) { gsr_set_error("tris is null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    if (!labels || !cluster_size) { gsr_set_error("labels and cluster_size are required"); return GSR_E_INVALID; }
    const MpWs w = mp_layout(ws, n_tris, -1);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh cluster workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    return mp_run_clusters(tris, n_tris, n_verts, labels, cluster_size, w, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- threshold, marks, scans
__global__ void __launch_bounds__(256) mp_rootkey_kernel(const int32_t* __restrict__ labels, const uint32_t* __restrict__ count,
                                                         int64_t F, uint32_t* __restrict__ key, uint32_t* __restrict__ header) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = t < F && labels[t] == (int32_t)t;
    if (t < F) key[t] = root ? count[t] : 0u;
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(header, (uint32_t)__popcll(m));
}

__global__ void mp_threshold_kernel(const uint32_t* __restrict__ sorted, int64_t F, uint32_t k, uint32_t* __restrict__ header) {
    const uint32_t n_clusters = header[0];
    const uint32_t kk = k < n_clusters ? k : n_clusters;     // >= 1: F > 0 has at least one root
    const uint32_t c = sorted[F - kk];
    header[1] = c > MP_MIN_CLUSTER ? c : MP_MIN_CLUSTER;
}

__global__ void __launch_bounds__(256) mp_mark_kernel(const int32_t* __restrict__ tris, const int32_t* __restrict__ csize,
                                                      int64_t F, const uint32_t* __restrict__ header,
                                                      uint8_t* __restrict__ used, uint8_t* __restrict__ emit) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F) return;
    const bool keep = (uint32_t)csize[t] >= header[1];
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (keep) used[a] = used[b] = used[c] = 1;     // racing stores of the same byte
    // the vertex remap is injective: degenerate after it iff two ORIGINAL indices are equal
    emit[t] = keep && a != b && b != c && a != c;
}

extern "C" int32_t gsr_mesh_filter_count(const int32_t* tris, int64_t n_tris, int64_t n_verts, int32_t cluster_to_keep,
                                         void* ws, size_t ws_bytes, int64_t* n_verts_out, int64_t* n_tris_out,
                                         gsr_stream_t stream_) {
    if (!n_verts_out || !n_tris_out) { gsr_set_error("n_verts_out / n_tris_out are required"); return GSR_E_INVALID; }
    *n_verts_out = *n_tris_out = 0;
    int rc = gsr_check_mesh_counts(n_tris, n_verts, MP_MAX_EDGES / 3, MP_TRIS_EXCEED_SORT);
    if (rc != GSR_OK) return rc;
    if (cluster_to_keep < 1) { gsr_set_error("cluster_to_keep must be >= 1 (got %d)", cluster_to_keep); return GSR_E_INVALID; }
    if (n_tris == 0) return GSR_OK;
    if (!tris) { gsr_set_error("tris is null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    if (n_verts == 0) { gsr_set_error("n_verts is 0 with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    const MpWs w = mp_layout(ws, n_tris, n_verts);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh filter workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    unsigned long long* host = gsr_pinned_words(2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int64_t F = n_tris;
    const unsigned fb = (unsigned)((F + 255) / 256);
    rc = mp_run_clusters(tris, F, n_verts, w.labels, w.csize, w, s);
    if (rc != GSR_OK) return rc;
    GSR_HIP_CHECK(hipMemsetAsync(w.header, 0, 64 * 4, s));
    hipLaunchKernelGGL(mp_rootkey_kernel, dim3(fb), dim3(256), 0, s, w.labels, w.count, F, w.kb, w.header);
    GSR_LAUNCH_CHECK();
    rc = gsr_radix_sort_pairs(w.kb, nullptr, w.ka, w.va, w.kt, w.vt, F, 0, mp_bits((uint64_t)F), w.sort_ws, s);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(mp_threshold_kernel, dim3(1), dim3(1), 0, s, w.ka, F, (uint32_t)cluster_to_keep, w.header);
    GSR_LAUNCH_CHECK();
    GSR_HIP_CHECK(hipMemsetAsync(w.used, 0, size_t(n_verts), s));
    hipLaunchKernelGGL(mp_mark_kernel, dim3(fb), dim3(256), 0, s, tris, w.csize, F, w.header, w.used, w.emit);
    GSR_LAUNCH_CHECK();
    rc = gsr_exclusive_scan_u8(w.used, w.vert_off, n_verts, w.scan_ws, s);
    if (rc != GSR_OK) return rc;
    rc = gsr_exclusive_scan_u8(w.emit, w.tri_off, F, w.scan_ws, s);   // (same stream: the first scan is done with scan_ws)
    if (rc != GSR_OK) return rc;
    // the one synchronisation of the filter (as gsr_mcubes_count's): the two totals size the caller's output buffers
    uint32_t* h = reinterpret_cast<uint32_t*>(host);
    GSR_HIP_CHECK(hipMemcpyAsync(h, w.vert_off + n_verts, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipMemcpyAsync(h + 1, w.tri_off + F, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    *n_verts_out = (int64_t)h[0];
    *n_tris_out = (int64_t)h[1];
    return GSR_OK;
}

extern "C" int32_t gsr_mesh_filter_emit(const float* verts, const float* colors, const int32_t* tris, int64_t n_tris,
                                        int64_t n_verts, void* ws, size_t ws_bytes, float* verts_out, float* colors_out,
                                        int32_t* tris_out, gsr_stream_t stream_) {
    int rc = gsr_check_mesh_counts(n_tris, n_verts, MP_MAX_EDGES / 3, MP_TRIS_EXCEED_SORT);
    if (rc != GSR_OK) return rc;
    if (n_tris == 0) return GSR_OK;
    if (!verts || !colors || !tris) { gsr_set_error("verts, colors and tris are required"); return GSR_E_INVALID; }
    if (!verts_out || !colors_out || !tris_out) { gsr_set_error("verts_out, colors_out and tris_out are required"); return GSR_E_INVALID; }
    if (n_verts == 0) { gsr_set_error("n_verts is 0 with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    const MpWs w = mp_layout(ws, n_tris, n_verts);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh filter workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    const void* src[2] = {verts, colors};
    void* dst[2] = {verts_out, colors_out};
    const int32_t row_bytes[2] = {12, 12};
    rc = gsr_compact_apply(2, src, dst, row_bytes, n_verts, w.used, w.vert_off, stream_);
    if (rc != GSR_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(mesh_emit_tris_kernel, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, s, tris, n_tris, w.emit,
                       w.tri_off, w.vert_off, tris_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
