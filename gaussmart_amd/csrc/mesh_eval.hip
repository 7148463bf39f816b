// DTU mesh evaluation on the device (include/gsr.h, "mesh evaluation: DTU Chamfer distance"): what the reference's
// scripts/eval_dtu/eval.py does with numpy, a multiprocessing pool and scikit-learn's KD-tree, restated as the rules
// EVAL_SAMPLE ... EVAL_MEAN of the header.  This object is compiled with -ffp-contract=off: every fp64 expression below
// rounds operation by operation, like numpy's.
//
//   me_sample_count_kernel  one thread per triangle: n1, n2 and the number of kept (i, j) pairs, row by row (the keep test
//                           is monotone in j, so a row's count is found from an estimate and corrected with the test itself)
//   me_sample_emit_kernel   one thread per triangle writes its samples behind the scan of the counts; the same set-up and
//                           the same keep test (me_keep) as the count kernel
//   me_gather_kernel        EVAL_ORDER: out[k] = points[perm[k]]
//   cloud_bounds / cloud_morton (cloud_common.h), me_leaf / me_level kernels   the search structure: the searched cloud in 30-bit Morton order,
//                           bounds on leaves of 64 points, nodes of 64 leaves and tops of 64 nodes
//   me_nearest_kernel       EVAL_NN: one thread per query in the queries' own Morton order; the leaf found by a binary search
//                           of the query's clamped code seeds the best distance, then only boxes not farther than it are opened
//   me_mis_round_kernel     EVAL_DOWNSAMPLE: one round of the lexicographically first maximal independent set
//   me_obs_kernel, me_plane_kernel   EVAL_OBSMASK, EVAL_PLANE
//   me_mean_partial_kernel, me_mean_final_kernel   EVAL_MEAN
//
// Box distances are formed in fp64 from the f32 bounds with the expression of EVAL_DIST; every operation of it is monotone,
// so a box's distance never exceeds the d^2 of a point inside it and pruning on `box > best` is exact.
#include "cloud_common.h"
#include <cmath>

#define ME_LEAF 64                   // points per leaf, leaves per node, nodes per top
#define ME_SAMPLE_CAP 16777216.0     // n1 * n2 above 2^24: the triangle is refused
#define ME_MIS_BATCH 8               // rounds between two read-backs of the "any undecided" word

// ---------------------------------------------------------------- EVAL_SAMPLE
struct MeTri {
    double p0[3], v1[3], v2[3];
    double n1, n2;
};

__device__ __forceinline__ double me_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// False: the triangle gives nothing.  n1 * n2 above the cap is reported by the caller.
__device__ __forceinline__ bool me_tri_setup(const float* __restrict__ verts, const int32_t* __restrict__ tris, int64_t t,
                                             int64_t V, double thresh, MeTri& T) {
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if ((uint64_t)i0 >= (uint64_t)V || (uint64_t)i1 >= (uint64_t)V || (uint64_t)i2 >= (uint64_t)V) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        T.p0[a] = (double)verts[3 * (int64_t)i0 + a];
        T.v1[a] = (double)verts[3 * (int64_t)i1 + a] - T.p0[a];
        T.v2[a] = (double)verts[3 * (int64_t)i2 + a] - T.p0[a];
    }
    const double l1 = me_norm3(T.v1[0], T.v1[1], T.v1[2]), l2 = me_norm3(T.v2[0], T.v2[1], T.v2[2]);
    const double cx = T.v1[1] * T.v2[2] - T.v1[2] * T.v2[1];
    const double cy = T.v1[2] * T.v2[0] - T.v1[0] * T.v2[2];
    const double cz = T.v1[0] * T.v2[1] - T.v1[1] * T.v2[0];
    const double area2 = me_norm3(cx, cy, cz);
    if (!(area2 > 0.0)) return false;
    const double thr = thresh * sqrt(l1 * l2 / area2);
    T.n1 = floor(l1 / thr);
    T.n2 = floor(l2 / thr);
    return T.n1 >= 1.0 && T.n2 >= 1.0;              // false for NaN as well
}

// the keep test of EVAL_SAMPLE, shared by the count and the emit kernel
__device__ __forceinline__ bool me_keep(double i, double j, double n1, double n2) {
    const double a = (i + 0.5) / n1, b = (j + 0.5) / n2;
    return a + b < 1.0;
}

// number of j in [0, n2] that row i keeps (the test is monotone in j: kept ones come first)
__device__ __forceinline__ int64_t me_row_count(double i, double n1, double n2) {
    const double a = (i + 0.5) / n1;
    double e = ceil((1.0 - a) * n2 - 0.5);
    e = fmin(fmax(e, 0.0), n2 + 1.0);
    while (e > 0.0 && !me_keep(i, e - 1.0, n1, n2)) e -= 1.0;
    while (e <= n2 && me_keep(i, e, n1, n2)) e += 1.0;
    return (int64_t)e;
}

// info[0]: 64-bit total of the counts, info[1]: triangles refused by the cap
__global__ void __launch_bounds__(256) me_sample_count_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                              int64_t F, int64_t V, double thresh, uint32_t* __restrict__ counts,
                                                              unsigned long long* __restrict__ info) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cnt = 0;
    bool refused = false;
    if (t < F) {
        MeTri T;
        if (me_tri_setup(verts, tris, t, V, thresh, T)) {
            if (!(T.n1 * T.n2 <= ME_SAMPLE_CAP)) {
                refused = true;
            } else {
                for (double i = 0.0; i <= T.n1; i += 1.0) {
                    const int64_t r = me_row_count(i, T.n1, T.n2);
                    if (r == 0) break;              // monotone in i as well
                    cnt += (unsigned long long)r;
                }
            }
        }
        counts[t] = (uint32_t)cnt;                  // below 2^26 under the cap
    }
    unsigned long long sum = cnt;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&info[0], sum);
    if (refused) atomicAdd(&info[1], 1ull);
}

__global__ void __launch_bounds__(256) me_sample_emit_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                             int64_t F, int64_t V, double thresh,
                                                             const uint32_t* __restrict__ off, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F) return;
    uint32_t w = off[t];
    const uint32_t end = off[t + 1];
    if (w == end) return;
    MeTri T;
    if (!me_tri_setup(verts, tris, t, V, thresh, T)) return;
    for (double i = 0.0; i <= T.n1 && w < end; i += 1.0) {
        const double a = (i + 0.5) / T.n1;
        for (double j = 0.0; j <= T.n2 && w < end; j += 1.0) {
            if (!me_keep(i, j, T.n1, T.n2)) break;
            const double b = (j + 0.5) / T.n2;
            float* q = out + 3 * (int64_t)w;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = (float)((T.v1[c] * a + T.v2[c] * b) + T.p0[c]);     // EVAL_POINT_F32
            ++w;
        }
    }
}

struct MeSampleWs {
    unsigned long long* info;   // [2]
    uint32_t* counts;           // [F]
    uint32_t* off;              // [F + 1]
    void* scan_ws;
    size_t bytes;
};

static MeSampleWs me_sample_layout(void* base, int64_t F) {
    MeSampleWs w{};
    GsrWsCursor c(base);
    const size_t f = size_t(F > 0 ? F : 1);
    w.info = c.take<unsigned long long>(16);
    w.counts = c.take<uint32_t>(f * 4);
    w.off = c.take<uint32_t>((f + 1) * 4);
    w.scan_ws = c.take(gsr_scan_workspace_bytes((int64_t)f));
    w.bytes = c.off;
    return w;
}

static int me_check_sample(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, double thresh,
                           void* ws, size_t ws_bytes, MeSampleWs& w) {
    int rc = gsr_check_count("n_tris", n_tris);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_count("n_verts", n_verts);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_positive("thresh", thresh);
    if (rc != GSR_OK) return rc;
    if (n_verts > 0 && !verts) { gsr_set_error("verts is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    if (n_tris > 0 && !tris) { gsr_set_error("tris is null with n_tris %lld", (long long)n_tris); return GSR_E_INVALID; }
    w = me_sample_layout(ws, n_tris);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: mesh sampling workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

extern "C" size_t gsr_mesh_sample_workspace_bytes(int64_t n_tris) { return me_sample_layout(nullptr, n_tris).bytes; }

extern "C" int32_t gsr_mesh_sample_count(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, double thresh,
                                         void* ws, size_t ws_bytes, int64_t* n_points_out, gsr_stream_t stream_) {
    if (!n_points_out) { gsr_set_error("n_points_out is required"); return GSR_E_INVALID; }
    *n_points_out = 0;
    MeSampleWs w;
    int rc = me_check_sample(verts, tris, n_tris, n_verts, thresh, ws, ws_bytes, w);
    if (rc != GSR_OK) return rc;
    *n_points_out = n_verts;
    if (n_tris == 0) return GSR_OK;
    unsigned long long* host = gsr_pinned_words(2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GSR_HIP_CHECK(hipMemsetAsync(w.info, 0, 16, s));
    hipLaunchKernelGGL(me_sample_count_kernel, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, s, verts, tris, n_tris,
                       n_verts, thresh, w.counts, w.info);
    GSR_LAUNCH_CHECK();
    rc = gsr_exclusive_scan_u32(w.counts, nullptr, w.off, n_tris, w.scan_ws, s);
    if (rc != GSR_OK) return rc;
    // the one read-back: the 64-bit total sizes the caller's output, the second word says whether a triangle was refused
    GSR_HIP_CHECK(hipMemcpyAsync(host, w.info, 16, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    if (host[1]) {
        gsr_set_error("%llu triangles ask for more than 2^24 samples each (n1 * n2): raise downsample_density or subdivide the mesh",
                      host[1]);
        return GSR_E_UNSUPPORTED;
    }
    if (host[0] + (unsigned long long)n_verts > 0x7fffffffULL) {
        gsr_set_error("%llu samples + %lld vertices exceed int32 indices: raise downsample_density", host[0], (long long)n_verts);
        return GSR_E_UNSUPPORTED;
    }
    *n_points_out = n_verts + (int64_t)host[0];
    return GSR_OK;
}

extern "C" int32_t gsr_mesh_sample_emit(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, double thresh,
                                        void* ws, size_t ws_bytes, float* points_out, gsr_stream_t stream_) {
    MeSampleWs w;
    int rc = me_check_sample(verts, tris, n_tris, n_verts, thresh, ws, ws_bytes, w);
    if (rc != GSR_OK) return rc;
    if (n_verts == 0) return GSR_OK;                // no vertex: every index is out of range, nothing was counted
    if (!points_out) { gsr_set_error("points_out is null with n_verts %lld", (long long)n_verts); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GSR_HIP_CHECK(hipMemcpyAsync(points_out, verts, size_t(n_verts) * 12, hipMemcpyDeviceToDevice, s));
    if (n_tris == 0) return GSR_OK;
    hipLaunchKernelGGL(me_sample_emit_kernel, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, s, verts, tris, n_tris,
                       n_verts, thresh, w.off, points_out + 3 * n_verts);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- EVAL_ORDER
__global__ void __launch_bounds__(256) me_gather_kernel(const float* __restrict__ points, const int32_t* __restrict__ perm,
                                                        int64_t n, int64_t n_src, float* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int32_t src = perm[k];
    const bool in = (uint64_t)src < (uint64_t)n_src;        // an index outside the source gives a NaN row, never a wild read
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * k + c] = in ? points[3 * (int64_t)src + c] : __uint_as_float(0x7fc00000u);
}

extern "C" int32_t gsr_points_gather(const float* points, int64_t n_src, const int32_t* perm, int64_t n, float* out,
                                     gsr_stream_t stream_) {
    int rc = gsr_check_count("n_src", n_src);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (n == 0) return GSR_OK;
    if (!perm || !out) { gsr_set_error("perm / out are null with n %lld", (long long)n); return GSR_E_INVALID; }
    if (n_src > 0 && !points) { gsr_set_error("points is null with n_src %lld", (long long)n_src); return GSR_E_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(me_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, perm, n, n_src, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- the search structure
struct MeTree {
    const float4* pts;          // [n] Morton order; w carries the point's index in the caller's array
    const uint32_t* codes;      // [n] sorted codes
    const float* leaf;          // [nl, 6] lo.xyz hi.xyz
    const float* node;          // [nn, 6]
    const float* top;           // [nt, 6]
    const uint32_t* mm;         // [6] bounds of the cloud as ordered words
    int n, nl, nn, nt;
};

// one wave per leaf: gathers its 64 points into Morton order and bounds them
__global__ void __launch_bounds__(256) me_leaf_kernel(const float* __restrict__ xyz, int n, const uint32_t* __restrict__ order,
                                                      float4* __restrict__ sorted, float* __restrict__ boxes, int nl) {
    const int lf = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (lf >= nl) return;
    const int64_t i = (int64_t)lf * ME_LEAF + (threadIdx.x & 63);
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (i < n) {
        const uint32_t src = order[i];
        const float x = xyz[3 * (int64_t)src], y = xyz[3 * (int64_t)src + 1], z = xyz[3 * (int64_t)src + 2];
        sorted[i] = make_float4(x, y, z, __uint_as_float(src));
        lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min_f32(lo[a]); hi[a] = wave_max_f32(hi[a]); }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { boxes[6 * (int64_t)lf + a] = lo[a]; boxes[6 * (int64_t)lf + 3 + a] = hi[a]; }
    }
}

// one thread per box of the level above: the bounds of its (up to) 64 children
__global__ void __launch_bounds__(256) me_level_kernel(const float* __restrict__ in, int n_in, float* __restrict__ out, int n_out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_out) return;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    const int e = min(n_in, (b + 1) * ME_LEAF);
    for (int k = b * ME_LEAF; k < e; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], in[6 * (int64_t)k + a]);
            hi[a] = fmaxf(hi[a], in[6 * (int64_t)k + 3 + a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { out[6 * (int64_t)b + a] = lo[a]; out[6 * (int64_t)b + 3 + a] = hi[a]; }
}

// EVAL_DIST between a query (already widened) and an f32 point
__device__ __forceinline__ double me_dist2(const double* q, float x, float y, float z) {
    const double dx = q[0] - (double)x, dy = q[1] - (double)y, dz = q[2] - (double)z;
    return (dx * dx + dy * dy) + dz * dz;
}

// EVAL_DIST's expression on the per-axis gaps to a box: every operation is monotone in the gaps, and a gap is the rounded
// difference to the nearest face, so the result is <= me_dist2 of every point inside the box
__device__ __forceinline__ double me_box_dist2(const double* q, const float* __restrict__ b) {
    const double dx = fmax(fmax((double)b[0] - q[0], q[0] - (double)b[3]), 0.0);
    const double dy = fmax(fmax((double)b[1] - q[1], q[1] - (double)b[4]), 0.0);
    const double dz = fmax(fmax((double)b[2] - q[2], q[2] - (double)b[5]), 0.0);
    return (dx * dx + dy * dy) + dz * dz;
}

// Visits every point whose box chain is not farther than vis.bound().  vis.point(d2, index) returns true to stop.
template <class Visitor>
__device__ __forceinline__ void me_visit_leaf(const MeTree& T, const double* q, int lf, Visitor& vis, bool& stop) {
    const int e = min(T.n, (lf + 1) * ME_LEAF);
    for (int k = lf * ME_LEAF; k < e && !stop; ++k) {
        const float4 p = T.pts[k];
        stop = vis.point(me_dist2(q, p.x, p.y, p.z), (int32_t)__float_as_uint(p.w));
    }
}

template <class Visitor>
__device__ __forceinline__ void me_traverse(const MeTree& T, const double* q, Visitor& vis) {
    bool stop = false;
    for (int t = 0; t < T.nt && !stop; ++t) {
        if (me_box_dist2(q, T.top + 6 * (int64_t)t) > vis.bound()) continue;
        const int ne = min(T.nn, (t + 1) * ME_LEAF);
        for (int nd = t * ME_LEAF; nd < ne && !stop; ++nd) {
            if (me_box_dist2(q, T.node + 6 * (int64_t)nd) > vis.bound()) continue;
            const int le = min(T.nl, (nd + 1) * ME_LEAF);
            for (int lf = nd * ME_LEAF; lf < le && !stop; ++lf) {
                if (me_box_dist2(q, T.leaf + 6 * (int64_t)lf) > vis.bound()) continue;
                me_visit_leaf(T, q, lf, vis, stop);
            }
        }
    }
}

// EVAL_NN: the smallest d^2, the smallest index among equal ones; nothing above `best` as it starts
struct MeNearest {
    double best;
    uint32_t idx;               // 0xffffffff: none yet
    __device__ __forceinline__ double bound() const { return best; }
    __device__ __forceinline__ bool point(double d2, int32_t j) {
        if (d2 < best || (d2 == best && (uint32_t)j < idx)) { best = d2; idx = (uint32_t)j; }
        return false;
    }
};

// `radius2`: +inf, or max_dist^2 grown by 2^-50 relative -- sqrt(d2) < max_dist implies d2 below it, so nothing that could
// pass the final `d < max_dist` is pruned; the decision itself is taken on d = sqrt(d2)
__global__ void __launch_bounds__(256) me_nearest_kernel(MeTree T, const float* __restrict__ query, int nq,
                                                         const uint32_t* __restrict__ qcodes, const uint32_t* __restrict__ qorder,
                                                         double radius2, double max_dist, double* __restrict__ dist_out,
                                                         int32_t* __restrict__ idx_out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nq) return;
    const uint32_t qi = qorder[s];
    const double q[3] = {(double)query[3 * (int64_t)qi], (double)query[3 * (int64_t)qi + 1], (double)query[3 * (int64_t)qi + 2]};
    MeNearest vis{radius2, 0xffffffffu};
    // seed: the leaf at the lower bound of the query's code among the sorted codes
    const uint32_t code = qcodes[s];
    int lo = 0, hi = T.n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (T.codes[mid] < code) lo = mid + 1; else hi = mid;
    }
    bool stop = false;
    me_visit_leaf(T, q, min(lo, T.n - 1) / ME_LEAF, vis, stop);
    me_traverse(T, q, vis);
    const double d = sqrt(vis.best);
    const bool found = vis.idx != 0xffffffffu && d < max_dist;
    dist_out[qi] = found ? d : INFINITY;
    idx_out[qi] = found ? (int32_t)vis.idx : -1;
}

__global__ void __launch_bounds__(256) me_fill_none_kernel(int64_t n, double* __restrict__ dist_out, int32_t* __restrict__ idx_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { dist_out[i] = INFINITY; idx_out[i] = -1; }
}

// EVAL_DOWNSAMPLE, one round.  state: 0 undecided, 1 kept, 2 removed; a state is written once and never changes again, so a
// stale 0 read here only postpones a decision to a later round.  `pending` (may be NULL): bit `bit` is set when a point is
// still undecided after this round.
struct MeMis {
    double t2;
    int32_t self;
    const int32_t* state;
    bool removed, waiting;
    __device__ __forceinline__ double bound() const { return t2; }
    __device__ __forceinline__ bool point(double d2, int32_t j) {
        if (j < self && d2 <= t2) {
            const int32_t st = __atomic_load_n(state + j, __ATOMIC_RELAXED);
            if (st == 1) { removed = true; return true; }
            if (st == 0) waiting = true;
        }
        return false;
    }
};

__global__ void __launch_bounds__(256) me_mis_round_kernel(MeTree T, double t2, int32_t* __restrict__ state,
                                                           uint32_t* __restrict__ pending, int bit) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= T.n) return;
    const float4 p = T.pts[s];
    const int32_t i = (int32_t)__float_as_uint(p.w);
    if (__atomic_load_n(state + i, __ATOMIC_RELAXED) != 0) return;
    const double q[3] = {(double)p.x, (double)p.y, (double)p.z};
    MeMis vis{t2, i, state, false, false};
    me_traverse(T, q, vis);
    if (vis.removed) __atomic_store_n(state + i, 2, __ATOMIC_RELAXED);
    else if (!vis.waiting) __atomic_store_n(state + i, 1, __ATOMIC_RELAXED);
    else if (pending && !(__atomic_load_n(pending, __ATOMIC_RELAXED) >> bit & 1u)) atomicOr(pending, 1u << bit);
}

__global__ void __launch_bounds__(256) me_state_to_keep_kernel(const int32_t* __restrict__ state, int64_t n, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = state[i] == 1;
}

struct MeSearchWs {
    uint32_t *mm, *pending;
    uint32_t *codes, *codes_sorted, *order, *kt, *vt;       // [max(n, nq)] each (the queries' sort reuses codes, kt, vt)
    uint32_t *cloud_codes;                                  // [n] the cloud's sorted codes, kept for the seeds
    uint32_t *qorder;                                       // [nq]
    int32_t* state;                                         // [n]
    float4* pts;
    float *leaf, *node, *top;
    void* sort_ws;
    int nl, nn, nt;
    size_t bytes;
};

static MeSearchWs me_search_layout(void* base, int64_t n_cloud, int64_t n_query) {
    MeSearchWs w{};
    GsrWsCursor c(base);
    const size_t n = size_t(n_cloud > 0 ? n_cloud : 1), nq = size_t(n_query > 0 ? n_query : 1), m = n > nq ? n : nq;
    w.nl = (int)((n + ME_LEAF - 1) / ME_LEAF);
    w.nn = (w.nl + ME_LEAF - 1) / ME_LEAF;
    w.nt = (w.nn + ME_LEAF - 1) / ME_LEAF;
    w.mm = c.take<uint32_t>(32);
    w.pending = c.take<uint32_t>(4);
    w.codes = c.take<uint32_t>(m * 4);
    w.codes_sorted = c.take<uint32_t>(m * 4);
    w.order = c.take<uint32_t>(m * 4);
    w.kt = c.take<uint32_t>(m * 4);
    w.vt = c.take<uint32_t>(m * 4);
    w.cloud_codes = c.take<uint32_t>(n * 4);
    w.qorder = c.take<uint32_t>(nq * 4);
    w.state = c.take<int32_t>(n * 4);
    w.pts = c.take<float4>(n * 16);
    w.leaf = c.take<float>(size_t(w.nl) * 24);
    w.node = c.take<float>(size_t(w.nn) * 24);
    w.top = c.take<float>(size_t(w.nt) * 24);
    // (the sort's workspace is not monotone in n: both sorts must fit)
    const size_t sa = gsr_sort_ws_bytes((int64_t)n), sb = gsr_sort_ws_bytes((int64_t)nq);
    w.sort_ws = c.take(sa > sb ? sa : sb);
    w.bytes = c.off;
    return w;
}

// builds the structure over `cloud` (n >= 1) in w; the sorted codes end up in w.cloud_codes
static int me_build_tree(const float* cloud, int64_t n, const MeSearchWs& w, MeTree& T, hipStream_t s) {
    int rc = cloud_bounds<true>(cloud, n, w.mm, s);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(cloud_morton_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cloud, n, w.mm, w.codes);
    GSR_LAUNCH_CHECK();
    rc = gsr_radix_sort_pairs(w.codes, nullptr, w.cloud_codes, w.order, w.kt, w.vt, n, 0, 30, w.sort_ws, s);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(me_leaf_kernel, dim3((w.nl + 3) / 4), dim3(256), 0, s, cloud, (int)n, w.order, w.pts, w.leaf, w.nl);
    hipLaunchKernelGGL(me_level_kernel, dim3((w.nn + 255) / 256), dim3(256), 0, s, w.leaf, w.nl, w.node, w.nn);
    hipLaunchKernelGGL(me_level_kernel, dim3((w.nt + 255) / 256), dim3(256), 0, s, w.node, w.nn, w.top, w.nt);
    GSR_LAUNCH_CHECK();
    T = MeTree{w.pts, w.cloud_codes, w.leaf, w.node, w.top, w.mm, (int)n, w.nl, w.nn, w.nt};
    return GSR_OK;
}

extern "C" size_t gsr_points_search_workspace_bytes(int64_t n_cloud, int64_t n_query) {
    return me_search_layout(nullptr, n_cloud, n_query).bytes;
}

extern "C" int32_t gsr_points_downsample(const float* points, int64_t n, double thresh, void* ws, size_t ws_bytes,
                                         uint8_t* keep_out, int32_t* rounds_out, gsr_stream_t stream_) {
    if (rounds_out) *rounds_out = 0;
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_positive("thresh", thresh);
    if (rc != GSR_OK) return rc;
    if (n == 0) return GSR_OK;
    if (!points || !keep_out) { gsr_set_error("points / keep_out are null with n %lld", (long long)n); return GSR_E_INVALID; }
    const MeSearchWs w = me_search_layout(ws, n, 0);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: point search workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    unsigned long long* host = gsr_pinned_words(1);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    MeTree T;
    rc = me_build_tree(points, n, w, T, s);
    if (rc != GSR_OK) return rc;
    GSR_HIP_CHECK(hipMemsetAsync(w.state, 0, size_t(n) * 4, s));
    const double t2 = thresh * thresh;
    const dim3 grid((unsigned)((n + 255) / 256));
    // every round decides at least the lowest undecided point, so n rounds always suffice
    int32_t rounds = 0;
    for (int64_t done = 0; done < n + ME_MIS_BATCH; done += ME_MIS_BATCH) {
        GSR_HIP_CHECK(hipMemsetAsync(w.pending, 0, 4, s));
        for (int r = 0; r < ME_MIS_BATCH; ++r) {
            hipLaunchKernelGGL(me_mis_round_kernel, grid, dim3(256), 0, s, T, t2, w.state, w.pending, r);
            GSR_LAUNCH_CHECK();
        }
        uint32_t* h = reinterpret_cast<uint32_t*>(host);
        GSR_HIP_CHECK(hipMemcpyAsync(h, w.pending, 4, hipMemcpyDeviceToHost, s));
        GSR_HIP_CHECK(hipStreamSynchronize(s));
        // bit r: somebody was undecided after round r of the batch; the bits are a prefix of ones
        int used = 0;
        while (used < ME_MIS_BATCH && (*h >> used & 1u)) ++used;
        if (used < ME_MIS_BATCH) { rounds += used + 1; break; }
        rounds += ME_MIS_BATCH;
    }
    if (rounds_out) *rounds_out = rounds;
    hipLaunchKernelGGL(me_state_to_keep_kernel, grid, dim3(256), 0, s, w.state, n, keep_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_points_nearest(const float* query, int64_t n_query, const float* cloud, int64_t n_cloud, double max_dist,
                                      void* ws, size_t ws_bytes, double* dist_out, int32_t* idx_out, gsr_stream_t stream_) {
    int rc = gsr_check_count("n_query", n_query);
    if (rc != GSR_OK) return rc;
    rc = gsr_check_count("n_cloud", n_cloud);
    if (rc != GSR_OK) return rc;
    if (!(max_dist > 0.0)) { gsr_set_error("max_dist must be > 0 (got %g; +inf: no limit)", max_dist); return GSR_E_INVALID; }
    if (n_query == 0) return GSR_OK;
    if (!query || !dist_out || !idx_out) {
        gsr_set_error("query / dist_out / idx_out are null with n_query %lld", (long long)n_query);
        return GSR_E_INVALID;
    }
    if (n_cloud > 0 && !cloud) { gsr_set_error("cloud is null with n_cloud %lld", (long long)n_cloud); return GSR_E_INVALID; }
    const MeSearchWs w = me_search_layout(ws, n_cloud, n_query);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: point search workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const dim3 grid((unsigned)((n_query + 255) / 256));
    if (n_cloud == 0) {
        hipLaunchKernelGGL(me_fill_none_kernel, grid, dim3(256), 0, s, n_query, dist_out, idx_out);
        GSR_LAUNCH_CHECK();
        return GSR_OK;
    }
    MeTree T;
    rc = me_build_tree(cloud, n_cloud, w, T, s);
    if (rc != GSR_OK) return rc;
    // the queries in their own Morton order (codes in the cloud's bounds, clamped): neighbouring lanes walk the same boxes
    hipLaunchKernelGGL(cloud_morton_kernel, grid, dim3(256), 0, s, query, n_query, w.mm, w.codes);
    GSR_LAUNCH_CHECK();
    rc = gsr_radix_sort_pairs(w.codes, nullptr, w.codes_sorted, w.qorder, w.kt, w.vt, n_query, 0, 30, w.sort_ws, s);
    if (rc != GSR_OK) return rc;
    const double radius2 = max_dist <= DBL_MAX ? (max_dist * max_dist) * (1.0 + 0x1p-50) : INFINITY;
    hipLaunchKernelGGL(me_nearest_kernel, grid, dim3(256), 0, s, T, query, (int)n_query, w.codes_sorted, w.qorder, radius2,
                       max_dist, dist_out, idx_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- EVAL_OBSMASK, EVAL_PLANE
struct MeObs {
    double bb0[3], bb1[3], res, patch;
    int32_t shape[3];
};

__global__ void __launch_bounds__(256) me_obs_kernel(const float* __restrict__ points, int64_t n, const uint8_t* __restrict__ mask,
                                                     MeObs o, uint8_t* __restrict__ inbound, uint8_t* __restrict__ in_obs,
                                                     uint8_t* inbound_out, uint8_t* in_obs_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool inb = true, grid = true;
    int64_t cell = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p = (double)points[3 * i + a];
        inb = inb && p >= o.bb0[a] - o.patch && p < o.bb1[a] + o.patch * 2.0;
        const double g = rint((p - o.bb0[a]) / o.res);                 // round half to even
        grid = grid && g >= 0.0 && g < (double)o.shape[a];             // false for NaN
        cell = cell * o.shape[a] + (grid ? (int64_t)g : 0);
    }
    const bool obs = inb && grid && mask[cell] != 0;
    inbound[i] = inb; in_obs[i] = obs;
    if (inbound_out) inbound_out[i] = inb;
    if (in_obs_out) in_obs_out[i] = obs;
}

struct MeObsWs {
    uint8_t *inbound, *in_obs;   // [n]
    uint32_t *off_in, *off_obs;  // [n + 1]
    void* scan_ws;
    size_t bytes;
};

static MeObsWs me_obs_layout(void* base, int64_t n_) {
    MeObsWs w{};
    GsrWsCursor c(base);
    const size_t n = size_t(n_ > 0 ? n_ : 1);
    w.inbound = c.take<uint8_t>(n);
    w.in_obs = c.take<uint8_t>(n);
    w.off_in = c.take<uint32_t>((n + 1) * 4);
    w.off_obs = c.take<uint32_t>((n + 1) * 4);
    w.scan_ws = c.take(gsr_scan_workspace_bytes((int64_t)n));
    w.bytes = c.off;
    return w;
}

extern "C" size_t gsr_points_obs_workspace_bytes(int64_t n) { return me_obs_layout(nullptr, n).bytes; }

extern "C" int32_t gsr_points_obs_filter_count(const float* points, int64_t n, const uint8_t* obs_mask, const int32_t* shape_host,
                                               const float* bb_host, double res, double patch, void* ws, size_t ws_bytes,
                                               uint8_t* inbound_out, uint8_t* in_obs_out, int64_t* n_in_out,
                                               int64_t* n_in_obs_out, gsr_stream_t stream_) {
    if (!n_in_out || !n_in_obs_out) { gsr_set_error("n_in_out / n_in_obs_out are required"); return GSR_E_INVALID; }
    *n_in_out = *n_in_obs_out = 0;
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (!shape_host || !bb_host) { gsr_set_error("shape_host and bb_host are required"); return GSR_E_INVALID; }
    if (shape_host[0] < 1 || shape_host[1] < 1 || shape_host[2] < 1) {
        gsr_set_error("the ObsMask shape must be >= 1 on every axis (got %d x %d x %d)", shape_host[0], shape_host[1], shape_host[2]);
        return GSR_E_INVALID;
    }
    if (!(res > 0.0) || !(res <= DBL_MAX)) { gsr_set_error("res must be > 0 and finite (got %g)", res); return GSR_E_INVALID; }
    if (!(patch >= 0.0) || !(patch <= DBL_MAX)) { gsr_set_error("patch must be >= 0 and finite (got %g)", patch); return GSR_E_INVALID; }
    if (!obs_mask) { gsr_set_error("obs_mask is null"); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!points) { gsr_set_error("points is null with n %lld", (long long)n); return GSR_E_INVALID; }
    const MeObsWs w = me_obs_layout(ws, n);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: ObsMask filter workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    unsigned long long* host = gsr_pinned_words(2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    MeObs o;
    for (int a = 0; a < 3; ++a) { o.bb0[a] = (double)bb_host[a]; o.bb1[a] = (double)bb_host[3 + a]; o.shape[a] = shape_host[a]; }
    o.res = res; o.patch = patch;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(me_obs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, obs_mask, o, w.inbound,
                       w.in_obs, inbound_out, in_obs_out);
    GSR_LAUNCH_CHECK();
    rc = gsr_exclusive_scan_u8(w.inbound, w.off_in, n, w.scan_ws, s);
    if (rc != GSR_OK) return rc;
    rc = gsr_exclusive_scan_u8(w.in_obs, w.off_obs, n, w.scan_ws, s);    // (same stream: the first scan is done with scan_ws)
    if (rc != GSR_OK) return rc;
    uint32_t* h = reinterpret_cast<uint32_t*>(host);
    GSR_HIP_CHECK(hipMemcpyAsync(h, w.off_in + n, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipMemcpyAsync(h + 1, w.off_obs + n, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    *n_in_out = (int64_t)h[0];
    *n_in_obs_out = (int64_t)h[1];
    return GSR_OK;
}

extern "C" int32_t gsr_points_obs_filter_emit(const float* points, int64_t n, void* ws, size_t ws_bytes, float* data_in_out,
                                              float* data_in_obs_out, gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (n == 0) return GSR_OK;
    if (!points) { gsr_set_error("points is null with n %lld", (long long)n); return GSR_E_INVALID; }
    const MeObsWs w = me_obs_layout(ws, n);
    if (!ws || ws_bytes < w.bytes) {
        gsr_set_error("ws_bytes: ObsMask filter workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return GSR_E_INVALID;
    }
    const int32_t row_bytes[1] = {12};
    const void* src[1] = {points};
    if (data_in_out) {
        void* dst[1] = {data_in_out};
        rc = gsr_compact_apply(1, src, dst, row_bytes, n, w.inbound, w.off_in, stream_);
        if (rc != GSR_OK) return rc;
    }
    if (data_in_obs_out) {
        void* dst[1] = {data_in_obs_out};
        rc = gsr_compact_apply(1, src, dst, row_bytes, n, w.in_obs, w.off_obs, stream_);
        if (rc != GSR_OK) return rc;
    }
    return GSR_OK;
}

struct MePlane { double p[4]; };

__global__ void __launch_bounds__(256) me_plane_kernel(const float* __restrict__ points, int64_t n, MePlane pl,
                                                       uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)points[3 * i], y = (double)points[3 * i + 1], z = (double)points[3 * i + 2];
    keep[i] = ((pl.p[0] * x + pl.p[1] * y) + pl.p[2] * z) + pl.p[3] > 0.0;
}

extern "C" int32_t gsr_points_plane_filter(const float* points, int64_t n, const double* plane_host, uint8_t* keep_out,
                                           gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (!plane_host) { gsr_set_error("plane_host (P0..P3) is required"); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!points || !keep_out) { gsr_set_error("points / keep_out are null with n %lld", (long long)n); return GSR_E_INVALID; }
    MePlane pl;
    for (int a = 0; a < 4; ++a) pl.p[a] = plane_host[a];
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(me_plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, pl, keep_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- EVAL_MEAN
// The fixed order of gsr_block_sum_256 (cloud_common.h) for the sum and, in the same pass, the count: below 2^31, so exact as a
// double in any order.
__global__ void __launch_bounds__(256) me_mean_partial_kernel(const double* __restrict__ dist, int64_t n, double* __restrict__ psum,
                                                              unsigned long long* __restrict__ pcnt) {
    __shared__ double s_val[2 * 256];
    double sum = 0.0;
    unsigned long long cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double d = dist[i];
        if (d <= DBL_MAX) { sum += d; ++cnt; }          // finite distances only (they are never negative)
    }
    double v[2] = {sum, (double)cnt};
    gsr_block_sum_256(v, s_val);
    if (threadIdx.x == 0) { psum[blockIdx.x] = v[0]; pcnt[blockIdx.x] = (unsigned long long)v[1]; }
}

__global__ void __launch_bounds__(256) me_mean_final_kernel(const double* __restrict__ psum, const unsigned long long* __restrict__ pcnt,
                                                            int blocks, double* __restrict__ mean_out, int64_t* __restrict__ count_out) {
    __shared__ double s_val[2 * 256];
    double sum = 0.0;
    unsigned long long cnt = 0;
    for (int b = threadIdx.x; b < blocks; b += 256) { sum += psum[b]; cnt += pcnt[b]; }
    double v[2] = {sum, (double)cnt};
    gsr_block_sum_256(v, s_val);
    if (threadIdx.x == 0) {
        *mean_out = v[1] > 0.0 ? v[0] / v[1] : __longlong_as_double(0x7ff8000000000000LL);    // empty: NaN, like numpy's mean
        if (count_out) *count_out = (int64_t)v[1];
    }
}

extern "C" size_t gsr_dist_mean_workspace_bytes(int64_t n) { (void)n; return gsr_align(GSR_PARTIAL_BLOCKS * 8) * 2; }

extern "C" int32_t gsr_dist_mean(const double* dist, int64_t n, void* ws, size_t ws_bytes, double* mean_out, int64_t* count_out,
                                 gsr_stream_t stream_) {
    int rc = gsr_check_count("n", n);
    if (rc != GSR_OK) return rc;
    if (!mean_out) { gsr_set_error("mean_out is required"); return GSR_E_INVALID; }
    if (n > 0 && !dist) { gsr_set_error("dist is null with n %lld", (long long)n); return GSR_E_INVALID; }
    if (!ws || ws_bytes < gsr_dist_mean_workspace_bytes(n)) {
        gsr_set_error("ws_bytes: mean workspace too small (%zu < %zu bytes)", ws_bytes, gsr_dist_mean_workspace_bytes(n));
        return GSR_E_INVALID;
    }
    GsrWsCursor c(ws);
    double* psum = c.take<double>(GSR_PARTIAL_BLOCKS * 8);
    unsigned long long* pcnt = c.take<unsigned long long>(GSR_PARTIAL_BLOCKS * 8);
    const unsigned blocks = gsr_partial_blocks(n);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (blocks > 0) {
        hipLaunchKernelGGL(me_mean_partial_kernel, dim3(blocks), dim3(256), 0, s, dist, n, psum, pcnt);
        GSR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(me_mean_final_kernel, dim3(1), dim3(256), 0, s, psum, pcnt, (int)blocks, mean_out, count_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
