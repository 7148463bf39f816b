// CK_LLOYD (include/gsr.h): the Lloyd iterations of many small, independent k-means fits over one set of camera centres, one
// workgroup per fit, everything in LDS and fp64.  Step 1 of the reference's identification/main.py runs 140 scikit-learn fits
// (identification/clustering_cameras.py: k = 3 .. 15, n_init = 10) over at most a few hundred points; the initial centres of all
// of them are drawn on the host (gaussmart_amd/camera_select.py, scikit-learn's random stream) and every fit goes out in this
// one launch.  Every sum has a stated order, so the numpy twin (camera_select.lloyd_batch_host) gives the same bits.
// Built with -ffp-contract=off: a fused multiply-add would round the squared distances differently from numpy.
#include "gsr_common.h"

#define CK_BLOCK 256
#define CK_CHUNK GSR_CK_CHUNK
#define CK_MAXN GSR_CK_MAX_CAMERAS
#define CK_KMAX GSR_CK_KMAX
#define CK_MAXCHUNKS (CK_MAXN / CK_CHUNK)
static_assert(CK_MAXN % CK_CHUNK == 0, "the cap is a whole number of chunks");
static_assert(CK_KMAX < 255, "labels are bytes in LDS and 255 is 'none yet'");

// why the loop ended: one LDS word, written by thread 0, read by every thread after a barrier
enum { CK_GO = 0, CK_STRICT = 1, CK_TOL = 2, CK_MAXITER = 3, CK_EMPTY = 4 };

struct CkShared {
    double x[3][CK_MAXN];                       // the points, one axis after the other
    double part[CK_KMAX][CK_MAXCHUNKS][4];      // per (cluster, chunk): sum x, sum y, sum z, members
    double centre[CK_KMAX][3], fresh[CK_KMAX][3], shift[CK_KMAX];
    uint8_t label[CK_MAXN];
    int changed, empty, exit_code;
};
static_assert(sizeof(CkShared) <= 160 * 1024, "one workgroup's LDS on gfx950");

// CK_LLOYD's distance: the three squares summed left to right
__device__ __forceinline__ double ck_sqdist(double x0, double x1, double x2, const double* c) {
    const double d0 = x0 - c[0], d1 = x1 - c[1], d2 = x2 - c[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// labels of every point against s.centre; ties go to the lowest cluster.  Returns whether a label of this thread changed.
__device__ __forceinline__ bool ck_assign(CkShared& s, int n, int k) {
    bool changed = false;
    for (int i = threadIdx.x; i < n; i += CK_BLOCK) {
        const double x0 = s.x[0][i], x1 = s.x[1][i], x2 = s.x[2][i];
        double best = ck_sqdist(x0, x1, x2, s.centre[0]);
        int arg = 0;
        for (int c = 1; c < k; ++c) {
            const double d = ck_sqdist(x0, x1, x2, s.centre[c]);
            if (d < best) { best = d; arg = c; }
        }
        changed |= s.label[i] != (uint8_t)arg;
        s.label[i] = (uint8_t)arg;
    }
    return changed;
}

__global__ void __launch_bounds__(CK_BLOCK) cam_lloyd_kernel(const double* __restrict__ x, int n,
                                                             const double* __restrict__ centres0, const int32_t* __restrict__ ks,
                                                             double tol, int max_iter, int32_t* __restrict__ labels,
                                                             double* __restrict__ centres, double* __restrict__ inertia,
                                                             int32_t* __restrict__ n_iter, int32_t* __restrict__ status) {
    __shared__ CkShared s;
    const int fit = blockIdx.x, t = threadIdx.x;
    const int k = ks[fit];
    if (k < 1 || k > CK_KMAX) {        // the same for the whole workgroup: nobody reaches a barrier
        if (t == 0) { status[fit] = 2; n_iter[fit] = 0; inertia[fit] = 0.0; }
        for (int i = t; i < n; i += CK_BLOCK) labels[(size_t)fit * n + i] = -1;
        for (int i = t; i < CK_KMAX * 3; i += CK_BLOCK) centres[(size_t)fit * CK_KMAX * 3 + i] = 0.0;
        return;
    }
    const int nchunks = (n + CK_CHUNK - 1) / CK_CHUNK;
    for (int i = t; i < n; i += CK_BLOCK) {
        s.x[0][i] = x[3 * (size_t)i]; s.x[1][i] = x[3 * (size_t)i + 1]; s.x[2][i] = x[3 * (size_t)i + 2];
        s.label[i] = 255;
    }
    if (t < 3 * k) s.centre[t / 3][t % 3] = centres0[(size_t)fit * CK_KMAX * 3 + t];
    if (t == 0) { s.changed = 0; s.empty = 0; s.exit_code = CK_GO; }
    __syncthreads();

    int it = 0, why = CK_GO;
    for (;;) {
        // A: labels
        if (ck_assign(s, n, k)) atomicOr(&s.changed, 1);
        __syncthreads();
        // B: per (cluster, chunk) sums, ascending index inside the chunk
        for (int task = t; task < k * nchunks; task += CK_BLOCK) {
            const int c = task / nchunks, ch = task - c * nchunks;
            const int end = min(n, (ch + 1) * CK_CHUNK);
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0;
            for (int j = ch * CK_CHUNK; j < end; ++j)
                if (s.label[j] == c) { s0 += s.x[0][j]; s1 += s.x[1][j]; s2 += s.x[2][j]; cnt += 1.0; }
            double* p = s.part[c][ch];
            p[0] = s0; p[1] = s1; p[2] = s2; p[3] = cnt;
        }
        __syncthreads();
        // C: the chunks in ascending order; the new centre and its squared shift
        if (t < k) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0;
            for (int ch = 0; ch < nchunks; ++ch) {
                const double* p = s.part[t][ch];
                s0 += p[0]; s1 += p[1]; s2 += p[2]; cnt += p[3];
            }
            if (cnt == 0.0) {
                atomicOr(&s.empty, 1);
            } else {
                const double f[3] = {s0 / cnt, s1 / cnt, s2 / cnt};
                s.fresh[t][0] = f[0]; s.fresh[t][1] = f[1]; s.fresh[t][2] = f[2];
                s.shift[t] = ck_sqdist(f[0], f[1], f[2], s.centre[t]);
            }
        }
        __syncthreads();
        // D: thread 0 decides; the centres move unless a cluster is empty
        const bool empty = s.empty != 0;
        if (t == 0) {
            int e = CK_GO;
            if (empty) {
                e = CK_EMPTY;
            } else {
                double shift = 0.0;
                for (int c = 0; c < k; ++c) shift += s.shift[c];
                if (!s.changed) e = CK_STRICT;
                else if (shift <= tol) e = CK_TOL;
                else if (it + 1 >= max_iter) e = CK_MAXITER;
            }
            s.changed = 0;
            s.exit_code = e;
        }
        if (!empty && t < 3 * k) s.centre[t / 3][t % 3] = s.fresh[t / 3][t % 3];
        __syncthreads();
        ++it;
        why = s.exit_code;          // the one word every wave leaves the loop by
        if (why != CK_GO) break;
    }
    if (why == CK_TOL || why == CK_MAXITER) {       // uniform: labels against the final centres
        ck_assign(s, n, k);
        __syncthreads();
    }
    // inertia: per chunk in ascending index, then the chunks in ascending order (part[0][ch][0] is free again)
    if (t < nchunks) {
        const int end = min(n, (t + 1) * CK_CHUNK);
        double acc = 0.0;
        for (int j = t * CK_CHUNK; j < end; ++j) acc += ck_sqdist(s.x[0][j], s.x[1][j], s.x[2][j], s.centre[s.label[j]]);
        s.part[0][t][0] = acc;
    }
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
        for (int ch = 0; ch < nchunks; ++ch) acc += s.part[0][ch][0];
        inertia[fit] = acc;
        n_iter[fit] = it;
        status[fit] = why == CK_EMPTY ? 1 : 0;
    }
    for (int i = t; i < n; i += CK_BLOCK) labels[(size_t)fit * n + i] = s.label[i];
    for (int i = t; i < CK_KMAX * 3; i += CK_BLOCK)
        centres[(size_t)fit * CK_KMAX * 3 + i] = i < 3 * k ? s.centre[i / 3][i % 3] : 0.0;
}

extern "C" size_t gsr_cam_lloyd_workspace_bytes(int32_t n, int32_t n_fits) {
    (void)n; (void)n_fits;
    return 0;       // up to GSR_CK_MAX_CAMERAS points a fit lives in LDS alone
}

extern "C" int32_t gsr_cam_lloyd(const double* x, int32_t n, const double* centres0, const int32_t* k, int32_t n_fits, double tol,
                                 int32_t max_iter, int32_t* labels, double* centres, double* inertia, int32_t* n_iter,
                                 int32_t* status, void* ws, size_t ws_bytes, gsr_stream_t stream_) {
    (void)ws; (void)ws_bytes;
    if (n < 1) { gsr_set_error("gsr_cam_lloyd: n must be >= 1 (got %d)", n); return GSR_E_INVALID; }
    if (n > GSR_CK_MAX_CAMERAS) {
        gsr_set_error("gsr_cam_lloyd: n %d exceeds GSR_CK_MAX_CAMERAS %d, the points one workgroup keeps in LDS; use the host route "
                      "(gaussmart_amd.camera_select.lloyd_batch_host)", n, GSR_CK_MAX_CAMERAS);
        return GSR_E_UNSUPPORTED;
    }
    if (n_fits < 0) { gsr_set_error("gsr_cam_lloyd: n_fits must be >= 0 (got %d)", n_fits); return GSR_E_INVALID; }
    if (max_iter < 1) { gsr_set_error("gsr_cam_lloyd: max_iter must be >= 1 (got %d)", max_iter); return GSR_E_INVALID; }
    if (!(tol >= 0.0)) { gsr_set_error("gsr_cam_lloyd: tol must be >= 0 (got %g)", tol); return GSR_E_INVALID; }
    if (n_fits == 0) return GSR_OK;
    if (!x || !centres0 || !k || !labels || !centres || !inertia || !n_iter || !status) {
        gsr_set_error("gsr_cam_lloyd: null buffer");
        return GSR_E_INVALID;
    }
    hipLaunchKernelGGL(cam_lloyd_kernel, dim3(n_fits), dim3(CK_BLOCK), 0, static_cast<hipStream_t>(stream_), x, n, centres0, k, tol,
                       max_iter, labels, centres, inertia, n_iter, status);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
