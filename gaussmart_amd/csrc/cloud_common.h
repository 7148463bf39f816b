// The primitives every point-cloud object shares (knn.hip, mesh_eval.hip, tnt_eval.hip, seg_init.hip): order-preserving
// float words, the bounds reduction, 30-bit Morton codes and the fixed-order block sum.  Header-only: each including object
// compiles its own copy under its own flags (mesh_emit.h's precedent of a static __global__ in a header).
//
// Contraction: mesh_eval.o, tnt_eval.o and seg_init.o are built with -ffp-contract=off, knn.o with -ffp-contract=fast, and
// the results of both kinds are held to the same bits.  Nothing below forms a multiply followed by an add or subtract --
// the Morton code is subtract, divide, multiply, clamp; the bounds are min / max; the block sum only adds -- so both settings
// generate the same arithmetic.  Anything added here that could contract must not be used from both kinds of object.
#pragma once
#include "gsr_common.h"
#include "wave_reduce.h"
#include <cfloat>

// ---------------------------------------------------------------- capped grids
// Workgroups (of 256 threads) of a grid-stride reduction over n elements.  The cap bounds the partial arrays and the number
// of atomics; a kernel launched with it must loop: i += gridDim.x * 256.
#define GSR_PARTIAL_BLOCKS 1024
static inline unsigned gsr_partial_blocks(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < GSR_PARTIAL_BLOCKS ? b : GSR_PARTIAL_BLOCKS);
}

// ---------------------------------------------------------------- ordered words
// u(a) < u(b) exactly when a < b (-0 below +0): integer atomicMin / atomicMax give the same word whatever the order of arrival
__device__ __forceinline__ uint32_t gsr_f2ord(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float gsr_ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }
__device__ __forceinline__ unsigned long long gsr_d2ord(double f) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(f);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double gsr_ord2d(unsigned long long u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

// ---------------------------------------------------------------- bounds
// mm[0..2]: the per-axis minimum of xyz[n, 3] as ordered words; WITH_MAX: mm[3..5] the maximum.  Without it the words behind
// mm[2] are never touched (tnt_eval.hip keeps its cell count and refusal flag there).  A NaN coordinate is passed over.
template <bool WITH_MAX>
static __global__ void __launch_bounds__(256) cloud_bounds_kernel(const float* __restrict__ xyz, int64_t n,
                                                                  uint32_t* __restrict__ mm) {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3 * i + a];
            lo[a] = fminf(lo[a], v);
            if (WITH_MAX) hi[a] = fmaxf(hi[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = wave_min_f32(lo[a]);
        if (WITH_MAX) hi[a] = wave_max_f32(hi[a]);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&mm[a], gsr_f2ord(lo[a]));
            if (WITH_MAX) atomicMax(&mm[3 + a], gsr_f2ord(hi[a]));
        }
    }
}

// clears the words (minimum: all ones, maximum: zero) and launches the reduction on its capped grid; n >= 1
template <bool WITH_MAX>
static int cloud_bounds(const float* xyz, int64_t n, uint32_t* mm, hipStream_t s) {
    GSR_HIP_CHECK(hipMemsetAsync(mm, 0xFF, 12, s));
    if (WITH_MAX) GSR_HIP_CHECK(hipMemsetAsync(mm + 3, 0x00, 12, s));
    hipLaunchKernelGGL(cloud_bounds_kernel<WITH_MAX>, dim3(gsr_partial_blocks(n)), dim3(256), 0, s, xyz, n, mm);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- Morton codes
__device__ __forceinline__ uint32_t gsr_spread10(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// 30-bit Morton code of a point in the bounds mm (six words of cloud_bounds<true>), clamped into them: a query may lie
// anywhere, and NaN gives 0
__device__ __forceinline__ uint32_t cloud_morton_code(const float* __restrict__ p, const uint32_t* __restrict__ mm) {
    uint32_t c = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = gsr_ord2f(mm[a]), ext = gsr_ord2f(mm[3 + a]) - lo;
        const float rel = ext > 0.f ? (p[a] - lo) / ext : 0.f;
        const uint32_t q = (uint32_t)fminf(fmaxf(rel * 1023.0f, 0.f), 1023.f);
        c |= gsr_spread10(q) << a;
    }
    return c;
}

static __global__ void __launch_bounds__(256) cloud_morton_kernel(const float* __restrict__ xyz, int64_t n,
                                                                  const uint32_t* __restrict__ mm,
                                                                  uint32_t* __restrict__ codes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) codes[i] = cloud_morton_code(xyz + 3 * i, mm);
}

// ---------------------------------------------------------------- fixed-order block sum
// The one order of EVAL_MEAN, TNT_ICP_SUMS, SEG_MEANSTD and SEG_STATS (include/gsr.h): a thread adds its own elements in
// index order, then this tree adds the 256 threads' values, d = 128, 64, ..., 1; a kernel launched on gsr_partial_blocks(n)
// workgroups writes one row of partials per workgroup and ONE workgroup adds those rows the same way (thread t takes rows
// t, t + 256, ...).  The grid depends on n alone, so a result has the same bits on every run.
// s: NV * 256 values of LDS, value q of thread t at s[q * 256 + t].  On return every thread holds the totals in v.  No
// barrier follows the last read: a caller that writes s again must put one in between.
template <class T, int NV>
__device__ __forceinline__ void gsr_block_sum_256(T (&v)[NV], T* s) {
#pragma unroll
    for (int q = 0; q < NV; ++q) s[q * 256 + threadIdx.x] = v[q];
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
#pragma unroll
            for (int q = 0; q < NV; ++q) s[q * 256 + threadIdx.x] += s[q * 256 + threadIdx.x + d];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = s[q * 256];
}
template <class T>
__device__ __forceinline__ T gsr_block_sum_256(T v, T* s) {
    T a[1] = {v};
    gsr_block_sum_256<T, 1>(a, s);
    return a[0];
}
