// LPIPS (lpipsPyTorch/modules/{lpips,networks,utils}.py of the reference) as kernels, fp32 throughout: the convolutions of
// the AlexNet / VGG16 trunks as implicit GEMMs on the f32-input matrix instruction, the max-pools, and the per-layer head.
// The rules are in include/gsr.h (LP_CONV, LP_POOL, LP_HEAD, LP_FORWARD); each has one named place below.
#include "cloud_common.h"
#include <type_traits>

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- LP_CONV
// out[b, co, oy, ox] = relu(bias[co] + sum_k w[co, k] * x[b, ci, oy s - p + ky, ox s - p + kx]), k = (ci KS + ky) KS + kx
// ascending: GEMM  D[co][pixel] = W[co][k] X[k][pixel]  with W the weight tensor as it lies in memory ([C_out][K] row-major)
// and X gathered on the fly (zero outside the image).  A workgroup of 4 waves owns BM output channels x BN pixels
// (BM 128: 2 x 2 waves, BN 128; BM 64: 1 x 4 waves, BN 256), a wave 2 x 2 tiles of 32 x 32, K in chunks of 32 through LDS
// with the next chunk's global loads issued between the chunk's 64 matrix instructions.  v_mfma_f32_32x32x2_f32 is a
// k-ordered fma chain, so every output element is ONE chain over k = 0 .. K-1 from 0, then + bias, then relu: no split-K, no
// atomics, the same bits on every run and for either image of the pair.  A tail chunk multiplies zeros: fma(0, 0, acc) = acc.
#define LP_KC 32
#define LP_ZMEAN0 (-0.030f)
#define LP_ZMEAN1 (-0.088f)
#define LP_ZMEAN2 (-0.188f)
#define LP_ZSTD0 0.458f
#define LP_ZSTD1 0.448f
#define LP_ZSTD2 0.450f

template <int KS, int BM, bool ZS>
__global__ void __launch_bounds__(256) lp_conv_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ y, int B, int C_in, int H, int W, int C_out, int OH,
                                                      int OW, int stride, int pad) {
    constexpr int WGM = BM / 64, WGN = 4 / WGM, BN = WGN * 64;
    constexpr int NA = BM * LP_KC / 256, NB = BN * LP_KC / 256;       // elements of a chunk per thread
    constexpr int LDA = BM + 1, BKSTEP = 256 / BN;  // LDA odd: the 32 lanes of a half-wave write 32 k rows into 32 banks
    __shared__ float As[LP_KC * LDA];               // [k][co]
    __shared__ float Bs[LP_KC * BN];                // [k][pixel]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave % WGM, wn = wave / WGM;
    const int K = C_in * KS * KS;
    const int64_t plane = (int64_t)OH * OW, npix = plane * B;
    const int64_t HW = (int64_t)H * W, CHW = HW * C_in;
    const int m0 = (int)blockIdx.y * BM;
    const int64_t p0 = (int64_t)blockIdx.x * BN;

    // the gather: a thread keeps ONE pixel of the tile and walks k, and the k of an element is the same for the whole wave
    // (bk0 is read as a scalar), so the split k -> (ci, ky, kx) and the offset ci H W + ky W + kx run on the scalar unit.
    // The weights: k fastest (32 consecutive floats of a row).
    const int bp = t % BN, bk0 = __builtin_amdgcn_readfirstlane(t / BN);
    const int ak = t & 31, am = t >> 5;
    const int64_t p = p0 + bp;
    const bool p_ok = p < npix;
    int iy0 = 0, ix0 = 0;
    const float* xb = x0;
    if (p_ok) {
        const int64_t b = p / plane, rem = p - b * plane;
        const int oy = (int)(rem / OW), ox = (int)(rem - (int64_t)oy * OW);
        iy0 = oy * stride - pad;
        ix0 = ox * stride - pad;
        xb = b == 0 ? x0 : x1 + (b - 1) * CHW;
    }
    const float* xp = xb + ((int64_t)iy0 * W + ix0);        // the window's corner: only formed into addresses inside the image
    // a tile whose every window lies inside the image (most of them) gathers without the four comparisons per element
    const bool inside = __syncthreads_and(p_ok && iy0 >= 0 && ix0 >= 0 && iy0 + KS <= H && ix0 + KS <= W);

    float ra[NA], rb[NB];
    // part kk (of LP_KC / 2) of a chunk's loads: the main loop issues one part behind each k-pair's matrix instructions, so
    // that the address arithmetic runs while the matrix pipe is busy
    auto load = [&](int k0, int kk, auto inside_tag) {
        constexpr bool INSIDE = decltype(inside_tag)::value;
#pragma unroll
        for (int j = kk * NA / (LP_KC / 2); j < (kk + 1) * NA / (LP_KC / 2); ++j) {
            const int m = m0 + am + 8 * j, k = k0 + ak;
            const bool ok = m < C_out && k < K;
            const float v = w[ok ? (int64_t)m * K + k : 0];       // no branch: what must not be read reads element 0
            ra[j] = ok ? v : 0.f;
        }
#pragma unroll
        for (int j = kk * NB / (LP_KC / 2); j < (kk + 1) * NB / (LP_KC / 2); ++j) {
            const int k = k0 + bk0 + BKSTEP * j;
            const bool kin = k < K;                 // scalar: false only in the tail chunk
            const int kc = kin ? k : 0;
            const int ci = kc / (KS * KS), r = kc - ci * (KS * KS);
            const int ky = r / KS, kx = r - ky * KS;
            const int64_t koff = (int64_t)ci * HW + (int64_t)ky * W + kx;
            const bool ok = kin && (INSIDE || (p_ok && (unsigned)(iy0 + ky) < (unsigned)H && (unsigned)(ix0 + kx) < (unsigned)W));
            float v = *(ok ? xp + koff : x0);       // no branch: what must not be read reads x0[0]
            // BaseNet.z_score in the load: only what lies inside the image is normalised, the padding stays 0
            if (ZS)
                v = (v - (ci == 0 ? LP_ZMEAN0 : ci == 1 ? LP_ZMEAN1 : LP_ZMEAN2)) / (ci == 0 ? LP_ZSTD0 : ci == 1 ? LP_ZSTD1 : LP_ZSTD2);
            rb[j] = ok ? v : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NA; ++j) As[ak * LDA + am + 8 * j] = ra[j];
#pragma unroll
        for (int j = 0; j < NB; ++j) Bs[(bk0 + BKSTEP * j) * BN + bp] = rb[j];
    };

    lp_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
    for (int kk = 0; kk < LP_KC / 2; ++kk) {
        if (inside) load(0, kk, std::true_type{});
        else load(0, kk, std::false_type{});
    }
    store();
    __syncthreads();
    const int lrow = lane >> 5, lcol = lane & 31;
    // one chunk: 16 k-pairs of 2 x 2 matrix instructions each; prefetch(kk) is what is issued behind pair kk
    auto chunk = [&](auto prefetch) {
#pragma unroll
        for (int kk = 0; kk < LP_KC / 2; ++kk) {
            const int krow = 2 * kk + lrow;         // lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31]
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[krow * LDA + wm * 64 + i * 32 + lcol];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[krow * BN + wn * 64 + j * 32 + lcol];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
            prefetch(kk);
        }
    };
    for (int k0 = 0; k0 < K; k0 += LP_KC) {
        const bool more = k0 + LP_KC < K;
        if (!more) chunk([](int) {});
        else if (inside) chunk([&](int kk) { load(k0 + LP_KC, kk, std::true_type{}); });
        else chunk([&](int kk) { load(k0 + LP_KC, kk, std::false_type{}); });
        __syncthreads();
        if (more) {
            store();
            __syncthreads();
        }
    }

    // C/D map: column = lane & 31 (the pixel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (the channel)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t q = p0 + wn * 64 + j * 32 + lcol;
        if (q >= npix) continue;
        const int64_t b = q / plane, rem = q - b * plane;
        float* yb = y + b * C_out * plane + rem;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
                if (co < C_out) {
                    const float v = acc[i][j][r] + bias[co];
                    yb[(int64_t)co * plane] = v < 0.f ? 0.f : v;      // relu; a NaN stays a NaN
                }
            }
        }
    }
}

template <int KS>
static int lp_launch_conv(const float* x0, const float* x1, const float* w, const float* bias, float* y, int B, int C_in, int H,
                          int W, int C_out, int OH, int OW, int stride, int pad, int zscore, hipStream_t s) {
    const int64_t npix = (int64_t)B * OH * OW;
    // the 64-wide tile where 128 would leave rows empty (64, 192); the 128-wide one otherwise
#define LP_CONV_LAUNCH(BM, ZS) \
    hipLaunchKernelGGL((lp_conv_kernel<KS, BM, ZS>), dim3((unsigned)((npix + 256 * 64 / BM - 1) / (256 * 64 / BM)), (unsigned)((C_out + BM - 1) / BM)), \
                       dim3(256), 0, s, x0, x1, w, bias, y, B, C_in, H, W, C_out, OH, OW, stride, pad)
    if (C_out % 128 == 0) {
        if (zscore) LP_CONV_LAUNCH(128, true);
        else LP_CONV_LAUNCH(128, false);
    } else {
        if (zscore) LP_CONV_LAUNCH(64, true);
        else LP_CONV_LAUNCH(64, false);
    }
#undef LP_CONV_LAUNCH
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

static int lp_conv_out(int n, int k, int s, int p) { return n + 2 * p < k ? 0 : (n + 2 * p - k) / s + 1; }

// x1: image 1 of the batch where it does not follow image 0 in memory (the pair of gsr_lpips_forward); else NULL
static int lp_conv(const float* x0, const float* x1, const float* w, const float* bias, float* y, int B, int C_in, int H, int W,
                   int C_out, int ks, int stride, int pad, int zscore, hipStream_t s) {
    if (B < 1 || C_in < 1 || C_out < 1 || H < 1 || W < 1 || stride < 1 || pad < 0) {
        gsr_set_error("lpips conv: B %d, C_in %d, C_out %d, H %d, W %d, stride %d must be >= 1 and pad %d >= 0", B, C_in, C_out, H, W,
                      stride, pad);
        return GSR_E_INVALID;
    }
    if (!x0 || !w || !bias || !y) { gsr_set_error("lpips conv: x / w / bias / y is null"); return GSR_E_INVALID; }
    if (zscore && C_in != 3) { gsr_set_error("lpips conv: zscore normalises 3 channels (got C_in %d)", C_in); return GSR_E_INVALID; }
    if ((int64_t)C_in * ks * ks > 0x7fffffffLL || C_out > 65535 * 64) {
        gsr_set_error("lpips conv: C_in %d x %d x %d or C_out %d exceeds the kernel's index range", C_in, ks, ks, C_out);
        return GSR_E_UNSUPPORTED;
    }
    const int OH = lp_conv_out(H, ks, stride, pad), OW = lp_conv_out(W, ks, stride, pad);
    if (OH < 1 || OW < 1) {
        gsr_set_error("lpips conv: a %dx%d image with pad %d is smaller than the %dx%d kernel", H, W, pad, ks, ks);
        return GSR_E_INVALID;
    }
    if (((int64_t)B * OH * OW + 127) / 128 > 0x7fffffffLL) { gsr_set_error("lpips conv: too many output pixels"); return GSR_E_UNSUPPORTED; }
    if (!x1) x1 = x0 + (int64_t)C_in * H * W;
    switch (ks) {
    case 3: return lp_launch_conv<3>(x0, x1, w, bias, y, B, C_in, H, W, C_out, OH, OW, stride, pad, zscore, s);
    case 5: return lp_launch_conv<5>(x0, x1, w, bias, y, B, C_in, H, W, C_out, OH, OW, stride, pad, zscore, s);
    case 11: return lp_launch_conv<11>(x0, x1, w, bias, y, B, C_in, H, W, C_out, OH, OW, stride, pad, zscore, s);
    default: gsr_set_error("lpips conv: kernel size %d is not one of 3, 5, 11", ks); return GSR_E_UNSUPPORTED;
    }
}

extern "C" int32_t gsr_lpips_conv(const float* x, const float* w, const float* bias, int32_t B, int32_t C_in, int32_t H, int32_t W,
                                  int32_t C_out, int32_t ksize, int32_t stride, int32_t pad, int32_t zscore, float* y,
                                  gsr_stream_t stream_) {
    return lp_conv(x, nullptr, w, bias, y, B, C_in, H, W, C_out, ksize, stride, pad, zscore, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- LP_POOL
// torch's max_pool2d, stride 2, floor mode, no padding: the maximum starts at -inf and a NaN wins
template <int KS>
__global__ void __launch_bounds__(256) lp_pool_kernel(const float* __restrict__ x, int64_t planes, int H, int W, int OH, int OW,
                                                      float* __restrict__ y) {
    const int64_t n = planes * OH * OW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t pl = i / ((int64_t)OH * OW), rem = i - pl * ((int64_t)OH * OW);
        const int oy = (int)(rem / OW), ox = (int)(rem - (int64_t)oy * OW);
        const float* src = x + pl * ((int64_t)H * W) + (int64_t)(2 * oy) * W + 2 * ox;
        float m = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < KS; ++dy)
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) {
                const float v = src[(int64_t)dy * W + dx];
                if (v > m || v != v) m = v;
            }
        y[i] = m;
    }
}

static int lp_pool(const float* x, int64_t planes, int H, int W, int ks, float* y, hipStream_t s) {
    if (ks != 2 && ks != 3) { gsr_set_error("lpips pool: window %d is not 2 or 3", ks); return GSR_E_UNSUPPORTED; }
    if (planes < 1 || H < ks || W < ks) {
        gsr_set_error("lpips pool: planes %lld must be >= 1 and the %dx%d plane at least the %dx%d window", (long long)planes, H, W, ks, ks);
        return GSR_E_INVALID;
    }
    if (!x || !y) { gsr_set_error("lpips pool: x / y is null"); return GSR_E_INVALID; }
    const int OH = (H - ks) / 2 + 1, OW = (W - ks) / 2 + 1;
    const int64_t n = planes * OH * OW;
    const int64_t blocks = (n + 255) / 256;
    const dim3 grid((unsigned)(blocks < 0x7fffffffLL ? blocks : 0x7fffffffLL));
    if (ks == 2) hipLaunchKernelGGL(lp_pool_kernel<2>, grid, dim3(256), 0, s, x, planes, H, W, OH, OW, y);
    else hipLaunchKernelGGL(lp_pool_kernel<3>, grid, dim3(256), 0, s, x, planes, H, W, OH, OW, y);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_lpips_pool(const float* x, int64_t planes, int32_t H, int32_t W, int32_t ksize, float* y, gsr_stream_t stream_) {
    return lp_pool(x, planes, H, W, ksize, y, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- LP_HEAD
// A workgroup takes 32 consecutive pixels at a time; its 256 threads are 8 channel groups x 32 pixels, and a thread keeps its
// C / 8 channels of BOTH images in registers: the maps are read once.  Per pixel: the squared norms (a thread adds its channels
// in order, then the 8 groups are added in order 0..7 through LDS), n = sqrt(.) + 1e-10, then sum_c w_c (x_c / nx - y_c / ny)^2
// with true divisions, as normalize_activation and LPIPS.forward order it.  The spatial mean is cloud_common.h's fixed order:
// a thread adds its pixels' values in index order, gsr_block_sum_256 adds the threads, one workgroup adds the capped grid's
// partials the same way and divides by H W.
#define LP_HEAD_MAXC 512
#define LP_HEAD_CPT (LP_HEAD_MAXC / 8)

static unsigned lp_head_blocks(int64_t npix) { return gsr_partial_blocks(((npix + 31) / 32) * 256); }

// CPT: channels a thread keeps; EXACT: C == 8 CPT (the trunks' widths), else C / 8 <= CPT is read at run time
template <int CPT, bool EXACT>
__global__ void __launch_bounds__(256) lp_head_kernel(const float* __restrict__ feat, const float* __restrict__ lin_w, int C,
                                                      int64_t npix, float* __restrict__ partial) {
    __shared__ float s_n[2 * 8 * 32];
    __shared__ float s_sum[256];
    const int t = threadIdx.x, px = t & 31, g = t >> 5;
    const int cpt = EXACT ? CPT : C / 8;
    const float* fx = feat + (int64_t)(g * cpt) * npix;
    const float* fy = fx + (int64_t)C * npix;
    const float* wg = lin_w + g * cpt;
    float total = 0.f;
    const int64_t groups = (npix + 31) / 32;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {     // the bound is uniform: every thread meets the barriers
        const int64_t p = grp * 32 + px;
        const bool ok = p < npix;
        float xv[CPT], yv[CPT];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            if (EXACT || i < cpt) {
                xv[i] = ok ? fx[(int64_t)i * npix + p] : 0.f;
                yv[i] = ok ? fy[(int64_t)i * npix + p] : 0.f;
                sx += xv[i] * xv[i];
                sy += yv[i] * yv[i];
            }
        }
        s_n[g * 32 + px] = sx;
        s_n[256 + g * 32 + px] = sy;
        __syncthreads();
        float nx = 0.f, ny = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) { nx += s_n[q * 32 + px]; ny += s_n[256 + q * 32 + px]; }
        __syncthreads();
        nx = sqrtf(nx) + 1e-10f;
        ny = sqrtf(ny) + 1e-10f;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            if (EXACT || i < cpt) {
                const float d = xv[i] / nx - yv[i] / ny;
                v += wg[i] * (d * d);
            }
        }
        total += v;          // a pixel past the end adds (0 / 1e-10 - 0 / 1e-10)^2 = 0
    }
    total = gsr_block_sum_256(total, s_sum);
    if (t == 0) partial[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) lp_head_final_kernel(const float* __restrict__ partial, int blocks, float count,
                                                            float* __restrict__ out) {
    __shared__ float s_sum[256];
    float v = 0.f;
    for (int b = threadIdx.x; b < blocks; b += 256) v += partial[b];
    v = gsr_block_sum_256(v, s_sum);
    if (threadIdx.x == 0) *out = v / count;
}

extern "C" size_t gsr_lpips_head_workspace_bytes(void) { return gsr_align(GSR_PARTIAL_BLOCKS * 4); }

static int lp_head(const float* feat, const float* lin_w, int C, int H, int W, void* ws, size_t ws_bytes, float* out, hipStream_t s) {
    if (C < 8 || C > LP_HEAD_MAXC || C % 8 != 0) {
        gsr_set_error("lpips head: C %d is not a multiple of 8 in [8, %d]", C, LP_HEAD_MAXC);
        return GSR_E_UNSUPPORTED;
    }
    if (H < 1 || W < 1) { gsr_set_error("lpips head: H %d and W %d must be >= 1", H, W); return GSR_E_INVALID; }
    if (!feat || !lin_w || !out) { gsr_set_error("lpips head: feat / lin_w / out is null"); return GSR_E_INVALID; }
    if (!ws || ws_bytes < gsr_lpips_head_workspace_bytes()) {
        gsr_set_error("ws_bytes: lpips head workspace too small (%zu < %zu bytes)", ws_bytes, gsr_lpips_head_workspace_bytes());
        return GSR_E_INVALID;
    }
    const int64_t npix = (int64_t)H * W;
    const unsigned blocks = lp_head_blocks(npix);
    float* partial = static_cast<float*>(ws);
#define LP_HEAD_LAUNCH(CPT, EXACT) \
    hipLaunchKernelGGL((lp_head_kernel<CPT, EXACT>), dim3(blocks), dim3(256), 0, s, feat, lin_w, C, npix, partial)
    switch (C) {
    case 64: LP_HEAD_LAUNCH(8, true); break;
    case 128: LP_HEAD_LAUNCH(16, true); break;
    case 192: LP_HEAD_LAUNCH(24, true); break;
    case 256: LP_HEAD_LAUNCH(32, true); break;
    case 384: LP_HEAD_LAUNCH(48, true); break;
    case 512: LP_HEAD_LAUNCH(64, true); break;
    default: LP_HEAD_LAUNCH(LP_HEAD_CPT, false); break;       // same order of additions, the channel count read at run time
    }
#undef LP_HEAD_LAUNCH
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(lp_head_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)blocks, (float)npix, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_lpips_head(const float* feat, const float* lin_w, int32_t C, int32_t H, int32_t W, void* ws, size_t ws_bytes,
                                  float* out, gsr_stream_t stream_) {
    return lp_head(feat, lin_w, C, H, W, ws, ws_bytes, out, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- LP_FORWARD
// the five layer values, added in layer order
__global__ void lp_sum5_kernel(const float* __restrict__ layer, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = (((layer[0] + layer[1]) + layer[2]) + layer[3]) + layer[4];
}

struct LpConvSpec { int c_in, c_out, ks, stride, pad, pool_before, tap; };   // pool_before: window of the pool in front (0: none)
static const LpConvSpec LP_ALEX[5] = {
    {3, 64, 11, 4, 2, 0, 1}, {64, 192, 5, 1, 2, 3, 1}, {192, 384, 3, 1, 1, 3, 1}, {384, 256, 3, 1, 1, 0, 1}, {256, 256, 3, 1, 1, 0, 1}};
static const LpConvSpec LP_VGG[13] = {
    {3, 64, 3, 1, 1, 0, 0},    {64, 64, 3, 1, 1, 0, 1},
    {64, 128, 3, 1, 1, 2, 0},  {128, 128, 3, 1, 1, 0, 1},
    {128, 256, 3, 1, 1, 2, 0}, {256, 256, 3, 1, 1, 0, 0}, {256, 256, 3, 1, 1, 0, 1},
    {256, 512, 3, 1, 1, 2, 0}, {512, 512, 3, 1, 1, 0, 0}, {512, 512, 3, 1, 1, 0, 1},
    {512, 512, 3, 1, 1, 2, 0}, {512, 512, 3, 1, 1, 0, 0}, {512, 512, 3, 1, 1, 0, 1}};

static bool lp_net(int net, const LpConvSpec** spec, int* n_conv, int* min_size) {
    if (net == GSR_LPIPS_ALEX) { *spec = LP_ALEX; *n_conv = 5; *min_size = 31; return true; }
    if (net == GSR_LPIPS_VGG) { *spec = LP_VGG; *n_conv = 13; *min_size = 16; return true; }
    gsr_set_error("lpips: net %d is neither GSR_LPIPS_ALEX nor GSR_LPIPS_VGG", net);
    return false;
}

// two ping-pong activation buffers (the first layer's output is the largest map of either trunk: 64 channels at the first
// layer's resolution against at most 48 channels' worth of it later), the head's partials and the five layer values
struct LpLayout {
    size_t act_bytes, total;
    float *act[2], *partial, *layer;
    LpLayout(const LpConvSpec* spec, int H, int W, void* ws) {
        const int OH = lp_conv_out(H, spec[0].ks, spec[0].stride, spec[0].pad), OW = lp_conv_out(W, spec[0].ks, spec[0].stride, spec[0].pad);
        act_bytes = (size_t)2 * 64 * (size_t)(OH > 0 ? OH : 0) * (size_t)(OW > 0 ? OW : 0) * 4;
        GsrWsCursor c(ws);
        act[0] = c.take<float>(act_bytes);
        act[1] = c.take<float>(act_bytes);
        partial = c.take<float>(gsr_lpips_head_workspace_bytes());
        layer = c.take<float>(5 * 4);
        total = c.off;
    }
};

extern "C" size_t gsr_lpips_workspace_bytes(int32_t net, int32_t H, int32_t W) {
    const LpConvSpec* spec;
    int n_conv, min_size;
    if (!lp_net(net, &spec, &n_conv, &min_size) || H < 1 || W < 1) return 0;
    return LpLayout(spec, H, W, nullptr).total;
}

extern "C" int32_t gsr_lpips_forward(int32_t net, const float* const* conv_w_host, const float* const* conv_b_host,
                                     const float* const* lin_w_host, const float* img0, const float* img1, int32_t channels,
                                     int32_t H, int32_t W, void* ws, size_t ws_bytes, float* out, gsr_stream_t stream_) {
    const LpConvSpec* spec;
    int n_conv, min_size;
    if (!lp_net(net, &spec, &n_conv, &min_size)) return GSR_E_INVALID;
    if (channels != 3) { gsr_set_error("lpips: images must have 3 channels (got %d)", channels); return GSR_E_INVALID; }
    if (H < min_size || W < min_size) {
        gsr_set_error("lpips: a %dx%d image is below the %s trunk's minimum of %dx%d", H, W, net == GSR_LPIPS_VGG ? "vgg" : "alex",
                      min_size, min_size);
        return GSR_E_INVALID;
    }
    if (!img0 || !img1 || !out) { gsr_set_error("lpips: img0 / img1 / out is null"); return GSR_E_INVALID; }
    if (!conv_w_host || !conv_b_host || !lin_w_host) { gsr_set_error("lpips: a weight table is null"); return GSR_E_INVALID; }
    for (int l = 0; l < n_conv; ++l)
        if (!conv_w_host[l] || !conv_b_host[l]) { gsr_set_error("lpips: weight or bias of convolution %d is null", l); return GSR_E_INVALID; }
    for (int l = 0; l < 5; ++l)
        if (!lin_w_host[l]) { gsr_set_error("lpips: linear weight %d is null", l); return GSR_E_INVALID; }
    LpLayout lay(spec, H, W, ws);
    if (!ws || ws_bytes < lay.total) {
        gsr_set_error("ws_bytes: lpips workspace too small (%zu < %zu bytes)", ws_bytes, lay.total);
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const float* cur = img0;
    const float* cur1 = img1;          // only the two input images are separate allocations
    int cur_buf = 1, h = H, w = W, tap = 0;
    for (int l = 0; l < n_conv; ++l) {
        const LpConvSpec& c = spec[l];
        int rc;
        if (c.pool_before) {
            float* dst = lay.act[cur_buf ^ 1];
            if ((rc = lp_pool(cur, (int64_t)2 * c.c_in, h, w, c.pool_before, dst, s)) != GSR_OK) return rc;
            h = (h - c.pool_before) / 2 + 1;
            w = (w - c.pool_before) / 2 + 1;
            cur = dst;
            cur_buf ^= 1;
        }
        float* dst = lay.act[cur_buf ^ 1];
        if ((rc = lp_conv(cur, cur1, conv_w_host[l], conv_b_host[l], dst, 2, c.c_in, h, w, c.c_out, c.ks, c.stride, c.pad, l == 0, s)) !=
            GSR_OK)
            return rc;
        h = lp_conv_out(h, c.ks, c.stride, c.pad);
        w = lp_conv_out(w, c.ks, c.stride, c.pad);
        cur = dst;
        cur1 = nullptr;
        cur_buf ^= 1;
        // the head runs as soon as its layer exists: nothing but the two buffers is ever kept
        if (c.tap) {
            if ((rc = lp_head(cur, lin_w_host[tap], c.c_out, h, w, lay.partial, gsr_lpips_head_workspace_bytes(), lay.layer + tap, s)) !=
                GSR_OK)
                return rc;
            ++tap;
        }
    }
    hipLaunchKernelGGL(lp_sum5_kernel, dim3(1), dim3(64), 0, s, lay.layer, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
