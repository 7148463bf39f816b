// DN_LINEAR and DN_NORM (rules in include/gsr.h): the matrix product with a weight and the LayerNorm of every ViT in the tree
// (dino.hip, sam.hip, sam_decoder.hip, through vit_common.h).  fp16 operands on the 32x32x16 f16 matrix instruction with fp32
// accumulation; the epilogues and the LayerNorm statistics in fp32.  No split-K and no atomics: every output element is one
// k-ordered chain, so the bits are the same on every run and for a row alone or among others.
#include "vit_common.h"

// ---------------------------------------------------------------- DN_NORM
// One wave per row, fp32: mean = sum / n, var = sum (x - mean)^2 / n (biased), y = (x - mean) / sqrt(var + eps) * g + b.  A
// lane adds its elements c = lane, lane + 64, ... in order; the 64 lanes are added by a xor butterfly (32, 16, ..., 1).
template <typename OUT>
__global__ void __launch_bounds__(256) dn_norm_kernel(const float* __restrict__ x, int64_t rows, int hidden, int64_t in_stride,
                                                      const dn_half* __restrict__ g, const dn_half* __restrict__ beta, float eps,
                                                      OUT* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * in_stride;
    float s = 0.f;
    for (int c = lane; c < hidden; c += 64) s += xr[c];
    const float mean = wave_sum_f32(s) / (float)hidden;
    float v = 0.f;
    for (int c = lane; c < hidden; c += 64) {
        const float d = xr[c] - mean;
        v += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum_f32(v) / (float)hidden + eps);
    OUT* yr = y + row * hidden;
    for (int c = lane; c < hidden; c += 64) yr[c] = (OUT)((xr[c] - mean) * rstd * (float)g[c] + (float)beta[c]);
}

int dn_norm(const float* x, int64_t rows, int hidden, int64_t in_stride, const dn_half* g, const dn_half* b, float eps, void* y,
            int out_f32, hipStream_t s) {
    if (rows < 1 || hidden < 1 || in_stride < hidden) {
        gsr_set_error("dino norm: rows %lld and hidden %d must be >= 1 and the row stride %lld at least hidden", (long long)rows, hidden,
                      (long long)in_stride);
        return GSR_E_INVALID;
    }
    if (!x || !g || !b || !y) { gsr_set_error("dino norm: x / weight / bias / y is null"); return GSR_E_INVALID; }
    if ((rows + 3) / 4 > 0x7fffffffLL) { gsr_set_error("dino norm: too many rows"); return GSR_E_UNSUPPORTED; }
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (out_f32) hipLaunchKernelGGL(dn_norm_kernel<float>, grid, dim3(256), 0, s, x, rows, hidden, in_stride, g, b, eps, static_cast<float*>(y));
    else hipLaunchKernelGGL(dn_norm_kernel<dn_half>, grid, dim3(256), 0, s, x, rows, hidden, in_stride, g, b, eps, static_cast<dn_half*>(y));
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_dino_norm(const float* x, int64_t rows, int32_t hidden, int64_t in_stride, const void* weight,
                                 const void* bias, float eps, int32_t out_f32, void* y, gsr_stream_t stream_) {
    return dn_norm(x, rows, hidden, in_stride, static_cast<const dn_half*>(weight), static_cast<const dn_half*>(bias), eps, y, out_f32,
                   static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- the necks' cast and transpose (SV_NECK, HV_NECK)
__global__ void __launch_bounds__(256) vit_cast_kernel(const float* __restrict__ x, int64_t n, dn_half* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (dn_half)x[i];
}

// [T,C] -> [C,T]; ADD: plus add[c] (one fp32 addition)
template <bool ADD>
__global__ void __launch_bounds__(256) vit_transpose_kernel(const float* __restrict__ in, int64_t T, int Cn, const float* __restrict__ add,
                                                            float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * Cn) return;
    const int64_t c = i / T, tok = i - c * T;
    const float v = in[tok * Cn + c];
    out[i] = ADD ? v + add[c] : v;
}

int vit_cast(const float* x, int64_t n, dn_half* y, hipStream_t s) {
    hipLaunchKernelGGL(vit_cast_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, y);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

int vit_transpose(const float* in, int64_t T, int Cn, const float* add, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((T * Cn + 255) / 256));
    if (add) hipLaunchKernelGGL(vit_transpose_kernel<true>, grid, dim3(256), 0, s, in, T, Cn, add, out);
    else hipLaunchKernelGGL(vit_transpose_kernel<false>, grid, dim3(256), 0, s, in, T, Cn, add, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- DN_LINEAR
// D[m][n] = sum_k x[m][k] w[n][k]: both operands have k fastest, which is what the matrix instruction's A and B fragments want
// (lane l: 8 consecutive k of row l & 31, k = 8 (l >> 5) + j).  A workgroup of 4 waves owns 128 rows x 128 columns, a wave
// 2 x 2 tiles of 32 x 32; K (a multiple of 64) goes through LDS in chunks of 64 with the next chunk's global loads issued
// before the chunk's 64 matrix instructions.  Rows past M and columns past N are loaded as zeros and not written.
// TAIL (HV_LINEAR, K a multiple of 8 that is no multiple of 64): the 16-byte loads past K give zeros too, so the last chunk adds
// exact zeros to the chain.  K a multiple of 64 never takes the TAIL kernels: its code and its bits are what they were.
#define DN_BM 128
#define DN_KC 64
#define DN_LD 72        // halves per LDS row: 144 bytes, 16-byte aligned, consecutive rows 4 banks apart

template <int EPI, bool TAIL>
__global__ void __launch_bounds__(256) dn_linear_kernel(const dn_half* __restrict__ x, const dn_half* __restrict__ w,
                                                        const dn_half* __restrict__ bias, const dn_half* __restrict__ lam,
                                                        void* __restrict__ out_, int64_t M, int K, int N, int64_t Np, int T,
                                                        int prefix) {
    __shared__ __attribute__((aligned(16))) dn_half As[DN_BM * DN_LD];
    __shared__ __attribute__((aligned(16))) dn_half Bs[DN_BM * DN_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5, wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * DN_BM;
    const int n0 = (int)blockIdx.y * DN_BM;
    const int lc = t & 7, lr = t >> 3;          // a thread loads 16 bytes: columns 8 lc .. 8 lc + 7 of rows lr + 32 i
    uint4 ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t m = m0 + lr + 32 * i;
            const int n = n0 + lr + 32 * i;
            const bool kin = !TAIL || k0 + 8 * lc < K;
            ra[i] = m < M && kin ? *reinterpret_cast<const uint4*>(x + m * K + k0 + 8 * lc) : make_uint4(0, 0, 0, 0);
            rb[i] = n < N && kin ? *reinterpret_cast<const uint4*>(w + (int64_t)n * K + k0 + 8 * lc) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<uint4*>(&As[(lr + 32 * i) * DN_LD + 8 * lc]) = ra[i];
            *reinterpret_cast<uint4*>(&Bs[(lr + 32 * i) * DN_LD + 8 * lc]) = rb[i];
        }
    };
    vit_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    load(0);
    for (int k0 = 0; k0 < K; k0 += DN_KC) {
        __syncthreads();            // the previous chunk's reads are done
        store();
        __syncthreads();
        if (k0 + DN_KC < K) load(k0 + DN_KC);
#pragma unroll
        for (int ks = 0; ks < DN_KC / 16; ++ks) {
            vit_h8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const vit_h8*>(&As[(wm * 64 + i * 32 + r) * DN_LD + ks * 16 + 8 * h]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const vit_h8*>(&Bs[(wn * 64 + j * 32 + r) * DN_LD + ks * 16 + 8 * h]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // C/D map: column = lane & 31 (n), row = vit_acc_row(reg, lane >> 5) (m)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + r;
        if (n >= N) continue;
        const float bn = bias ? (float)bias[n] : 0.f;
        const float ln = EPI == DN_EPI_RESID ? (float)lam[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t m = m0 + wm * 64 + i * 32 + vit_acc_row(q, h);
                if (m >= M) continue;
                const float v = acc[i][j][q] + bn;
                if (EPI == DN_EPI_BIAS) {
                    static_cast<dn_half*>(out_)[m * N + n] = (dn_half)v;
                } else if (EPI == DN_EPI_GELU) {
                    static_cast<dn_half*>(out_)[m * N + n] = (dn_half)vit_gelu(v);
                } else if (EPI == DN_EPI_RESID) {
                    float* o = static_cast<float*>(out_) + m * N + n;
                    *o = fmaf(ln, v, *o);
                } else if (EPI == DN_EPI_RESID1) {      // SAM: no LayerScale, resid += acc + bias (one fp32 addition after the bias's)
                    float* o = static_cast<float*>(out_) + m * N + n;
                    *o = *o + v;
                } else if (EPI == DN_EPI_F32) {         // SAM's neck: acc + bias stored as fp32
                    static_cast<float*>(out_)[m * N + n] = v;
                } else if (EPI == DN_EPI_POS) {         // SAM's embedding: (acc + bias) + fp32(pos[m][n]), stored as fp32
                    static_cast<float*>(out_)[m * N + n] = v + (float)lam[m * N + n];
                } else if (EPI == DN_EPI_SKIP_GELU) {   // SAM2's up-scaling: one fp32 addition after the bias's, then the GELU
                    const float skip = reinterpret_cast<const float*>(lam)[(m % Np) * N + n];
                    static_cast<dn_half*>(out_)[m * N + n] = (dn_half)vit_gelu(v + skip);
                } else {                                // DN_EPI_EMBED
                    const int64_t b = m / Np, p = m - b * Np;
                    static_cast<float*>(out_)[(b * T + prefix + p) * N + n] = v;
                }
            }
        }
    }
}

// the checks that DN_LINEAR and HV_LINEAR share, and the launch; K is checked by the two callers
static int dn_linear_launch(const dn_half* x, const dn_half* w, const dn_half* bias, const dn_half* lam, void* out, int64_t M, int K,
                            int N, int epi, hipStream_t s, DnEmbedRows embed) {
    if (!x || !w || !out) { gsr_set_error("dino linear: x / w / out is null"); return GSR_E_INVALID; }
    if ((epi == DN_EPI_RESID || epi == DN_EPI_POS || epi == DN_EPI_SKIP_GELU) && !lam) { gsr_set_error("dino linear: the residual epilogue needs lambda"); return GSR_E_INVALID; }
    if (epi == DN_EPI_SKIP_GELU && embed.Np < 1) { gsr_set_error("dino linear: the skip epilogue needs the rows of its table"); return GSR_E_INVALID; }
    if ((M + DN_BM - 1) / DN_BM > 0x7fffffffLL || (N + DN_BM - 1) / DN_BM > 65535) {
        gsr_set_error("dino linear: M %lld or N %d exceeds the launch grid", (long long)M, N);
        return GSR_E_UNSUPPORTED;
    }
    const dim3 grid((unsigned)((M + DN_BM - 1) / DN_BM), (unsigned)((N + DN_BM - 1) / DN_BM));
    const bool tail = K % DN_KC != 0;
#define DN_LINEAR_LAUNCH(E)                                                                                                              \
    do {                                                                                                                                 \
        if (tail) hipLaunchKernelGGL((dn_linear_kernel<E, true>), grid, dim3(256), 0, s, x, w, bias, lam, out, M, K, N, embed.Np, embed.T, embed.prefix); \
        else hipLaunchKernelGGL((dn_linear_kernel<E, false>), grid, dim3(256), 0, s, x, w, bias, lam, out, M, K, N, embed.Np, embed.T, embed.prefix);     \
    } while (0)
    switch (epi) {
    case DN_EPI_BIAS: DN_LINEAR_LAUNCH(DN_EPI_BIAS); break;
    case DN_EPI_GELU: DN_LINEAR_LAUNCH(DN_EPI_GELU); break;
    case DN_EPI_RESID: DN_LINEAR_LAUNCH(DN_EPI_RESID); break;
    case DN_EPI_EMBED: DN_LINEAR_LAUNCH(DN_EPI_EMBED); break;
    case DN_EPI_RESID1: DN_LINEAR_LAUNCH(DN_EPI_RESID1); break;
    case DN_EPI_F32: DN_LINEAR_LAUNCH(DN_EPI_F32); break;
    case DN_EPI_POS: DN_LINEAR_LAUNCH(DN_EPI_POS); break;
    case DN_EPI_SKIP_GELU: DN_LINEAR_LAUNCH(DN_EPI_SKIP_GELU); break;
    default: gsr_set_error("dino linear: epilogue %d is not one of GSR_DINO_EPI_*", epi); return GSR_E_INVALID;
    }
#undef DN_LINEAR_LAUNCH
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

int dn_linear(const dn_half* x, const dn_half* w, const dn_half* bias, const dn_half* lam, void* out, int64_t M, int K, int N,
              int epi, hipStream_t s, DnEmbedRows embed) {
    if (M < 1 || K < 64 || N < 1 || K % 64 != 0) {
        gsr_set_error("dino linear: M %lld and N %d must be >= 1 and K %d a positive multiple of 64", (long long)M, N, K);
        return GSR_E_INVALID;
    }
    return dn_linear_launch(x, w, bias, lam, out, M, K, N, epi, s, embed);
}

// HV_LINEAR: DN_LINEAR for any K that is a multiple of 8 (a row of 8 halves is one 16-byte load)
int dn_linear_k8(const dn_half* x, const dn_half* w, const dn_half* bias, const dn_half* lam, void* out, int64_t M, int K, int N,
                 int epi, hipStream_t s) {
    if (M < 1 || K < 8 || N < 1 || K % 8 != 0) {
        gsr_set_error("sam2 linear: M %lld and N %d must be >= 1 and K %d a positive multiple of 8", (long long)M, N, K);
        return GSR_E_INVALID;
    }
    return dn_linear_launch(x, w, bias, lam, out, M, K, N, epi, s, {1, 0, 0});
}

extern "C" int32_t gsr_dino_linear(const void* x, const void* w, const void* bias, const void* lambda, int64_t M, int32_t K,
                                   int32_t N, int32_t epilogue, void* out, gsr_stream_t stream_) {
    if (epilogue < DN_EPI_BIAS || epilogue > DN_EPI_RESID) {
        gsr_set_error("dino linear: epilogue %d is not one of GSR_DINO_EPI_*", epilogue);
        return GSR_E_INVALID;
    }
    return dn_linear(static_cast<const dn_half*>(x), static_cast<const dn_half*>(w), static_cast<const dn_half*>(bias),
                     static_cast<const dn_half*>(lambda), out, M, K, N, epilogue, static_cast<hipStream_t>(stream_));
}
