// DINOv3 ViT encoder (transformers' DINOv3ViTModel, inference only) as kernels: fp16 operands on the 32x32x16 f16 matrix
// instruction with fp32 accumulation; the residual stream, the LayerNorm statistics, the softmax and the input normalisation
// in fp32.  (The reference's .half() model keeps the residual stream in fp16; this one deliberately does not.)  The rules
// are in include/gsr.h (DN_EMBED, DN_NORM, DN_LINEAR, DN_ROPE, DN_ATTN, DN_POOL, DN_COS); each has one named place below.
// No split-K and no atomics: every output element is one k-ordered chain, so the bits are the same on every run and for an
// image alone or inside a batch.
#include "cloud_common.h"
#include "dino_internal.h"

typedef _Float16 dn_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 dn_h4 __attribute__((ext_vector_type(4)));
typedef float dn_f32x16 __attribute__((ext_vector_type(16)));

#define DN_PATCH 16
#define DN_PATCH_K (3 * DN_PATCH * DN_PATCH)
#define DN_HEAD 64
#define DN_MAX_BATCH 8

// row of a 32x32 accumulator held in register `reg` of a lane of half `h` (the column is lane & 31)
__device__ __forceinline__ int dn_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ---------------------------------------------------------------- DN_EMBED (gather)
// patches[b Np + p][c 256 + ky 16 + kx] = fp16((x[b,c,16 py + ky,16 px + kx] - mean[c]) / std[c]): the subtraction and the true
// division in fp32, one rounding to fp16.  A thread writes the 8 kx of half a patch row.  Rows and columns past 16 Hp, 16 Wp
// are never read.
__global__ void __launch_bounds__(256) dn_im2col_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int B, int H,
                                                        int W, int Hp, int Wp, float m0, float m1, float m2, float s0, float s1,
                                                        float s2, dn_half* __restrict__ patches) {
    const int64_t Np = (int64_t)Hp * Wp, n = (int64_t)B * Np * (DN_PATCH_K / 8);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t row = i / (DN_PATCH_K / 8);
    const int part = (int)(i - row * (DN_PATCH_K / 8));
    const int c = part >> 5, ky = (part >> 1) & 15, kx0 = (part & 1) * 8;
    const int b = (int)(row / Np);
    const int64_t p = row - (int64_t)b * Np;
    const int py = (int)(p / Wp), px = (int)(p - (int64_t)py * Wp);
    const float* img = b == 0 ? x0 : x1 + (int64_t)(b - 1) * 3 * H * W;
    const float* src = img + ((int64_t)c * H + (py * DN_PATCH + ky)) * W + px * DN_PATCH + kx0;
    const float mean = c == 0 ? m0 : c == 1 ? m1 : m2, sd = c == 0 ? s0 : c == 1 ? s1 : s2;
    dn_h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (dn_half)((src[e] - mean) / sd);
    *reinterpret_cast<dn_h8*>(patches + row * DN_PATCH_K + part * 8) = v;
}

// CLS and register rows of the residual stream: copied from the weights (fp16 -> fp32, exact)
__global__ void __launch_bounds__(256) dn_prefix_kernel(const dn_half* __restrict__ cls, const dn_half* __restrict__ reg, int B,
                                                        int T, int prefix, int hidden, float* __restrict__ out) {
    const int64_t n = (int64_t)B * prefix * hidden;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % hidden);
    const int64_t bt = i / hidden;
    const int tk = (int)(bt % prefix), b = (int)(bt / prefix);
    out[((int64_t)b * T + tk) * hidden + c] = tk == 0 ? (float)cls[c] : (float)reg[(int64_t)(tk - 1) * hidden + c];
}

// ---------------------------------------------------------------- DN_NORM
// One wave per row, fp32: mean = sum / n, var = sum (x - mean)^2 / n (biased), y = (x - mean) / sqrt(var + eps) * g + b.  A
// lane adds its elements c = lane, lane + 64, ... in order; the 64 lanes are added by a xor butterfly (32, 16, ..., 1).
__device__ __forceinline__ float dn_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

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
    const float mean = dn_wave_sum(s) / (float)hidden;
    float v = 0.f;
    for (int c = lane; c < hidden; c += 64) {
        const float d = xr[c] - mean;
        v += d * d;
    }
    const float rstd = 1.0f / sqrtf(dn_wave_sum(v) / (float)hidden + eps);
    OUT* yr = y + row * hidden;
    for (int c = lane; c < hidden; c += 64) yr[c] = (OUT)((xr[c] - mean) * rstd * (float)g[c] + (float)beta[c]);
}

// ---------------------------------------------------------------- DN_LINEAR
// D[m][n] = sum_k x[m][k] w[n][k]: both operands have k fastest, which is what the matrix instruction's A and B fragments want
// (lane l: 8 consecutive k of row l & 31, k = 8 (l >> 5) + j).  A workgroup of 4 waves owns 128 rows x 128 columns, a wave
// 2 x 2 tiles of 32 x 32; K (a multiple of 64) goes through LDS in chunks of 64 with the next chunk's global loads issued
// before the chunk's 64 matrix instructions.  Rows past M and columns past N are loaded as zeros and not written.
#define DN_BM 128
#define DN_KC 64
#define DN_LD 72        // halves per LDS row: 144 bytes, 16-byte aligned, consecutive rows 4 banks apart
// the epilogue values DN_EPI_* are in dino_internal.h (sam.hip launches this kernel too)

template <int EPI>
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
            ra[i] = m < M ? *reinterpret_cast<const uint4*>(x + m * K + k0 + 8 * lc) : make_uint4(0, 0, 0, 0);
            rb[i] = n < N ? *reinterpret_cast<const uint4*>(w + (int64_t)n * K + k0 + 8 * lc) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<uint4*>(&As[(lr + 32 * i) * DN_LD + 8 * lc]) = ra[i];
            *reinterpret_cast<uint4*>(&Bs[(lr + 32 * i) * DN_LD + 8 * lc]) = rb[i];
        }
    };
    dn_f32x16 acc[2][2];
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
            dn_h8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const dn_h8*>(&As[(wm * 64 + i * 32 + r) * DN_LD + ks * 16 + 8 * h]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const dn_h8*>(&Bs[(wn * 64 + j * 32 + r) * DN_LD + ks * 16 + 8 * h]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // C/D map: column = lane & 31 (n), row = dn_acc_row(reg, lane >> 5) (m)
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
                const int64_t m = m0 + wm * 64 + i * 32 + dn_acc_row(q, h);
                if (m >= M) continue;
                const float v = acc[i][j][q] + bn;
                if (EPI == DN_EPI_BIAS) {
                    static_cast<dn_half*>(out_)[m * N + n] = (dn_half)v;
                } else if (EPI == DN_EPI_GELU) {
                    static_cast<dn_half*>(out_)[m * N + n] = (dn_half)(0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)));
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
                } else {
                    const int64_t b = m / Np, p = m - b * Np;
                    static_cast<float*>(out_)[(b * T + prefix + p) * N + n] = v;
                }
            }
        }
    }
}

int dn_linear(const dn_half* x, const dn_half* w, const dn_half* bias, const dn_half* lam, void* out, int64_t M, int K, int N,
              int epi, int64_t Np, int T, int prefix, hipStream_t s) {
    if (M < 1 || K < 64 || N < 1 || K % 64 != 0) {
        gsr_set_error("dino linear: M %lld and N %d must be >= 1 and K %d a positive multiple of 64", (long long)M, N, K);
        return GSR_E_INVALID;
    }
    if (!x || !w || !out) { gsr_set_error("dino linear: x / w / out is null"); return GSR_E_INVALID; }
    if ((epi == DN_EPI_RESID || epi == DN_EPI_POS) && !lam) { gsr_set_error("dino linear: the residual epilogue needs lambda"); return GSR_E_INVALID; }
    if ((M + DN_BM - 1) / DN_BM > 0x7fffffffLL || (N + DN_BM - 1) / DN_BM > 65535) {
        gsr_set_error("dino linear: M %lld or N %d exceeds the launch grid", (long long)M, N);
        return GSR_E_UNSUPPORTED;
    }
    const dim3 grid((unsigned)((M + DN_BM - 1) / DN_BM), (unsigned)((N + DN_BM - 1) / DN_BM));
#define DN_LINEAR_LAUNCH(E) hipLaunchKernelGGL((dn_linear_kernel<E>), grid, dim3(256), 0, s, x, w, bias, lam, out, M, K, N, Np, T, prefix)
    switch (epi) {
    case DN_EPI_BIAS: DN_LINEAR_LAUNCH(DN_EPI_BIAS); break;
    case DN_EPI_GELU: DN_LINEAR_LAUNCH(DN_EPI_GELU); break;
    case DN_EPI_RESID: DN_LINEAR_LAUNCH(DN_EPI_RESID); break;
    case DN_EPI_EMBED: DN_LINEAR_LAUNCH(DN_EPI_EMBED); break;
    case DN_EPI_RESID1: DN_LINEAR_LAUNCH(DN_EPI_RESID1); break;
    case DN_EPI_F32: DN_LINEAR_LAUNCH(DN_EPI_F32); break;
    case DN_EPI_POS: DN_LINEAR_LAUNCH(DN_EPI_POS); break;
    default: gsr_set_error("dino linear: epilogue %d is not one of GSR_DINO_EPI_*", epi); return GSR_E_INVALID;
    }
#undef DN_LINEAR_LAUNCH
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_dino_linear(const void* x, const void* w, const void* bias, const void* lambda, int64_t M, int32_t K,
                                   int32_t N, int32_t epilogue, void* out, gsr_stream_t stream_) {
    if (epilogue < DN_EPI_BIAS || epilogue > DN_EPI_RESID) {
        gsr_set_error("dino linear: epilogue %d is not one of GSR_DINO_EPI_*", epilogue);
        return GSR_E_INVALID;
    }
    return dn_linear(static_cast<const dn_half*>(x), static_cast<const dn_half*>(w), static_cast<const dn_half*>(bias),
                     static_cast<const dn_half*>(lambda), out, M, K, N, epilogue, 1, 0, 0, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- shared argument checks
static int dn_check_cfg(const GsrDinoConfig* c) {
    if (!c) { gsr_set_error("dino: cfg is null"); return GSR_E_INVALID; }
    if (c->heads < 1 || c->hidden != DN_HEAD * c->heads) {
        gsr_set_error("dino: hidden %d is not 64 * heads (%d heads; the head dimension is fixed at 64)", c->hidden, c->heads);
        return GSR_E_INVALID;
    }
    if (c->layers < 1) { gsr_set_error("dino: layers %d must be >= 1", c->layers); return GSR_E_INVALID; }
    if (c->intermediate < 64 || c->intermediate % 64 != 0) {
        gsr_set_error("dino: intermediate %d is not a positive multiple of 64", c->intermediate);
        return GSR_E_INVALID;
    }
    if (c->registers < 0) { gsr_set_error("dino: registers %d must be >= 0", c->registers); return GSR_E_INVALID; }
    if (!(c->rope_theta > 0.f) || !(c->ln_eps >= 0.f)) { gsr_set_error("dino: rope_theta must be > 0 and ln_eps >= 0"); return GSR_E_INVALID; }
    for (int i = 0; i < 3; ++i)
        if (!(c->image_std[i] > 0.f)) { gsr_set_error("dino: image_std[%d] must be > 0", i); return GSR_E_INVALID; }
    return GSR_OK;
}

static int dn_check_image(int B, int H, int W) {
    if (B < 1 || B > DN_MAX_BATCH) { gsr_set_error("dino: B %d is outside 1 .. %d", B, DN_MAX_BATCH); return GSR_E_INVALID; }
    if (H < DN_PATCH || W < DN_PATCH) { gsr_set_error("dino: a %dx%d image is below one 16x16 patch", H, W); return GSR_E_INVALID; }
    if ((int64_t)(H / DN_PATCH) * (W / DN_PATCH) > (1 << 24)) { gsr_set_error("dino: a %dx%d image has too many patches", H, W); return GSR_E_UNSUPPORTED; }
    return GSR_OK;
}

// ---------------------------------------------------------------- DN_EMBED
static int dn_embed(const GsrDinoConfig* c, const float* x0, const float* x1, int B, int H, int W, const dn_half* cls,
                    const dn_half* reg, const dn_half* pw, const dn_half* pb, dn_half* patches, float* out, hipStream_t s) {
    const int Hp = H / DN_PATCH, Wp = W / DN_PATCH, prefix = 1 + c->registers;
    const int64_t Np = (int64_t)Hp * Wp;
    const int T = (int)(prefix + Np);
    if (!x1) x1 = x0 + (int64_t)3 * H * W;
    const int64_t n_gather = (int64_t)B * Np * (DN_PATCH_K / 8);
    hipLaunchKernelGGL(dn_im2col_kernel, dim3((unsigned)((n_gather + 255) / 256)), dim3(256), 0, s, x0, x1, B, H, W, Hp, Wp,
                       c->image_mean[0], c->image_mean[1], c->image_mean[2], c->image_std[0], c->image_std[1], c->image_std[2], patches);
    GSR_LAUNCH_CHECK();
    const int64_t n_prefix = (int64_t)B * prefix * c->hidden;
    hipLaunchKernelGGL(dn_prefix_kernel, dim3((unsigned)((n_prefix + 255) / 256)), dim3(256), 0, s, cls, reg, B, T, prefix, c->hidden, out);
    GSR_LAUNCH_CHECK();
    return dn_linear(patches, pw, pb, nullptr, out, (int64_t)B * Np, DN_PATCH_K, c->hidden, DN_EPI_EMBED, Np, T, prefix, s);
}

extern "C" size_t gsr_dino_embed_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B < 1 || H < DN_PATCH || W < DN_PATCH) return 0;
    return gsr_align((size_t)B * (size_t)(H / DN_PATCH) * (size_t)(W / DN_PATCH) * DN_PATCH_K * 2);
}

extern "C" int32_t gsr_dino_embed(const GsrDinoConfig* cfg, const float* x0, const float* x1, int32_t B, int32_t H, int32_t W,
                                  const void* cls, const void* reg, const void* patch_w, const void* patch_b, void* ws,
                                  size_t ws_bytes, float* out, gsr_stream_t stream_) {
    int rc;
    if ((rc = dn_check_cfg(cfg)) != GSR_OK || (rc = dn_check_image(B, H, W)) != GSR_OK) return rc;
    if (!x0 || !cls || !patch_w || !out || (cfg->registers > 0 && !reg)) {
        gsr_set_error("dino embed: x0 / cls / reg / patch_w / out is null");
        return GSR_E_INVALID;
    }
    if (!ws || ws_bytes < gsr_dino_embed_workspace_bytes(B, H, W)) {
        gsr_set_error("ws_bytes: dino embed workspace too small (%zu < %zu bytes)", ws_bytes, gsr_dino_embed_workspace_bytes(B, H, W));
        return GSR_E_INVALID;
    }
    return dn_embed(cfg, x0, x1, B, H, W, static_cast<const dn_half*>(cls), static_cast<const dn_half*>(reg),
                    static_cast<const dn_half*>(patch_w), static_cast<const dn_half*>(patch_b), static_cast<dn_half*>(ws), out,
                    static_cast<hipStream_t>(stream_));
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

// ---------------------------------------------------------------- DN_ROPE
// In place on the patch tokens of q and k (fp16 [B,T,64 heads]); a thread takes the pair (i, i + 32) of one head of one token.
// fp32: coord = 2 ((idx + 0.5) / n) - 1, inv_freq = theta^(-j / 16), angle = 2 pi coord inv_freq; i < 16 is the y coordinate with
// j = i, 16 <= i < 32 the x coordinate with j = i - 16; out[i] = q[i] cos - q[i + 32] sin, out[i + 32] = q[i + 32] cos + q[i] sin
// (two products and one addition each, in fp32), one rounding to fp16.
__global__ void __launch_bounds__(256) dn_rope_kernel(dn_half* __restrict__ q, dn_half* __restrict__ k, int B, int T, int heads,
                                                      int Hp, int Wp, float theta) {
    const int64_t Np = (int64_t)Hp * Wp, n = (int64_t)B * Np * heads * 32;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int i = (int)(idx & 31);
    int64_t rest = idx >> 5;
    const int head = (int)(rest % heads);
    rest /= heads;
    const int64_t p = rest % Np;
    const int b = (int)(rest / Np);
    const int py = (int)(p / Wp), px = (int)(p - (int64_t)py * Wp);
    const float coord = i < 16 ? 2.0f * (((float)py + 0.5f) / (float)Hp) - 1.0f : 2.0f * (((float)px + 0.5f) / (float)Wp) - 1.0f;
    const float inv_freq = 1.0f / powf(theta, (float)(i & 15) * 0.0625f);
    const float angle = 6.283185307179586f * coord * inv_freq;
    const float cs = cosf(angle), sn = sinf(angle);
    const int64_t at = ((int64_t)b * T + (T - Np) + p) * ((int64_t)heads * DN_HEAD) + head * DN_HEAD + i;
    dn_half* both[2] = {q, k};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        if (!both[w]) continue;
        const float lo = (float)both[w][at], hi = (float)both[w][at + 32];
        both[w][at] = (dn_half)(lo * cs - hi * sn);
        both[w][at + 32] = (dn_half)(hi * cs + lo * sn);
    }
}

static int dn_rope(dn_half* q, dn_half* k, int B, int T, int heads, int Hp, int Wp, float theta, hipStream_t s) {
    if (B < 1 || heads < 1 || Hp < 1 || Wp < 1 || (int64_t)Hp * Wp > T) {
        gsr_set_error("dino rope: B %d, heads %d, Hp %d, Wp %d must be >= 1 and Hp Wp <= T (%d)", B, heads, Hp, Wp, T);
        return GSR_E_INVALID;
    }
    if (!q && !k) { gsr_set_error("dino rope: q and k are both null"); return GSR_E_INVALID; }
    if (!(theta > 0.f)) { gsr_set_error("dino rope: theta must be > 0"); return GSR_E_INVALID; }
    const int64_t n = (int64_t)B * Hp * Wp * heads * 32;
    if ((n + 255) / 256 > 0x7fffffffLL) { gsr_set_error("dino rope: too many elements"); return GSR_E_UNSUPPORTED; }
    hipLaunchKernelGGL(dn_rope_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q, k, B, T, heads, Hp, Wp, theta);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_dino_rope(void* q, void* k, int32_t B, int32_t T, int32_t heads, int32_t Hp, int32_t Wp, float theta,
                                 gsr_stream_t stream_) {
    return dn_rope(static_cast<dn_half*>(q), static_cast<dn_half*>(k), B, T, heads, Hp, Wp, theta, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- DN_ATTN
// One pass, flash style.  A workgroup of 4 waves owns 128 query rows of one head, a wave 32 of them; K and V go through LDS in
// tiles of 64 rows (V transposed on the way in), the next tile's global loads issued before the tile's matrix instructions.
// The first product is S^T = K Q^T (A = K, B = Q^T, Q's four fragments stay in registers): the result has the query on the
// lane and the kv index in the registers, so the maximum and the sum of a query's row are per-lane loops plus one exchange
// between the lane halves, and P^T (rounded to fp16) is the B operand of O^T = V^T P^T as it lies: no lane movement, no LDS.
// The k order of that second product is the accumulator's row order (dn_acc_row), which the V^T fragment follows.
// The scores are kept in base 2 (one fp32 product with log2(e) / 8), so p = 2^(t - m) is one v_exp_f32.
// Rows of K and V past T are never read; their scores are -inf before the maximum.  Query rows past T are not written.
#define DA_BQ 128
#define DA_BKV 64
#define DA_LDV 68       // halves per row of the V^T image: 136 bytes (8-byte aligned reads), the paired stores 2 to a bank
#define DA_LOG2E_8 0.18033688011112042592f      // log2(e) / 8: the scores are kept in base 2, p = 2^(s2 - m2) is one v_exp_f32

__global__ void __launch_bounds__(256) dn_attn_kernel(const dn_half* __restrict__ q, const dn_half* __restrict__ k,
                                                      const dn_half* __restrict__ v, dn_half* __restrict__ o, int T, int hidden) {
    __shared__ __attribute__((aligned(16))) dn_half Ks[DA_BKV * DN_LD];       // [kv][d]
    __shared__ __attribute__((aligned(16))) dn_half Vt[DN_HEAD * DA_LDV];     // [d][kv]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int64_t base = (int64_t)blockIdx.z * T * hidden + (int64_t)blockIdx.y * DN_HEAD;
    const int qrow = (int)blockIdx.x * DA_BQ + wave * 32 + r;
    dn_h8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        if (qrow < T) qf[ks] = *reinterpret_cast<const dn_h8*>(q + base + (int64_t)qrow * hidden + ks * 16 + 8 * h);
        else
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[ks][e] = (dn_half)0.f;
    }
    dn_f32x16 acc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[dt][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int lc = t & 7, lr = t >> 3;      // a thread loads columns 8 lc .. 8 lc + 7 of the two adjacent rows 2 lr, 2 lr + 1
    uint4 rk[2], rv[2];
    auto load = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = kv0 + 2 * lr + i;
            const int64_t off = base + (int64_t)row * hidden + 8 * lc;
            rk[i] = row < T ? *reinterpret_cast<const uint4*>(k + off) : make_uint4(0, 0, 0, 0);
            rv[i] = row < T ? *reinterpret_cast<const uint4*>(v + off) : make_uint4(0, 0, 0, 0);
        }
    };
    load(0);
    for (int kv0 = 0; kv0 < T; kv0 += DA_BKV) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(&Ks[(2 * lr + i) * DN_LD + 8 * lc]) = rk[i];
        {   // V transposed: the two rows' values of one d are neighbours in V^T, one 4-byte store per d
            const dn_h8 v0 = *reinterpret_cast<const dn_h8*>(&rv[0]), v1 = *reinterpret_cast<const dn_h8*>(&rv[1]);
            typedef _Float16 dn_h2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                dn_h2 pr;
                pr[0] = v0[e];
                pr[1] = v1[e];
                *reinterpret_cast<dn_h2*>(&Vt[(8 * lc + e) * DA_LDV + 2 * lr]) = pr;
            }
        }
        __syncthreads();
        if (kv0 + DA_BKV < T) load(kv0 + DA_BKV);

        dn_f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kb][e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const dn_h8 a = *reinterpret_cast<const dn_h8*>(&Ks[(kb * 32 + r) * DN_LD + ks * 16 + 8 * h]);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[ks], s[kb], 0, 0, 0);
            }
        }
        const bool tail = kv0 + DA_BKV > T;
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float sv = s[kb][e] * DA_LOG2E_8;
                if (tail && kv0 + kb * 32 + dn_acc_row(e, h) >= T) sv = -INFINITY;
                s[kb][e] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);           // finite: kv0 < T, so row kv0 of this tile is valid
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __builtin_amdgcn_exp2f(s[kb][e] - m_new);
                s[kb][e] = p;
                psum += p;
            }
        psum += __shfl_xor(psum, 32, 64);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[dt][e] *= alpha;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                dn_h8 pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (dn_half)s[kb][8 * ss + e];
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    // element j of half h is kv 16 ss + 8 (j >> 2) + 4 h + (j & 3) of the block: two runs of 4 consecutive kv
                    const dn_half* vp = &Vt[(dt * 32 + r) * DA_LDV + kb * 32 + ss * 16 + 4 * h];
                    const dn_h4 lo = *reinterpret_cast<const dn_h4*>(vp), hi = *reinterpret_cast<const dn_h4*>(vp + 8);
                    dn_h8 a;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = lo[e]; a[4 + e] = hi[e]; }
                    acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf, acc[dt], 0, 0, 0);
                }
            }
    }
    if (qrow >= T) return;
    dn_half* orow = o + base + (int64_t)qrow * hidden;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            dn_h4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = (dn_half)(acc[dt][4 * g + e] / l_run);
            *reinterpret_cast<dn_h4*>(orow + dt * 32 + 8 * g + 4 * h) = out;
        }
}

static int dn_attn(const dn_half* q, const dn_half* k, const dn_half* v, dn_half* o, int B, int T, int heads, hipStream_t s) {
    if (B < 1 || B > 65535 || T < 1 || heads < 1 || heads > 65535) {
        gsr_set_error("dino attn: B %d, T %d and heads %d must be >= 1 (B, heads <= 65535)", B, T, heads);
        return GSR_E_INVALID;
    }
    if (!q || !k || !v || !o) { gsr_set_error("dino attn: q / k / v / out is null"); return GSR_E_INVALID; }
    hipLaunchKernelGGL(dn_attn_kernel, dim3((unsigned)((T + DA_BQ - 1) / DA_BQ), (unsigned)heads, (unsigned)B), dim3(256), 0, s, q, k, v, o,
                       T, heads * DN_HEAD);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_dino_attn(const void* q, const void* k, const void* v, int32_t B, int32_t T, int32_t heads, void* out,
                                 gsr_stream_t stream_) {
    return dn_attn(static_cast<const dn_half*>(q), static_cast<const dn_half*>(k), static_cast<const dn_half*>(v),
                   static_cast<dn_half*>(out), B, T, heads, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- DN_COS
// One workgroup, fp32: thread t adds the products of elements t, t + 256, ... in order, gsr_block_sum_256 adds the threads;
// out = lambda16 * (dot / (max(sqrt(aa), 1e-8) * max(sqrt(bb), 1e-8))).
__global__ void __launch_bounds__(256) dn_cos_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, float lambda16,
                                                     float* __restrict__ out) {
    __shared__ float s_sum[3 * 256];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += 256) {
        const float x = a[i], y = b[i];
        acc[0] += x * y;
        acc[1] += x * x;
        acc[2] += y * y;
    }
    gsr_block_sum_256<float, 3>(acc, s_sum);
    if (threadIdx.x == 0) *out = lambda16 * (acc[0] / (fmaxf(sqrtf(acc[1]), 1e-8f) * fmaxf(sqrtf(acc[2]), 1e-8f)));
}

extern "C" int32_t gsr_dino_cosine(const float* a, const float* b, int32_t n, float lambda16, float* out, gsr_stream_t stream_) {
    if (n < 1) { gsr_set_error("dino cosine: n %d must be >= 1", n); return GSR_E_INVALID; }
    if (!a || !b || !out) { gsr_set_error("dino cosine: a / b / out is null"); return GSR_E_INVALID; }
    hipLaunchKernelGGL(dn_cos_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream_), a, b, n, lambda16, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

// ---------------------------------------------------------------- the whole encoder (DN_POOL at its end)
struct DnLayout {
    int Hp, Wp, T;
    int64_t M;
    size_t total;
    float* resid;
    dn_half *xn, *q, *k, *v, *att, *mlp, *patches;
    DnLayout(const GsrDinoConfig* c, int B, int H, int W, void* ws) {
        Hp = H / DN_PATCH;
        Wp = W / DN_PATCH;
        T = 1 + c->registers + Hp * Wp;
        M = (int64_t)B * T;
        const size_t row = (size_t)M * c->hidden;
        GsrWsCursor cur(ws);
        resid = cur.take<float>(row * 4);
        xn = cur.take<dn_half>(row * 2);
        q = cur.take<dn_half>(row * 2);
        k = cur.take<dn_half>(row * 2);
        v = cur.take<dn_half>(row * 2);
        att = cur.take<dn_half>(row * 2);
        mlp = cur.take<dn_half>((size_t)M * c->intermediate * 2);
        patches = cur.take<dn_half>((size_t)B * Hp * Wp * DN_PATCH_K * 2);
        total = cur.off;
    }
};

extern "C" size_t gsr_dino_workspace_bytes(const GsrDinoConfig* cfg, int32_t B, int32_t H, int32_t W) {
    if (dn_check_cfg(cfg) != GSR_OK || dn_check_image(B, H, W) != GSR_OK) return 0;
    return DnLayout(cfg, B, H, W, nullptr).total;
}

extern "C" int32_t gsr_dino_num_weights(int32_t layers) { return layers < 1 ? 0 : GSR_DINO_W_LAYER0 + GSR_DINO_W_PER_LAYER * layers + 2; }

extern "C" int32_t gsr_dino_forward(const GsrDinoConfig* cfg, const void* const* weights_host, int32_t n_weights, const float* x0,
                                    const float* x1, int32_t B, int32_t H, int32_t W, void* ws, size_t ws_bytes, float* pooled,
                                    float* last_hidden, gsr_stream_t stream_) {
    int rc;
    if ((rc = dn_check_cfg(cfg)) != GSR_OK || (rc = dn_check_image(B, H, W)) != GSR_OK) return rc;
    if (!weights_host || n_weights != gsr_dino_num_weights(cfg->layers)) {
        gsr_set_error("dino: the weight table is null or has %d entries (%d layers need %d)", n_weights, cfg->layers,
                      gsr_dino_num_weights(cfg->layers));
        return GSR_E_INVALID;
    }
    if (!x0 || !pooled) { gsr_set_error("dino: x0 / pooled is null"); return GSR_E_INVALID; }
    auto wp = [&](int i) { return static_cast<const dn_half*>(weights_host[i]); };
    // biases of q, k, v, o, up and down may be absent (NULL); everything else is required
    for (int i = 0; i < n_weights; ++i) {
        bool optional = i == GSR_DINO_W_PATCH_B || (i == GSR_DINO_W_REG && cfg->registers == 0);
        if (i >= GSR_DINO_W_LAYER0 && i < n_weights - 2) {
            const int f = (i - GSR_DINO_W_LAYER0) % GSR_DINO_W_PER_LAYER;
            optional = f == GSR_DINO_L_Q_B || f == GSR_DINO_L_K_B || f == GSR_DINO_L_V_B || f == GSR_DINO_L_O_B || f == GSR_DINO_L_UP_B ||
                       f == GSR_DINO_L_DOWN_B;
        }
        if (!optional && !weights_host[i]) { gsr_set_error("dino: weight %d of the table is null", i); return GSR_E_INVALID; }
    }
    DnLayout lay(cfg, B, H, W, ws);
    if (!ws || ws_bytes < lay.total) {
        gsr_set_error("ws_bytes: dino workspace too small (%zu < %zu bytes)", ws_bytes, lay.total);
        return GSR_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int hid = cfg->hidden, inter = cfg->intermediate, T = lay.T;
    const int64_t M = lay.M;
    if ((rc = dn_embed(cfg, x0, x1, B, H, W, wp(GSR_DINO_W_CLS), wp(GSR_DINO_W_REG), wp(GSR_DINO_W_PATCH_W), wp(GSR_DINO_W_PATCH_B),
                       lay.patches, lay.resid, s)) != GSR_OK)
        return rc;
    for (int l = 0; l < cfg->layers; ++l) {
        const int w0 = GSR_DINO_W_LAYER0 + GSR_DINO_W_PER_LAYER * l;
        if ((rc = dn_norm(lay.resid, M, hid, hid, wp(w0 + GSR_DINO_L_NORM1_W), wp(w0 + GSR_DINO_L_NORM1_B), cfg->ln_eps, lay.xn, 0, s)) != GSR_OK) return rc;
        if ((rc = dn_linear(lay.xn, wp(w0 + GSR_DINO_L_Q_W), wp(w0 + GSR_DINO_L_Q_B), nullptr, lay.q, M, hid, hid, DN_EPI_BIAS, 1, 0, 0, s)) != GSR_OK) return rc;
        if ((rc = dn_linear(lay.xn, wp(w0 + GSR_DINO_L_K_W), wp(w0 + GSR_DINO_L_K_B), nullptr, lay.k, M, hid, hid, DN_EPI_BIAS, 1, 0, 0, s)) != GSR_OK) return rc;
        if ((rc = dn_linear(lay.xn, wp(w0 + GSR_DINO_L_V_W), wp(w0 + GSR_DINO_L_V_B), nullptr, lay.v, M, hid, hid, DN_EPI_BIAS, 1, 0, 0, s)) != GSR_OK) return rc;
        if ((rc = dn_rope(lay.q, lay.k, B, T, cfg->heads, lay.Hp, lay.Wp, cfg->rope_theta, s)) != GSR_OK) return rc;
        if ((rc = dn_attn(lay.q, lay.k, lay.v, lay.att, B, T, cfg->heads, s)) != GSR_OK) return rc;
        if ((rc = dn_linear(lay.att, wp(w0 + GSR_DINO_L_O_W), wp(w0 + GSR_DINO_L_O_B), wp(w0 + GSR_DINO_L_LS1), lay.resid, M, hid, hid, DN_EPI_RESID, 1, 0, 0, s)) != GSR_OK) return rc;
        if ((rc = dn_norm(lay.resid, M, hid, hid, wp(w0 + GSR_DINO_L_NORM2_W), wp(w0 + GSR_DINO_L_NORM2_B), cfg->ln_eps, lay.xn, 0, s)) != GSR_OK) return rc;
        if ((rc = dn_linear(lay.xn, wp(w0 + GSR_DINO_L_UP_W), wp(w0 + GSR_DINO_L_UP_B), nullptr, lay.mlp, M, hid, inter, DN_EPI_GELU, 1, 0, 0, s)) != GSR_OK) return rc;
        if ((rc = dn_linear(lay.mlp, wp(w0 + GSR_DINO_L_DOWN_W), wp(w0 + GSR_DINO_L_DOWN_B), wp(w0 + GSR_DINO_L_LS2), lay.resid, M, inter, hid, DN_EPI_RESID, 1, 0, 0, s)) != GSR_OK) return rc;
    }
    // DN_POOL: the final LayerNorm in f32; row 0 of each image is the pooled output (the same kernel on the same row: same bits)
    if ((rc = dn_norm(lay.resid, B, hid, (int64_t)T * hid, wp(n_weights - 2), wp(n_weights - 1), cfg->ln_eps, pooled, 1, s)) != GSR_OK) return rc;
    if (last_hidden && (rc = dn_norm(lay.resid, M, hid, hid, wp(n_weights - 2), wp(n_weights - 1), cfg->ln_eps, last_hidden, 1, s)) != GSR_OK) return rc;
    return GSR_OK;
}
