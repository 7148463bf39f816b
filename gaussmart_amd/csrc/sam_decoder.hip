// SAM's prompt encoder and mask decoder (transformers' SamPromptEncoder / SamMaskDecoder with the stock configuration: hidden
// 256, two two-way layers, 8 heads, 4 mask tokens, one foreground point per prompt, multimask output) as kernels.  The rules
// are in include/gsr.h (SD_PROMPT, SD_IMAGE, SD_TOKENS, SD_T2I, SD_I2T, SD_UP, SD_HEADS); each has one named place below.
// Every matrix product with a weight is DN_LINEAR (vit.hip, through vit_common.h): fp16 operands, one k-ascending fp32
// chain per output element, rows independent of each other.  The attention cores, the LayerNorms of the image stream and the
// mask product are the kernels of this file.  No split-K, no float atomics: a point's bits depend on its own data only.
// SAM2's decoder (Sam2PromptEncoder / Sam2MaskDecoder; the S2D_* deltas in include/gsr.h) runs the same body: the kernels that
// walk a point's tokens take their number as a template parameter (7: SAM, 8: SAM2 with the object-score token in front), the
// eps of the four block norms is an argument, and the up-scaling takes the two high-resolution skips when they are given.
#include "vit_common.h"

#define SD_C 256           // hidden
#define SD_CI 128           // internal width of the cross attentions: 8 heads of 16
#define SD_HEADS_N 8
#define SD_TOK 7            // SAM: iou, 4 mask tokens, the point, not-a-point
#define SD_TOK2 8           // SAM2: obj_score, iou, 4 mask tokens, the point, not-a-point
#define SD_MLP 2048
#define SD_MAX_GRID 64
#define SD_MAX_POINTS 65535
#define SD_EPS 1e-6f        // SamMaskDecoderConfig.layer_norm_eps and SamLayerNorm's default
#define SD_EPS_FINAL 1e-5f  // layer_norm_final_attn is a plain nn.LayerNorm; so are SAM2's layer_norm1..4
// Where SAM2's feat_s0 is added.  1 (the product): in conv2's epilogue (DN_EPI_SKIP_GELU).  0 (a developer build, `make
// BUILD=build_ab OUT=../lib_ab/libgsr_hip.so EXTRA_DEFS=-DSD_SKIP0_EPILOGUE=0`): conv2 stored as fp32, then one elementwise
// kernel.  The same bits; profiles/sam2_bench.txt has both times (the up-scaling of 256 points at g = 64: 3.31 against 3.50 ms).
#ifndef SD_SKIP0_EPILOGUE
#define SD_SKIP0_EPILOGUE 1
#endif

// ---------------------------------------------------------------- SD_PROMPT
// out[p][0][c] = sinf(arg_c) + fp32(point1[c]), out[p][0][128 + c] = cosf(arg_c) + fp32(point1[128 + c]), out[p][1][:] = fp32(nap);
// arg_c = (ax G[0][c] + ay G[1][c]) * fp32(2 pi), a = 2 ((coordinate + 0.5) / S) - 1: every operation one fp32 rounding.
__global__ void __launch_bounds__(128) sd_prompt_kernel(const float* __restrict__ points, float S, const float* __restrict__ G,
                                                        const dn_half* __restrict__ point1, const dn_half* __restrict__ nap,
                                                        float* __restrict__ out) {
    const int64_t p = blockIdx.x;
    const int c = threadIdx.x;
    const float ax = 2.0f * ((points[2 * p] + 0.5f) / S) - 1.0f, ay = 2.0f * ((points[2 * p + 1] + 0.5f) / S) - 1.0f;
    const float arg = (ax * G[c] + ay * G[128 + c]) * 6.28318530717958647692f;
    float* o = out + p * 2 * SD_C;
    o[c] = sinf(arg) + (float)point1[c];
    o[128 + c] = cosf(arg) + (float)point1[128 + c];
    o[SD_C + c] = (float)nap[c];
    o[SD_C + 128 + c] = (float)nap[128 + c];
}

static int sd_prompt(const float* points, int P, int S, const float* G, const dn_half* point1, const dn_half* nap, float* out,
                     hipStream_t s) {
    hipLaunchKernelGGL(sd_prompt_kernel, dim3((unsigned)P), dim3(128), 0, s, points, (float)S, G, point1, nap, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

static int sd_check_points(int P) {
    if (P < 1 || P > SD_MAX_POINTS) { gsr_set_error("sam decoder: P %d is outside 1 .. %d", P, SD_MAX_POINTS); return GSR_E_INVALID; }
    return GSR_OK;
}
static int sd_check_grid(int g) {
    if (g < 1 || g > SD_MAX_GRID) { gsr_set_error("sam decoder: grid %d is outside 1 .. %d", g, SD_MAX_GRID); return GSR_E_INVALID; }
    return GSR_OK;
}

extern "C" int32_t gsr_sam_dec_prompt(const float* points, int32_t P, int32_t image_size, const float* gauss, const void* point1,
                                      const void* not_a_point, float* out, gsr_stream_t stream_) {
    GSR_TRY(sd_check_points(P));
    if (image_size < 16 || image_size > 16 * SD_MAX_GRID) {
        gsr_set_error("sam decoder: image_size %d is outside 16 .. %d", image_size, 16 * SD_MAX_GRID);
        return GSR_E_INVALID;
    }
    if (!points || !gauss || !point1 || !not_a_point || !out) {
        gsr_set_error("sam dec prompt: points / gauss / point1 / not_a_point / out is null");
        return GSR_E_INVALID;
    }
    return sd_prompt(points, P, image_size, gauss, static_cast<const dn_half*>(point1), static_cast<const dn_half*>(not_a_point), out,
                     static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- SD_IMAGE (layout)
// E16[t][c] = fp16(emb[c][t] + fp32(no_mask[c])), PE16[t][c] = fp16(pe[c][t])
__global__ void __launch_bounds__(256) sd_image_kernel(const float* __restrict__ emb, const float* __restrict__ pe,
                                                       const dn_half* __restrict__ no_mask, int T, dn_half* __restrict__ E16,
                                                       dn_half* __restrict__ PE16) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * SD_C) return;
    const int t = i / SD_C, c = i - t * SD_C;
    E16[i] = (dn_half)(emb[(int64_t)c * T + t] + (float)no_mask[c]);
    PE16[i] = (dn_half)pe[(int64_t)c * T + t];
}

// ---------------------------------------------------------------- SD_TOKENS (elementwise parts)
// tok[p][j], with o = TOK - 7 (SAM2: row 0 is obj_score_token): j = o iou_token, o + 1 .. o + 4 mask_tokens, o + 5 and o + 6 the
// two sparse tokens of the point; written twice (queries and their positional term are the same tensor at the start)
template <int TOK>
__global__ void __launch_bounds__(256) sd_tokens_kernel(const dn_half* __restrict__ obj_tok, const dn_half* __restrict__ iou_tok,
                                                        const dn_half* __restrict__ mask_tok, const float* __restrict__ sparse,
                                                        float* __restrict__ tok0, float* __restrict__ q) {
    constexpr int o = TOK - SD_TOK;
    const int64_t p = blockIdx.x;
    const int c = threadIdx.x;
    for (int j = 0; j < TOK; ++j) {
        float v;
        if (j < o) v = (float)obj_tok[c];
        else if (j == o) v = (float)iou_tok[c];
        else if (j < o + 5) v = (float)mask_tok[(j - o - 1) * SD_C + c];
        else v = sparse[(p * 2 + (j - o - 5)) * SD_C + c];
        tok0[(p * TOK + j) * SD_C + c] = v;
        q[(p * TOK + j) * SD_C + c] = v;
    }
}

// y = fp16(a + b) (b NULL: fp16(a))
__global__ void __launch_bounds__(256) sd_addcast_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                         dn_half* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (dn_half)(b ? a[i] + b[i] : a[i]);
}

__global__ void __launch_bounds__(256) sd_relu_kernel(dn_half* __restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && x[i] < (dn_half)0.f) x[i] = (dn_half)0.f;
}

// token self-attention: TOK queries, TOK keys, 8 heads of 32; q, k, v f32 [P,TOK,256]; thread = (head, query), 8 TOK <= 64 of
// them (TOK = 8 fills the workgroup); out fp16
template <int TOK>
__global__ void __launch_bounds__(64) sd_self_attn_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, dn_half* __restrict__ out) {
    const int64_t p = blockIdx.x;
    const int t = threadIdx.x;
    if (t >= SD_HEADS_N * TOK) return;
    const int h = t / TOK, i = t - h * TOK;
    const float* qr = q + (p * TOK + i) * SD_C + h * 32;
    float s[TOK], m = -INFINITY;
#pragma unroll
    for (int j = 0; j < TOK; ++j) {
        const float* kr = k + (p * TOK + j) * SD_C + h * 32;
        float acc = 0.f;
        for (int d = 0; d < 32; ++d) acc = fmaf(qr[d], kr[d], acc);
        s[j] = acc * 0.17677669529663688110f;       // 32^-1/2
        m = fmaxf(m, s[j]);
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < TOK; ++j) {
        s[j] = expf(s[j] - m);
        l += s[j];
    }
    dn_half* o = out + (p * TOK + i) * SD_C + h * 32;
    for (int d = 0; d < 32; ++d) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < TOK; ++j) acc = fmaf(s[j], v[(p * TOK + j) * SD_C + h * 32 + d], acc);
        o[d] = (dn_half)(acc / l);
    }
}

// ---------------------------------------------------------------- SD_T2I
// One workgroup per (point, head): TOK queries of 16 over T keys.  Thread t takes keys t, t + 256, ... in order; the key is
// fp32(kx) + kpe (kpe NULL: fp32(kx)), the score (sum_d q_d k_d, d ascending, fmaf) * scale.  Pass 1: the maximum per query
// (xor butterfly over the wave, then the four waves).  Pass 2 computes the same scores again, p = expf(s - m), and adds p and
// p v per thread in key order; the 64 lanes are added by a xor butterfly, the four waves in order.  out = fp16(acc / l).
template <int TOK>
__global__ void __launch_bounds__(256) sd_t2i_kernel(const float* __restrict__ q, const dn_half* __restrict__ kx,
                                                     const float* __restrict__ kpe, const dn_half* __restrict__ v, int T,
                                                     int64_t kv_stride, float scale, dn_half* __restrict__ out) {
    __shared__ float qs[TOK][16];
    __shared__ float red[4][TOK * 17];
    const int64_t p = blockIdx.x;
    const int h = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < TOK * 16) qs[t >> 4][t & 15] = q[(p * TOK + (t >> 4)) * SD_CI + h * 16 + (t & 15)];
    __syncthreads();
    const dn_half* kp = kx + p * kv_stride + h * 16;
    const dn_half* vp = v + p * kv_stride + h * 16;
    const float* pp = kpe ? kpe + h * 16 : nullptr;
    auto scores = [&](int key, float* s) {
        float kk[16];
        const vit_h8 a = *reinterpret_cast<const vit_h8*>(kp + (int64_t)key * SD_CI), b = *reinterpret_cast<const vit_h8*>(kp + (int64_t)key * SD_CI + 8);
#pragma unroll
        for (int d = 0; d < 8; ++d) { kk[d] = (float)a[d]; kk[8 + d] = (float)b[d]; }
        if (pp) {
#pragma unroll
            for (int d = 0; d < 16; ++d) kk[d] = kk[d] + pp[(int64_t)key * SD_CI + d];
        }
#pragma unroll
        for (int j = 0; j < TOK; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < 16; ++d) acc = fmaf(qs[j][d], kk[d], acc);
            s[j] = acc * scale;
        }
    };
    float m[TOK];
#pragma unroll
    for (int j = 0; j < TOK; ++j) m[j] = -INFINITY;
    for (int key = t; key < T; key += 256) {
        float s[TOK];
        scores(key, s);
#pragma unroll
        for (int j = 0; j < TOK; ++j) m[j] = fmaxf(m[j], s[j]);
    }
#pragma unroll
    for (int j = 0; j < TOK; ++j) m[j] = wave_max_f32(m[j]);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < TOK; ++j) red[wave][j] = m[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TOK; ++j) m[j] = fmaxf(fmaxf(red[0][j], red[1][j]), fmaxf(red[2][j], red[3][j]));
    __syncthreads();        // red is written again below

    float l[TOK], acc[TOK][16];
#pragma unroll
    for (int j = 0; j < TOK; ++j) {
        l[j] = 0.f;
#pragma unroll
        for (int d = 0; d < 16; ++d) acc[j][d] = 0.f;
    }
    for (int key = t; key < T; key += 256) {
        float s[TOK], vv[16];
        scores(key, s);
        const vit_h8 a = *reinterpret_cast<const vit_h8*>(vp + (int64_t)key * SD_CI), b = *reinterpret_cast<const vit_h8*>(vp + (int64_t)key * SD_CI + 8);
#pragma unroll
        for (int d = 0; d < 8; ++d) { vv[d] = (float)a[d]; vv[8 + d] = (float)b[d]; }
#pragma unroll
        for (int j = 0; j < TOK; ++j) {
            const float pr = expf(s[j] - m[j]);
            l[j] += pr;
#pragma unroll
            for (int d = 0; d < 16; ++d) acc[j][d] = fmaf(pr, vv[d], acc[j][d]);
        }
    }
#pragma unroll
    for (int j = 0; j < TOK; ++j) {
        l[j] = wave_sum_f32(l[j]);
#pragma unroll
        for (int d = 0; d < 16; ++d) acc[j][d] = wave_sum_f32(acc[j][d]);
    }
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < TOK; ++j) {
            red[wave][j * 17 + 16] = l[j];
#pragma unroll
            for (int d = 0; d < 16; ++d) red[wave][j * 17 + d] = acc[j][d];
        }
    __syncthreads();
    if (t < TOK * 16) {
        const int j = t >> 4, d = t & 15;
        const float lt = ((red[0][j * 17 + 16] + red[1][j * 17 + 16]) + red[2][j * 17 + 16]) + red[3][j * 17 + 16];
        const float at = ((red[0][j * 17 + d] + red[1][j * 17 + d]) + red[2][j * 17 + d]) + red[3][j * 17 + d];
        out[(p * TOK + j) * SD_CI + h * 16 + d] = (dn_half)(at / lt);
    }
}

template <int TOK>
static int sd_t2i(const float* q, const dn_half* kx, const float* kpe, const dn_half* v, int P, int T, int shared, float scale,
                  dn_half* out, hipStream_t s) {
    hipLaunchKernelGGL(sd_t2i_kernel<TOK>, dim3((unsigned)P, SD_HEADS_N), dim3(256), 0, s, q, kx, kpe, v, T,
                       shared ? (int64_t)0 : (int64_t)T * SD_CI, scale, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

template <int TOK>
static int sd_t2i_entry(const float* q, const void* kx, const float* kpe, const void* v, int P, int T, int shared, void* out,
                        gsr_stream_t stream_) {
    GSR_TRY(sd_check_points(P));
    if (T < 1 || T > SD_MAX_GRID * SD_MAX_GRID) { gsr_set_error("sam dec t2i: T %d is outside 1 .. %d", T, SD_MAX_GRID * SD_MAX_GRID); return GSR_E_INVALID; }
    if (!q || !kx || !v || !out) { gsr_set_error("sam dec t2i: q / kx / v / out is null"); return GSR_E_INVALID; }
    return sd_t2i<TOK>(q, static_cast<const dn_half*>(kx), kpe, static_cast<const dn_half*>(v), P, T, shared != 0, 0.25f,
                       static_cast<dn_half*>(out), static_cast<hipStream_t>(stream_));
}

extern "C" int32_t gsr_sam_dec_t2i(const float* q, const void* kx, const float* kpe, const void* v, int32_t P, int32_t T,
                                   int32_t shared, void* out, gsr_stream_t stream_) {
    return sd_t2i_entry<SD_TOK>(q, kx, kpe, v, P, T, shared, out, stream_);
}

extern "C" int32_t gsr_sam2_dec_t2i(const float* q, const void* kx, const float* kpe, const void* v, int32_t P, int32_t T,
                                    int32_t shared, void* out, gsr_stream_t stream_) {
    return sd_t2i_entry<SD_TOK2>(q, kx, kpe, v, P, T, shared, out, stream_);
}

// ---------------------------------------------------------------- SD_I2T
// thread = (image token, head); the TOK keys and values of the point are in LDS.  q = fp32(qx) + qpe; s_j = (sum_d q_d k_jd) *
// 1/4, d ascending, fmaf; p_j = expf(s_j - max); ctx_d = (sum_j p_j v_jd) / (sum_j p_j), j ascending; stored as fp16.
template <int TOK>
__global__ void __launch_bounds__(256) sd_i2t_kernel(const dn_half* __restrict__ qx, const float* __restrict__ qpe,
                                                     const float* __restrict__ k, const float* __restrict__ v, int T,
                                                     int64_t q_stride, dn_half* __restrict__ ctx) {
    __shared__ float ks[TOK * SD_CI], vs[TOK * SD_CI];
    const int64_t p = blockIdx.y;
    const int t = threadIdx.x;
    for (int i = t; i < TOK * SD_CI; i += 256) {
        ks[i] = k[p * TOK * SD_CI + i];
        vs[i] = v[p * TOK * SD_CI + i];
    }
    __syncthreads();
    const int tok = (int)blockIdx.x * 32 + (t >> 3), h = t & 7;
    if (tok >= T) return;
    const dn_half* qr = qx + p * q_stride + (int64_t)tok * SD_CI + h * 16;
    const float* pr = qpe + (int64_t)tok * SD_CI + h * 16;
    const vit_h8 a = *reinterpret_cast<const vit_h8*>(qr), b = *reinterpret_cast<const vit_h8*>(qr + 8);
    float qq[16];
#pragma unroll
    for (int d = 0; d < 8; ++d) { qq[d] = (float)a[d] + pr[d]; qq[8 + d] = (float)b[d] + pr[8 + d]; }
    float s[TOK], m = -INFINITY;
#pragma unroll
    for (int j = 0; j < TOK; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < 16; ++d) acc = fmaf(qq[d], ks[j * SD_CI + h * 16 + d], acc);
        s[j] = acc * 0.25f;
        m = fmaxf(m, s[j]);
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < TOK; ++j) {
        s[j] = expf(s[j] - m);
        l += s[j];
    }
    vit_h8 o[2];
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < TOK; ++j) acc = fmaf(s[j], vs[j * SD_CI + h * 16 + d], acc);
        o[d >> 3][d & 7] = (dn_half)(acc / l);
    }
    dn_half* dst = ctx + (p * T + tok) * SD_CI + h * 16;
    *reinterpret_cast<vit_h8*>(dst) = o[0];
    *reinterpret_cast<vit_h8*>(dst + 8) = o[1];
}

// x_out[row] = fp16(LayerNorm(fp32(x[row]) + a[row])): one wave per row of 256, a lane owns channels 4 lane .. 4 lane + 3;
// DN_NORM's formula (mean = sum / 256, biased variance of the differences), the lanes added by a xor butterfly.  x may be
// x_out (a row is read completely before it is written).
__global__ void __launch_bounds__(256) sd_addnorm_kernel(const dn_half* x, const float* __restrict__ a, int64_t rows, int T,
                                                         int64_t x_stride, const dn_half* __restrict__ g,
                                                         const dn_half* __restrict__ beta, float eps, dn_half* x_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t p = row / T, tok = row - p * T;
    const vit_h4 xv = *reinterpret_cast<const vit_h4*>(x + p * x_stride + tok * SD_C + 4 * lane);
    const float4 av = *reinterpret_cast<const float4*>(a + row * SD_C + 4 * lane);
    float y[4] = {(float)xv[0] + av.x, (float)xv[1] + av.y, (float)xv[2] + av.z, (float)xv[3] + av.w};
    const float mean = wave_sum_f32(((y[0] + y[1]) + y[2]) + y[3]) / (float)SD_C;
    float var = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        y[e] = y[e] - mean;
        var += y[e] * y[e];
    }
    const float rstd = 1.0f / sqrtf(wave_sum_f32(var) / (float)SD_C + eps);
    vit_h4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (dn_half)(y[e] * rstd * (float)g[4 * lane + e] + (float)beta[4 * lane + e]);
    *reinterpret_cast<vit_h4*>(x_out + row * SD_C + 4 * lane) = o;
}

// ctx fp16 [P T,128] and att f32 [P T,256] are the caller's; eps is layer_norm4's
template <int TOK>
static int sd_i2t(const dn_half* qx, const float* qpe, const float* k, const float* v, const dn_half* x, int P, int T, int shared,
                  const dn_half* ow, const dn_half* ob, const dn_half* lw, const dn_half* lb, float eps, dn_half* ctx, float* att,
                  dn_half* x_out, hipStream_t s) {
    const int64_t rows = (int64_t)P * T;
    hipLaunchKernelGGL(sd_i2t_kernel<TOK>, dim3((unsigned)((T + 31) / 32), (unsigned)P), dim3(256), 0, s, qx, qpe, k, v, T,
                       shared ? (int64_t)0 : (int64_t)T * SD_CI, ctx);
    GSR_LAUNCH_CHECK();
    GSR_TRY(dn_linear(ctx, ow, ob, nullptr, att, rows, SD_CI, SD_C, DN_EPI_F32, s));
    hipLaunchKernelGGL(sd_addnorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, att, rows, T,
                       shared ? (int64_t)0 : (int64_t)T * SD_C, lw, lb, eps, x_out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

struct SdI2tLayout {
    size_t total;
    dn_half* ctx;
    float* att;
    SdI2tLayout(int P, int T, void* ws) {
        GsrWsCursor cur(ws);
        ctx = cur.take<dn_half>((size_t)P * T * SD_CI * 2);
        att = cur.take<float>((size_t)P * T * SD_C * 4);
        total = cur.off;
    }
};

extern "C" size_t gsr_sam_dec_i2t_workspace_bytes(int32_t P, int32_t T) {
    if (P < 1 || P > SD_MAX_POINTS || T < 1 || T > SD_MAX_GRID * SD_MAX_GRID) return 0;
    return SdI2tLayout(P, T, nullptr).total;
}

template <int TOK>
static int sd_i2t_entry(const void* qx, const float* qpe, const float* k, const float* v, const void* x, int P, int T, int shared,
                        const void* out_w, const void* out_b, const void* ln_w, const void* ln_b, float eps, void* ws, size_t ws_bytes,
                        void* x_out, gsr_stream_t stream_) {
    GSR_TRY(sd_check_points(P));
    if (T < 1 || T > SD_MAX_GRID * SD_MAX_GRID) { gsr_set_error("sam dec i2t: T %d is outside 1 .. %d", T, SD_MAX_GRID * SD_MAX_GRID); return GSR_E_INVALID; }
    if (!qx || !qpe || !k || !v || !x || !out_w || !out_b || !ln_w || !ln_b || !x_out) {
        gsr_set_error("sam dec i2t: an input, a weight or x_out is null");
        return GSR_E_INVALID;
    }
    SdI2tLayout lay(P, T, ws);
    if (!vit_check_ws("sam dec i2t", ws, ws_bytes, lay.total)) return GSR_E_INVALID;
    auto hp = [](const void* p) { return static_cast<const dn_half*>(p); };
    return sd_i2t<TOK>(hp(qx), qpe, k, v, hp(x), P, T, shared != 0, hp(out_w), hp(out_b), hp(ln_w), hp(ln_b), eps, lay.ctx, lay.att,
                       static_cast<dn_half*>(x_out), static_cast<hipStream_t>(stream_));
}

extern "C" int32_t gsr_sam_dec_i2t(const void* qx, const float* qpe, const float* k, const float* v, const void* x, int32_t P, int32_t T,
                                   int32_t shared, const void* out_w, const void* out_b, const void* ln_w, const void* ln_b, void* ws,
                                   size_t ws_bytes, void* x_out, gsr_stream_t stream_) {
    return sd_i2t_entry<SD_TOK>(qx, qpe, k, v, x, P, T, shared, out_w, out_b, ln_w, ln_b, SD_EPS, ws, ws_bytes, x_out, stream_);
}

// the workspace does not depend on the number of tokens
extern "C" size_t gsr_sam2_dec_i2t_workspace_bytes(int32_t P, int32_t T) { return gsr_sam_dec_i2t_workspace_bytes(P, T); }

extern "C" int32_t gsr_sam2_dec_i2t(const void* qx, const float* qpe, const float* k, const float* v, const void* x, int32_t P, int32_t T,
                                    int32_t shared, const void* out_w, const void* out_b, const void* ln_w, const void* ln_b, float eps,
                                    void* ws, size_t ws_bytes, void* x_out, gsr_stream_t stream_) {
    if (!(eps > 0.f)) { gsr_set_error("sam2 dec i2t: eps %g is not positive", (double)eps); return GSR_E_INVALID; }
    return sd_i2t_entry<SD_TOK2>(qx, qpe, k, v, x, P, T, shared, out_w, out_b, ln_w, ln_b, eps, ws, ws_bytes, x_out, stream_);
}

// ---------------------------------------------------------------- SD_UP
// SAM2's two high-resolution skips in the layouts of the two convolutions' outputs, once per call and shared by every point:
// s1t[(t 4 + tap) 64 + c] = feat_s1[c][2 y + dy][2 x + dx] and s0t[((t 4 + tap1) 4 + tap2) 32 + c] = feat_s0[c][4 y + 2 dy1 + dy2]
// [4 x + 2 dx1 + dx2], t = y g + x, tap = dy 2 + dx.  Thread i writes s0t[i] and, for i < 256 T, s1t[i].
__global__ void __launch_bounds__(256) sd_skips_kernel(const float* __restrict__ s0, const float* __restrict__ s1, int g,
                                                       float* __restrict__ s0t, float* __restrict__ s1t) {
    const int T = g * g;
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * 512) return;
    {
        const int c = i & 31, tap2 = (i >> 5) & 3, tap1 = (i >> 7) & 3, t = i >> 9;
        const int y = t / g, x = t - y * g;
        const int Y = 4 * y + 2 * (tap1 >> 1) + (tap2 >> 1), X = 4 * x + 2 * (tap1 & 1) + (tap2 & 1);
        s0t[i] = s0[((int64_t)c * 4 * g + Y) * 4 * g + X];
    }
    if (i < T * 256) {
        const int c = i & 63, tap = (i >> 6) & 3, t = i >> 8;
        const int y = t / g, x = t - y * g;
        const int Y = 2 * y + (tap >> 1), X = 2 * x + (tap & 1);
        s1t[i] = s1[((int64_t)c * 2 * g + Y) * 2 * g + X];
    }
}

// rows of 64 channels (one output pixel of the first transposed convolution each): fp16(gelu(LayerNorm(row))); one wave per
// row, a lane per channel.  skip (SAM2, else NULL): row r takes skip[r mod skip_rows] first, one fp32 addition before the
// statistics.
__global__ void __launch_bounds__(256) sd_up_norm_kernel(const float* __restrict__ u, int64_t rows, const float* __restrict__ skip,
                                                         int skip_rows, const dn_half* __restrict__ g,
                                                         const dn_half* __restrict__ beta, dn_half* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float x = u[row * 64 + lane];
    if (skip) x = x + skip[(row % skip_rows) * 64 + lane];
    const float mean = wave_sum_f32(x) / 64.0f;
    const float d = x - mean;
    const float rstd = 1.0f / sqrtf(wave_sum_f32(d * d) / 64.0f + SD_EPS);
    y[row * 64 + lane] = (dn_half)vit_gelu(d * rstd * (float)g[lane] + (float)beta[lane]);
}

#if !SD_SKIP0_EPILOGUE
// y[r][n] = fp16(gelu(c[r][n] + skip[r mod skip_rows][n])) over rows of 128
__global__ void __launch_bounds__(256) sd_skip_gelu_kernel(const float* __restrict__ c, const float* __restrict__ skip, int64_t n,
                                                           int64_t skip_n, dn_half* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (dn_half)vit_gelu(c[i] + skip[i % skip_n]);
}
#endif

// low_res[p][m][Y][X] = sum_c hyper[m][p][c] fp32(c2[((p T + t) 4 + tap1) 128 + tap2 32 + c]), c ascending, fmaf; t = (Y >> 2) g +
// (X >> 2), tap1 = ((Y >> 1) & 1) 2 + ((X >> 1) & 1), tap2 = (Y & 1) 2 + (X & 1).  A thread per output pixel, X fastest.
__global__ void __launch_bounds__(256) sd_mask_kernel(const dn_half* __restrict__ c2, const float* __restrict__ hyper, int g, int P,
                                                      float* __restrict__ low_res) {
    __shared__ float hs[3 * 32];
    const int64_t p = blockIdx.y;
    const int L = 4 * g;
    if (threadIdx.x < 96) hs[threadIdx.x] = hyper[((int64_t)(threadIdx.x >> 5) * P + p) * 32 + (threadIdx.x & 31)];
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= L * L) return;
    const int Y = i / L, X = i - Y * L;
    const int64_t t = (int64_t)(Y >> 2) * g + (X >> 2);
    const int tap1 = ((Y >> 1) & 1) * 2 + ((X >> 1) & 1), tap2 = (Y & 1) * 2 + (X & 1);
    const dn_half* src = c2 + (((p * g * g + t) * 4 + tap1) * 128 + tap2 * 32);
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const vit_h8 a = *reinterpret_cast<const vit_h8*>(src + 8 * q);
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[m] = fmaf(hs[m * 32 + 8 * q + e], (float)a[e], acc[m]);
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) low_res[((p * 3 + m) * L + Y) * L + X] = acc[m];
}

// u32 f32 [P T,256] (later fp16 [P T 4,128] in the same bytes) and u16 fp16 [P T 4,64] are the caller's; s0t and s1t are
// sd_skips_kernel's tables (SAM2) or both NULL (SAM); c32 f32 [P T 4,128] exists in the SD_SKIP0_EPILOGUE=0 build only
static int sd_upscale(const dn_half* x, int g, int P, const dn_half* c1w, const dn_half* c1b, const dn_half* lw, const dn_half* lb,
                      const dn_half* c2w, const dn_half* c2b, const float* hyper, const float* s0t, const float* s1t, float* u32,
                      dn_half* u16, float* c32, float* low_res, hipStream_t s) {
    const int T = g * g;
    const int64_t rows = (int64_t)P * T;
    GSR_TRY(dn_linear(x, c1w, c1b, nullptr, u32, rows, SD_C, SD_C, DN_EPI_F32, s));
    hipLaunchKernelGGL(sd_up_norm_kernel, dim3((unsigned)(rows)), dim3(256), 0, s, u32, rows * 4, s1t, 4 * T, lw, lb, u16);
    GSR_LAUNCH_CHECK();
    dn_half* c2 = reinterpret_cast<dn_half*>(u32);
    if (s0t) {
#if SD_SKIP0_EPILOGUE
        GSR_TRY(dn_linear(u16, c2w, c2b, reinterpret_cast<const dn_half*>(s0t), c2, rows * 4, 64, 128, DN_EPI_SKIP_GELU, s, {4 * T, 0, 0}));
#else
        GSR_TRY(dn_linear(u16, c2w, c2b, nullptr, c32, rows * 4, 64, 128, DN_EPI_F32, s));
        const int64_t n = rows * 4 * 128;
        hipLaunchKernelGGL(sd_skip_gelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c32, s0t, n, (int64_t)T * 512, c2);
        GSR_LAUNCH_CHECK();
#endif
    } else
        GSR_TRY(dn_linear(u16, c2w, c2b, nullptr, c2, rows * 4, 64, 128, DN_EPI_GELU, s));
    const int L = 4 * g;
    hipLaunchKernelGGL(sd_mask_kernel, dim3((unsigned)((L * L + 255) / 256), (unsigned)P), dim3(256), 0, s, c2, hyper, g, P, low_res);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

static int sd_skips(const float* feat_s0, const float* feat_s1, int g, float* s0t, float* s1t, hipStream_t s) {
    hipLaunchKernelGGL(sd_skips_kernel, dim3((unsigned)(g * g * 2)), dim3(256), 0, s, feat_s0, feat_s1, g, s0t, s1t);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

struct SdUpLayout {
    size_t total;
    float *u32, *s0t, *s1t, *c32 = nullptr;
    dn_half* u16;
    SdUpLayout(int g, int P, bool skips, void* ws) {
        GsrWsCursor cur(ws);
        u32 = cur.take<float>((size_t)P * g * g * SD_C * 4);
        u16 = cur.take<dn_half>((size_t)P * g * g * 4 * 64 * 2);
        s0t = skips ? cur.take<float>((size_t)g * g * 512 * 4) : nullptr;
        s1t = skips ? cur.take<float>((size_t)g * g * 256 * 4) : nullptr;
#if !SD_SKIP0_EPILOGUE
        if (skips) c32 = cur.take<float>((size_t)P * g * g * 4 * 128 * 4);
#endif
        total = cur.off;
    }
};

extern "C" size_t gsr_sam_dec_upscale_workspace_bytes(int32_t g, int32_t P) {
    if (g < 1 || g > SD_MAX_GRID || P < 1 || P > SD_MAX_POINTS) return 0;
    return SdUpLayout(g, P, false, nullptr).total;
}

extern "C" size_t gsr_sam2_dec_upscale_workspace_bytes(int32_t g, int32_t P) {
    if (g < 1 || g > SD_MAX_GRID || P < 1 || P > SD_MAX_POINTS) return 0;
    return SdUpLayout(g, P, true, nullptr).total;
}

// feat_s0 and feat_s1 both NULL: SAM
static int sd_upscale_entry(const void* x, int g, int P, const void* conv1_w, const void* conv1_b, const void* ln_w, const void* ln_b,
                            const void* conv2_w, const void* conv2_b, const float* hyper, const float* feat_s0, const float* feat_s1,
                            void* ws, size_t ws_bytes, float* low_res, gsr_stream_t stream_) {
    GSR_TRY(sd_check_grid(g));
    GSR_TRY(sd_check_points(P));
    if (!x || !conv1_w || !conv1_b || !ln_w || !ln_b || !conv2_w || !conv2_b || !hyper || !low_res) {
        gsr_set_error("sam dec upscale: x / a weight / hyper / low_res is null");
        return GSR_E_INVALID;
    }
    const bool skips = feat_s0 != nullptr;
    SdUpLayout lay(g, P, skips, ws);
    if (!vit_check_ws("sam dec upscale", ws, ws_bytes, lay.total)) return GSR_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (skips) GSR_TRY(sd_skips(feat_s0, feat_s1, g, lay.s0t, lay.s1t, s));
    auto hp = [](const void* p) { return static_cast<const dn_half*>(p); };
    return sd_upscale(hp(x), g, P, hp(conv1_w), hp(conv1_b), hp(ln_w), hp(ln_b), hp(conv2_w), hp(conv2_b), hyper, lay.s0t, lay.s1t,
                      lay.u32, lay.u16, lay.c32, low_res, s);
}

extern "C" int32_t gsr_sam_dec_upscale(const void* x, int32_t g, int32_t P, const void* conv1_w, const void* conv1_b, const void* ln_w,
                                       const void* ln_b, const void* conv2_w, const void* conv2_b, const float* hyper, void* ws,
                                       size_t ws_bytes, float* low_res, gsr_stream_t stream_) {
    return sd_upscale_entry(x, g, P, conv1_w, conv1_b, ln_w, ln_b, conv2_w, conv2_b, hyper, nullptr, nullptr, ws, ws_bytes, low_res,
                            stream_);
}

extern "C" int32_t gsr_sam2_dec_upscale(const void* x, int32_t g, int32_t P, const void* conv1_w, const void* conv1_b, const void* ln_w,
                                        const void* ln_b, const void* conv2_w, const void* conv2_b, const float* hyper,
                                        const float* feat_s0, const float* feat_s1, void* ws, size_t ws_bytes, float* low_res,
                                        gsr_stream_t stream_) {
    if (!feat_s0 || !feat_s1) { gsr_set_error("sam2 dec upscale: feat_s0 / feat_s1 is null"); return GSR_E_INVALID; }
    return sd_upscale_entry(x, g, P, conv1_w, conv1_b, ln_w, ln_b, conv2_w, conv2_b, hyper, feat_s0, feat_s1, ws, ws_bytes, low_res,
                            stream_);
}

// ---------------------------------------------------------------- SD_HEADS (gather)
// rows[k][p] = fp16(tokens[p][o + (k == 0 ? 0 : k + 1)]), o = TOK - 7: the iou token and mask tokens 1..3
template <int TOK>
__global__ void __launch_bounds__(256) sd_heads_gather_kernel(const float* __restrict__ q, int P, dn_half* __restrict__ rows) {
    constexpr int o = TOK - SD_TOK;
    const int64_t p = blockIdx.x;
    const int c = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) rows[((int64_t)k * P + p) * SD_C + c] = (dn_half)q[(p * TOK + o + (k == 0 ? 0 : k + 1)) * SD_C + c];
}

// SAM2's IoU head ends in a sigmoid: x = 1 / (1 + expf(-x)), every operation one fp32 rounding
__global__ void __launch_bounds__(256) sd_sigmoid_kernel(float* __restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = 1.0f / (1.0f + expf(-x[i]));
}

// ---------------------------------------------------------------- the whole decoder
struct SdLayout {
    size_t total;
    // per image
    dn_half *E16, *PE16, *kx0, *v0, *qx0;
    float* pe_proj[5];      // t2i layer 0, i2t layer 0, t2i layer 1, i2t layer 1, final: proj(pe) + bias, f32 [T,128]
    // tokens
    float *sparse, *tok0, *qa, *qb, *qf, *kf, *vf, *hyper;
    dn_half *h16, *h16b, *c16, *m16, *heads16, *t16a, *t16b;
    // per point and image token
    dn_half *x16, *b1, *b2;
    float* a32;
    // SAM2's skips, per image
    float *s0t, *s1t, *c32 = nullptr;
    SdLayout(int g, int P, int tok, bool skips, void* ws) {
        const size_t T = (size_t)g * g, R = (size_t)P * tok, PT = (size_t)P * T;
        GsrWsCursor cur(ws);
        E16 = cur.take<dn_half>(T * SD_C * 2);
        PE16 = cur.take<dn_half>(T * SD_C * 2);
        kx0 = cur.take<dn_half>(T * SD_CI * 2);
        v0 = cur.take<dn_half>(T * SD_CI * 2);
        qx0 = cur.take<dn_half>(T * SD_CI * 2);
        for (int i = 0; i < 5; ++i) pe_proj[i] = cur.take<float>(T * SD_CI * 4);
        sparse = cur.take<float>((size_t)P * 2 * SD_C * 4);
        tok0 = cur.take<float>(R * SD_C * 4);
        qa = cur.take<float>(R * SD_C * 4);
        qb = cur.take<float>(R * SD_C * 4);
        qf = cur.take<float>(R * SD_C * 4);
        kf = cur.take<float>(R * SD_C * 4);
        vf = cur.take<float>(R * SD_C * 4);
        hyper = cur.take<float>((size_t)3 * P * 32 * 4);
        h16 = cur.take<dn_half>(R * SD_C * 2);
        h16b = cur.take<dn_half>(R * SD_C * 2);
        c16 = cur.take<dn_half>(R * SD_C * 2);
        m16 = cur.take<dn_half>(R * SD_MLP * 2);
        heads16 = cur.take<dn_half>((size_t)4 * P * SD_C * 2);
        t16a = cur.take<dn_half>((size_t)P * SD_C * 2);
        t16b = cur.take<dn_half>((size_t)P * SD_C * 2);
        x16 = cur.take<dn_half>(PT * SD_C * 2);
        // b1 and b2 are contiguous: together they hold the up-scaling's fp16 [P T 4,64]
        const size_t half_bytes = gsr_align(PT * SD_CI * 2);
        b1 = cur.take<dn_half>(2 * half_bytes);
        b2 = b1 ? reinterpret_cast<dn_half*>(reinterpret_cast<char*>(b1) + half_bytes) : nullptr;
        a32 = cur.take<float>(PT * SD_C * 4);
        s0t = skips ? cur.take<float>(T * 512 * 4) : nullptr;
        s1t = skips ? cur.take<float>(T * 256 * 4) : nullptr;
#if !SD_SKIP0_EPILOGUE
        if (skips) c32 = cur.take<float>(PT * 4 * 128 * 4);
#endif
        total = cur.off;
    }
};

// What SAM2's decoder has and SAM's has not.  SAM: {SD_EPS, NULL, NULL, NULL, false}.
struct SdModel {
    float eps;                      // layer_norm1..4 of the two-way layers
    const dn_half* obj_tok;         // row 0 of the tokens (TOK = 8)
    const float *feat_s0, *feat_s1; // the skips of the up-scaling
    bool sigmoid;                   // the IoU head's last activation
};

// One body for both models.  The arguments are checked by the callers; weights_host has the GSR_SAMD_* slots.
template <int TOK>
static int sd_decode(const SdModel& model, int g, const void* const* weights_host, const float* emb, const float* pe, const float* points,
                     int P, int image_size, void* ws, size_t ws_bytes, float* low_res, float* iou, hipStream_t s) {
    const bool skips = model.feat_s0 != nullptr;
    SdLayout lay(g, P, TOK, skips, ws);
    if (!vit_check_ws("sam decoder", ws, ws_bytes, lay.total)) return GSR_E_INVALID;
    const int T = g * g;
    const int64_t R = (int64_t)P * TOK, PT = (int64_t)P * T;
    auto W = [&](int i) { return static_cast<const dn_half*>(weights_host[i]); };
    auto lin = [&](const dn_half* x, int wi, int bi, void* out, int64_t M, int K, int N, int epi) -> int {
        return dn_linear(x, W(wi), bi < 0 ? nullptr : W(bi), nullptr, out, M, K, N, epi, s);
    };
    auto addcast = [&](const float* a, const float* b, dn_half* y) -> int {
        const int64_t n = R * SD_C;
        hipLaunchKernelGGL(sd_addcast_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, n, y);
        GSR_LAUNCH_CHECK();
        return GSR_OK;
    };
    auto relu = [&](dn_half* x, int64_t n) -> int {
        hipLaunchKernelGGL(sd_relu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n);
        GSR_LAUNCH_CHECK();
        return GSR_OK;
    };
    float *q = lay.qa, *q_alt = lay.qb;
    auto norm = [&](int wi, float eps) -> int {
        const int r = dn_norm(q, R, SD_C, SD_C, W(wi), W(wi + 1), eps, q_alt, 1, s);
        float* tmp = q; q = q_alt; q_alt = tmp;
        return r;
    };

    // SD_PROMPT and the tokens
    GSR_TRY(sd_prompt(points, P, image_size, static_cast<const float*>(weights_host[GSR_SAMD_W_GAUSS]), W(GSR_SAMD_W_POINT1),
                    W(GSR_SAMD_W_NOT_A_POINT), lay.sparse, s));
    hipLaunchKernelGGL(sd_tokens_kernel<TOK>, dim3((unsigned)P), dim3(256), 0, s, model.obj_tok, W(GSR_SAMD_W_IOU_TOKEN),
                       W(GSR_SAMD_W_MASK_TOKENS), lay.sparse, lay.tok0, q);
    GSR_LAUNCH_CHECK();

    // SD_IMAGE
    hipLaunchKernelGGL(sd_image_kernel, dim3((unsigned)((T * SD_C + 255) / 256)), dim3(256), 0, s, emb, pe, W(GSR_SAMD_W_NO_MASK), T, lay.E16,
                       lay.PE16);
    GSR_LAUNCH_CHECK();
    if (skips) GSR_TRY(sd_skips(model.feat_s0, model.feat_s1, g, lay.s0t, lay.s1t, s));
    const int l0 = GSR_SAMD_W_LAYER0, l1 = GSR_SAMD_W_LAYER0 + GSR_SAMD_W_PER_LAYER, fin = GSR_SAMD_W_FINAL;
    GSR_TRY(lin(lay.PE16, l0 + GSR_SAMD_L_T2I + 2, l0 + GSR_SAMD_L_T2I + 3, lay.pe_proj[0], T, SD_C, SD_CI, DN_EPI_F32));
    GSR_TRY(lin(lay.PE16, l0 + GSR_SAMD_L_I2T + 0, l0 + GSR_SAMD_L_I2T + 1, lay.pe_proj[1], T, SD_C, SD_CI, DN_EPI_F32));
    GSR_TRY(lin(lay.PE16, l1 + GSR_SAMD_L_T2I + 2, l1 + GSR_SAMD_L_T2I + 3, lay.pe_proj[2], T, SD_C, SD_CI, DN_EPI_F32));
    GSR_TRY(lin(lay.PE16, l1 + GSR_SAMD_L_I2T + 0, l1 + GSR_SAMD_L_I2T + 1, lay.pe_proj[3], T, SD_C, SD_CI, DN_EPI_F32));
    GSR_TRY(lin(lay.PE16, fin + 2, fin + 3, lay.pe_proj[4], T, SD_C, SD_CI, DN_EPI_F32));
    GSR_TRY(lin(lay.E16, l0 + GSR_SAMD_L_T2I + 2, -1, lay.kx0, T, SD_C, SD_CI, DN_EPI_BIAS));
    GSR_TRY(lin(lay.E16, l0 + GSR_SAMD_L_T2I + 4, l0 + GSR_SAMD_L_T2I + 5, lay.v0, T, SD_C, SD_CI, DN_EPI_BIAS));
    GSR_TRY(lin(lay.E16, l0 + GSR_SAMD_L_I2T + 0, -1, lay.qx0, T, SD_C, SD_CI, DN_EPI_BIAS));

    // token -> image attention with the weights at `a`: queries += out_proj(attention)
    auto t2i = [&](int a, int first, const float* kpe) -> int {
        GSR_TRY(addcast(q, lay.tok0, lay.h16));
        GSR_TRY(lin(lay.h16, a + 0, a + 1, lay.qf, R, SD_C, SD_CI, DN_EPI_F32));
        if (!first) {
            GSR_TRY(lin(lay.x16, a + 2, -1, lay.b1, PT, SD_C, SD_CI, DN_EPI_BIAS));
            GSR_TRY(lin(lay.x16, a + 4, a + 5, lay.b2, PT, SD_C, SD_CI, DN_EPI_BIAS));
        }
        GSR_TRY(sd_t2i<TOK>(lay.qf, first ? lay.kx0 : lay.b1, kpe, first ? lay.v0 : lay.b2, P, T, first, 0.25f, lay.c16, s));
        return lin(lay.c16, a + 6, a + 7, q, R, SD_CI, SD_C, DN_EPI_RESID1);
    };

    for (int l = 0; l < 2; ++l) {
        const int b = GSR_SAMD_W_LAYER0 + GSR_SAMD_W_PER_LAYER * l;
        // SD_TOKENS: self-attention
        const int sa = b + GSR_SAMD_L_SELF;
        if (l == 0) {
            GSR_TRY(addcast(q, nullptr, lay.h16));
            GSR_TRY(lin(lay.h16, sa + 4, sa + 5, lay.vf, R, SD_C, SD_C, DN_EPI_F32));
        } else {
            GSR_TRY(addcast(q, lay.tok0, lay.h16));
            GSR_TRY(addcast(q, nullptr, lay.h16b));
            GSR_TRY(lin(lay.h16b, sa + 4, sa + 5, lay.vf, R, SD_C, SD_C, DN_EPI_F32));
        }
        GSR_TRY(lin(lay.h16, sa + 0, sa + 1, lay.qf, R, SD_C, SD_C, DN_EPI_F32));
        GSR_TRY(lin(lay.h16, sa + 2, sa + 3, lay.kf, R, SD_C, SD_C, DN_EPI_F32));
        hipLaunchKernelGGL(sd_self_attn_kernel<TOK>, dim3((unsigned)P), dim3(64), 0, s, lay.qf, lay.kf, lay.vf, lay.c16);
        GSR_LAUNCH_CHECK();
        GSR_TRY(lin(lay.c16, sa + 6, sa + 7, q, R, SD_C, SD_C, l == 0 ? DN_EPI_F32 : DN_EPI_RESID1));
        GSR_TRY(norm(b + GSR_SAMD_L_NORM1, model.eps));
        // SD_T2I
        GSR_TRY(t2i(b + GSR_SAMD_L_T2I, l == 0, lay.pe_proj[2 * l]));
        GSR_TRY(norm(b + GSR_SAMD_L_NORM2, model.eps));
        // SD_TOKENS: MLP
        GSR_TRY(addcast(q, nullptr, lay.h16));
        GSR_TRY(lin(lay.h16, b + GSR_SAMD_L_MLP + 0, b + GSR_SAMD_L_MLP + 1, lay.m16, R, SD_C, SD_MLP, DN_EPI_BIAS));
        GSR_TRY(relu(lay.m16, R * SD_MLP));
        GSR_TRY(lin(lay.m16, b + GSR_SAMD_L_MLP + 2, b + GSR_SAMD_L_MLP + 3, q, R, SD_MLP, SD_C, DN_EPI_RESID1));
        GSR_TRY(norm(b + GSR_SAMD_L_NORM3, model.eps));
        // SD_I2T
        const int it = b + GSR_SAMD_L_I2T;
        GSR_TRY(addcast(q, lay.tok0, lay.h16));
        GSR_TRY(addcast(q, nullptr, lay.h16b));
        GSR_TRY(lin(lay.h16, it + 2, it + 3, lay.kf, R, SD_C, SD_CI, DN_EPI_F32));
        GSR_TRY(lin(lay.h16b, it + 4, it + 5, lay.vf, R, SD_C, SD_CI, DN_EPI_F32));
        if (l > 0) GSR_TRY(lin(lay.x16, it + 0, -1, lay.b1, PT, SD_C, SD_CI, DN_EPI_BIAS));
        GSR_TRY(sd_i2t<TOK>(l == 0 ? lay.qx0 : lay.b1, lay.pe_proj[2 * l + 1], lay.kf, lay.vf, l == 0 ? lay.E16 : lay.x16, P, T, l == 0,
                          W(it + 6), W(it + 7), W(b + GSR_SAMD_L_NORM4), W(b + GSR_SAMD_L_NORM4 + 1), model.eps, lay.b2, lay.a32, lay.x16,
                          s));
    }
    GSR_TRY(t2i(fin, 0, lay.pe_proj[4]));
    GSR_TRY(norm(fin + 8, SD_EPS_FINAL));

    // SD_HEADS
    hipLaunchKernelGGL(sd_heads_gather_kernel<TOK>, dim3((unsigned)P), dim3(256), 0, s, q, P, lay.heads16);
    GSR_LAUNCH_CHECK();
    for (int k = 0; k < 4; ++k) {
        const int a = k == 0 ? GSR_SAMD_W_IOU : GSR_SAMD_W_HYPER + 6 * (k - 1);
        GSR_TRY(lin(lay.heads16 + (int64_t)k * P * SD_C, a + 0, a + 1, lay.t16a, P, SD_C, SD_C, DN_EPI_BIAS));
        GSR_TRY(relu(lay.t16a, (int64_t)P * SD_C));
        GSR_TRY(lin(lay.t16a, a + 2, a + 3, lay.t16b, P, SD_C, SD_C, DN_EPI_BIAS));
        GSR_TRY(relu(lay.t16b, (int64_t)P * SD_C));
        if (k == 0)     // rows 1..3 of the IoU head's last layer [4,256]: columns 1..3 of its output
            GSR_TRY(dn_linear(lay.t16b, W(a + 4) + SD_C, W(a + 5) + 1, nullptr, iou, P, SD_C, 3, DN_EPI_F32, s));
        else
            GSR_TRY(lin(lay.t16b, a + 4, a + 5, lay.hyper + (int64_t)(k - 1) * P * 32, P, SD_C, 32, DN_EPI_F32));
    }
    if (model.sigmoid) {
        hipLaunchKernelGGL(sd_sigmoid_kernel, dim3((unsigned)((3 * P + 255) / 256)), dim3(256), 0, s, iou, (int64_t)3 * P);
        GSR_LAUNCH_CHECK();
    }
    // SD_UP
    const int up = GSR_SAMD_W_UP;
    return sd_upscale(lay.x16, g, P, W(up), W(up + 1), W(up + 2), W(up + 3), W(up + 4), W(up + 5), lay.hyper, lay.s0t, lay.s1t, lay.a32,
                      lay.b1, lay.c32, low_res, s);
}

// the refusals the two models share; `count` is the length of the model's weight table
static int sd_decode_check(int g, const void* const* weights_host, int n_weights, int count, const float* emb, const float* pe,
                           const float* points, int P, int image_size, const float* low_res, const float* iou) {
    GSR_TRY(sd_check_grid(g));
    GSR_TRY(sd_check_points(P));
    if (image_size != 16 * g) { gsr_set_error("sam decoder: image_size %d is not 16 x grid %d", image_size, g); return GSR_E_INVALID; }
    if (!weights_host || n_weights != count) {
        gsr_set_error("sam decoder: the weight table is null or has %d entries (%d are needed)", n_weights, count);
        return GSR_E_INVALID;
    }
    if (!vit_check_table("sam decoder", weights_host, n_weights)) return GSR_E_INVALID;
    if (!emb || !pe || !points || !low_res || !iou) { gsr_set_error("sam decoder: emb / pe / points / low_res / iou is null"); return GSR_E_INVALID; }
    return GSR_OK;
}

extern "C" int32_t gsr_sam_dec_num_weights(void) { return GSR_SAMD_W_COUNT; }

extern "C" size_t gsr_sam_decode_workspace_bytes(int32_t g, int32_t P) {
    if (g < 1 || g > SD_MAX_GRID || P < 1 || P > SD_MAX_POINTS) return 0;
    return SdLayout(g, P, SD_TOK, false, nullptr).total;
}

extern "C" int32_t gsr_sam_decode(int32_t g, const void* const* weights_host, int32_t n_weights, const float* emb, const float* pe,
                                  const float* points, int32_t P, int32_t image_size, void* ws, size_t ws_bytes, float* low_res,
                                  float* iou, gsr_stream_t stream_) {
    GSR_TRY(sd_decode_check(g, weights_host, n_weights, GSR_SAMD_W_COUNT, emb, pe, points, P, image_size, low_res, iou));
    const SdModel sam = {SD_EPS, nullptr, nullptr, nullptr, false};
    return sd_decode<SD_TOK>(sam, g, weights_host, emb, pe, points, P, image_size, ws, ws_bytes, low_res, iou,
                             static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- SAM2
extern "C" int32_t gsr_sam2_dec_num_weights(void) { return GSR_SAM2D_W_COUNT; }

extern "C" size_t gsr_sam2_decode_workspace_bytes(int32_t g, int32_t P) {
    if (g < 1 || g > SD_MAX_GRID || P < 1 || P > SD_MAX_POINTS) return 0;
    return SdLayout(g, P, SD_TOK2, true, nullptr).total;
}

extern "C" int32_t gsr_sam2_decode(int32_t g, const void* const* weights_host, int32_t n_weights, const float* feat_s0,
                                   const float* feat_s1, const float* emb, const float* pe, const float* points, int32_t P,
                                   int32_t image_size, void* ws, size_t ws_bytes, float* low_res, float* iou, gsr_stream_t stream_) {
    GSR_TRY(sd_decode_check(g, weights_host, n_weights, GSR_SAM2D_W_COUNT, emb, pe, points, P, image_size, low_res, iou));
    if (!feat_s0 || !feat_s1) { gsr_set_error("sam2 decoder: feat_s0 / feat_s1 is null"); return GSR_E_INVALID; }
    const SdModel sam2 = {SD_EPS_FINAL, static_cast<const dn_half*>(weights_host[GSR_SAM2D_W_OBJ_TOKEN]), feat_s0, feat_s1, true};
    return sd_decode<SD_TOK2>(sam2, g, weights_host, emb, pe, points, P, image_size, ws, ws_bytes, low_res, iou,
                              static_cast<hipStream_t>(stream_));
}
