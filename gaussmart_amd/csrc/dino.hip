// DINOv3 ViT encoder (transformers' DINOv3ViTModel, inference only) as kernels: fp16 operands on the 32x32x16 f16 matrix
// instruction with fp32 accumulation; the residual stream, the LayerNorm statistics, the softmax and the input normalisation
// in fp32.  (The reference's .half() model keeps the residual stream in fp16; this one deliberately does not.)  The rules
// are in include/gsr.h (DN_EMBED, DN_NORM, DN_LINEAR, DN_ROPE, DN_ATTN, DN_POOL, DN_COS); each has one named place below,
// except DN_LINEAR and DN_NORM, which are in vit.hip.
// No split-K and no atomics: every output element is one k-ordered chain, so the bits are the same on every run and for an
// image alone or inside a batch.
#include "cloud_common.h"
#include "vit_attn.h"

#define DN_HEAD 64
#define DN_MAX_BATCH 8

// ---------------------------------------------------------------- DN_EMBED (gather)
// patches[b Np + p][c 256 + ky 16 + kx] = fp16((x[b,c,16 py + ky,16 px + kx] - mean[c]) / std[c]): the subtraction and the true
// division in fp32, one rounding to fp16.  A thread writes the 8 kx of half a patch row (vit_patch_part).  Rows and columns
// past 16 Hp, 16 Wp are never read.
__global__ void __launch_bounds__(256) dn_im2col_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int B, int H,
                                                        int W, int Hp, int Wp, float m0, float m1, float m2, float s0, float s1,
                                                        float s2, dn_half* __restrict__ patches) {
    const int64_t Np = (int64_t)Hp * Wp;
    VitPatchPart a;
    if (!vit_patch_part((int64_t)B * Np, a)) return;
    const int b = (int)(a.row / Np);
    const int64_t p = a.row - (int64_t)b * Np;
    const int py = (int)(p / Wp), px = (int)(p - (int64_t)py * Wp);
    const float* img = b == 0 ? x0 : x1 + (int64_t)(b - 1) * 3 * H * W;
    const float* src = img + ((int64_t)a.c * H + (py * VIT_PATCH + a.ky)) * W + px * VIT_PATCH + a.kx0;
    const float mean = a.c == 0 ? m0 : a.c == 1 ? m1 : m2, sd = a.c == 0 ? s0 : a.c == 1 ? s1 : s2;
    vit_h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (dn_half)((src[e] - mean) / sd);
    vit_patch_store(patches, a, v);
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
    if (H < VIT_PATCH || W < VIT_PATCH) { gsr_set_error("dino: a %dx%d image is below one 16x16 patch", H, W); return GSR_E_INVALID; }
    if ((int64_t)(H / VIT_PATCH) * (W / VIT_PATCH) > (1 << 24)) { gsr_set_error("dino: a %dx%d image has too many patches", H, W); return GSR_E_UNSUPPORTED; }
    return GSR_OK;
}

// ---------------------------------------------------------------- DN_EMBED
static int dn_embed(const GsrDinoConfig* c, const float* x0, const float* x1, int B, int H, int W, const dn_half* cls,
                    const dn_half* reg, const dn_half* pw, const dn_half* pb, dn_half* patches, float* out, hipStream_t s) {
    const int Hp = H / VIT_PATCH, Wp = W / VIT_PATCH, prefix = 1 + c->registers;
    const int64_t Np = (int64_t)Hp * Wp;
    const int T = (int)(prefix + Np);
    if (!x1) x1 = x0 + (int64_t)3 * H * W;
    hipLaunchKernelGGL(dn_im2col_kernel, dim3(vit_patch_blocks((int64_t)B * Np)), dim3(256), 0, s, x0, x1, B, H, W, Hp, Wp,
                       c->image_mean[0], c->image_mean[1], c->image_mean[2], c->image_std[0], c->image_std[1], c->image_std[2], patches);
    GSR_LAUNCH_CHECK();
    const int64_t n_prefix = (int64_t)B * prefix * c->hidden;
    hipLaunchKernelGGL(dn_prefix_kernel, dim3((unsigned)((n_prefix + 255) / 256)), dim3(256), 0, s, cls, reg, B, T, prefix, c->hidden, out);
    GSR_LAUNCH_CHECK();
    return dn_linear(patches, pw, pb, nullptr, out, (int64_t)B * Np, VIT_PATCH_K, c->hidden, DN_EPI_EMBED, s, {Np, T, prefix});
}

extern "C" size_t gsr_dino_embed_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B < 1 || H < VIT_PATCH || W < VIT_PATCH) return 0;
    return gsr_align((size_t)B * (size_t)(H / VIT_PATCH) * (size_t)(W / VIT_PATCH) * VIT_PATCH_K * 2);
}

extern "C" int32_t gsr_dino_embed(const GsrDinoConfig* cfg, const float* x0, const float* x1, int32_t B, int32_t H, int32_t W,
                                  const void* cls, const void* reg, const void* patch_w, const void* patch_b, void* ws,
                                  size_t ws_bytes, float* out, gsr_stream_t stream_) {
    GSR_TRY(dn_check_cfg(cfg));
    GSR_TRY(dn_check_image(B, H, W));
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
// The tile of vit_attn.h at HD = 64.  A workgroup of 4 waves owns 128 query rows of one head, a wave 32 of them; K and V go
// through LDS in tiles of 64 rows (V transposed on the way in), the next tile's global loads issued before the tile's matrix
// instructions.  The base-2 score is one fp32 product with log2(e) / 8.
// Rows of K and V past T are never read; their scores are -inf before the maximum.  Query rows past T are not written.
#define DA_LOG2E_8 0.18033688011112042592f      // log2(e) / 8: the scores are kept in base 2, p = 2^(s2 - m2) is one v_exp_f32

__global__ void __launch_bounds__(256) dn_attn_kernel(const dn_half* __restrict__ q, const dn_half* __restrict__ k,
                                                      const dn_half* __restrict__ v, dn_half* __restrict__ o, int T, int hidden) {
    typedef VitAttnTile<DN_HEAD> Tile;
    __shared__ __attribute__((aligned(16))) dn_half Ks[VA_BKV * Tile::LDK];     // [kv][d]
    __shared__ __attribute__((aligned(16))) dn_half Vt[DN_HEAD * VA_LDV];       // [d][kv]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int64_t base = (int64_t)blockIdx.z * T * hidden + (int64_t)blockIdx.y * DN_HEAD;
    const int qrow = (int)blockIdx.x * VA_BQ + wave * 32 + r;
    vit_h8 qf[Tile::KS];
#pragma unroll
    for (int ks = 0; ks < Tile::KS; ++ks) {
        if (qrow < T) qf[ks] = *reinterpret_cast<const vit_h8*>(q + base + (int64_t)qrow * hidden + ks * 16 + 8 * h);
        else
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[ks][e] = (dn_half)0.f;
    }
    Tile tile;
    tile.init();

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
    for (int kv0 = 0; kv0 < T; kv0 += VA_BKV) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(&Ks[(2 * lr + i) * Tile::LDK + 8 * lc]) = rk[i];
        {   // V transposed: the two rows' values of one d are neighbours in V^T, one 4-byte store per d
            const vit_h8 v0 = *reinterpret_cast<const vit_h8*>(&rv[0]), v1 = *reinterpret_cast<const vit_h8*>(&rv[1]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                vit_h2 pr;
                pr[0] = v0[e];
                pr[1] = v1[e];
                *reinterpret_cast<vit_h2*>(&Vt[(8 * lc + e) * VA_LDV + 2 * lr]) = pr;
            }
        }
        __syncthreads();
        if (kv0 + VA_BKV < T) load(kv0 + VA_BKV);

        const bool tail = kv0 + VA_BKV > T;     // row kv0 of the tile is valid, so the tile's maximum is finite
        tile.step(Ks, Vt, qf, r, h, [&](float raw, int jj) {
            const float sv = raw * DA_LOG2E_8;
            return tail && kv0 + jj >= T ? -INFINITY : sv;
        });
    }
    if (qrow >= T) return;
    tile.store(o + base + (int64_t)qrow * hidden, h);
}

static int dn_attn(const dn_half* q, const dn_half* k, const dn_half* v, dn_half* o, int B, int T, int heads, hipStream_t s) {
    if (B < 1 || B > 65535 || T < 1 || heads < 1 || heads > 65535) {
        gsr_set_error("dino attn: B %d, T %d and heads %d must be >= 1 (B, heads <= 65535)", B, T, heads);
        return GSR_E_INVALID;
    }
    if (!q || !k || !v || !o) { gsr_set_error("dino attn: q / k / v / out is null"); return GSR_E_INVALID; }
    hipLaunchKernelGGL(dn_attn_kernel, dim3((unsigned)((T + VA_BQ - 1) / VA_BQ), (unsigned)heads, (unsigned)B), dim3(256), 0, s, q, k, v, o,
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
        Hp = H / VIT_PATCH;
        Wp = W / VIT_PATCH;
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
        patches = cur.take<dn_half>((size_t)B * Hp * Wp * VIT_PATCH_K * 2);
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
    GSR_TRY(dn_check_cfg(cfg));
    GSR_TRY(dn_check_image(B, H, W));
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
    GSR_TRY(dn_embed(cfg, x0, x1, B, H, W, wp(GSR_DINO_W_CLS), wp(GSR_DINO_W_REG), wp(GSR_DINO_W_PATCH_W), wp(GSR_DINO_W_PATCH_B),
                     lay.patches, lay.resid, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const int w0 = GSR_DINO_W_LAYER0 + GSR_DINO_W_PER_LAYER * l;
        GSR_TRY(dn_norm(lay.resid, M, hid, hid, wp(w0 + GSR_DINO_L_NORM1_W), wp(w0 + GSR_DINO_L_NORM1_B), cfg->ln_eps, lay.xn, 0, s));
        GSR_TRY(dn_linear(lay.xn, wp(w0 + GSR_DINO_L_Q_W), wp(w0 + GSR_DINO_L_Q_B), nullptr, lay.q, M, hid, hid, DN_EPI_BIAS, s));
        GSR_TRY(dn_linear(lay.xn, wp(w0 + GSR_DINO_L_K_W), wp(w0 + GSR_DINO_L_K_B), nullptr, lay.k, M, hid, hid, DN_EPI_BIAS, s));
        GSR_TRY(dn_linear(lay.xn, wp(w0 + GSR_DINO_L_V_W), wp(w0 + GSR_DINO_L_V_B), nullptr, lay.v, M, hid, hid, DN_EPI_BIAS, s));
        GSR_TRY(dn_rope(lay.q, lay.k, B, T, cfg->heads, lay.Hp, lay.Wp, cfg->rope_theta, s));
        GSR_TRY(dn_attn(lay.q, lay.k, lay.v, lay.att, B, T, cfg->heads, s));
        GSR_TRY(dn_linear(lay.att, wp(w0 + GSR_DINO_L_O_W), wp(w0 + GSR_DINO_L_O_B), wp(w0 + GSR_DINO_L_LS1), lay.resid, M, hid, hid, DN_EPI_RESID, s));
        GSR_TRY(dn_norm(lay.resid, M, hid, hid, wp(w0 + GSR_DINO_L_NORM2_W), wp(w0 + GSR_DINO_L_NORM2_B), cfg->ln_eps, lay.xn, 0, s));
        GSR_TRY(dn_linear(lay.xn, wp(w0 + GSR_DINO_L_UP_W), wp(w0 + GSR_DINO_L_UP_B), nullptr, lay.mlp, M, hid, inter, DN_EPI_GELU, s));
        GSR_TRY(dn_linear(lay.mlp, wp(w0 + GSR_DINO_L_DOWN_W), wp(w0 + GSR_DINO_L_DOWN_B), wp(w0 + GSR_DINO_L_LS2), lay.resid, M, inter, hid, DN_EPI_RESID, s));
    }
    // DN_POOL: the final LayerNorm in f32; row 0 of each image is the pooled output (the same kernel on the same row: same bits)
    GSR_TRY(dn_norm(lay.resid, B, hid, (int64_t)T * hid, wp(n_weights - 2), wp(n_weights - 1), cfg->ln_eps, pooled, 1, s));
    if (last_hidden) GSR_TRY(dn_norm(lay.resid, M, hid, hid, wp(n_weights - 2), wp(n_weights - 1), cfg->ln_eps, last_hidden, 1, s));
    return GSR_OK;
}
