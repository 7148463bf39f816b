// SAM2's image encoder (transformers' Sam2VisionModel: the Hiera trunk and the FPN neck, plus what Sam2Model.get_image_features
// and get_image_embeddings add for a still image) as kernels.  The rules are in include/gsr.h (HV_EMBED, HV_LINEAR, HV_ATTN,
// HV_POOL, HV_NECK); each has one named place below, except HV_LINEAR, which is DN_LINEAR's body in vit.hip.  The LayerNorms
// are DN_NORM's, the attention tile is vit_attn.h's.  No split-K, no atomics: the bits are the same on every run, and a
// window's output depends on its own tokens only.
#include "cloud_common.h"
#include "vit_attn.h"

#define HV_MAX_GRID 256             // tokens per side of the first stage
#define HV_STAGES 4
#define HV_PATCH_K 152              // 3 x 7 x 7 = 147, zero-padded to a multiple of 8
#define HV_LOG2E 1.44269504088896340736f

// ---------------------------------------------------------------- HV_EMBED (gather)
// patches[p][c 49 + ky 7 + kx] = fp16(x[c, 4 py + ky - 3, 4 px + kx - 3]), zero outside the image (only rows and columns < 0
// can be: 4 (g - 1) + 3 = S - 1) and for k = 147 .. 151.  A thread writes 8 consecutive k of one patch row.
__global__ void __launch_bounds__(256) hv_im2col_kernel(const float* __restrict__ x, int S, int g, dn_half* __restrict__ patches) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g * g * (HV_PATCH_K / 8)) return;
    const int64_t row = i / (HV_PATCH_K / 8);
    const int part = (int)(i - row * (HV_PATCH_K / 8));
    const int py = (int)(row / g), px = (int)(row - (int64_t)py * g);
    vit_h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = 8 * part + e;
        const int c = k / 49, tap = k - 49 * c, ky = tap / 7, kx = tap - 7 * ky;
        const int y = 4 * py + ky - 3, xx = 4 * px + kx - 3;
        v[e] = (k < 147 && y >= 0 && xx >= 0) ? (dn_half)x[((int64_t)c * S + y) * S + xx] : (dn_half)0.f;
    }
    *reinterpret_cast<vit_h8*>(patches + row * HV_PATCH_K + 8 * part) = v;
}

static int hv_check_image(int S) {
    if (S < 4 || S % 4 != 0 || S / 4 > HV_MAX_GRID) {
        gsr_set_error("sam2: image_size %d must be a multiple of 4 in 4 .. %d", S, 4 * HV_MAX_GRID);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

static int hv_embed(const float* x, int S, int embed, const dn_half* pw, const dn_half* pb, const dn_half* pos, dn_half* patches,
                    float* out, hipStream_t s) {
    const int g = S / 4;
    const int64_t n = (int64_t)g * g * (HV_PATCH_K / 8);
    hipLaunchKernelGGL(hv_im2col_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, S, g, patches);
    GSR_LAUNCH_CHECK();
    return dn_linear_k8(patches, pw, pb, pos, out, (int64_t)g * g, HV_PATCH_K, embed, DN_EPI_POS, s);
}

extern "C" size_t gsr_sam2_embed_workspace_bytes(int32_t S) {
    if (S < 4) return 0;
    return gsr_align((size_t)(S / 4) * (size_t)(S / 4) * HV_PATCH_K * 2);
}

extern "C" int32_t gsr_sam2_embed(const float* pixel_values, int32_t S, int32_t embed, const void* patch_w, const void* patch_b,
                                  const void* pos_table, void* ws, size_t ws_bytes, float* out, gsr_stream_t stream_) {
    GSR_TRY(hv_check_image(S));
    if (embed < 1) { gsr_set_error("sam2 embed: embed %d must be >= 1", embed); return GSR_E_INVALID; }
    if (!pixel_values || !patch_w || !patch_b || !pos_table || !out) {
        gsr_set_error("sam2 embed: pixel_values / patch_w / patch_b / pos_table / out is null");
        return GSR_E_INVALID;
    }
    if (!vit_check_ws("sam2 embed", ws, ws_bytes, gsr_sam2_embed_workspace_bytes(S))) return GSR_E_INVALID;
    return hv_embed(pixel_values, S, embed, static_cast<const dn_half*>(patch_w), static_cast<const dn_half*>(patch_b),
                    static_cast<const dn_half*>(pos_table), static_cast<dn_half*>(ws), out, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- HV_LINEAR
extern "C" int32_t gsr_sam2_linear(const void* x, const void* w, const void* bias, const void* lambda, int64_t M, int32_t K,
                                   int32_t N, int32_t epilogue, void* out, gsr_stream_t stream_) {
    if (epilogue != DN_EPI_BIAS && epilogue != DN_EPI_GELU && epilogue != DN_EPI_RESID && epilogue != DN_EPI_RESID1 &&
        epilogue != DN_EPI_F32) {
        gsr_set_error("sam2 linear: epilogue %d is not GSR_DINO_EPI_BIAS, _GELU, _RESID, GSR_SAM2_EPI_RESID1 or _F32", epilogue);
        return GSR_E_INVALID;
    }
    return dn_linear_k8(static_cast<const dn_half*>(x), static_cast<const dn_half*>(w), static_cast<const dn_half*>(bias),
                        static_cast<const dn_half*>(lambda), out, M, K, N, epilogue, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- HV_ATTN
// The tile of vit_attn.h over the s s keys of one window (s = g: the whole grid).  HD is the tile's width, hd <= HD the head's
// own (a multiple of 8): the 16-byte chunks of q, k and v past hd are zeros in the fragments and in LDS, and are not stored.
// A workgroup owns up to 128 queries of one head of one window, a wave 32 of them; a window with fewer queries is launched
// with fewer waves.  stride 2: query (i, j) of the window is the elementwise maximum of the four fp16 q rows (2 i .. 2 i + 1,
// 2 j .. 2 j + 1), taken while the fragment is loaded, and its output goes to the g / 2 grid.  Keys past s s are never read
// (scores -inf before the maximum).  The base-2 score is (raw scale) log2(e).
template <int HD>
__global__ void __launch_bounds__(256) hv_attn_kernel(const dn_half* __restrict__ qkv, dn_half* __restrict__ o, int g, int s, int nwx,
                                                      int stride, int heads, int hd, float scale) {
    typedef VitAttnTile<HD> Tile;
    constexpr int KS = Tile::KS, DT = Tile::DT, LDK = Tile::LDK, CHT = HD / 8;
    __shared__ __attribute__((aligned(16))) dn_half Ks[VA_BKV * LDK];       // [kv][d]
    __shared__ __attribute__((aligned(16))) dn_half Vt[DT * 32 * VA_LDV];   // [d][kv]
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int hidden = heads * hd, ch = hd >> 3;
    const int64_t ld = 3 * (int64_t)hidden;
    const int head = (int)blockIdx.y, win = (int)blockIdx.z, wy = win / nwx, wx = win - wy * nwx;
    const int S2 = s * s, sq = s / stride, go = g / stride;
    const int ql = (int)blockIdx.x * VA_BQ + wave * 32 + r;
    const int qh = ql / sq, qw = ql - qh * sq;
    const bool qok = ql < sq * sq;
    // the query's first token on the input grid, and its place on the output grid
    const int64_t qtok = qok ? (int64_t)(wy * s + qh * stride) * g + wx * s + qw * stride : 0;
    const int64_t otok = qok ? (int64_t)(wy * sq + qh) * go + wx * sq + qw : 0;
    vit_h8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int col = ks * 16 + 8 * h;
        if (qok && col < hd) {
            const dn_half* src = qkv + qtok * ld + head * hd + col;
            vit_h8 a = *reinterpret_cast<const vit_h8*>(src);
            if (stride == 2) {
                const vit_h8 b = *reinterpret_cast<const vit_h8*>(src + ld), c = *reinterpret_cast<const vit_h8*>(src + (int64_t)g * ld),
                             d = *reinterpret_cast<const vit_h8*>(src + (int64_t)g * ld + ld);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const dn_half m0 = b[e] > a[e] ? b[e] : a[e], m1 = d[e] > c[e] ? d[e] : c[e];
                    a[e] = m1 > m0 ? m1 : m0;
                }
            }
            qf[ks] = a;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[ks][e] = (dn_half)0.f;
        }
    }
    for (int i = HD * VA_LDV + t; i < DT * 32 * VA_LDV; i += nt) Vt[i] = (dn_half)0.f;     // rows HD .. 32 DT - 1: never stored below
    Tile tile;
    tile.init();

    for (int kv0 = 0; kv0 < S2; kv0 += VA_BKV) {
        __syncthreads();            // the previous tile's reads are done
        for (int c = t; c < VA_BKV * CHT; c += nt) {
            const int row = c / CHT, col = c - row * CHT, j = kv0 + row;
            uint4 kk = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
            if (j < S2 && col < ch) {
                const int kh = j / s, kw = j - kh * s;
                const dn_half* src = qkv + ((int64_t)(wy * s + kh) * g + wx * s + kw) * ld + hidden + head * hd + 8 * col;
                kk = *reinterpret_cast<const uint4*>(src);
                vv = *reinterpret_cast<const uint4*>(src + hidden);
            }
            *reinterpret_cast<uint4*>(&Ks[row * LDK + 8 * col]) = kk;
            const vit_h8 v8 = *reinterpret_cast<const vit_h8*>(&vv);
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[(8 * col + e) * VA_LDV + row] = v8[e];
        }
        __syncthreads();

        // key kv0 of the tile is inside the window, so the tile's maximum is finite
        tile.step(Ks, Vt, qf, r, h, [&](float raw, int jj) { return kv0 + jj < S2 ? (raw * scale) * HV_LOG2E : -INFINITY; });
    }
    if (!qok) return;
    dn_half* orow = o + otok * hidden + head * hd;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int d0 = dt * 32 + 8 * q4 + 4 * h;
            if (d0 >= hd) continue;
            vit_h4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = (dn_half)(tile.acc[dt][4 * q4 + e] / tile.l_run);
            *reinterpret_cast<vit_h4*>(orow + d0) = out;
        }
}

static int hv_check_attn(int g, int w, int stride, int heads, int hd) {
    if (g < 1 || g > HV_MAX_GRID) { gsr_set_error("sam2 attn: grid %d is outside 1 .. %d", g, HV_MAX_GRID); return GSR_E_INVALID; }
    if (hd != 56 && hd != 64 && hd != 72 && hd != 80 && hd != 96) {
        gsr_set_error("sam2 attn: head_dim %d is not built (56, 64, 72, 80 and 96 are)", hd);
        return GSR_E_INVALID;
    }
    if (heads < 1 || heads > 1024) { gsr_set_error("sam2 attn: heads %d is outside 1 .. 1024", heads); return GSR_E_INVALID; }
    if (stride != 1 && stride != 2) { gsr_set_error("sam2 attn: query stride %d is not 1 or 2", stride); return GSR_E_INVALID; }
    if (w < 0 || w > g) { gsr_set_error("sam2 attn: window %d must be 0 (global) or 1 .. the grid %d", w, g); return GSR_E_INVALID; }
    if (w == 0 && stride != 1) { gsr_set_error("sam2 attn: a global block cannot pool its queries (it cannot be a stage start)"); return GSR_E_INVALID; }
    const int s = w == 0 ? g : w;
    if (g % s != 0) { gsr_set_error("sam2 attn: the grid %d is not a multiple of the window %d", g, s); return GSR_E_INVALID; }
    if (s % stride != 0) { gsr_set_error("sam2 attn: the window %d is not a multiple of the query stride %d", s, stride); return GSR_E_INVALID; }
    if ((g / s) * (g / s) > 65535) { gsr_set_error("sam2 attn: %d windows exceed the launch grid", (g / s) * (g / s)); return GSR_E_UNSUPPORTED; }
    return GSR_OK;
}

// arguments are checked by the callers (hv_check_attn, non-null pointers)
static int hv_attn(const dn_half* qkv, int g, int w, int stride, int heads, int hd, dn_half* out, hipStream_t st) {
    const int s = w == 0 ? g : w, nw = g / s, nq = (s / stride) * (s / stride);
    const float scale = (float)(1.0 / sqrt((double)hd));
    const dim3 grid((unsigned)((nq + VA_BQ - 1) / VA_BQ), (unsigned)heads, (unsigned)(nw * nw));
    const int waves = nq >= VA_BQ ? 4 : (nq + 31) / 32;
    const dim3 block(64 * waves);
    if (hd <= 64) hipLaunchKernelGGL(hv_attn_kernel<64>, grid, block, 0, st, qkv, out, g, s, nw, stride, heads, hd, scale);
    else if (hd <= 80) hipLaunchKernelGGL(hv_attn_kernel<80>, grid, block, 0, st, qkv, out, g, s, nw, stride, heads, hd, scale);
    else hipLaunchKernelGGL(hv_attn_kernel<96>, grid, block, 0, st, qkv, out, g, s, nw, stride, heads, hd, scale);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_sam2_attn(const void* qkv, int32_t g, int32_t window, int32_t query_stride, int32_t heads, int32_t head_dim,
                                 void* out, gsr_stream_t stream_) {
    GSR_TRY(hv_check_attn(g, window, query_stride, heads, head_dim));
    if (!qkv || !out) { gsr_set_error("sam2 attn: qkv / out is null"); return GSR_E_INVALID; }
    return hv_attn(static_cast<const dn_half*>(qkv), g, window, query_stride, heads, head_dim, static_cast<dn_half*>(out),
                   static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- HV_POOL
// out[(y, x)][c] = max of in[(2 y + a, 2 x + b)][c], a, b in {0, 1}: fp32, exact
__global__ void __launch_bounds__(256) hv_pool_kernel(const float* __restrict__ in, int g, int Cn, float* __restrict__ out) {
    const int go = g / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)go * go * Cn) return;
    const int c = (int)(i % Cn);
    const int64_t tok = i / Cn;
    const int y = (int)(tok / go), x = (int)(tok - (int64_t)y * go);
    const float* p = in + ((int64_t)(2 * y) * g + 2 * x) * Cn + c;
    out[i] = fmaxf(fmaxf(p[0], p[Cn]), fmaxf(p[(int64_t)g * Cn], p[(int64_t)g * Cn + Cn]));
}

static int hv_pool(const float* in, int g, int Cn, float* out, hipStream_t s) {
    const int64_t n = (int64_t)(g / 2) * (g / 2) * Cn;
    hipLaunchKernelGGL(hv_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, g, Cn, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_sam2_pool(const float* x, int32_t g, int32_t channels, float* out, gsr_stream_t stream_) {
    if (g < 2 || g > HV_MAX_GRID || g % 2 != 0) { gsr_set_error("sam2 pool: grid %d must be even in 2 .. %d", g, HV_MAX_GRID); return GSR_E_INVALID; }
    if (channels < 1 || channels > (1 << 20)) { gsr_set_error("sam2 pool: channels %d is outside 1 .. 2^20", channels); return GSR_E_INVALID; }
    if (!x || !out) { gsr_set_error("sam2 pool: x / out is null"); return GSR_E_INVALID; }
    return hv_pool(x, g, channels, out, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- HV_NECK
// lat[(y, x)][c] += up[(y / 2, x / 2)][c]: the top-down path's nearest up-sampling by 2 and its one fp32 addition, in place
__global__ void __launch_bounds__(256) hv_topdown_kernel(float* __restrict__ lat, const float* __restrict__ up, int g, int Cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g * g * Cn) return;
    const int c = (int)(i % Cn);
    const int64_t tok = i / Cn;
    const int y = (int)(tok / g), x = (int)(tok - (int64_t)y * g);
    lat[i] = lat[i] + up[((int64_t)(y / 2) * (g / 2) + x / 2) * Cn + c];
}

struct HvNeckLayout {
    size_t total;
    dn_half* xh[HV_STAGES];     // the stage-end streams rounded to fp16
    float* lat[HV_STAGES];      // the lateral maps, then the top-down sums, [T_i,D]
    dn_half* ph;                // a level's sum rounded to fp16 for conv_s0 / conv_s1
    float* cs;                  // their output before the transposition
    HvNeckLayout(int g0, int embed, int D, void* ws) {
        GsrWsCursor cur(ws);
        for (int i = 0; i < HV_STAGES; ++i) {
            const size_t T = (size_t)(g0 >> i) * (g0 >> i);
            xh[i] = cur.take<dn_half>(T * ((size_t)embed << i) * 2);
            lat[i] = cur.take<float>(T * D * 4);
        }
        ph = cur.take<dn_half>((size_t)g0 * g0 * D * 2);
        cs = cur.take<float>((size_t)g0 * g0 * (D / 4) * 4);
        total = cur.off;
    }
};

static int hv_check_neck(int g0, int embed, int D, int top_down_mask) {
    if (g0 < 8 || g0 > HV_MAX_GRID || g0 % 8 != 0) { gsr_set_error("sam2 neck: the first grid %d must be a multiple of 8 in 8 .. %d", g0, HV_MAX_GRID); return GSR_E_INVALID; }
    if (embed < 8 || embed % 8 != 0 || embed > 4096) { gsr_set_error("sam2 neck: embed %d must be a multiple of 8 in 8 .. 4096", embed); return GSR_E_INVALID; }
    if (D < 64 || D % 64 != 0 || D > 4096) { gsr_set_error("sam2 neck: fpn_hidden %d must be a multiple of 64 in 64 .. 4096", D); return GSR_E_INVALID; }
    if (top_down_mask < 0 || top_down_mask > 15) { gsr_set_error("sam2 neck: top_down_mask %d is outside 0 .. 15", top_down_mask); return GSR_E_INVALID; }
    return GSR_OK;
}

static int hv_neck_cast(const float* x, int i, int g0, int embed, const HvNeckLayout& lay, hipStream_t s) {
    const int64_t n = (int64_t)(g0 >> i) * (g0 >> i) * ((int64_t)embed << i);
    return vit_cast(x, n, lay.xh[i], s);
}

// nw: the GSR_SAM2_W_NECK entries of the weight table; the four streams are in lay.xh already
static int hv_neck_finish(int g0, int embed, int D, int top_down_mask, const void* const* nw, const HvNeckLayout& lay, float* out0,
                          float* out1, float* out2, hipStream_t s) {
    auto hp = [&](int i) { return static_cast<const dn_half*>(nw[i]); };
    for (int i = HV_STAGES - 1; i >= 0; --i) {
        const int g = g0 >> i;
        GSR_TRY(dn_linear_k8(lay.xh[i], hp(2 * i), hp(2 * i + 1), nullptr, lay.lat[i], (int64_t)g * g, embed << i, D, DN_EPI_F32, s));
        if (i < HV_STAGES - 1 && ((top_down_mask >> i) & 1)) {
            const int64_t n = (int64_t)g * g * D;
            hipLaunchKernelGGL(hv_topdown_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lay.lat[i], lay.lat[i + 1], g, D);
            GSR_LAUNCH_CHECK();
        }
    }
    float* outs[2] = {out0, out1};
    for (int i = 0; i < 2; ++i) {           // conv_s0 on level 0, conv_s1 on level 1
        const int g = g0 >> i, Co = i == 0 ? D / 8 : D / 4;
        const int64_t T = (int64_t)g * g;
        GSR_TRY(vit_cast(lay.lat[i], T * D, lay.ph, s));
        GSR_TRY(dn_linear_k8(lay.ph, hp(8 + 2 * i), hp(9 + 2 * i), nullptr, lay.cs, T, D, Co, DN_EPI_F32, s));
        GSR_TRY(vit_transpose(lay.cs, T, Co, nullptr, outs[i], s));
    }
    const int64_t T2 = (int64_t)(g0 >> 2) * (g0 >> 2);
    return vit_transpose(lay.lat[2], T2, D, static_cast<const float*>(nw[12]), out2, s);
}

extern "C" size_t gsr_sam2_neck_workspace_bytes(int32_t g0, int32_t embed, int32_t fpn_hidden) {
    if (hv_check_neck(g0, embed, fpn_hidden, 0) != GSR_OK) return 0;
    return HvNeckLayout(g0, embed, fpn_hidden, nullptr).total;
}

extern "C" int32_t gsr_sam2_neck(const float* const* streams_host, int32_t g0, int32_t embed, int32_t fpn_hidden, int32_t top_down_mask,
                                 const void* const* neck_weights_host, void* ws, size_t ws_bytes, float* out0, float* out1, float* out2,
                                 gsr_stream_t stream_) {
    GSR_TRY(hv_check_neck(g0, embed, fpn_hidden, top_down_mask));
    if (!streams_host || !neck_weights_host || !out0 || !out1 || !out2) {
        gsr_set_error("sam2 neck: streams / weights / an output is null");
        return GSR_E_INVALID;
    }
    for (int i = 0; i < HV_STAGES; ++i)
        if (!streams_host[i]) { gsr_set_error("sam2 neck: stream %d is null", i); return GSR_E_INVALID; }
    for (int i = 0; i < GSR_SAM2_W_NECK; ++i)
        if (!neck_weights_host[i]) { gsr_set_error("sam2 neck: weight %d is null", i); return GSR_E_INVALID; }
    HvNeckLayout lay(g0, embed, fpn_hidden, ws);
    if (!vit_check_ws("sam2 neck", ws, ws_bytes, lay.total)) return GSR_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    for (int i = 0; i < HV_STAGES; ++i) GSR_TRY(hv_neck_cast(streams_host[i], i, g0, embed, lay, s));
    return hv_neck_finish(g0, embed, fpn_hidden, top_down_mask, neck_weights_host, lay, out0, out1, out2, s);
}

// ---------------------------------------------------------------- the whole encoder
static int hv_total_blocks(const GsrSam2Config* c) { return c->blocks[0] + c->blocks[1] + c->blocks[2] + c->blocks[3]; }

static bool hv_is_global(const GsrSam2Config* c, int block) {
    for (int i = 0; i < c->num_global; ++i)
        if (c->global_host[i] == block) return true;
    return false;
}

static int hv_check_cfg(const GsrSam2Config* c) {
    if (!c) { gsr_set_error("sam2: cfg is null"); return GSR_E_INVALID; }
    GSR_TRY(hv_check_image(c->image_size));
    if (c->query_stride[0] != 2 || c->query_stride[1] != 2) {
        gsr_set_error("sam2: query stride %dx%d is not built (2x2 is)", c->query_stride[0], c->query_stride[1]);
        return GSR_E_INVALID;
    }
    if (c->ln_eps != 1e-6f) { gsr_set_error("sam2: ln_eps %g is not 1e-6", (double)c->ln_eps); return GSR_E_INVALID; }
    if (c->num_global < 0 || c->num_global > 4096 || (c->num_global > 0 && !c->global_host)) {
        gsr_set_error("sam2: num_global %d is outside 0 .. 4096 or global_host is null", c->num_global);
        return GSR_E_INVALID;
    }
    const int g0 = c->image_size / 4;
    GSR_TRY(hv_check_neck(g0, c->dims[0], c->fpn_hidden, c->top_down_mask));
    int block = 0;
    for (int i = 0; i < HV_STAGES; ++i) {
        const int g = g0 >> i;
        if (c->blocks[i] < 1 || c->blocks[i] > 4096) { gsr_set_error("sam2: stage %d has %d blocks (1 .. 4096)", i, c->blocks[i]); return GSR_E_INVALID; }
        if (i > 0 && c->dims[i] != 2 * c->dims[i - 1]) {
            gsr_set_error("sam2: stage %d has width %d, not twice stage %d's %d", i, c->dims[i], i - 1, c->dims[i - 1]);
            return GSR_E_INVALID;
        }
        if (c->heads[i] < 1 || c->dims[i] % c->heads[i] != 0) {
            gsr_set_error("sam2: stage %d's width %d is not a multiple of its %d heads", i, c->dims[i], c->heads[i]);
            return GSR_E_INVALID;
        }
        if (c->windows[i] < 1) { gsr_set_error("sam2: stage %d's window %d must be >= 1", i, c->windows[i]); return GSR_E_INVALID; }
        for (int b = 0; b < c->blocks[i]; ++b, ++block) {
            const bool start = i > 0 && b == 0, glob = hv_is_global(c, block);
            if (start && glob) {
                gsr_set_error("sam2: block %d is global and the first of stage %d: a global block cannot pool its queries", block, i);
                return GSR_E_INVALID;
            }
            // a stage start runs on the previous stage's grid with the previous stage's window
            const int gb = start ? 2 * g : g, wb = glob ? 0 : (start ? c->windows[i - 1] : c->windows[i]);
            GSR_TRY(hv_check_attn(gb, wb, start ? 2 : 1, c->heads[i], c->dims[i] / c->heads[i]));
        }
    }
    return GSR_OK;
}

struct HvLayout {
    size_t total;
    float *resid[2], *proj;
    dn_half *xn, *qkv, *att, *mlp, *patches;
    void* neck;
    HvLayout(const GsrSam2Config* c, void* ws) {
        const int g0 = c->image_size / 4;
        const size_t row = (size_t)g0 * g0 * c->dims[0];        // tokens x width of stage 0: every later stage has half of it
        GsrWsCursor cur(ws);
        resid[0] = cur.take<float>(row * 4);
        resid[1] = cur.take<float>(row * 4);
        proj = cur.take<float>(row * 2 * 4);                    // a stage start's projected residual before the pooling
        xn = cur.take<dn_half>(row * 2);
        qkv = cur.take<dn_half>(row * 6 * 2);                   // a stage start's qkv: the old grid at three times the new width
        att = cur.take<dn_half>(row * 2);
        mlp = cur.take<dn_half>(row * 4 * 2);
        patches = cur.take<dn_half>((size_t)g0 * g0 * HV_PATCH_K * 2);
        neck = cur.take<void>(HvNeckLayout(g0, c->dims[0], c->fpn_hidden, nullptr).total);
        total = cur.off;
    }
};

extern "C" size_t gsr_sam2_workspace_bytes(const GsrSam2Config* cfg) {
    if (hv_check_cfg(cfg) != GSR_OK) return 0;
    return HvLayout(cfg, nullptr).total;
}

extern "C" int32_t gsr_sam2_num_weights(int32_t total_blocks) {
    return total_blocks < 1 ? 0 : GSR_SAM2_W_BLOCK0 + GSR_SAM2_W_PER_BLOCK * total_blocks + GSR_SAM2_W_NECK;
}

extern "C" int32_t gsr_sam2_encode(const GsrSam2Config* cfg, const void* const* weights_host, int32_t n_weights,
                                   const float* pixel_values, void* ws, size_t ws_bytes, float* out0, float* out1, float* out2,
                                   gsr_stream_t stream_) {
    GSR_TRY(hv_check_cfg(cfg));
    const int nblocks = hv_total_blocks(cfg);
    if (!weights_host || n_weights != gsr_sam2_num_weights(nblocks)) {
        gsr_set_error("sam2: the weight table is null or has %d entries (%d blocks need %d)", n_weights, nblocks, gsr_sam2_num_weights(nblocks));
        return GSR_E_INVALID;
    }
    {   // only the projection of a block that is no stage start may be absent
        int block = 0;
        for (int i = 0; i < HV_STAGES; ++i)
            for (int b = 0; b < cfg->blocks[i]; ++b, ++block)
                for (int f = 0; f < GSR_SAM2_W_PER_BLOCK; ++f) {
                    const bool optional = (f == GSR_SAM2_B_PROJ_W || f == GSR_SAM2_B_PROJ_B) && !(i > 0 && b == 0);
                    if (!optional && !weights_host[GSR_SAM2_W_BLOCK0 + GSR_SAM2_W_PER_BLOCK * block + f]) {
                        gsr_set_error("sam2: weight %d of block %d is null", f, block);
                        return GSR_E_INVALID;
                    }
                }
        if (!vit_check_table("sam2", weights_host, GSR_SAM2_W_BLOCK0) || !vit_check_table("sam2", weights_host, n_weights, n_weights - GSR_SAM2_W_NECK))
            return GSR_E_INVALID;
    }
    if (!pixel_values || !out0 || !out1 || !out2) { gsr_set_error("sam2: pixel_values / an output is null"); return GSR_E_INVALID; }
    HvLayout lay(cfg, ws);
    if (!vit_check_ws("sam2", ws, ws_bytes, lay.total)) return GSR_E_INVALID;
    auto wp = [&](int i) { return static_cast<const dn_half*>(weights_host[i]); };
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int g0 = cfg->image_size / 4;
    HvNeckLayout nl(g0, cfg->dims[0], cfg->fpn_hidden, lay.neck);
    int cur = 0;        // which of the two residual buffers holds the stream
    GSR_TRY(hv_embed(pixel_values, cfg->image_size, cfg->dims[0], wp(GSR_SAM2_W_PATCH_W), wp(GSR_SAM2_W_PATCH_B), wp(GSR_SAM2_W_POS),
                     lay.patches, lay.resid[cur], s));
    int block = 0;
    for (int i = 0; i < HV_STAGES; ++i) {
        const int g = g0 >> i, dim = cfg->dims[i], heads = cfg->heads[i], hd = dim / heads;
        const int64_t T = (int64_t)g * g;
        for (int b = 0; b < cfg->blocks[i]; ++b, ++block) {
            const int w0 = GSR_SAM2_W_BLOCK0 + GSR_SAM2_W_PER_BLOCK * block;
            const bool start = i > 0 && b == 0;
            const int win = hv_is_global(cfg, block) ? 0 : (start ? cfg->windows[i - 1] : cfg->windows[i]);
            if (start) {
                // n = LN1(x) on the old grid at the old width; residual = HV_POOL(proj(n)); the queries are pooled inside HV_ATTN
                const int din = dim / 2, gin = 2 * g;
                const int64_t Tin = 4 * T;
                GSR_TRY(dn_norm(lay.resid[cur], Tin, din, din, wp(w0 + GSR_SAM2_B_NORM1_W), wp(w0 + GSR_SAM2_B_NORM1_B), cfg->ln_eps, lay.xn, 0, s));
                GSR_TRY(dn_linear_k8(lay.xn, wp(w0 + GSR_SAM2_B_PROJ_W), wp(w0 + GSR_SAM2_B_PROJ_B), nullptr, lay.proj, Tin, din, dim, DN_EPI_F32, s));
                GSR_TRY(hv_pool(lay.proj, gin, dim, lay.resid[cur ^ 1], s));
                cur ^= 1;
                GSR_TRY(dn_linear_k8(lay.xn, wp(w0 + GSR_SAM2_B_QKV_W), wp(w0 + GSR_SAM2_B_QKV_B), nullptr, lay.qkv, Tin, din, 3 * dim, DN_EPI_BIAS, s));
                GSR_TRY(hv_attn(lay.qkv, gin, win, 2, heads, hd, lay.att, s));
            } else {
                GSR_TRY(dn_norm(lay.resid[cur], T, dim, dim, wp(w0 + GSR_SAM2_B_NORM1_W), wp(w0 + GSR_SAM2_B_NORM1_B), cfg->ln_eps, lay.xn, 0, s));
                GSR_TRY(dn_linear_k8(lay.xn, wp(w0 + GSR_SAM2_B_QKV_W), wp(w0 + GSR_SAM2_B_QKV_B), nullptr, lay.qkv, T, dim, 3 * dim, DN_EPI_BIAS, s));
                GSR_TRY(hv_attn(lay.qkv, g, win, 1, heads, hd, lay.att, s));
            }
            float* resid = lay.resid[cur];
            GSR_TRY(dn_linear_k8(lay.att, wp(w0 + GSR_SAM2_B_OUT_W), wp(w0 + GSR_SAM2_B_OUT_B), nullptr, resid, T, dim, dim, DN_EPI_RESID1, s));
            GSR_TRY(dn_norm(resid, T, dim, dim, wp(w0 + GSR_SAM2_B_NORM2_W), wp(w0 + GSR_SAM2_B_NORM2_B), cfg->ln_eps, lay.xn, 0, s));
            GSR_TRY(dn_linear_k8(lay.xn, wp(w0 + GSR_SAM2_B_MLP1_W), wp(w0 + GSR_SAM2_B_MLP1_B), nullptr, lay.mlp, T, dim, 4 * dim, DN_EPI_GELU, s));
            GSR_TRY(dn_linear_k8(lay.mlp, wp(w0 + GSR_SAM2_B_MLP2_W), wp(w0 + GSR_SAM2_B_MLP2_B), nullptr, resid, T, 4 * dim, dim, DN_EPI_RESID1, s));
        }
        GSR_TRY(hv_neck_cast(lay.resid[cur], i, g0, cfg->dims[0], nl, s));      // the stage-end stream, as HV_NECK reads it
    }
    return hv_neck_finish(g0, cfg->dims[0], cfg->fpn_hidden, cfg->top_down_mask, weights_host + (n_weights - GSR_SAM2_W_NECK), nl, out0, out1,
                          out2, s);
}
