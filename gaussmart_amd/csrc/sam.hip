// SAM automatic mask generation (transformers' SamVisionEncoder; the reference's identification/sam.py): the ViT image encoder
// with windowed attention and the decomposed relative-position bias, and the selection of the candidate masks, as kernels.
// The rules are in include/gsr.h (SV_EMBED, SV_ATTN, SV_NECK, SM_SCORE, SM_NMS, SM_EMIT); each has one named place below.
// The matrix products outside attention are DN_LINEAR's and the LayerNorms DN_NORM's (vit.hip, through vit_common.h).
// No split-K, no float atomics: the bits are the same on every run.
#include <climits>
#include "cloud_common.h"
#include "vit_attn.h"

#define SV_MAX_GRID 256             // tokens per side: g g windows of size 1 must fit the launch grid's z

// ---------------------------------------------------------------- SV_EMBED (gather)
// patches[p][c 256 + ky 16 + kx] = fp16(x[c,16 py + ky,16 px + kx]): DN_EMBED's k order, the input already normalised.
__global__ void __launch_bounds__(256) sv_im2col_kernel(const float* __restrict__ x, int S, int g, dn_half* __restrict__ patches) {
    VitPatchPart a;
    if (!vit_patch_part((int64_t)g * g, a)) return;
    const int py = (int)(a.row / g), px = (int)(a.row - (int64_t)py * g);
    const float* src = x + ((int64_t)a.c * S + (py * VIT_PATCH + a.ky)) * S + px * VIT_PATCH + a.kx0;
    vit_h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (dn_half)src[e];
    vit_patch_store(patches, a, v);
}

static int sv_embed(const float* x, int S, int hidden, const dn_half* pw, const dn_half* pb, const dn_half* pos, dn_half* patches,
                    float* out, hipStream_t s) {
    const int g = S / VIT_PATCH;
    hipLaunchKernelGGL(sv_im2col_kernel, dim3(vit_patch_blocks((int64_t)g * g)), dim3(256), 0, s, x, S, g, patches);
    GSR_LAUNCH_CHECK();
    return dn_linear(patches, pw, pb, pos, out, (int64_t)g * g, VIT_PATCH_K, hidden, DN_EPI_POS, s);
}

static int sv_check_image(int S) {
    if (S < VIT_PATCH || S % VIT_PATCH != 0 || S / VIT_PATCH > SV_MAX_GRID) {
        gsr_set_error("sam: image_size %d must be a multiple of 16 in 16 .. %d", S, VIT_PATCH * SV_MAX_GRID);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

extern "C" size_t gsr_sam_embed_workspace_bytes(int32_t S) {
    if (S < VIT_PATCH) return 0;
    return gsr_align((size_t)(S / VIT_PATCH) * (size_t)(S / VIT_PATCH) * VIT_PATCH_K * 2);
}

extern "C" int32_t gsr_sam_embed(const float* pixel_values, int32_t S, int32_t hidden, const void* patch_w, const void* patch_b,
                                 const void* pos_embed, void* ws, size_t ws_bytes, float* out, gsr_stream_t stream_) {
    GSR_TRY(sv_check_image(S));
    if (hidden < 1) { gsr_set_error("sam embed: hidden %d must be >= 1", hidden); return GSR_E_INVALID; }
    if (!pixel_values || !patch_w || !patch_b || !pos_embed || !out) {
        gsr_set_error("sam embed: pixel_values / patch_w / patch_b / pos_embed / out is null");
        return GSR_E_INVALID;
    }
    if (!vit_check_ws("sam embed", ws, ws_bytes, gsr_sam_embed_workspace_bytes(S))) return GSR_E_INVALID;
    return sv_embed(pixel_values, S, hidden, static_cast<const dn_half*>(patch_w), static_cast<const dn_half*>(patch_b),
                    static_cast<const dn_half*>(pos_embed), static_cast<dn_half*>(ws), out, static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- SV_ATTN: the bias pre-pass
// rel[((tok heads + head) 2 + axis) s + k] = sum_d fp32(q_d) fp32(R_axis[pos - k + s - 1][d]), pos the token's row (axis 0) or
// column (axis 1) inside its window: d ascending, every product exact in fp32 (two fp16 factors), one fp32 rounding per
// addition, stored as fp32.  T heads 2 s values: not a score matrix.
__global__ void __launch_bounds__(256) sv_rel_kernel(const dn_half* __restrict__ qkv, const dn_half* __restrict__ Rh,
                                                     const dn_half* __restrict__ Rw, int g, int s, int heads, int hd,
                                                     float* __restrict__ rel) {
    const int64_t n = (int64_t)g * g * heads * 2 * s;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % s);
    int64_t rest = i / s;
    const int axis = (int)(rest & 1);
    rest >>= 1;
    const int head = (int)(rest % heads);
    const int64_t tok = rest / heads;
    const int y = (int)(tok / g), x = (int)(tok - (int64_t)y * g);
    const int pos = axis ? x % s : y % s;
    const dn_half* q = qkv + tok * 3 * heads * hd + head * hd;
    const dn_half* R = (axis ? Rw : Rh) + (int64_t)(pos - k + s - 1) * hd;
    float acc = 0.f;
    for (int d = 0; d < hd; ++d) acc = fmaf((float)q[d], (float)R[d], acc);
    rel[i] = acc;
}

// ---------------------------------------------------------------- SV_ATTN
// The tile of vit_attn.h (DN_ATTN's scheme) over the s s positions of one window.  A workgroup of 4 waves owns 128 window
// positions of one head of one window; positions outside the grid are padded: as queries they are computed on zeros and never
// written, as keys they are real and their k and v are the k and v thirds of the qkv bias (what DN_LINEAR gives on a zero row),
// read from the bias itself: the padded layout is synthesised, not stored.  K and V tiles of 64 go through LDS (V transposed);
// positions past s s are zeros there and their scores -inf before the maximum.  The base-2 score is ((raw scale + bh) + bw)
// log2(e), the two bias terms from the pre-pass.  The bits of a window depend on its own data only.
#define SA_LOG2E 1.44269504088896340736f

template <int HD>
__global__ void __launch_bounds__(256) sv_attn_kernel(const dn_half* __restrict__ qkv, const dn_half* __restrict__ qkv_bias,
                                                      const float* __restrict__ rel, dn_half* __restrict__ o, int g, int s, int nwx,
                                                      int heads, float scale) {
    typedef VitAttnTile<HD> Tile;
    constexpr int KS = Tile::KS, DT = Tile::DT, LDK = Tile::LDK, CH = HD / 8;
    __shared__ __attribute__((aligned(16))) dn_half Ks[VA_BKV * LDK];       // [kv][d]
    __shared__ __attribute__((aligned(16))) dn_half Vt[DT * 32 * VA_LDV];   // [d][kv]
    __shared__ int s_kh[VA_BKV], s_kw[VA_BKV];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int hidden = heads * HD;
    const int64_t ld = 3 * (int64_t)hidden;
    const int head = (int)blockIdx.y, win = (int)blockIdx.z, wy = win / nwx, wx = win - wy * nwx;
    const int S2 = s * s;
    const int ql = (int)blockIdx.x * VA_BQ + wave * 32 + r;
    const int qh = ql / s, qw = ql - qh * s, qy = wy * s + qh, qx = wx * s + qw;
    const bool qok = ql < S2 && qy < g && qx < g;
    const int64_t qtok = qok ? (int64_t)qy * g + qx : 0;
    vit_h8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (qok) qf[ks] = *reinterpret_cast<const vit_h8*>(qkv + qtok * ld + head * HD + ks * 16 + 8 * h);
        else
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[ks][e] = (dn_half)0.f;
    }
    const float* relq = rel + (qtok * heads + head) * 2 * s;        // rh at [0, s), rw at [s, 2 s)
    for (int i = HD * VA_LDV + t; i < DT * 32 * VA_LDV; i += 256) Vt[i] = (dn_half)0.f;   // rows HD .. 32 DT - 1: never stored below
    Tile tile;
    tile.init();

    for (int kv0 = 0; kv0 < S2; kv0 += VA_BKV) {
        __syncthreads();            // the previous tile's reads are done
        for (int c = t; c < VA_BKV * CH; c += 256) {
            const int row = c / CH, col = c - row * CH, j = kv0 + row;
            uint4 kk = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
            if (j < S2) {
                const int kh = j / s, kw = j - kh * s, ky = wy * s + kh, kx = wx * s + kw;
                const dn_half* src = (ky < g && kx < g) ? qkv + ((int64_t)ky * g + kx) * ld + hidden : qkv_bias + hidden;
                src += head * HD + 8 * col;
                kk = *reinterpret_cast<const uint4*>(src);
                vv = *reinterpret_cast<const uint4*>(src + hidden);
            }
            *reinterpret_cast<uint4*>(&Ks[row * LDK + 8 * col]) = kk;
            const vit_h8 v8 = *reinterpret_cast<const vit_h8*>(&vv);
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[(8 * col + e) * VA_LDV + row] = v8[e];
        }
        if (t < VA_BKV) {
            const int j = kv0 + t;
            const int kh = j < S2 ? j / s : -1;
            s_kh[t] = kh;
            s_kw[t] = j < S2 ? j - kh * s : 0;
        }
        __syncthreads();

        // position kv0 of the tile is inside the window, so the tile's maximum is finite
        tile.step(Ks, Vt, qf, r, h, [&](float raw, int jj) {
            const int kh = s_kh[jj];
            float tv = -INFINITY;
            if (kh >= 0) {
                const float bh = qok ? relq[kh] : 0.f, bw = qok ? relq[s + s_kw[jj]] : 0.f;
                tv = ((raw * scale + bh) + bw) * SA_LOG2E;
            }
            return tv;
        });
    }
    if (!qok) return;
    tile.store(o + qtok * hidden + head * HD, h);
}


static int sv_check_attn(int g, int w, int heads, int hd, int rel_rows) {
    if (g < 1 || g > SV_MAX_GRID) { gsr_set_error("sam attn: grid %d is outside 1 .. %d", g, SV_MAX_GRID); return GSR_E_INVALID; }
    if (hd != 64 && hd != 80) { gsr_set_error("sam attn: head_dim %d is not built (64 and 80 are)", hd); return GSR_E_INVALID; }
    if (heads < 1 || heads > 1024) { gsr_set_error("sam attn: heads %d is outside 1 .. 1024", heads); return GSR_E_INVALID; }
    if (w < 0 || w > SV_MAX_GRID) { gsr_set_error("sam attn: window %d must be 0 (global) or 1 .. %d", w, SV_MAX_GRID); return GSR_E_INVALID; }
    const int s = w == 0 ? g : w;
    if (rel_rows != 2 * s - 1) {
        gsr_set_error("sam attn: a relative-position table of %d rows where a layer of size %d needs exactly %d (the tables are "
                      "never interpolated)", rel_rows, s, 2 * s - 1);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

static size_t sv_rel_bytes(int g, int s, int heads) { return gsr_align((size_t)g * g * heads * 2 * s * 4); }

// arguments are checked by the callers (sv_check_attn, non-null pointers)
static int sv_attn(const dn_half* qkv, const dn_half* qkv_bias, const dn_half* Rh, const dn_half* Rw, int g, int w, int heads, int hd,
                   float* rel, dn_half* out, hipStream_t st) {
    const int s = w == 0 ? g : w, nw = (g + s - 1) / s;
    const int64_t n_rel = (int64_t)g * g * heads * 2 * s;
    hipLaunchKernelGGL(sv_rel_kernel, dim3((unsigned)((n_rel + 255) / 256)), dim3(256), 0, st, qkv, Rh, Rw, g, s, heads, hd, rel);
    GSR_LAUNCH_CHECK();
    const float scale = (float)(1.0 / sqrt((double)hd));
    const dim3 grid((unsigned)((s * s + VA_BQ - 1) / VA_BQ), (unsigned)heads, (unsigned)(nw * nw));
    if (hd == 64) hipLaunchKernelGGL(sv_attn_kernel<64>, grid, dim3(256), 0, st, qkv, qkv_bias, rel, out, g, s, nw, heads, scale);
    else hipLaunchKernelGGL(sv_attn_kernel<80>, grid, dim3(256), 0, st, qkv, qkv_bias, rel, out, g, s, nw, heads, scale);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" size_t gsr_sam_attn_workspace_bytes(int32_t g, int32_t window, int32_t heads) {
    if (g < 1 || g > SV_MAX_GRID || window < 0 || window > SV_MAX_GRID || heads < 1 || heads > 1024) return 0;
    return sv_rel_bytes(g, window == 0 ? g : window, heads);
}

extern "C" int32_t gsr_sam_attn(const void* qkv, const void* qkv_bias, const void* rel_pos_h, const void* rel_pos_w, int32_t rel_rows,
                                int32_t g, int32_t window, int32_t heads, int32_t head_dim, void* ws, size_t ws_bytes, void* out,
                                gsr_stream_t stream_) {
    GSR_TRY(sv_check_attn(g, window, heads, head_dim, rel_rows));
    if (!qkv || !qkv_bias || !rel_pos_h || !rel_pos_w || !out) {
        gsr_set_error("sam attn: qkv / qkv_bias / rel_pos_h / rel_pos_w / out is null");
        return GSR_E_INVALID;
    }
    if (!vit_check_ws("sam attn", ws, ws_bytes, gsr_sam_attn_workspace_bytes(g, window, heads))) return GSR_E_INVALID;
    return sv_attn(static_cast<const dn_half*>(qkv), static_cast<const dn_half*>(qkv_bias), static_cast<const dn_half*>(rel_pos_h),
                   static_cast<const dn_half*>(rel_pos_w), g, window, heads, head_dim, static_cast<float*>(ws),
                   static_cast<dn_half*>(out), static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- SV_NECK
// col[t][c 9 + ky 3 + kx] = ln[(y + ky - 1) g + (x + kx - 1)][c], zero outside the grid: Conv2d's own weight order [C,C,3,3]
__global__ void __launch_bounds__(256) sv_im2col3_kernel(const dn_half* __restrict__ ln, int g, int Cn, dn_half* __restrict__ col) {
    const int64_t n = (int64_t)g * g * 9 * Cn;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % (9 * Cn));
    const int64_t tok = i / (9 * Cn);
    const int c = k / 9, tap = k - 9 * c, ky = tap / 3, kx = tap - 3 * ky;
    const int y = (int)(tok / g) + ky - 1, x = (int)(tok % g) + kx - 1;
    col[i] = (y >= 0 && y < g && x >= 0 && x < g) ? ln[((int64_t)y * g + x) * Cn + c] : (dn_half)0.f;
}

struct SvNeckLayout {
    size_t total;
    dn_half *xh, *ln, *col;
    float *c1, *c2;
    SvNeckLayout(int g, int hidden, int Cn, void* ws) {
        const size_t T = (size_t)g * g;
        GsrWsCursor cur(ws);
        xh = cur.take<dn_half>(T * hidden * 2);
        c1 = cur.take<float>(T * Cn * 4);
        ln = cur.take<dn_half>(T * Cn * 2);
        col = cur.take<dn_half>(T * 9 * Cn * 2);
        c2 = cur.take<float>(T * Cn * 4);
        total = cur.off;
    }
};

static int sv_neck(const float* x, int g, int hidden, int Cn, const dn_half* conv1, const dn_half* ln1w, const dn_half* ln1b,
                   const dn_half* conv2, const dn_half* ln2w, const dn_half* ln2b, float eps, const SvNeckLayout& lay, float* out,
                   hipStream_t s) {
    const int64_t T = (int64_t)g * g;
    GSR_TRY(vit_cast(x, T * hidden, lay.xh, s));
    GSR_TRY(dn_linear(lay.xh, conv1, nullptr, nullptr, lay.c1, T, hidden, Cn, DN_EPI_F32, s));
    GSR_TRY(dn_norm(lay.c1, T, Cn, Cn, ln1w, ln1b, eps, lay.ln, 0, s));
    hipLaunchKernelGGL(sv_im2col3_kernel, dim3((unsigned)((T * 9 * Cn + 255) / 256)), dim3(256), 0, s, lay.ln, g, Cn, lay.col);
    GSR_LAUNCH_CHECK();
    GSR_TRY(dn_linear(lay.col, conv2, nullptr, nullptr, lay.c2, T, 9 * Cn, Cn, DN_EPI_F32, s));
    GSR_TRY(dn_norm(lay.c2, T, Cn, Cn, ln2w, ln2b, eps, lay.c1, 1, s));
    GSR_TRY(vit_transpose(lay.c1, T, Cn, nullptr, out, s));
    return GSR_OK;
}

static int sv_check_neck(int g, int hidden, int Cn) {
    if (g < 1 || g > SV_MAX_GRID) { gsr_set_error("sam neck: grid %d is outside 1 .. %d", g, SV_MAX_GRID); return GSR_E_INVALID; }
    if (hidden < 64 || hidden % 64 != 0 || Cn < 64 || Cn % 64 != 0) {
        gsr_set_error("sam neck: hidden %d and output_channels %d must be positive multiples of 64", hidden, Cn);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

extern "C" size_t gsr_sam_neck_workspace_bytes(int32_t g, int32_t hidden, int32_t channels) {
    if (g < 1 || g > SV_MAX_GRID || hidden < 64 || channels < 64) return 0;
    return SvNeckLayout(g, hidden, channels, nullptr).total;
}

extern "C" int32_t gsr_sam_neck(const float* x, int32_t g, int32_t hidden, int32_t channels, const void* conv1_w, const void* ln1_w,
                                const void* ln1_b, const void* conv2_w, const void* ln2_w, const void* ln2_b, void* ws,
                                size_t ws_bytes, float* out, gsr_stream_t stream_) {
    GSR_TRY(sv_check_neck(g, hidden, channels));
    if (!x || !conv1_w || !ln1_w || !ln1_b || !conv2_w || !ln2_w || !ln2_b || !out) {
        gsr_set_error("sam neck: x / a weight / out is null");
        return GSR_E_INVALID;
    }
    SvNeckLayout lay(g, hidden, channels, ws);
    if (!vit_check_ws("sam neck", ws, ws_bytes, lay.total)) return GSR_E_INVALID;
    auto hp = [](const void* p) { return static_cast<const dn_half*>(p); };
    return sv_neck(x, g, hidden, channels, hp(conv1_w), hp(ln1_w), hp(ln1_b), hp(conv2_w), hp(ln2_w), hp(ln2_b), 1e-6f, lay, out,
                   static_cast<hipStream_t>(stream_));
}

// ---------------------------------------------------------------- the whole encoder
static int sv_check_cfg(const GsrSamConfig* c) {
    if (!c) { gsr_set_error("sam: cfg is null"); return GSR_E_INVALID; }
    GSR_TRY(sv_check_image(c->image_size));
    if (c->head_dim != 64 && c->head_dim != 80) { gsr_set_error("sam: head_dim %d is not built (64 and 80 are)", c->head_dim); return GSR_E_INVALID; }
    if (c->heads < 1 || c->heads > 1024 || c->hidden != c->heads * c->head_dim) {
        gsr_set_error("sam: hidden %d is not heads (%d) x head_dim (%d)", c->hidden, c->heads, c->head_dim);
        return GSR_E_INVALID;
    }
    if (c->hidden % 64 != 0 || c->mlp_dim < 64 || c->mlp_dim % 64 != 0 || c->output_channels < 64 || c->output_channels % 64 != 0) {
        gsr_set_error("sam: hidden %d, mlp_dim %d and output_channels %d must be positive multiples of 64", c->hidden, c->mlp_dim,
                      c->output_channels);
        return GSR_E_INVALID;
    }
    if (c->layers < 1 || c->layers > 4096) { gsr_set_error("sam: layers %d is outside 1 .. 4096", c->layers); return GSR_E_INVALID; }
    if (c->ln_eps != 1e-6f) { gsr_set_error("sam: ln_eps %g is not 1e-6", (double)c->ln_eps); return GSR_E_INVALID; }
    if (!c->window_host || !c->rel_rows_host) { gsr_set_error("sam: window_host / rel_rows_host is null"); return GSR_E_INVALID; }
    const int g = c->image_size / VIT_PATCH;
    for (int l = 0; l < c->layers; ++l)
        GSR_TRY(sv_check_attn(g, c->window_host[l], c->heads, c->head_dim, c->rel_rows_host[l]));
    return GSR_OK;
}

struct SvLayout {
    size_t total;
    float *resid, *rel;
    dn_half *xn, *qkv, *att, *mlp, *patches;
    void* neck;
    SvLayout(const GsrSamConfig* c, void* ws) {
        const int g = c->image_size / VIT_PATCH;
        const size_t T = (size_t)g * g, row = T * c->hidden;
        int smax = 1;
        for (int l = 0; l < c->layers; ++l) {
            const int sl = c->window_host[l] == 0 ? g : c->window_host[l];
            if (sl > smax) smax = sl;
        }
        GsrWsCursor cur(ws);
        resid = cur.take<float>(row * 4);
        xn = cur.take<dn_half>(row * 2);
        qkv = cur.take<dn_half>(row * 3 * 2);
        att = cur.take<dn_half>(row * 2);
        mlp = cur.take<dn_half>(T * c->mlp_dim * 2);
        patches = cur.take<dn_half>(T * VIT_PATCH_K * 2);
        rel = cur.take<float>(sv_rel_bytes(g, smax, c->heads));
        neck = cur.take<void>(SvNeckLayout(g, c->hidden, c->output_channels, nullptr).total);
        total = cur.off;
    }
};

extern "C" size_t gsr_sam_workspace_bytes(const GsrSamConfig* cfg) {
    if (sv_check_cfg(cfg) != GSR_OK) return 0;
    return SvLayout(cfg, nullptr).total;
}

extern "C" int32_t gsr_sam_num_weights(int32_t layers) { return layers < 1 ? 0 : GSR_SAM_W_LAYER0 + GSR_SAM_W_PER_LAYER * layers + GSR_SAM_W_NECK; }

extern "C" int32_t gsr_sam_encode(const GsrSamConfig* cfg, const void* const* weights_host, int32_t n_weights,
                                  const float* pixel_values, void* ws, size_t ws_bytes, float* out, gsr_stream_t stream_) {
    GSR_TRY(sv_check_cfg(cfg));
    if (!weights_host || n_weights != gsr_sam_num_weights(cfg->layers)) {
        gsr_set_error("sam: the weight table is null or has %d entries (%d layers need %d)", n_weights, cfg->layers,
                      gsr_sam_num_weights(cfg->layers));
        return GSR_E_INVALID;
    }
    if (!vit_check_table("sam", weights_host, n_weights)) return GSR_E_INVALID;
    if (!pixel_values || !out) { gsr_set_error("sam: pixel_values / out is null"); return GSR_E_INVALID; }
    SvLayout lay(cfg, ws);
    if (!vit_check_ws("sam", ws, ws_bytes, lay.total)) return GSR_E_INVALID;
    auto wp = [&](int i) { return static_cast<const dn_half*>(weights_host[i]); };
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int hid = cfg->hidden, g = cfg->image_size / VIT_PATCH;
    const int64_t T = (int64_t)g * g;
    GSR_TRY(sv_embed(pixel_values, cfg->image_size, hid, wp(GSR_SAM_W_PATCH_W), wp(GSR_SAM_W_PATCH_B), wp(GSR_SAM_W_POS), lay.patches,
                     lay.resid, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const int w0 = GSR_SAM_W_LAYER0 + GSR_SAM_W_PER_LAYER * l;
        GSR_TRY(dn_norm(lay.resid, T, hid, hid, wp(w0 + GSR_SAM_L_NORM1_W), wp(w0 + GSR_SAM_L_NORM1_B), cfg->ln_eps, lay.xn, 0, s));
        GSR_TRY(dn_linear(lay.xn, wp(w0 + GSR_SAM_L_QKV_W), wp(w0 + GSR_SAM_L_QKV_B), nullptr, lay.qkv, T, hid, 3 * hid, DN_EPI_BIAS, s));
        GSR_TRY(sv_attn(lay.qkv, wp(w0 + GSR_SAM_L_QKV_B), wp(w0 + GSR_SAM_L_REL_H), wp(w0 + GSR_SAM_L_REL_W), g, cfg->window_host[l],
                        cfg->heads, cfg->head_dim, lay.rel, lay.att, s));
        GSR_TRY(dn_linear(lay.att, wp(w0 + GSR_SAM_L_PROJ_W), wp(w0 + GSR_SAM_L_PROJ_B), nullptr, lay.resid, T, hid, hid, DN_EPI_RESID1, s));
        GSR_TRY(dn_norm(lay.resid, T, hid, hid, wp(w0 + GSR_SAM_L_NORM2_W), wp(w0 + GSR_SAM_L_NORM2_B), cfg->ln_eps, lay.xn, 0, s));
        GSR_TRY(dn_linear(lay.xn, wp(w0 + GSR_SAM_L_LIN1_W), wp(w0 + GSR_SAM_L_LIN1_B), nullptr, lay.mlp, T, hid, cfg->mlp_dim, DN_EPI_GELU, s));
        GSR_TRY(dn_linear(lay.mlp, wp(w0 + GSR_SAM_L_LIN2_W), wp(w0 + GSR_SAM_L_LIN2_B), nullptr, lay.resid, T, cfg->mlp_dim, hid, DN_EPI_RESID1, s));
    }
    const int n0 = n_weights - GSR_SAM_W_NECK;
    SvNeckLayout nl(g, hid, cfg->output_channels, lay.neck);
    return sv_neck(lay.resid, g, hid, cfg->output_channels, wp(n0), wp(n0 + 1), wp(n0 + 2), wp(n0 + 3), wp(n0 + 4), wp(n0 + 5), cfg->ln_eps,
                   nl, out, s);
}

// ---------------------------------------------------------------- SM_SCORE / SM_EMIT: the pixel value
struct SmGeom {
    int L, ih, iw, oh, ow, identity;
    float sh, sw;       // fp32(ih) / fp32(oh), fp32(iw) / fp32(ow): F.interpolate's scale when a size is given
    int direct;         // SAM2's one step: (L, L) -> (oh, ow) with ih = iw = L, the taps are the logits themselves
};

// F.interpolate(L -> 4 L, bilinear, align_corners=False) at pixel (Y, X): src = max(0.25 (Y + 0.5) - 0.5, 0), i0 = floor(src),
// i1 = min(i0 + 1, L - 1), lambda = src - i0; value = (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11), every
// operation one fp32 rounding, no contraction.
__device__ __forceinline__ float sm_up(const float* __restrict__ p, int L, int Y, int X) {
    const float sy = fmaxf(0.25f * ((float)Y + 0.5f) - 0.5f, 0.f), sx = fmaxf(0.25f * ((float)X + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)sy, L - 1), x0 = min((int)sx, L - 1);
    const int y1 = y0 + (y0 < L - 1), x1 = x0 + (x0 < L - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * p[y0 * L + x0] + lx * p[y0 * L + x1]) + ly * (hx * p[y1 * L + x0] + lx * p[y1 * L + x1]);
}

// the second F.interpolate, (ih, iw) -> (oh, ow), whose four taps are pixels of the first one's crop [:ih,:iw]
__device__ __forceinline__ float sm_value(const float* __restrict__ p, const SmGeom& G, int y, int x) {
    if (G.identity) return sm_up(p, G.L, y, x);
    const float sy = fmaxf(G.sh * ((float)y + 0.5f) - 0.5f, 0.f), sx = fmaxf(G.sw * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)sy, G.ih - 1), x0 = min((int)sx, G.iw - 1);
    const int y1 = y0 + (y0 < G.ih - 1), x1 = x0 + (x0 < G.iw - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    if (G.direct) return hy * (hx * p[y0 * G.L + x0] + lx * p[y0 * G.L + x1]) + ly * (hx * p[y1 * G.L + x0] + lx * p[y1 * G.L + x1]);
    return hy * (hx * sm_up(p, G.L, y0, x0) + lx * sm_up(p, G.L, y0, x1)) + ly * (hx * sm_up(p, G.L, y1, x0) + lx * sm_up(p, G.L, y1, x1));
}

// One workgroup per mask: thread t takes pixels t, t + 256, ... (row-major); int32 counts and box extremes, added / compared
// over the wave by a xor butterfly and over the four waves in order by thread 0.  Integer arithmetic: the order cannot show.
__global__ void __launch_bounds__(256) sm_score_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ skip, SmGeom G,
                                                       float tau, float tau_hi, float tau_lo, int32_t* __restrict__ counts,
                                                       float* __restrict__ boxes) {
    __shared__ int red[4][7];
    const int64_t mask = blockIdx.x;
    const int t = threadIdx.x;
    if (skip && skip[mask]) {       // uniform over the workgroup; the logits are not read
        if (t < 3) counts[mask * 3 + t] = 0;
        if (t < 4) boxes[mask * 4 + t] = 0.f;
        return;
    }
    const float* p = logits + mask * G.L * G.L;
    int v[7] = {0, 0, 0, INT_MAX, INT_MAX, -1, -1};        // area, inter, union, x0, y0, x1, y1
    const int npix = G.oh * G.ow;
    for (int i = t; i < npix; i += 256) {
        const int y = i / G.ow, x = i - y * G.ow;
        const float val = sm_value(p, G, y, x);
        v[1] += val > tau_hi;
        v[2] += val > tau_lo;
        if (val > tau) {
            v[0] += 1;
            v[3] = min(v[3], x);
            v[4] = min(v[4], y);
            v[5] = max(v[5], x);
            v[6] = max(v[6], y);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] += __shfl_xor(v[k], d, 64);
        v[3] = min(v[3], __shfl_xor(v[3], d, 64));
        v[4] = min(v[4], __shfl_xor(v[4], d, 64));
        v[5] = max(v[5], __shfl_xor(v[5], d, 64));
        v[6] = max(v[6], __shfl_xor(v[6], d, 64));
    }
    if ((t & 63) == 0)
#pragma unroll
        for (int k = 0; k < 7; ++k) red[t >> 6][k] = v[k];
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < 4; ++w) {
        for (int k = 0; k < 3; ++k) v[k] += red[w][k];
        v[3] = min(v[3], red[w][3]);
        v[4] = min(v[4], red[w][4]);
        v[5] = max(v[5], red[w][5]);
        v[6] = max(v[6], red[w][6]);
    }
    for (int k = 0; k < 3; ++k) counts[mask * 3 + k] = v[k];
    for (int k = 0; k < 4; ++k) boxes[mask * 4 + k] = v[0] > 0 ? (float)v[3 + k] : 0.f;
}

__global__ void __launch_bounds__(256) sm_emit_kernel(const float* __restrict__ logits, const int32_t* __restrict__ index, int n,
                                                      SmGeom G, float tau, uint8_t* __restrict__ out) {
    const int npix = G.oh * G.ow;
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int mask = index[blockIdx.y];
    uint8_t bit = 0;
    if (mask >= 0 && mask < n) {
        const int y = i / G.ow, x = i - y * G.ow;
        bit = sm_value(logits + (int64_t)mask * G.L * G.L, G, y, x) > tau;
    }
    out[(int64_t)blockIdx.y * npix + i] = bit;
}

static int sm_geom(int L, int ih, int iw, int oh, int ow, SmGeom* G) {
    if (L < 1 || L > 4096) { gsr_set_error("sam masks: L %d is outside 1 .. 4096", L); return GSR_E_INVALID; }
    if (ih < 1 || iw < 1 || ih > 4 * L || iw > 4 * L) {
        gsr_set_error("sam masks: the input size %dx%d must lie inside the %dx%d frame", ih, iw, 4 * L, 4 * L);
        return GSR_E_INVALID;
    }
    if (oh < 1 || ow < 1 || (int64_t)oh * ow > (1 << 28)) { gsr_set_error("sam masks: the output size %dx%d must be 1x1 .. 2^28 pixels", oh, ow); return GSR_E_INVALID; }
    G->L = L; G->ih = ih; G->iw = iw; G->oh = oh; G->ow = ow;
    G->identity = oh == ih && ow == iw;
    G->sh = (float)ih / (float)oh;
    G->sw = (float)iw / (float)ow;
    G->direct = 0;
    return GSR_OK;
}

// SAM2's postprocess_masks: one F.interpolate from the L x L logits to the mask size
static int sm_geom_direct(int L, int oh, int ow, SmGeom* G) {
    GSR_TRY(sm_geom(L, L, L, oh, ow, G));
    G->identity = 0;
    G->direct = 1;
    return GSR_OK;
}

static int sm_score(const SmGeom& G, const float* logits, int32_t n, float tau, float delta, const uint8_t* skip, int32_t* counts,
                    float* boxes, gsr_stream_t stream_) {
    if (n < 0) { gsr_set_error("sam mask score: n %d must be >= 0", n); return GSR_E_INVALID; }
    if (!(delta >= 0.f) || !(tau == tau)) { gsr_set_error("sam mask score: tau must be a number and delta >= 0"); return GSR_E_INVALID; }
    if (n == 0) return GSR_OK;
    if (!logits || !counts || !boxes) { gsr_set_error("sam mask score: logits / counts / boxes is null"); return GSR_E_INVALID; }
    hipLaunchKernelGGL(sm_score_kernel, dim3((unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream_), logits, skip, G, tau,
                       tau + delta, tau - delta, counts, boxes);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_sam_mask_score(const float* logits, int32_t n, int32_t L, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                                      float tau, float delta, const uint8_t* skip, int32_t* counts, float* boxes,
                                      gsr_stream_t stream_) {
    SmGeom G;
    GSR_TRY(sm_geom(L, ih, iw, oh, ow, &G));
    return sm_score(G, logits, n, tau, delta, skip, counts, boxes, stream_);
}

extern "C" int32_t gsr_sam_mask_score_direct(const float* logits, int32_t n, int32_t L, int32_t oh, int32_t ow, float tau, float delta,
                                             const uint8_t* skip, int32_t* counts, float* boxes, gsr_stream_t stream_) {
    SmGeom G;
    GSR_TRY(sm_geom_direct(L, oh, ow, &G));
    return sm_score(G, logits, n, tau, delta, skip, counts, boxes, stream_);
}

static int sm_emit(const SmGeom& G, const float* logits, int32_t n, float tau, const int32_t* index, int32_t m, uint8_t* out,
                   gsr_stream_t stream_) {
    const int oh = G.oh, ow = G.ow;
    if (n < 0 || m < 0 || m > 65535) { gsr_set_error("sam mask emit: n %d must be >= 0 and m %d in 0 .. 65535", n, m); return GSR_E_INVALID; }
    if (m == 0) return GSR_OK;
    if (!logits || !index || !out) { gsr_set_error("sam mask emit: logits / index / out is null"); return GSR_E_INVALID; }
    hipLaunchKernelGGL(sm_emit_kernel, dim3((unsigned)((oh * ow + 255) / 256), (unsigned)m), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       logits, index, n, G, tau, out);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

extern "C" int32_t gsr_sam_mask_emit(const float* logits, int32_t n, int32_t L, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                                     float tau, const int32_t* index, int32_t m, uint8_t* out, gsr_stream_t stream_) {
    SmGeom G;
    GSR_TRY(sm_geom(L, ih, iw, oh, ow, &G));
    return sm_emit(G, logits, n, tau, index, m, out, stream_);
}

extern "C" int32_t gsr_sam_mask_emit_direct(const float* logits, int32_t n, int32_t L, int32_t oh, int32_t ow, float tau,
                                            const int32_t* index, int32_t m, uint8_t* out, gsr_stream_t stream_) {
    SmGeom G;
    GSR_TRY(sm_geom_direct(L, oh, ow, &G));
    return sm_emit(G, logits, n, tau, index, m, out, stream_);
}

// ---------------------------------------------------------------- SM_NMS
#define SM_NMS_MAX (3 * 64 * 64)

// rank of candidate i among the candidates: how many precede it (higher score, or the same score and a lower index)
__global__ void __launch_bounds__(256) sm_rank_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ keep_in, int n,
                                                      int32_t* __restrict__ order) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (keep_in && !keep_in[i])) return;
    const float si = scores[i];
    if (!(si == si)) return;
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        if (keep_in && !keep_in[j]) continue;
        const float sj = scores[j];
        rank += (sj > si) || (sj == si && j < i);
    }
    order[rank] = i;
}

// One workgroup walks the candidates in order; all threads see the same flags after each barrier.
__global__ void __launch_bounds__(1024) sm_nms_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                      const uint8_t* __restrict__ keep_in, int n, float theta,
                                                      const int32_t* __restrict__ order, int32_t* __restrict__ kept,
                                                      int32_t* __restrict__ count) {
    __shared__ uint8_t supp[SM_NMS_MAX];
    __shared__ int s_m;
    const int t = threadIdx.x;
    if (t == 0) s_m = 0;
    __syncthreads();
    int mine = 0;
    for (int i = t; i < n; i += 1024) {
        supp[i] = 0;
        const float si = scores[i];
        mine += (!keep_in || keep_in[i]) && si == si;
    }
    if (mine) atomicAdd(&s_m, mine);        // an integer count in LDS
    __syncthreads();
    const int m = s_m;
    int n_kept = 0;
    for (int b = 0; b < m; ++b) {
        __syncthreads();
        if (supp[b]) continue;
        const int ib = order[b];
        if (t == 0) kept[n_kept] = ib;
        ++n_kept;
        const float bx0 = boxes[4 * ib], by0 = boxes[4 * ib + 1], bx1 = boxes[4 * ib + 2], by1 = boxes[4 * ib + 3];
        const float ab = (bx1 - bx0) * (by1 - by0);
        for (int c = b + 1 + t; c < m; c += 1024) {
            if (supp[c]) continue;
            const float* q = boxes + 4 * order[c];
            const float ac = (q[2] - q[0]) * (q[3] - q[1]);
            const float w = fmaxf(fminf(bx1, q[2]) - fmaxf(bx0, q[0]), 0.f), hgt = fmaxf(fminf(by1, q[3]) - fmaxf(by0, q[1]), 0.f);
            const float inter = w * hgt;
            const float iou = inter / (ab + ac - inter);
            if (iou > theta) supp[c] = 1;       // NaN compares false
        }
    }
    if (t == 0) *count = n_kept;
}

extern "C" size_t gsr_sam_nms_workspace_bytes(int32_t n) { return n < 1 ? 0 : gsr_align((size_t)n * 4); }

extern "C" int32_t gsr_sam_nms(const float* boxes, const float* scores, const uint8_t* keep_in, int32_t n, float theta, void* ws,
                               size_t ws_bytes, int32_t* kept, int32_t* count, gsr_stream_t stream_) {
    if (n < 1 || n > SM_NMS_MAX) { gsr_set_error("sam nms: n %d is outside 1 .. %d", n, SM_NMS_MAX); return GSR_E_INVALID; }
    if (!boxes || !scores || !kept || !count) { gsr_set_error("sam nms: boxes / scores / kept / count is null"); return GSR_E_INVALID; }
    if (!vit_check_ws("sam nms", ws, ws_bytes, gsr_sam_nms_workspace_bytes(n))) return GSR_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    int32_t* order = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(sm_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scores, keep_in, n, order);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sm_nms_kernel, dim3(1), dim3(1024), 0, s, boxes, scores, keep_in, n, theta, order, kept, count);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
