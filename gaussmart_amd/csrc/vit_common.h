// What the ViT kernels (dino.hip, sam.hip, sam2.hip, sam_decoder.hip) share: the DN_LINEAR and DN_NORM launchers with their epilogue
// values and the necks' cast and transpose (defined in vit.hip, rules in include/gsr.h), the fragment types of the 32x32x16 f16
// matrix instruction and the map of its accumulator, the erf GELU, the index arithmetic of the 16x16 patch gather, GSR_TRY, and
// the workspace and weight-table checks of the entry points.  The attention tile is in vit_attn.h.
#pragma once
#include "gsr_common.h"
#include "wave_reduce.h"

typedef _Float16 dn_half;
typedef _Float16 vit_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 vit_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 vit_h2 __attribute__((ext_vector_type(2)));
typedef float vit_f32x16 __attribute__((ext_vector_type(16)));

// return a launcher's code unless it is GSR_OK
#define GSR_TRY(call)                                      \
    do {                                                   \
        const int gsr_try_rc_ = (call);                    \
        if (gsr_try_rc_ != GSR_OK) return gsr_try_rc_;     \
    } while (0)

// ---------------------------------------------------------------- DN_LINEAR and DN_NORM (vit.hip)
// 0..3 are DINO's and keep their bits; 4..6 were added for SAM's encoder (no LayerScale, fp32 stores), 7 for SAM2's decoder.
enum {
    DN_EPI_BIAS = 0,    // fp16(acc + bias)
    DN_EPI_GELU = 1,    // fp16(gelu(acc + bias))
    DN_EPI_RESID = 2,   // resid = fma(lambda[n], acc + bias, resid), fp32
    DN_EPI_EMBED = 3,   // DINO's patch rows behind the prefix tokens, fp32
    DN_EPI_RESID1 = 4,  // resid = resid + (acc + bias), fp32
    DN_EPI_F32 = 5,     // acc + bias, fp32
    DN_EPI_POS = 6,     // (acc + bias) + fp32(lam[m N + n]), fp32: lam is an fp16 [M,N] table here
    DN_EPI_SKIP_GELU = 7    // fp16(gelu((acc + bias) + tab[(m mod Np) N + n])): lam points to an F32 [Np,N] table here
};

// DN_EPI_EMBED's scatter: row b Np + p of the product is stored as row b T + prefix + p.  DN_EPI_SKIP_GELU reads Np alone
// (the rows of its table); no other epilogue reads any of it.
struct DnEmbedRows {
    int64_t Np;
    int T, prefix;
};

int dn_linear(const dn_half* x, const dn_half* w, const dn_half* bias, const dn_half* lam, void* out, int64_t M, int K, int N,
              int epi, hipStream_t s, DnEmbedRows embed = {1, 0, 0});
// HV_LINEAR (sam2.hip): the same product for any K that is a multiple of 8; K a multiple of 64 runs DN_LINEAR's own kernels
int dn_linear_k8(const dn_half* x, const dn_half* w, const dn_half* bias, const dn_half* lam, void* out, int64_t M, int K, int N,
                 int epi, hipStream_t s);
int dn_norm(const float* x, int64_t rows, int hidden, int64_t in_stride, const dn_half* g, const dn_half* b, float eps, void* y,
            int out_f32, hipStream_t s);
// the necks' element-wise passes (SV_NECK, HV_NECK): y = fp16(x) over n values; out [C,T] = in [T,C] transposed, plus add[c] where
// add is given (one fp32 addition)
int vit_cast(const float* x, int64_t n, dn_half* y, hipStream_t s);
int vit_transpose(const float* in, int64_t T, int Cn, const float* add, float* out, hipStream_t s);

// ---------------------------------------------------------------- device helpers
// row of a 32x32 accumulator held in register `reg` of a lane of half `h` (the column is lane & 31)
__device__ __forceinline__ int vit_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// the erf GELU, every operation one fp32 rounding
__device__ __forceinline__ float vit_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// The patch gather of DN_EMBED and SV_EMBED: patches[row][c 256 + ky 16 + kx] is pixel (16 py + ky, 16 px + kx) of channel c.
// Thread i writes the 8 kx of half a patch row: k = 8 part .. 8 part + 7 of row `row`.  The kernel finds the pixels and
// converts them.
#define VIT_PATCH 16
#define VIT_PATCH_K (3 * VIT_PATCH * VIT_PATCH)

struct VitPatchPart {
    int64_t row;
    int part, c, ky, kx0;
};

// false for the threads past the last of `rows` patch rows
__device__ __forceinline__ bool vit_patch_part(int64_t rows, VitPatchPart& a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * (VIT_PATCH_K / 8)) return false;
    a.row = i / (VIT_PATCH_K / 8);
    a.part = (int)(i - a.row * (VIT_PATCH_K / 8));
    a.c = a.part >> 5;
    a.ky = (a.part >> 1) & 15;
    a.kx0 = (a.part & 1) * 8;
    return true;
}

__device__ __forceinline__ void vit_patch_store(dn_half* __restrict__ patches, const VitPatchPart& a, vit_h8 v) {
    *reinterpret_cast<vit_h8*>(patches + a.row * VIT_PATCH_K + a.part * 8) = v;
}

static inline unsigned vit_patch_blocks(int64_t rows) { return (unsigned)((rows * (VIT_PATCH_K / 8) + 255) / 256); }

// ---------------------------------------------------------------- argument checks of the entry points (host)
// false, with the error set, when the workspace is missing or holds fewer than `need` bytes; `who` names it ("sam neck")
static inline bool vit_check_ws(const char* who, const void* ws, size_t have, size_t need) {
    if (ws && have >= need) return true;
    gsr_set_error("ws_bytes: %s workspace too small (%zu < %zu bytes)", who, have, need);
    return false;
}

// false, with the error set, at the first null among entries first .. n - 1 of a weight table
static inline bool vit_check_table(const char* who, const void* const* table, int n, int first = 0) {
    for (int i = first; i < n; ++i)
        if (!table[i]) {
            gsr_set_error("%s: weight %d of the table is null", who, i);
            return false;
        }
    return true;
}
