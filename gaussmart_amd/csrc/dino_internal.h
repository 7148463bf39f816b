// What sam.hip shares with dino.hip: the DN_LINEAR and DN_NORM launchers (defined in dino.hip, rules in include/gsr.h) and the
// epilogue values.  0..3 are DINO's and keep their bits; 4..6 were added for SAM's encoder (no LayerScale, fp32 stores).
#pragma once
#include "gsr_common.h"

typedef _Float16 dn_half;

enum {
    DN_EPI_BIAS = 0,    // fp16(acc + bias)
    DN_EPI_GELU = 1,    // fp16(gelu(acc + bias))
    DN_EPI_RESID = 2,   // resid = fma(lambda[n], acc + bias, resid), fp32
    DN_EPI_EMBED = 3,   // DINO's patch rows behind the prefix tokens, fp32
    DN_EPI_RESID1 = 4,  // resid = resid + (acc + bias), fp32
    DN_EPI_F32 = 5,     // acc + bias, fp32
    DN_EPI_POS = 6      // (acc + bias) + fp32(lam[m N + n]), fp32: lam is an fp16 [M,N] table here
};

int dn_linear(const dn_half* x, const dn_half* w, const dn_half* bias, const dn_half* lam, void* out, int64_t M, int K, int N,
              int epi, int64_t Np, int T, int prefix, hipStream_t s);
int dn_norm(const float* x, int64_t rows, int hidden, int64_t in_stride, const dn_half* g, const dn_half* b, float eps, void* y,
            int out_f32, hipStream_t s);
