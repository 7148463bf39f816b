// The attention tile of DN_ATTN (dino.hip) and SV_ATTN (sam.hip): one pass, flash style, a wave owns 32 queries of one head.
// The first product is S^T = K Q^T (A = K, B = Q^T, Q's fragments stay in registers): the result has the query on the lane and
// the kv index in the registers, so the maximum and the sum of a query's row are per-lane loops plus one exchange between the
// lane halves, and P^T (rounded to fp16) is the B operand of O^T = V^T P^T as it lies: no lane movement, no LDS.  The k order
// of that second product is the accumulator's row order (vit_acc_row), which the V^T fragment follows.  The scores are kept in
// base 2, so p = 2^(t - m) is one v_exp_f32.  How K and V^T reach LDS, and how a raw score becomes a base-2 score, is the
// kernel's.
#pragma once
#include "vit_common.h"

#define VA_BQ 128       // queries of a workgroup: 4 waves of 32
#define VA_BKV 64       // kv rows of a tile
#define VA_LDV 68       // halves per row of the V^T image: 136 bytes (8-byte aligned reads), paired stores 2 to a bank

// HD = 80: five k-steps of 16, and the O^T tiles cover 96 rows of which rows 80..95 of V^T must be zeros and are never stored.
template <int HD>
struct VitAttnTile {
    static constexpr int KS = HD / 16, DT = (HD + 31) / 32;
    static constexpr int LDK = HD + 8;      // halves per row of the K image: 16-byte aligned, consecutive rows 4 banks apart
    vit_f32x16 acc[DT];
    float m_run, l_run;

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[dt][e] = 0.f;
        m_run = -INFINITY;
        l_run = 0.f;
    }

    // One tile of 64 kv rows: Ks [64][LDK] and Vt [32 DT][VA_LDV] in LDS, r = lane & 31, h = lane >> 5.  score(raw, jj) gives
    // the base-2 score of kv row jj of the tile, or -inf; at least one row of a tile must be finite.
    template <typename SCORE>
    __device__ __forceinline__ void step(const dn_half* Ks, const dn_half* Vt, const vit_h8 (&qf)[KS], int r, int h, SCORE score) {
        vit_f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kb][e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const vit_h8 a = *reinterpret_cast<const vit_h8*>(&Ks[(kb * 32 + r) * LDK + ks * 16 + 8 * h]);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[ks], s[kb], 0, 0, 0);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float sv = score(s[kb][e], kb * 32 + vit_acc_row(e, h));
                s[kb][e] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
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
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[dt][e] *= alpha;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                vit_h8 pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (dn_half)s[kb][8 * ss + e];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    // element j of half h is kv 16 ss + 8 (j >> 2) + 4 h + (j & 3) of the block: two runs of 4 consecutive kv
                    const dn_half* vp = &Vt[(dt * 32 + r) * VA_LDV + kb * 32 + ss * 16 + 4 * h];
                    const vit_h4 lo = *reinterpret_cast<const vit_h4*>(vp), hi = *reinterpret_cast<const vit_h4*>(vp + 8);
                    vit_h8 a;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = lo[e]; a[4 + e] = hi[e]; }
                    acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf, acc[dt], 0, 0, 0);
                }
            }
    }

    // the lane's query: orow[d] = fp16(acc / l_run) for the d < HD of lane half h
    __device__ __forceinline__ void store(dn_half* orow, int h) const {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d0 = dt * 32 + 8 * g + 4 * h;
                if (HD % 32 != 0 && d0 >= HD) continue;
                vit_h4 out;
#pragma unroll
                for (int e = 0; e < 4; ++e) out[e] = (dn_half)(acc[dt][4 * g + e] / l_run);
                *reinterpret_cast<vit_h4*>(orow + d0) = out;
            }
    }
};
