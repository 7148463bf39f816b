// The per-pixel half of K7, shared by render_bwd.hip (RGB payload, general and NOSURF kernel) and render_bwd_wide.hip
// (wide payloads): where a lane's pixel lies, what the forward saved for it, which gradients arrive for it, and the exact
// derivative of one compositing step.  The kernels keep what really differs between them: how list entries are staged,
// how the payload's term of q is formed, what becomes of the blending weight, and the row store.
//
// These are statement macros over the kernel's own locals, like GSR_GATHER5, not inline functions, and that is on purpose:
// the gradients have to stay bit-identical from build to build of the same arithmetic, the file is compiled with
// -ffp-contract=fast, and which product of a sum the backend fuses into an fma follows the order of the instructions it
// is handed.  The same arithmetic behind __forceinline__ functions (results through a struct) kept every register count
// and the whole instruction histogram and still changed low bits of the gradients on the card; the same tokens in the
// same place cannot.  Each macro names what it reads (<-) and what it declares or updates (->).
#pragma once
#include "pair_eval.h"
#include "render_bwd_shared.h"

// XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so workgroup b
// takes tile (b % 8) * per_xcd + b / 8 -- every XCD owns one contiguous band of tiles, and the records shared by
// neighbouring tiles are fetched into ONE L2 instead of several
#define RB_TILE_OF_WORKGROUP() ((int)(blockIdx.x & 7u) * p.per_xcd + (int)(blockIdx.x >> 3))

// <- tile_lin, wave.  -> qx0, qy0: the wave's 8x8 quad of the tile
#define RB_QUAD_ORIGIN()                                                                                       \
    const int tile_y = tile_lin / p.gx, tile_x = tile_lin - tile_y * p.gx;                                      \
    const int qx0 = tile_x * GSR_TILE + (wave & 1) * 8, qy0 = tile_y * GSR_TILE + (wave >> 1) * 8

// <- qx0, qy0, grp (DPP row = 4x4 pixel block of the quad), l16 (pixel of the block; same mapping as render_fwd).
// -> pxi, pyi, inside, pxf, pyf, pix_id, HW
#define RB_PIXEL()                                                                                             \
    const int pxi = qx0 + (grp & 1) * 4 + (l16 & 3), pyi = qy0 + (grp >> 1) * 4 + (l16 >> 2);                  \
    const bool inside = pxi < p.W && pyi < p.H;                                                                 \
    const float pxf = (float)pxi, pyf = (float)pyi;                                                             \
    const int pix_id = pyi * p.W + pxi;                                                                         \
    const int HW = p.W * p.H

// -> last_contributor, and max_contrib: the deepest list entry any pixel of THIS QUAD reached (wave-uniform)
#define RB_QUAD_DEPTH()                                                                                        \
    const int last_contributor = inside ? (int)p.n_contrib[pix_id] : 0;                                         \
    int max_contrib = last_contributor;                                                                         \
    _Pragma("unroll")                                                                                           \
    for (int d = 32; d > 0; d >>= 1) max_contrib = max(max_contrib, __shfl_xor(max_contrib, d, 64));            \
    max_contrib = __builtin_amdgcn_readfirstlane(max_contrib)

// Per-pixel state saved by the forward (final_D = sum m w, final_D2 = sum m^2 w; NOSURF: the three that only the surface
// channels read are not loaded), the two quirk flags, and `lit`:
// a pixel nothing was blended into takes no part in the reference's backward (its loop over contributors is empty), so
// whatever gradient arrives for it must not be read: the replay is branch-free -- an idle lane contributes
// 0 * (its pixel's gradient) to the 16-lane sums -- and the reference's OWN objective sends NaN to exactly these pixels
// (gaussian_renderer/__init__.py:131-132: depth / alpha with alpha = 0, nan_to_num on the value only).
// <- NOSURF.  -> clamp_pass, filter_depth_quirk, T_final, final_D, final_D2, final_A, median_contributor, lit
#define RB_PIXEL_STATE()                                                                                       \
    const bool clamp_pass = (p.flags & GSR_FLAG_CLAMP_PASSTHROUGH) != 0;                                        \
    const bool filter_depth_quirk = (p.flags & GSR_FLAG_FILTER_DEPTH_GRAD) != 0;                                \
    const float T_final = inside ? p.final_T[pix_id] : 0.f;                                                     \
    const float final_D = (!NOSURF && inside) ? p.final_T[pix_id + HW] : 0.f;                                   \
    const float final_D2 = (!NOSURF && inside) ? p.final_T[pix_id + 2 * HW] : 0.f;                              \
    const float final_A = 1.0f - T_final;                                                                       \
    const int median_contributor = (!NOSURF && inside) ? (int)p.n_contrib[pix_id + HW] : 0;                     \
    const bool lit = inside && last_contributor > 0

// dL/dallmap of the pixel (NOSURF: identically zero by the caller's promise, nothing is loaded).
// -> dL_ddepth, dL_daccum, dL_dn0..2, dL_dmedian, dL_dreg
#define RB_ALLMAP_GRADS()                                                                                      \
    float dL_ddepth = 0.f, dL_daccum = 0.f, dL_dreg = 0.f, dL_dmedian = 0.f;                                    \
    float dL_dn0 = 0.f, dL_dn1 = 0.f, dL_dn2 = 0.f;                                                             \
    if (!NOSURF && lit) {                                                                                       \
        dL_ddepth = p.dL_dallmap[pix_id + 0 * HW];                                                              \
        dL_daccum = p.dL_dallmap[pix_id + 1 * HW];                                                              \
        dL_dn0 = p.dL_dallmap[pix_id + 2 * HW];                                                                 \
        dL_dn1 = p.dL_dallmap[pix_id + 3 * HW];                                                                 \
        dL_dn2 = p.dL_dallmap[pix_id + 4 * HW];                                                                 \
        dL_dmedian = p.dL_dallmap[pix_id + 5 * HW];                                                             \
        dL_dreg = p.dL_dallmap[pix_id + 6 * HW];                                                                \
    }

// Which channels of dL/dallmap reach this quad at all (wave-uniform).  dm_live = false: the forward returned channels 5
// and 6 as constants (GSR_FLAG_NO_DIST_MEDIAN), gradients sent to them are ignored.
// <- dm_live.  -> quad_has_dist, quad_has_median, quad_has_surf
#define RB_QUAD_FLAGS()                                                                                        \
    const bool quad_has_dist = dm_live && __any(dL_dreg != 0.f), quad_has_median = dm_live && __any(dL_dmedian != 0.f); \
    const bool quad_has_surf = !NOSURF && __any(dL_ddepth != 0.f || dL_daccum != 0.f || dL_dn0 != 0.f || dL_dn1 != 0.f || dL_dn2 != 0.f)

// -> the running state of the back-to-front recursion
#define RB_STATE_BEGIN()                                                                                       \
    float T = T_final;                                                                                          \
    float last_alpha = 0.f, last_q = 0.f, acc_q = 0.f, last_dL_dT = 0.f

// One compositing step undone.  Branch-free: EVERY lane runs the gradient math (masked-off lanes would cost the same
// issue slots), and a lane that does not blend this splat gets alpha = G = 0 and harmless finite geometry, which makes
// all of its partial derivatives exact zeros and leaves its recursion state untouched (T / (1 - 0) = T; the suffix sums
// advance by a zero-weight term).
// <- pr (GsrPair), active.  -> alpha, G, c_d, sx, sy, inv_pz, one_m_alpha, inv_oma, w;  T advanced
#define RB_BLEND()                                                                                             \
    const float alpha = active ? pr.alpha : 0.f, G = active ? pr.G : 0.f, c_d = active ? pr.depth : 1.f;        \
    const float sx = active ? pr.sx : 0.f, sy = active ? pr.sy : 0.f, inv_pz = active ? pr.inv_pz : 0.f;        \
    const float one_m_alpha = 1.0f - alpha;                                                                     \
    const float inv_oma = gsr_rcp(one_m_alpha);                                                                 \
    T = T * inv_oma;                                                                                            \
    const float w = alpha * T

// Colour, expected depth, alpha and normal share one suffix recursion,
//   q_i = c_i . dL/dC + z_i dL/dD + 1 dL/dA + n_i . dL/dN,
// and the kernel forms q: the order of its terms differs between the kernels and is part of their results.
// <- q.  -> dL_dalpha (so far);  acc_q, last_q advanced
#define RB_SUFFIX()                                                                                            \
    acc_q = last_alpha * last_q + (1.f - last_alpha) * acc_q;                                                   \
    last_q = q;                                                                                                 \
    float dL_dalpha = q - acc_q

// The pair's partial derivatives but the payload's (row layout GSR_GR_*).
// The surface channels -- depth, alpha, normal -- carry no gradient before the regularizers switch on.  Median depth and
// distortion are skipped (wave-uniformly) when the whole quad receives no gradient on that channel -- the reference's
// defaults (depth_ratio = 0, lambda_dist = 0) make both identically zero, and every term is a multiple of it.  alpha also
// scales how much background shows through; alpha = min(0.99, opa * G) (clamp quirk).  dL/dTu = -dL/dk = dL/dp x l,
// dL/dTv = -dL/dl = k x dL/dp.  tiny_any (pair_eval.h: a denormal p.z): the empty asm keeps this a BRANCH -- if-converted
// it cost three vector instructions on every pair, +3.7 % of K7's issue.  NOSURF gT[6..8]: the general form with
// dL_dz = +0: 0 * s - a - b == -a - b up to the sign of a zero.
// <- opa (the record's opacity), a1 (Tw.xy in .zw), cidx, and all of the above.
// -> gT[0..8], gxy0, gxy1, gn0..2, gopa (declared by the kernel);  last_alpha, last_dL_dT advanced
#define RB_PARTIALS()                                                                                          \
    gn0 = 0.f; gn1 = 0.f; gn2 = 0.f;                                                                            \
    if (quad_has_surf) { gn0 = w * dL_dn0; gn1 = w * dL_dn1; gn2 = w * dL_dn2; }                                \
                                                                                                                \
    float dL_dz = NOSURF ? 0.f : w * dL_ddepth;                                                                 \
    if (quad_has_median && active && cidx == median_contributor - 1) dL_dz += dL_dmedian;                       \
    if (quad_has_dist) {                                                                                        \
        float dmd_dd;                                                                                           \
        const float m_d = gsr_depth_map(c_d, dmd_dd);                                                           \
        const float dL_dweight = (final_D2 + m_d * m_d * final_A - 2.f * m_d * final_D) * dL_dreg;              \
        dL_dalpha += dL_dweight - last_dL_dT;                                                                   \
        last_dL_dT = dL_dweight * alpha + one_m_alpha * last_dL_dT;                                             \
        dL_dz += 2.0f * w * (m_d * final_A - final_D) * dL_dreg * dmd_dd;                                       \
    }                                                                                                           \
                                                                                                                \
    dL_dalpha *= T;                                                                                             \
    last_alpha = alpha;                                                                                         \
    dL_dalpha -= T_final * inv_oma * bg_dot_dpixel;                                                             \
                                                                                                                \
    const float dL_daraw = (clamp_pass || pr.araw <= GSR_ALPHA_MAX) ? dL_dalpha : 0.f;                          \
    const float dL_dG = opa * dL_daraw;                                                                         \
    gopa = G * dL_daraw;                                                                                        \
                                                                                                                \
    const float Twx = a1.z, Twy = a1.w;                                                                         \
    if (pr.use3d) {                                                                                             \
        const float dL_dsx = NOSURF ? dL_dG * (-G * sx) : dL_dG * (-G * sx) + dL_dz * Twx;                      \
        const float dL_dsy = NOSURF ? dL_dG * (-G * sy) : dL_dG * (-G * sy) + dL_dz * Twy;                      \
        float dpx = dL_dsx * inv_pz, dpy = dL_dsy * inv_pz;                                                     \
        if (__builtin_expect(pr.tiny_any, 0)) {                                                                 \
            asm volatile("");                                                                                   \
            const float zs = pr.tiny ? GSR_TINY_PZ_SCALE : 1.f; dpx *= zs; dpy *= zs;                           \
        }                                                                                                       \
        const float dpz = -(dpx * sx + dpy * sy);                                                               \
        const float ux = dpy * pr.lz - dpz * pr.ly, uy = dpz * pr.lx - dpx * pr.lz, uz = dpx * pr.ly - dpy * pr.lx; \
        const float vx = pr.ky * dpz - pr.kz * dpy, vy = pr.kz * dpx - pr.kx * dpz, vz = pr.kx * dpy - pr.ky * dpx; \
        gT[0] = ux; gT[1] = uy; gT[2] = uz;                                                                     \
        gT[3] = vx; gT[4] = vy; gT[5] = vz;                                                                     \
        if (NOSURF) {                                                                                           \
            gT[6] = 0.f - pxf * ux - pyf * vx;                                                                  \
            gT[7] = 0.f - pxf * uy - pyf * vy;                                                                  \
            gT[8] = 0.f - pxf * uz - pyf * vz;                                                                  \
        } else {                                                                                                \
            gT[6] = dL_dz * sx - pxf * ux - pyf * vx;                                                           \
            gT[7] = dL_dz * sy - pxf * uy - pyf * vy;                                                           \
            gT[8] = dL_dz - pxf * uz - pyf * vz;                                                                \
        }                                                                                                       \
        gxy0 = 0.f; gxy1 = 0.f;                                                                                 \
    } else {                                                                                                    \
        gxy0 = dL_dG * (-G * GSR_FILTER_INV_SQUARE * pr.dx);                                                    \
        gxy1 = dL_dG * (-G * GSR_FILTER_INV_SQUARE * pr.dy);                                                    \
        gT[0] = 0.f; gT[1] = 0.f; gT[2] = 0.f; gT[3] = 0.f; gT[4] = 0.f; gT[5] = 0.f;                           \
        gT[6] = (!NOSURF && filter_depth_quirk) ? sx * dL_dz : 0.f;                                             \
        gT[7] = (!NOSURF && filter_depth_quirk) ? sy * dL_dz : 0.f;                                             \
        gT[8] = dL_dz;                                                                                          \
    }
