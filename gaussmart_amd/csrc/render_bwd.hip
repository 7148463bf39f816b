// K7 render_bwd: back-to-front replay of every tile -- no floating-point atomics anywhere.
//
// Restates the [U]/[P] backward of the surfel compositing (colour, expected depth, alpha, normal,
// median depth, distortion), see DESIGN.md section "render_bwd" for the recursion; it is the exact
// derivative of render_fwd except for the two flagged quirks (GSR_FLAG_*).
//
// MI355X mapping: WAVE-INDEPENDENT, like the forward, and BLOCK-INDEPENDENT inside the wave.  Each wave64 of
// a tile's workgroup owns an 8x8 pixel quad and never synchronises with the other three; each DPP row of
// 16 lanes owns one 4x4 pixel block of that quad and walks ITS OWN list:
//   * the wave starts at the deepest list entry ANY OF ITS 64 PIXELS reached (quad-level, not tile-level)
//     and walks the (tile, depth)-ordered list backwards.  A SCAN FRONT reads only the touch words, 64 list
//     positions per chunk (coalesced, two chunks in flight), and appends the positions whose nibble for THIS quad
//     is non-zero to a small wave-private ring in LDS (ballot + mbcnt prefix, deep -> shallow).  A batch is the
//     next 64 RING entries, not 64 consecutive list entries: only entries the forward blended into this quad are
//     followed (inst_row -> slot_off), gathered and staged -- at 1M/1080p that is 0.30x the records and 0.33x the
//     batches of consecutive batching, and full batches cost 7 % fewer iterations (scripts/model_k7_batches.py).
//     Ids and emission indices run two batches ahead, row slots one batch ahead, the 80-byte records are gathered by
//     id at the start of their batch (lane l fetches ring entry l) and staged in the wave's private LDS slice;
//   * the forward left 4 bits per (instance, quad): "blended into >= 1 pixel of block g".  Four ballots
//     turn them into one 64-bit to-do mask PER BLOCK; every iteration each row takes the deepest entry
//     of its own mask, so the wave needs max_g |list_g| iterations instead of |union of the lists|
//     (measured at 1M/1080p: 0.67x the iterations; lane utilisation 30 % -> 45 %);
//   * the suffix recursions of colour, depth, alpha and normal are collapsed into ONE scalar
//     recursion (they are linear: q_i = c_i.dL/dC + z_i dL/dD + dL/dA + n_i.dL/dN);
//   * the 18 partial derivatives are summed over the 16 pixels of the block with the transposed butterfly
//     of wave_reduce.h (DPP only, ~50 VALU) and land one per lane, which store them straight into the
//     block's OWN 80-byte sub-row of that instance (16 sub-rows per instance) plus a 1-byte flag;
//   * reduce_rows adds the flagged sub-rows in fixed order => bitwise reproducible gradients, and
//     HBM sees plain streaming stores instead of ~18 atomics per pixel-splat pair.
#include <stdlib.h>
#include "gsr_common.h"
#include "wave_reduce.h"

#include "rb_replay.h"

#ifndef RB_MIN_WAVES
#define RB_MIN_WAVES 6   // <= 80 VGPRs.  Round 2's kernel needed 72 (seven waves per SIMD); with the two-array rows and the
                         // row_begin side job it takes the 80 (six waves).  A 72-register variant -- xy address derived from
                         // the row address, side job behind the tile's work -- runs seven waves again and is 1 % SLOWER
                         // (K7 0.669 vs 0.662 ms, profiles/r03_notes/ab_k7_seven_waves_again.log): behind the tile the job's
                         // two memory trips are a tail nothing overlaps, in front they hide behind the tile's own first loads
#endif
// (Wide per-pixel payloads have their own kernel: render_bwd_wide.hip.)
// PROBE (developer builds only: make PROBES=1, scripts/dev_probe.py): 1 = eight more dependent VALU per iteration,
// 4 = eight more dependent SALU, 6 = 20 KB more LDS per workgroup (fewer waves per SIMD), 8 = four LDS reads of the record
// instead of five (WRONG gradients).
#ifdef GSR_DEV_PROBES
// PROBE 7 (round 4): every wave leaves its lifetime on the shader clock (s_memtime) and on the 100 MHz s_memrealtime
// clock: their ratio is the clock the chip holds under this kernel (scripts/dev_clock_probe.py).
#define RB_STAMP_WAVES 65536
__device__ unsigned long long g_rb_stamps[2 * RB_STAMP_WAVES];
extern "C" int gsr_probe_read_stamps_bwd(void* dst, size_t bytes) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_rb_stamps), bytes < sizeof(g_rb_stamps) ? bytes : sizeof(g_rb_stamps)) == hipSuccess ? 0 : -1;
}
#endif
// NOSURF (round 4; GSR_FLAG_NO_SURFACE_GRAD): the caller promises that dL/dallmap is identically zero -- the reference's own
// evaluation flags (scripts/dtu_eval.py:45: --lambda_normal 0 --lambda_dist 0) and the first 7,000 iterations of EVERY run
// (train.py:132-133: lambda_normal from 7,000, lambda_dist from 3,000 and 0 by default).  Then no gradient reaches depth,
// alpha, normal, median depth or distortion: dL/dz = 0 and dL/dn = 0 identically, the per-pixel state loses five loads and
// ten registers, and the staged record needs neither the normal nor the cull rect: 16 floats instead of 20, FOUR per-lane
// ds_read_b128 per iteration instead of five (the fifth was worth 4 % of the kernel: DESIGN.md section 4, probe 8).  The
// entry's first gradient row and its touch nibble share the sixteenth word: row + popcount of the touch bits of the quads
// before this one (28 bits; the launcher falls back to the general kernel beyond 2^28 rows) | this quad's nibble << 28.
// The entry's list position (the general record carries it beside the nibble) has no room in those sixteen words: it sits in
// a 64-word array beside the records and costs one ds_read_b32 per iteration next to the four ds_read_b128.
// Same arithmetic in the same order for everything that is not multiplied by one of those zeros, so the gradients equal the
// general kernel's fed with a zero dL/dallmap bit for bit (tests/test_gpu_rasterizer.py).
template <int PROBE = 0, bool NOSURF = false>
__global__ void __launch_bounds__(RB_BLOCK, NOSURF ? 8 : RB_MIN_WAVES) render_bwd_kernel(RenderBwdParams p) {
#ifdef GSR_DEV_PROBES
    unsigned long long stamp_t0 = 0, stamp_c0 = 0;
    if (PROBE == 7) { stamp_t0 = __builtin_amdgcn_s_memrealtime(); stamp_c0 = __builtin_amdgcn_s_memtime(); }
#endif
    __shared__ float s_probe_pad[PROBE == 6 ? 5120 : 1];
    if (PROBE == 6 && p.W < 0) s_probe_pad[threadIdx.x] = 1.f;
    constexpr int RS = NOSURF ? 4 : 5;          // float4 parts of a staged record
    __shared__ float4 s_rec_all[RB_WAVES][64 * RS];
    // the scan front's ring: list position | this quad's touch nibble << 28, and the number of gradient rows the entry has
    // in the quads before this one (0..12)
    __shared__ uint32_t s_ring_all[RB_WAVES][RB_RING];
    __shared__ uint8_t s_rcnt_all[RB_WAVES][RB_RING];
    __shared__ uint32_t s_pos_all[NOSURF ? RB_WAVES : 1][NOSURF ? 64 : 1];   // NOSURF: list position of staged entry j

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    float4* s_rec = s_rec_all[wave];
    uint32_t* s_ring = s_ring_all[wave];
    uint8_t* s_rcnt = s_rcnt_all[wave];
    uint32_t* s_pos = s_pos_all[NOSURF ? wave : 0];
    // (the prologue and the per-pair backward are rb_replay.h's statement macros over these locals)
    const int tile_lin = RB_TILE_OF_WORKGROUP();
    rb_row_begin_job(p);
    if (tile_lin >= p.n_tiles) return;
    RB_QUAD_ORIGIN();
    const int grp = lane >> 4, l16 = lane & 15;   // DPP row = 4x4 pixel block
    const uint32_t below_mask = ((1u << grp) - 1u) << 28;   // nibble bits (bits 28..31 of a staged word) of the blocks before mine in this quad
    const uint32_t quads_below_mask = ((1u << (8 * wave)) - 1u) & 0x0F0F0F0Fu;   // ... of the quads before mine
    const uint32_t pick_shift = (uint32_t)grp * 16u;   // where this row's pick sits in the packed 64-bit scalar
    RB_PIXEL();

    const uint32_t tile = (uint32_t)tile_lin;
    const uint32_t r0 = p.ranges[2 * tile];
    // the forward wrote quad w's touch byte of a list entry only below covered[w] (wave-uniform)
    const uint4 cov4 = *reinterpret_cast<const uint4*>(p.covered + 4 * tile);

    RB_QUAD_DEPTH();
    if (max_contrib == 0) return;

    RB_PIXEL_STATE();
    float dL_dpix0 = 0.f, dL_dpix1 = 0.f, dL_dpix2 = 0.f;
    if (lit) { dL_dpix0 = p.dL_dcolor[pix_id]; dL_dpix1 = p.dL_dcolor[pix_id + HW]; dL_dpix2 = p.dL_dcolor[pix_id + 2 * HW]; }
    RB_ALLMAP_GRADS();
    const float bg_dot_dpixel = p.bg[0] * dL_dpix0 + p.bg[1] * dL_dpix1 + p.bg[2] * dL_dpix2;

    const bool dm_live = !NOSURF && (p.flags & (uint32_t)GSR_FLAG_NO_DIST_MEDIAN) == 0;
    RB_QUAD_FLAGS();

    RB_STATE_BEGIN();

    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pf0, pf1, pf2, pf3, pf4;
    uint32_t pf_slot = 0;    // named (not an array): keeps the prefetch in VGPRs, not scratch.  slot_off[emission index] of the
                             // prefetched entry: a dependent load, so the emission indices run two batches ahead

    // ---- scan front.  List positions [0, sc) are still to scan.  The ring holds, from r_base on: the `nb` entries of the
    // current batch (until they are staged), the `nb_nxt` entries of the next one, and up to 64 entries that wait for the
    // batch after that, up to r_tail -- never more than 128 (all of this is wave-uniform).  tw0 / tw1 hold the raw touch
    // words of the next two chunks, lane l <-> position top - 1 - l, so the ring order is the list order backwards.  A fill
    // stops at exactly 64 waiting entries: a chunk that holds more keeps the rest for the next fill (the lanes already
    // taken are zeroed), so every batch but a list's last is full.
    int sc = max_contrib;
    uint32_t r_base = 0, r_tail = 0;
    auto load_chunk = [&](int top) -> uint32_t {
        const int pos = top - 1 - lane;
        return pos >= 0 ? p.touch[(size_t)r0 + (uint32_t)pos] : 0u;
    };
    uint32_t tw0 = load_chunk(sc), tw1 = load_chunk(sc - 64);
    auto scan_fill = [&](uint32_t held) {      // held: ring entries from r_base on that already belong to a batch
        while (sc > 0) {
            const uint32_t need = 64u - (r_tail - r_base - held);
            if (need == 0u) break;
            const int pos = sc - 1 - lane;
            const uint32_t t = pos >= 0 ? rb_defined_touch(tw0, (uint32_t)pos, cov4) : 0u;
            const uint32_t nib = (t >> (8 * wave)) & 0xFu;
            const unsigned long long b = __ballot(nib != 0);
            const uint32_t rank = rb_mbcnt(b), n_set = (uint32_t)__popcll(b);
            const bool take = nib != 0 && rank < need;
            if (take) {
                const uint32_t at = (r_tail + rank) & (uint32_t)(RB_RING - 1);
                s_ring[at] = (uint32_t)pos | (nib << 28);
                s_rcnt[at] = (uint8_t)__popc(t & quads_below_mask);
            }
            if (n_set <= need) {
                r_tail += n_set;
                sc = max(sc - 64, 0);
                tw0 = tw1; tw1 = load_chunk(sc - 64);
            } else {
                r_tail += need;
                if (take) tw0 = 0u;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto ring_pos = [&](uint32_t first) -> uint32_t {      // list position of ring entry first + lane
        return s_ring[(first + (uint32_t)lane) & (uint32_t)(RB_RING - 1)] & 0x0FFFFFFFu;
    };
    // emission indices run two batches ahead of the replay, ids and row slots one batch ahead
    uint32_t ids_cur = 0u, rows_nxt = 0u;
    int nb, nb_nxt;      // entries of the current and of the next batch
    {
        scan_fill(0u);
        nb = (int)min(64u, r_tail - r_base);
        if (lane < nb) {
            const uint32_t pos = ring_pos(r_base);
            ids_cur = p.point_list[r0 + pos];
            pf_slot = p.slot_off[p.inst_row[r0 + pos]];
        }
        __builtin_amdgcn_wave_barrier();   // the ring reads precede the fill's writes
        scan_fill((uint32_t)nb);
        nb_nxt = (int)min(64u, r_tail - r_base - (uint32_t)nb);
        if (lane < nb_nxt) rows_nxt = p.inst_row[r0 + ring_pos(r_base + (uint32_t)nb)];
    }

    while (nb > 0) {
        // The records of THIS batch are gathered here, not a batch ahead: holding the next batch's 20 registers per lane
        // through the replay cost two waves per SIMD (92 VGPRs, 5 waves -> 72, 7 waves), and seven waves hide the gather's
        // latency better than the prefetch did (K7 0.660 -> 0.640 ms same-box).  The ids, the row
        // slots, the emission indices and the scan front's two chunks -- five registers -- still run ahead; the ring words
        // wait in LDS.
        GSR_GATHER5(ids_cur, nb);
        uint32_t pk_of_lane = 0u;      // list position | this quad's nibble (one bit per 4x4 block: blended there?) << 28
        // first gradient row of staged entry `lane` IN THIS QUAD (its rows are dense, in (quad, block) order of the set bits)
        uint32_t slot_of_lane = 0u;
        if (lane < nb) {
            const uint32_t at = (r_base + (uint32_t)lane) & (uint32_t)(RB_RING - 1);
            pk_of_lane = s_ring[at];
            slot_of_lane = pf_slot + s_rcnt[at];
        }
        // the record's two cull-rect words mean nothing to the backward: the staged copy carries the entry's first row
        // and its position | nibble word there instead, so a block that picks entry j reads them with the record (they used
        // to come through two ds_bpermute per iteration)
        if (NOSURF) {   // [Tu Tv.x | Tv.yz Tw.xy | Tw.z xy opacity | rgb (first row in this quad | this quad's nibble << 28)]
            const uint32_t packed = slot_of_lane | (pk_of_lane & 0xF0000000u);
            s_rec[lane * RS] = pf0; s_rec[lane * RS + 1] = pf1;
            s_rec[lane * RS + 2] = make_float4(pf2.x, pf2.y, pf2.z, pf3.z);
            s_rec[lane * RS + 3] = make_float4(pf3.w, pf4.x, pf4.y, __uint_as_float(packed));
            s_pos[lane] = pk_of_lane & 0x0FFFFFFFu;
        } else {
            s_rec[lane * 5] = pf0; s_rec[lane * 5 + 1] = pf1; s_rec[lane * 5 + 2] = pf2; s_rec[lane * 5 + 3] = pf3;
            s_rec[lane * 5 + 4] = make_float4(pf4.x, pf4.y, __uint_as_float(slot_of_lane), __uint_as_float(pk_of_lane));
        }
        int nb_nn;
        {   // prefetch: ids and row slots of the next (shallower) batch; this batch leaves the ring; refill; emission
            // indices of the batch after the next
            pf_slot = 0u; ids_cur = 0u;
            if (lane < nb_nxt) {
                ids_cur = p.point_list[r0 + ring_pos(r_base + (uint32_t)nb)];
                pf_slot = p.slot_off[rows_nxt];
            }
            r_base += (uint32_t)nb;
            __builtin_amdgcn_wave_barrier();   // the ring reads precede the fill's writes
            scan_fill((uint32_t)nb_nxt);
            nb_nn = (int)min(64u, r_tail - r_base - (uint32_t)nb_nxt);
            rows_nxt = 0u;
            if (lane < nb_nn) rows_nxt = p.inst_row[r0 + ring_pos(r_base + (uint32_t)nb_nxt)];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // only the splats the forward blended into >= 1 pixel of a block carry any gradient there: one to-do
        // mask per 4x4 block (= DPP row), held by all 16 lanes of the row
        // (the four masks live in SGPRs: picking and clearing bits is scalar work, the vector unit only selects)
        // (the ring is ordered deep -> shallow, so staged entry 0 is the batch's deepest: the deepest entry of a block is the
        // lowest set bit of its mask, which s_ff1 finds and reports as -1 on an empty mask by itself -- two scalar
        // instructions per block and iteration)
        unsigned long long m0, m1, m2, m3;
        {
            const uint32_t t = lane < nb ? pk_of_lane >> 28 : 0u;
            m0 = __ballot((t & 1u) != 0); m1 = __ballot((t & 2u) != 0);
            m2 = __ballot((t & 4u) != 0); m3 = __ballot((t & 8u) != 0);
        }
        float probe_v = pxf; uint32_t probe_s = (uint32_t)__builtin_amdgcn_readfirstlane(nb);
        for (;;) {
            // deepest entry of each block's mask first; the four picks reach the lanes packed in one 64-bit scalar
            const int r0_ = rb_take_first(m0), r1_ = rb_take_first(m1), r2_ = rb_take_first(m2), r3_ = rb_take_first(m3);
            const uint32_t p01 = rb_pack16(r0_, r1_), p23 = rb_pack16(r2_, r3_);
            if ((p01 & p23) == 0xFFFFFFFFu) break;                  // all four masks were empty
            const unsigned long long picks = ((unsigned long long)p23 << 32) | p01;
            const int pick = (int)(short)(picks >> pick_shift);     // this row's pick; -1: none
            const bool has = pick >= 0;
            const int j = max(pick, 0);                             // (a row without a pick reads entry 0 and drops the result)
            const float4 a0 = s_rec[j * RS + 0], a1 = PROBE == 8 ? a0 : s_rec[j * RS + 1], a2 = s_rec[j * RS + 2];
            const float4 a3 = s_rec[j * RS + 3];     // general: [n.y n.z opacity r]; NOSURF: [r g b packed row | nibble]
            const float opa = NOSURF ? a2.w : a3.z;
            if (PROBE == 1) {
#pragma unroll
                for (int q = 0; q < 8; ++q) asm volatile("v_fma_f32 %0, %0, %0, %0" : "+v"(probe_v));
            }
            if (PROBE == 4) {
#pragma unroll
                for (int q = 0; q < 8; ++q) asm volatile("s_add_u32 %0, %0, 1" : "+s"(probe_s) : : "scc");
            }
            // first gradient row in this quad, this quad's touch nibble and the 0-based position in the tile list of this
            // row's entry (staged with the record)
            uint32_t rec_slot, rec_touch;      // (rec_touch: the nibble sits in bits 28..31, the rest is not looked at)
            int cidx;
            float4 a4;
            if (NOSURF) {
                rec_touch = __float_as_uint(a3.w);
                rec_slot = rec_touch & 0x0FFFFFFFu;
                cidx = (int)s_pos[j];
                a4 = make_float4(a3.y, a3.z, 0.f, 0.f);
            } else {
                a4 = s_rec[j * 5 + 4];
                rec_touch = __float_as_uint(a4.w);
                rec_slot = __float_as_uint(a4.z);
                cidx = (int)(rec_touch & 0x0FFFFFFFu);
            }
            GsrPair pr;
            const bool ok = gsr_pair_eval(pxf, pyf, a0, a1, a2, opa, pr);
            const bool active = has && cidx < last_contributor && ok;
            float gT[9];
            float gxy0, gxy1, gn0, gn1, gn2, gopa, gc0, gc1, gc2;
            {
                RB_BLEND();
                // q of the suffix recursion: surface + colour, from 0
                const float c0 = NOSURF ? a3.x : a3.w, c1 = a4.x, c2 = a4.y;
                const float n0 = a2.w, n1 = a3.x, n2 = a3.y;    // (only read when quad_has_surf)
                float q = 0.f;
                if (quad_has_surf) q = c_d * dL_ddepth + dL_daccum + n0 * dL_dn0 + n1 * dL_dn1 + n2 * dL_dn2;
                q += c0 * dL_dpix0 + c1 * dL_dpix1 + c2 * dL_dpix2;
                RB_SUFFIX();
                gc0 = w * dL_dpix0; gc1 = w * dL_dpix1; gc2 = w * dL_dpix2;
                RB_PARTIALS();
            }

            // block-level sums (16 lanes), stored by the lanes that end up holding them (row layout GSR_GR_*)
            {
                const float v16[16] = {gT[0], gT[1], gT[2], gT[3], gT[4], gT[5], gT[6], gT[7], gT[8],
                                       gn0, gn1, gn2, gopa, gc0, gc1, gc2};
                const float tot = row_sum16_transposed(v16, l16);
                const float xy = row_sum2(gxy0, gxy1, l16);
                // every row whose to-do bit was set writes its slot (zeros if no pixel turned out active), so
                // the reduction never reads a row that was not written
                // (rec_slot already counts the quads before this one and rec_touch holds this quad's nibble only)
                const size_t slot = (size_t)rec_slot + __popc(rec_touch & below_mask);
                if (has) {
                    p.grad_rows[slot * RB_ROW + l16] = tot;                   // one aligned 64-byte store per row
                    if ((l16 & 7) == 0) p.grad_xy[slot * GSR_GROW_XY + (l16 >> 3)] = xy;
                }
            }
        }
        if (PROBE == 1 && probe_v == 1.2345f) T += 1.f;
        if (PROBE == 4 && probe_s == 0x7fffffffu) T += 1.f;
        __builtin_amdgcn_wave_barrier();   // all reads of this batch precede the next batch's LDS writes
        nb = nb_nxt; nb_nxt = nb_nn;
    }
#ifdef GSR_DEV_PROBES
    if (PROBE == 7) {
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), t1 = __builtin_amdgcn_s_memrealtime();
        const uint32_t w = blockIdx.x * 4u + (uint32_t)wave;
        if (lane == 0 && w < RB_STAMP_WAVES) { g_rb_stamps[2 * w] = c1 - stamp_c0; g_rb_stamps[2 * w + 1] = t1 - stamp_t0; }
    }
#endif
}

// Wide payload: add a Gaussian's feature rows (same dense slots as the geometry rows) in fixed order.  One thread
// per (depth rank, 4-channel piece); writes dL_dcolors [N,C] by Gaussian id (zeros for Gaussians with no instance).
// As in reduce_rows, a Gaussian with more than RF_BIG rows is noted (by its piece-0 thread) and summed afterwards by the
// whole workgroup -- 256 / C4 row lanes per piece, partials combined through LDS in lane order -- instead of one thread
// walking tens of thousands of rows.
#define RF_BIG 192
__global__ void __launch_bounds__(256) reduce_feat_rows_kernel(long long n_threads, int C4,
                                                               const uint32_t* __restrict__ order,
                                                               const uint32_t* __restrict__ row_begin,
                                                               const float4* __restrict__ rows,
                                                               float4* __restrict__ out) {
    __shared__ uint32_t s_big[256];
    __shared__ int s_nbig;
    __shared__ float4 s_part[256];
    if (threadIdx.x == 0) s_nbig = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_threads) {
        const int r = (int)(t / C4), q = (int)(t - (long long)r * C4);
        // (row_begin[r] = slot_off[offs[r]] comes from the render_bwd launch; the destination is read here, beside the row
        // range, and four rows are in flight per thread: the kernel is bound by its chain of dependent loads, not by bytes)
        const uint32_t s0 = row_begin[r], s1 = row_begin[r + 1], dst = order[r];
        if (s1 - s0 > (uint32_t)RF_BIG) {
            if (q == 0) s_big[atomicAdd(&s_nbig, 1)] = (uint32_t)r;
        } else {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (uint32_t sl = s0; sl < s1; sl += 4) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (sl + u < s1) v[u] = rows[(size_t)(sl + u) * C4 + q];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
            }
            out[(size_t)dst * C4 + q] = acc;
        }
    }
    __syncthreads();
    const int nbig = s_nbig;                       // uniform over the workgroup
    const int L = 256 / C4;                        // row lanes per piece
    const int q = (int)threadIdx.x % C4, rl = (int)threadIdx.x / C4;
    for (int b = 0; b < nbig; ++b) {
        const uint32_t rb = s_big[b];
        const uint32_t s0 = row_begin[rb], s1 = row_begin[rb + 1];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rl < L)
            for (uint32_t sl = s0 + (uint32_t)rl; sl < s1; sl += (uint32_t)L) {
                const float4 v = rows[(size_t)sl * C4 + q];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        s_part[threadIdx.x] = acc;
        __syncthreads();
        if ((int)threadIdx.x < C4) {
            float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int l = 0; l < L; ++l) {
                const float4 v = s_part[l * C4 + threadIdx.x];
                tot.x += v.x; tot.y += v.y; tot.z += v.z; tot.w += v.w;
            }
            out[(size_t)order[rb] * C4 + threadIdx.x] = tot;
        }
        __syncthreads();
    }
}

int gsr_launch_reduce_feat_rows(int N, int C, const uint32_t* order, const uint32_t* row_begin,
                                const float* feat_rows, float* dL_dcolors, hipStream_t s) {
    if (N <= 0) return GSR_OK;
    GsrProfileScope prof(GSR_K_PREPROCESS_BWD, s);
    const int C4 = C / 4;
    const long long n_threads = (long long)N * C4;
    hipLaunchKernelGGL(reduce_feat_rows_kernel, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, s, n_threads, C4,
                       order, row_begin, reinterpret_cast<const float4*>(feat_rows),
                       reinterpret_cast<float4*>(dL_dcolors));
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}

int gsr_launch_render_bwd(const GsrView& v, const uint32_t* ranges, const uint32_t* covered, const uint32_t* inst_row,
                          const float* splat, const uint32_t* touch, const uint32_t* slot_off, const float* final_T,
                          const uint32_t* n_contrib, const float* dL_dcolor, const float* dL_dallmap, float* grad_rows,
                          float* grad_xy, int N, const uint32_t* offs, uint32_t* row_begin, const float* feat,
                          const uint32_t* point_list, float* feat_rows, size_t max_rows, hipStream_t s) {
    RenderBwdParams p;
    p.W = v.width; p.H = v.height; p.gx = (v.width + GSR_TILE - 1) / GSR_TILE;
    const int gy = (v.height + GSR_TILE - 1) / GSR_TILE;
    p.flags = v.flags;
    p.ranges = ranges; p.covered = covered; p.inst_row = inst_row; p.splat = reinterpret_cast<const float4*>(splat); p.touch = touch;
    p.slot_off = slot_off; p.bg = v.bg;
    p.final_T = final_T; p.n_contrib = n_contrib; p.dL_dcolor = dL_dcolor; p.dL_dallmap = dL_dallmap;
    p.grad_rows = grad_rows; p.grad_xy = grad_xy;
    p.N = N; p.offs = offs; p.row_begin = row_begin;
    p.feat = feat; p.point_list = point_list; p.feat_rows = feat_rows; p.C = v.channels;
    if (p.gx <= 0 || gy <= 0) return GSR_OK;
    GsrProfileScope prof(GSR_K_RENDER_BWD, s);
    p.n_tiles = p.gx * gy; p.per_xcd = (p.n_tiles + 7) / 8;
    const dim3 grid(8 * p.per_xcd), block(RB_BLOCK);
    // no gradient on any allmap channel (the caller's promise) and row indices that fit 28 bits: the 4-part-record kernel
    const bool nosurf = feat == nullptr && (v.flags & (uint32_t)GSR_FLAG_NO_SURFACE_GRAD) != 0 && max_rows < (size_t(1) << 28);
    if (nosurf) {
        hipLaunchKernelGGL((render_bwd_kernel<0, true>), grid, block, 0, s, p);
    } else if (feat == nullptr) {
#ifdef GSR_DEV_PROBES
        const char* e = getenv("GSR_K7_PROBE");   // re-read per launch
        switch (e ? atoi(e) : 0) {
            case 1: hipLaunchKernelGGL((render_bwd_kernel<1>), grid, block, 0, s, p); break;
            case 4: hipLaunchKernelGGL((render_bwd_kernel<4>), grid, block, 0, s, p); break;
            case 6: hipLaunchKernelGGL((render_bwd_kernel<6>), grid, block, 0, s, p); break;
            case 7: hipLaunchKernelGGL((render_bwd_kernel<7>), grid, block, 0, s, p); break;
            case 8: hipLaunchKernelGGL((render_bwd_kernel<8>), grid, block, 0, s, p); break;
            default: hipLaunchKernelGGL((render_bwd_kernel<>), grid, block, 0, s, p);
        }
#else
        hipLaunchKernelGGL((render_bwd_kernel<>), grid, block, 0, s, p);
#endif
    } else {
        const int rc = gsr_launch_render_bwd_wide(p, v.channels, grid, s);   // render_bwd_wide.hip
        if (rc != GSR_OK) return rc;
    }
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
