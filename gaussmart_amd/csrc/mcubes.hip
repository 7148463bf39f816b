// Marching cubes over the allocated blocks of a TSDF volume (include/gsr.h, "mesh export").  One workgroup per block,
// 256 threads, 16 voxels per thread (voxel entry threadIdx.x + 256 z).
//
//   mc_cube_kernel       per cube: valid (MC_SKIP_WEIGHT0) and the sign case           -> code u16 per voxel
//   mc_count_kernel      per voxel: which of its +x/+y/+z edges carry a vertex (a valid cube of the edge crosses it) and
//                        the cube's triangle count; per-block totals                      -> edge bits u8 per voxel
//   mc_scan_*            exclusive scans of the two per-block totals (scan_bodies.h); the host reads the two grand totals
//   mc_emit_verts_kernel vertices in (slot, thread, z) order; first vertex index per voxel -> vert_off u32 per voxel
//   mc_emit_tris_kernel  triangles in the same order, vertex indices read through the grid
#include "tsdf_common.h"
#include "mc_tables.h"

// recalled Open3D rule (include/gsr.h): a cube with a corner of weight 0 -- or in an unallocated block -- is skipped
#define MC_SKIP_WEIGHT0(w) (!((w) > 0.f))
#define MC_VALID 0x100
// the offsets are u32 scans: exact while the grand totals fit; mc_count_kernel also sums them in 64 bits, and the host (and the
// emit kernels) refuse a volume whose totals do not fit
#define MC_MAX_VERTS 0x7fffffffull   // int32 triangle indices
#define MC_MAX_TRIS_TOTAL 0xffffffffull

struct McWs {
    unsigned long long* totals;   // [0] vertices, [1] triangles, summed in 64 bits (read back by the host)
    uint16_t* code;     // [A * 4096]
    uint8_t* edges;     // [A * 4096]
    uint32_t* vert_off; // [A * 4096]
    uint32_t* counts;   // [2][A]
    uint32_t* scans;    // [2][A + 1]
    uint32_t* partial;  // [2][tiles]
    size_t bytes;
};

static McWs mc_ws_layout(void* base, int64_t A) {
    McWs w{};
    GsrWsCursor c(base);
    w.totals = c.take<unsigned long long>(64 * 4);
    w.code = c.take<uint16_t>(A * TSDF_BV * 2);
    w.edges = c.take<uint8_t>(A * TSDF_BV);
    w.vert_off = c.take<uint32_t>(A * TSDF_BV * 4);
    w.counts = c.take<uint32_t>(2 * A * 4);
    w.scans = c.take<uint32_t>(2 * (A + 1) * 4);
    w.partial = c.take<uint32_t>(2 * scan_tiles(A) * 4 + 4);
    w.bytes = c.off;
    return w;
}

struct McArgs {
    TsdfGrid g;
    const int* block_index;
    const int* slot_block;
    const float* pool;
    int64_t plane;   // pool_blocks * 4096
    McWs ws;
};

// grid voxel coordinates of entry l of a slot's block
__device__ __forceinline__ void mc_voxel(const McArgs& a, int slot, int l, int& vx, int& vy, int& vz) {
    int bx, by, bz;
    tsdf_block_coords(a.g, a.slot_block[slot], bx, by, bz);
    vx = bx * TSDF_B + (l & 15);
    vy = by * TSDF_B + ((l >> 4) & 15);
    vz = bz * TSDF_B + (l >> 8);
}

// pool index of grid voxel (vx, vy, vz), -1 if unallocated / outside
__device__ __forceinline__ int64_t mc_index(const McArgs& a, int vx, int vy, int vz) {
    int l = 0;
    const int s = tsdf_voxel_slot(a.g, a.block_index, vx, vy, vz, l);
    return s < 0 ? -1 : (int64_t)s * TSDF_BV + l;
}

__global__ void __launch_bounds__(TSDF_THREADS) mc_cube_kernel(McArgs a) {
    const int slot = blockIdx.x;
    for (int z = 0; z < TSDF_B; ++z) {
        const int l = threadIdx.x + TSDF_THREADS * z;
        int vx, vy, vz;
        mc_voxel(a, slot, l, vx, vy, vz);
        uint32_t cs = 0;
        bool valid = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int64_t i = mc_index(a, vx + (c & 1), vy + ((c >> 1) & 1), vz + (c >> 2));
            if (i < 0 || MC_SKIP_WEIGHT0(a.pool[a.plane + i])) { valid = false; break; }
            if (a.pool[i] < 0.f) cs |= 1u << c;
        }
        a.ws.code[(int64_t)slot * TSDF_BV + l] = valid ? (uint16_t)(MC_VALID | cs) : 0;
    }
}

// edge bits of a voxel: edge a carries a vertex when a valid cube containing it crosses it (the cube at origin v - o, o in
// {0,1}^3 with o_a = 0, holds the edge from its corner o to corner o + e_a)
__device__ __forceinline__ uint32_t mc_edge_bits(const McArgs& a, int vx, int vy, int vz) {
    uint32_t bits = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            if ((o >> ax) & 1) continue;
            const int64_t i = mc_index(a, vx - (o & 1), vy - ((o >> 1) & 1), vz - (o >> 2));
            if (i < 0) continue;
            const uint32_t code = a.ws.code[i];
            if (!(code & MC_VALID)) continue;
            if (((code >> o) ^ (code >> (o | (1 << ax)))) & 1) bits |= 1u << ax;
            break;   // every valid cube of the edge sees the same two signs
        }
    }
    return bits;
}

__global__ void __launch_bounds__(TSDF_THREADS) mc_count_kernel(McArgs a) {
    __shared__ uint32_t red[2][TSDF_THREADS / 64];
    const int slot = blockIdx.x;
    uint32_t nv = 0, nt = 0;
    for (int z = 0; z < TSDF_B; ++z) {
        const int l = threadIdx.x + TSDF_THREADS * z;
        const int64_t i = (int64_t)slot * TSDF_BV + l;
        int vx, vy, vz;
        mc_voxel(a, slot, l, vx, vy, vz);
        const uint32_t bits = mc_edge_bits(a, vx, vy, vz);
        a.ws.edges[i] = (uint8_t)bits;
        nv += __popc(bits);
        const uint32_t code = a.ws.code[i];
        if (code & MC_VALID) nt += mc_num_tris[code & 0xff];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        nv += __shfl_down(nv, d, 64);
        nt += __shfl_down(nt, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = nv;
        red[1][threadIdx.x >> 6] = nt;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t s = 0;
        for (int w = 0; w < TSDF_THREADS / 64; ++w) s += red[threadIdx.x][w];
        a.ws.counts[threadIdx.x * (int64_t)gridDim.x + slot] = s;
        atomicAdd(&a.ws.totals[threadIdx.x], (unsigned long long)s);   // integer sum: exact in any order
    }
}

__global__ void __launch_bounds__(SCAN_BLOCK) mc_scan_reduce_kernel(const uint32_t* __restrict__ counts,
                                                                    uint32_t* __restrict__ partial, int64_t n) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    scan_reduce_body<uint32_t>(counts + blockIdx.y * n, nullptr, partial + blockIdx.y * scan_tiles(n), n, blockIdx.x, wt);
}

__global__ void __launch_bounds__(SCAN_BLOCK) mc_scan_apply_kernel(const uint32_t* __restrict__ counts,
                                                                   const uint32_t* __restrict__ partial,
                                                                   uint32_t* __restrict__ scans, int64_t n) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    uint32_t* out = scans + blockIdx.y * (n + 1);
    scan_apply_body<uint32_t>(counts + blockIdx.y * n, nullptr, partial + blockIdx.y * scan_tiles(n), out, n, blockIdx.x, wt);
}

__device__ __forceinline__ bool mc_totals_fit(const McArgs& a) {
    return a.ws.totals[0] <= MC_MAX_VERTS && a.ws.totals[1] <= MC_MAX_TRIS_TOTAL;
}

__global__ void __launch_bounds__(TSDF_THREADS) mc_emit_verts_kernel(McArgs a, float* __restrict__ verts,
                                                                     float* __restrict__ colors) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    if (!mc_totals_fit(a)) return;   // the count call refused this volume: the u32 offsets may have wrapped
    const int slot = blockIdx.x;
    const int64_t base = (int64_t)slot * TSDF_BV;
    uint32_t mine = 0;
    for (int z = 0; z < TSDF_B; ++z) mine += __popc(a.ws.edges[base + threadIdx.x + TSDF_THREADS * z]);
    uint32_t total;
    uint32_t run = a.ws.scans[slot] + block_excl_scan(mine, total, wt);
    const float vs = a.g.vs;
    for (int z = 0; z < TSDF_B; ++z) {
        const int l = threadIdx.x + TSDF_THREADS * z;
        const int64_t i = base + l;
        a.ws.vert_off[i] = run;
        const uint32_t bits = a.ws.edges[i];
        if (!bits) continue;
        int vx, vy, vz;
        mc_voxel(a, slot, l, vx, vy, vz);
        const float f0 = fabsf(a.pool[i]);
        const float c0[3] = {a.pool[2 * a.plane + i], a.pool[3 * a.plane + i], a.pool[4 * a.plane + i]};
        const float p0[3] = {((float)(vx + a.g.lo[0] * TSDF_B) + 0.5f) * vs, ((float)(vy + a.g.lo[1] * TSDF_B) + 0.5f) * vs,
                             ((float)(vz + a.g.lo[2] * TSDF_B) + 0.5f) * vs};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!((bits >> ax) & 1)) continue;
            // the neighbour is allocated with weight > 0: a valid cube holds this edge
            const int64_t j = mc_index(a, vx + (ax == 0), vy + (ax == 1), vz + (ax == 2));
            const float f1 = fabsf(a.pool[j]);
            const float den = f0 + f1;
            float* pv = verts + 3 * (int64_t)run;
            float* pc = colors + 3 * (int64_t)run;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pv[k] = p0[k] + (k == ax ? f0 / den * vs : 0.f);
                pc[k] = (c0[k] * f1 + a.pool[(2 + k) * a.plane + j] * f0) / den / 255.f;
            }
            ++run;
        }
    }
}

__global__ void __launch_bounds__(TSDF_THREADS) mc_emit_tris_kernel(McArgs a, int32_t* __restrict__ tris) {
    __shared__ uint32_t wt[SCAN_BLOCK / 64];
    if (!mc_totals_fit(a)) return;
    const int slot = blockIdx.x;
    const int64_t base = (int64_t)slot * TSDF_BV;
    uint32_t mine = 0;
    for (int z = 0; z < TSDF_B; ++z) {
        const uint32_t code = a.ws.code[base + threadIdx.x + TSDF_THREADS * z];
        if (code & MC_VALID) mine += mc_num_tris[code & 0xff];
    }
    uint32_t total;
    uint32_t run = a.ws.scans[((int64_t)gridDim.x + 1) + slot] + block_excl_scan(mine, total, wt);
    for (int z = 0; z < TSDF_B; ++z) {
        const int l = threadIdx.x + TSDF_THREADS * z;
        const uint32_t code = a.ws.code[base + l];
        if (!(code & MC_VALID)) continue;
        const int cs = code & 0xff, nt = mc_num_tris[cs];
        if (!nt) continue;
        int vx, vy, vz;
        mc_voxel(a, slot, l, vx, vy, vz);
        for (int t = 0; t < nt; ++t) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = mc_tri_edges[cs][3 * t + k];
                const int c = mc_edge_corner[e], ax = mc_edge_axis[e];
                const int64_t j = mc_index(a, vx + (c & 1), vy + ((c >> 1) & 1), vz + (c >> 2));
                tris[3 * (int64_t)run + k] = (int32_t)(a.ws.vert_off[j] + __popc(a.ws.edges[j] & ((1u << ax) - 1u)));
            }
            ++run;
        }
    }
}

// ---------------------------------------------------------------- host side
extern "C" size_t gsr_mcubes_workspace_bytes(int64_t n_alloc) { return mc_ws_layout(nullptr, n_alloc < 0 ? 0 : n_alloc).bytes; }

static int mc_setup(const GsrTsdfVolume* vol, void* ws, size_t ws_bytes, McArgs& a) {
    int64_t n = 0;
    int rc = tsdf_check_volume(vol, a.g, n);
    if (rc != GSR_OK) return rc;
    if (vol->n_alloc < 0 || vol->n_alloc > n) { gsr_set_error("n_alloc %lld out of range", (long long)vol->n_alloc); return GSR_E_INVALID; }
    if (vol->n_alloc == 0) return GSR_OK;
    if (!vol->block_index || !vol->pool || !vol->workspace || vol->pool_blocks < vol->n_alloc) {
        gsr_set_error("volume buffers missing or pool smaller than n_alloc");
        return GSR_E_INVALID;
    }
    a.ws = mc_ws_layout(ws, vol->n_alloc);
    if (!ws || ws_bytes < a.ws.bytes) { gsr_set_error("marching-cubes workspace too small (%zu < %zu bytes)", ws_bytes, a.ws.bytes); return GSR_E_INVALID; }
    a.block_index = vol->block_index;
    a.slot_block = tsdf_ws_layout(vol->workspace, n).slot_block;
    a.pool = vol->pool;
    a.plane = vol->pool_blocks * TSDF_BV;
    return GSR_OK;
}

extern "C" int32_t gsr_mcubes_count(const GsrTsdfVolume* vol, void* ws, size_t ws_bytes, int64_t* n_verts, int64_t* n_tris,
                                    gsr_stream_t stream_) {
    if (!n_verts || !n_tris) { gsr_set_error("n_verts / n_tris are required"); return GSR_E_INVALID; }
    *n_verts = *n_tris = 0;
    McArgs a{};
    int rc = mc_setup(vol, ws, ws_bytes, a);
    if (rc != GSR_OK || vol->n_alloc == 0) return rc;
    const int64_t A = vol->n_alloc;
    unsigned long long* host = gsr_pinned_words(2);
    if (!host) { gsr_set_error("pinned host allocation failed"); return GSR_E_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GSR_HIP_CHECK(hipMemsetAsync(a.ws.totals, 0, 16, s));
    hipLaunchKernelGGL(mc_cube_kernel, dim3((unsigned)A), dim3(TSDF_THREADS), 0, s, a);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)A), dim3(TSDF_THREADS), 0, s, a);
    GSR_LAUNCH_CHECK();
    const dim3 sg((unsigned)scan_tiles(A), 2);
    hipLaunchKernelGGL(mc_scan_reduce_kernel, sg, dim3(SCAN_BLOCK), 0, s, a.ws.counts, a.ws.partial, A);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(mc_scan_apply_kernel, sg, dim3(SCAN_BLOCK), 0, s, a.ws.counts, a.ws.partial, a.ws.scans, A);
    GSR_LAUNCH_CHECK();
    // the one synchronisation of the extraction (as gsr_forward's): the two totals size the caller's output buffers
    GSR_HIP_CHECK(hipMemcpyAsync(host, a.ws.totals, 16, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    if (host[0] > MC_MAX_VERTS || host[1] > MC_MAX_TRIS_TOTAL) {
        gsr_set_error("%llu mesh vertices / %llu triangles exceed int32 indices / 32-bit offsets: raise voxel_size",
                      (unsigned long long)host[0], (unsigned long long)host[1]);
        return GSR_E_UNSUPPORTED;
    }
    *n_verts = (int64_t)host[0];
    *n_tris = (int64_t)host[1];
    return GSR_OK;
}

extern "C" int32_t gsr_mcubes_emit(const GsrTsdfVolume* vol, void* ws, size_t ws_bytes, float* verts, float* colors,
                                   int32_t* tris, gsr_stream_t stream_) {
    McArgs a{};
    int rc = mc_setup(vol, ws, ws_bytes, a);
    if (rc != GSR_OK || vol->n_alloc == 0) return rc;
    if (!verts || !colors || !tris) { gsr_set_error("verts, colors and tris are required"); return GSR_E_INVALID; }
    const int64_t A = vol->n_alloc;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(mc_emit_verts_kernel, dim3((unsigned)A), dim3(TSDF_THREADS), 0, s, a, verts, colors);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(mc_emit_tris_kernel, dim3((unsigned)A), dim3(TSDF_THREADS), 0, s, a, tris);
    GSR_LAUNCH_CHECK();
    return GSR_OK;
}
