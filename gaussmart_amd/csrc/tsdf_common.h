// Shared by tsdf.hip and mcubes.hip: the volume geometry of GsrTsdfVolume (include/gsr.h) and the workspace layout.
#pragma once
#include "gsr_common.h"
#include "scan_bodies.h"

#define TSDF_B 16                    // voxels per block edge
#define TSDF_BV (TSDF_B * TSDF_B * TSDF_B)
#define TSDF_THREADS 256             // one workgroup per block, TSDF_BV / TSDF_THREADS = 16 voxels per thread (one z slice each)

struct TsdfGrid {
    int lo[3];
    int dim[3];
    float vs;
};

__host__ __device__ static inline int64_t scan_tiles(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

// linear block id -> grid block coordinates, and back (x fastest)
__device__ __forceinline__ void tsdf_block_coords(const TsdfGrid& g, int b, int& bx, int& by, int& bz) {
    bx = b % g.dim[0];
    const int r = b / g.dim[0];
    by = r % g.dim[1];
    bz = r / g.dim[1];
}

// slot of the block holding grid voxel (vx, vy, vz) (voxel coordinates relative to the grid's first voxel), -1 if outside
// the grid or unallocated; l = the voxel's entry inside its block
__device__ __forceinline__ int tsdf_voxel_slot(const TsdfGrid& g, const int* __restrict__ block_index, int vx, int vy, int vz,
                                               int& l) {
    if (vx < 0 || vy < 0 || vz < 0) return -1;
    const int bx = vx >> 4, by = vy >> 4, bz = vz >> 4;
    if (bx >= g.dim[0] || by >= g.dim[1] || bz >= g.dim[2]) return -1;
    l = (vx & 15) + TSDF_B * ((vy & 15) + TSDF_B * (vz & 15));
    return block_index[bx + (int64_t)g.dim[0] * (by + (int64_t)g.dim[1] * bz)];
}

// TSDF workspace (n_blocks = grid blocks): [header u32 x 64][stamp i32][slot_block i32][touched i32][flags u8 x 2]
// [scans u32 x 2 (n + 1)][scan partials u32 x 2].  Private to the library except slot_block, whose offset gsr_tsdf_sizes reports
// (callers never re-derive this layout)
struct TsdfWs {
    uint32_t* header;   // [0] out-of-AABB flag of the current view, [1] touched blocks, [2] new blocks
    int* stamp;         // last view (n_views + 1) that touched the block
    int* slot_block;    // slot -> linear block id
    int* touched;       // this view's touched blocks, grid order
    uint8_t* flags;     // [2][n]: touched, new
    uint32_t* scans;    // [2][n + 1]
    uint32_t* partial;  // [2][tiles]
    size_t slot_block_offset;   // byte offset of slot_block (reported by gsr_tsdf_sizes)
    size_t bytes;
};

static inline TsdfWs tsdf_ws_layout(void* base, int64_t n) {
    TsdfWs w{};
    GsrWsCursor c(base);
    w.header = c.take<uint32_t>(64 * 4);
    w.stamp = c.take<int>(n * 4);
    w.slot_block_offset = c.off;
    w.slot_block = c.take<int>(n * 4);
    w.touched = c.take<int>(n * 4);
    w.flags = c.take<uint8_t>(2 * n);
    w.scans = c.take<uint32_t>(2 * (n + 1) * 4);
    w.partial = c.take<uint32_t>(2 * scan_tiles(n) * 4 + 4);
    w.bytes = c.off;
    return w;
}

// shared argument checks of every entry point (include/gsr.h); fills the grid and the block count
int tsdf_check_volume(const GsrTsdfVolume* vol, TsdfGrid& g, int64_t& n_blocks);
