// The triangle emission shared by the cluster filter (mesh_post.hip) and the mask culling (mesh_cull.hip): both end in
// marks, two exclusive scans and this kernel; the vertex rows move through compact.hip's gsr_compact_apply.
#pragma once
#include "gsr_common.h"

// emit[t] != 0: triangle t is written at row tri_off[t] with its three indices remapped through vert_off (the exclusive scan
// of the vertex marks).  Order is preserved; every vertex of an emitted triangle must be a marked one.
static __global__ void __launch_bounds__(256) mesh_emit_tris_kernel(const int32_t* __restrict__ tris, int64_t F,
                                                                    const uint8_t* __restrict__ emit,
                                                                    const uint32_t* __restrict__ tri_off,
                                                                    const uint32_t* __restrict__ vert_off,
                                                                    int32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F || !emit[t]) return;
    const int64_t o = 3 * (int64_t)tri_off[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[o + k] = (int32_t)vert_off[tris[3 * t + k]];
}
