/*
 * gsr.h -- C ABI of libgsr_hip.so: MI355X (gfx950) differentiable 2D-Gaussian-surfel rasterizer
 * and 3-nearest-neighbour mean squared distance.
 *
 * What this replaces in alevalve/gaussmart (paths relative to the reference checkout):
 *   - the native extension `diff_surfel_rasterization._C` (submodules/diff-surfel-rasterization,
 *     an EMPTY un-pinned submodule: .gitmodules:1-3), reached through
 *     `GaussianRasterizer(raster_settings)(means3D, means2D, shs, colors_precomp, opacities,
 *     scales, rotations, cov3D_precomp)`            gaussian_renderer/__init__.py:14,37-53,97-106
 *   - `simple_knn._C.distCUDA2(points)` (submodules/simple-knn, EMPTY: .gitmodules:4-6)
 *                                                   scene/gaussian_model.py:22,261
 * The reference constrains only the Python operator surface; this C layer is what a binding for
 * that surface calls (see INTEGRATION.md for the ctypes / pybind11 stubs).
 *
 * Conventions
 *   - every pointer marked `device` is HIP device memory owned by the CALLER; the library never
 *     frees or retains it and keeps no global mutable state besides the opt-in profiler and one
 *     64-byte pinned host slot per calling thread (the read-back below);
 *   - all work is enqueued on `stream`; gsr_forward performs exactly one stream synchronisation
 *     (to learn the number of tile instances) before it asks for the instance-sized buffers;
 *     gsr_backward synchronises only for scenes whose worst-case gradient rows exceed
 *     GSR_EXACT_ROWS_BYTES (environment, default 8 GiB), to size that buffer exactly;
 *   - matrices are row-major 4x4 in the reference's transposed / row-vector convention
 *     (viewmatrix = W2C^T, projmatrix = viewmatrix @ P^T; scene/cameras.py:56-58);
 *   - return value 0 = ok, negative = GSR_E_*; gsr_last_error() gives the thread's last message.
 */
#ifndef GSR_H_
#define GSR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_ABI_VERSION 18  /* 5: BINNING carries row_count / slot_off / the scan workspace, 72-byte gradient rows, GsrRowScanJob;
                                6: gsr_surface_maps_forward / _backward;
                                7: TSDF fusion and marching cubes (GsrTsdfVolume, gsr_tsdf_*, gsr_mcubes_*);
                                8: mesh post-processing (gsr_mesh_*) and gsr_depth_aabb;
                                9: mesh culling by view masks (gsr_mask_dilate_*, gsr_mesh_cull_*);
                                10: mesh depth rendering and culling by visibility (gsr_mesh_depth_*, gsr_mesh_vis_*);
                                11: DTU mesh evaluation (gsr_mesh_sample_*, gsr_points_*, gsr_dist_mean);
                                12: Tanks-and-Temples mesh evaluation (gsr_mesh_face_centres, gsr_points_transform / _crop_polygon /
                                    _voxel_*, gsr_icp_sums, gsr_dist_score);
                                13: segment-aware initialisation of the point cloud (GsrSegView, gsr_seg_*);
                                14: unbounded mesh export (GsrUnbView, gsr_unb_*);
                                15: LPIPS (gsr_lpips_*);
                                16: frame kernels of the trajectory and viewer pictures (gsr_frame_*);
                                17: DINOv3 ViT encoder and its cosine term (GsrDinoConfig, gsr_dino_*);
                                18: SAM image encoder and mask selection (GsrSamConfig, gsr_sam_*); still 18 with SAM's
                                    prompt encoder and mask decoder (gsr_sam_dec_*, gsr_sam_decode), with SAM2's image
                                    encoder (GsrSam2Config, gsr_sam2_*) and with SAM2's prompt encoder and mask decoder
                                    (gsr_sam2_dec_*, gsr_sam2_decode), and with the gsr_buffer_field names "tile_rect" and
                                    "color_jac", and with the camera clustering of the view selection (gsr_cam_lloyd):
                                    additions only, no existing struct or signature changed */
#define GSR_MAX_CHANNELS 64   /* widest per-pixel payload of gsr_forward / gsr_backward */

typedef void* gsr_stream_t; /* hipStream_t */

enum {
    GSR_OK = 0,
    GSR_E_INVALID = -1,     /* bad argument combination (mirrors the operator's Python checks) */
    GSR_E_HIP = -2,         /* a HIP runtime call failed                                        */
    GSR_E_ALLOC = -3,       /* the caller's allocator returned NULL                             */
    GSR_E_UNSUPPORTED = -4  /* e.g. channels not in {3, 4..64 step 4}, sh_degree > 3            */
};

/* GsrView.flags: reproduce the two places where the recalled upstream backward is not the
 * derivative of its forward.  GSR_FLAGS_UPSTREAM is what the Python operator passes. */
enum {
    GSR_FLAG_CLAMP_PASSTHROUGH = 1, /* gradient flows through alpha = min(0.99, o*G) when clamped */
    GSR_FLAG_FILTER_DEPTH_GRAD = 2, /* low-pass branch: dL/dz also added to dL/dTw.x,.y times s   */
    GSR_FLAGS_UPSTREAM = 3,
    GSR_FLAG_AABB_GRAD_CUTOFF1 = 512, /* third recalled non-derivative (a reviewer's recollection of upstream backward.cu, as
                                       unverifiable here as the two above): the gradient of the screen-space centre
                                       (dL/dmean2D of the low-pass branch -> T) is chained with the weights (1, 1, -1)
                                       although the forward's centre uses (cutoff^2, cutoff^2, -1) = (9, 9, -1).  Not
                                       part of GSR_FLAGS_UPSTREAM; kernels and oracle implement both settings */
    GSR_FLAG_DEBUG_NO_CULL = 4,     /* test aid: ignore the per-wave cull rect (results are bit-identical) */
    GSR_FLAG_DEBUG_RECT_CULL_ONLY = 64, /* test / measurement aid: cull with the rect only, skip the ellipse test (same results) */
    GSR_FLAG_DEFER_COLOR = 16,      /* enqueue the SH colour pass as LATE as possible -- after binning, right before the
                                       compositing -- and announce it through the allocator (GSR_BUF_SYNC_SH): the caller
                                       may make the stream wait there for SH parameters that are still being updated on
                                       another stream (pipelined data-parallel step); the geometry inputs (means, scales,
                                       rotations, opacities) must be final when gsr_forward is called */
    GSR_FLAG_RAW_PARAMS = 8,        /* opacities are logits, scales are log-scales, rotations un-normalised:
                                       the activations of scene/gaussian_model.py:37-43 (sigmoid, exp,
                                       normalize) run inside the kernels and the gradients returned are
                                       w.r.t. the raw parameters */
    GSR_FLAG_FORWARD_ONLY = 128,    /* gsr_forward for inference (render.py / view.py under torch.no_grad();
                                       utils/mesh_utils.py:100-123): colour, allmap and radii are produced as usual, but
                                       nothing is kept for a backward -- the IMAGE buffer is not requested (out->image =
                                       NULL), the touch words of BINNING are not written and gsr_backward must not be
                                       called with these buffers.  Honoured for 3-channel output; ignored for wide payloads */
    GSR_FLAG_COLOR_CACHED = 256,    /* `shs` AND `colors_precomp` given, channels = 3: colors_precomp is a COLOUR CACHE, f32[13 N] =
                                       [ rgb [N,3] | clamp bits u32 [N] | d(rgb)/d(dir) [N,9] ], holding the SH colour of THIS view
                                       for THESE coefficients and positions as gsr_adam_sh_factored_next left it.  gsr_forward
                                       copies rgb / clamp bits of the visible Gaussians into its records where the SH colour
                                       pass would run (same position in the stream, same GSR_FLAG_DEFER_COLOR handling) and
                                       never reads the coefficients; gsr_backward (pass the same pointer and flag) takes
                                       d(rgb)/d(dir) from the cache.  The caller guarantees that the cache matches */
    GSR_FLAG_NO_DIST_MEDIAN = 4096, /* gsr_forward + gsr_backward (RGB payload): the caller consumes neither the distortion (allmap
                                       channel 6) nor the median depth (channel 5) -- the reference's default training configuration,
                                       lambda_dist = 0 and depth_ratio = 0 (arguments/__init__.py:72,87).  Both channels come back
                                       as zeros (not accumulated: the distortion arithmetic is 10 % of the forward), the other five
                                       and the colour are those of the general forward bit for bit; the backward treats the two
                                       channels as constants */
    GSR_FLAG_COLOR_ONLY = 2048,     /* gsr_forward (RGB payload, not with GSR_FLAG_FORWARD_ONLY): the caller does not consume allmap -- a
                                       trainer while no regularizer is active.  out->allmap is NOT written, the kept image state
                                       holds T and the last contributor only; colour, radii and everything the backward walks are
                                       those of the general forward bit for bit.  The backward of such a forward must carry
                                       GSR_FLAG_NO_SURFACE_GRAD (gsr_backward rejects it otherwise) */
    GSR_FLAG_NO_SURFACE_GRAD = 1024, /* gsr_backward only: the caller promises that dL_dallmap is identically zero (it must still
                                       point at W*H*7 zeros) -- the reference's evaluation flags (scripts/dtu_eval.py:45:
                                       --lambda_normal 0 --lambda_dist 0) and the first 7,000 iterations of every run
                                       (train.py:132-133).  The compositing backward then runs without the surface terms on a
                                       16-float staged record; same gradients as without the flag, bit for bit */
    GSR_FLAG_TIGHT_TILES = 8192,    /* gsr_forward: a Gaussian's tile rect is the reference's (the square of its major 3-sigma
                                       extent) INTERSECTED with the tiles its alpha box reaches -- the conservative pixel box of
                                       {alpha >= 1/255} in the splat record, the one the compositing kernels cull every 8x8 quad
                                       with.  A tile is kept iff at least one of its four quads passes that cull, so only list
                                       entries that every wave of their tile rejects are never created: colour, allmap, radii
                                       and every gradient are those of the default lists bit for bit.  tiles_touched, tile_rect,
                                       point_list, ranges and num_rendered are NOT the reference's any more (a Gaussian may keep
                                       radii > 0 and no tile at all); callers that compare lists leave the flag off */
    GSR_FLAG_FACTORED_SH_GRAD = 32  /* gsr_backward with `shs`: the SH gradient of one view is the outer product
                                       basis_k(dir) x g_c of the 16 basis values of the view direction and the
                                       clamp-masked colour gradient g = dL/drgb (utils/sh_utils.py:57-112 is linear in
                                       the coefficients).  With this flag the [N,M,3] arrays dL_dshs / dL_dshs_rest are
                                       NOT written (may be NULL); dL_dcolors, f32[3N + 4], receives g as [N,3] (zeros for
                                       culled Gaussians) followed by the camera position (x, y, z, 0) -- the whole
                                       factored gradient of the view in one contiguous record -- and
                                       gsr_adam_sh_factored rebuilds the gradient inside the optimiser step.  48 -> 3 floats per Gaussian written, re-read and -- in the view-parallel
                                       step -- exchanged between GPUs */
};

/* GaussianRasterizationSettings (gaussian_renderer/__init__.py:37-51) */
typedef struct GsrView {
    int32_t width, height;
    float tanfovx, tanfovy;
    float scale_modifier;
    int32_t sh_degree;       /* active degree, 0..3                                  */
    int32_t sh_coeffs;       /* coefficients stored per Gaussian (shs is [N, M, 3])  */
    int32_t channels;        /* 3 (RGB), or 4..GSR_MAX_CHANNELS (multiple of 4) with
                                colors_precomp [N,channels]: wide per-pixel payload  */
    uint32_t flags;          /* GSR_FLAG_*                                           */
    const float* bg;         /* device f32[channels]                                 */
    const float* viewmatrix; /* device f32[16]                                       */
    const float* projmatrix; /* device f32[16]                                       */
    const float* campos;     /* device f32[3]                                        */
} GsrView;

/* Operator inputs (gaussian_renderer/__init__.py:97-106).  Exactly one of shs / colors_precomp
 * and exactly one of (scales, rotations) / transmat_precomp must be non-NULL. */
typedef struct GsrGaussians {
    int32_t count;                 /* N                                              */
    const float* means3D;          /* device [N,3]                                   */
    const float* shs;              /* device [N,M,3] or NULL                         */
    const float* colors_precomp;   /* device [N,channels] or NULL (16-byte aligned when channels != 3) */
    const float* opacities;        /* device [N] (post-sigmoid)                      */
    const float* scales;           /* device [N,2] (post-exp) or NULL                */
    const float* rotations;        /* device [N,4] (w,x,y,z) or NULL                 */
    const float* transmat_precomp; /* device [N,9] rows Tu,Tv,Tw, or NULL            */
    const float* shs_rest;         /* device [N,M-1,3] or NULL.  When non-NULL, `shs` holds only
                                      the DC coefficient [N,1,3] (split storage = the model's two
                                      feature parameters, no concatenation needed)               */
} GsrGaussians;

/* Buffers the forward hands to the backward.  The caller allocates them through the callback
 * (two-phase: the instance-sized ones are requested after the scan) and keeps them alive until
 * the backward has run.  GSR_BUF_SCRATCH may be released as soon as the call returns
 * (stream-ordered). */
enum { GSR_BUF_GEOM = 0, GSR_BUF_BINNING = 1, GSR_BUF_IMAGE = 2, GSR_BUF_SCRATCH = 3,
       GSR_BUF_SCRATCH2 = 4, GSR_BUF_COUNT = 5,
       /* not a buffer: with GSR_FLAG_DEFER_COLOR the allocator is called once with this kind and 0 bytes right before
          the SH colour pass is enqueued (the last moment the SH parameters may still be in flight on another
          stream: the callback may enqueue a stream wait); any non-NULL return value means "go on" */
       GSR_BUF_SYNC_SH = 100,
       /* not a buffer either: with GSR_FLAG_DEFER_COLOR the allocator is first asked, with this kind and 0 bytes right
          after the geometry pass, for a SECOND stream (hipStream_t) on which the SH parameters will be ready (e.g. the
          stream that is still updating them).  Non-NULL: the colour pass is enqueued on that stream at once, ordered
          after the geometry pass by an event, and only the compositing waits for it -- sorting and binning overlap the
          parameter update AND the colour pass; GSR_BUF_SYNC_SH is then not announced.  NULL: the colour pass stays on
          the call's stream at the late position described above */
       GSR_BUF_COLOR_STREAM = 101 };

/* Must return device memory of >= bytes, 256-byte aligned, or NULL. */
typedef void* (*gsr_alloc_fn)(void* ctx, int32_t which, size_t bytes);

typedef struct GsrForwardOut {
    float* out_color;      /* device [channels,H,W]                                   */
    float* out_allmap;     /* device [7,H,W]: depth, alpha, normal xyz (view space), median
                              depth, distortion (gaussian_renderer/__init__.py:117-141) */
    int32_t* radii;        /* device [N]                                              */
    int32_t num_rendered;  /* out: number of (Gaussian, tile) instances D             */
    void* geom;            /* out: the pointers the allocator returned                */
    void* binning;
    void* image;
} GsrForwardOut;

typedef struct GsrGrads {
    float* dL_dmeans3D;   /* device [N,3]                                              */
    float* dL_dmeans2D;   /* device [N,3]: densification statistic, .z = 0
                             (consumer scene/gaussian_model.py:551-553)                */
    float* dL_dopacity;   /* device [N]                                                */
    float* dL_dshs;       /* device [N,M,3] or NULL                                    */
    float* dL_dcolors;    /* device [N,channels] or NULL (when colors_precomp was given; with
                             GSR_FLAG_FACTORED_SH_GRAD: f32[3N + 4], see the flag)  */
    float* dL_dscales;    /* device [N,2] or NULL                                      */
    float* dL_drotations; /* device [N,4] or NULL                                      */
    float* dL_dtransmat;  /* device [N,9] or NULL (when transmat_precomp was given)    */
    float* dL_dshs_rest;  /* device [N,M-1,3] or NULL (when shs_rest was given)        */
} GsrGrads;

int32_t gsr_abi_version(void);
const char* gsr_last_error(void);

/* Forward: preprocess -> depth sort -> scan -> instance emit -> tile sort -> ranges -> composite. */
int32_t gsr_forward(const GsrView* view, const GsrGaussians* g, GsrForwardOut* out,
                    gsr_alloc_fn alloc, void* alloc_ctx, gsr_stream_t stream);

/* Backward: back-to-front replay per 8x8 pixel quad (one independent list walk per 4x4 block) writing one dense
 * gradient row per (instance, block) the forward blended, then a per-Gaussian reduction + chain rule.  Every element of every non-NULL GsrGrads array is
 * written (no pre-zeroing needed).  Deterministic: no floating-point atomics. */
int32_t gsr_backward(const GsrView* view, const GsrGaussians* g, int32_t num_rendered,
                     const int32_t* radii, const void* geom, const void* binning,
                     const void* image, const float* dL_dcolor, const float* dL_dallmap,
                     GsrGrads* grads, gsr_alloc_fn alloc, void* alloc_ctx, gsr_stream_t stream);

/* The backward starts with an exclusive scan of the per-instance gradient-row counts the forward left in BINNING (two
 * small launches).  Nothing between the forward and the backward depends on it, so kernels that run in between can carry it
 * as a side job: gsr_row_scan_job describes it (pointers into BINNING), gsr_loss_forward_job / gsr_loss_backward_finish
 * take the description and run its two halves in extra workgroups of their own launches (recording that in `stage`), and
 * gsr_backward_with_job skips the scan when it finds both halves done for exactly its buffers.  Entirely optional: with
 * stage < 2 (or no job) the backward scans itself. */
typedef struct GsrRowScanJob {
    const void* counts;      /* device u8[n]   (BINNING "row_count") */
    void* slot_off;          /* device u32[n + 1] */
    void* workspace;         /* device, scan partials */
    int64_t n;               /* instances (num_rendered) */
    int32_t stage;           /* host-side: 0 = nothing enqueued, 1 = first half enqueued, 2 = both */
} GsrRowScanJob;
int32_t gsr_row_scan_job(const void* binning, int32_t num_rendered, int32_t width, int32_t height, GsrRowScanJob* job);
int32_t gsr_backward_with_job(const GsrView* view, const GsrGaussians* g, int32_t num_rendered,
                              const int32_t* radii, const void* geom, const void* binning,
                              const void* image, const float* dL_dcolor, const float* dL_dallmap,
                              GsrGrads* grads, const GsrRowScanJob* job, gsr_alloc_fn alloc, void* alloc_ctx,
                              gsr_stream_t stream);

/* Introspection of the saved buffers, for parity tests.  Writes byte offset and size of a named
 * field inside buffer `which` for a problem of N Gaussians, D instances, W x H pixels.
 * Names: GEOM: "splat" f32[N,20], "clamped" u32[N], "tiles_touched" u32[N], "depth_key" u32[N],
 *        "order" u32[N] (depth rank -> Gaussian id), "offs" u32[N+1] (depth rank -> first emission index),
 *        "tile_rect" u32[N,2] (x0 | y0 << 16, width | height << 16 on the 16-pixel tile grid; 0, 0 when culled),
 *        "color_jac" f32[N,3,3] (d rgb[c] / d dir[a] of the SH colour pass, direction components independent; written
 *        for visible Gaussians only, and present only after a gsr_forward that is neither GSR_FLAG_FORWARD_ONLY nor
 *        GSR_FLAG_COLOR_CACHED and whose colour pass is the 16-lane form -- otherwise the region is absent or stale);
 *        BINNING: "point_list" u32[D], "inst_row" u32[D] (emission index of each list entry), "ranges" u32[tiles,2],
 *                 "covered" u32[tiles,4] (list entries each 8x8 quad staged), "touch" u32[D] (per list entry: one byte per
 *                 quad, one bit per 4x4 block it was blended into; a quad's byte is defined below its `covered`),
 *                 "row_count" u8[D] (gradient rows per instance, by emission index: left by the forward for the backward);
 *        IMAGE: "final_T" f32[3,H,W], "n_contrib" u32[2,H,W]. */
int32_t gsr_buffer_field(int32_t which, const char* name, int32_t N, int32_t D, int32_t W,
                         int32_t H, size_t* offset, size_t* bytes);

/* distCUDA2 (scene/gaussian_model.py:261): mean squared distance to the 3 nearest other points. */
size_t gsr_knn3_workspace_bytes(int32_t n);
int32_t gsr_knn3(const float* xyz, int32_t n, float* out_mean_sqdist, void* workspace,
                 size_t workspace_bytes, gsr_stream_t stream);

/* Stable LSD radix sort of (u32 key, u32 value) pairs on bits [begin_bit, end_bit): the sort the
 * binning uses, exposed so it can be checked bit-exactly at any size. */
size_t gsr_sort_workspace_bytes(int32_t n);
int32_t gsr_sort_pairs_u32(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out,
                           uint32_t* vals_out, int32_t n, int32_t begin_bit, int32_t end_bit,
                           void* workspace, size_t workspace_bytes, gsr_stream_t stream);

/* Fused photometric loss: (1-lambda)*mean|x-y| + lambda*(1 - mean SSIM(x,y)) with
 * the reference's SSIM (utils/loss_utils.py:38-57: 11x11 Gaussian window sigma 1.5, zero padding)
 * as used at train.py:113-114.  img, gt: device f32 [C,H,W].
 * forward : writes maps f32[3,C,H,W] (partials of SSIM kept for the backward) and
 *           partials f32[gsr_loss_num_partials(H,W)] = per-block (sum SSIM, sum |x-y|) pairs which
 *           the caller adds up (fixed order => reproducible loss value).
 * backward: dimg f32[C,H,W] = grad_scale[0] * dloss/dimg (grad_scale is a DEVICE scalar, so no
 *           host sync is needed to chain it). */
int32_t gsr_loss_num_partials(int32_t H, int32_t W);
int32_t gsr_loss_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                         float* maps, float* partials, gsr_stream_t stream);
int32_t gsr_loss_backward(const float* img, const float* gt, const float* maps, int32_t C, int32_t H,
                          int32_t W, float lambda_dssim, const float* grad_scale, float* dimg,
                          gsr_stream_t stream);

/* Fused surface regularizers: from the rasterizer's allmap [7,H,W] straight to
 *   normal_loss = lambda_normal * mean(1 - rend_normal . surf_normal),  dist_loss = lambda_dist * mean(allmap[6])
 * i.e. gaussian_renderer/__init__.py:117-156 + utils/point_utils.py:9-37 + train.py:132-140 of the
 * reference.  kinv_host: HOST f32[9], row-major inverse of the pixel intrinsics the reference builds
 * at utils/point_utils.py:11-17 (ray(x,y) = kinv * [x,y,1] in camera space).
 * forward : partials f32[gsr_loss_num_partials(H,W)] = per-block (sum normal error, sum distortion).
 * backward: d_allmap f32[7,H,W] = grad_scale[0] * d(normal_loss + dist_loss)/d(allmap), every
 *           element written; grad_scale is a DEVICE scalar. */
int32_t gsr_regularizer_forward(const float* allmap, int32_t H, int32_t W, const float* kinv_host,
                                float depth_ratio, float* partials, gsr_stream_t stream);
int32_t gsr_regularizer_backward(const float* allmap, int32_t H, int32_t W, const float* kinv_host,
                                 float depth_ratio, float lambda_normal, float lambda_dist,
                                 const float* grad_scale, float* d_allmap, gsr_stream_t stream);
/* gsr_regularizer_backward that ALSO leaves the partials gsr_regularizer_forward would have written (partials != NULL): the
 * backward evaluates every pixel's surface normal anyway, so a caller that runs the backward right after the forward and
 * reads the loss value only afterwards needs no forward launch of the regularizer at all. */
int32_t gsr_regularizer_backward_partials(const float* allmap, int32_t H, int32_t W, const float* kinv_host,
                                          float depth_ratio, float lambda_normal, float lambda_dist,
                                          const float* grad_scale, float* d_allmap, float* partials,
                                          gsr_stream_t stream);

/* The maps the reference's render() derives from allmap (gaussian_renderer/__init__.py:117-156, utils/point_utils.py:9-37) as
 * TENSORS, for callers that keep the reference's own objective instead of gsr_regularizer_*:
 *   out7[0:3] = allmap[2:5] @ world_view[:3,:3].T   (rend_normal, world space)      rot_host: HOST f32[9] = world_view[:3,:3]
 *   out7[3]   = (1-r) nan_to_num(allmap[0] / allmap[1]) + r nan_to_num(allmap[5])   (surf_depth)
 *   out7[4:7] = normalize(cross of the finite differences of the back-projected depth) * allmap[1], 0 on the border
 *               (surf_normal, world space; alpha not differentiated)                rays_world_host: HOST f32[9] =
 *               c2w[:3,:3] K^-1, ray(x,y) = that * [x,y,1]
 * backward: d_allmap f32[7,H,W] from d_out7 f32[7,H,W] (every element of both read / written; rend_alpha = allmap[1] and
 * rend_dist = allmap[6] are plain slices the caller differentiates itself).  At pixels with allmap[1] = 0 torch leaves 0 / 0
 * on channels 0 and 1; this writes 0 (no splat covers such a pixel and gsr_backward never reads its gradient). */
int32_t gsr_surface_maps_forward(const float* allmap, int32_t H, int32_t W, const float* rays_world_host,
                                 const float* rot_host, float depth_ratio, float* out7, gsr_stream_t stream);
int32_t gsr_surface_maps_backward(const float* allmap, int32_t H, int32_t W, const float* rays_world_host,
                                  const float* rot_host, float depth_ratio, const float* d_out7, float* d_allmap,
                                  gsr_stream_t stream);

/* The whole training objective from the partials of gsr_loss_forward (and, when reg_partials is
 * non-NULL, gsr_regularizer_forward) in one tiny launch:
 *   out5 = { (1-l)*l1 + l*(1-ssim) + ln*normal + ld*dist,  l1,  ssim,  mean normal error,  mean dist }
 * (train.py:113-143).  Fixed summation order => reproducible loss value. */
int32_t gsr_objective_finish(const float* loss_partials, int32_t C, int32_t H, int32_t W,
                             const float* reg_partials, float lambda_dssim, float lambda_normal,
                             float lambda_dist, float* out5, gsr_stream_t stream);

/* gsr_loss_backward and gsr_objective_finish as ONE launch: the backward kernel does not depend on the five scalars, so the
 * workgroup that computes them rides along with it (one kernel boundary less between the forward and the backward of the
 * objective).  For callers that run the backward right after the forward and read the loss value only afterwards: out5 is
 * written by THIS call, not by the forward.  Same values as the two separate calls.  (GsrRowScanJob: see gsr_row_scan_job.) */
int32_t gsr_loss_backward_finish(const float* img, const float* gt, const float* maps, int32_t C, int32_t H,
                                 int32_t W, float lambda_dssim, const float* grad_scale, float* dimg,
                                 const float* loss_partials, const float* reg_partials, float lambda_normal,
                                 float lambda_dist, float* out5 /* NULL: no scalars */,
                                 GsrRowScanJob* job /* NULL, or a job at stage 1: its second half rides along */,
                                 gsr_stream_t stream);
/* gsr_loss_forward with the first half of a row-scan job (NULL, or stage 0 -> 1) in extra workgroups of its launch.
 * out5_invalidate (may be NULL): five floats the launch fills with NaN -- the objective's scalars of a caller that lets
 * gsr_loss_backward_finish write them later, so that a value read before that is visibly invalid. */
int32_t gsr_loss_forward_job(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                             float* maps, float* partials, GsrRowScanJob* job, float* out5_invalidate, gsr_stream_t stream);

/* Dense Adam step over up to 8 parameter tensors in one launch; the update of
 * torch.optim.Adam as the reference configures it (scene/gaussian_model.py:282-295).  All arrays
 * are HOST arrays of length `count`; the pointers inside are device f32 buffers of numel[i]
 * elements.  step_size[i] = lr_i / (1 - beta1^t), inv_bc2_sqrt[i] = 1 / sqrt(1 - beta2^t). */
int32_t gsr_adam_step(int32_t count, float* const* params, const float* const* grads,
                      float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                      const float* step_size, const float* inv_bc2_sqrt, double beta1, double beta2,
                      double eps, gsr_stream_t stream);
/* The same step; keep_old (may be NULL, entries may be NULL): per tensor a device f32 buffer of numel[i] elements that
 * receives the parameter's values BEFORE the update, in the same pass (the factored SH step of the next view needs the
 * positions the backward saw while the positions move: one launch and 24 B per Gaussian less than a copy beside the step). */
int32_t gsr_adam_step_keep(int32_t count, float* const* params, const float* const* grads,
                           float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                           const float* step_size, const float* inv_bc2_sqrt, double beta1, double beta2,
                           double eps, float* const* keep_old, gsr_stream_t stream);

/* Adam step of the two SH parameter tensors (features_dc [N,1,3], features_rest [N,M-1,3]) from FACTORED gradients
 * (GSR_FLAG_FACTORED_SH_GRAD), for the Gaussians [first, first + count):
 *     grad[i,k,c] = grad_scale * sum_{r < n_views} basis_k( normalize(xyz[i] - campos[r]) ) * color_grad[r,i,c]
 * with basis_k = 0 above `sh_degree` (the reference's active degree), summed in view order (reproducible).  One launch:
 * the 48 gradient values of a Gaussian are formed in registers / LDS and never touch HBM.
 *   xyz         device f32 [N,3]: the positions the backward saw (update xyz AFTER this call, or pass a snapshot)
 *   color_grad  device f32 [n_views, view_stride] floats; view r's [N,3] block starts at color_grad + r * view_stride
 *   campos      device f32 [n_views, campos_stride]; n_views <= 16
 *   *_dc / *_rest: parameter, exp_avg, exp_avg_sq of the two tensors; step sizes as for gsr_adam_step.
 * n_views = 1, grad_scale = 1 reproduces gsr_backward's dL_dshs followed by gsr_adam_step. */
int32_t gsr_adam_sh_factored(int32_t first, int32_t count, int32_t sh_coeffs, int32_t sh_degree, const float* xyz,
                             int32_t n_views, const float* color_grad, int64_t view_stride, const float* campos,
                             int32_t campos_stride, float grad_scale,
                             float* p_dc, float* m_dc, float* v_dc, float step_size_dc, float inv_bc2_sqrt_dc,
                             float* p_rest, float* m_rest, float* v_rest, float step_size_rest, float inv_bc2_sqrt_rest,
                             double beta1, double beta2, double eps, gsr_stream_t stream);

/* The same step, followed -- for the same Gaussians, from the coefficients just written, still on chip -- by the SH colour of
 * the NEXT view: color_cache f32[13 n_total] = [ rgb [n_total,3] (+0.5, clamped at 0) | clamp bits u32 [n_total] |
 * d(rgb)/d(dir) [n_total,9] ] for camera position campos_next (device f32[3]), positions xyz_next (device [n_total,3]: the
 * positions the next forward will see, i.e. AFTER their own optimiser step) and active degree sh_degree_next.  A forward /
 * backward with GSR_FLAG_COLOR_CACHED then skips the SH colour pass and its 192-byte read per Gaussian altogether. */
int32_t gsr_adam_sh_factored_next(int32_t first, int32_t count, int32_t sh_coeffs, int32_t sh_degree, const float* xyz,
                                  int32_t n_views, const float* color_grad, int64_t view_stride, const float* campos,
                                  int32_t campos_stride, float grad_scale,
                                  float* p_dc, float* m_dc, float* v_dc, float step_size_dc, float inv_bc2_sqrt_dc,
                                  float* p_rest, float* m_rest, float* v_rest, float step_size_rest, float inv_bc2_sqrt_rest,
                                  double beta1, double beta2, double eps,
                                  const float* xyz_next, const float* campos_next, int32_t sh_degree_next, int32_t n_total,
                                  float* color_cache, gsr_stream_t stream);

/* Row compaction of the per-Gaussian tensors (pruning, scene/gaussian_model.py:398-470: `tensor[mask]` for the six
 * parameters, their Adam moments and the densification statistics).  Two calls:
 *   gsr_compact_plan  : exclusive scan of the device bool mask `keep` [n_rows] into workspace memory;
 *                       *offsets_out (device u32 [n_rows + 1], inside `ws`) maps row -> new row, its last entry is
 *                       the number of rows kept -- the caller reads it to size the destination tensors;
 *   gsr_compact_apply : ONE launch moving up to 24 tensors (row sizes multiples of 4 bytes, host arrays of device
 *                       pointers) from src[i] to dst[i]. */
size_t gsr_compact_workspace_bytes(int64_t n_rows);
int32_t gsr_compact_plan(const uint8_t* keep, int64_t n_rows, void* ws, size_t ws_bytes,
                         const uint32_t** offsets_out, gsr_stream_t stream);
int32_t gsr_compact_apply(int32_t count, const void* const* src, void* const* dst, const int32_t* row_bytes,
                          int64_t n_rows, const uint8_t* keep, const uint32_t* offsets, gsr_stream_t stream);

/* Densification statistics of one iteration (train.py:199-203; scene/gaussian_model.py:551-553) in one launch, no host
 * synchronisation: for radii[i] > 0: max_radii2D[i] = max(max_radii2D[i], radii[i]); xyz_gradient_accum[i] +=
 * ||grad2d[i,:]||; denom[i] += 1.  grad2d = means2D.grad [N,3]; the three state arrays are device f32 [N]. */
int32_t gsr_densify_stats(int32_t n, const int32_t* radii, const float* grad2d, float* max_radii2D,
                          float* xyz_gradient_accum, float* denom, gsr_stream_t stream);

/* ---------------------------------------------------------------- mesh export: TSDF fusion + marching cubes
 * The bounded mesh path of the reference (utils/mesh_utils.py:125-170, Open3D's ScalableTSDFVolume with RGB8 colour, then
 * its marching cubes), as kernels (tsdf.hip, mcubes.hip).
 *
 * Volume: voxel g (integer, world-anchored) has its centre at (g + 0.5) * voxel_size; voxels are grouped in 16^3 blocks,
 * block b holds voxels [16 b, 16 b + 16).  A dense int32 block-index grid covers the block AABB [block_lo, block_hi)
 * (x fastest); an entry is -1 or a slot of the voxel pool.  The pool is SoA, f32 [5][pool_blocks][4096]: tsdf, weight,
 * r, g, b (colour on the 0..255 scale); voxel (x, y, z) of a block is entry x + 16 (y + 16 z).  A new block starts at 0
 * everywhere: the caller zero-fills pool memory it adds.  Slots are handed out in block-grid order by a scan over each view's
 * new blocks (no atomic counter), so the pool layout and the order of the emitted mesh are the same on every run.
 *
 * Recalled Open3D rules (from memory of Open3D's ScalableTSDFVolume / RGBD integration, not read: neither its source nor a
 * build is available to this project -- like the three recalled quirks of the rasterizer above), each kept in one named
 * place of tsdf.hip / mcubes.hip:
 *   TSDF_TOUCH_STRIDE 4          blocks are allocated from the depth pixels on a stride-4 lattice, each marking the blocks
 *                                that overlap [p - sdf_trunc, p + sdf_trunc] (p: the pixel's back-projected point)
 *   TSDF_PIXEL_ROUND 0.5         a voxel reads pixel ((int)(fx x/z + cx + 0.5), (int)(fy y/z + cy + 0.5))
 *   TSDF_BORDER 1e-4             ... only when 1e-4 <= u_f < W - 1e-4 (same for v_f)
 *   tsdf_ray_multiplier()        sdf = (d - z) * sqrt(1 + ((u-cx)/fx)^2 + ((v-cy)/fy)^2)  (distance along the ray)
 *   MC_SKIP_WEIGHT0              a cube with a corner of weight 0 (or in an unallocated block) produces nothing
 * A depth pixel is valid when 0 < d <= depth_trunc and (mask == NULL or mask != 0).
 *
 * Host arrays: intrinsics_host = {fx, fy, cx, cy}; w2c_host = row-major 4x4 world-to-camera (column-vector convention,
 * p_cam = w2c p_world: the TRANSPOSE of the rasterizer's viewmatrix).  depth f32 [H,W], rgb f32 [3,H,W] (clipped to
 * [0,1] and truncated to uint8 inside), mask uint8 [H,W] or NULL. */
#define GSR_TSDF_BLOCK_CAP (1LL << 28)   /* most blocks in a grid (the grid alone is 1 GiB at the cap) */

typedef struct GsrTsdfVolume {
    float voxel_size, sdf_trunc;
    int32_t block_lo[3], block_hi[3];   /* block AABB, hi exclusive; hi == lo on an axis: an empty grid */
    int32_t* block_index;               /* device int32 [n_blocks]; the caller fills it with -1 before the first touch */
    float* pool;                        /* device f32 [5][pool_blocks][4096] */
    int64_t pool_blocks;                /* capacity of the pool (slots); integrate needs pool_blocks >= n_alloc */
    int64_t n_alloc;                    /* slots in use; advanced by gsr_tsdf_touch */
    int32_t n_views;                    /* touches so far; advanced by gsr_tsdf_touch */
    void* workspace;                    /* device, gsr_tsdf_sizes' bytes; ZERO-filled by the caller before the first touch */
    size_t workspace_bytes;
} GsrTsdfVolume;

/* Checks voxel_size, sdf_trunc and the block AABB (GSR_E_INVALID; over GSR_TSDF_BLOCK_CAP blocks: GSR_E_UNSUPPORTED, with a
 * message that names voxel_size and depth_trunc) and gives the grid's block count and the workspace size.  Host only.
 * slot_block_offset (may be NULL): byte offset in the workspace of the slot -> linear block id map, int32 [n_blocks] in slot
 * order.  A caller that loads a volume itself (no touch) fills block_index, that map and n_alloc consistently. */
int32_t gsr_tsdf_sizes(const GsrTsdfVolume* vol, int64_t* n_blocks, size_t* workspace_bytes, size_t* slot_block_offset);

/* One view, first half: marks the blocks its valid depth touches (pixels on the stride-4 lattice), gives the new ones
 * pool slots and lists this view's touched blocks in the workspace.  ONE stream synchronisation (reads back the counts):
 * on return vol->n_alloc and vol->n_views are advanced and *n_touched is the list's length; the caller then grows the pool
 * to n_alloc slots (zero-filled) before gsr_tsdf_integrate.  A touched block outside the AABB fails the call with
 * GSR_E_INVALID and changes nothing (no block is dropped silently).  An empty grid launches nothing. */
int32_t gsr_tsdf_touch(GsrTsdfVolume* vol, const float* depth, const uint8_t* mask, int32_t H, int32_t W,
                       const float* intrinsics_host, const float* w2c_host, float depth_trunc, int64_t* n_touched,
                       gsr_stream_t stream);

/* One view, second half: updates every voxel of the n_touched blocks listed by the preceding gsr_tsdf_touch (same view,
 * same arguments).  Per voxel, z = camera depth of the centre (skip if <= 0), the pixel is found as above, skip if invalid,
 * sdf as above, skip unless sdf > -sdf_trunc; t = min(1, sdf / sdf_trunc); tsdf = (tsdf w + t) / (w + 1), colour likewise
 * with rgb8, w += 1.  One thread per voxel, no atomics: bitwise reproducible. */
int32_t gsr_tsdf_integrate(const GsrTsdfVolume* vol, const float* depth, const uint8_t* mask, const float* rgb, int32_t H,
                           int32_t W, const float* intrinsics_host, const float* w2c_host, float depth_trunc,
                           int64_t n_touched, gsr_stream_t stream);

/* Marching cubes over the allocated blocks.  Cube (x,y,z) has its corners at voxels +{0,1}^3, read across block borders
 * through the grid; case bit i set when tsdf_i < 0 (gaussmart_amd/csrc/mc_tables.h, generated by scripts/gen_mc_tables.py).
 * Each voxel owns its +x, +y, +z edges: one vertex per crossing edge that a produced cube uses (welded, none unreferenced),
 * at p0 + |f0| / (|f0| + |f1|) voxel_size along the edge, colour (c0 |f1| + c1 |f0|) / (|f0| + |f1|) / 255.  Triangle normals
 * (v1-v0)x(v2-v0) point toward positive tsdf.
 *   gsr_mcubes_count: cube codes and per-block counts, scans, and ONE stream synchronisation to read the two totals;
 *   gsr_mcubes_emit : vertices f32 [n_verts,3], colours f32 [n_verts,3], triangles int32 [n_tris,3] (same workspace,
 *                     nothing else enqueued on it in between).
 * No allocated block: nothing is launched and both totals are 0.  Totals above 2^31 - 1 vertices (int32 indices) or 2^32 - 1
 * triangles (32-bit offsets): GSR_E_UNSUPPORTED from gsr_mcubes_count, and gsr_mcubes_emit writes nothing. */
size_t gsr_mcubes_workspace_bytes(int64_t n_alloc);
int32_t gsr_mcubes_count(const GsrTsdfVolume* vol, void* ws, size_t ws_bytes, int64_t* n_verts, int64_t* n_tris,
                         gsr_stream_t stream);
int32_t gsr_mcubes_emit(const GsrTsdfVolume* vol, void* ws, size_t ws_bytes, float* verts, float* colors, int32_t* tris,
                        gsr_stream_t stream);

/* Running world-space AABB of one view's back-projected valid depth (what places the TSDF grid before the first touch).
 * A pixel is valid exactly as in gsr_tsdf_touch; its point is pc = ((u - cx) d / fx, (v - cy) d / fy, d), pw = R pc + t in fp32,
 * with c2w_host the row-major 4x4 camera-to-world matrix (only its first three rows are read).  bounds: device u32 [6] =
 * (min x, y, z, max x, y, z), floats in the order-preserving encoding  key(f) = bits(f) ^ (bits(f) >> 31 ? 0xffffffff :
 * 0x80000000); the caller initialises it to (0xffffffff x 3, 0 x 3) and decodes it once after the last view.  Per-wave min /
 * max, then one integer atomicMin / atomicMax per wave and axis: exact and order-independent.  No synchronisation, no host
 * read; a view without a valid pixel leaves bounds untouched. */
int32_t gsr_depth_aabb(const float* depth, const uint8_t* mask, int32_t H, int32_t W, const float* intrinsics_host,
                       const float* c2w_host, float depth_trunc, uint32_t* bounds, gsr_stream_t stream);

/* ---------------------------------------------------------------- mesh export: triangle clusters and the cluster filter
 * The reference's post_process_mesh (utils/mesh_utils.py:21-42: Open3D's cluster_connected_triangles, then
 * remove_triangles_by_mask / remove_unreferenced_vertices / remove_degenerate_triangles) as kernels (mesh_post.hip), with the
 * semantics of gaussmart_amd/mesh.py: post_process_mesh, bit for bit:
 *   - two triangles are linked when they share an undirected edge (min(a,b), max(a,b)); clusters are the connected
 *     components (all triangles of a non-manifold edge are linked);
 *   - k = min(cluster_to_keep, number of clusters); threshold = max(k-th largest cluster size, 50); a triangle is kept when
 *     its cluster's size is >= threshold (ties are kept);
 *   - a vertex is kept when a kept triangle uses it (decided BEFORE degenerate triangles are dropped); vertices are
 *     compacted in order, triangle indices remapped, then triangles with two equal indices are dropped; order is preserved.
 * tris: device int32 [n_tris,3].  A vertex index outside [0, n_verts) is the caller's error: it is NOT checked on the device
 * (gsr_mesh_clusters only sorts by the indices; the filter indexes per-vertex arrays with them).
 *   gsr_mesh_clusters    : labels[t] = smallest triangle index of t's cluster, cluster_size[t] = its triangle count.  Edge
 *                          records sorted by (lo, hi) with the library's radix sort (two stable sorts over the bits n_verts - 1
 *                          uses), lock-free union-find, integer counts: identical on every run.  No synchronisation.
 *   gsr_mesh_filter_count: clusters, the threshold (on the device), the keep marks and the two scans; ONE stream
 *                          synchronisation reads the two totals.  ws: gsr_mesh_filter_workspace_bytes(n_tris, n_verts).
 *   gsr_mesh_filter_emit : vertices / colours f32 [n_verts_out,3] and triangles int32 [n_tris_out,3] (same arguments, same
 *                          workspace, nothing else enqueued on it in between).
 * n_tris == 0: nothing is launched, the totals are 0.  Negative counts, cluster_to_keep < 1, a null pointer with a non-zero
 * count or a workspace that is too small: GSR_E_INVALID, the message names the argument.  3 n_tris > 2^31 - 1 (the sort's
 * element count) or n_verts > 2^31 - 1: GSR_E_UNSUPPORTED. */
size_t gsr_mesh_clusters_workspace_bytes(int64_t n_tris);
size_t gsr_mesh_filter_workspace_bytes(int64_t n_tris, int64_t n_verts);
int32_t gsr_mesh_clusters(const int32_t* tris, int64_t n_tris, int64_t n_verts, int32_t* labels, int32_t* cluster_size,
                          void* ws, size_t ws_bytes, gsr_stream_t stream);
int32_t gsr_mesh_filter_count(const int32_t* tris, int64_t n_tris, int64_t n_verts, int32_t cluster_to_keep, void* ws,
                              size_t ws_bytes, int64_t* n_verts_out, int64_t* n_tris_out, gsr_stream_t stream);
int32_t gsr_mesh_filter_emit(const float* verts, const float* colors, const int32_t* tris, int64_t n_tris, int64_t n_verts,
                             void* ws, size_t ws_bytes, float* verts_out, float* colors_out, int32_t* tris_out,
                             gsr_stream_t stream);

/* ---------------------------------------------------------------- mesh evaluation: culling by view masks
 * The reference's cull_scan (scripts/eval_dtu/evaluate_single_scene.py:19-101: skimage's binary_dilation with disk(24), a
 * projection of every vertex into every view, grid_sample on the dilated mask, trimesh's update_vertices / update_faces) as
 * kernels (mesh_cull.hip).  Inputs: a mesh (f32 vertices [V,3], optional f32 colours [V,3], int32 triangles [F,3]) and n views,
 * each with a row-major 3x4 projection and a uint8 mask [H,W].  The rules, each in this one place:
 *   CULL_MASK_BINARISE  a mask pixel is set when its byte is non-zero (the reference divides channel 0 by 256 and lets the
 *                       dilation treat non-zero as true).
 *   CULL_DISK           the structuring element of radius r is dx^2 + dy^2 <= r^2.  RECALLED from scikit-image's `disk`, which
 *                       is not available to read here (like the Open3D rules of the block above).  Pixels outside the image
 *                       count as unset; r = 0 is the identity (binarised); the reference uses r = 24.
 *   CULL_PROJECT        the per-view matrix is Pn = P / ||P[2,:3]||, P = (world_mat @ scale_mat)[:3,:4], formed on the host in
 *                       float64 from the float32 matrices and passed as f32 (gaussmart_amd/mesh_cull.py: dtu_projection, which
 *                       refuses det(P[:,:3]) <= 0).  For det > 0 it equals the reference's K/K[2,2] @ inverse(pose) of
 *                       load_K_Rt_from_P (scripts/eval_dtu/render_utils.py:31-52): the third row carries true camera depth,
 *                       which matters only because of the + 1e-6.  On the device in fp32, fmaf in this order:
 *                         p.k = fmaf(Pn[k][2], z, fmaf(Pn[k][1], y, fmaf(Pn[k][0], x, Pn[k][3])))      k = x, y, z
 *                         u = p.x / (p.z + 1e-6f),  v = p.y / (p.z + 1e-6f)
 *                         gx = (u / (Wn - 1) - 0.5f) * 2,  gy = (v / (Hn - 1) - 0.5f) * 2
 *                         valid = -1 < gx < 1 && -1 < gy < 1   (strict; NaN makes it false)
 *                       Wn, Hn: the size the pixel coordinates are normalised by (the reference hard-codes 1600 x 1200, DTU's
 *                       mask size; the Python layer defaults to the mask size).  Wn = 1 or Hn = 1 divides by zero: no vertex
 *                       is valid in such a view.  Depth gets no special treatment: a vertex behind the camera is handled
 *                       exactly as the formula says.
 *   CULL_SAMPLE         ix = nearbyint((gx + 1) / 2 * (W - 1)), half to even; iy likewise with H.  The sample is the dilated
 *                       mask at (iy, ix) when that is inside the image, else 0: grid_sample(mode='nearest',
 *                       padding_mode='zeros', align_corners=True).
 *   CULL_VOTE           a view keeps a vertex when sample != 0 || !valid; a vertex is kept when every view keeps it.  With
 *                       zero views every vertex is kept.
 *   CULL_COMPACT        a triangle is kept when its three vertices are kept.  Kept vertices are compacted in order, whether or
 *                       not a kept triangle still uses them; triangles are remapped with their order preserved; degenerate
 *                       triangles are NOT dropped (trimesh's update_vertices(mask) + update_faces(face_mask); not the rule of
 *                       the cluster filter above).
 *   CULL_TO_WORLD       output vertex = fmaf(v, s, t) per component in fp32, scale_offset_host = (s, t.x, t.y, t.z) with s =
 *                       scale_mat_0[0,0], t = scale_mat_0[:3,3]; NULL: the vertex is copied unchanged.  Colours are carried
 *                       through unchanged.  DEVIATION: the reference does this product in float64 inside trimesh; meshes
 *                       here are f32 end to end.
 *   gsr_mask_dilate_disk : masks, out: device uint8 [n,H,W]; out is 0 / 1.  Exact integer work in two passes (per row the
 *                          horizontal distance to the nearest set pixel, capped at r + 1, in ws; then per pixel the rows dy in
 *                          [-r, r] against the integer span table w(dy) = floor(sqrt(r^2 - dy^2))): the same bytes whatever the
 *                          launch shape.  radius 0 ... 127; larger: GSR_E_UNSUPPORTED.  No synchronisation.
 *   gsr_mesh_cull_count  : the vote (one thread per vertex over the views in index order, out at the first view that removes
 *                          it), the triangle marks and the two scans; ONE stream synchronisation per call reads the two
 *                          totals (a caller that passes the views in k chunks pays the marks, scans and read-back k times).
 *                          dilated: device uint8 [n_views,H,W], non-zero = set; proj_host: host f32 [n_views,12], uploaded into
 *                          ws.  vertex_keep (device uint8 [n_verts], may be NULL) is IN / OUT: on entry the marks left by the
 *                          calls for earlier chunks of views (the caller fills it with 1 before the first), on return those
 *                          marks ANDed with this call's views -- so the views may arrive in chunks and the totals of the
 *                          last call are those of all views.  NULL: the marks start as all kept.
 *                          ws: gsr_mesh_cull_workspace_bytes(n_tris, n_verts, n_views).
 *   gsr_mesh_cull_emit   : vertices / colours f32 [n_verts_out,3] and triangles int32 [n_tris_out,3] of the preceding count
 *                          call (same mesh, same workspace, nothing else enqueued on it in between); colors NULL: colors_out
 *                          is not written.
 * n_verts == 0 launches nothing and the totals are 0; n_tris == 0 launches nothing for the triangles (the vertices of a mesh
 * without triangles are still culled: CULL_COMPACT keeps vertices no triangle uses).  Negative counts, H, W, Wn or Hn < 1, a
 * negative radius, a null pointer with a non-zero count or a workspace that is too small: GSR_E_INVALID before anything is
 * launched, the message names the argument.  A vertex index outside [0, n_verts) is the caller's error, as above. */
size_t gsr_mask_dilate_workspace_bytes(int32_t n, int32_t H, int32_t W);
int32_t gsr_mask_dilate_disk(const uint8_t* masks, int32_t n, int32_t H, int32_t W, int32_t radius, uint8_t* out, void* ws,
                             size_t ws_bytes, gsr_stream_t stream);
size_t gsr_mesh_cull_workspace_bytes(int64_t n_tris, int64_t n_verts, int32_t n_views);
int32_t gsr_mesh_cull_count(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, const uint8_t* dilated,
                            int32_t n_views, int32_t H, int32_t W, int32_t Wn, int32_t Hn, const float* proj_host, void* ws,
                            size_t ws_bytes, uint8_t* vertex_keep, int64_t* n_verts_out, int64_t* n_tris_out,
                            gsr_stream_t stream);
int32_t gsr_mesh_cull_emit(const float* verts, const float* colors, const int32_t* tris, int64_t n_tris, int64_t n_verts,
                           const float* scale_offset_host, void* ws, size_t ws_bytes, float* verts_out, float* colors_out,
                           int32_t* tris_out, gsr_stream_t stream);

/* ---------------------------------------------------------------- mesh evaluation: culling by visibility
 * The reference's Tanks-and-Temples culling (scripts/eval_tnt/cull_mesh.py: pyrender's depth image of the mesh itself from
 * every camera of the trajectory, point_masks at lines 126-176, trimesh's update_faces / remove_unreferenced_vertices) as
 * kernels (mesh_vis.hip).  Inputs: a mesh (f32 vertices [V,3], optional f32 colours [V,3], int32 triangles [F,3]) and n views
 * that share one pinhole fx, fy, cx, cy and an image size H x W.  The rules, each in this one place:
 *   VIS_CAMERA   a view is an OpenCV world-to-camera matrix (x right, y down, z forward), row-major f32 [3,4], formed on the
 *                host in float64 as inverse(camera-to-world) and rounded once (gaussmart_amd/mesh_visibility.py: w2c_from_c2w).
 *                Camera-space position in fp32, fmaf in mc_vote's order:
 *                  p.k = fmaf(M[k][2], z, fmaf(M[k][1], y, fmaf(M[k][0], x, M[k][3])))      k = x, y, z
 *   VIS_RAY      pixel (i, j) (column, row) asks the ray d = ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1).  RECALLED from
 *                pyrender's IntrinsicsCamera projection matrix and OpenGL's sampling at pixel centres; pyrender is not
 *                available to read here (like Open3D and scikit-image in the blocks above).  The half pixel is deliberate:
 *                the reference renders at pixel centres and then samples the image as if pixel i sat at u = i (VIS_SAMPLE).
 *                Both are kept.
 *   VIS_COVER    with camera-space vertices p0, p1, p2 and b0 = (p1 x p2).d, b1 = (p2 x p0).d, b2 = (p0 x p1).d the ray hits
 *                the triangle when the three are all >= 0 or all <= 0 and not all zero: both faces are drawn (the reference's
 *                SKIP_CULL_FACES).  There is no clipping in screen space: a triangle that crosses the camera plane is handled
 *                by this homogeneous form and by VIS_RANGE.  The cross product of an edge is a x b = (ay bz - az by, ...) with
 *                each product and each difference rounded on its own (so a x a = 0 and a x b = -(b x a) exactly), formed from
 *                the endpoint with the smaller vertex index to the other and negated when that reverses the edge; the dot
 *                product is fmaf(c.x, d.x, fmaf(c.y, d.y, c.z)).  Two triangles that share an edge therefore see exactly
 *                opposite values there: a closed mesh has no cracks.  A triangle with a non-finite camera-space coordinate,
 *                or with an index outside [0, V), draws nothing.  GUARD: when all three vertices have p.z >= near, only pixels
 *                with umin - 1 <= i + 0.5 <= umax + 1 (u = fmaf(fx, p.x / p.z, cx) over the three vertices; rows likewise)
 *                are asked.  In exact arithmetic every hit lies inside [umin, umax]; in fp32 the edge functions of a triangle
 *                whose edges are shorter than about |p| fx 2^-23 are rounding noise farther out than one pixel, and such hits
 *                are not wanted.  A triangle with a vertex nearer than `near` (but not all three) is asked at every pixel.
 *   VIS_DEPTH    n = (p1 - p0) x (p2 - p0) (the same cross product), z = (n.p0) / (n.d) with n.p0 = fmaf(n.x, p0.x,
 *                fmaf(n.y, p0.y, n.z p0.z)) and n.d as the dot product above: the plane form.  (The determinant form
 *                det / (b0 + b1 + b2) loses 3e-4 relative on sub-pixel triangles in fp32, the plane form 2e-6.)  n.d == 0: no
 *                hit.
 *   VIS_RANGE    a hit counts when near <= z <= far (0.01 and 20 in the reference); this rejects a non-finite z as well.  A
 *                pixel's depth is the smallest such z over all triangles, 0.0 when there is none.  DEVIATION: OpenGL's
 *                depth buffer quantises z (24 bits of a non-linear function of it) and pyrender converts back; that is not
 *                reproduced, the image holds the fp32 z itself.
 *   VIS_PROJECT  (the vote; p by VIS_CAMERA)  z = p.z + 1e-8f,  u = fmaf(fx, p.x, cx p.z) / z,  v = fmaf(fy, p.y, cy p.z) / z
 *                (the product cx p.z rounded on its own; the reference's K @ p, then the division),
 *                in_frustum = 0 <= u <= W - 1 && 0 <= v <= H - 1 && z > 0 (false for NaN).
 *   VIS_SAMPLE   ds is the bilinear sample of the view's depth image at (u, v) with pixel i at u = i:
 *                grid_sample(align_corners=True, padding_mode='border').  x0 = floor(u), y0 = floor(v),
 *                  ds = I[y0][x0] (x0 + 1 - u)(y0 + 1 - v) + I[y0][x0+1] (u - x0)(y0 + 1 - v)
 *                     + I[y0+1][x0] (x0 + 1 - u)(v - y0) + I[y0+1][x0+1] (u - x0)(v - y0)
 *                each weight one rounded product, the taps added in this order with fmaf; a tap outside the image (only
 *                possible at u = W - 1 or v = H - 1, where its weight is 0) is left out.  A no-hit 0 blends with hit depths
 *                like any other value, as in the reference.  Only in_frustum vertices are sampled, so the border clamp
 *                never acts.
 *   VIS_VOTE     a view sees a vertex when in_frustum && (ds > 0 ? z < ds + eps : true), eps = 0.005 in the reference.  A
 *                vertex is kept when at least min_views views see it (20 in the reference).
 *   VIS_COMPACT  a triangle stays when its three vertices are kept (degenerate ones too); ONLY vertices that a staying
 *                triangle uses are emitted, in order (trimesh's remove_unreferenced_vertices: the "used vertices" rule of the
 *                cluster filter, not CULL_COMPACT), triangles remapped with their order preserved.
 *   gsr_mesh_depth_render : depth_out: device f32 [n_views,H,W] by VIS_CAMERA ... VIS_RANGE.  w2c_host: host f32 [n_views,12],
 *                          uploaded into ws (gsr_mesh_depth_workspace_bytes(n_tris, n_views): 4 bytes per (triangle, view) for
 *                          the work list of the pairs whose pixel box exceeds 8 x 8).  Depths are stored with atomicMin on
 *                          the bit pattern of the positive float, so the images are the same bits on every run, for every
 *                          order of the triangles and every split of the views over calls.  near must be > 0 and below a
 *                          finite far.  n_tris * n_views must stay below 2^32 (GSR_E_UNSUPPORTED: pass fewer views).  No
 *                          synchronisation.
 *   gsr_mesh_vis_count    : VIS_PROJECT ... VIS_VOTE for n_views depth images (device f32 [n_views,H,W]) and their matrices
 *                          (host f32 [n_views,12]; they travel as kernel arguments, 64 views a launch); intrinsics: host f32
 *                          (fx, fy, cx, cy).  counts_inout: device int32 [n_verts], IN / OUT: the caller zeroes it before the
 *                          first chunk of views and every call adds the views that see the vertex, in index order, and stops
 *                          at min_views: the count is CLAMPED at min_views (a vertex that has reached it is not looked at
 *                          again).  No synchronisation.
 *   gsr_mesh_vis_compact_count / gsr_mesh_vis_emit : VIS_COMPACT from the counts, as gsr_mesh_cull_count / _emit: marks, two
 *                          scans and ONE stream synchronisation that reads the two totals; vertex_keep (device uint8
 *                          [n_verts], may be NULL) receives count >= min_views.  ws: gsr_mesh_vis_workspace_bytes(n_tris,
 *                          n_verts), the same for both calls, nothing else enqueued on it in between.  colors NULL: colors_out
 *                          is not written.  n_tris == 0: both totals are 0 and nothing is read back.
 * Negative counts, H or W < 1, near <= 0, near >= far, a null pointer with a non-zero count or a workspace that is too small:
 * GSR_E_INVALID before anything is launched, the message names the argument. */
size_t gsr_mesh_depth_workspace_bytes(int64_t n_tris, int32_t n_views);
int32_t gsr_mesh_depth_render(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, const float* w2c_host,
                              int32_t n_views, int32_t H, int32_t W, float fx, float fy, float cx, float cy, float near,
                              float far, float* depth_out, void* ws, size_t ws_bytes, gsr_stream_t stream);
int32_t gsr_mesh_vis_count(const float* verts, int64_t n_verts, const float* depths, int32_t n_views, int32_t H, int32_t W,
                           const float* w2c_host, const float* intrinsics, float eps, int32_t min_views, int32_t* counts_inout,
                           gsr_stream_t stream);
size_t gsr_mesh_vis_workspace_bytes(int64_t n_tris, int64_t n_verts);
int32_t gsr_mesh_vis_compact_count(const int32_t* tris, int64_t n_tris, int64_t n_verts, const int32_t* counts,
                                   int32_t min_views, void* ws, size_t ws_bytes, uint8_t* vertex_keep, int64_t* n_verts_out,
                                   int64_t* n_tris_out, gsr_stream_t stream);
int32_t gsr_mesh_vis_emit(const float* verts, const float* colors, const int32_t* tris, int64_t n_tris, int64_t n_verts,
                          void* ws, size_t ws_bytes, float* verts_out, float* colors_out, int32_t* tris_out,
                          gsr_stream_t stream);

/* ---------------------------------------------------------------- mesh evaluation: DTU Chamfer distance
 * The reference's scripts/eval_dtu/eval.py (sampling the mesh, shuffle, greedy down-sampling, ObsMask and ground-plane
 * filters, the two nearest-neighbour searches and their means) as kernels (mesh_eval.hip).  All arithmetic is fp64 on the
 * device unless stated, and mesh_eval.o is compiled with -ffp-contract=off, so every expression below rounds operation by
 * operation as numpy's does.  Point clouds are f32 [n,3]; counts are int32-indexable (more: GSR_E_UNSUPPORTED).  The rules,
 * each in this one place:
 *   EVAL_SAMPLE     (eval.py:50-71)  vertices f32, widened to fp64.  Per triangle v1 = p1 - p0, v2 = p2 - p0,
 *                   l1 = sqrt((v1x^2 + v1y^2) + v1z^2), l2 likewise, area2 = |v1 x v2| with the same order of sums and
 *                   v1 x v2 = (v1y v2z - v1z v2y, v1z v2x - v1x v2z, v1x v2y - v1y v2x).  A triangle with `area2 > 0` false
 *                   or with an index outside [0, V) gives nothing.  thr = thresh sqrt(l1 l2 / area2), n1 = floor(l1 / thr),
 *                   n2 = floor(l2 / thr); n1 = 0 or n2 = 0 (or NaN): no sample.  For i = 0 ... n1 (outer), j = 0 ... n2 (inner):
 *                   a = (i + 0.5) / n1, b = (j + 0.5) / n2, the sample is kept iff a + b < 1 and is q = (v1 a + v2 b) + p0.
 *                   (For n1, n2 < 80 this fp64 test equals the integer test (2i+1) n2 + (2j+1) n1 < 2 n1 n2; the fp64 form
 *                   is the rule.)  The output cloud is the V vertices, then the samples in triangle order.
 *                   CAP: a triangle with n1 n2 > 2^24 is refused (GSR_E_UNSUPPORTED, the message names downsample_density).
 *   EVAL_POINT_F32  a sample is rounded once, fp64 -> f32, when it is stored.  DEVIATION: the reference keeps fp64 points;
 *                   DTU coordinates are millimetres up to about 500, an f32 ulp there is 3e-5 mm against a sampling density
 *                   of 0.2 mm.
 *   EVAL_ORDER      the reference shuffles with an unseeded generator; here the caller passes the permutation (device int32
 *                   [n]) and gsr_points_gather applies it: out[k] = points[perm[k]].
 *   EVAL_DIST       for f32 points a, b: dx = (double)a.x - (double)b.x (dy, dz likewise), d2 = (dx dx + dy dy) + dz dz,
 *                   d = sqrt(d2).  Used for every decision and every reported distance.  Pruning bounds are the same
 *                   expression on the fp64 gaps between the query and a box's f32 faces: every operation is monotone, so a
 *                   bound never exceeds the d2 of a point inside the box, and boxes are skipped only when bound > limit.
 *   EVAL_DOWNSAMPLE (eval.py:86-94)  in the order given, point i is kept iff no kept j < i has d2 <= thresh^2 (thresh^2 in
 *                   fp64; inclusive, as radius_neighbors is): the lexicographically first maximal independent set.  Built in
 *                   rounds over three states: an undecided point becomes removed when some lower neighbour is kept, kept when
 *                   all lower neighbours are removed.  A state is written once, so asynchronous in-place updates give the
 *                   sequential result on every run.  The host launches 8 rounds, reads one word back (bit r: somebody was
 *                   undecided after round r) and goes on while the last bit is set; at most n rounds (a sorted chain).
 *   EVAL_NN         (eval.py:119-134)  per query the nearest point of the other cloud by EVAL_DIST: f64 distance and int32
 *                   index, the smallest index among exactly equal d2.  Finite max_dist: a query whose nearest point has
 *                   d >= max_dist gives +inf and -1 (the search prunes at max_dist^2 (1 + 2^-50); the decision is taken on
 *                   d itself).  max_dist = +inf gives the true nearest point.  An empty cloud gives +inf and -1.  Exact for
 *                   any cloud: the searched cloud is sorted by 30-bit Morton code, bounded in leaves of 64 points, nodes of
 *                   64 leaves and tops of 64 nodes; queries run in their own Morton order (codes clamped into the cloud's
 *                   bounds), are seeded from the leaf at the lower bound of their code, and open only boxes whose bound is
 *                   not above the best d2 so far.  Non-finite coordinates are not supported (no fault, no promise).
 *   EVAL_OBSMASK    (eval.py:98-110)  BB widened from f32 [2,3]; Res and patch fp64.  inbound = all(p >= BB0 - patch) &&
 *                   all(p < BB1 + patch 2).  g = rint((p - BB0) / Res), half to even; in_obs = inbound && 0 <= g < shape on
 *                   the three axes && ObsMask[gx][gy][gz] != 0 (uint8, C order of that index).  DEVIATION: the reference
 *                   forms BB0 - patch in f32; here in fp64.  Two compacted clouds, order kept: data_in (inbound), data_in_obs.
 *   EVAL_PLANE      (eval.py:126-130)  a ground-truth point is used when ((P0 x + P1 y) + P2 z) + P3 > 0.
 *   EVAL_MEAN       the mean of the finite entries of a distance array: thread t of workgroup b (of min(1024, ceil(n / 256)))
 *                   adds its elements in index order, a fixed tree adds the 256 sums, one workgroup adds the partials the same
 *                   way: the same bits on every run.  No finite entry: NaN, as numpy's mean of an empty array.
 *   gsr_mesh_sample_count / _emit : EVAL_SAMPLE.  _count: per-triangle counts, their scan and ONE stream synchronisation that
 *                   reads the total; *n_points_out = n_verts + samples.  _emit: points_out device f32 [n_points,3]; same ws
 *                   (gsr_mesh_sample_workspace_bytes(n_tris)), nothing else enqueued on it in between, same thresh.
 *   gsr_points_downsample : EVAL_DOWNSAMPLE; keep_out device uint8 [n]; *rounds_out (host, may be NULL) the rounds it took.
 *                   ws: gsr_points_search_workspace_bytes(n, 0).  Synchronises once per 8 rounds.
 *   gsr_points_nearest : EVAL_NN; dist_out device f64 [n_query], idx_out device int32 [n_query].
 *                   ws: gsr_points_search_workspace_bytes(n_cloud, n_query).  No synchronisation.
 *   gsr_points_obs_filter_count / _emit : EVAL_OBSMASK as gsr_mesh_vis_compact_count / _emit: flags, two scans, ONE
 *                   synchronisation for the two totals; inbound_out / in_obs_out (device uint8 [n], may be NULL) receive the
 *                   flags.  shape_host: host int32 [3]; bb_host: host f32 [6].  _emit: either output may be NULL.
 *   gsr_points_plane_filter : EVAL_PLANE; plane_host: host f64 [4]; keep_out device uint8 [n] (compact with gsr_compact_*).
 *   gsr_dist_mean  : EVAL_MEAN; mean_out device f64 [1], count_out device int64 [1] (may be NULL).  No synchronisation.
 * Negative counts, thresh <= 0, max_dist <= 0, a null pointer with a non-zero count or a workspace that is too small:
 * GSR_E_INVALID before anything is launched, the message names the argument. */
size_t gsr_mesh_sample_workspace_bytes(int64_t n_tris);
int32_t gsr_mesh_sample_count(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, double thresh, void* ws,
                              size_t ws_bytes, int64_t* n_points_out, gsr_stream_t stream);
int32_t gsr_mesh_sample_emit(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, double thresh, void* ws,
                             size_t ws_bytes, float* points_out, gsr_stream_t stream);
int32_t gsr_points_gather(const float* points, int64_t n_src, const int32_t* perm, int64_t n, float* out, gsr_stream_t stream);
size_t gsr_points_search_workspace_bytes(int64_t n_cloud, int64_t n_query);
int32_t gsr_points_downsample(const float* points, int64_t n, double thresh, void* ws, size_t ws_bytes, uint8_t* keep_out,
                              int32_t* rounds_out, gsr_stream_t stream);
int32_t gsr_points_nearest(const float* query, int64_t n_query, const float* cloud, int64_t n_cloud, double max_dist, void* ws,
                           size_t ws_bytes, double* dist_out, int32_t* idx_out, gsr_stream_t stream);
size_t gsr_points_obs_workspace_bytes(int64_t n);
int32_t gsr_points_obs_filter_count(const float* points, int64_t n, const uint8_t* obs_mask, const int32_t* shape_host,
                                    const float* bb_host, double res, double patch, void* ws, size_t ws_bytes,
                                    uint8_t* inbound_out, uint8_t* in_obs_out, int64_t* n_in_out, int64_t* n_in_obs_out,
                                    gsr_stream_t stream);
int32_t gsr_points_obs_filter_emit(const float* points, int64_t n, void* ws, size_t ws_bytes, float* data_in_out,
                                   float* data_in_obs_out, gsr_stream_t stream);
int32_t gsr_points_plane_filter(const float* points, int64_t n, const double* plane_host, uint8_t* keep_out, gsr_stream_t stream);
size_t gsr_dist_mean_workspace_bytes(int64_t n);
int32_t gsr_dist_mean(const double* dist, int64_t n, void* ws, size_t ws_bytes, double* mean_out, int64_t* count_out,
                      gsr_stream_t stream);

/* ---------------------------------------------------------------- mesh evaluation: Tanks-and-Temples F-score
 * The reference's scripts/eval_tnt/run.py (the mesh as a cloud, crop, voxel-grid down-sampling, three ICP refinements, the
 * precision / recall histograms and the F-score) without Open3D or trimesh: kernels in tnt_eval.hip around EVAL_NN's
 * gsr_points_nearest.  Open3D cannot be run beside this code, so the rules below are the rules; they restate what Open3D
 * 0.9 - 0.18 does where that is deterministic and name each deviation.  All arithmetic is fp64 on the device unless stated,
 * tnt_eval.o is compiled with -ffp-contract=off, point clouds are f32 [n,3], counts are int32-indexable (more:
 * GSR_E_UNSUPPORTED).  No floating-point atomic is used: every result has the same bits on every run.  The rules, each in
 * this one place:
 *   TNT_CLOUD       (run.py:94-108)  the evaluated cloud is the mesh's V vertices followed by its F face centres; a centre
 *                   is ((p0 + p1) + p2) / 3 on the fp64-widened f32 vertices, rounded once to f32.  The caller checks the
 *                   index range; the kernel gives a NaN row for an index outside [0, V), never a wild read.
 *   TNT_TRANSFORM   x' = ((T00 x + T01 y) + T02 z) + T03, y' and z' likewise with rows 1 and 2 of the host fp64 4x4 row-major
 *                   matrix T (passed by value); the last row must be (0, 0, 0, 1) (Open3D divides by w; a similarity never
 *                   needs that).
 *   TNT_POINT_F32   a transformed point, a face centre and a voxel's mean are rounded once, fp64 -> f32, when stored.
 *                   DEVIATION: the reference keeps fp64 points; TnT coordinates are metres up to a few tens, an f32 ulp there
 *                   is about 2e-6 m against the smallest tau of 3e-3 m.
 *   TNT_CROP        (Open3D SelectionPolygonVolume::CropInPolygon)  orthogonal_axis a in {0: X, 1: Y, 2: Z}; (u, v) = (1, 2)
 *                   for X, (0, 2) for Y, (0, 1) for Z.  A point p is kept iff min(axis_min, axis_max) <= p[a] <=
 *                   max(axis_min, axis_max) and the number of nodes strictly < p.u over the polygon's edges (i, j = (i + 1)
 *                   mod m) is odd.  An edge gives a node when (Pi.v < p.v && Pj.v >= p.v) || (Pj.v < p.v && Pi.v >= p.v); the
 *                   node is Pi.u + (p.v - Pi.v) / (Pj.v - Pi.v) * (Pj.u - Pi.u), evaluated left to right.  The polygon is a
 *                   device fp64 [m,3] array, 1 <= m <= 256 (more: GSR_E_UNSUPPORTED).
 *   TNT_VOXEL       (Open3D VoxelDownSample)  lo = per-axis minimum of the cloud - 0.5 voxel; cell = floor((p - lo) / voxel)
 *                   per axis; one output point per occupied cell: the sum of the cell's points in ascending input index,
 *                   added sequentially, divided by their number.  Output order: ascending (ix, iy, iz).  DEVIATION: Open3D's
 *                   order is its hash map's and unspecified.  A cell index >= 2^21 on an axis (or a non-finite coordinate) is
 *                   refused: GSR_E_UNSUPPORTED, the message names voxel_size.  Built as: minimum, 63-bit keys ix << 42 |
 *                   iy << 21 | iz, a stable sort of the key's two words from low to high, run heads, their scan; one thread
 *                   per cell walks its run, which is what makes the order of the sum the rule (a cloud that falls into one
 *                   cell is summed by one thread: slow, correct).
 *   TNT_UNIFORM     (registration.py:124-128)  n > max_points (default 4e6): keep the indices 0, k, 2k, ... with
 *                   k = int(round(n / max_points)), Python's round; applied with gsr_points_gather.
 *   TNT_ICP_SUMS    correspondences are gsr_points_nearest(source, target, max_dist = threshold): by EVAL_NN source point i
 *                   corresponds to target idx[i] when d < threshold.  Pass 1 over the pairs (i, idx[i] >= 0): count, sum s,
 *                   sum t, sum d^2 (d = dist[i]).  The host forms the means sm, tm.  Pass 2: sum (t - tm)(s - sm)^T (row-major,
 *                   rows t) and sum |s - sm|^2 = (dx dx + dy dy) + dz dz.  Both passes add in EVAL_MEAN's fixed order.
 *   TNT_ICP_APPLY   DEVIATION for the sake of f32 points: every ICP iteration transforms the ORIGINAL source by the cumulative
 *                   fp64 T (T <- U T on the host), one rounding per iteration, not a rounding of a rounding.
 *   TNT_SCORE       (evaluation.py:173-215)  the int64 count of d < tau, and np.histogram's counts for explicit edges e_0 <=
 *                   ... <= e_B: bin k holds e_k <= d < e_(k+1), the last bin also d == e_B; anything else (NaN, +inf) is in
 *                   no bin.  A value's bin is found by a binary search against the edge values themselves (the caller forms
 *                   them with numpy, so their bits are numpy's); int32 bins in LDS per workgroup, integer atomics to the
 *                   global bins.  1 <= B <= 4096 (more: GSR_E_UNSUPPORTED).
 *   gsr_mesh_face_centres : TNT_CLOUD's centres; centres_out device f32 [n_tris,3].
 *   gsr_points_transform : TNT_TRANSFORM; transform_host: host f64 [16]; out device f32 [n,3] (may not alias points).
 *   gsr_points_crop_polygon : TNT_CROP; polygon device f64 [n_polygon,3]; keep_out device uint8 [n] (compact with gsr_compact_*).
 *   gsr_points_voxel_count / _emit : TNT_VOXEL as gsr_mesh_sample_count / _emit.  _count: keys, sort, heads, scan and ONE
 *                   stream synchronisation that reads the number of cells.  _emit: points_out device f32 [n_cells,3],
 *                   cell_of_point_out (device int32 [n], may be NULL) the output row of every input point; same ws
 *                   (gsr_points_voxel_workspace_bytes(n)), nothing else enqueued on it in between.
 *   gsr_icp_sums   : TNT_ICP_SUMS; dist / idx: gsr_points_nearest's outputs for `source`; means_host NULL: pass 1, out =
 *                   (count, sum s.xyz, sum t.xyz, sum d^2, 0, 0); means_host = host f64 [6] (sm, tm): pass 2, out = (the 9
 *                   sums row-major, sum |s - sm|^2).  out device f64 [10]; ws: gsr_icp_sums_workspace_bytes(n_source).  An
 *                   idx outside [0, n_target) is no pair.  No synchronisation.
 *   gsr_dist_score : TNT_SCORE; edges_host: host f64 [n_bins + 1], finite and not decreasing; count_out device int64 [1],
 *                   hist_out device int64 [n_bins]; ws: gsr_dist_score_workspace_bytes(n_bins).  No synchronisation.
 * Negative counts, voxel_size / tau <= 0, an axis outside 0..2, a null pointer with a non-zero count or a workspace that is
 * too small: GSR_E_INVALID before anything is launched, the message names the argument. */
int32_t gsr_mesh_face_centres(const float* verts, const int32_t* tris, int64_t n_tris, int64_t n_verts, float* centres_out,
                              gsr_stream_t stream);
int32_t gsr_points_transform(const float* points, int64_t n, const double* transform_host, float* out, gsr_stream_t stream);
int32_t gsr_points_crop_polygon(const float* points, int64_t n, int32_t orthogonal_axis, double axis_min, double axis_max,
                                const double* polygon, int32_t n_polygon, uint8_t* keep_out, gsr_stream_t stream);
size_t gsr_points_voxel_workspace_bytes(int64_t n);
int32_t gsr_points_voxel_count(const float* points, int64_t n, double voxel_size, void* ws, size_t ws_bytes, int64_t* n_cells_out,
                               gsr_stream_t stream);
int32_t gsr_points_voxel_emit(const float* points, int64_t n, double voxel_size, void* ws, size_t ws_bytes, float* points_out,
                              int32_t* cell_of_point_out, gsr_stream_t stream);
size_t gsr_icp_sums_workspace_bytes(int64_t n_source);
int32_t gsr_icp_sums(const float* source, int64_t n_source, const float* target, int64_t n_target, const double* dist,
                     const int32_t* idx, const double* means_host, void* ws, size_t ws_bytes, double* out, gsr_stream_t stream);
size_t gsr_dist_score_workspace_bytes(int32_t n_bins);
int32_t gsr_dist_score(const double* dist, int64_t n, const double* edges_host, int32_t n_bins, double tau, void* ws,
                       size_t ws_bytes, int64_t* count_out, int64_t* hist_out, gsr_stream_t stream);

/* ---------------------------------------------------------------- segment-aware initialisation of the point cloud
 * What the reference does to the initial cloud before training: the convex-hull filter (filter/hull_removal.py:10-25), the
 * labelling of points by view masks (identification/main.py:114-148, identification/pc_projection.py:21-135) and the
 * per-segment augmentation (scene/gaussian_model.py:132-258); kernels in seg_init.hip.  The masks are somebody else's
 * (segments_NNN.npz); SAM, the camera clustering and the DINO encoder are not part of this.  All geometry decisions are
 * fp64 on the device, seg_init.o is compiled with -ffp-contract=off, points are f32 or f64 [n,3] (point_f64 = 0 / 1) and
 * are widened on load, counts are int32-indexable (more: GSR_E_UNSUPPORTED).  No floating-point atomic is used: every
 * result has the same bits on every run.  The rules, each in this one place:
 *   SEG_HULL        d_i = min over the facets f, in index order, of |((n_f.x p.x + n_f.y p.y) + n_f.z p.z) + o_f| / |n_f|,
 *                   |n_f| = sqrt((x x + y y) + z z) formed once per facet; equations [F,4] are scipy's ConvexHull.equations
 *                   (Qhull runs on the host).  A NaN distance stays (np.min).  No N x F matrix exists.
 *   SEG_MEANSTD     population mean and standard deviation (np.std, ddof = 0): mean = sum d / n, std = sqrt(sum (d - mean)^2
 *                   / n), each sum in a fixed order (thread t of workgroup b adds elements b 256 + t, + blocks 256, ...; a
 *                   fixed tree over the 256 threads; the partials likewise).  n = 0: NaN, NaN.
 *   SEG_FILTER      keep_i = (d_i - mean) / std >= -theta (theta = 1.96).  std = 0 (every point on the hull) makes z NaN and
 *                   nothing is kept, which is what numpy yields.  Formed by the caller on the device arrays.
 *   SEG_LABEL       one view's masks [M,H,W] (uint8, set = non-zero): label[y,x] = the highest m with masks[m,y,x] != 0, or
 *                   -1; area[m] = number of set pixels of mask m.  The reference overwrites mask by mask, so the last, i.e.
 *                   the highest, index wins (pc_projection.py:125-133).  M <= 32767 (more: GSR_E_UNSUPPORTED); M = 0 gives an
 *                   all -1 map.
 *   SEG_AREAS       areas[m] = max over the views of area[m] (the caller's dict).  The reference keys by the per-view mask
 *                   index, so index 3 of view 0 and index 3 of view 2 are the same segment id; that is kept.
 *   SEG_PROJ_DTU    s = scale_mat [p;1], c = world_mat s, each row ((m0 a + m1 b) + m2 c) + m3 d; u = fx (c.x / c.w) + cx,
 *                   v = fy (c.y / c.w) + cy, z = c.z with fx, fy, cx, cy = camera_mat[0,0], [1,1], [0,2], [1,2].  If fewer than
 *                   0.1 n points have 0 <= u < 1554 and 0 <= v < 1162 (the reference's hard-coded size; an int64 count by
 *                   integer atomics, read from device memory by the later kernels) the view uses the normalised rays instead:
 *                   r = (p - cam_pos) / |p - cam_pos|, u = (r.x / (r.z + 1e-10)) (1554 / 3) + 1554 / 2, v likewise with 1162;
 *                   z stays c.z.  cam_pos = -inv(world_mat[:3,:3]) world_mat[:3,3] is formed by the host with numpy.
 *   SEG_PROJ_NERF   c = R p + t (R, t from world_mat), q = K c (K = camera_mat, 3x3), each row (m0 a + m1 b) + m2 c;
 *                   u = q.x / q.z, v = q.y / q.z, z = c.z.
 *   SEG_PROJ_TYT    lo, hi = per-axis minimum / maximum over the points without a NaN (one reduction shared by all views);
 *                   u = nan_to_num((0.1 + (1 - 2 0.1) (p.x - lo.x) / ((hi.x - lo.x) + 1e-10)) img_w), v likewise with y and
 *                   img_h; z = ((p - cam_pos) . world_mat[2,:3]) added left to right, cam_pos = -R^T t formed by the host.  If
 *                   every point has a NaN, u = v = z = 0.
 *   SEG_ASSIGN      a point takes the label of the first view, in order, with (a) n_masks > 0, (b) 0 <= u < W and 0 <= v < H
 *                   (W, H: that view's label map), (c) z > 0, (d) label[rint(clip(v, 0, H - 1)), rint(clip(u, 0, W - 1))] != -1,
 *                   rint rounding half to even; else -1.  Any NaN makes (b) or (c) false.  Views may differ in size.
 *   SEG_STATS       per label l in [0, n_labels), over the points in ascending index (a stable sort by label): count; mean =
 *                   sum p / count; cov = sum (p - mean)(p - mean)^T / (count - 1) (torch.cov, correction 1); std = sqrt of its
 *                   diagonal; mean colour.  fp64 from the f32 inputs, thread t of the label's workgroup adds the run's elements
 *                   t, t + 256, ... and SEG_MEANSTD's tree adds the 256 sums; the caller rounds once to f32.  count 0: NaN
 *                   means; count 0 or 1: NaN cov and std.
 *   SEG_FACTOR      (caller, batched fp64 on the host) eigh(cov), eigenvalues clamped at 1e-6, V diag(w) V^T, times alpha^2 =
 *                   0.25, Cholesky factor L.  A segment whose L is not finite takes diag(0.5 std) (the reference's except
 *                   branch).
 *   SEG_PLAN        (caller) labels in ascending order; -1 and counts < 5 are skipped; target = max(int(sqrt(area) 0.1), 10),
 *                   area = areas.get(label, median of the areas); add = target - count where positive.
 *   SEG_EMIT        new point i belongs to the segment s with offsets[s] <= i < offsets[s + 1] (binary search); xyz = mean_s +
 *                   L_s eps_i in fp64, each row (l0 e0 + l1 e1) + l2 e2, rounded once to f32; colour = mean colour of s, label
 *                   = labels[s].  eps is the caller's torch.randn((total, 3), generator=...).  DEVIATION: the reference draws
 *                   one MultivariateNormal.sample per segment from the global generator; that random stream is not reproduced.
 *   gsr_seg_hull_distance : SEG_HULL; equations device f64 [n_facets,4]; out device f64 [n].
 *   gsr_seg_mean_std : SEG_MEANSTD; out device f64 [2]; ws: gsr_seg_mean_std_workspace_bytes(n).
 *   gsr_seg_label_map : SEG_LABEL; masks device uint8 [n_masks,H,W]; label device int16 [H,W]; area device int64 [n_masks].
 *   gsr_seg_views_prepare : copies views_host [n_views] into ws, checks that every view with masks has its label map inside
 *                   label_maps (label_elems int16 elements), and enqueues SEG_PROJ_TYT's bounds and SEG_PROJ_DTU's counts.
 *                   ws: gsr_seg_views_workspace_bytes(n_views); the two calls below take the same ws, points and n.
 *   gsr_seg_project : SEG_PROJ_* of view `view`; uv_out device f64 [n,2], z_out device f64 [n].
 *   gsr_seg_assign : SEG_ASSIGN; label_maps device int16 (every view's map at its label_offset); out device int32 [n].
 *   gsr_seg_stats  : SEG_STATS; points, colors device f32 [n,3]; order device int64 [n]; seg_off device int64 [n_labels + 1];
 *                   count_out device int64 [n_labels]; stats_out device f64 [n_labels,18]: mean 3, cov 9, std 3, colour 3.
 *   gsr_seg_augment_emit : SEG_EMIT; eps device f32 [total,3]; offsets device int64 [n_segs + 1]; mean, mean_color device f32
 *                   [n_segs,3]; tril device f32 [n_segs,9]; labels device int64 [n_segs]; outputs device f32 [total,3] twice and
 *                   int64 [total].
 * None of these calls synchronises.  Negative counts, a kind outside the three, a null pointer with a non-zero count or a
 * workspace that is too small: GSR_E_INVALID before anything is launched, the message names the argument. */
#define GSR_SEG_DTU 0
#define GSR_SEG_NERF 1
#define GSR_SEG_TYT 2
typedef struct GsrSegView {
    int32_t kind;             /* GSR_SEG_DTU / _NERF / _TYT */
    int32_t width, height;    /* of this view's label map */
    int32_t n_masks;
    int64_t label_offset;     /* first element of this view's map in label_maps */
    double world_mat[16];     /* row-major 4x4 */
    double scale_mat[16];     /* DTU */
    double camera_mat[9];     /* row-major 3x3 */
    double cam_pos[3];        /* DTU fallback and TYT: the camera centre, formed by the host */
    double img_w, img_h;      /* TYT: the image size of the normalisation */
} GsrSegView;
int32_t gsr_seg_hull_distance(const void* points, int32_t point_f64, int64_t n, const double* equations, int32_t n_facets,
                              double* out, gsr_stream_t stream);
size_t gsr_seg_mean_std_workspace_bytes(int64_t n);
int32_t gsr_seg_mean_std(const double* d, int64_t n, double* out, void* ws, size_t ws_bytes, gsr_stream_t stream);
int32_t gsr_seg_label_map(const uint8_t* masks, int32_t n_masks, int32_t H, int32_t W, int16_t* label, int64_t* area,
                          gsr_stream_t stream);
size_t gsr_seg_views_workspace_bytes(int32_t n_views);
int32_t gsr_seg_views_prepare(const void* points, int32_t point_f64, int64_t n, const GsrSegView* views_host, int32_t n_views,
                              int64_t label_elems, void* ws, size_t ws_bytes, gsr_stream_t stream);
int32_t gsr_seg_project(const void* points, int32_t point_f64, int64_t n, void* ws, size_t ws_bytes, int32_t n_views, int32_t view,
                        double* uv_out, double* z_out, gsr_stream_t stream);
int32_t gsr_seg_assign(const void* points, int32_t point_f64, int64_t n, void* ws, size_t ws_bytes, int32_t n_views,
                       const int16_t* label_maps, int32_t* out, gsr_stream_t stream);
int32_t gsr_seg_stats(const float* points, const float* colors, const int64_t* order, const int64_t* seg_off, int64_t n,
                      int32_t n_labels, int64_t* count_out, double* stats_out, gsr_stream_t stream);
int32_t gsr_seg_augment_emit(const float* eps, const int64_t* offsets, int32_t n_segs, const float* mean, const float* tril,
                             const float* mean_color, const int64_t* labels, int64_t total, float* out_xyz, float* out_color,
                             int64_t* out_label, gsr_stream_t stream);

/* ---------------------------------------------------------------- unbounded mesh export
 * The reference's GaussianExtractor.extract_mesh_unbounded (utils/mesh_utils.py:184-279) and marching_cubes_with_contraction
 * (utils/mcube_utils.py:17-95) as kernels (unbounded.hip; Python: gaussmart_amd/mesh_unbounded.py).  A TSDF field is
 * evaluated on a lattice in contracted space against every view, meshed with gsr_mcubes_*, and the vertices are taken back
 * to the world.  Rules, each in one named place of unbounded.hip (fp32 unless said otherwise; the object is built without
 * fused multiply-adds so that every kernel that runs the shared body rounds alike):
 *   UNB_LATTICE   resolution % crop == 0, n = resolution / crop: the reference's n^3 crops of `crop` points share their
 *                 boundary planes, so they are ONE lattice of G = n (crop - 1) + 1 points per axis; point g sits at
 *                 s = -R + g (2R / (G - 1)), formed in fp64 and rounded to fp32.
 *   UNB_CONTRACT  m = |s| (Euclidean norm of the 3-vector); y = s if m < 1, else (1 / (2 - m)) * (s / m); world point
 *                 x = y radius + center.  For m >= 2 the rule is whatever this arithmetic gives (m > 2: a mirrored point,
 *                 m == 2: a non-finite point that no view accepts); no special case.
 *   UNB_TRUNC     trunc = 5 voxel_size (voxel_size = 2 radius / resolution, rounded once to f32 by the caller), times
 *                 1 / (2 - min(m, 1.9)) where m > 1; for points given in world space (contracted = 0) the plain constant.
 *   UNB_PROJECT   p = [x, 1] @ full_proj_transform, z = p.w, (u, v) = p.xy / z; accepted when -1 < u < 1, -1 < v < 1 and
 *                 z > 0, all strict (a NaN fails them).
 *   UNB_SAMPLE    grid_sample(bilinear, padding_mode = border, align_corners = True): pixel coordinate (u + 1) / 2 (W - 1),
 *                 clamped to [0, W - 1]; taps nw, ne, sw, se with clamped indices, summed in that order.
 *   UNB_FUSE      views in table order: sdf = d - z, accepted further only if sdf > -trunc; t = clamp(sdf / trunc, -1, 1);
 *                 tsdf = (tsdf w + t) / (w + 1), rgb = (rgb w + c) / (w + 1), w += 1.  Start: tsdf = 1, rgb = 0, w = 1 (the
 *                 reference's start; it dims colours by n / (n + 1)).
 *   UNB_ALLOC     the lattice is cut in 16^3 blocks (block b holds lattice points [16 b, 16 b + 16), points beyond G - 1 do
 *                 not exist).  Pass 1 keeps two flags per block: bit 0 = has a negative value, bit 1 = has a non-negative
 *                 one.  Block a is an ANCHOR when the union of the flags over a + {0,1}^3 has both bits; the allocated set
 *                 is the anchors dilated by + {0,1}^3 (every corner of every cube that starts in an anchor).  Slots are
 *                 handed out in grid order by a scan.  Pass 2 evaluates the allocated blocks again, into the pool, with
 *                 weight 1 on the lattice and 0 beyond it.
 *   UNB_VERTEX    gsr_mcubes_* run on that volume with voxel_size 1, so a vertex arrives as (lattice position + 0.5) per
 *                 axis; s = -R + (p - 0.5) (2R / (G - 1)) in fp64, rounded to fp32, then UNB_CONTRACT's inverse, times
 *                 radius plus center, clipped to +-max_range.
 *   UNB_COLOUR    vertex colours are the rgb of gsr_unb_points(vertices, contracted = 0), on the 0..1 scale.
 *
 * GsrUnbView: one record per view in a DEVICE table (read with uniform loads); col_x / col_y / col_w = columns 0, 1 and 3 of
 * the row-major full_proj_transform; depth f32 [H,W] and rgb f32 [3,H,W] on the device; sizes may differ between views.
 * The table's contents are the caller's contract (the library cannot read them on the host).
 *
 *   gsr_unb_lattice_size : G and ceil(G / 16) of (resolution, crop).  Host only.
 *   gsr_unb_points       : points device f32 [n,3] (contracted samples, or world points with contracted = 0); tsdf_out f32 [n];
 *                          rgb_out f32 [n,3] or NULL.  n == 0 launches nothing.
 *   gsr_unb_lattice_box  : the field of lattice points lo + [0, dims) as dense f32 [dims0, dims1, dims2] (z fastest).
 *   gsr_unb_block_flags  : pass 1; flags device u8 [ceil(G/16)^3], x fastest.  One byte per block, no atomics.
 *   gsr_unb_alloc        : UNB_ALLOC on a volume whose block AABB is [0, ceil(G/16))^3: fills block_index and the slot map,
 *                          sets vol->n_alloc.  ONE stream synchronisation (reads the count back).
 *   gsr_unb_fill         : pass 2 into vol->pool (planes tsdf and weight; the colour planes are not written).
 *   gsr_unb_finish       : UNB_VERTEX in place on device f32 [n,3].
 * No entry but gsr_unb_alloc synchronises.  A null table, n_views <= 0, resolution % crop != 0, an empty or out-of-lattice
 * box, a non-positive radius / trunc / R: GSR_E_INVALID before anything touches the device.  No floating-point atomics: the
 * results are the same bits on every run. */
typedef struct GsrUnbView {
    float col_x[4], col_y[4], col_w[4];
    const float* depth;
    const float* rgb;
    int32_t height, width;
} GsrUnbView;
int32_t gsr_unb_lattice_size(int32_t resolution, int32_t crop, int32_t* G, int32_t* blocks_per_axis);
int32_t gsr_unb_points(const GsrUnbView* views, int32_t n_views, const float* points, int64_t n, const float* center_host,
                       float radius, float trunc, int32_t contracted, float* tsdf_out, float* rgb_out, gsr_stream_t stream);
int32_t gsr_unb_lattice_box(const GsrUnbView* views, int32_t n_views, double R, int32_t resolution, int32_t crop,
                            const int32_t* lo_host, const int32_t* dims_host, const float* center_host, float radius, float trunc,
                            float* out, gsr_stream_t stream);
int32_t gsr_unb_block_flags(const GsrUnbView* views, int32_t n_views, double R, int32_t resolution, int32_t crop,
                            const float* center_host, float radius, float trunc, uint8_t* flags, gsr_stream_t stream);
int32_t gsr_unb_alloc(GsrTsdfVolume* vol, int32_t resolution, int32_t crop, const uint8_t* flags, gsr_stream_t stream);
int32_t gsr_unb_fill(const GsrTsdfVolume* vol, const GsrUnbView* views, int32_t n_views, double R, int32_t resolution,
                     int32_t crop, const float* center_host, float radius, float trunc, gsr_stream_t stream);
int32_t gsr_unb_finish(float* verts, int64_t n, double R, int32_t resolution, int32_t crop, const float* center_host,
                       float radius, float max_range, gsr_stream_t stream);

/* ---------------------------------------------------------------- LPIPS
 * The reference's lpipsPyTorch (modules/lpips.py, networks.py, utils.py; called at metrics.py:73 and train.py:326) as kernels
 * (lpips.hip; Python: gaussmart_amd/lpips.py): the AlexNet / VGG16 trunk on the pair of images as a batch of 2, and after each
 * tapped layer the distance of the two unit-normalised feature maps.  fp32 throughout, no reduced-precision format.  Rules:
 *   LP_CONV     y[b,co,oy,ox] = relu(bias[co] + sum_k w[co,k] x[b,ci,oy s - p + ky,ox s - p + kx]); x, y NCHW f32, w
 *               [C_out,C_in,ks,ks] as torch lays it out, zero padding.  The sum is ONE f32 fma chain from 0 over
 *               k = (ci ks + ky) ks + kx ascending (the f32-input matrix instruction), then + bias, then relu; no split over k
 *               and no atomics, so the bits do not depend on the run, the tile or the image's place in the batch.  ks in
 *               {3, 5, 11}; any stride >= 1, pad >= 0, C_in, C_out >= 1 and any output plane >= 1x1.  zscore != 0 (C_in == 3
 *               only): every element read from inside the image is first taken through BaseNet.z_score, (x - mean[ci]) /
 *               std[ci] with mean (-.030, -.088, -.188) and std (.458, .448, .450) as f32 and a true division; the padding
 *               stays 0.
 *   LP_POOL     torch's max_pool2d(ks, stride 2) in floor mode without padding, ks 2 (VGG) or 3 (AlexNet): out = (n - ks) / 2
 *               + 1 per axis; the maximum starts at -inf and a NaN wins.  H, W >= ks.
 *   LP_HEAD     feat f32 [2,C,H,W] (the pair), lin_w f32 [C]; per pixel nx = sqrt(sum_c x_c^2) + 1e-10 (ny likewise) and
 *               v = sum_c w_c (x_c / nx - y_c / ny)^2, every operation in f32 (modules/utils.py:6-8, modules/lpips.py:33-36).
 *               The 256 threads of a workgroup are 8 channel groups x 32 consecutive pixels; a thread adds its C / 8
 *               channels in ascending order and the 8 groups' norms are added in order 0..7.  The mean over H W is the fixed
 *               order of EVAL_MEAN: a thread adds the values of its pixels in index order, the tree d = 128 .. 1 adds the 256
 *               threads, ONE workgroup adds the min(ceil(H W / 32), 1024) partials the same way and divides by H W.  C a
 *               multiple of 8 in [8, 512] (else GSR_E_UNSUPPORTED).  The maps are read once.
 *   LP_FORWARD  taps: VGG after the relus of conv 1_2, 2_2, 3_3, 4_3, 5_3; AlexNet after each of its five relus (its last pool
 *               is never computed).  A head runs as soon as its layer exists; the five values are added in layer order,
 *               (((l0 + l1) + l2) + l3) + l4.  The workspace is two activation buffers of 2 x 64 x (first layer's output
 *               plane) floats, the head's partials and five floats.  Minimum image: 16x16 for VGG (four pools), 31x31 for
 *               AlexNet (11x11 stride 4 pad 2, then two 3x3 pools).
 *
 *   gsr_lpips_conv  : LP_CONV; y device f32 [B,C_out,OH,OW], OH = (H + 2 pad - ks) / stride + 1.
 *   gsr_lpips_pool  : LP_POOL on `planes` planes of H x W.
 *   gsr_lpips_head  : LP_HEAD; out device f32 [1]; ws: gsr_lpips_head_workspace_bytes().
 *   gsr_lpips_forward : conv_w_host / conv_b_host: HOST arrays of the trunk's device pointers in layer order (5 for AlexNet,
 *                     13 for VGG16); lin_w_host: host array of 5 device pointers f32 [C_l]; img0, img1 device f32 [3,H,W],
 *                     taken as they are (the caller's value range); out device f32 [1]; ws: gsr_lpips_workspace_bytes(net, H,
 *                     W) (0 for an unknown net or an empty image).
 * None of these calls synchronises.  An image below the minimum, channels != 3, a null pointer, an unknown net or kernel
 * size, a workspace that is too small: GSR_E_INVALID / GSR_E_UNSUPPORTED before anything is launched, with a message.  All
 * element offsets are 64-bit. */
#define GSR_LPIPS_ALEX 0
#define GSR_LPIPS_VGG 1
int32_t gsr_lpips_conv(const float* x, const float* w, const float* bias, int32_t B, int32_t C_in, int32_t H, int32_t W,
                       int32_t C_out, int32_t ksize, int32_t stride, int32_t pad, int32_t zscore, float* y, gsr_stream_t stream);
int32_t gsr_lpips_pool(const float* x, int64_t planes, int32_t H, int32_t W, int32_t ksize, float* y, gsr_stream_t stream);
size_t gsr_lpips_head_workspace_bytes(void);
int32_t gsr_lpips_head(const float* feat, const float* lin_w, int32_t C, int32_t H, int32_t W, void* ws, size_t ws_bytes,
                       float* out, gsr_stream_t stream);
size_t gsr_lpips_workspace_bytes(int32_t net, int32_t H, int32_t W);
int32_t gsr_lpips_forward(int32_t net, const float* const* conv_w_host, const float* const* conv_b_host,
                          const float* const* lin_w_host, const float* img0, const float* img1, int32_t channels, int32_t H,
                          int32_t W, void* ws, size_t ws_bytes, float* out, gsr_stream_t stream);

/* ---------------------------------------------------------------- frame kernels
 * The reference's utils/render_utils.py (save_img_u8, save_img_f32, create_videos:219-266) and utils/image_utils.py
 * (gradient_map, colormap) on maps that already sit in device memory (frame.hip; Python: gaussmart_amd/frames.py): only u8
 * frames, and the fp32 depth a TIFF needs, have to cross to the host.  Rules:
 *   FRAME_U8        uint8(clip(nan_to_num(x), 0, 1) * 255.0f): NaN -> 0, +inf -> 255, -inf -> 0, ONE fp32 multiply, truncation.
 *                   in f32 [B,C,H,W], C in {1, 3, 4}; out u8 [B,H,W,C].  W % 4 == 0 (and a 16-byte aligned input): a thread
 *                   takes four consecutive pixels of a row, one 16-byte load per channel plane, its 4 C bytes stored as whole
 *                   dwords; otherwise one pixel per thread.  Both paths give the same bytes.
 *   FRAME_STATS     the elements at k <= 8 given ranks (0-based) of the ascending nan_to_num(values): values become
 *                   order-preserving u32 keys (sign bit set: all bits flipped, else the sign bit set; -0 sorts below +0),
 *                   gsr_sort_pairs_u32 sorts them, one kernel picks the k keys and turns them back.  ONE read-back (the k
 *                   floats, one stream synchronisation).  1 <= n <= 2^31 - 1.
 *   FRAME_DEPTH     d = nan_to_num(depth) (NaN -> 0, +-inf -> +-FLT_MAX) is written as fp32 where `clean` is not NULL (the
 *                   TIFF payload).  The video frame (where `frame` is not NULL; one of the two is required): t = ((double)logf(d) - min(lo, hi)) / |hi - lo| in fp64 (numpy 2 promotes
 *                   the reference's normalisation to fp64 through its float64 limits), a NaN t (d < 0, or hi == lo with
 *                   log d == lo) gives (0, 0, 0); otherwise t is clipped to [0, 1], the index is trunc(t * 256) with 256 ->
 *                   255, and the pixel is that row of `table` (device u8 [256,3], staged once per workgroup).  d == 0 gives
 *                   t = -inf, index 0; hi == lo gives +-inf, index 0 or 255: IEEE, as numpy.  depth f32 [B,1,H,W], frame u8
 *                   [B,H,W,3].  Four pixels per thread with one 16-byte load, one 16-byte store and three dword stores where
 *                   the pointers are 16-byte aligned; a scalar tail.
 *   FRAME_SOBEL     gradient_map: per channel, with zero padding and a = row y - 1, m = row y, b = row y + 1 at columns
 *                   x - 1, x, x + 1 (indices 0, 1, 2):
 *                     gx = ((((-.25 a0 + .25 a2) + -.5 m0) + .5 m2) + -.25 b0) + .25 b2
 *                     gy = ((((-.25 a0 + -.5 a1) + -.25 a2) + .25 b0) + .5 b1) + .25 b2
 *                   (the non-zero weights of the 3x3 kernel / 4 in row-major order, added left to right; the weights are
 *                   powers of two, so the products are exact and this order alone decides the bits), mag_c = sqrt(gx gx +
 *                   gy gy), out = sqrt(sum_c mag_c mag_c) with c ascending from 0.  fp32, no fused multiply-add.  image f32
 *                   [C,H,W] -> out f32 [1,H,W], one launch, C looped inside; four pixels of a row per thread.
 *   FRAME_MINMAX    bounds device u32 [2]: the minimum and the maximum of x as order-preserving words (FRAME_STATS' key).
 *                   The call resets them itself; 16-byte loads, wave reduction, one integer atomic per wave and bound, no
 *                   read-back.  A NaN in x is skipped (fminf / fmaxf).
 *   FRAME_COLORMAP  colormap: index = rint((x - min) / (max - min) * 255) in fp32, each operation rounded on its own, IEEE
 *                   division, half to even (torch.round); out[c] = table[index][c] with table device f32 [256,3] staged once
 *                   per workgroup; x f32 [H,W] -> out f32 [3,H,W].  DEVIATION: max == min gives index 0 everywhere (the
 *                   reference converts NaN to an integer there).  A NaN in x: unspecified colour, never an access outside
 *                   the table.
 * Only gsr_frame_order_stats synchronises.  Empty inputs launch nothing (order_stats and minmax need n >= 1).  Bad sizes,
 * null pointers, a workspace that is too small: GSR_E_INVALID / GSR_E_UNSUPPORTED before anything is launched.  All element
 * offsets are 64-bit; no floating-point atomics. */
int32_t gsr_frame_to_u8(const float* in, int32_t B, int32_t C, int32_t H, int32_t W, uint8_t* out, gsr_stream_t stream);
size_t gsr_frame_order_stats_workspace_bytes(int64_t n);
int32_t gsr_frame_order_stats(const float* values, int64_t n, const int64_t* ranks_host, int32_t k, float* out_host, void* ws,
                              size_t ws_bytes, gsr_stream_t stream);
int32_t gsr_frame_depth_vis(const float* depth, int32_t B, int32_t H, int32_t W, double lo, double hi, const uint8_t* table,
                            float* clean, uint8_t* frame, gsr_stream_t stream);
int32_t gsr_frame_sobel(const float* image, int32_t C, int32_t H, int32_t W, float* out, gsr_stream_t stream);
int32_t gsr_frame_minmax(const float* x, int64_t n, uint32_t* bounds, gsr_stream_t stream);
int32_t gsr_frame_colormap(const float* x, int32_t H, int32_t W, const uint32_t* bounds, const float* table, float* out,
                           gsr_stream_t stream);

/* ---------------------------------------------------------------- DINOv3 ViT encoder
 * transformers' DINOv3ViTModel (models/dinov3_vit/modeling_dinov3_vit.py), which the reference's DINOImageEncoder runs in fp16
 * (identification/feature_extraction.py:18-43) for the cosine term of utils/loss_utils.py:77-97, as inference kernels (dino.hip,
 * DN_LINEAR and DN_NORM in vit.hip;
 * Python: gaussmart_amd/dino.py).  head_dim is 64 and the patch 16 x 16; hidden = 64 heads, layers >= 1, intermediate a multiple
 * of 64, registers >= 0, B in 1..8, H, W >= 16 are run-time parameters.  EVERY weight is stored in fp16 (the reference's
 * .half()) and widened exactly where it is used in fp32.  Matrix products take fp16 operands on v_mfma_f32_32x32x16_f16 and
 * accumulate in fp32: one k-ascending chain per output element, no split-K, no atomics, so the bits are the same on every run
 * and for an image alone or inside a batch.  DEVIATION, on purpose: the reference keeps the residual stream in fp16; here it is
 * fp32, as are the LayerNorm statistics, the softmax and the input normalisation.  Rules, with every rounding they perform:
 *   DN_EMBED   x f32 [B,3,H,W] in the caller's range; xn = (x - mean[c]) / std[c] in fp32 (subtraction, true division), ROUNDED
 *              TO fp16; the 16x16 stride-16 convolution is a product over K = 768 (k = c 256 + ky 16 + kx) with the fp16 weight
 *              [hidden,768], fp32 accumulation, + fp32(bias) in fp32, stored as fp32 (no output rounding).  Hp = H / 16,
 *              Wp = W / 16 in integer division: trailing rows and columns are not read, as Conv2d does.  Token order: CLS,
 *              registers, patches row-major; CLS and register rows are the fp16 weights widened.  Output: the fp32 residual
 *              stream [B,T,hidden], T = 1 + registers + Hp Wp.
 *   DN_NORM    per row, fp32: mean = sum / n; var = sum (x - mean)^2 / n (biased); y = (x - mean) * (1 / sqrt(var + eps)) * g
 *              + b with g, b the fp16 weights widened; ROUNDED TO fp16 (the next product's operand), or stored as fp32 with
 *              out_f32 (the final norm).  Sums: a lane adds elements lane, lane + 64, ... in order, the 64 lanes by a xor
 *              butterfly.  x rows are in_stride elements apart (the pooled rows are T hidden apart).
 *   DN_LINEAR  acc[m][n] = sum_k x[m][k] w[n][k], x fp16 [M,K], w fp16 [N,K] row-major (torch's Linear), fp32 accumulation,
 *              K a multiple of 64, any M and N (tails are masked, nothing is padded by the caller).  Epilogues:
 *                GSR_DINO_EPI_BIAS   y = acc + fp32(bias[n]) (bias NULL: + 0), ROUNDED TO fp16.
 *                GSR_DINO_EPI_GELU   u = acc + fp32(bias[n]); y = 0.5 u (1 + erf(u / sqrt 2)) in fp32 (erff), ROUNDED TO fp16.
 *                GSR_DINO_EPI_RESID  resid[m][n] = fma(fp32(lambda[n]), acc + fp32(bias[n]), resid[m][n]) in fp32: LayerScale
 *                                    and the residual addition, ONE fp32 rounding after the bias addition's.
 *   DN_ROPE    in place on q and k (fp16 [B,T,hidden]) of the Hp Wp patch tokens (the last ones of each image) only.  fp32:
 *              coord = 2 ((i + 0.5) / Hp) - 1 for patch row i, likewise over Wp; inv_freq_j = 1 / theta^(j / 16), j < 16;
 *              angle = 2 pi coord inv_freq, laid out as [y: 16, x: 16] and tiled twice to 64; q' = q cos + rotate_half(q) sin
 *              with rotate_half(q) = cat(-q[32:], q[:32]): two fp32 products and one fp32 addition per element, ROUNDED TO
 *              fp16.  (modeling_dinov3_vit.py: get_patches_center_coordinates, DINOv3ViTRopePositionEmbedding,
 *              apply_rotary_pos_emb.)
 *   DN_ATTN    per image and head, non-causal, scale 1/8, in base 2: t_j = (sum_d q_d k_jd) * fp32(log2(e) / 8) (fp16 operands, fp32
 *              accumulation, ONE fp32 rounding for the product), one pass over KV tiles of 64 with a running maximum m and sum
 *              l in fp32: p_j = 2^(t_j - m) (fp32 subtraction, v_exp_f32: 1 ulp); l adds the UNROUNDED p_j; p_j is ROUNDED TO
 *              fp16 for the P V product (fp16 v, fp32 accumulation, rescaled by 2^(m_old - m_new) in fp32 when the maximum
 *              moves); out = acc / l in fp32, ROUNDED TO fp16.  No T x T matrix
 *              exists in memory.  kv rows past T are never read and their scores are -inf before the maximum; query rows past
 *              T are not written.  q, k, v, out: fp16 [B,T,hidden], head h in columns 64 h .. 64 h + 63.
 *   DN_POOL    the final LayerNorm (DN_NORM, fp32 out); pooled[b] is row 0 (CLS) of image b, last_hidden every row.
 *   DN_COS     out = lambda16 * (dot / (max(sqrt(aa), 1e-8) * max(sqrt(bb), 1e-8))), dot = sum a_i b_i, aa = sum a_i^2,
 *              bb = sum b_i^2 in fp32: thread t of 256 adds elements t, t + 256, ... in order, then a fixed tree over the
 *              threads.  lambda16 is the fp16-rounded lambda passed as a float (F.cosine_similarity's definition, times the
 *              reference's fp16 lambda).
 * Weight table of gsr_dino_forward: a HOST array of gsr_dino_num_weights(layers) DEVICE pointers to fp16 arrays, in this order
 * (names: DINOv3ViTModel.state_dict()):
 *   GSR_DINO_W_CLS embeddings.cls_token [hidden]; _REG embeddings.register_tokens [registers,hidden] (NULL with 0 registers);
 *   _PATCH_W embeddings.patch_embeddings.weight [hidden,768]; _PATCH_B its bias [hidden];
 *   then per layer l at GSR_DINO_W_LAYER0 + GSR_DINO_W_PER_LAYER l + GSR_DINO_L_*: norm1.weight, norm1.bias, attention.q_proj
 *   weight, bias, k_proj weight, bias, v_proj weight, bias, o_proj weight, bias, layer_scale1.lambda1, norm2.weight, norm2.bias,
 *   mlp.up_proj weight, bias, mlp.down_proj weight, bias, layer_scale2.lambda1; a projection's bias may be NULL (k_proj of ViT-B);
 *   last: norm.weight, norm.bias.
 * Entry points (all work on the caller's stream, the caller owns every buffer, nothing synchronises):
 *   gsr_dino_embed   : DN_EMBED; x1: image 1 where it does not follow image 0 in memory (else NULL; images 2.. follow x1);
 *                      ws: gsr_dino_embed_workspace_bytes (the fp16 patch rows).
 *   gsr_dino_norm / _linear / _rope / _attn : one rule each, for the tests.  _rope: q or k may be NULL.
 *   gsr_dino_forward : the encoder on B images; pooled f32 [B,hidden]; last_hidden f32 [B,T,hidden] or NULL; ws:
 *                      gsr_dino_workspace_bytes(cfg, B, H, W) (0 for a refused configuration).
 *   gsr_dino_cosine  : DN_COS; a, b device f32 [n]; out device f32 [1].
 * hidden != 64 heads, intermediate % 64 != 0, H or W < 16, B outside 1..8, a workspace that is too small, a null required
 * pointer, a weight table of the wrong length: GSR_E_INVALID before anything is launched, with a message. */
typedef struct GsrDinoConfig {
    int32_t hidden, heads, layers, intermediate, registers;
    float rope_theta, ln_eps;
    float image_mean[3], image_std[3];
} GsrDinoConfig;
enum { GSR_DINO_EPI_BIAS = 0, GSR_DINO_EPI_GELU = 1, GSR_DINO_EPI_RESID = 2 };
enum { GSR_DINO_W_CLS = 0, GSR_DINO_W_REG, GSR_DINO_W_PATCH_W, GSR_DINO_W_PATCH_B, GSR_DINO_W_LAYER0 };
enum { GSR_DINO_L_NORM1_W = 0, GSR_DINO_L_NORM1_B, GSR_DINO_L_Q_W, GSR_DINO_L_Q_B, GSR_DINO_L_K_W, GSR_DINO_L_K_B, GSR_DINO_L_V_W,
       GSR_DINO_L_V_B, GSR_DINO_L_O_W, GSR_DINO_L_O_B, GSR_DINO_L_LS1, GSR_DINO_L_NORM2_W, GSR_DINO_L_NORM2_B, GSR_DINO_L_UP_W,
       GSR_DINO_L_UP_B, GSR_DINO_L_DOWN_W, GSR_DINO_L_DOWN_B, GSR_DINO_L_LS2, GSR_DINO_W_PER_LAYER };
size_t gsr_dino_embed_workspace_bytes(int32_t B, int32_t H, int32_t W);
int32_t gsr_dino_embed(const GsrDinoConfig* cfg, const float* x0, const float* x1, int32_t B, int32_t H, int32_t W, const void* cls,
                       const void* reg, const void* patch_w, const void* patch_b, void* ws, size_t ws_bytes, float* out,
                       gsr_stream_t stream);
int32_t gsr_dino_norm(const float* x, int64_t rows, int32_t hidden, int64_t in_stride, const void* weight, const void* bias,
                      float eps, int32_t out_f32, void* y, gsr_stream_t stream);
int32_t gsr_dino_linear(const void* x, const void* w, const void* bias, const void* lambda, int64_t M, int32_t K, int32_t N,
                        int32_t epilogue, void* out, gsr_stream_t stream);
int32_t gsr_dino_rope(void* q, void* k, int32_t B, int32_t T, int32_t heads, int32_t Hp, int32_t Wp, float theta,
                      gsr_stream_t stream);
int32_t gsr_dino_attn(const void* q, const void* k, const void* v, int32_t B, int32_t T, int32_t heads, void* out,
                      gsr_stream_t stream);
size_t gsr_dino_workspace_bytes(const GsrDinoConfig* cfg, int32_t B, int32_t H, int32_t W);
int32_t gsr_dino_num_weights(int32_t layers);
int32_t gsr_dino_forward(const GsrDinoConfig* cfg, const void* const* weights_host, int32_t n_weights, const float* x0,
                         const float* x1, int32_t B, int32_t H, int32_t W, void* ws, size_t ws_bytes, float* pooled,
                         float* last_hidden, gsr_stream_t stream);
int32_t gsr_dino_cosine(const float* a, const float* b, int32_t n, float lambda16, float* out, gsr_stream_t stream);

/* ---------------------------------------------------------------- SAM automatic mask generation
 * transformers' SamVisionEncoder (models/sam/modeling_sam.py; segment_anything's ImageEncoderViT), which the reference's
 * SAMSegmentation runs in fp32 inside SamAutomaticMaskGenerator (identification/sam.py:41-46,65-92), and the selection of that
 * generator's candidate masks, as inference kernels (sam.hip; Python: gaussmart_amd/sam.py).  The prompt encoder and the mask
 * decoder have a part of their own below (SD_*).  Patch 16 x 16, g = image_size / 16 tokens per side (g <= 256), T = g g; head_dim 64 or 80, hidden =
 * heads head_dim; hidden, mlp_dim and output_channels multiples of 64; layers >= 1; per layer a window size w (0: global
 * attention, else w >= 1); ln_eps 1e-6; one image per call.  A layer's two relative-position tables have EXACTLY 2 s - 1
 * rows, s = g for a global layer and s = w otherwise (then the twin's F.interpolate of the table is the identity); any
 * other length is refused.  EVERY weight is fp16; the residual stream, the LayerNorm statistics and the softmax are fp32:
 * the deviation from the twin's fp16 model that DN_* states, and from the reference's fp32 model in the operands'
 * precision.  Matrix products outside attention are DN_LINEAR (one k-ascending fp32 chain per element) with the epilogues
 * below, LayerNorms are DN_NORM.  Rules, with every rounding:
 *   SV_EMBED   pixel_values f32 [3,S,S], normalised and padded by the caller, ROUNDED TO fp16; the 16x16 stride-16
 *              convolution is a product over K = 768 in DN_EMBED's k order (k = c 256 + ky 16 + kx), fp32 accumulation,
 *              v = acc + fp32(bias[n]), then v + fp32(pos_embed[y][x][n]): two fp32 additions, stored as fp32.  Output: the
 *              fp32 stream [T,hidden], row-major over the grid; no prefix tokens.
 *   layer      xn = DN_NORM(stream) fp16; qkv = DN_LINEAR(xn, qkv.weight, qkv.bias) ROUNDED TO fp16 [T,3 hidden] (q of
 *              head h in columns h head_dim .., k at hidden + .., v at 2 hidden + ..); SV_ATTN; stream += proj (+ bias):
 *              resid = resid + (acc + bias), ONE fp32 addition after the bias's (no LayerScale); xn = DN_NORM(stream);
 *              lin1 with exact GELU (GSR_DINO_EPI_GELU) ROUNDED TO fp16; stream += lin2 (+ bias) likewise.
 *   SV_ATTN    per head and window.  s = g: one window; s = w: ceil(g / w)^2 windows over the grid zero-padded AFTER
 *              layer_norm1.  A padded position is a real KEY of its window: its k and v are the k and v thirds of qkv.bias
 *              (what DN_LINEAR gives on a zero row: fp16(0 + fp32(bias)) = bias), read from the bias; the padded layout is
 *              synthesised, never stored.  Padded QUERIES are not computed into memory or written.  Bias pre-pass (one
 *              launch per layer): rh[q][kh] = sum_d fp32(q_d) fp32(Rh[qh - kh + s - 1][d]), rw likewise over columns, q the
 *              UNSCALED fp16 query, d ascending, the products exact in fp32, one fp32 rounding per addition, STORED AS
 *              fp32 [T,heads,2,s] (2 s values per query and head, not a score row).  Score, fp32, in this order:
 *              t = (((sum_d q_d k_d) * fp32(head_dim^-1/2)) + rh[q][kh]) + rw[q][kw], then t2 = t * fp32(log2 e): FOUR fp32
 *              roundings after the fp32 chain of the product.  One pass over KV tiles of 64 window positions (row-major in
 *              the window) with a running maximum m and sum l in fp32: p = 2^(t2 - m) (v_exp_f32), l adds the UNROUNDED
 *              p, p is ROUNDED TO fp16 for the P V product (fp16 v, fp32 accumulation, rescaled by 2^(m_old - m_new)); out =
 *              acc / l in fp32, ROUNDED TO fp16 [T,hidden].  No score matrix over all keys exists in memory for any layer.
 *              head_dim 80 is five k-steps of 16; the output tiles cover 96 rows of which rows 80..95 are zeros and never
 *              stored.  Positions past s s are never read (scores -inf before the maximum).  A window's bits depend on its
 *              own data only, not on the workgroup that runs it.
 *   SV_NECK    the stream ROUNDED TO fp16; conv1 (1x1, no bias): DN_LINEAR over K = hidden, stored as fp32; channel
 *              LayerNorm per token (DN_NORM, eps 1e-6) ROUNDED TO fp16; conv2 (3x3, padding 1, no bias): DN_LINEAR over
 *              K = 9 C with k = c 9 + ky 3 + kx (Conv2d's own weight layout [C,C,3,3]), zero rows outside the grid, stored
 *              as fp32; channel LayerNorm in fp32, not rounded.  Output f32 [C,g,g].
 *   SM_SCORE   logits f32 [n,L,L]; S = 4 L; input size (ih, iw) <= S; output size (oh, ow); threshold tau, offset delta; a
 *              skip byte per mask (NULL: none).  The value at output pixel (y, x) is F.interpolate(L -> S, bilinear,
 *              align_corners=False), the crop [:ih,:iw], then F.interpolate((ih, iw) -> (oh, ow)), evaluated on the fly from
 *              at most 16 taps, all in fp32 without contraction.  One interpolation along an axis: src = max(scale (dst +
 *              0.5) - 0.5, 0) with scale = 0.25 for the first step and fp32(in) / fp32(out) for the second; i0 = floor(src),
 *              i1 = min(i0 + 1, in - 1), l = src - i0; value = (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx
 *              v11), where the second step's v are first-step values.  (oh, ow) = (ih, iw): the second step is skipped, as
 *              it is the identity.  No up-sampled plane exists in memory.  Per mask: int32 counts[3] = {area: values > tau,
 *              inter: > tau + delta, union: > tau - delta} (tau +- delta one fp32 operation each) and the box of the > tau set
 *              as inclusive XYXY in f32, [0,0,0,0] when the set is empty.  One workgroup per mask, integer sums: thread t
 *              takes pixels t, t + 256, ..., then a fixed tree; no float atomics; the same bits on every run.  A mask with
 *              skip set is not read; its counts and box are zeros.
 *   SM_NMS     boxes f32 [n,4] XYXY, scores f32 [n], keep_in bytes (NULL: all), theta; n <= 3 64^2.  Candidates: keep_in
 *              set and a score that is not NaN.  Order: score descending, ties by index ascending.  iou = inter / (a1 + a2
 *              - inter) in fp32 without contraction, areas (x1 - x0)(y1 - y0) (no + 1: torchvision.ops.box_iou), inter =
 *              max(min(x1) - max(x0), 0) max(min(y1) - max(y0), 0).  A box is suppressed if a KEPT earlier box has iou >
 *              theta; NaN compares false (two zero-area boxes keep each other).  Output: the kept indices in that order
 *              and their count, on the device.
 *   SM_EMIT    for index[m] (mask numbers; outside 0..n-1: a zero plane) the > tau set as uint8 [m,oh,ow], from the same
 *              device function as SM_SCORE: a pixel SM_SCORE counted is set here, bit for bit.  m <= 65535.
 *   one step   gsr_sam_mask_score_direct / _emit_direct: SM_SCORE and SM_EMIT with SAM2's geometry (postprocess_masks): the value
 *              at output pixel (y, x) is ONE F.interpolate((L, L) -> (oh, ow), bilinear, align_corners=False) of the logits:
 *              the axis rule above with scale = fp32(L) / fp32(out) and the four taps read from the logits themselves.  The
 *              same kernels; everything else as SM_SCORE / SM_EMIT state it.
 * Weight table of gsr_sam_encode: a HOST array of gsr_sam_num_weights(layers) DEVICE pointers to fp16 arrays (16-byte
 * aligned), none NULL, in this order (names: SamVisionEncoder.state_dict()):
 *   GSR_SAM_W_PATCH_W patch_embed.projection.weight [hidden,768]; _PATCH_B its bias; _POS pos_embed [g,g,hidden];
 *   per layer l at GSR_SAM_W_LAYER0 + GSR_SAM_W_PER_LAYER l + GSR_SAM_L_*: layers.l.layer_norm1.weight, .bias, attn.qkv.weight
 *   [3 hidden,hidden], attn.qkv.bias, attn.rel_pos_h [2 s - 1,head_dim], attn.rel_pos_w, attn.proj.weight, .bias,
 *   layer_norm2.weight, .bias, mlp.lin1.weight [mlp_dim,hidden], .bias, mlp.lin2.weight, .bias;
 *   last (GSR_SAM_W_NECK entries): neck.conv1.weight [C,hidden], neck.layer_norm1.weight, .bias, neck.conv2.weight [C,C,3,3],
 *   neck.layer_norm2.weight, .bias.
 * GsrSamConfig.window_host and .rel_rows_host are HOST arrays of `layers` entries: the window size of each layer and the row
 * count of its two tables (the C side cannot see a device array's length).
 * Entry points (all on the caller's stream, the caller owns every buffer, nothing synchronises):
 *   gsr_sam_embed / _attn / _neck / _mask_score / _nms / _mask_emit : one rule each; ws from the *_workspace_bytes beside it.
 *       _attn: qkv fp16 [g g,3 hidden] as the layer rule lays it out; window 0 = global; out fp16 [g g,hidden].
 *   gsr_sam_encode : the encoder; pixel_values f32 [3,S,S]; out f32 [C,g,g]; ws: gsr_sam_workspace_bytes(cfg) (0 for a
 *       refused configuration).
 * Any other configuration, a null required pointer, a workspace that is too small, a weight table or a relative-position
 * table of the wrong length: GSR_E_INVALID before anything is launched, with a message. */
typedef struct GsrSamConfig {
    int32_t hidden, heads, head_dim, layers, mlp_dim, output_channels, image_size;
    float ln_eps;
    const int32_t* window_host;
    const int32_t* rel_rows_host;
} GsrSamConfig;
enum { GSR_SAM_W_PATCH_W = 0, GSR_SAM_W_PATCH_B, GSR_SAM_W_POS, GSR_SAM_W_LAYER0 };
enum { GSR_SAM_L_NORM1_W = 0, GSR_SAM_L_NORM1_B, GSR_SAM_L_QKV_W, GSR_SAM_L_QKV_B, GSR_SAM_L_REL_H, GSR_SAM_L_REL_W, GSR_SAM_L_PROJ_W,
       GSR_SAM_L_PROJ_B, GSR_SAM_L_NORM2_W, GSR_SAM_L_NORM2_B, GSR_SAM_L_LIN1_W, GSR_SAM_L_LIN1_B, GSR_SAM_L_LIN2_W, GSR_SAM_L_LIN2_B,
       GSR_SAM_W_PER_LAYER };
enum { GSR_SAM_W_NECK = 6 };
size_t gsr_sam_embed_workspace_bytes(int32_t image_size);
int32_t gsr_sam_embed(const float* pixel_values, int32_t image_size, int32_t hidden, const void* patch_w, const void* patch_b,
                      const void* pos_embed, void* ws, size_t ws_bytes, float* out, gsr_stream_t stream);
size_t gsr_sam_attn_workspace_bytes(int32_t g, int32_t window, int32_t heads);
int32_t gsr_sam_attn(const void* qkv, const void* qkv_bias, const void* rel_pos_h, const void* rel_pos_w, int32_t rel_rows, int32_t g,
                     int32_t window, int32_t heads, int32_t head_dim, void* ws, size_t ws_bytes, void* out, gsr_stream_t stream);
size_t gsr_sam_neck_workspace_bytes(int32_t g, int32_t hidden, int32_t channels);
int32_t gsr_sam_neck(const float* x, int32_t g, int32_t hidden, int32_t channels, const void* conv1_w, const void* ln1_w,
                     const void* ln1_b, const void* conv2_w, const void* ln2_w, const void* ln2_b, void* ws, size_t ws_bytes,
                     float* out, gsr_stream_t stream);
size_t gsr_sam_workspace_bytes(const GsrSamConfig* cfg);
int32_t gsr_sam_num_weights(int32_t layers);
int32_t gsr_sam_encode(const GsrSamConfig* cfg, const void* const* weights_host, int32_t n_weights, const float* pixel_values,
                       void* ws, size_t ws_bytes, float* out, gsr_stream_t stream);
int32_t gsr_sam_mask_score(const float* logits, int32_t n, int32_t L, int32_t ih, int32_t iw, int32_t oh, int32_t ow, float tau,
                           float delta, const uint8_t* skip, int32_t* counts, float* boxes, gsr_stream_t stream);
int32_t gsr_sam_mask_emit(const float* logits, int32_t n, int32_t L, int32_t ih, int32_t iw, int32_t oh, int32_t ow, float tau,
                          const int32_t* index, int32_t m, uint8_t* out, gsr_stream_t stream);
int32_t gsr_sam_mask_score_direct(const float* logits, int32_t n, int32_t L, int32_t oh, int32_t ow, float tau, float delta,
                                  const uint8_t* skip, int32_t* counts, float* boxes, gsr_stream_t stream);
int32_t gsr_sam_mask_emit_direct(const float* logits, int32_t n, int32_t L, int32_t oh, int32_t ow, float tau, const int32_t* index,
                                 int32_t m, uint8_t* out, gsr_stream_t stream);
size_t gsr_sam_nms_workspace_bytes(int32_t n);
int32_t gsr_sam_nms(const float* boxes, const float* scores, const uint8_t* keep_in, int32_t n, float theta, void* ws,
                    size_t ws_bytes, int32_t* kept, int32_t* count, gsr_stream_t stream);

/* ---------------------------------------------------------------- SAM: the prompt encoder and the mask decoder
 * transformers' SamPromptEncoder and SamMaskDecoder in the stock configuration (SamPromptEncoderConfig(), SamMaskDecoderConfig()):
 * hidden 256, two two-way layers, 8 heads, self-attention width 256 (head_dim 32), cross-attention width 128 (head_dim 16),
 * MLP 2048 with ReLU, 4 mask tokens and 1 IoU token, IoU head 256-256-4, up-scaling 256 -> 64 -> 32 by two 2x2 stride-2
 * transposed convolutions (sam_decoder.hip; Python: gaussmart_amd/sam.py).  g = image_size / 16 with 1 <= g <= 64, T = g g (any
 * value); P points, 1 <= P <= 65535.  One prompt is ONE foreground point (label 1) plus the padding token: 7 tokens per point
 * (iou, mask 0..3, point, not-a-point).  multimask output: masks 1..3 and IoU columns 1..3; mask 0's hypernetwork is not
 * computed.  Boxes, mask prompts and several points per prompt are not built.  SAM2's decoder is the next section.
 * Precision: every weight is fp16 except the positional matrix; every product with a weight is DN_LINEAR (fp16 operands, one
 * k-ascending fp32 chain per element, rows independent); LayerNorm statistics (DN_NORM's formula), softmax and the token stream
 * are fp32; the per-point image stream is STORED AS fp16 between stages.  No split-K, no float atomics: a point's bits do not
 * depend on the other points of the call.  LayerNorm eps is 1e-6 except layer_norm_final_attn's 1e-5.  Rules:
 *   SD_PROMPT  point (x, y) f32 in the input frame, S = image_size, G = shared_embedding.positional_embedding f32 [2,128] (NOT
 *              rounded to fp16): a = 2 ((c + 0.5) / S) - 1 per coordinate, arg_j = (ax G[0][j] + ay G[1][j]) * fp32(2 pi), every
 *              operation one fp32 rounding, no contraction; token 0 = [sinf(arg), cosf(arg)] + fp32(point_embed.1) (precise
 *              sinf / cosf, not the hardware approximations), token 1 = fp32(not_a_point_embed).  Output f32 [P,2,256].
 *   SD_IMAGE   once per call: src0[t][c] = fp16(emb[c][t] + fp32(no_mask_embed[c])), pe16[t][c] = fp16(pe[c][t]); for layer 0
 *              kx0 = fp16(k_proj(src0) WITHOUT bias), v0 = fp16(v_proj(src0) + bias) of the token->image attention and qx0 =
 *              fp16(q_proj(src0) without bias) of the image->token attention; for each of the five cross attentions (t2i 0,
 *              i2t 0, t2i 1, i2t 1, final) the positional term proj(pe16) + bias as f32 [T,128] (k_proj for t2i / final,
 *              q_proj for i2t): proj(keys + pe) = proj(keys) + proj(pe).
 *   SD_TOKENS  tokens f32 [P,7,256], qpe = their initial value.  An operand of a product is fp16(tokens) or fp16(tokens + qpe)
 *              (one fp32 addition); q, k, v of the token side are STORED AS fp32.  Self-attention: 8 heads of 32, score
 *              (sum_d q_d k_d, d ascending, fmaf) * fp32(32^-1/2), p = expf(s - max), out = (sum_j p_j v_j, j ascending, fmaf)
 *              / (sum_j p_j), ROUNDED TO fp16; layer 0: q = k = v = tokens and tokens = out_proj(out) (no residual); layer 1:
 *              q = k = tokens + qpe, v = tokens, tokens += out_proj(out) (one fp32 addition after the bias's).  MLP: lin1
 *              ROUNDED TO fp16 then ReLU, tokens += lin2.  layer_norm1..3 and layer_norm_final_attn: DN_NORM in fp32.
 *   SD_T2I     q = q_proj(fp16(tokens + qpe)) f32 [P,7,128]; key of image token t: fp32(kx[t]) + kpe[t] (kx fp16 [T,128] is
 *              kx0 for layer 0, else fp16(k_proj(stream) without bias) per point; kpe of SD_IMAGE); v fp16 [T,128] = v0 or
 *              fp16(v_proj(stream) + bias).  Per (point, head): score = (sum_d q_d k_d, d ascending, fmaf) * 1/4.  A thread
 *              takes keys t, t + 256, ... in order; maximum per query over all keys; p = expf(s - max); l and p v are added
 *              per thread in key order (fmaf), the 64 lanes by a xor butterfly (32, 16, .., 1), the four waves in order;
 *              out = acc / l ROUNDED TO fp16 [P,7,128]; tokens += out_proj(out).  No [T,7] score array is stored.
 *   SD_I2T     per image token and head: q = fp32(qx[t]) + qpe[t] (qx fp16 = qx0 for layer 0, else fp16(q_proj(stream) without
 *              bias)); k = k_proj(fp16(tokens + qpe)), v = v_proj(fp16(tokens)), f32 [P,7,128]; score = (sum_d q_d k_jd) * 1/4,
 *              p_j = expf(s_j - max), ctx = (sum_j p_j v_j) / (sum_j p_j), j ascending, ROUNDED TO fp16 [P,T,128]; a =
 *              out_proj(ctx) + bias as fp32; stream = fp16(layer_norm4(fp32(stream) + a)), the stream of layer 0 being src0.
 *   SD_UP      u = conv1(stream) + bias as fp32 [P T,4,64] (one DN_LINEAR over K = 256 with the weight laid out [(dy 2 + dx) 64
 *              + co][ci]); per (token, tap) the channel LayerNorm over 64 (eps 1e-6), exact GELU, ROUNDED TO fp16; conv2
 *              likewise over K = 64 to [.,(dy 2 + dx) 32 + co] with exact GELU in the epilogue, ROUNDED TO fp16; low_res[p][m]
 *              [4 y + 2 dy1 + dy2][4 x + 2 dx1 + dx2] = sum_c hyper[m][p][c] fp32(c2[c]), c ascending, fmaf, for m = masks
 *              1..3.  The [P,32,4g,4g] up-scaled embedding is stored as fp16 once; low_res is f32 [P,3,4g,4g].
 *   SD_HEADS   after layer_norm_final_attn: hyper[m] = MLP_m(fp16(mask token m)) for m = 1..3 and iou = columns 1..3 of the
 *              IoU head on fp16(iou token); hidden layers ROUNDED TO fp16 then ReLU, the last layer stored as fp32.
 * Weight table of gsr_sam_decode: a HOST array of gsr_sam_dec_num_weights() (= GSR_SAMD_W_COUNT) DEVICE pointers, none NULL,
 * fp16 unless stated (names: SamModel.state_dict()):
 *   GSR_SAMD_W_GAUSS prompt_encoder.shared_embedding.positional_embedding F32 [2,128]; _POINT1 prompt_encoder.point_embed.1.weight;
 *   _NOT_A_POINT prompt_encoder.not_a_point_embed.weight; _NO_MASK prompt_encoder.no_mask_embed.weight; _IOU_TOKEN
 *   mask_decoder.iou_token.weight; _MASK_TOKENS mask_decoder.mask_tokens.weight [4,256];
 *   per layer l at GSR_SAMD_W_LAYER0 + GSR_SAMD_W_PER_LAYER l (mask_decoder.transformer.layers.l.): GSR_SAMD_L_SELF self_attn.
 *   {q,k,v,out}_proj.{weight,bias} (8 entries in that order), _NORM1 layer_norm1.{weight,bias}, _T2I cross_attn_token_to_image
 *   (8), _NORM2, _MLP mlp.lin1.{weight,bias}, mlp.lin2.{weight,bias}, _NORM3, _NORM4, _I2T cross_attn_image_to_token (8);
 *   GSR_SAMD_W_FINAL mask_decoder.transformer.final_attn_token_to_image (8) and layer_norm_final_attn.{weight,bias};
 *   GSR_SAMD_W_UP upscale_conv1.weight re-laid as [(dy 2 + dx) 64 + co][256], its bias repeated 4 times [256],
 *   upscale_layer_norm.{weight,bias}, upscale_conv2.weight as [(dy 2 + dx) 32 + co][64], its bias repeated 4 times [128];
 *   GSR_SAMD_W_HYPER output_hypernetworks_mlps.m.{proj_in,layers.0,proj_out}.{weight,bias} for m = 1, 2, 3 (18);
 *   GSR_SAMD_W_IOU iou_prediction_head.{proj_in,layers.0,proj_out}.{weight,bias} (6; proj_out whole, [4,256] and [4]).
 * Entry points (caller's stream, caller's buffers, nothing synchronises; anything refused is GSR_E_INVALID before a launch):
 *   gsr_sam_dec_prompt  SD_PROMPT.
 *   gsr_sam_dec_t2i     SD_T2I's attention: q f32 [P,7,128]; kx, v fp16 [T,128] (shared != 0) or [P,T,128]; kpe f32 [T,128] or
 *                       NULL (no positional term); out fp16 [P,7,128].
 *   gsr_sam_dec_i2t     SD_I2T whole: qx fp16 [T,128] / [P,T,128] and x fp16 [T,256] / [P,T,256] by `shared`; out_w [256,128],
 *                       out_b, ln_w, ln_b fp16; x_out fp16 [P,T,256] (may be x when shared == 0).
 *   gsr_sam_dec_upscale SD_UP: x fp16 [P,T,256], the six GSR_SAMD_W_UP arrays, hyper f32 [3,P,32]; low_res f32 [P,3,4g,4g].
 *   gsr_sam_decode      everything: emb, pe f32 [256,g,g]; points f32 [P,2]; image_size = 16 g; low_res f32 [P,3,4g,4g]; iou f32
 *                       [P,3].  ws: gsr_sam_decode_workspace_bytes(g, P), about 2 KiB per point and image token. */
enum { GSR_SAMD_W_GAUSS = 0, GSR_SAMD_W_POINT1, GSR_SAMD_W_NOT_A_POINT, GSR_SAMD_W_NO_MASK, GSR_SAMD_W_IOU_TOKEN,
       GSR_SAMD_W_MASK_TOKENS, GSR_SAMD_W_LAYER0 };
enum { GSR_SAMD_L_SELF = 0, GSR_SAMD_L_NORM1 = 8, GSR_SAMD_L_T2I = 10, GSR_SAMD_L_NORM2 = 18, GSR_SAMD_L_MLP = 20, GSR_SAMD_L_NORM3 = 24,
       GSR_SAMD_L_NORM4 = 26, GSR_SAMD_L_I2T = 28, GSR_SAMD_W_PER_LAYER = 36 };
enum { GSR_SAMD_W_FINAL = GSR_SAMD_W_LAYER0 + 2 * GSR_SAMD_W_PER_LAYER, GSR_SAMD_W_UP = GSR_SAMD_W_FINAL + 10,
       GSR_SAMD_W_HYPER = GSR_SAMD_W_UP + 6, GSR_SAMD_W_IOU = GSR_SAMD_W_HYPER + 18, GSR_SAMD_W_COUNT = GSR_SAMD_W_IOU + 6 };
int32_t gsr_sam_dec_prompt(const float* points, int32_t P, int32_t image_size, const float* gauss, const void* point1,
                           const void* not_a_point, float* out, gsr_stream_t stream);
int32_t gsr_sam_dec_t2i(const float* q, const void* kx, const float* kpe, const void* v, int32_t P, int32_t T, int32_t shared,
                        void* out, gsr_stream_t stream);
size_t gsr_sam_dec_i2t_workspace_bytes(int32_t P, int32_t T);
int32_t gsr_sam_dec_i2t(const void* qx, const float* qpe, const float* k, const float* v, const void* x, int32_t P, int32_t T,
                        int32_t shared, const void* out_w, const void* out_b, const void* ln_w, const void* ln_b, void* ws,
                        size_t ws_bytes, void* x_out, gsr_stream_t stream);
size_t gsr_sam_dec_upscale_workspace_bytes(int32_t g, int32_t P);
int32_t gsr_sam_dec_upscale(const void* x, int32_t g, int32_t P, const void* conv1_w, const void* conv1_b, const void* ln_w,
                            const void* ln_b, const void* conv2_w, const void* conv2_b, const float* hyper, void* ws, size_t ws_bytes,
                            float* low_res, gsr_stream_t stream);
int32_t gsr_sam_dec_num_weights(void);
size_t gsr_sam_decode_workspace_bytes(int32_t g, int32_t P);
int32_t gsr_sam_decode(int32_t g, const void* const* weights_host, int32_t n_weights, const float* emb, const float* pe,
                       const float* points, int32_t P, int32_t image_size, void* ws, size_t ws_bytes, float* low_res, float* iou,
                       gsr_stream_t stream);

/* ---------------------------------------------------------------- SAM2: the prompt encoder and the mask decoder
 * transformers' Sam2PromptEncoder and Sam2MaskDecoder (models/sam2/modeling_sam2.py, stock configuration) for one foreground
 * point per prompt and multimask output, on the kernels of the section above (sam_decoder.hip; Python: gaussmart_amd/sam2.py).
 * Sizes, limits and precision are SD_*'s: hidden 256, two two-way layers, 8 heads, widths 256 and 128, MLP 2048 with ReLU, four
 * mask tokens, skip_first_layer_pe, 1 <= g <= 64, 1 <= P <= 65535, fp16 operands with one k-ascending fp32 chain per element,
 * fp32 token stream, statistics and softmax, the per-point image stream stored as fp16, no split-K, no float atomics, a
 * point's bits independent of the other points of the call.  Every SD_* rule holds as written except for these deltas:
 *   S2D_TOKENS 8 tokens per point: obj_score_token, iou_token, mask tokens 0..3, the point, not-a-point.  The IoU token is
 *              row 1 and the mask tokens are rows 2..5; wherever SD_TOKENS, SD_T2I and SD_I2T say 7, read 8.  The object-score
 *              token takes part in every attention.  Its head (pred_obj_score_head) is NOT computed: the automatic mask
 *              generator ignores the object score, and so does gaussmart_amd.sam2.decode_host2.
 *   S2D_EPS    layer_norm1..4 of both two-way layers are plain nn.LayerNorm: eps 1e-5 (SAM: 1e-6).  layer_norm_final_attn
 *              keeps 1e-5 and upscale_layer_norm keeps 1e-6.
 *   S2D_UP     the two high-resolution maps of the image encoder (gsr_sam2_encode's out0 and out1), the same for every point
 *              and never copied per point: feat_s0 f32 [32,4g,4g], feat_s1 f32 [64,2g,2g].  u = (conv1(stream) + bias) +
 *              feat_s1[co][2 y + dy][2 x + dx]: ONE fp32 addition after the bias's, BEFORE the statistics of the channel
 *              LayerNorm over 64 (eps 1e-6), then exact GELU, ROUNDED TO fp16.  c2 = fp16(gelu((conv2(.) + bias) + feat_s0[co]
 *              [4 y + 2 dy1 + dy2][4 x + 2 dx1 + dx2])): ONE fp32 addition after the bias's, before the GELU, in the product's
 *              epilogue.  Once per call the two maps are re-laid as f32 [T,4,64] and f32 [T,4,4,32], the layouts of the two
 *              convolutions' outputs (tap-major).
 *   S2D_HEADS  iou = 1 / (1 + expf(-z)) on the IoU head's fp32 output z (columns 1..3): the negation exact, expf precise, the
 *              addition and the quotient one fp32 rounding each.
 * SD_PROMPT holds as it is with row 1 of prompt_encoder.point_embed.weight [4,256] in point_embed.1's place.
 * Weight table of gsr_sam2_decode: gsr_sam2_dec_num_weights() (= GSR_SAM2D_W_COUNT = 119) entries.  Entries 0 ..
 * GSR_SAMD_W_COUNT - 1 are GSR_SAMD_*'s slots under Sam2Model.state_dict()'s names: o_proj in the out_proj slots, mlp.proj_in /
 * mlp.proj_out in the mlp.lin1 / mlp.lin2 slots, row 1 of prompt_encoder.point_embed.weight in GSR_SAMD_W_POINT1; then
 *   GSR_SAM2D_W_OBJ_TOKEN mask_decoder.obj_score_token.weight [1,256].
 * Entry points (caller's stream, caller's buffers, nothing synchronises):
 *   gsr_sam2_dec_t2i     gsr_sam_dec_t2i with q f32 [P,8,128] and out fp16 [P,8,128].
 *   gsr_sam2_dec_i2t     gsr_sam_dec_i2t with k, v f32 [P,8,128] and layer_norm4's eps (> 0) as an argument; the workspace of
 *                        gsr_sam2_dec_i2t_workspace_bytes.
 *   gsr_sam2_dec_upscale gsr_sam_dec_upscale with S2D_UP's feat_s0 and feat_s1; ws: gsr_sam2_dec_upscale_workspace_bytes.
 *   gsr_sam2_decode      everything: feat_s0, feat_s1 as above; emb, pe f32 [256,g,g]; points f32 [P,2]; image_size = 16 g;
 *                        low_res f32 [P,3,4g,4g]; iou f32 [P,3].  ws: gsr_sam2_decode_workspace_bytes(g, P).
 * GSR_E_INVALID before any launch: g outside 1 .. 64, P outside 1 .. 65535, image_size != 16 g, a null pointer or a null
 * table entry, a table of the wrong length, a short workspace.  The *_workspace_bytes functions return 0 for a refused shape.
 * Not built: the object-score output, boxes and mask prompts, several points per prompt, single-mask output with its dynamic
 * stability selection. */
enum { GSR_SAM2D_W_OBJ_TOKEN = GSR_SAMD_W_COUNT, GSR_SAM2D_W_COUNT = GSR_SAMD_W_COUNT + 1 };
int32_t gsr_sam2_dec_t2i(const float* q, const void* kx, const float* kpe, const void* v, int32_t P, int32_t T, int32_t shared,
                         void* out, gsr_stream_t stream);
size_t gsr_sam2_dec_i2t_workspace_bytes(int32_t P, int32_t T);
int32_t gsr_sam2_dec_i2t(const void* qx, const float* qpe, const float* k, const float* v, const void* x, int32_t P, int32_t T,
                         int32_t shared, const void* out_w, const void* out_b, const void* ln_w, const void* ln_b, float eps, void* ws,
                         size_t ws_bytes, void* x_out, gsr_stream_t stream);
size_t gsr_sam2_dec_upscale_workspace_bytes(int32_t g, int32_t P);
int32_t gsr_sam2_dec_upscale(const void* x, int32_t g, int32_t P, const void* conv1_w, const void* conv1_b, const void* ln_w,
                             const void* ln_b, const void* conv2_w, const void* conv2_b, const float* hyper, const float* feat_s0,
                             const float* feat_s1, void* ws, size_t ws_bytes, float* low_res, gsr_stream_t stream);
int32_t gsr_sam2_dec_num_weights(void);
size_t gsr_sam2_decode_workspace_bytes(int32_t g, int32_t P);
int32_t gsr_sam2_decode(int32_t g, const void* const* weights_host, int32_t n_weights, const float* feat_s0, const float* feat_s1,
                        const float* emb, const float* pe, const float* points, int32_t P, int32_t image_size, void* ws,
                        size_t ws_bytes, float* low_res, float* iou, gsr_stream_t stream);

/* ---------------------------------------------------------------- SAM2: the Hiera image encoder and its FPN neck
 * transformers' Sam2VisionModel (models/sam2/modeling_sam2.py: Sam2HieraDetModel and Sam2VisionNeck) plus what
 * Sam2Model.get_image_features / get_image_embeddings add for a still image, as inference kernels (sam2.hip; Python:
 * gaussmart_amd/sam2.py); what the reference's SAMSegmentation(sam2=True) runs inside SAM2AutomaticMaskGenerator.  Four stages;
 * stage i has the grid g_i = (image_size / 4) >> i (g_0 <= 256, a multiple of 8), the width dims[i] = 2 dims[i - 1], heads[i]
 * heads of head_dim dims[i] / heads[i] in {56, 64, 72, 80, 96}, blocks[i] blocks and the window windows[i]; the blocks are numbered
 * through the stages and those in global_host attend over the whole grid.  MLP ratio 4, erf GELU, ln_eps 1e-6, query stride
 * 2 x 2, one image per call.  EVERY weight is fp16 except no_memory_embedding; the residual stream, the LayerNorm statistics
 * and the softmax are fp32, as SV_* states for SAM.  Rules, with every rounding:
 *   HV_LINEAR  DN_LINEAR for any K that is a multiple of 8: the 16-byte loads past K give zeros, so the last chunk of 64 adds
 *              exact zeros to the k-ascending chain.  K a multiple of 64 runs DN_LINEAR's own kernels: the same bits.  Epilogues:
 *              GSR_DINO_EPI_BIAS, _GELU, _RESID, and GSR_SAM2_EPI_RESID1 (resid = resid + (acc + bias), one fp32 addition after
 *              the bias's) and GSR_SAM2_EPI_F32 (acc + bias stored as fp32).
 *   HV_EMBED   pixel_values f32 [3,S,S], normalised by the caller, ROUNDED TO fp16; the 7x7 stride-4 padding-3 convolution is
 *              a product over K = 152: k = c 49 + ky 7 + kx for k < 147 (Conv2d's own weight order), pixel (4 py + ky - 3,
 *              4 px + kx - 3), zero outside the image (only the top and left padding is ever read) and for k >= 147, where the
 *              weight rows are zero-padded too; v = acc + fp32(bias[n]), then v + fp32(pos[y][x][n]): two fp32 additions,
 *              stored as fp32 [g_0 g_0,dims[0]].  pos is an fp16 [g_0,g_0,dims[0]] table the caller computes once:
 *              F.interpolate(pos_embed, (g_0, g_0), bicubic) + pos_embed_window tiled (Sam2HieraDetModel._get_pos_embed), in
 *              fp32, ROUNDED TO fp16.
 *   block      n = DN_NORM(stream) fp16.  First block of stage i > 0 (on grid g_(i-1), width dims[i-1], window windows[i-1]):
 *              residual = HV_POOL(proj(n) + bias as fp32) on grid g_i; every other block: residual = stream.  qkv =
 *              HV_LINEAR(n, qkv.weight, qkv.bias) ROUNDED TO fp16 [T,3 dims[i]] (q of head h in columns h head_dim .., k at
 *              dims[i] + .., v at 2 dims[i] + ..); HV_ATTN; stream = residual + (attn.proj(att) + bias), one fp32 addition
 *              after the bias's; n = DN_NORM(stream); mlp.proj_in with erf GELU ROUNDED TO fp16; stream += mlp.proj_out
 *              (+ bias) likewise.
 *   HV_ATTN    qkv fp16 [g,g,3 hidden]; window w (0: the whole grid), query stride 1 or 2, heads, head_dim.  Windows are the
 *              non-overlapping w x w blocks of the grid (g a multiple of w).  stride 2: the query of pooled position (i, j) of
 *              a window is the elementwise maximum of the four fp16 q rows (2 i .. 2 i + 1, 2 j .. 2 j + 1) of that window
 *              (exact), and the output lies on the g / 2 grid at (wy w / 2 + i, wx w / 2 + j); the keys are all w w tokens of
 *              the window.  Score, fp32: t2 = ((sum_d q_d k_d) * fp32(head_dim^-1/2)) * fp32(log2 e), TWO fp32 roundings after
 *              the fp32 chain of the product; no bias terms.  Then SV_ATTN's one pass: KV tiles of 64 keys (row-major in the
 *              window), running maximum m and sum l in fp32, p = 2^(t2 - m) (v_exp_f32), l adds the UNROUNDED p, p ROUNDED TO
 *              fp16 for the P V product (fp16 v, fp32 accumulation, rescaled by 2^(m_old - m_new)); out = acc / l in fp32,
 *              ROUNDED TO fp16 [T_out,hidden].  head_dim 56 and 64 run the tile of width 64, 72 and 80 the tile of 80, 96 the
 *              tile of 96 (six k-steps); the columns of q, k and v past head_dim are zeros in the tile and never stored.  Keys
 *              past w w are never read.  A workgroup owns up to 128 queries of one head of one window and has one wave per 32
 *              of them; a window's bits depend on its own tokens only.
 *   HV_POOL    out[y][x][c] = max of the four in[2 y + a][2 x + b][c], fp32 [g,g,C] -> [g/2,g/2,C]: exact.
 *   HV_NECK    the four stage-end streams ROUNDED TO fp16; lateral_i = HV_LINEAR(stream_i, convs[3 - i].weight [D,dims[i]], its
 *              bias) stored as fp32 (the 1x1 convolutions; convs[0] belongs to the widest, lowest-resolution map); from level 2
 *              down to 0: prev_i = lateral_i + prev_(i+1)[y / 2][x / 2] (nearest, one fp32 addition) if bit i of top_down_mask
 *              is set, else lateral_i; prev_3 = lateral_3.  out0 = conv_s0(fp16(prev_0)) + bias [D/8,g_0,g_0], out1 =
 *              conv_s1(fp16(prev_1)) + bias [D/4,g_1,g_1] (HV_LINEAR over K = D, stored as fp32), out2 = prev_2 +
 *              no_memory_embedding (f32, one fp32 addition) [D,g_2,g_2].  The neck's sine position encodings are not computed:
 *              the image path does not read them.
 * Weight table of gsr_sam2_encode: a HOST array of gsr_sam2_num_weights(total blocks) DEVICE pointers to fp16 arrays (16-byte
 * aligned) unless stated, in this order (names: Sam2Model.state_dict() under vision_encoder.):
 *   GSR_SAM2_W_PATCH_W backbone.patch_embed.projection.weight as [dims[0],152] (147 columns and 5 zeros); _PATCH_B its bias; _POS
 *   the position table of HV_EMBED;
 *   per block b at GSR_SAM2_W_BLOCK0 + GSR_SAM2_W_PER_BLOCK b + GSR_SAM2_B_*: backbone.blocks.b.layer_norm1.weight, .bias,
 *   attn.qkv.weight [3 dim_out,dim], .bias, attn.proj.weight, .bias, layer_norm2.weight, .bias, mlp.proj_in.weight, .bias,
 *   mlp.proj_out.weight, .bias, proj.weight [dim_out,dim], .bias (the last two NULL unless the block starts a stage);
 *   last (GSR_SAM2_W_NECK entries; gsr_sam2_neck takes these alone): for stage i = 0 .. 3 neck.convs.(3 - i).weight [D,dims[i]]
 *   and .bias; mask_decoder.conv_s0.weight [D/8,D], .bias; mask_decoder.conv_s1.weight [D/4,D], .bias; no_memory_embedding
 *   F32 [D].
 * Entry points (caller's stream, caller's buffers, nothing synchronises):
 *   gsr_sam2_embed / _linear / _attn / _pool / _neck : one rule each; ws from the *_workspace_bytes beside it.  _neck:
 *       streams_host is a HOST array of the four DEVICE streams f32 [g_i g_i,dims[i]]; the outputs are out0, out1, out2 above.
 *   gsr_sam2_encode : pixel_values f32 [3,S,S] -> out0, out1, out2; ws: gsr_sam2_workspace_bytes(cfg) (0 when refused).
 * Refused with GSR_E_INVALID before anything is launched, with a message: a grid that is not a multiple of its window (a
 * stage start: the previous grid and the previous window), a query stride other than 2 x 2, a stage that does not double its
 * width, a global block that starts a stage, a head_dim that is not built, a null required pointer, a short workspace, a
 * weight table of the wrong length. */
typedef struct GsrSam2Config {
    int32_t image_size, fpn_hidden, top_down_mask, num_global;
    int32_t blocks[4], dims[4], heads[4], windows[4];
    int32_t query_stride[2];
    float ln_eps;
    const int32_t* global_host;     /* HOST array of num_global block numbers */
} GsrSam2Config;
enum { GSR_SAM2_EPI_RESID1 = 4, GSR_SAM2_EPI_F32 = 5 };
enum { GSR_SAM2_W_PATCH_W = 0, GSR_SAM2_W_PATCH_B, GSR_SAM2_W_POS, GSR_SAM2_W_BLOCK0 };
enum { GSR_SAM2_B_NORM1_W = 0, GSR_SAM2_B_NORM1_B, GSR_SAM2_B_QKV_W, GSR_SAM2_B_QKV_B, GSR_SAM2_B_OUT_W, GSR_SAM2_B_OUT_B,
       GSR_SAM2_B_NORM2_W, GSR_SAM2_B_NORM2_B, GSR_SAM2_B_MLP1_W, GSR_SAM2_B_MLP1_B, GSR_SAM2_B_MLP2_W, GSR_SAM2_B_MLP2_B,
       GSR_SAM2_B_PROJ_W, GSR_SAM2_B_PROJ_B, GSR_SAM2_W_PER_BLOCK };
enum { GSR_SAM2_W_NECK = 13 };
size_t gsr_sam2_embed_workspace_bytes(int32_t image_size);
int32_t gsr_sam2_embed(const float* pixel_values, int32_t image_size, int32_t embed, const void* patch_w, const void* patch_b,
                       const void* pos_table, void* ws, size_t ws_bytes, float* out, gsr_stream_t stream);
int32_t gsr_sam2_linear(const void* x, const void* w, const void* bias, const void* lambda, int64_t M, int32_t K, int32_t N,
                        int32_t epilogue, void* out, gsr_stream_t stream);
int32_t gsr_sam2_attn(const void* qkv, int32_t g, int32_t window, int32_t query_stride, int32_t heads, int32_t head_dim, void* out,
                      gsr_stream_t stream);
int32_t gsr_sam2_pool(const float* x, int32_t g, int32_t channels, float* out, gsr_stream_t stream);
size_t gsr_sam2_neck_workspace_bytes(int32_t g0, int32_t embed, int32_t fpn_hidden);
int32_t gsr_sam2_neck(const float* const* streams_host, int32_t g0, int32_t embed, int32_t fpn_hidden, int32_t top_down_mask,
                      const void* const* neck_weights_host, void* ws, size_t ws_bytes, float* out0, float* out1, float* out2,
                      gsr_stream_t stream);
size_t gsr_sam2_workspace_bytes(const GsrSam2Config* cfg);
int32_t gsr_sam2_num_weights(int32_t total_blocks);
int32_t gsr_sam2_encode(const GsrSam2Config* cfg, const void* const* weights_host, int32_t n_weights, const float* pixel_values,
                        void* ws, size_t ws_bytes, float* out0, float* out1, float* out2, gsr_stream_t stream);

/* ---------------------------------------------------------------- camera clustering (step 1 of identification/main.py)
 * The reference picks the views it segments by k-means over the camera centres (identification/clustering_cameras.py):
 * scikit-learn's KMeans for every k from 3 to 15 with n_init = 10, 130 independent fits of at most a few hundred points in three
 * dimensions.  The initial centres are drawn on the host from scikit-learn's random stream (gaussmart_amd/camera_select.py);
 * the Lloyd iterations of ALL fits are one launch of gsr_cam_lloyd, one workgroup per fit, the points in LDS.  fp64 throughout,
 * no fused multiply-add, and every sum in a stated order, so that camera_select.lloyd_batch_host (numpy) gives the same bits in
 * labels, centres, inertia, n_iter and status.
 *   CK_LLOYD   x f64 [n,3] (the caller has subtracted the mean), per fit f: k_f in 1 .. GSR_CK_KMAX and centres0[f] f64
 *              [GSR_CK_KMAX,3] (rows >= k_f are not read).  d(i, c) = ((x_i0 - c_0)^2 + (x_i1 - c_1)^2) + (x_i2 - c_2)^2, the
 *              three squares summed left to right.  One iteration, from the centres C:
 *                label_i = the lowest c at which d(i, c) is smallest (a later c wins only with a strictly smaller d);
 *                for every cluster c and every chunk of GSR_CK_CHUNK consecutive indices (chunk j holds indices 64 j ..
 *                  min(n, 64 j + 64) - 1): the sums of x_0, x_1, x_2 and the member count over the chunk's members of c, each
 *                  started at +0 and added in ascending index; then, started at +0 again, the chunks added in ascending j;
 *                a cluster without members: status = 1 and the fit ENDS with this iteration's labels, the centres C unmoved,
 *                  n_iter counting this iteration (the caller redoes the fit on the host, which relocates such a centre as
 *                  scikit-learn does);
 *                new_c = sum / count, one division per axis; shift = sum over c ascending, from +0, of d(new_c, C_c);
 *                the centres become the new ones; then, in this order: labels equal to the previous iteration's (the first
 *                  iteration compares with "none") -> stop (strict convergence); shift <= tol -> stop; max_iter iterations
 *                  done -> stop.  After either of the last two stops the labels are computed once more against the final
 *                  centres.
 *              inertia = per chunk, from +0 in ascending index, the sum of d(i, centre of label_i); then the chunks from +0 in
 *              ascending order.  n_iter = iterations run.  This is scikit-learn 1.7's _kmeans_single_lloyd with the distances
 *              written out instead of expanded, without its relocation of empty clusters and with the shift's square roots
 *              (squared again there) left out.
 * Outputs per fit: labels i32 [n], centres f64 [GSR_CK_KMAX,3] (rows >= k_f are 0), inertia f64, n_iter i32, status i32 (0 done,
 * 1 a cluster lost all members, 2 k_f outside 1 .. GSR_CK_KMAX: labels -1, nothing iterated).  k, like every array, is DEVICE
 * memory; the caller's stream, nothing synchronises.  No workspace is needed up to the cap (gsr_cam_lloyd_workspace_bytes is 0
 * and ws may be NULL); the arguments stay so that a route through global memory would not change the signature.
 * Refused before anything is launched, with a message: n < 1, n_fits < 0, max_iter < 1, tol < 0 or NaN, a null array (all
 * GSR_E_INVALID); n > GSR_CK_MAX_CAMERAS (GSR_E_UNSUPPORTED; 24 bytes of LDS per point, 96 KiB of the CU's 160 KiB at the cap,
 * beside 32 KiB of chunk sums: the message names the host route, camera_select.lloyd_batch_host). */
#define GSR_CK_KMAX 16
#define GSR_CK_CHUNK 64
#define GSR_CK_MAX_CAMERAS 4096
size_t gsr_cam_lloyd_workspace_bytes(int32_t n, int32_t n_fits);
int32_t gsr_cam_lloyd(const double* x, int32_t n, const double* centres0, const int32_t* k, int32_t n_fits, double tol,
                      int32_t max_iter, int32_t* labels, double* centres, double* inertia, int32_t* n_iter, int32_t* status,
                      void* ws, size_t ws_bytes, gsr_stream_t stream);

/* Opt-in per-kernel timing with HIP events on the launch stream (bench.py's roofline figures).
 * `mask`: bit k enables kernel k in the order of the names below (-1 = all, 0 = off); timing only
 * the few big kernels keeps the event overhead out of the measured step.
 * Kernel names: "preprocess_fwd", "sort_hist", "sort_scatter", "scan", "emit_instances",
 * "finalize_bins", "render_fwd", "render_bwd", "preprocess_bwd", "knn", "loss_fwd", "loss_bwd", "regularizer_fwd", "regularizer_bwd", "adam". */
void gsr_profile_enable(int32_t mask);
void gsr_profile_reset(void);
int32_t gsr_profile_read(const char* kernel, double* total_ms, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_ */
