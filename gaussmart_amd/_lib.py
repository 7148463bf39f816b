"""ctypes binding of libgsr_hip.so (C ABI: include/gsr.h).

There is deliberately no fallback: if the HIP library has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C gaussmart_amd/csrc`) loading
raises, and every operator in this package raises with it.
"""
import ctypes as C
import os
import threading

# torch ships its own libamdhip64.so.7; it must be the HIP runtime this process uses (device
# pointers and streams come from torch), so it has to be loaded BEFORE libgsr_hip.so, whose
# DT_NEEDED entry then binds to the already-loaded SONAME instead of /opt/rocm's copy.
import torch  # noqa: F401  (import order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSR_LIB_PATH: developer aid for same-box A/B runs of two builds of the library (scripts/ab_builds.sh)
LIB_PATH = os.environ.get("GSR_LIB_PATH") or os.path.join(_HERE, "lib", "libgsr_hip.so")
ABI_VERSION = 18
GSR_LPIPS_ALEX, GSR_LPIPS_VGG = 0, 1
GSR_DINO_EPI_BIAS, GSR_DINO_EPI_GELU, GSR_DINO_EPI_RESID = 0, 1, 2
GSR_DINO_W_LAYER0, GSR_DINO_W_PER_LAYER = 4, 18      # include/gsr.h: the weight table of gsr_dino_forward
GSR_SAM_W_LAYER0, GSR_SAM_W_PER_LAYER, GSR_SAM_W_NECK = 3, 14, 6     # include/gsr.h: the weight table of gsr_sam_encode
GSR_SAM2_EPI_RESID1, GSR_SAM2_EPI_F32 = 4, 5
GSR_SAM2_W_BLOCK0, GSR_SAM2_W_PER_BLOCK, GSR_SAM2_W_NECK = 3, 14, 13     # include/gsr.h: the weight table of gsr_sam2_encode
# include/gsr.h: the weight table of gsr_sam_decode (head, per two-way layer, final attention, up-scaling, hypernetworks, IoU head)
GSR_SAMD_W_LAYER0, GSR_SAMD_W_PER_LAYER, GSR_SAMD_W_FINAL, GSR_SAMD_W_UP, GSR_SAMD_W_HYPER, GSR_SAMD_W_IOU, GSR_SAMD_W_COUNT = 6, 36, 78, 88, 94, 112, 118
# include/gsr.h: the weight table of gsr_sam2_decode is gsr_sam_decode's under SAM2's names plus the object-score token
GSR_SAMD_W_POINT1 = 1
GSR_SAM2D_W_OBJ_TOKEN, GSR_SAM2D_W_COUNT = 118, 119
GSR_CK_KMAX, GSR_CK_CHUNK, GSR_CK_MAX_CAMERAS = 16, 64, 4096     # include/gsr.h: CK_LLOYD (gaussmart_amd/camera_select.py)

GSR_BUF_GEOM, GSR_BUF_BINNING, GSR_BUF_IMAGE, GSR_BUF_SCRATCH, GSR_BUF_SCRATCH2 = range(5)
GSR_BUF_SYNC_SH = 100     # not a buffer: "the SH colour pass is about to be enqueued" (GSR_FLAG_DEFER_COLOR)
GSR_BUF_COLOR_STREAM = 101   # not a buffer: "a second stream for the SH colour pass?" (GSR_FLAG_DEFER_COLOR); 0 = none
GSR_FLAG_CLAMP_PASSTHROUGH = 1
GSR_FLAG_FILTER_DEPTH_GRAD = 2
GSR_FLAGS_UPSTREAM = 3
GSR_FLAG_DEBUG_NO_CULL = 4
GSR_FLAG_RAW_PARAMS = 8
GSR_FLAG_DEFER_COLOR = 16
GSR_FLAG_DEBUG_RECT_CULL_ONLY = 64
GSR_FLAG_COLOR_CACHED = 256      # shs + colour cache of this view (gsr_adam_sh_factored_next): no SH colour pass
GSR_FLAG_FORWARD_ONLY = 128      # inference: keep nothing for a backward (no touch words, no per-pixel state)
GSR_FLAG_AABB_GRAD_CUTOFF1 = 512  # recalled quirk 3: centre gradient chained with weights (1, 1, -1) (include/gsr.h)
GSR_FLAG_NO_DIST_MEDIAN = 4096   # forward + backward: distortion and median depth are not consumed (lambda_dist = 0, depth_ratio = 0)
GSR_FLAG_COLOR_ONLY = 2048       # forward: allmap is not consumed (no regularizer active): not accumulated, not written
GSR_FLAG_NO_SURFACE_GRAD = 1024  # backward: dL/dallmap is identically zero (no regularizer active): 4-part-record kernel
GSR_FLAG_TIGHT_TILES = 8192      # forward: tile rects clipped to the tiles the alpha box reaches (same results, shorter lists)
GSR_FLAG_FACTORED_SH_GRAD = 32   # backward writes the masked colour gradient [N,3] instead of the SH gradient arrays

KERNEL_NAMES = ("preprocess_fwd", "sort_hist", "sort_scatter", "scan", "emit_instances",
                "finalize_bins", "render_fwd", "render_bwd", "preprocess_bwd", "knn", "loss_fwd", "loss_bwd",
                "regularizer_fwd", "regularizer_bwd", "adam")


class GsrView(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
                ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32), ("channels", C.c_int32),
                ("flags", C.c_uint32),
                ("bg", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p),
                ("campos", C.c_void_p)]


class GsrGaussians(C.Structure):
    _fields_ = [("count", C.c_int32),
                ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
                ("opacities", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p),
                ("transmat_precomp", C.c_void_p), ("shs_rest", C.c_void_p)]


class GsrForwardOut(C.Structure):
    _fields_ = [("out_color", C.c_void_p), ("out_allmap", C.c_void_p), ("radii", C.c_void_p),
                ("num_rendered", C.c_int32),
                ("geom", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p)]


class GsrGrads(C.Structure):
    _fields_ = [("dL_dmeans3D", C.c_void_p), ("dL_dmeans2D", C.c_void_p), ("dL_dopacity", C.c_void_p),
                ("dL_dshs", C.c_void_p), ("dL_dcolors", C.c_void_p), ("dL_dscales", C.c_void_p),
                ("dL_drotations", C.c_void_p), ("dL_dtransmat", C.c_void_p), ("dL_dshs_rest", C.c_void_p)]


class GsrRowScanJob(C.Structure):
    """include/gsr.h: the scan of the backward's row counts, offered to kernels between the forward and the backward."""
    _fields_ = [("counts", C.c_void_p), ("slot_off", C.c_void_p), ("workspace", C.c_void_p), ("n", C.c_int64),
                ("stage", C.c_int32)]


class GsrTsdfVolume(C.Structure):
    """include/gsr.h: a block-sparse TSDF volume in caller-owned device memory (gaussmart_amd/tsdf.py)."""
    _fields_ = [("voxel_size", C.c_float), ("sdf_trunc", C.c_float),
                ("block_lo", C.c_int32 * 3), ("block_hi", C.c_int32 * 3),
                ("block_index", C.c_void_p), ("pool", C.c_void_p), ("pool_blocks", C.c_int64), ("n_alloc", C.c_int64),
                ("n_views", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class GsrUnbView(C.Structure):
    """include/gsr.h: one view of the unbounded field's device table (gaussmart_amd/mesh_unbounded.py)."""
    _fields_ = [("col_x", C.c_float * 4), ("col_y", C.c_float * 4), ("col_w", C.c_float * 4),
                ("depth", C.c_void_p), ("rgb", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32)]


class GsrSegView(C.Structure):
    """include/gsr.h: one view of the segment assignment (gaussmart_amd/segment_init.py)."""
    _fields_ = [("kind", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("n_masks", C.c_int32),
                ("label_offset", C.c_int64), ("world_mat", C.c_double * 16), ("scale_mat", C.c_double * 16),
                ("camera_mat", C.c_double * 9), ("cam_pos", C.c_double * 3), ("img_w", C.c_double), ("img_h", C.c_double)]


class GsrSamConfig(C.Structure):
    """include/gsr.h: the run-time shape of SAM's image encoder (gaussmart_amd/sam.py); the two pointers are host arrays."""
    _fields_ = [("hidden", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32), ("layers", C.c_int32),
                ("mlp_dim", C.c_int32), ("output_channels", C.c_int32), ("image_size", C.c_int32), ("ln_eps", C.c_float),
                ("window_host", C.POINTER(C.c_int32)), ("rel_rows_host", C.POINTER(C.c_int32))]


class GsrSam2Config(C.Structure):
    """include/gsr.h: the run-time shape of SAM2's Hiera encoder and FPN neck (gaussmart_amd/sam2.py); global_host is a host array."""
    _fields_ = [("image_size", C.c_int32), ("fpn_hidden", C.c_int32), ("top_down_mask", C.c_int32), ("num_global", C.c_int32),
                ("blocks", C.c_int32 * 4), ("dims", C.c_int32 * 4), ("heads", C.c_int32 * 4), ("windows", C.c_int32 * 4),
                ("query_stride", C.c_int32 * 2), ("ln_eps", C.c_float), ("global_host", C.POINTER(C.c_int32))]


class GsrDinoConfig(C.Structure):
    """include/gsr.h: the run-time shape of the DINOv3 ViT encoder (gaussmart_amd/dino.py)."""
    _fields_ = [("hidden", C.c_int32), ("heads", C.c_int32), ("layers", C.c_int32), ("intermediate", C.c_int32),
                ("registers", C.c_int32), ("rope_theta", C.c_float), ("ln_eps", C.c_float),
                ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3)]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t)

_lock = threading.Lock()
_lib = None


class GsrError(RuntimeError):
    pass


def lib():
    """The loaded library (loads on first use).  Raises if it is missing or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GsrError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C gaussmart_amd/csrc`). "
                "gaussmart_amd has no CPU fallback.")
        hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(hip_rt):
            C.CDLL(hip_rt, mode=C.RTLD_GLOBAL)
        L = C.CDLL(LIB_PATH)
        L.gsr_abi_version.restype = C.c_int32
        L.gsr_last_error.restype = C.c_char_p
        if L.gsr_abi_version() != ABI_VERSION:
            raise GsrError(f"libgsr_hip.so ABI {L.gsr_abi_version()} != expected {ABI_VERSION}; rebuild")
        L.gsr_forward.restype = C.c_int32
        L.gsr_forward.argtypes = [C.POINTER(GsrView), C.POINTER(GsrGaussians), C.POINTER(GsrForwardOut),
                                  ALLOC_FN, C.c_void_p, C.c_void_p]
        L.gsr_backward.restype = C.c_int32
        L.gsr_backward.argtypes = [C.POINTER(GsrView), C.POINTER(GsrGaussians), C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(GsrGrads), ALLOC_FN, C.c_void_p, C.c_void_p]
        L.gsr_buffer_field.restype = C.c_int32
        L.gsr_buffer_field.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.gsr_knn3_workspace_bytes.restype = C.c_size_t
        L.gsr_knn3_workspace_bytes.argtypes = [C.c_int32]
        L.gsr_knn3.restype = C.c_int32
        L.gsr_knn3.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.gsr_sort_workspace_bytes.restype = C.c_size_t
        L.gsr_sort_workspace_bytes.argtypes = [C.c_int32]
        L.gsr_sort_pairs_u32.restype = C.c_int32
        L.gsr_sort_pairs_u32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.gsr_loss_num_partials.restype = C.c_int32
        L.gsr_loss_num_partials.argtypes = [C.c_int32, C.c_int32]
        L.gsr_loss_forward.restype = C.c_int32
        L.gsr_loss_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        L.gsr_loss_backward.restype = C.c_int32
        L.gsr_loss_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsr_regularizer_forward.restype = C.c_int32
        L.gsr_regularizer_forward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_float,
                                              C.c_void_p, C.c_void_p]
        L.gsr_regularizer_backward.restype = C.c_int32
        L.gsr_regularizer_backward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_float,
                                               C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        # (every symbol below is part of ABI 5 / 6 / 7: a library without one of them fails the version check above, so there are
        # no per-symbol guards)
        L.gsr_regularizer_backward_partials.restype = C.c_int32
        L.gsr_regularizer_backward_partials.argtypes = L.gsr_regularizer_backward.argtypes[:-1] + [C.c_void_p, C.c_void_p]
        L.gsr_surface_maps_forward.restype = C.c_int32
        L.gsr_surface_maps_forward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                               C.c_float, C.c_void_p, C.c_void_p]
        L.gsr_surface_maps_backward.restype = C.c_int32
        L.gsr_surface_maps_backward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsr_row_scan_job.restype = C.c_int32
        L.gsr_row_scan_job.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(GsrRowScanJob)]
        L.gsr_backward_with_job.restype = C.c_int32
        L.gsr_backward_with_job.argtypes = L.gsr_backward.argtypes[:10] + [C.POINTER(GsrRowScanJob)] + \
            L.gsr_backward.argtypes[10:]
        L.gsr_loss_forward_job.restype = C.c_int32
        L.gsr_loss_forward_job.argtypes = L.gsr_loss_forward.argtypes[:-1] + [C.POINTER(GsrRowScanJob), C.c_void_p, C.c_void_p]
        L.gsr_loss_backward_finish.restype = C.c_int32
        L.gsr_loss_backward_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                               C.c_float, C.c_void_p, C.POINTER(GsrRowScanJob), C.c_void_p]
        L.gsr_objective_finish.restype = C.c_int32
        L.gsr_objective_finish.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_float,
                                           C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.gsr_adam_step.restype = C.c_int32
        L.gsr_adam_step.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.gsr_adam_step_keep.restype = C.c_int32
        L.gsr_adam_step_keep.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), C.c_double, C.c_double, C.c_double, C.POINTER(C.c_void_p),
                                         C.c_void_p]
        L.gsr_adam_sh_factored.restype = C.c_int32
        L.gsr_adam_sh_factored.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_int32, C.c_float,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                           C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.gsr_adam_sh_factored_next.restype = C.c_int32
        L.gsr_adam_sh_factored_next.argtypes = L.gsr_adam_sh_factored.argtypes[:-1] + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                                                       C.c_void_p, C.c_void_p]
        L.gsr_compact_workspace_bytes.restype = C.c_size_t
        L.gsr_compact_workspace_bytes.argtypes = [C.c_int64]
        L.gsr_compact_plan.restype = C.c_int32
        L.gsr_compact_plan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.c_void_p]
        L.gsr_compact_apply.restype = C.c_int32
        L.gsr_compact_apply.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                        C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsr_densify_stats.restype = C.c_int32
        L.gsr_densify_stats.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        V = C.POINTER(GsrTsdfVolume)
        L.gsr_tsdf_sizes.restype = C.c_int32
        L.gsr_tsdf_sizes.argtypes = [V, C.POINTER(C.c_int64), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.gsr_tsdf_touch.restype = C.c_int32
        L.gsr_tsdf_touch.argtypes = [V, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int64), C.c_void_p]
        L.gsr_tsdf_integrate.restype = C.c_int32
        L.gsr_tsdf_integrate.argtypes = [V, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), C.c_float, C.c_int64, C.c_void_p]
        L.gsr_mcubes_workspace_bytes.restype = C.c_size_t
        L.gsr_mcubes_workspace_bytes.argtypes = [C.c_int64]
        L.gsr_mcubes_count.restype = C.c_int32
        L.gsr_mcubes_count.argtypes = [V, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        L.gsr_mcubes_emit.restype = C.c_int32
        L.gsr_mcubes_emit.argtypes = [V, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsr_depth_aabb.restype = C.c_int32
        L.gsr_depth_aabb.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.c_float, C.c_void_p, C.c_void_p]
        L.gsr_mesh_clusters_workspace_bytes.restype = C.c_size_t
        L.gsr_mesh_clusters_workspace_bytes.argtypes = [C.c_int64]
        L.gsr_mesh_filter_workspace_bytes.restype = C.c_size_t
        L.gsr_mesh_filter_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
        L.gsr_mesh_clusters.restype = C.c_int32
        L.gsr_mesh_clusters.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]
        L.gsr_mesh_filter_count.restype = C.c_int32
        L.gsr_mesh_filter_count.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        L.gsr_mesh_filter_emit.restype = C.c_int32
        L.gsr_mesh_filter_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsr_mask_dilate_workspace_bytes.restype = C.c_size_t
        L.gsr_mask_dilate_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.gsr_mask_dilate_disk.restype = C.c_int32
        L.gsr_mask_dilate_disk.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p]
        L.gsr_mesh_cull_workspace_bytes.restype = C.c_size_t
        L.gsr_mesh_cull_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32]
        L.gsr_mesh_cull_count.restype = C.c_int32
        L.gsr_mesh_cull_count.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        L.gsr_mesh_cull_emit.restype = C.c_int32
        L.gsr_mesh_cull_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsr_mesh_depth_workspace_bytes.restype = C.c_size_t
        L.gsr_mesh_depth_workspace_bytes.argtypes = [C.c_int64, C.c_int32]
        L.gsr_mesh_depth_render.restype = C.c_int32
        L.gsr_mesh_depth_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.gsr_mesh_vis_count.restype = C.c_int32
        L.gsr_mesh_vis_count.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
        L.gsr_mesh_vis_workspace_bytes.restype = C.c_size_t
        L.gsr_mesh_vis_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
        L.gsr_mesh_vis_compact_count.restype = C.c_int32
        L.gsr_mesh_vis_compact_count.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                                 C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        L.gsr_mesh_vis_emit.restype = C.c_int32
        L.gsr_mesh_vis_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        vp, i64, f64, sz, fp = C.c_void_p, C.c_int64, C.c_double, C.c_size_t, C.POINTER(C.c_float)
        for name, res, args in (
                ("gsr_mesh_sample_workspace_bytes", sz, [i64]),
                ("gsr_mesh_sample_count", C.c_int32, [vp, vp, i64, i64, f64, vp, sz, C.POINTER(i64), vp]),
                ("gsr_mesh_sample_emit", C.c_int32, [vp, vp, i64, i64, f64, vp, sz, vp, vp]),
                ("gsr_points_gather", C.c_int32, [vp, i64, vp, i64, vp, vp]),
                ("gsr_points_search_workspace_bytes", sz, [i64, i64]),
                ("gsr_points_downsample", C.c_int32, [vp, i64, f64, vp, sz, vp, C.POINTER(C.c_int32), vp]),
                ("gsr_points_nearest", C.c_int32, [vp, i64, vp, i64, f64, vp, sz, vp, vp, vp]),
                ("gsr_points_obs_workspace_bytes", sz, [i64]),
                ("gsr_points_obs_filter_count", C.c_int32, [vp, i64, vp, vp, vp, f64, f64, vp, sz, vp, vp, C.POINTER(i64),
                                                            C.POINTER(i64), vp]),
                ("gsr_points_obs_filter_emit", C.c_int32, [vp, i64, vp, sz, vp, vp, vp]),
                ("gsr_points_plane_filter", C.c_int32, [vp, i64, vp, vp, vp]),
                ("gsr_dist_mean_workspace_bytes", sz, [i64]),
                ("gsr_dist_mean", C.c_int32, [vp, i64, vp, sz, vp, vp, vp]),
                ("gsr_mesh_face_centres", C.c_int32, [vp, vp, i64, i64, vp, vp]),
                ("gsr_points_transform", C.c_int32, [vp, i64, vp, vp, vp]),
                ("gsr_points_crop_polygon", C.c_int32, [vp, i64, C.c_int32, f64, f64, vp, C.c_int32, vp, vp]),
                ("gsr_points_voxel_workspace_bytes", sz, [i64]),
                ("gsr_points_voxel_count", C.c_int32, [vp, i64, f64, vp, sz, C.POINTER(i64), vp]),
                ("gsr_points_voxel_emit", C.c_int32, [vp, i64, f64, vp, sz, vp, vp, vp]),
                ("gsr_icp_sums_workspace_bytes", sz, [i64]),
                ("gsr_icp_sums", C.c_int32, [vp, i64, vp, i64, vp, vp, vp, vp, sz, vp, vp]),
                ("gsr_dist_score_workspace_bytes", sz, [C.c_int32]),
                ("gsr_dist_score", C.c_int32, [vp, i64, vp, C.c_int32, f64, vp, sz, vp, vp, vp]),
                ("gsr_seg_hull_distance", C.c_int32, [vp, C.c_int32, i64, vp, C.c_int32, vp, vp]),
                ("gsr_seg_mean_std_workspace_bytes", sz, [i64]),
                ("gsr_seg_mean_std", C.c_int32, [vp, i64, vp, vp, sz, vp]),
                ("gsr_seg_label_map", C.c_int32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]),
                ("gsr_seg_views_workspace_bytes", sz, [C.c_int32]),
                ("gsr_seg_views_prepare", C.c_int32, [vp, C.c_int32, i64, C.POINTER(GsrSegView), C.c_int32, i64, vp, sz, vp]),
                ("gsr_seg_project", C.c_int32, [vp, C.c_int32, i64, vp, sz, C.c_int32, C.c_int32, vp, vp, vp]),
                ("gsr_seg_assign", C.c_int32, [vp, C.c_int32, i64, vp, sz, C.c_int32, vp, vp, vp]),
                ("gsr_seg_stats", C.c_int32, [vp, vp, vp, vp, i64, C.c_int32, vp, vp, vp]),
                ("gsr_seg_augment_emit", C.c_int32, [vp, vp, C.c_int32, vp, vp, vp, vp, i64, vp, vp, vp, vp]),
                ("gsr_unb_lattice_size", C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
                ("gsr_unb_points", C.c_int32, [vp, C.c_int32, vp, i64, fp, C.c_float, C.c_float, C.c_int32, vp, vp, vp]),
                ("gsr_unb_lattice_box", C.c_int32, [vp, C.c_int32, f64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_int32), fp, C.c_float, C.c_float, vp, vp]),
                ("gsr_unb_block_flags", C.c_int32, [vp, C.c_int32, f64, C.c_int32, C.c_int32, fp, C.c_float, C.c_float, vp, vp]),
                ("gsr_unb_alloc", C.c_int32, [V, C.c_int32, C.c_int32, vp, vp]),
                ("gsr_unb_fill", C.c_int32, [V, vp, C.c_int32, f64, C.c_int32, C.c_int32, fp, C.c_float, C.c_float, vp]),
                ("gsr_unb_finish", C.c_int32, [vp, i64, f64, C.c_int32, C.c_int32, fp, C.c_float, C.c_float, vp]),
                ("gsr_lpips_conv", C.c_int32, [vp, vp, vp] + [C.c_int32] * 9 + [vp, vp]),
                ("gsr_lpips_pool", C.c_int32, [vp, i64, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
                ("gsr_lpips_head_workspace_bytes", sz, []),
                ("gsr_lpips_head", C.c_int32, [vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, sz, vp, vp]),
                ("gsr_lpips_workspace_bytes", sz, [C.c_int32, C.c_int32, C.c_int32]),
                ("gsr_lpips_forward", C.c_int32, [C.c_int32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, C.c_int32,
                                                  C.c_int32, C.c_int32, vp, sz, vp, vp]),
                ("gsr_frame_to_u8", C.c_int32, [vp] + [C.c_int32] * 4 + [vp, vp]),
                ("gsr_frame_order_stats_workspace_bytes", sz, [i64]),
                ("gsr_frame_order_stats", C.c_int32, [vp, i64, C.POINTER(i64), C.c_int32, fp, vp, sz, vp]),
                ("gsr_frame_depth_vis", C.c_int32, [vp, C.c_int32, C.c_int32, C.c_int32, f64, f64, vp, vp, vp, vp]),
                ("gsr_frame_sobel", C.c_int32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
                ("gsr_frame_minmax", C.c_int32, [vp, i64, vp, vp]),
                ("gsr_frame_colormap", C.c_int32, [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]),
                ("gsr_dino_embed_workspace_bytes", sz, [C.c_int32] * 3),
                ("gsr_dino_embed", C.c_int32, [C.POINTER(GsrDinoConfig), vp, vp] + [C.c_int32] * 3 + [vp] * 5 + [sz, vp, vp]),
                ("gsr_dino_norm", C.c_int32, [vp, i64, C.c_int32, i64, vp, vp, C.c_float, C.c_int32, vp, vp]),
                ("gsr_dino_linear", C.c_int32, [vp, vp, vp, vp, i64, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
                ("gsr_dino_rope", C.c_int32, [vp, vp] + [C.c_int32] * 5 + [C.c_float, vp]),
                ("gsr_dino_attn", C.c_int32, [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
                ("gsr_dino_workspace_bytes", sz, [C.POINTER(GsrDinoConfig)] + [C.c_int32] * 3),
                ("gsr_dino_num_weights", C.c_int32, [C.c_int32]),
                ("gsr_dino_forward", C.c_int32, [C.POINTER(GsrDinoConfig), C.POINTER(vp), C.c_int32, vp, vp] + [C.c_int32] * 3 +
                 [vp, sz, vp, vp, vp]),
                ("gsr_dino_cosine", C.c_int32, [vp, vp, C.c_int32, C.c_float, vp, vp]),
                ("gsr_sam_embed_workspace_bytes", sz, [C.c_int32]),
                ("gsr_sam_embed", C.c_int32, [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, sz, vp, vp]),
                ("gsr_sam_attn_workspace_bytes", sz, [C.c_int32] * 3),
                ("gsr_sam_attn", C.c_int32, [vp] * 4 + [C.c_int32] * 5 + [vp, sz, vp, vp]),
                ("gsr_sam_neck_workspace_bytes", sz, [C.c_int32] * 3),
                ("gsr_sam_neck", C.c_int32, [vp] + [C.c_int32] * 3 + [vp] * 7 + [sz, vp, vp]),
                ("gsr_sam_workspace_bytes", sz, [C.POINTER(GsrSamConfig)]),
                ("gsr_sam_num_weights", C.c_int32, [C.c_int32]),
                ("gsr_sam_encode", C.c_int32, [C.POINTER(GsrSamConfig), C.POINTER(vp), C.c_int32, vp, vp, sz, vp, vp]),
                ("gsr_sam_mask_score", C.c_int32, [vp] + [C.c_int32] * 6 + [C.c_float, C.c_float, vp, vp, vp, vp]),
                ("gsr_sam_mask_emit", C.c_int32, [vp] + [C.c_int32] * 6 + [C.c_float, vp, C.c_int32, vp, vp]),
                ("gsr_sam_nms_workspace_bytes", sz, [C.c_int32]),
                ("gsr_sam_nms", C.c_int32, [vp, vp, vp, C.c_int32, C.c_float, vp, sz, vp, vp, vp]),
                ("gsr_sam_dec_prompt", C.c_int32, [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]),
                ("gsr_sam_dec_t2i", C.c_int32, [vp] * 4 + [C.c_int32] * 3 + [vp, vp]),
                ("gsr_sam_dec_i2t_workspace_bytes", sz, [C.c_int32] * 2),
                ("gsr_sam_dec_i2t", C.c_int32, [vp] * 5 + [C.c_int32] * 3 + [vp] * 5 + [sz, vp, vp]),
                ("gsr_sam_dec_upscale_workspace_bytes", sz, [C.c_int32] * 2),
                ("gsr_sam_dec_upscale", C.c_int32, [vp, C.c_int32, C.c_int32] + [vp] * 8 + [sz, vp, vp]),
                ("gsr_sam_dec_num_weights", C.c_int32, []),
                ("gsr_sam_decode_workspace_bytes", sz, [C.c_int32] * 2),
                ("gsr_sam_decode", C.c_int32, [C.c_int32, C.POINTER(vp), C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, sz, vp, vp, vp]),
                ("gsr_sam_mask_score_direct", C.c_int32, [vp] + [C.c_int32] * 4 + [C.c_float, C.c_float, vp, vp, vp, vp]),
                ("gsr_sam_mask_emit_direct", C.c_int32, [vp] + [C.c_int32] * 4 + [C.c_float, vp, C.c_int32, vp, vp]),
                ("gsr_sam2_embed_workspace_bytes", sz, [C.c_int32]),
                ("gsr_sam2_embed", C.c_int32, [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, sz, vp, vp]),
                ("gsr_sam2_linear", C.c_int32, [vp, vp, vp, vp, i64, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
                ("gsr_sam2_attn", C.c_int32, [vp] + [C.c_int32] * 5 + [vp, vp]),
                ("gsr_sam2_pool", C.c_int32, [vp, C.c_int32, C.c_int32, vp, vp]),
                ("gsr_sam2_neck_workspace_bytes", sz, [C.c_int32] * 3),
                ("gsr_sam2_neck", C.c_int32, [C.POINTER(vp)] + [C.c_int32] * 4 + [C.POINTER(vp), vp, sz, vp, vp, vp, vp]),
                ("gsr_sam2_workspace_bytes", sz, [C.POINTER(GsrSam2Config)]),
                ("gsr_sam2_num_weights", C.c_int32, [C.c_int32]),
                ("gsr_sam2_encode", C.c_int32, [C.POINTER(GsrSam2Config), C.POINTER(vp), C.c_int32, vp, vp, sz, vp, vp, vp, vp]),
                ("gsr_sam2_dec_t2i", C.c_int32, [vp] * 4 + [C.c_int32] * 3 + [vp, vp]),
                ("gsr_sam2_dec_i2t_workspace_bytes", sz, [C.c_int32] * 2),
                ("gsr_sam2_dec_i2t", C.c_int32, [vp] * 5 + [C.c_int32] * 3 + [vp] * 4 + [C.c_float, vp, sz, vp, vp]),
                ("gsr_sam2_dec_upscale_workspace_bytes", sz, [C.c_int32] * 2),
                ("gsr_sam2_dec_upscale", C.c_int32, [vp, C.c_int32, C.c_int32] + [vp] * 10 + [sz, vp, vp]),
                ("gsr_sam2_dec_num_weights", C.c_int32, []),
                ("gsr_sam2_decode_workspace_bytes", sz, [C.c_int32] * 2),
                ("gsr_sam2_decode", C.c_int32, [C.c_int32, C.POINTER(vp), C.c_int32, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, sz, vp, vp,
                                                vp]),
                ("gsr_cam_lloyd_workspace_bytes", sz, [C.c_int32] * 2),
                ("gsr_cam_lloyd", C.c_int32, [vp, C.c_int32, vp, vp, C.c_int32, f64, C.c_int32] + [vp] * 6 + [sz, vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        L.gsr_profile_enable.restype = None
        L.gsr_profile_enable.argtypes = [C.c_int32]
        L.gsr_profile_reset.restype = None
        L.gsr_profile_read.restype = C.c_int32
        L.gsr_profile_read.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().gsr_last_error().decode("utf-8", "replace")
        # argument-combination errors surface as plain Exception text the reference's callers expect
        raise GsrError(f"libgsr_hip error {rc}: {msg}")


def buffer_field(which: int, name: str, N: int, D: int, W: int, H: int):
    off, nbytes = C.c_size_t(), C.c_size_t()
    check(lib().gsr_buffer_field(which, name.encode(), N, D, W, H, C.byref(off), C.byref(nbytes)))
    return off.value, nbytes.value


def profile_enable(kernels=True):
    """True = all kernels, False = off, or an iterable of kernel names."""
    if kernels is True:
        mask = -1
    elif not kernels:
        mask = 0
    else:
        mask = 0
        for k in kernels:
            mask |= 1 << KERNEL_NAMES.index(k)
    lib().gsr_profile_enable(mask)


def profile_reset():
    lib().gsr_profile_reset()


def profile_read():
    """{kernel: (total_ms, launches)} accumulated since the last reset (synchronises the events)."""
    out = {}
    for k in KERNEL_NAMES:
        ms, n = C.c_double(), C.c_int32()
        check(lib().gsr_profile_read(k.encode(), C.byref(ms), C.byref(n)))
        out[k] = (ms.value, n.value)
    return out
