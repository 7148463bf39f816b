"""Mesh culling by view masks: the cull_scan step of the reference's DTU evaluation
(scripts/eval_dtu/evaluate_single_scene.py:19-101) without cv2, scikit-image, trimesh or Open3D.  Every view's object mask is
dilated by a disk, every vertex is projected into every view, and a vertex stays when no view sees it outside its dilated mask.
The rules (CULL_MASK_BINARISE ... CULL_TO_WORLD) are listed in include/gsr.h; the device path runs them as HIP kernels
(gsr_mask_dilate_disk, gsr_mesh_cull_*), the host path restates them in numpy + scipy.

    inst = load_dtu_instance("DTU/scan24")                       # cameras.npz + mask/*.png
    culled = cull_mesh_by_masks(mesh, inst.proj, inst.masks, scale=inst.scale, offset=inst.offset, device="cuda")
    culled.write_ply("culled_mesh.ply")
"""
import ctypes as C
import glob
import os
from collections import namedtuple

import numpy as np
import torch

from . import _dev, _lib
from .mesh import DeviceTriangleMesh, TriangleMesh

DEFAULT_RADIUS = 24          # the reference's disk(24)
MAX_RADIUS = 127
# Device bytes one chunk of views may take for its dilated masks plus the dilation's workspace (2 bytes per pixel; masks that
# arrive from the host add a third for the upload).  DTU's 64 views of 1600 x 1200 need 246 MB: one chunk.
VIEW_CHUNK_BYTES = 1 << 30

DtuInstance = namedtuple("DtuInstance", "proj masks scale offset")


# ---------------------------------------------------------------- host half of CULL_PROJECT, loading
def dtu_projection(world_mat, scale_mat, dtype=np.float32):
    """CULL_PROJECT, host half: Pn = P / ||P[2,:3]|| with P = (world_mat @ scale_mat)[:3,:4], formed in float64 from the
    float32 matrices; returns [3,4] rounded to `dtype` (float32: what the kernels take).  For det(P[:,:3]) > 0 this is
    K/K[2,2] @ inverse(pose) of the reference's load_K_Rt_from_P; det <= 0 is refused."""
    wm = np.asarray(world_mat, np.float32).astype(np.float64)
    sm = np.asarray(scale_mat, np.float32).astype(np.float64)
    if wm.shape != (4, 4) or sm.shape != (4, 4):
        raise ValueError(f"dtu_projection: world_mat and scale_mat must be 4x4, got {wm.shape} and {sm.shape}")
    P = (wm @ sm)[:3, :4]
    det = np.linalg.det(P[:, :3])
    if not det > 0:
        raise ValueError(f"dtu_projection: det(P[:, :3]) = {det:g} is not positive: not a projection K [R|t] with a "
                         "right-handed rotation")
    return (P / np.linalg.norm(P[2, :3])).astype(dtype)


def load_dtu_instance(instance_dir):
    """Reads cameras.npz (world_mat_i, scale_mat_i) and mask/*.png (sorted; channel 0 of an image with channels, the single
    channel otherwise) of one DTU scan directory.  DtuInstance(proj f32 [n,3,4], masks uint8 [n,H,W], scale, offset) with
    scale / offset of CULL_TO_WORLD from scale_mat_0."""
    from PIL import Image
    cam_file = os.path.join(instance_dir, "cameras.npz")
    if not os.path.isfile(cam_file):
        raise FileNotFoundError(f"{cam_file}: no such file")
    paths = sorted(glob.glob(os.path.join(instance_dir, "mask", "*.png")))
    if not paths:
        raise FileNotFoundError(f"{os.path.join(instance_dir, 'mask')}: no *.png masks")
    cams = np.load(cam_file)
    n_cams = sum(1 for k in cams.files if k.startswith("world_mat_") and not k.startswith("world_mat_inv_"))
    if n_cams != len(paths):
        raise ValueError(f"{instance_dir}: {len(paths)} masks but {n_cams} cameras in cameras.npz")
    masks = []
    for p in paths:
        a = np.asarray(Image.open(p))
        a = a[..., 0] if a.ndim == 3 else a
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        elif a.dtype != np.uint8:
            a = (a != 0).astype(np.uint8)
        if masks and a.shape != masks[0].shape:
            raise ValueError(f"{p}: mask size {a.shape[1]}x{a.shape[0]} differs from {masks[0].shape[1]}x{masks[0].shape[0]} "
                             f"of {paths[0]}")
        masks.append(np.ascontiguousarray(a))
    for i in range(n_cams):
        for k in (f"world_mat_{i}", f"scale_mat_{i}"):
            if k not in cams.files:
                raise ValueError(f"{cam_file}: {k} is missing")
    proj = np.stack([dtu_projection(cams[f"world_mat_{i}"], cams[f"scale_mat_{i}"]) for i in range(n_cams)])
    sm0 = cams["scale_mat_0"].astype(np.float32)
    return DtuInstance(proj, np.stack(masks), float(sm0[0, 0]), sm0[:3, 3].copy())


def _check_views(proj, masks_shape, radius, norm_size):
    proj = np.ascontiguousarray(np.asarray(proj, np.float32).reshape(-1, 3, 4))
    if len(masks_shape) != 3:
        raise ValueError(f"masks must be uint8 [n,H,W], got shape {list(masks_shape)}")
    n, H, W = (int(s) for s in masks_shape)
    if len(proj) != n:
        raise ValueError(f"{len(proj)} projections for {n} masks")
    if n and (H < 1 or W < 1):
        raise ValueError(f"empty masks {W}x{H}")
    if not 0 <= int(radius) <= MAX_RADIUS:
        raise _lib.GsrError(f"radius must be in [0, {MAX_RADIUS}], got {radius}")
    Hn, Wn = (max(H, 1), max(W, 1)) if norm_size is None else (int(norm_size[0]), int(norm_size[1]))
    if Hn < 1 or Wn < 1:
        raise ValueError(f"norm_size must be (Hn, Wn) >= 1, got {norm_size}")
    return proj, n, H, W, Hn, Wn


def _scale_offset(scale, offset):
    if scale is None and offset is None:
        return None
    so = np.zeros(4, np.float32)
    so[0] = 1.0 if scale is None else scale
    if offset is not None:
        so[1:] = np.asarray(offset, np.float32).reshape(3)
    return so


# ---------------------------------------------------------------- device path
def dilate_masks(masks, radius=DEFAULT_RADIUS):
    """CULL_MASK_BINARISE + CULL_DISK on the device: uint8 [n,H,W] (non-zero = set) -> uint8 [n,H,W] of 0 / 1."""
    if not isinstance(masks, torch.Tensor) or not masks.is_cuda:
        raise _lib.GsrError("dilate_masks: masks must be a device tensor (no CPU path)")
    if masks.dtype != torch.uint8 or masks.dim() != 3:
        raise ValueError(f"dilate_masks: masks must be uint8 [n,H,W], got {masks.dtype} {list(masks.shape)}")
    L = _lib.lib()
    masks = masks.contiguous()
    n, H, W = masks.shape
    out = torch.empty_like(masks)
    if n == 0 or H == 0 or W == 0:
        return out
    dev = masks.device
    ws = _dev.workspace(L.gsr_mask_dilate_workspace_bytes(n, H, W), dev)
    with torch.cuda.device(dev):
        stream = _dev.stream(dev)
        _lib.check(L.gsr_mask_dilate_disk(C.c_void_p(masks.data_ptr()), n, H, W, int(radius), C.c_void_p(out.data_ptr()),
                                          C.c_void_p(ws.data_ptr()), ws.numel(), stream))
    return out


def cull_mesh_by_masks(mesh, proj, masks, radius=DEFAULT_RADIUS, norm_size=None, scale=None, offset=None, return_keep=False,
                       device=None, chunk_bytes=None):
    """cull_scan on the device.  mesh: a DeviceTriangleMesh, or a TriangleMesh with device=; proj: f32 [n,3,4] (dtu_projection);
    masks: uint8 [n,H,W], a device tensor or a host array / tensor (uploaded chunk by chunk); norm_size: (Hn, Wn) the pixel
    coordinates are normalised by, default the mask size; scale / offset: CULL_TO_WORLD.  The views are dilated and voted on in
    chunks of at most chunk_bytes (default VIEW_CHUNK_BYTES) of device memory; the AND across chunks lives in the vertex marks
    (every chunk is one gsr_mesh_cull_count call with its scans and one synchronisation; DTU's 64 views are one chunk).
    Returns a DeviceTriangleMesh, with return_keep=True also the device uint8 [V] keep mask."""
    if isinstance(mesh, TriangleMesh):
        if device is None:
            raise ValueError("cull_mesh_by_masks: a host TriangleMesh needs device=")
        if len(mesh.triangles) and (mesh.triangles.min() < 0 or mesh.triangles.max() >= len(mesh.vertices)):
            raise ValueError("cull_mesh_by_masks: a triangle index lies outside the vertex array")
        mesh = DeviceTriangleMesh(torch.from_numpy(mesh.vertices).to(device), torch.from_numpy(mesh.triangles).to(device),
                                  torch.from_numpy(mesh.vertex_colors).to(device))
    if not mesh.vertices.is_cuda:
        raise _lib.GsrError("cull_mesh_by_masks: the mesh must live on the device (no CPU path)")
    if not isinstance(masks, torch.Tensor):
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if masks.dtype != torch.uint8:
        raise ValueError(f"cull_mesh_by_masks: masks must be uint8, got {masks.dtype}")
    proj, n, H, W, Hn, Wn = _check_views(proj, masks.shape, radius, norm_size)
    so = _scale_offset(scale, offset)
    L = _lib.lib()
    dev = mesh.device
    F, V = len(mesh.triangles), len(mesh.vertices)
    budget = VIEW_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    per_view = (2 if masks.is_cuda else 3) * H * W
    chunk = max(1, budget // max(per_view, 1))
    keep = torch.ones(V, dtype=torch.uint8, device=dev)
    ws = _dev.workspace(L.gsr_mesh_cull_workspace_bytes(F, V, min(chunk, n)), dev)
    with torch.cuda.device(dev):
        stream = _dev.stream(dev)
        nv, nt = C.c_int64(), C.c_int64()
        vp, tp = C.c_void_p(mesh.vertices.data_ptr()), C.c_void_p(mesh.triangles.data_ptr())
        for a in ([0] if n == 0 else range(0, n, chunk)):        # zero views: one call that keeps everything
            b = min(a + chunk, n)
            dil = dilate_masks(masks[a:b].to(dev), radius) if b > a else None
            pj = np.ascontiguousarray(proj[a:b]).reshape(-1)
            _lib.check(L.gsr_mesh_cull_count(vp, tp, F, V, C.c_void_p(dil.data_ptr()) if dil is not None else None, b - a,
                                             max(H, 1), max(W, 1), Wn, Hn, pj.ctypes.data_as(C.c_void_p),
                                             C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(keep.data_ptr()),
                                             C.byref(nv), C.byref(nt), stream))
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        cols = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        if nv.value:
            _lib.check(L.gsr_mesh_cull_emit(vp, C.c_void_p(mesh.vertex_colors.data_ptr()), tp, F, V,
                                            so.ctypes.data_as(C.c_void_p) if so is not None else None,
                                            C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(verts.data_ptr()),
                                            C.c_void_p(cols.data_ptr()), C.c_void_p(tris.data_ptr()), stream))
    out = DeviceTriangleMesh(verts, tris, cols)
    return (out, keep) if return_keep else out


# ---------------------------------------------------------------- host path
def disk_spans(radius):
    """CULL_DISK as the integer span table w(dy) = floor(sqrt(r^2 - dy^2)), dy = -r ... r (w^2 <= r^2 - dy^2 < (w + 1)^2)."""
    r = int(radius)
    w = np.zeros(2 * r + 1, np.int64)
    for dy in range(-r, r + 1):
        rest, k = r * r - dy * dy, 0
        while (k + 1) * (k + 1) <= rest:
            k += 1
        w[dy + r] = k
    return w


def dilate_masks_host(masks, radius=DEFAULT_RADIUS):
    """CULL_MASK_BINARISE + CULL_DISK with scipy's exact Euclidean feature transform: a pixel is set when the nearest set pixel
    of the input lies at an integer squared distance <= r^2.  uint8 [n,H,W] -> uint8 [n,H,W] of 0 / 1."""
    from scipy import ndimage
    masks = np.asarray(masks)
    out = np.zeros(masks.shape, np.uint8)
    r2 = int(radius) ** 2
    for i, m in enumerate(masks):
        m = m != 0
        if not m.any():
            continue
        iy, ix = ndimage.distance_transform_edt(~m, return_distances=False, return_indices=True)
        yy, xx = np.indices(m.shape)
        out[i] = ((iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2) <= r2
    return out


def _fma32(a, b, c):
    # fmaf on float32 operands: the product is exact in float64; the sum is rounded to float64, then to float32
    return (np.float64(a) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def vote_host(vertices, proj, dilated, norm_size=None):
    """CULL_PROJECT (float32, the order of include/gsr.h), CULL_SAMPLE and CULL_VOTE in numpy: bool [V]."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    n, H, W = dilated.shape
    Hn, Wn = (H, W) if norm_size is None else norm_size
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    keep = np.ones(len(v), bool)
    f = np.float32
    with np.errstate(all="ignore"):
        for i in range(n):
            m = np.asarray(proj[i], np.float32).reshape(12)
            p = [_fma32(m[4 * k + 2], z, _fma32(m[4 * k + 1], y, _fma32(m[4 * k], x, m[4 * k + 3]))) for k in range(3)]
            den = p[2] + f(1e-6)
            gx = (p[0] / den / f(Wn - 1) - f(0.5)) * f(2)
            gy = (p[1] / den / f(Hn - 1) - f(0.5)) * f(2)
            valid = (gx > -1) & (gx < 1) & (gy > -1) & (gy < 1)
            fx = np.rint((gx + f(1)) / f(2) * f(W - 1))
            fy = np.rint((gy + f(1)) / f(2) * f(H - 1))
            inside = valid & (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
            sample = np.zeros(len(v), bool)
            sample[inside] = dilated[i][fy[inside].astype(np.int64), fx[inside].astype(np.int64)] != 0
            keep &= sample | ~valid
    return keep


def compact_host(mesh, keep, scale=None, offset=None):
    """CULL_COMPACT and CULL_TO_WORLD in numpy."""
    keep = np.asarray(keep, bool)
    tris = mesh.triangles
    tkeep = keep[tris].all(axis=1) if len(tris) else np.zeros(0, bool)
    remap = (np.cumsum(keep) - 1).astype(np.int32)
    verts = mesh.vertices[keep]
    so = _scale_offset(scale, offset)
    if so is not None:
        verts = _fma32(so[0], verts, so[1:][None, :])
    return TriangleMesh(verts, remap[tris[tkeep]].reshape(-1, 3), mesh.vertex_colors[keep])


def cull_mesh_by_masks_host(mesh, proj, masks, radius=DEFAULT_RADIUS, norm_size=None, scale=None, offset=None,
                            return_keep=False):
    """cull_scan on the host (numpy + scipy), the same rules as cull_mesh_by_masks: a TriangleMesh in, a TriangleMesh out
    (with return_keep=True also the bool [V] keep mask)."""
    if isinstance(mesh, DeviceTriangleMesh):
        mesh = mesh.cpu()
    masks = np.ascontiguousarray(masks.cpu().numpy() if isinstance(masks, torch.Tensor) else masks)
    if masks.dtype != np.uint8:
        raise ValueError(f"cull_mesh_by_masks_host: masks must be uint8, got {masks.dtype}")
    proj, n, H, W, Hn, Wn = _check_views(proj, masks.shape, radius, norm_size)
    if len(mesh.triangles) and (mesh.triangles.min() < 0 or mesh.triangles.max() >= len(mesh.vertices)):
        raise ValueError("cull_mesh_by_masks_host: a triangle index lies outside the vertex array")
    keep = vote_host(mesh.vertices, proj, dilate_masks_host(masks, radius), (Hn, Wn)) if n else np.ones(len(mesh.vertices), bool)
    out = compact_host(mesh, keep, scale, offset)
    return (out, keep) if return_keep else out
