"""Mesh culling by visibility: the reference's Tanks-and-Temples step scripts/eval_tnt/cull_mesh.py without pyrender, trimesh or
Open3D.  The mesh's own depth is rendered from every camera of a trajectory, every vertex is projected into every view and
compared with the depth sampled there, a vertex stays when at least min_views views see it unoccluded, a triangle stays when
its three vertices stay, and vertices no triangle uses any more are dropped.  The rules (VIS_CAMERA ... VIS_COMPACT) are listed
in include/gsr.h; the device path runs them as HIP kernels (gsr_mesh_depth_render, gsr_mesh_vis_*), the host path restates them
in numpy float32 for small meshes and `--host`.

    c2w = load_trajectory("Truck/transforms.json")                     # or an .npy of [n,4,4] / [n,3,4] camera-to-world
    culled = cull_mesh_by_visibility(mesh, c2w, 1080, 1920, fx, fy, cx, cy, device="cuda")
    culled.write_ply("mesh_cull.ply")

Not rebuilt: trimesh's process=True / merge_vertices on load (welding of duplicate vertices).  Meshes from this project's
marching cubes are welded already; a mesh from elsewhere with duplicated vertices is culled as it is.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import torch

from . import _dev, _lib
from .mesh import DeviceTriangleMesh, TriangleMesh
from .mesh_cull import VIEW_CHUNK_BYTES, _fma32

# the reference's constants for Tanks and Temples (scripts/eval_tnt/cull_mesh.py:387-392, 40, 125, 175)
TNT_H, TNT_W = 1080, 1920
TNT_FX, TNT_FY = 1163.8678928442187, 1172.793101201448
TNT_CX, TNT_CY = 962.3120628412543, 542.0667209577691
DEFAULT_NEAR, DEFAULT_FAR, DEFAULT_EPS, DEFAULT_MIN_VIEWS = 0.01, 20.0, 0.005, 20
_HOST_BOX = 8          # host path: boxes up to 8 x 8 pixels are evaluated together, larger ones one triangle at a time


# ---------------------------------------------------------------- cameras
def w2c_from_c2w(c2w, opengl=True):
    """VIS_CAMERA, host half: camera-to-world [n,4,4] or [n,3,4] -> world-to-camera f32 [n,3,4], inverted in float64 and rounded
    once.  opengl=True: the pose's y and z axes (columns 1 and 2) are negated first, OpenGL -> OpenCV, as the reference does
    with nerfstudio poses."""
    m = np.asarray(c2w, np.float64)
    if m.ndim != 3 or m.shape[1:] not in ((4, 4), (3, 4)):
        raise ValueError(f"w2c_from_c2w: poses must be [n,4,4] or [n,3,4], got {list(m.shape)}")
    full = np.tile(np.eye(4), (len(m), 1, 1))
    full[:, :3, :] = m[:, :3, :]
    if opengl:
        full[:, :3, 1:3] *= -1.0
    return np.ascontiguousarray(np.linalg.inv(full)[:, :3, :].astype(np.float32)) if len(m) else np.zeros((0, 3, 4), np.float32)


def _up_rotation(a):
    """The rotation that takes the unit vector a to +z (Rodrigues' form, with the reference's 1e-8 in the denominator)."""
    b = np.array([0.0, 0.0, 1.0])
    v, c = np.cross(a, b), float(a @ b)
    if c < -1 + 1e-8:
        # DEVIATION: the reference perturbs `a` with random noise here; a half turn about x is the same kind of answer every time
        return np.diag([1.0, -1.0, -1.0])
    s2 = float(v @ v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K * ((1 - c) / (s2 + 1e-8))


def orient_center_scale(poses):
    """What the reference's get_traj does to nerfstudio poses, in float64: rotate so that the mean of the cameras' y axes (their
    "up") points to +z, move the mean camera position to the origin, then divide the positions by the largest |coordinate|
    among them.  [n,3or4,4] -> [n,4,4]."""
    p = np.asarray(poses, np.float64)[:, :3, :]
    mean_t = p[:, :, 3].mean(0)
    up = p[:, :, 1].mean(0)
    R = _up_rotation(up / np.linalg.norm(up))
    out = np.tile(np.eye(4), (len(p), 1, 1))
    out[:, :3, :3] = R @ p[:, :, :3]
    out[:, :3, 3] = (p[:, :, 3] - mean_t) @ R.T
    out[:, :3, 3] *= 1.0 / np.abs(out[:, :3, 3]).max()
    return out


def load_trajectory(path):
    """Camera-to-world poses float64 [n,4,4] of a trajectory file.  `.npy`: [n,4,4] or [n,3,4], taken as they are.  `.json`
    (nerfstudio / sdfstudio transforms): frames[].transform_matrix ordered by the frame number in file_path (its last run of
    digits), rounded to float32 as the reference does, then orient_center_scale."""
    if path.endswith(".npy"):
        m = np.asarray(np.load(path), np.float64)
        if m.ndim != 3 or m.shape[1:] not in ((4, 4), (3, 4)):
            raise ValueError(f"{path}: poses must be [n,4,4] or [n,3,4], got {list(m.shape)}")
        out = np.tile(np.eye(4), (len(m), 1, 1))
        out[:, :3, :] = m[:, :3, :]
        return out
    if path.endswith(".json"):
        with open(path, encoding="UTF-8") as f:
            meta = json.load(f)
        frames = {}
        for fr in meta["frames"]:
            digits = re.findall(r"\d+", os.path.basename(fr["file_path"]))
            if not digits:
                raise ValueError(f"{path}: no frame number in file_path {fr['file_path']!r}")
            if int(digits[-1]) in frames:
                raise ValueError(f"{path}: frame number {int(digits[-1])} occurs twice")
            frames[int(digits[-1])] = np.asarray(fr["transform_matrix"], np.float64)
        if not frames:
            raise ValueError(f"{path}: no frames")
        poses = np.stack([frames[k] for k in sorted(frames)]).astype(np.float32)
        return orient_center_scale(poses)
    raise ValueError(f"{path}: a trajectory is an .npy or a .json file")


def _check_views(w2c, H, W, near, far):
    w2c = np.ascontiguousarray(np.asarray(w2c, np.float32).reshape(-1, 3, 4))
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"image size must be >= 1 x 1, got {W}x{H}")
    if not (0 < near < far and np.isfinite(far)):
        raise ValueError(f"need 0 < near < far < inf, got near {near}, far {far}")
    return w2c, H, W


def _to_device_mesh(mesh, device, who):
    if isinstance(mesh, TriangleMesh):
        if device is None:
            raise ValueError(f"{who}: a host TriangleMesh needs device=")
        if len(mesh.triangles) and (mesh.triangles.min() < 0 or mesh.triangles.max() >= len(mesh.vertices)):
            raise ValueError(f"{who}: a triangle index lies outside the vertex array")
        mesh = DeviceTriangleMesh(torch.from_numpy(mesh.vertices).to(device), torch.from_numpy(mesh.triangles).to(device),
                                  torch.from_numpy(mesh.vertex_colors).to(device))
    if not mesh.vertices.is_cuda:
        raise _lib.GsrError(f"{who}: the mesh must live on the device (no CPU path; see the *_host functions)")
    return mesh


# ---------------------------------------------------------------- device path
def _views_per_call(F, H, W, budget):
    """Views whose depth images (4 H W bytes) and work list (4 F bytes) fit the budget; n_tris * n_views stays below 2^32."""
    n = max(1, int(budget) // max(4 * H * W + 4 * F, 1))
    return max(1, min(n, (2 ** 32 - 1) // max(F, 1)))


def render_mesh_depth(mesh, w2c, H, W, fx, fy, cx, cy, near=DEFAULT_NEAR, far=DEFAULT_FAR, chunk_bytes=None):
    """VIS_CAMERA ... VIS_RANGE on the device: the mesh's depth (camera z, 0.0 where nothing is hit) from every view, device f32
    [n,H,W].  mesh: a DeviceTriangleMesh; w2c: f32 [n,3,4] (w2c_from_c2w).  The work list of the kernels takes 4 bytes per
    (triangle, view): the views are rendered in groups whose lists stay below chunk_bytes (default VIEW_CHUNK_BYTES)."""
    mesh = _to_device_mesh(mesh, None, "render_mesh_depth")
    w2c, H, W = _check_views(w2c, H, W, near, far)
    L = _lib.lib()
    dev = mesh.device
    n, F, V = len(w2c), len(mesh.triangles), len(mesh.vertices)
    out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    budget = VIEW_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    chunk = max(1, min(budget // max(4 * F, 1), (2 ** 32 - 1) // max(F, 1)))
    ws = _dev.workspace(L.gsr_mesh_depth_workspace_bytes(F, min(chunk, n)), dev)
    with torch.cuda.device(dev):
        stream = _dev.stream(dev)
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            m = np.ascontiguousarray(w2c[a:b]).reshape(-1)
            _lib.check(L.gsr_mesh_depth_render(C.c_void_p(mesh.vertices.data_ptr()), C.c_void_p(mesh.triangles.data_ptr()), F, V,
                                               m.ctypes.data_as(C.c_void_p), b - a, H, W, fx, fy, cx, cy, near, far,
                                               C.c_void_p(out[a:b].data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), stream))
    return out


def visibility_counts(vertices, w2c, depths, fx, fy, cx, cy, eps=DEFAULT_EPS, min_views=DEFAULT_MIN_VIEWS, counts=None):
    """VIS_PROJECT ... VIS_VOTE on the device: per vertex the number of views that see it, CLAMPED at min_views (a vertex that
    has reached min_views is not looked at again), device int32 [V].  vertices: device f32 [V,3]; depths: device f32 [n,H,W]
    (render_mesh_depth).  counts: an earlier result to continue from with further views (changed in place and returned)."""
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda:
        raise _lib.GsrError("visibility_counts: vertices must be a device tensor (no CPU path; see visibility_counts_host)")
    if not isinstance(depths, torch.Tensor) or depths.device != vertices.device or depths.dtype != torch.float32 or depths.dim() != 3:
        raise ValueError("visibility_counts: depths must be a float32 [n,H,W] tensor on the vertices' device")
    vertices = vertices.to(torch.float32).contiguous()
    depths = depths.contiguous()
    w2c = np.ascontiguousarray(np.asarray(w2c, np.float32).reshape(-1, 3, 4))
    n, H, W = depths.shape
    if len(w2c) != n:
        raise ValueError(f"visibility_counts: {len(w2c)} matrices for {n} depth images")
    dev, V = vertices.device, len(vertices)
    if counts is None:
        counts = torch.zeros(V, dtype=torch.int32, device=dev)
    elif counts.dtype != torch.int32 or counts.shape != (V,) or counts.device != dev or not counts.is_contiguous():
        raise ValueError("visibility_counts: counts must be a contiguous int32 [V] tensor on the vertices' device")
    if n == 0 or V == 0:
        return counts
    if H < 1 or W < 1:
        raise ValueError(f"visibility_counts: empty depth images {W}x{H}")
    L = _lib.lib()
    intr = np.array([fx, fy, cx, cy], np.float32)
    with torch.cuda.device(dev):
        stream = _dev.stream(dev)
        _lib.check(L.gsr_mesh_vis_count(C.c_void_p(vertices.data_ptr()), V, C.c_void_p(depths.data_ptr()), n, H, W,
                                        w2c.ctypes.data_as(C.c_void_p), intr.ctypes.data_as(C.c_void_p), eps, int(min_views),
                                        C.c_void_p(counts.data_ptr()), stream))
    return counts


def compact_by_counts(mesh, counts, min_views=DEFAULT_MIN_VIEWS, return_keep=False):
    """VIS_COMPACT on the device from the counts of visibility_counts: a DeviceTriangleMesh (and the uint8 [V] keep mask)."""
    L = _lib.lib()
    dev = mesh.device
    F, V = len(mesh.triangles), len(mesh.vertices)
    keep = torch.empty(V, dtype=torch.uint8, device=dev)
    ws = _dev.workspace(L.gsr_mesh_vis_workspace_bytes(F, V), dev)
    with torch.cuda.device(dev):
        stream = _dev.stream(dev)
        nv, nt = C.c_int64(), C.c_int64()
        vp, tp = C.c_void_p(mesh.vertices.data_ptr()), C.c_void_p(mesh.triangles.data_ptr())
        _lib.check(L.gsr_mesh_vis_compact_count(tp, F, V, C.c_void_p(counts.data_ptr()), int(min_views), C.c_void_p(ws.data_ptr()),
                                                ws.numel(), C.c_void_p(keep.data_ptr()), C.byref(nv), C.byref(nt), stream))
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        cols = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        if nt.value:
            _lib.check(L.gsr_mesh_vis_emit(vp, C.c_void_p(mesh.vertex_colors.data_ptr()), tp, F, V, C.c_void_p(ws.data_ptr()),
                                           ws.numel(), C.c_void_p(verts.data_ptr()), C.c_void_p(cols.data_ptr()),
                                           C.c_void_p(tris.data_ptr()), stream))
    out = DeviceTriangleMesh(verts, tris, cols)
    return (out, keep) if return_keep else out


def cull_mesh_by_visibility(mesh, c2w, H, W, fx, fy, cx, cy, far=DEFAULT_FAR, eps=DEFAULT_EPS, min_views=DEFAULT_MIN_VIEWS,
                            opengl=True, return_keep=False, device=None, chunk_bytes=None, near=DEFAULT_NEAR):
    """The reference's cull_mesh on the device.  mesh: a DeviceTriangleMesh, or a TriangleMesh with device=; c2w: camera-to-world
    poses [n,4,4] or [n,3,4] (load_trajectory), OpenGL axes when opengl=True.  The views are rendered and voted on in chunks
    whose depth images and work lists stay below chunk_bytes (default VIEW_CHUNK_BYTES) of device memory; the per-vertex count
    lives across the chunks.  Returns a DeviceTriangleMesh, with return_keep=True also the device uint8 [V] keep mask."""
    mesh = _to_device_mesh(mesh, device, "cull_mesh_by_visibility")
    w2c, H, W = _check_views(w2c_from_c2w(c2w, opengl), H, W, near, far)
    n, F, V = len(w2c), len(mesh.triangles), len(mesh.vertices)
    chunk = _views_per_call(F, H, W, VIEW_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
    counts = torch.zeros(V, dtype=torch.int32, device=mesh.device)
    for a in range(0, n, chunk):
        depths = render_mesh_depth(mesh, w2c[a:a + chunk], H, W, fx, fy, cx, cy, near, far, chunk_bytes=1 << 62)
        visibility_counts(mesh.vertices, w2c[a:a + chunk], depths, fx, fy, cx, cy, eps, min_views, counts=counts)
        del depths
    return compact_by_counts(mesh, counts, min_views, return_keep)


# ---------------------------------------------------------------- host path (numpy float32, the same rules)
def _camera32(w2c, v):
    m = np.asarray(w2c, np.float32).reshape(12)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([_fma32(m[4 * k + 2], z, _fma32(m[4 * k + 1], y, _fma32(m[4 * k], x, m[4 * k + 3]))) for k in range(3)], 1)


def _fma32v(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _edge32(pa, ia, pb, ib):
    fwd = (ia <= ib)[:, None]
    return np.where(fwd, _cross32(pa, pb), -_cross32(pb, pa))


def _hits32(c0, c1, c2, n, np0, dx, dy, near, far):
    """VIS_COVER, VIS_DEPTH, VIS_RANGE for triangle rows [T,...] against rays dx, dy broadcastable to [T,P]: z, inf = no hit."""
    def dot(c):
        return _fma32v(c[:, 0:1], dx, _fma32v(c[:, 1:2], dy, c[:, 2:3]))
    b0, b1, b2 = dot(c0), dot(c1), dot(c2)
    pos = (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
    neg = (b0 <= 0) & (b1 <= 0) & (b2 <= 0)
    nd = dot(n)
    z = np0[:, None] / nd
    ok = (pos ^ neg) & (nd != 0) & (z >= np.float32(near)) & (z <= np.float32(far))
    return np.where(ok, z, np.float32(np.inf))


def _raster_view32(p, tris, H, W, fx, fy, cx, cy, near, far):
    f = np.float32
    fx, fy, cx, cy, near = f(fx), f(fy), f(cx), f(cy), f(near)
    img = np.full(H * W, np.inf, np.float32)
    inside = ((tris >= 0) & (tris < len(p))).all(1) if len(tris) else np.zeros(0, bool)
    tris = tris[inside]
    if not len(tris):
        return np.zeros((H, W), np.float32)
    i0, i1, i2 = tris[:, 0], tris[:, 1], tris[:, 2]
    p0, p1, p2 = p[i0], p[i1], p[i2]
    zs = np.stack([p0[:, 2], p1[:, 2], p2[:, 2]], 1)
    ok = np.isfinite(p0).all(1) & np.isfinite(p1).all(1) & np.isfinite(p2).all(1) & ~(zs < near).all(1)
    front = ok & (zs >= near).all(1)
    x0, x1 = np.zeros(len(tris), np.int64), np.full(len(tris), W - 1, np.int64)
    y0, y1 = np.zeros(len(tris), np.int64), np.full(len(tris), H - 1, np.int64)
    q = [a[front] for a in (p0, p1, p2)]
    u = np.stack([_fma32v(fx, a[:, 0] / a[:, 2], cx) for a in q], 1)
    v = np.stack([_fma32v(fy, a[:, 1] / a[:, 2], cy) for a in q], 1)
    x0[front] = np.clip(np.ceil(u.min(1) - f(1.5)), 0, W).astype(np.int64)
    x1[front] = np.clip(np.floor(u.max(1) + f(0.5)), -1, W - 1).astype(np.int64)
    y0[front] = np.clip(np.ceil(v.min(1) - f(1.5)), 0, H).astype(np.int64)
    y1[front] = np.clip(np.floor(v.max(1) + f(0.5)), -1, H - 1).astype(np.int64)
    ok &= (x0 <= x1) & (y0 <= y1)
    c0, c1, c2 = _edge32(p1, i1, p2, i2), _edge32(p2, i2, p0, i0), _edge32(p0, i0, p1, i1)
    n = _cross32(p1 - p0, p2 - p0)
    np0 = _fma32v(n[:, 0], p0[:, 0], _fma32v(n[:, 1], p0[:, 1], n[:, 2] * p0[:, 2]))
    rx = ((np.arange(W, dtype=np.float32) + f(0.5)) - cx) / fx           # VIS_RAY
    ry = ((np.arange(H, dtype=np.float32) + f(0.5)) - cy) / fy
    small = ok & (x1 - x0 < _HOST_BOX) & (y1 - y0 < _HOST_BOX)
    oy, ox = (a.reshape(-1) for a in np.mgrid[0:_HOST_BOX, 0:_HOST_BOX])
    ids = np.nonzero(small)[0]
    for a in range(0, len(ids), 16384):
        t = ids[a:a + 16384]
        px, py = x0[t, None] + ox[None, :], y0[t, None] + oy[None, :]
        valid = (px <= x1[t, None]) & (py <= y1[t, None])
        px, py = np.minimum(px, W - 1), np.minimum(py, H - 1)
        z = _hits32(c0[t], c1[t], c2[t], n[t], np0[t], rx[px], ry[py], near, far)
        z[~valid] = np.inf
        np.minimum.at(img, (py * W + px).reshape(-1), z.reshape(-1))
    for t in np.nonzero(ok & ~small)[0]:
        yy, xx = np.mgrid[y0[t]:y1[t] + 1, x0[t]:x1[t] + 1]
        yy, xx = yy.reshape(1, -1), xx.reshape(1, -1)
        s = slice(t, t + 1)
        z = _hits32(c0[s], c1[s], c2[s], n[s], np0[s], rx[xx], ry[yy], near, far)
        np.minimum.at(img, (yy * W + xx).reshape(-1), z.reshape(-1))
    img[~np.isfinite(img)] = 0.0
    return img.reshape(H, W)


def render_mesh_depth_host(mesh, w2c, H, W, fx, fy, cx, cy, near=DEFAULT_NEAR, far=DEFAULT_FAR):
    """VIS_CAMERA ... VIS_RANGE in numpy float32: f32 [n,H,W].  For small meshes: the work is O(sum of the triangles' pixel
    boxes) in Python-sized steps."""
    if isinstance(mesh, DeviceTriangleMesh):
        mesh = mesh.cpu()
    w2c, H, W = _check_views(w2c, H, W, near, far)
    v = np.asarray(mesh.vertices, np.float32).reshape(-1, 3)
    tris = np.asarray(mesh.triangles, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        out = [_raster_view32(_camera32(m, v), tris, H, W, fx, fy, cx, cy, near, far) for m in w2c]
    return np.stack(out) if out else np.zeros((0, H, W), np.float32)


def visibility_counts_host(vertices, w2c, depths, fx, fy, cx, cy, eps=DEFAULT_EPS, min_views=None):
    """VIS_PROJECT ... VIS_VOTE in numpy float32: int32 [V], the number of views that see each vertex (clamped at min_views
    when one is given, as the device path does)."""
    f = np.float32
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    depths = np.asarray(depths, np.float32)
    w2c = np.asarray(w2c, np.float32).reshape(-1, 3, 4)
    n, H, W = depths.shape
    if len(w2c) != n:
        raise ValueError(f"visibility_counts_host: {len(w2c)} matrices for {n} depth images")
    fx, fy, cx, cy, eps = f(fx), f(fy), f(cx), f(cy), f(eps)
    counts = np.zeros(len(v), np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            p = _camera32(w2c[i], v)
            z = p[:, 2] + f(1e-8)
            pu = _fma32v(fx, p[:, 0], cx * p[:, 2]) / z
            pv = _fma32v(fy, p[:, 1], cy * p[:, 2]) / z
            inf = (pu >= 0) & (pu <= W - 1) & (pv >= 0) & (pv <= H - 1) & (z > 0)
            k = np.nonzero(inf)[0]
            u, w, zz = pu[k], pv[k], z[k]
            xf, yf = np.floor(u), np.floor(w)
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            ax, ay, bx, by = u - xf, w - yf, (xf + f(1)) - u, (yf + f(1)) - w
            right, down = x0 + 1 < W, y0 + 1 < H
            xr, yd = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            img = depths[i]
            ds = img[y0, x0] * (bx * by)
            ds = np.where(right, _fma32v(img[y0, xr], ax * by, ds), ds)
            ds = np.where(down, _fma32v(img[yd, x0], bx * ay, ds), ds)
            ds = np.where(right & down, _fma32v(img[yd, xr], ax * ay, ds), ds)
            counts[k] += np.where(ds > 0, zz < ds + eps, True)
    return counts if min_views is None else np.minimum(counts, max(int(min_views), 0)).astype(np.int32)


def compact_host(mesh, keep):
    """VIS_COMPACT in numpy."""
    keep = np.asarray(keep, bool)
    tris = mesh.triangles
    tkeep = keep[tris].all(axis=1) if len(tris) else np.zeros(0, bool)
    used = np.zeros(len(keep), bool)
    used[tris[tkeep].reshape(-1)] = True
    remap = (np.cumsum(used) - 1).astype(np.int32)
    return TriangleMesh(mesh.vertices[used], remap[tris[tkeep]].reshape(-1, 3), mesh.vertex_colors[used])


def cull_mesh_by_visibility_host(mesh, c2w, H, W, fx, fy, cx, cy, far=DEFAULT_FAR, eps=DEFAULT_EPS, min_views=DEFAULT_MIN_VIEWS,
                                 opengl=True, return_keep=False, near=DEFAULT_NEAR):
    """The reference's cull_mesh on the host, the same rules as cull_mesh_by_visibility: a TriangleMesh in, a TriangleMesh out
    (with return_keep=True also the bool [V] keep mask)."""
    if isinstance(mesh, DeviceTriangleMesh):
        mesh = mesh.cpu()
    if len(mesh.triangles) and (mesh.triangles.min() < 0 or mesh.triangles.max() >= len(mesh.vertices)):
        raise ValueError("cull_mesh_by_visibility_host: a triangle index lies outside the vertex array")
    w2c, H, W = _check_views(w2c_from_c2w(c2w, opengl), H, W, near, far)
    depths = render_mesh_depth_host(mesh, w2c, H, W, fx, fy, cx, cy, near, far)
    keep = visibility_counts_host(mesh.vertices, w2c, depths, fx, fy, cx, cy, eps) >= int(min_views)
    out = compact_host(mesh, keep)
    return (out, keep) if return_keep else out
