"""Segment-aware initialisation of the point cloud: the reference's convex-hull filter (filter/hull_removal.py), its labelling
of points by view masks (identification/main.py:114-148, identification/pc_projection.py) and its per-segment augmentation
(scene/gaussian_model.py:132-258), without Open3D, SAM or a subprocess.  The rules (SEG_HULL ... SEG_EMIT) are listed in
include/gsr.h; the device path runs them as HIP kernels (gsr_seg_*), the `*_host` twins restate them in numpy float64
(`--host` of gaussmart_amd.segment_cli).  The masks are somebody else's (`segments_NNN.npz`).

    keep, pts, col, _ = hull_filter(points, colors=colors, device="cuda")
    labels, areas = label_points(pts, cameras, "dtu", masks_per_view, device="cuda")
    pcd = BasicPointCloud(pts.cpu().numpy(), col.cpu().numpy(), normals, labels.cpu().numpy(), areas)
    gaussians.create_from_pcd(pcd, extent, generator=g)

Deviations from the reference: the convex hull itself is scipy's on the host (Qhull is no kernel), everything after it is on
the device; the new points' noise is one torch.randn((total, 3), generator=...) and not one MultivariateNormal.sample per
segment from the global generator (SEG_EMIT); the per-segment sums are fp64 and rounded once (SEG_STATS); the
uniform-upsampling branch labels its new points 0 (the reference forgets to extend `_segments` there).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import (device_points as _device_points, points64 as _points64, ptr as _ptr, stream as _stream,
                   workspace as _workspace)
from .compaction import compact_rows

KINDS = {"dtu": 0, "nerf": 1, "tyt": 2}
THETA = 1.96
MAX_MASKS = 32767
# the reference's hard-coded constants (pc_projection.py:48-63, :82, :89; gaussian_model.py:132, :199-204)
DTU_W, DTU_H = 1554, 1162
DTU_MIN_FRACTION = 0.1
TYT_DEFAULT_SIZE = (982, 543)
TYT_PADDING = 0.1
EPS = 1e-10
ALPHA = 0.5
MIN_EIGENVALUE = 1e-6
MIN_SEGMENT_POINTS = 5
MIN_TARGET = 10
# Device bytes the mask planes of one label-map launch may take when the masks arrive from the host (they are uploaded and
# labelled chunk by chunk; 100 SAM masks at 1554 x 1162 are 180 MB: one chunk)
VIEW_CHUNK_BYTES = 1 << 30


# ---------------------------------------------------------------- SEG_HULL, SEG_MEANSTD, SEG_FILTER
def hull_equations(points):
    """scipy's ConvexHull.equations f64 [F,4] of a host or device cloud.  Fewer than 4 points or a degenerate hull: ValueError."""
    from scipy.spatial import ConvexHull, QhullError
    p = _points64(points, keep_f64=True)
    if len(p) < 4:
        raise ValueError(f"hull_filter: a convex hull needs at least 4 points, got {len(p)}")
    try:
        return np.ascontiguousarray(ConvexHull(p).equations, np.float64)
    except QhullError as e:
        raise ValueError(f"hull_filter: the convex hull is degenerate (Qhull: {str(e).strip().splitlines()[0]})") from e


def _equations(equations, who):
    eq = np.ascontiguousarray(np.asarray(equations, np.float64))
    if eq.ndim != 2 or eq.shape[1] != 4 or len(eq) < 1:
        raise ValueError(f"{who}: equations must be [F,4] with F >= 1, got {list(eq.shape)}")
    return eq


def hull_distances(points, equations=None, device=None):
    """SEG_HULL on the device: device f64 [n].  equations: [F,4] (default: scipy's hull of the points)."""
    points, f64 = _device_points(points, device, "hull_distances", keep_f64=True)
    eq = _equations(hull_equations(points) if equations is None else equations, "hull_distances")
    dev, n = points.device, len(points)
    eq_d = torch.from_numpy(eq).to(dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_seg_hull_distance(_ptr(points), f64, n, _ptr(eq_d), len(eq), _ptr(out), _stream(dev)))
    return out


def mean_std(d):
    """SEG_MEANSTD on the device: device f64 [2] (mean, population std)."""
    if not isinstance(d, torch.Tensor) or not d.is_cuda:
        raise _lib.GsrError("mean_std: d must live on the device (no CPU path; see mean_std_host)")
    d = d.to(torch.float64).contiguous().reshape(-1)
    dev, n = d.device, d.numel()
    L = _lib.lib()
    out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _workspace(L.gsr_seg_mean_std_workspace_bytes(n), dev)
    with torch.cuda.device(dev):
        _lib.check(L.gsr_seg_mean_std(_ptr(d), n, _ptr(out), _ptr(ws), ws.numel(), _stream(dev)))
    return out


def hull_filter(points, theta=THETA, colors=None, normals=None, device=None, equations=None):
    """SEG_FILTER on the device: (keep bool [n], points, colors, normals) with the three arrays compacted (None stays None)."""
    pts, _ = _device_points(points, device, "hull_filter", keep_f64=True)
    d = hull_distances(pts, equations)
    ms = mean_std(d)
    keep = (d - ms[0]) / ms[1] >= -float(theta)

    def rows(a):
        if a is None:
            return None
        a = torch.as_tensor(a).to(pts.device).contiguous()
        if a.shape[0] != len(pts):
            raise ValueError(f"hull_filter: an attribute has {a.shape[0]} rows for {len(pts)} points")
        return a[keep]
    return keep, compact_rows([pts], keep)[0] if len(pts) else pts, rows(colors), rows(normals)


def hull_distances_host(points, equations=None):
    """SEG_HULL in numpy, facet by facet (no N x F matrix): f64 [n]."""
    p = _points64(points, keep_f64=True)
    eq = _equations(hull_equations(p) if equations is None else equations, "hull_distances_host")
    best = np.full(len(p), np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a, b, c, o in eq:
            norm = np.sqrt((a * a + b * b) + c * c)
            d = np.abs(((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + o) / norm
            best = np.where((d < best) | np.isnan(d), d, best)
    return best


def mean_std_host(d):
    """SEG_MEANSTD with numpy's own (pairwise) sums: f64 [2]."""
    d = np.asarray(d, np.float64).reshape(-1)
    return np.array([np.mean(d), np.std(d)]) if len(d) else np.array([np.nan, np.nan])


def hull_filter_host(points, theta=THETA, colors=None, normals=None, equations=None):
    p = np.asarray(points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points)
    d = hull_distances_host(p, equations)
    m, s = mean_std_host(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        keep = (d - m) / s >= -float(theta)
    rows = lambda a: None if a is None else np.asarray(a)[keep]
    return keep, p[keep], rows(colors), rows(normals)


# ---------------------------------------------------------------- SEG_LABEL, SEG_AREAS
def _mask_planes(masks, who):
    """-> uint8 [M,H,W] (tensor or array as it came), set = non-zero."""
    if isinstance(masks, (list, tuple)):
        masks = np.stack([np.asarray(m) for m in masks]) if len(masks) else np.zeros((0, 0, 0), np.uint8)
    if isinstance(masks, np.ndarray):
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3:
        raise ValueError(f"{who}: masks must be [M,H,W], got {getattr(masks, 'shape', type(masks))}")
    if masks.shape[0] > MAX_MASKS:
        raise _lib.GsrError(f"{who}: a view may have {MAX_MASKS} masks (labels are int16), got {masks.shape[0]}")
    masks = masks.contiguous()
    if masks.dtype == torch.bool:
        return masks.view(torch.uint8)
    return masks if masks.dtype == torch.uint8 else (masks != 0).view(torch.uint8)


def build_label_map(masks, device=None, chunk_bytes=None):
    """SEG_LABEL on the device: (label int16 [H,W], area int64 [M]).  masks: bool / uint8 [M,H,W], a device tensor or a host
    array (uploaded and labelled in chunks of planes of at most chunk_bytes, default VIEW_CHUNK_BYTES; a later chunk's set
    pixels overwrite an earlier one's, which is SEG_LABEL's highest index)."""
    masks = _mask_planes(masks, "build_label_map")
    if not masks.is_cuda and device is None:
        raise _lib.GsrError("build_label_map: host masks need device= (no CPU path; see build_label_map_host)")
    dev = masks.device if masks.is_cuda else torch.device(device)
    M, H, W = masks.shape
    L = _lib.lib()
    label = torch.full((H, W), -1, dtype=torch.int16, device=dev)
    area = torch.zeros(M, dtype=torch.int64, device=dev)
    budget = VIEW_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    step = M if masks.is_cuda else max(1, budget // max(H * W, 1))
    with torch.cuda.device(dev):
        if M == 0:
            _lib.check(L.gsr_seg_label_map(None, 0, H, W, _ptr(label), None, _stream(dev)))
        for m0 in range(0, M, max(step, 1)):
            part = masks[m0:m0 + step].to(dev)
            if m0 == 0 and len(part) == M:
                _lib.check(L.gsr_seg_label_map(_ptr(part), M, H, W, _ptr(label), _ptr(area), _stream(dev)))
                break
            lab = torch.empty((H, W), dtype=torch.int16, device=dev)
            _lib.check(L.gsr_seg_label_map(_ptr(part), len(part), H, W, _ptr(lab), _ptr(area[m0:]), _stream(dev)))
            label = torch.where(lab >= 0, lab + m0, label)
    return label, area


def build_label_map_host(masks):
    """SEG_LABEL in numpy: (label int16 [H,W], area int64 [M])."""
    masks = _mask_planes(masks, "build_label_map_host").cpu().numpy()
    M, H, W = masks.shape
    label = np.full((H, W), -1, np.int16)
    for m in range(M):
        label[masks[m] != 0] = m
    return label, (masks != 0).sum(axis=(1, 2)).astype(np.int64)


def merge_mask_areas(areas_per_view):
    """SEG_AREAS: {mask index: largest area over the views}.  The key is the per-view mask index, as in the reference: index 3
    of one view and index 3 of another are the same segment id."""
    out = {}
    for areas in areas_per_view:
        a = areas.detach().cpu().numpy() if isinstance(areas, torch.Tensor) else np.asarray(areas)
        for m, v in enumerate(a.reshape(-1).tolist()):
            out[m] = max(out.get(m, 0), int(v))
    return out


# ---------------------------------------------------------------- SEG_PROJ_*, SEG_ASSIGN
def _kind(kind):
    if isinstance(kind, str) and kind.lower() in KINDS:
        return KINDS[kind.lower()]
    raise ValueError(f"dataset type must be one of {sorted(KINDS)}, got {kind!r}")


def camera_terms(camera, kind):
    """The host-side terms of one view: dict(kind, world_mat f64 [4,4], scale_mat [4,4], camera_mat [3,3], cam_pos [3],
    img_w, img_h)."""
    k = _kind(kind)
    world = np.asarray(camera["world_mat"], np.float64)
    if world.shape == (3, 4):
        world = np.vstack([world, [0.0, 0.0, 0.0, 1.0]])
    if world.shape != (4, 4):
        raise ValueError(f"camera: world_mat must be 4x4 (or 3x4), got {list(world.shape)}")
    cam_mat = np.asarray(camera["camera_mat"], np.float64) if "camera_mat" in camera else np.eye(3)
    if cam_mat.ndim != 2 or cam_mat.shape[0] < 3 or cam_mat.shape[1] < 3:
        raise ValueError(f"camera: camera_mat must be at least 3x3, got {list(cam_mat.shape)}")
    scale = np.asarray(camera["scale_mat"], np.float64) if "scale_mat" in camera else np.eye(4)
    if k == KINDS["dtu"] and scale.shape != (4, 4):
        raise ValueError(f"camera: scale_mat must be 4x4, got {list(scale.shape)}")
    pos = np.full(3, np.nan)
    w, h = TYT_DEFAULT_SIZE
    if k == KINDS["dtu"]:
        try:
            pos = -np.linalg.inv(world[:3, :3]) @ world[:3, 3]
        except np.linalg.LinAlgError:
            pass                                        # only the fallback reads it; the reference would raise there
    elif k == KINDS["tyt"]:
        pos = -world[:3, :3].T @ world[:3, 3]
        if "img_size" in camera:
            w, h = (float(v) for v in np.asarray(camera["img_size"]).reshape(-1)[:2])
    return {"kind": k, "world_mat": np.ascontiguousarray(world), "scale_mat": np.ascontiguousarray(scale if scale.shape == (4, 4) else np.eye(4)),
            "camera_mat": np.ascontiguousarray(cam_mat[:3, :3]), "cam_pos": np.asarray(pos, np.float64), "img_w": float(w), "img_h": float(h)}


def _seg_views(cameras, kind, shapes):
    """cameras: list of camera dicts; shapes: per view (n_masks, H, W, label_offset) -> (ctypes array, terms)."""
    arr = (_lib.GsrSegView * max(len(cameras), 1))()
    for i, (cam, (m, H, W, off)) in enumerate(zip(cameras, shapes)):
        t = camera_terms(cam, kind)
        v = arr[i]
        v.kind, v.width, v.height, v.n_masks, v.label_offset = t["kind"], int(W), int(H), int(m), int(off)
        v.world_mat[:] = t["world_mat"].reshape(-1).tolist()
        v.scale_mat[:] = t["scale_mat"].reshape(-1).tolist()
        v.camera_mat[:] = t["camera_mat"].reshape(-1).tolist()
        v.cam_pos[:] = t["cam_pos"].tolist()
        v.img_w, v.img_h = t["img_w"], t["img_h"]
    return arr


def _prepare(points, f64, arr, n_views, label_elems):
    L = _lib.lib()
    dev = points.device
    ws = _workspace(L.gsr_seg_views_workspace_bytes(n_views), dev)
    _lib.check(L.gsr_seg_views_prepare(_ptr(points), f64, len(points), arr, n_views, label_elems, _ptr(ws), ws.numel(), _stream(dev)))
    return ws


def project_points(points, camera, kind, device=None):
    """SEG_PROJ_* of one view on the device: (uv f64 [n,2], z f64 [n])."""
    points, f64 = _device_points(points, device, "project_points", keep_f64=True)
    dev, n = points.device, len(points)
    arr = _seg_views([camera], kind, [(0, 0, 0, 0)])
    uv = torch.empty((n, 2), dtype=torch.float64, device=dev)
    z = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = _prepare(points, f64, arr, 1, 0)
        _lib.check(_lib.lib().gsr_seg_project(_ptr(points), f64, n, _ptr(ws), ws.numel(), 1, 0, _ptr(uv), _ptr(z), _stream(dev)))
    return uv, z


def assign_segments(points, cameras, kind, label_maps, n_masks=None, device=None):
    """SEG_ASSIGN on the device: int32 [n].  label_maps: per view a device int16 [H,W] map (build_label_map) or None for a
    view without masks; n_masks: per view the number of masks (default: 1 where a map is given, which is all (a) asks)."""
    points, f64 = _device_points(points, device, "assign_segments", keep_f64=True)
    dev, n = points.device, len(points)
    if len(cameras) != len(label_maps):
        raise ValueError(f"assign_segments: {len(cameras)} cameras for {len(label_maps)} label maps")
    shapes, flat, off = [], [], 0
    for i, lm in enumerate(label_maps):
        m = (0 if lm is None else 1) if n_masks is None else int(n_masks[i])
        if lm is None or m == 0:
            shapes.append((0, 0, 0, 0))
            continue
        if not lm.is_cuda or lm.dtype != torch.int16 or lm.dim() != 2:
            raise _lib.GsrError("assign_segments: a label map must be a device int16 [H,W] tensor (build_label_map)")
        shapes.append((m, lm.shape[0], lm.shape[1], off))
        flat.append(lm.reshape(-1))
        off += lm.numel()
    maps = torch.cat(flat) if flat else torch.empty(0, dtype=torch.int16, device=dev)
    arr = _seg_views(cameras, kind, shapes)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _prepare(points, f64, arr, len(cameras), maps.numel())
        _lib.check(_lib.lib().gsr_seg_assign(_ptr(points), f64, n, _ptr(ws), ws.numel(), len(cameras), _ptr(maps), _ptr(out),
                                             _stream(dev)))
    return out


def label_points(points, cameras, kind, masks_per_view, device=None, chunk_bytes=None):
    """Step 2 of the reference on the device: the label maps view by view, then one assignment.  masks_per_view: per view
    [M,H,W] masks (or None / an empty list).  Returns (labels int32 [n] on the device, mask_areas dict)."""
    points, _ = _device_points(points, device, "label_points", keep_f64=True)
    maps, areas, counts = [], [], []
    for masks in masks_per_view:
        if masks is None or len(masks) == 0:
            maps.append(None); counts.append(0)
            continue
        lm, area = build_label_map(masks, points.device, chunk_bytes)
        maps.append(lm); areas.append(area); counts.append(len(area))
    return assign_segments(points, cameras, kind, maps, counts), merge_mask_areas(areas)


def _nan_to_num(a):
    return np.clip(np.where(np.isnan(a), 0.0, a), -np.finfo(np.float64).max, np.finfo(np.float64).max)


def project_points_host(points, camera, kind):
    """SEG_PROJ_* in numpy, term by term as the rules state them: (uv f64 [n,2], z f64 [n])."""
    p = _points64(points, keep_f64=True)
    t = camera_terms(camera, kind)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    Wm, K = t["world_mat"], t["camera_mat"]
    with np.errstate(all="ignore"):
        if t["kind"] == KINDS["dtu"]:
            S = t["scale_mat"]
            s = [((S[r, 0] * x + S[r, 1] * y) + S[r, 2] * z) + S[r, 3] for r in range(4)]
            c = [((Wm[r, 0] * s[0] + Wm[r, 1] * s[1]) + Wm[r, 2] * s[2]) + Wm[r, 3] * s[3] for r in range(4)]
            u, v, depth = K[0, 0] * (c[0] / c[3]) + K[0, 2], K[1, 1] * (c[1] / c[3]) + K[1, 2], c[2]
            inside = (u >= 0) & (u < DTU_W) & (v >= 0) & (v < DTU_H)
            if float(inside.sum()) < DTU_MIN_FRACTION * float(len(p)):
                d = p - t["cam_pos"]
                length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                r = d / length[:, None]
                u = (r[:, 0] / (r[:, 2] + EPS)) * (DTU_W / 3) + DTU_W / 2
                v = (r[:, 1] / (r[:, 2] + EPS)) * (DTU_H / 3) + DTU_H / 2
        elif t["kind"] == KINDS["nerf"]:
            c = [((Wm[r, 0] * x + Wm[r, 1] * y) + Wm[r, 2] * z) + Wm[r, 3] for r in range(3)]
            q = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
            u, v, depth = q[0] / q[2], q[1] / q[2], c[2]
        else:
            ok = ~np.isnan(p).any(axis=1)
            if not ok.any():
                return np.zeros((len(p), 2)), np.zeros(len(p))
            lo, hi = p[ok].min(axis=0), p[ok].max(axis=0)
            span = 1 - 2 * TYT_PADDING
            u = _nan_to_num((TYT_PADDING + span * (x - lo[0]) / ((hi[0] - lo[0]) + EPS)) * t["img_w"])
            v = _nan_to_num((TYT_PADDING + span * (y - lo[1]) / ((hi[1] - lo[1]) + EPS)) * t["img_h"])
            d = p - t["cam_pos"]
            depth = (d[:, 0] * Wm[2, 0] + d[:, 1] * Wm[2, 1]) + d[:, 2] * Wm[2, 2]
    return np.stack([u, v], axis=1), np.asarray(depth).copy()


def assign_segments_host(points, cameras, kind, label_maps, n_masks=None):
    """SEG_ASSIGN in numpy: int32 [n].  label_maps: per view an int16 [H,W] array or None."""
    p = _points64(points, keep_f64=True)
    out = np.full(len(p), -1, np.int32)
    for i, (cam, lm) in enumerate(zip(cameras, label_maps)):
        m = (0 if lm is None else 1) if n_masks is None else int(n_masks[i])
        if lm is None or m == 0 or lm.size == 0:
            continue
        lm = np.asarray(lm)
        H, W = lm.shape
        uv, z = project_points_host(p, cam, kind)
        with np.errstate(invalid="ignore"):
            vis = (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H) & (z > 0) & (out == -1)
        xs = np.rint(np.clip(uv[vis, 0], 0, W - 1)).astype(np.int64)
        ys = np.rint(np.clip(uv[vis, 1], 0, H - 1)).astype(np.int64)
        out[vis] = lm[ys, xs]
    return out


def label_points_host(points, cameras, kind, masks_per_view):
    maps, areas, counts = [], [], []
    for masks in masks_per_view:
        if masks is None or len(masks) == 0:
            maps.append(None); counts.append(0)
            continue
        lm, area = build_label_map_host(masks)
        maps.append(lm); areas.append(area); counts.append(len(area))
    return assign_segments_host(points, cameras, kind, maps, counts), merge_mask_areas(areas)


# ---------------------------------------------------------------- SEG_STATS, SEG_FACTOR
def _stats_dict(count, s64):
    f = lambda a: a.to(torch.float32)
    return {"count": count, "mean": f(s64[:, 0:3]), "cov": f(s64[:, 3:12]).reshape(-1, 3, 3), "std": f(s64[:, 12:15]),
            "mean_color": f(s64[:, 15:18]), "f64": s64}


def segment_stats(points, sh_colors, labels, n_labels):
    """SEG_STATS on the device for the labels 0 .. n_labels - 1: dict(count int64 [L], mean f32 [L,3], cov f32 [L,3,3], std f32
    [L,3], mean_color f32 [L,3], f64 = the unrounded [L,18] rows)."""
    for t in (points, sh_colors, labels):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.GsrError("segment_stats: points, sh_colors and labels must live on the device (no CPU path; see segment_stats_host)")
    points, sh_colors = points.to(torch.float32).contiguous(), sh_colors.to(torch.float32).contiguous()
    n, dev, n_labels = len(points), points.device, int(n_labels)
    if points.shape != (n, 3) or sh_colors.shape != (n, 3) or labels.shape != (n,):
        raise ValueError(f"segment_stats: points / sh_colors must be [n,3] and labels [n], got {list(points.shape)}, "
                         f"{list(sh_colors.shape)}, {list(labels.shape)}")
    if n_labels < 0:
        raise ValueError(f"segment_stats: n_labels must be >= 0, got {n_labels}")
    sorted_labels, order = torch.sort(labels.to(torch.int64), stable=True)
    seg_off = torch.searchsorted(sorted_labels, torch.arange(n_labels + 1, device=dev)).contiguous()
    count = torch.zeros(n_labels, dtype=torch.int64, device=dev)
    s64 = torch.zeros((n_labels, 18), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_seg_stats(_ptr(points), _ptr(sh_colors), _ptr(order.contiguous()), _ptr(seg_off), n, n_labels,
                                            _ptr(count), _ptr(s64), _stream(dev)))
    return _stats_dict(count, s64)


def segment_stats_host(points, sh_colors, labels, n_labels):
    """SEG_STATS in numpy float64 (numpy's own summation order): the same dict, on the CPU."""
    p = np.asarray(torch.as_tensor(points).detach().cpu().numpy(), np.float32).astype(np.float64).reshape(-1, 3)
    c = np.asarray(torch.as_tensor(sh_colors).detach().cpu().numpy(), np.float32).astype(np.float64).reshape(-1, 3)
    lab = np.asarray(torch.as_tensor(labels).detach().cpu().numpy()).reshape(-1)
    s64 = np.full((int(n_labels), 18), np.nan)
    count = np.zeros(int(n_labels), np.int64)
    with np.errstate(all="ignore"):
        for l in range(int(n_labels)):
            sel = lab == l
            k = int(sel.sum())
            count[l] = k
            if k == 0:
                continue
            q = p[sel]
            mean = q.sum(axis=0) / k
            d = q - mean
            cov = (d.T @ d) / (k - 1.0) if k > 1 else np.full((3, 3), np.nan)
            s64[l, 0:3], s64[l, 3:12], s64[l, 12:15], s64[l, 15:18] = mean, cov.reshape(-1), np.sqrt(np.diag(cov)), c[sel].sum(axis=0) / k
    return _stats_dict(torch.from_numpy(count), torch.from_numpy(s64))


def segment_factors(stats, rows=None):
    """SEG_FACTOR: the Cholesky factor of alpha^2 times the eigenvalue-clamped covariance, f32 [S,3,3] on the CPU, for the
    rows (labels) given (default all).  Batched torch float64 on the host; a factor that is not finite is diag(0.5 std)."""
    s64 = stats["f64"].detach().cpu()
    if rows is not None:
        s64 = s64[torch.as_tensor(rows, dtype=torch.int64)]
    cov, std = s64[:, 3:12].reshape(-1, 3, 3).clone(), s64[:, 12:15]
    if len(cov) == 0:
        return torch.zeros((0, 3, 3), dtype=torch.float32)
    bad = ~torch.isfinite(cov).all(dim=(1, 2))
    cov[bad] = torch.eye(3, dtype=torch.float64)
    w, V = torch.linalg.eigh(cov)
    w = torch.clamp(w, min=MIN_EIGENVALUE)
    scaled = (ALPHA ** 2) * (V @ torch.diag_embed(w) @ V.transpose(1, 2))
    tril, info = torch.linalg.cholesky_ex(scaled)
    bad = bad | (info != 0) | ~torch.isfinite(tril).all(dim=(1, 2))
    tril[bad] = torch.diag_embed(0.5 * std[bad])
    return tril.to(torch.float32)


# ---------------------------------------------------------------- SEG_PLAN, SEG_EMIT
def plan_augmentation(counts, mask_areas):
    """SEG_PLAN: (labels int64 [S] ascending, add int64 [S]) of the segments that receive new points.  counts: points per
    label 0 .. L - 1 (label -1 is never in it); mask_areas: {label: area}."""
    counts = np.asarray(counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else counts, np.int64).reshape(-1)
    if not mask_areas or len(counts) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    median = np.median(list(mask_areas.values()))
    labels = np.arange(len(counts), dtype=np.int64)
    area = np.array([mask_areas.get(int(l), median) for l in labels], np.float64)
    target = np.maximum((np.sqrt(area) * 0.1).astype(np.int64), MIN_TARGET)
    add = target - counts
    sel = (counts >= MIN_SEGMENT_POINTS) & (add > 0)
    return labels[sel], add[sel]


def _offsets(add):
    return np.concatenate([[0], np.cumsum(np.asarray(add, np.int64))]).astype(np.int64)


def augment_emit(eps, offsets, mean, tril, mean_color, labels):
    """SEG_EMIT on the device: (xyz f32 [total,3], color f32 [total,3], label int64 [total])."""
    if not isinstance(eps, torch.Tensor) or not eps.is_cuda:
        raise _lib.GsrError("augment_emit: eps must live on the device (no CPU path; see augment_emit_host)")
    dev = eps.device
    eps = eps.to(torch.float32).contiguous()
    f = lambda a, dt: torch.as_tensor(a).to(device=dev, dtype=dt).contiguous()
    offsets, labels = f(offsets, torch.int64), f(labels, torch.int64)
    mean, tril, mean_color = f(mean, torch.float32), f(tril, torch.float32).reshape(-1, 9), f(mean_color, torch.float32)
    S, total = len(labels), len(eps)
    if offsets.shape != (S + 1,) or mean.shape != (S, 3) or tril.shape != (S, 9) or mean_color.shape != (S, 3) or eps.shape != (total, 3):
        raise ValueError("augment_emit: offsets [S+1], mean [S,3], tril [S,3,3], mean_color [S,3], labels [S], eps [total,3] expected")
    off_h = offsets.cpu()
    if S and (int(off_h[0]) != 0 or int(off_h[-1]) != total or bool((off_h[1:] < off_h[:-1]).any())):
        raise ValueError("augment_emit: offsets must rise from 0 to len(eps)")
    xyz = torch.empty((total, 3), dtype=torch.float32, device=dev)
    col = torch.empty((total, 3), dtype=torch.float32, device=dev)
    lab = torch.empty(total, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_seg_augment_emit(_ptr(eps), _ptr(offsets), S, _ptr(mean), _ptr(tril), _ptr(mean_color), _ptr(labels),
                                                   total, _ptr(xyz), _ptr(col), _ptr(lab), _stream(dev)))
    return xyz, col, lab


def augment_emit_host(eps, offsets, mean, tril, mean_color, labels):
    """SEG_EMIT in numpy: the same three arrays as CPU tensors."""
    n = lambda a, dt: np.asarray(torch.as_tensor(a).detach().cpu().numpy(), dt)
    eps, off = n(eps, np.float32).astype(np.float64).reshape(-1, 3), n(offsets, np.int64)
    mean, L = n(mean, np.float32).astype(np.float64), n(tril, np.float32).astype(np.float64).reshape(-1, 3, 3)
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    e, Ls = eps, L[seg]
    le = (Ls[:, :, 0] * e[:, None, 0] + Ls[:, :, 1] * e[:, None, 1]) + Ls[:, :, 2] * e[:, None, 2]
    xyz = (mean[seg] + le).astype(np.float32)
    return torch.from_numpy(xyz), torch.from_numpy(n(mean_color, np.float32)[seg]), torch.from_numpy(n(labels, np.int64)[seg])


def _augment(points, sh_colors, segments, plan, generator, host):
    labels, add = plan
    empty = (points.new_zeros((0, 3)), sh_colors.new_zeros((0, 3)), torch.zeros(0, dtype=torch.int64, device=points.device))
    if len(labels) == 0:
        return empty
    n_labels = int(labels.max()) + 1
    stats = (segment_stats_host if host else segment_stats)(points, sh_colors, segments, n_labels)
    tril = segment_factors(stats, labels)
    total = int(add.sum())
    eps = torch.randn((total, 3), generator=generator, device=points.device, dtype=torch.float32)
    rows = torch.as_tensor(labels, dtype=torch.int64, device=stats["mean"].device)
    return (augment_emit_host if host else augment_emit)(eps, _offsets(add), stats["mean"][rows], tril, stats["mean_color"][rows], labels)


def augment_point_cloud(points, sh_colors, segments, mask_areas, generator=None):
    """The reference's mask-area augmentation on the device: (new xyz f32 [T,3], new SH colours f32 [T,3], new labels int64 [T]).
    points, sh_colors f32 [n,3], segments int [n], all on the device; generator: a device torch.Generator for the noise."""
    if not points.is_cuda:
        raise _lib.GsrError("augment_point_cloud: the cloud must live on the device (no CPU path; see augment_point_cloud_host)")
    segments = segments.to(torch.int64)
    n_labels = int(segments.max()) + 1 if len(segments) else 0
    counts = torch.bincount(segments[segments >= 0], minlength=max(n_labels, 0)) if n_labels > 0 else torch.zeros(0, dtype=torch.int64)
    return _augment(points, sh_colors, segments, plan_augmentation(counts, mask_areas), generator, False)


def augment_point_cloud_host(points, sh_colors, segments, mask_areas, generator=None):
    points, sh_colors, segments = (torch.as_tensor(t).detach().cpu() for t in (points, sh_colors, segments))
    segments = segments.to(torch.int64)
    n_labels = int(segments.max()) + 1 if len(segments) else 0
    counts = torch.bincount(segments[segments >= 0], minlength=max(n_labels, 0)) if n_labels > 0 else torch.zeros(0, dtype=torch.int64)
    return _augment(points.float(), sh_colors.float(), segments, plan_augmentation(counts, mask_areas), generator, True)


def uniform_plan(n):
    """The uniform-upsampling branch as a plan: the whole cloud is segment 0 and receives max(int(0.1 n), 10) points."""
    return np.zeros(1, np.int64), np.array([max(int(n * 0.1), MIN_TARGET)], np.int64)


def augment_uniform(points, sh_colors, generator=None):
    """The reference's uniform_upsampling branch (device, or the host twin for CPU tensors); the new points get label 0."""
    if len(points) < 2:
        raise ValueError(f"augment_uniform: a covariance needs at least 2 points, got {len(points)}")
    zeros = torch.zeros(len(points), dtype=torch.int64, device=points.device)
    return _augment(points.float(), sh_colors.float(), zeros, uniform_plan(len(points)), generator, not points.is_cuda)
