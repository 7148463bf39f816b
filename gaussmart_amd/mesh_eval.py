"""DTU mesh evaluation: the Chamfer half of the reference's scripts/eval_dtu/eval.py without Open3D, scikit-learn or a
multiprocessing pool.  The mesh is sampled to a point cloud, shuffled, thinned greedily to one point per `downsample_density`,
cut to the observed volume (ObsMask) and compared with the scanner's cloud in both directions.  The rules (EVAL_SAMPLE ...
EVAL_MEAN) are listed in include/gsr.h; the device path runs them as HIP kernels (gsr_mesh_sample_*, gsr_points_*,
gsr_dist_mean), the `*_host` twins restate them in numpy float64 with scipy's cKDTree for the searches (`--host`).

    inst = load_dtu_eval_instance("DTU/Offical_DTU_Dataset", 24)
    res = evaluate_dtu_mesh(TriangleMesh.read_ply("culled_mesh.ply"), device="cuda", **inst)
    print(res["mean_d2s"], res["mean_s2d"], res["overall"])

Deviations from the reference: points are float32 (EVAL_POINT_F32); the shuffle is a permutation the caller passes (default:
numpy's default_rng(0)), so a result can be repeated.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._dev import (device_points as _device_points, points64 as _points64, ptr as _ptr, stream as _stream,
                   workspace as _workspace)
from .compaction import compact_rows
from .mesh import DeviceTriangleMesh, TriangleMesh

DEFAULT_DENSITY, DEFAULT_PATCH, DEFAULT_MAX_DIST, DEFAULT_VIS_DIST = 0.2, 60.0, 20.0, 10.0
SAMPLE_CAP = 2 ** 24       # n1 * n2 of one triangle (include/gsr.h, EVAL_SAMPLE)


def default_order(n, seed=0):
    """EVAL_ORDER's default permutation."""
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


# ---------------------------------------------------------------- device path
def _check_thresh(thresh, who):
    thresh = float(thresh)
    if not (0 < thresh < np.inf):
        raise ValueError(f"{who}: thresh must be > 0 and finite, got {thresh}")
    return thresh


def sample_mesh_points(mesh, thresh=DEFAULT_DENSITY, device=None):
    """EVAL_SAMPLE on the device: the mesh's vertices followed by the samples of its triangles, device f32 [n,3]."""
    thresh = _check_thresh(thresh, "sample_mesh_points")
    if isinstance(mesh, TriangleMesh):
        if device is None:
            raise ValueError("sample_mesh_points: a host TriangleMesh needs device=")
        mesh = DeviceTriangleMesh(torch.from_numpy(mesh.vertices).to(device), torch.from_numpy(mesh.triangles).to(device))
    if not mesh.vertices.is_cuda:
        raise _lib.GsrError("sample_mesh_points: the mesh must live on the device (no CPU path; see sample_mesh_points_host)")
    L = _lib.lib()
    dev, F, V = mesh.device, len(mesh.triangles), len(mesh.vertices)
    ws = _workspace(L.gsr_mesh_sample_workspace_bytes(F), dev)
    with torch.cuda.device(dev):
        n = C.c_int64()
        args = (_ptr(mesh.vertices), _ptr(mesh.triangles), F, V, thresh, _ptr(ws), ws.numel())
        _lib.check(L.gsr_mesh_sample_count(*args, C.byref(n), _stream(dev)))
        out = torch.empty((n.value, 3), dtype=torch.float32, device=dev)
        _lib.check(L.gsr_mesh_sample_emit(*args, _ptr(out), _stream(dev)))
    return out


def gather_points(points, order):
    """EVAL_ORDER on the device: points[order]; order: int32 [n] (host array or device tensor)."""
    points = _device_points(points, None, "gather_points")
    dev = points.device
    order = torch.as_tensor(np.ascontiguousarray(order, np.int32) if isinstance(order, np.ndarray) else order)
    order = order.to(dev, torch.int32).contiguous()
    if order.dim() != 1:
        raise ValueError("gather_points: order must be a vector")
    if len(order) and (int(order.min()) < 0 or int(order.max()) >= len(points)):
        raise ValueError("gather_points: order has an entry outside [0, n)")
    out = torch.empty((len(order), 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_points_gather(_ptr(points), len(points), _ptr(order), len(order), _ptr(out), _stream(dev)))
    return out


def downsample_points(points, thresh=DEFAULT_DENSITY, device=None, return_rounds=False):
    """EVAL_DOWNSAMPLE on the device, in the order the points come in: the device bool [n] keep mask (and the number of rounds
    the independent-set construction took)."""
    thresh = _check_thresh(thresh, "downsample_points")
    points = _device_points(points, device, "downsample_points")
    L = _lib.lib()
    dev, n = points.device, len(points)
    keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = _workspace(L.gsr_points_search_workspace_bytes(n, 0), dev)
    rounds = C.c_int32()
    with torch.cuda.device(dev):
        _lib.check(L.gsr_points_downsample(_ptr(points), n, thresh, _ptr(ws), ws.numel(), _ptr(keep), C.byref(rounds), _stream(dev)))
    keep = keep.bool()
    return (keep, rounds.value) if return_rounds else keep


def nearest_distance(query, cloud, max_dist=np.inf, device=None):
    """EVAL_NN on the device: for every query point the distance (device f64 [nq]) to and the index (device int32 [nq]) of the
    nearest point of `cloud`; +inf and -1 where that distance is >= max_dist (or the cloud is empty)."""
    max_dist = float(max_dist)
    if not max_dist > 0:
        raise ValueError(f"nearest_distance: max_dist must be > 0, got {max_dist}")
    query = _device_points(query, device, "nearest_distance")
    cloud = _device_points(cloud, query.device, "nearest_distance")
    L = _lib.lib()
    dev, nq, nc = query.device, len(query), len(cloud)
    dist = torch.empty(nq, dtype=torch.float64, device=dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    ws = _workspace(L.gsr_points_search_workspace_bytes(nc, nq), dev)
    with torch.cuda.device(dev):
        _lib.check(L.gsr_points_nearest(_ptr(query), nq, _ptr(cloud), nc, max_dist, _ptr(ws), ws.numel(), _ptr(dist), _ptr(idx),
                                        _stream(dev)))
    return dist, idx


def _obs_args(obs_mask, bb, res, patch_size):
    obs = np.ascontiguousarray(np.asarray(obs_mask) != 0, np.uint8)
    bb = np.ascontiguousarray(np.asarray(bb, np.float32).reshape(2, 3))
    res, patch = float(np.asarray(res, np.float64).reshape(-1)[0]), float(patch_size)
    if obs.ndim != 3 or min(obs.shape) < 1:
        raise ValueError(f"ObsMask must be a non-empty 3-D array, got {list(obs.shape)}")
    if not (0 < res < np.inf) or not (0 <= patch < np.inf):
        raise ValueError(f"need Res > 0 and patch_size >= 0, got {res}, {patch}")
    return obs, bb, res, patch


def filter_by_obs_mask(points, obs_mask, bb, res, patch_size=DEFAULT_PATCH, device=None):
    """EVAL_OBSMASK on the device: (data_in, data_in_obs, inbound, in_obs) -- the two compacted clouds (device f32) and the two
    device bool [n] masks over `points`."""
    points = _device_points(points, device, "filter_by_obs_mask")
    obs, bb, res, patch = _obs_args(obs_mask, bb, res, patch_size)
    L = _lib.lib()
    dev, n = points.device, len(points)
    obs_d = torch.from_numpy(obs).to(dev)
    shape = np.array(obs.shape, np.int32)
    inb = torch.zeros(n, dtype=torch.uint8, device=dev)
    ino = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = _workspace(L.gsr_points_obs_workspace_bytes(n), dev)
    with torch.cuda.device(dev):
        n_in, n_obs = C.c_int64(), C.c_int64()
        _lib.check(L.gsr_points_obs_filter_count(_ptr(points), n, _ptr(obs_d), shape.ctypes.data_as(C.c_void_p),
                                                 bb.ctypes.data_as(C.c_void_p), res, patch, _ptr(ws), ws.numel(), _ptr(inb),
                                                 _ptr(ino), C.byref(n_in), C.byref(n_obs), _stream(dev)))
        data_in = torch.empty((n_in.value, 3), dtype=torch.float32, device=dev)
        data_in_obs = torch.empty((n_obs.value, 3), dtype=torch.float32, device=dev)
        _lib.check(L.gsr_points_obs_filter_emit(_ptr(points), n, _ptr(ws), ws.numel(), _ptr(data_in), _ptr(data_in_obs),
                                                _stream(dev)))
    return data_in, data_in_obs, inb.bool(), ino.bool()


def filter_by_plane(points, plane, device=None):
    """EVAL_PLANE on the device: the device bool [n] mask of the points above the plane P (4 numbers)."""
    points = _device_points(points, device, "filter_by_plane")
    plane = np.ascontiguousarray(np.asarray(plane, np.float64).reshape(4))
    dev, n = points.device, len(points)
    keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_points_plane_filter(_ptr(points), n, plane.ctypes.data_as(C.c_void_p), _ptr(keep), _stream(dev)))
    return keep.bool()


def distance_mean(dist):
    """EVAL_MEAN on the device: (mean of the finite entries as a Python float, their number); NaN for none."""
    if not dist.is_cuda or dist.dtype != torch.float64:
        raise _lib.GsrError("distance_mean: a float64 device tensor is needed (no CPU path; see distance_mean_host)")
    dist = dist.contiguous().reshape(-1)
    L = _lib.lib()
    dev, n = dist.device, dist.numel()
    ws = _workspace(L.gsr_dist_mean_workspace_bytes(n), dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.gsr_dist_mean(_ptr(dist), n, _ptr(ws), ws.numel(), _ptr(mean), _ptr(cnt), _stream(dev)))
    return float(mean.item()), int(cnt.item())


def _rows(points, mask):
    return compact_rows([points], mask)[0] if len(points) else points


def evaluate_dtu_mesh(mesh, stl_points, obs_mask, bb, res, plane, *, downsample_density=DEFAULT_DENSITY, patch_size=DEFAULT_PATCH,
                      max_dist=DEFAULT_MAX_DIST, order=None, device=None, timings=None):
    """eval.py on the device.  mesh: a DeviceTriangleMesh, a TriangleMesh (with device=), or an [n,3] point cloud (the
    reference's --mode pcd); stl_points: the scanner's cloud [m,3]; obs_mask, bb, res, plane: ObsMask{scan}_10.mat's ObsMask, BB,
    Res and Plane{scan}.mat's P (load_dtu_eval_instance).  order: EVAL_ORDER's permutation (default default_order(n)).
    Returns a dict: mean_d2s, mean_s2d, overall (Python floats), dist_d2s / idx_d2s (per point of data_in_obs), dist_s2d /
    idx_s2d (per ground-truth point above the plane), order, keep (over the shuffled cloud), inbound, in_obs (over data_down),
    above (over stl_points), data_down, rounds.  timings: a dict that receives wall times per stage in ms (synchronises)."""
    import time
    if isinstance(mesh, (np.ndarray, torch.Tensor)):
        cloud = _device_points(mesh, device, "evaluate_dtu_mesh")
    else:
        cloud = None
    dev = cloud.device if cloud is not None else (mesh.device if isinstance(mesh, DeviceTriangleMesh) else torch.device(device))
    stl = _device_points(stl_points, dev, "evaluate_dtu_mesh")
    t = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            torch.cuda.synchronize(dev)
            t.append(time.perf_counter())
            timings[name] = timings.get(name, 0.0) + 1e3 * (t[-1] - t[-2])

    if cloud is None:
        cloud = sample_mesh_points(mesh, downsample_density, device=dev)
    lap("sample_ms")
    order = default_order(len(cloud)) if order is None else np.ascontiguousarray(order, np.int32)
    if order.shape != (len(cloud),):
        raise ValueError(f"evaluate_dtu_mesh: order must have {len(cloud)} entries, got {list(order.shape)}")
    shuffled = gather_points(cloud, order)
    lap("order_ms")
    keep, rounds = downsample_points(shuffled, downsample_density, return_rounds=True)
    data_down = _rows(shuffled, keep)
    lap("downsample_ms")
    data_in, data_in_obs, inbound, in_obs = filter_by_obs_mask(data_down, obs_mask, bb, res, patch_size)
    above = filter_by_plane(stl, plane)
    stl_above = _rows(stl, above)
    lap("filters_ms")
    dist_d2s, idx_d2s = nearest_distance(data_in_obs, stl, max_dist)
    lap("search_d2s_ms")
    dist_s2d, idx_s2d = nearest_distance(stl_above, data_in, max_dist)
    lap("search_s2d_ms")
    mean_d2s, _ = distance_mean(dist_d2s)
    mean_s2d, _ = distance_mean(dist_s2d)
    lap("means_ms")
    return {"mean_d2s": mean_d2s, "mean_s2d": mean_s2d, "overall": (mean_d2s + mean_s2d) / 2, "dist_d2s": dist_d2s,
            "idx_d2s": idx_d2s, "dist_s2d": dist_s2d, "idx_s2d": idx_s2d, "order": order, "keep": keep, "inbound": inbound,
            "in_obs": in_obs, "above": above, "data_down": data_down, "rounds": rounds}


# ---------------------------------------------------------------- host path (numpy float64 + cKDTree)
def _dist2(a, b):
    """EVAL_DIST on float64 copies of float32 points."""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def sample_mesh_points_host(mesh, thresh=DEFAULT_DENSITY):
    """EVAL_SAMPLE in numpy: f32 [n,3]."""
    thresh = _check_thresh(thresh, "sample_mesh_points_host")
    if isinstance(mesh, DeviceTriangleMesh):
        mesh = mesh.cpu()
    verts, tris = np.asarray(mesh.vertices, np.float32), np.asarray(mesh.triangles, np.int64).reshape(-1, 3)
    V = len(verts)
    tris = tris[((tris >= 0) & (tris < V)).all(1)]
    v = verts.astype(np.float64)
    p0 = v[tris[:, 0]]
    v1, v2 = v[tris[:, 1]] - p0, v[tris[:, 2]] - p0
    with np.errstate(all="ignore"):
        l1, l2 = _norm3(v1), _norm3(v2)
        cr = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                       v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], 1)
        area2 = _norm3(cr)
        thr = thresh * np.sqrt(l1 * l2 / area2)
        n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
        ok = (area2 > 0) & (n1 >= 1) & (n2 >= 1)
        if (ok & ~(n1 * n2 <= SAMPLE_CAP)).any():
            raise _lib.GsrError("a triangle asks for more than 2^24 samples (n1 * n2): raise downsample_density")
    # triangles with the same (n1, n2) keep the same (i, j) pairs: one pass per distinct pair of counts, written to the
    # triangles' places in the output
    sel = np.nonzero(ok)[0]
    combos, inv = np.unique(np.stack([n1[sel], n2[sel]], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    grids = []
    for m1, m2 in combos:
        a, b = (np.arange(int(m1) + 1) + 0.5) / m1, (np.arange(int(m2) + 1) + 0.5) / m2
        ii, jj = np.nonzero(a[:, None] + b[None, :] < 1)
        grids.append((a[ii], b[jj]))
    counts = np.array([len(g[0]) for g in grids], np.int64)[inv] if len(sel) else np.zeros(0, np.int64)
    start = V + np.concatenate([[0], np.cumsum(counts)])
    out = np.empty((int(start[-1]), 3), np.float32)
    out[:V] = verts
    for c, (a, b) in enumerate(grids):
        if len(a) == 0:
            continue
        ts = sel[inv == c]
        q = (v1[ts][:, None, :] * a[None, :, None] + v2[ts][:, None, :] * b[None, :, None]) + p0[ts][:, None, :]
        rows = start[:-1][inv == c][:, None] + np.arange(len(a))[None, :]
        out[rows.reshape(-1)] = q.reshape(-1, 3).astype(np.float32)
    return out


def downsample_points_host(points, thresh=DEFAULT_DENSITY):
    """EVAL_DOWNSAMPLE on the host: bool [n].  cKDTree proposes the pairs (a slightly larger radius), EVAL_DIST decides."""
    from scipy.spatial import cKDTree
    thresh = _check_thresh(thresh, "downsample_points_host")
    p = _points64(points)
    n = len(p)
    keep = np.ones(n, bool)
    if n < 2:
        return keep
    pairs = cKDTree(p).query_pairs(thresh * (1 + 1e-9), output_type="ndarray")
    pairs = pairs[_dist2(p[pairs[:, 0]], p[pairs[:, 1]]) <= thresh * thresh]
    lo, hi = pairs.min(1), pairs.max(1)
    srt = np.argsort(lo, kind="stable")
    lo, hi = lo[srt], hi[srt]
    start = np.searchsorted(lo, np.arange(n + 1))
    for i in range(n):
        if keep[i] and start[i] < start[i + 1]:
            keep[hi[start[i]:start[i + 1]]] = False
    return keep


def nearest_distance_host(query, cloud, max_dist=np.inf):
    """EVAL_NN on the host: (f64 [nq] distances, int32 [nq] indices).  cKDTree proposes candidates, EVAL_DIST decides."""
    from scipy.spatial import cKDTree
    max_dist = float(max_dist)
    if not max_dist > 0:
        raise ValueError(f"nearest_distance_host: max_dist must be > 0, got {max_dist}")
    q, c = _points64(query), _points64(cloud)
    nq, nc = len(q), len(c)
    dist, idx = np.full(nq, np.inf), np.full(nq, -1, np.int32)
    if nq == 0 or nc == 0:
        return dist, idx
    k = min(4, nc)
    tree = cKDTree(c)
    cand = tree.query(q, k=k)[1].reshape(nq, k)
    d2 = _dist2(q[:, None, :], c[cand])
    best = d2.min(1)
    pick = np.where(d2 == best[:, None], cand, nc).min(1)
    # all k candidates tie: there may be more of them, and a lower index among those
    for i in np.nonzero((d2 == best[:, None]).all(1) & (nc > k))[0]:
        near = np.asarray(tree.query_ball_point(q[i], np.sqrt(best[i]) * (1 + 1e-9) + 1e-300), np.int64)
        dd = _dist2(q[i][None], c[near])
        pick[i] = near[dd == dd.min()].min()
        best[i] = dd.min()
    d = np.sqrt(best)
    found = d < max_dist
    dist[found], idx[found] = d[found], pick[found]
    return dist, idx


def filter_by_obs_mask_host(points, obs_mask, bb, res, patch_size=DEFAULT_PATCH):
    """EVAL_OBSMASK in numpy: (data_in, data_in_obs, inbound, in_obs)."""
    obs, bb, res, patch = _obs_args(obs_mask, bb, res, patch_size)
    p32 = np.ascontiguousarray(np.asarray(points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points,
                                          np.float32)).reshape(-1, 3)
    p, b = p32.astype(np.float64), bb.astype(np.float64)
    inbound = ((p >= b[:1] - patch) & (p < b[1:] + patch * 2)).all(1)
    g = np.rint((p - b[:1]) / res)
    grid = ((g >= 0) & (g < np.array(obs.shape, np.float64)[None])).all(1)
    gi = np.where(grid[:, None], g, 0).astype(np.int64)
    in_obs = inbound & grid & (obs[gi[:, 0], gi[:, 1], gi[:, 2]] != 0)
    return p32[inbound], p32[in_obs], inbound, in_obs


def filter_by_plane_host(points, plane):
    p, P = _points64(points), np.asarray(plane, np.float64).reshape(4)
    return ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] > 0


def distance_mean_host(dist):
    d = np.asarray(dist, np.float64)
    d = d[np.isfinite(d)]
    return (float(d.mean()) if len(d) else float("nan")), len(d)


def evaluate_dtu_mesh_host(mesh, stl_points, obs_mask, bb, res, plane, *, downsample_density=DEFAULT_DENSITY,
                           patch_size=DEFAULT_PATCH, max_dist=DEFAULT_MAX_DIST, order=None, timings=None):
    """evaluate_dtu_mesh on the host, with the same keys (numpy arrays)."""
    import time
    t = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            t.append(time.perf_counter())
            timings[name] = timings.get(name, 0.0) + 1e3 * (t[-1] - t[-2])

    if isinstance(mesh, (np.ndarray, torch.Tensor)):
        cloud = _points64(mesh).astype(np.float32)
    else:
        cloud = sample_mesh_points_host(mesh, downsample_density)
    stl = _points64(stl_points).astype(np.float32)
    lap("sample_ms")
    order = default_order(len(cloud)) if order is None else np.ascontiguousarray(order, np.int32)
    if order.shape != (len(cloud),):
        raise ValueError(f"evaluate_dtu_mesh_host: order must have {len(cloud)} entries, got {list(order.shape)}")
    shuffled = cloud[order]
    lap("order_ms")
    keep = downsample_points_host(shuffled, downsample_density)
    data_down = shuffled[keep]
    lap("downsample_ms")
    data_in, data_in_obs, inbound, in_obs = filter_by_obs_mask_host(data_down, obs_mask, bb, res, patch_size)
    above = filter_by_plane_host(stl, plane)
    lap("filters_ms")
    dist_d2s, idx_d2s = nearest_distance_host(data_in_obs, stl, max_dist)
    lap("search_d2s_ms")
    dist_s2d, idx_s2d = nearest_distance_host(stl[above], data_in, max_dist)
    lap("search_s2d_ms")
    mean_d2s, mean_s2d = distance_mean_host(dist_d2s)[0], distance_mean_host(dist_s2d)[0]
    lap("means_ms")
    return {"mean_d2s": mean_d2s, "mean_s2d": mean_s2d, "overall": (mean_d2s + mean_s2d) / 2, "dist_d2s": dist_d2s,
            "idx_d2s": idx_d2s, "dist_s2d": dist_s2d, "idx_s2d": idx_s2d, "order": order, "keep": keep, "inbound": inbound,
            "in_obs": in_obs, "above": above, "data_down": data_down, "rounds": None}


# ---------------------------------------------------------------- files
def read_points_ply(path):
    """The vertex positions f32 [n,3] of a binary little-endian PLY, with or without faces."""
    return TriangleMesh.read_ply(path).vertices


def load_dtu_eval_instance(dataset_dir, scan):
    """The evaluation inputs of one DTU scan as evaluate_dtu_mesh's keyword arguments: stl_points
    (Points/stl/stl{scan:03}_total.ply), obs_mask, bb, res (ObsMask/ObsMask{scan}_10.mat) and plane (ObsMask/Plane{scan}.mat)."""
    from scipy.io import loadmat
    scan = int(scan)
    obs_file = os.path.join(dataset_dir, "ObsMask", f"ObsMask{scan}_10.mat")
    plane_file = os.path.join(dataset_dir, "ObsMask", f"Plane{scan}.mat")
    stl_file = os.path.join(dataset_dir, "Points", "stl", f"stl{scan:03}_total.ply")
    for f in (obs_file, plane_file, stl_file):
        if not os.path.isfile(f):
            raise FileNotFoundError(f"{f}: no such file")
    m = loadmat(obs_file)
    return {"stl_points": read_points_ply(stl_file), "obs_mask": np.ascontiguousarray(m["ObsMask"] != 0, np.uint8),
            "bb": np.asarray(m["BB"], np.float32).reshape(2, 3), "res": float(np.asarray(m["Res"]).reshape(-1)[0]),
            "plane": np.asarray(loadmat(plane_file)["P"], np.float64).reshape(4)}


def error_colors(n, rows, dist, max_dist=DEFAULT_MAX_DIST, vis_dist=DEFAULT_VIS_DIST):
    """The reference's error colouring: blue for points that were not compared, white to red with the distance up to vis_dist
    for the `rows` that were, green where the distance is >= max_dist.  f64 [n,3]."""
    col = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1))
    d = np.asarray(dist, np.float64)
    alpha = (np.minimum(d, vis_dist) / vis_dist)[:, None]
    col[rows] = np.array([[1.0, 0.0, 0.0]]) * alpha + np.array([[1.0, 1.0, 1.0]]) * (1 - alpha)
    col[rows[d >= max_dist]] = np.array([0.0, 1.0, 0.0])
    return col
