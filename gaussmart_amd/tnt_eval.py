"""Tanks-and-Temples mesh evaluation: the reference's scripts/eval_tnt/run.py (the mesh as a point cloud, crop, voxel-grid
down-sampling, three ICP refinements, precision / recall histograms and the F-score) without Open3D or trimesh.  The rules
(TNT_CLOUD ... TNT_SCORE) are listed in include/gsr.h; the device path runs them as HIP kernels (gsr_mesh_face_centres,
gsr_points_transform / _crop_polygon / _voxel_*, gsr_icp_sums, gsr_dist_score) around mesh_eval's nearest_distance, the
`*_host` twins restate them in numpy float64 with scipy's cKDTree for the searches (`--host`).

    inst = load_tnt_instance("TNT_GT/Barn")
    init = align_trajectories(camera_centres(read_trajectory_log("Barn.log")), inst["gt_centres"])
    res = evaluate_tnt_mesh(TriangleMesh.read_ply("culled_mesh.ply"), inst["gt_points"], inst["crop"], SCENE_TAU["Barn"], init,
                            device="cuda")
    print(res["precision"], res["recall"], res["fscore"])

Deviations from the reference: points are float32 (TNT_POINT_F32, TNT_ICP_APPLY); the voxel grid's output order is defined
(TNT_VOXEL); the first alignment of the camera centres is a deterministic re-fitted Umeyama, not a random RANSAC
(align_trajectories); normals are not estimated (nothing that is scored reads them); precision + recall == 0 gives fscore 0.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from . import mesh_eval as ME
from ._dev import (device_points as _device_points, points64 as _points64, ptr as _ptr, stream as _stream,
                   workspace as _workspace)
from .mesh import DeviceTriangleMesh, TriangleMesh

MAX_POINT_NUMBER = 4e6
MAX_POLYGON, MAX_BINS = 256, 4096
AXES = {"X": 0, "Y": 1, "Z": 2}
# the benchmark's published distance threshold per scene, in metres
SCENE_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
             "Truck": 0.005}



def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _positive(v, name, who):
    v = float(v)
    if not (0 < v < np.inf):
        raise ValueError(f"{who}: {name} must be > 0 and finite, got {v}")
    return v


def _transform(T, who):
    T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(4, 4))
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"{who}: the last row of the transformation must be (0, 0, 0, 1), got {T[3].tolist()}")
    return T


def _crop_args(crop, who):
    """(axis index, axis_min, axis_max, polygon f64 [m,3]) of a crop volume dict (load_crop_volume)."""
    axis = crop["orthogonal_axis"]
    if isinstance(axis, str):
        if axis.upper() not in AXES:
            raise ValueError(f"{who}: orthogonal_axis must be X, Y or Z, got {axis!r}")
        axis = AXES[axis.upper()]
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise ValueError(f"{who}: orthogonal_axis must be X, Y or Z")
    poly = np.ascontiguousarray(np.asarray(crop["bounding_polygon"], np.float64).reshape(-1, 3))
    lo, hi = float(crop["axis_min"]), float(crop["axis_max"])
    if len(poly) < 1 or np.isnan(lo) or np.isnan(hi):
        raise ValueError(f"{who}: the crop volume needs a polygon and axis_min / axis_max")
    if len(poly) > MAX_POLYGON:
        raise _lib.GsrError(f"{who}: a crop polygon may have {MAX_POLYGON} vertices, got {len(poly)}")
    return axis, lo, hi, poly


def _uv(axis):
    return (1, 2) if axis == 0 else (0, 2) if axis == 1 else (0, 1)


def score_edges(tau, stretch=5):
    """The reference's histogram edges; their bits are numpy's."""
    return np.arange(0, tau * stretch, tau / 100)


def uniform_stride(n, max_points=MAX_POINT_NUMBER):
    """TNT_UNIFORM: the stride k, or 0 when the cloud is kept as it is."""
    return int(round(n / float(max_points))) if n > max_points else 0


# ---------------------------------------------------------------- device path
def mesh_to_cloud(mesh, device=None):
    """TNT_CLOUD on the device: the mesh's vertices followed by its face centres, device f32 [V + F, 3]."""
    if isinstance(mesh, TriangleMesh):
        if device is None:
            raise ValueError("mesh_to_cloud: a host TriangleMesh needs device=")
        mesh = DeviceTriangleMesh(torch.from_numpy(mesh.vertices).to(device), torch.from_numpy(mesh.triangles).to(device))
    if not mesh.vertices.is_cuda:
        raise _lib.GsrError("mesh_to_cloud: the mesh must live on the device (no CPU path; see mesh_to_cloud_host)")
    verts = mesh.vertices.to(torch.float32).contiguous()
    tris = mesh.triangles.to(torch.int32).contiguous().reshape(-1, 3)
    dev, F, V = verts.device, len(tris), len(verts)
    if F and (int(tris.min()) < 0 or int(tris.max()) >= V):
        raise ValueError("mesh_to_cloud: a triangle has an index outside [0, V)")
    out = torch.empty((V + F, 3), dtype=torch.float32, device=dev)
    out[:V] = verts
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_mesh_face_centres(_ptr(verts), _ptr(tris), F, V, _ptr(out[V:]), _stream(dev)))
    return out


def transform_points(points, transformation, device=None):
    """TNT_TRANSFORM on the device: device f32 [n,3]."""
    T = _transform(transformation, "transform_points")
    points = _device_points(points, device, "transform_points")
    dev, n = points.device, len(points)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_points_transform(_ptr(points), n, _hp(T), _ptr(out), _stream(dev)))
    return out


def crop_points(points, crop, device=None, return_mask=False):
    """TNT_CROP on the device: the points inside the crop volume, order kept (and the device bool [n] mask)."""
    points = _device_points(points, device, "crop_points")
    axis, lo, hi, poly = _crop_args(crop, "crop_points")
    dev, n = points.device, len(points)
    poly_d = torch.from_numpy(poly).to(dev)
    keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gsr_points_crop_polygon(_ptr(points), n, axis, lo, hi, _ptr(poly_d), len(poly), _ptr(keep),
                                                      _stream(dev)))
    keep = keep.bool()
    out = ME._rows(points, keep)
    return (out, keep) if return_mask else out


def voxel_down_sample(points, voxel_size, device=None, return_cells=False):
    """TNT_VOXEL on the device: one point per occupied cell, device f32 [cells,3] in ascending (ix, iy, iz) (and the device
    int32 [n] output row of every input point)."""
    voxel_size = _positive(voxel_size, "voxel_size", "voxel_down_sample")
    points = _device_points(points, device, "voxel_down_sample")
    L = _lib.lib()
    dev, n = points.device, len(points)
    ws = _workspace(L.gsr_points_voxel_workspace_bytes(n), dev)
    cells = torch.empty(n, dtype=torch.int32, device=dev) if return_cells else None
    with torch.cuda.device(dev):
        m = C.c_int64()
        args = (_ptr(points), n, voxel_size, _ptr(ws), ws.numel())
        _lib.check(L.gsr_points_voxel_count(*args, C.byref(m), _stream(dev)))
        out = torch.empty((m.value, 3), dtype=torch.float32, device=dev)
        _lib.check(L.gsr_points_voxel_emit(*args, _ptr(out), _ptr(cells), _stream(dev)))
    return (out, cells) if return_cells else out


def uniform_down_sample(points, max_points=MAX_POINT_NUMBER, device=None):
    """TNT_UNIFORM on the device (gsr_points_gather)."""
    points = _device_points(points, device, "uniform_down_sample")
    k = uniform_stride(len(points), max_points)
    if k <= 1:
        return points
    return ME.gather_points(points, torch.arange(0, len(points), k, dtype=torch.int32, device=points.device))


def icp_sums(source, target, dist, idx, means=None):
    """TNT_ICP_SUMS on the device, read back: f64 [10].  means None: (count, sum s, sum t, sum d^2, 0, 0); means = (sm, tm) as
    six numbers: (the 9 entries of sum (t - tm)(s - sm)^T, sum |s - sm|^2)."""
    source = _device_points(source, None, "icp_sums")
    target = _device_points(target, source.device, "icp_sums")
    if dist.dtype != torch.float64 or idx.dtype != torch.int32 or dist.shape != (len(source),) or idx.shape != (len(source),):
        raise ValueError("icp_sums: dist (f64) and idx (int32) must be nearest_distance's outputs for source")
    dist, idx = dist.contiguous(), idx.contiguous()
    L = _lib.lib()
    dev, n = source.device, len(source)
    mu = None if means is None else np.ascontiguousarray(np.asarray(means, np.float64).reshape(6))
    ws = _workspace(L.gsr_icp_sums_workspace_bytes(n), dev)
    out = torch.empty(10, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.gsr_icp_sums(_ptr(source), n, _ptr(target), len(target), _ptr(dist), _ptr(idx),
                                  None if mu is None else _hp(mu), _ptr(ws), ws.numel(), _ptr(out), _stream(dev)))
    return out.cpu().numpy()


def score_distances(dist, tau, edges):
    """TNT_SCORE on the device: (the number of distances < tau, np.histogram(dist, edges)[0] as int64 [B])."""
    tau = _positive(tau, "tau", "score_distances")
    if not dist.is_cuda or dist.dtype != torch.float64:
        raise _lib.GsrError("score_distances: a float64 device tensor is needed (no CPU path; see score_distances_host)")
    edges = np.ascontiguousarray(np.asarray(edges, np.float64).reshape(-1))
    B = len(edges) - 1
    if B < 1:
        raise ValueError("score_distances: at least two edges are needed")
    if B > MAX_BINS:
        raise _lib.GsrError(f"score_distances: at most {MAX_BINS} bins, got {B}")
    dist = dist.contiguous().reshape(-1)
    L = _lib.lib()
    dev, n = dist.device, dist.numel()
    ws = _workspace(L.gsr_dist_score_workspace_bytes(B), dev)
    out = torch.empty(1 + B, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.gsr_dist_score(_ptr(dist), n, _hp(edges), B, tau, _ptr(ws), ws.numel(), _ptr(out), _ptr(out[1:]), _stream(dev)))
    out = out.cpu().numpy()                 # (synchronises: `edges` has been consumed)
    return int(out[0]), out[1:].copy()


# ---------------------------------------------------------------- host path (numpy float64 + cKDTree)
def _points32(points):
    p = np.asarray(points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points)
    return np.ascontiguousarray(p, np.float32).reshape(-1, 3)


def mesh_to_cloud_host(mesh):
    """TNT_CLOUD in numpy: f32 [V + F, 3]."""
    if isinstance(mesh, DeviceTriangleMesh):
        mesh = mesh.cpu()
    verts, tris = np.asarray(mesh.vertices, np.float32).reshape(-1, 3), np.asarray(mesh.triangles, np.int64).reshape(-1, 3)
    if len(tris) and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError("mesh_to_cloud_host: a triangle has an index outside [0, V)")
    v = verts.astype(np.float64)
    centres = ((v[tris[:, 0]] + v[tris[:, 1]]) + v[tris[:, 2]]) / 3.0
    return np.concatenate([verts, centres.astype(np.float32)], 0)


def transform_points_host(points, transformation):
    """TNT_TRANSFORM in numpy: f32 [n,3]."""
    T, p = _transform(transformation, "transform_points_host"), _points64(points)
    out = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)]
    return np.stack(out, 1).astype(np.float32).reshape(-1, 3)


def crop_mask_host(points, crop):
    """TNT_CROP in numpy: bool [n]."""
    axis, lo, hi, poly = _crop_args(crop, "crop_mask_host")
    p = _points64(points)
    u, v = _uv(axis)
    pu, pv = p[:, u], p[:, v]
    inside = (p[:, axis] >= min(lo, hi)) & (p[:, axis] <= max(lo, hi))
    nodes = np.zeros(len(p), np.int64)
    m = len(poly)
    with np.errstate(all="ignore"):
        for i in range(m):
            Pi, Pj = poly[i], poly[(i + 1) % m]
            hit = ((Pi[v] < pv) & (Pj[v] >= pv)) | ((Pj[v] < pv) & (Pi[v] >= pv))
            node = Pi[u] + (pv - Pi[v]) / (Pj[v] - Pi[v]) * (Pj[u] - Pi[u])
            nodes += hit & (node < pu)
    return inside & (nodes % 2 == 1)


def crop_points_host(points, crop, return_mask=False):
    keep = crop_mask_host(points, crop)
    out = _points32(points)[keep]
    return (out, keep) if return_mask else out


def voxel_down_sample_host(points, voxel_size, return_cells=False):
    """TNT_VOXEL in numpy: f32 [cells,3] (and the int32 [n] output row of every input point).  The r-th point of every cell is
    added in round r, so each cell's sum is sequential in ascending input index."""
    voxel_size = _positive(voxel_size, "voxel_size", "voxel_down_sample_host")
    p32 = _points32(points)
    p, n = p32.astype(np.float64), len(p32)
    if n == 0:
        return (np.zeros((0, 3), np.float32), np.zeros(0, np.int32)) if return_cells else np.zeros((0, 3), np.float32)
    lo = p32.min(0).astype(np.float64) - 0.5 * voxel_size
    with np.errstate(all="ignore"):
        c = np.floor((p - lo[None]) / voxel_size)
    if not ((c >= 0) & (c < 2 ** 21)).all():
        raise _lib.GsrError(f"voxel_size {voxel_size:g} gives 2^21 or more cells on an axis (or a coordinate is not finite): "
                            "raise voxel_size")
    c = c.astype(np.int64)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.concatenate([[True], ks[1:] != ks[:-1]])
    start = np.nonzero(head)[0]
    count = np.diff(np.concatenate([start, [n]]))
    acc = np.zeros((len(start), 3))
    for r in range(int(count.max())):
        sel = np.nonzero(count > r)[0]
        acc[sel] += p[order[start[sel] + r]]
    out = (acc / count[:, None].astype(np.float64)).astype(np.float32)
    if not return_cells:
        return out
    cells = np.empty(n, np.int32)
    cells[order] = (np.cumsum(head) - 1).astype(np.int32)
    return out, cells


def uniform_down_sample_host(points, max_points=MAX_POINT_NUMBER):
    p = _points32(points)
    k = uniform_stride(len(p), max_points)
    return p if k <= 1 else p[::k]


def icp_sums_host(source, target, dist, idx, means=None, rng=None):
    """TNT_ICP_SUMS in numpy (numpy's own order of summation): f64 [10].  rng: a numpy Generator that permutes the pairs
    before they are added -- the tests measure with it how much the order of the sum matters."""
    s, t = _points64(source), _points64(target)
    idx, dist = np.asarray(idx), np.asarray(dist, np.float64)
    rows = np.nonzero((idx >= 0) & (idx < len(t)))[0]
    if rng is not None:
        rows = rng.permutation(rows)
    s, t, d = s[rows], t[idx[rows]], dist[rows]
    out = np.zeros(10)
    if means is None:
        out[0] = len(rows)
        out[1:4], out[4:7], out[7] = s.sum(0), t.sum(0), (d * d).sum()
    else:
        mu = np.asarray(means, np.float64).reshape(6)
        ds, dt = s - mu[None, :3], t - mu[None, 3:]
        out[:9] = (dt[:, :, None] * ds[:, None, :]).sum(0).reshape(9)
        out[9] = ((ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2]).sum()
    return out


def score_distances_host(dist, tau, edges):
    """TNT_SCORE in numpy."""
    tau = _positive(tau, "tau", "score_distances_host")
    d = np.asarray(dist, np.float64).reshape(-1)
    return int(np.count_nonzero(d < tau)), np.histogram(d, np.asarray(edges, np.float64))[0].astype(np.int64)


# ---------------------------------------------------------------- the two paths behind one set of names
class _DeviceOps:
    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GsrError("tnt_eval: the device path needs a GPU (no CPU fall-back; see the *_host functions)")

    def points(self, p):
        return _device_points(p, self.device, "tnt_eval")

    def cloud(self, mesh):
        return mesh_to_cloud(mesh, device=self.device)

    transform = staticmethod(transform_points)
    crop = staticmethod(crop_points)
    voxel = staticmethod(voxel_down_sample)
    uniform = staticmethod(uniform_down_sample)
    nearest = staticmethod(ME.nearest_distance)
    sums = staticmethod(icp_sums)
    score = staticmethod(score_distances)

    def sync(self):
        torch.cuda.synchronize(self.device)


class _HostOps:
    def __init__(self, rng=None, observer=None):
        self.rng, self.observer = rng, observer

    points = staticmethod(_points32)
    cloud = staticmethod(mesh_to_cloud_host)
    transform = staticmethod(transform_points_host)
    crop = staticmethod(crop_points_host)
    voxel = staticmethod(voxel_down_sample_host)
    uniform = staticmethod(uniform_down_sample_host)
    score = staticmethod(score_distances_host)

    def nearest(self, query, cloud, max_dist=np.inf):
        if self.observer is not None:
            self.observer(query, cloud, max_dist)
        return ME.nearest_distance_host(query, cloud, max_dist)

    def sums(self, source, target, dist, idx, means=None):
        return icp_sums_host(source, target, dist, idx, means, self.rng)

    def sync(self):
        pass


def _ops_for(points, device):
    if device is None and isinstance(points, torch.Tensor) and points.is_cuda:
        device = points.device
    if device is None and isinstance(points, DeviceTriangleMesh):
        device = points.device
    if device is None:
        raise ValueError("tnt_eval: host data needs device= (or use the *_host function)")
    return _DeviceOps(device)


# ---------------------------------------------------------------- Umeyama and ICP
def umeyama_from_sums(count, mean_s, mean_t, cov_sum, sq_sum):
    """Eigen's umeyama with scaling from TNT_ICP_SUMS' numbers: the 4x4 similarity that maps the sources onto the targets.
    cov_sum: sum (t - tm)(s - sm)^T, 3x3 (or 9 numbers, row-major); sq_sum: sum |s - sm|^2.  Fewer than 3 pairs or a zero
    source variance: the identity."""
    T = np.eye(4)
    n = float(count)
    if n < 3 or not sq_sum > 0:
        return T
    mean_s, mean_t = np.asarray(mean_s, np.float64).reshape(3), np.asarray(mean_t, np.float64).reshape(3)
    var_s = float(sq_sum) / n
    sigma = np.asarray(cov_sum, np.float64).reshape(3, 3) / n
    U, D, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = (U * S[None, :]) @ Vt
    c = float((D * S).sum()) / var_s
    T[:3, :3] = c * R
    T[:3, 3] = mean_t - c * (R @ mean_s)
    return T


def _icp(ops, source, target, threshold, max_iteration, relative_fitness, relative_rmse):
    threshold = _positive(threshold, "threshold", "registration_icp")
    source, target = ops.points(source), ops.points(target)
    n = len(source)
    T = np.eye(4)

    def evaluate(cur):
        if n == 0 or len(target) == 0:
            return None, None, np.zeros(10)
        dist, idx = ops.nearest(cur, target, threshold)
        return dist, idx, ops.sums(cur, target, dist, idx)

    def figures(p1):
        cnt = int(p1[0])
        return (cnt / n if n else 0.0), (float(np.sqrt(p1[7] / cnt)) if cnt else 0.0)

    cur = source
    dist, idx, p1 = evaluate(cur)
    fitness, rmse = figures(p1)
    trace, iterations = [(int(p1[0]), rmse)], 0
    if int(p1[0]) > 0:
        for _ in range(int(max_iteration)):
            cnt = int(p1[0])
            if cnt > 0:
                means = p1[1:7] / cnt
                p2 = ops.sums(cur, target, dist, idx, means)
                update = umeyama_from_sums(cnt, means[:3], means[3:], p2[:9], p2[9])
            else:
                update = np.eye(4)
            T = update @ T
            T[3] = [0.0, 0.0, 0.0, 1.0]
            cur = ops.transform(source, T)                  # TNT_ICP_APPLY
            dist, idx, p1 = evaluate(cur)
            last = (fitness, rmse)
            fitness, rmse = figures(p1)
            trace.append((int(p1[0]), rmse))
            iterations += 1
            if abs(last[0] - fitness) < relative_fitness and abs(last[1] - rmse) < relative_rmse:
                break
    return {"transformation": T, "fitness": fitness, "inlier_rmse": rmse, "iterations": iterations, "trace": trace}


def registration_icp(source, target, threshold, max_iteration=20, relative_fitness=1e-6, relative_rmse=1e-6, device=None):
    """Open3D's point-to-point ICP with scaling on the device (TNT_ICP_SUMS, TNT_ICP_APPLY), from the identity.  Returns a dict:
    transformation (f64 4x4), fitness, inlier_rmse, iterations, trace (one (correspondences, rmse) per evaluation, the first
    before any update).  Two small read-backs per iteration: the first pass's sums, then the second's."""
    return _icp(_ops_for(source, device), source, target, threshold, max_iteration, relative_fitness, relative_rmse)


def registration_icp_host(source, target, threshold, max_iteration=20, relative_fitness=1e-6, relative_rmse=1e-6, rng=None,
                          observer=None):
    """registration_icp on the host.  rng: see icp_sums_host.  observer(query, cloud, max_dist): called before every
    nearest-neighbour search -- the tests assert the margins of their fixtures in it."""
    return _icp(_HostOps(rng, observer), source, target, threshold, max_iteration, relative_fitness, relative_rmse)


def _prepare(ops, points, crop, trans=None, voxel_size=None, uniform=None):
    p = ops.points(points)
    if trans is not None:
        p = ops.transform(p, trans)
    if crop is not None:
        p = ops.crop(p, crop)
    if voxel_size is not None:
        p = ops.voxel(p, voxel_size)
    if uniform is not None:
        p = ops.uniform(p, uniform)
    return p


def _registration(ops, source, target_cropped, init_trans, crop, threshold, max_itr, voxel_size=None, uniform=None):
    init_trans = _transform(init_trans, "registration")
    s = _prepare(ops, source, crop, init_trans, voxel_size, uniform)
    t = _prepare(ops, target_cropped, None, None, voxel_size, uniform)
    reg = _icp(ops, s, t, threshold, max_itr, 1e-6, 1e-6)
    reg["transformation"] = reg["transformation"] @ init_trans
    reg["n_source"], reg["n_target"] = len(s), len(t)
    return reg


def registration_vol_ds(source, gt_target, init_trans, crop, voxel_size, threshold, max_itr, device=None):
    """registration.py:164-200 on the device: both clouds cropped (the source after init_trans) and voxel-down-sampled, ICP,
    transformation = reg.transformation @ init_trans."""
    ops = _ops_for(source, device)
    return _registration(ops, source, _prepare(ops, gt_target, crop), init_trans, crop, threshold, max_itr, voxel_size=voxel_size)


def registration_unif(source, gt_target, init_trans, crop, threshold, max_itr, max_points=MAX_POINT_NUMBER, device=None):
    """registration.py:132-161 on the device: as registration_vol_ds with TNT_UNIFORM in place of the voxel grid."""
    ops = _ops_for(source, device)
    return _registration(ops, source, _prepare(ops, gt_target, crop), init_trans, crop, threshold, max_itr, uniform=max_points)


def registration_vol_ds_host(source, gt_target, init_trans, crop, voxel_size, threshold, max_itr):
    ops = _HostOps()
    return _registration(ops, source, _prepare(ops, gt_target, crop), init_trans, crop, threshold, max_itr, voxel_size=voxel_size)


def registration_unif_host(source, gt_target, init_trans, crop, threshold, max_itr, max_points=MAX_POINT_NUMBER):
    ops = _HostOps()
    return _registration(ops, source, _prepare(ops, gt_target, crop), init_trans, crop, threshold, max_itr, uniform=max_points)


def align_trajectories(src_centres, dst_centres, threshold=0.2):
    """The first alignment from corresponding camera centres (host only): Umeyama with scaling on all pairs, re-fitted on the
    pairs with |T s - t| < threshold until that set stops changing (at most 10 rounds).  While fewer than 3 pairs pass the
    threshold (gross outliers can pull the first fit that far off), the half of the current pairs with the smallest residuals
    is taken instead.  DEVIATION: the reference runs a random RANSAC over the same identity correspondences."""
    s, t = np.asarray(src_centres, np.float64).reshape(-1, 3), np.asarray(dst_centres, np.float64).reshape(-1, 3)
    if len(s) != len(t):
        raise ValueError(f"align_trajectories: {len(s)} source and {len(t)} target centres")

    def fit(rows):
        a, b = s[rows], t[rows]
        if len(a) < 3:
            return np.eye(4)
        ma, mb = a.mean(0), b.mean(0)
        da, db = a - ma, b - mb
        return umeyama_from_sums(len(a), ma, mb, db.T @ da, (da * da).sum())

    rows = np.arange(len(s))
    T = fit(rows)
    for _ in range(10):
        r = np.linalg.norm(s @ T[:3, :3].T + T[:3, 3] - t, axis=1)
        new = np.nonzero(r < threshold)[0]
        if len(new) < 3:
            if len(rows) < 6:
                break
            new = np.sort(rows[np.argsort(r[rows], kind="stable")[:len(rows) // 2]])
        if np.array_equal(new, rows):
            break
        rows = new
        T = fit(rows)
    return T


# ---------------------------------------------------------------- scores
def _evaluate_histo(ops, source, target_cropped, trans, crop, voxel_size, tau, stretch):
    tau = _positive(tau, "tau", "evaluate_histo")
    s = _prepare(ops, source, crop, _transform(trans, "evaluate_histo"), voxel_size)
    t = _prepare(ops, target_cropped, None, None, voxel_size)
    res = {"cloud_source": s, "cloud_target": t, "tau": tau, "stretch": stretch}
    if len(s) == 0 or len(t) == 0:
        res.update(precision=0.0, recall=0.0, fscore=0.0, edges=np.array([0.0]), cum_source=np.array([0.0]),
                   cum_target=np.array([0.0]), hist_source=np.zeros(0, np.int64), hist_target=np.zeros(0, np.int64),
                   dist_source=None, dist_target=None)
        return res
    edges = score_edges(tau, stretch)
    d1 = ops.nearest(s, t, np.inf)[0]
    d2 = ops.nearest(t, s, np.inf)[0]
    c1, h1 = ops.score(d1, tau, edges)
    c2, h2 = ops.score(d2, tau, edges)
    precision, recall = c1 / len(s), c2 / len(t)
    fscore = 2 * recall * precision / (recall + precision) if recall + precision > 0 else 0.0
    res.update(precision=precision, recall=recall, fscore=fscore, edges=edges, cum_source=np.cumsum(h1).astype(float) / len(s),
               cum_target=np.cumsum(h2).astype(float) / len(t), hist_source=h1, hist_target=h2, dist_source=d1, dist_target=d2)
    return res


def evaluate_histo(source, target, trans, crop, voxel_size, tau, stretch=5, device=None):
    """evaluation.py:60-170 on the device: the source under `trans`, both clouds cropped and voxel-down-sampled, the two nearest
    distances (max_dist = inf) and TNT_SCORE.  Returns a dict: precision, recall, fscore, edges, cum_source, cum_target,
    hist_source, hist_target (int64), dist_source, dist_target, cloud_source, cloud_target."""
    ops = _ops_for(source, device)
    return _evaluate_histo(ops, source, _prepare(ops, target, crop), trans, crop, voxel_size, tau, stretch)


def evaluate_histo_host(source, target, trans, crop, voxel_size, tau, stretch=5):
    ops = _HostOps()
    return _evaluate_histo(ops, source, _prepare(ops, target, crop), trans, crop, voxel_size, tau, stretch)


def _evaluate(ops, mesh, gt_points, crop, tau, init_transform, max_points, stretch, timings):
    import time
    tau = _positive(tau, "tau", "evaluate_tnt_mesh")
    t = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            ops.sync()
            t.append(time.perf_counter())
            timings[name] = timings.get(name, 0.0) + 1e3 * (t[-1] - t[-2])

    cloud = ops.points(mesh) if isinstance(mesh, (np.ndarray, torch.Tensor)) else ops.cloud(mesh)
    gt = _prepare(ops, gt_points, crop)
    lap("cloud_ms")
    r2 = _registration(ops, cloud, gt, init_transform, crop, tau * 80, 20, voxel_size=tau)
    lap("icp1_ms")
    r3 = _registration(ops, cloud, gt, r2["transformation"], crop, tau * 20, 20, voxel_size=tau / 2.0)
    lap("icp2_ms")
    r = _registration(ops, cloud, gt, r3["transformation"], crop, 2 * tau, 20, uniform=max_points)
    lap("icp3_ms")
    res = _evaluate_histo(ops, cloud, gt, r["transformation"], crop, tau / 2.0, tau, stretch)
    lap("score_ms")
    res["transformation"] = r["transformation"]
    res["registrations"] = [r2, r3, r]
    return res


def evaluate_tnt_mesh(mesh, gt_points, crop, tau, init_transform, *, max_points=MAX_POINT_NUMBER, stretch=5, device=None,
                      timings=None):
    """run.py:155-184 on the device.  mesh: a DeviceTriangleMesh, a TriangleMesh (with device=) or an [n,3] cloud; gt_points: the
    scanner's cloud; crop: the crop volume dict (load_crop_volume) or None; init_transform: the first alignment
    (align_trajectories).  registration_vol_ds(tau, 80 tau, 20), registration_vol_ds(tau / 2, 20 tau, 20),
    registration_unif(2 tau, 20), evaluate_histo(tau / 2, tau).  Returns evaluate_histo's dict plus transformation (the final
    one) and registrations (the three ICP results).  timings: a dict that receives wall times per stage in ms (synchronises)."""
    ops = _ops_for(mesh, device)
    return _evaluate(ops, mesh, gt_points, crop, tau, init_transform, max_points, stretch, timings)


def evaluate_tnt_mesh_host(mesh, gt_points, crop, tau, init_transform, *, max_points=MAX_POINT_NUMBER, stretch=5, timings=None,
                           observer=None):
    """evaluate_tnt_mesh on the host, with the same keys (numpy arrays).  observer: see registration_icp_host."""
    return _evaluate(_HostOps(None, observer), mesh, gt_points, crop, tau, init_transform, max_points, stretch, timings)


# ---------------------------------------------------------------- files
def read_trajectory_log(path):
    """The camera-to-world matrices f64 [k,4,4] of a .log trajectory: blocks of one metadata line and four matrix lines."""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if len(lines) % 5:
        raise ValueError(f"{path}: {len(lines)} lines are not blocks of 1 + 4")
    mats = [np.array([[float(x) for x in ln.split()] for ln in lines[b + 1:b + 5]], np.float64) for b in range(0, len(lines), 5)]
    if any(m.shape != (4, 4) for m in mats):
        raise ValueError(f"{path}: a block does not hold a 4x4 matrix")
    return np.stack(mats) if mats else np.zeros((0, 4, 4))


def camera_centres(poses):
    return np.asarray(poses, np.float64).reshape(-1, 4, 4)[:, :3, 3].copy()


def load_crop_volume(path):
    """The crop volume dict of a SelectionPolygonVolume json: orthogonal_axis, axis_min, axis_max, bounding_polygon f64 [m,3]."""
    with open(path) as f:
        d = json.load(f)
    crop = {"orthogonal_axis": str(d["orthogonal_axis"]).upper(), "axis_min": float(d["axis_min"]), "axis_max": float(d["axis_max"]),
            "bounding_polygon": np.asarray(d["bounding_polygon"], np.float64).reshape(-1, 3)}
    _crop_args(crop, "load_crop_volume")
    return crop


def load_tnt_instance(dataset_dir):
    """The evaluation inputs of one scene directory <scene>/: gt_points (<scene>.ply), crop (<scene>.json), gt_trans
    (<scene>_trans.txt), gt_poses (<scene>_COLMAP_SfM.log) and gt_centres (the camera centres of gt_poses under gt_trans)."""
    scene = os.path.basename(os.path.normpath(dataset_dir))
    files = {k: os.path.join(dataset_dir, scene + suffix) for k, suffix in
             (("ply", ".ply"), ("json", ".json"), ("trans", "_trans.txt"), ("log", "_COLMAP_SfM.log"))}
    for f in files.values():
        if not os.path.isfile(f):
            raise FileNotFoundError(f"{f}: no such file")
    gt_trans = np.loadtxt(files["trans"]).reshape(4, 4)
    poses = read_trajectory_log(files["log"])
    c = camera_centres(poses)
    return {"scene": scene, "gt_points": ME.read_points_ply(files["ply"]), "crop": load_crop_volume(files["json"]),
            "gt_trans": gt_trans, "gt_poses": poses, "gt_centres": c @ gt_trans[:3, :3].T + gt_trans[:3, 3]}
