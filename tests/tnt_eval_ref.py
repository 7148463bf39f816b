"""TEST-ONLY scalar-loop restatement of the Tanks-and-Temples evaluation rules TNT_CLOUD ... TNT_SCORE (include/gsr.h), written
for readability, and the fixtures the CPU and the GPU tests share.  The reference scripts cannot be imported (they need
Open3D and trimesh)."""
import math

import numpy as np

from mesh_eval_ref import cached, icosphere, nearest  # noqa: F401  (shared helpers)

UV = {0: (1, 2), 1: (0, 2), 2: (0, 1)}

# The spread of the host twin's ICP result over 20 random orders of adding the correspondences, measured on icp_fixture() by
# tests/test_tnt_eval_cpu.py::test_icp_sum_order_spread: the largest relative deviation of an entry of the transformation (against
# its largest |entry|) or of the rmse.  It is the noise floor of the rule itself; the device is held to 16 x this figure.
ICP_SPREAD = 2.03e-14
ICP_BAR_FACTOR = 16


def f64(points):
    return np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)


# ---------------------------------------------------------------- TNT_CLOUD, TNT_TRANSFORM
def face_centres(verts, tris):
    v = f64(verts)
    out = np.empty((len(tris), 3), np.float32)
    for k, (a, b, c) in enumerate(np.asarray(tris).reshape(-1, 3)):
        for ax in range(3):
            out[k, ax] = np.float32(((v[a, ax] + v[b, ax]) + v[c, ax]) / 3.0)
    return out


def transform(points, T):
    p, T = f64(points), np.asarray(T, np.float64).reshape(4, 4)
    out = np.empty((len(p), 3), np.float32)
    for k, (x, y, z) in enumerate(p):
        for r in range(3):
            out[k, r] = np.float32(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3])
    return out


# ---------------------------------------------------------------- TNT_CROP
def crop_point(p, axis, axis_min, axis_max, poly):
    u, v = UV[axis]
    if not (min(axis_min, axis_max) <= p[axis] <= max(axis_min, axis_max)):
        return False
    nodes, m = 0, len(poly)
    for i in range(m):
        Pi, Pj = poly[i], poly[(i + 1) % m]
        if (Pi[v] < p[v] and Pj[v] >= p[v]) or (Pj[v] < p[v] and Pi[v] >= p[v]):
            node = Pi[u] + (p[v] - Pi[v]) / (Pj[v] - Pi[v]) * (Pj[u] - Pi[u])
            if node < p[u]:
                nodes += 1
    return nodes % 2 == 1


def crop_mask(points, axis, axis_min, axis_max, poly):
    poly = np.asarray(poly, np.float64).reshape(-1, 3)
    return np.array([crop_point(p, axis, float(axis_min), float(axis_max), poly) for p in f64(points)], bool).reshape(-1)


# ---------------------------------------------------------------- TNT_VOXEL
def voxel(points, voxel_size):
    """(f32 [cells,3] in ascending (ix, iy, iz), int32 [n] output row of every point).  ValueError for an index >= 2^21."""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    if len(p) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    lo = [float(p32[:, a].min()) - 0.5 * voxel_size for a in range(3)]
    cells = {}
    for k, x in enumerate(p):
        c = tuple(math.floor((x[a] - lo[a]) / voxel_size) for a in range(3))
        if not all(0 <= ci < 2 ** 21 for ci in c):
            raise ValueError("voxel_size")
        if c not in cells:
            cells[c] = [0.0, 0.0, 0.0, 0, []]
        e = cells[c]
        for a in range(3):
            e[a] += x[a]                               # sequential, ascending input index
        e[3] += 1
        e[4].append(k)
    out = np.empty((len(cells), 3), np.float32)
    row = np.empty(len(p), np.int32)
    for r, c in enumerate(sorted(cells)):
        e = cells[c]
        for a in range(3):
            out[r, a] = np.float32(e[a] / float(e[3]))
        row[e[4]] = r
    return out, row


# ---------------------------------------------------------------- TNT_SCORE
def score(dist, tau, edges):
    """(count of d < tau, histogram): bins [e_k, e_(k+1)), the last one closed; scalar loops."""
    edges = [float(e) for e in edges]
    B = len(edges) - 1
    hist, count = np.zeros(B, np.int64), 0
    for d in np.asarray(dist, np.float64).reshape(-1):
        count += bool(d < tau)
        for k in range(B):
            if edges[k] <= d < edges[k + 1] or (k == B - 1 and d == edges[B]):
                hist[k] += 1
                break
    return count, hist


# ---------------------------------------------------------------- fixtures
SIZES = (0, 1, 255, 256, 257, 4097)


def cloud(n, seed, scale=10.0):
    return ((np.random.default_rng(seed).random((n, 3)) - 0.4) * scale).astype(np.float32)


def dyadic(n, seed):
    return (np.random.default_rng(seed).integers(-40, 40, size=(n, 3)) * 0.25).astype(np.float32)


# name -> (make the cloud, voxel size): the voxel-grid cases of tests/test_gpu_tnt_eval.py, which
# tests/test_cloud_scale_ref_cpu.py also runs the fast reference over
VOXEL = {f"n{n}": (lambda n=n: cloud(n, 60 + n, 4.0), 0.37) for n in SIZES}
VOXEL.update({
    "n20000": (lambda: cloud(20000, 61, 6.0), 0.21),
    "dyadic_on_faces": (lambda: dyadic(4097, 62), 0.5),
    "negative": (lambda: -np.abs(cloud(4097, 63, 5.0)) - 3.0, 0.3),
    "copies_of_one_point": (lambda: np.repeat(cloud(1, 64), 4097, 0), 0.1),
    "one_cell_distinct": (lambda: cloud(4097, 65, 1.0), 50.0),
})


def similarity(scale, axis, degrees, translation):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * R, translation
    return T


def apply64(T, p):
    return np.asarray(p, np.float64) @ T[:3, :3].T + T[:3, 3]


CONCAVE_XY = np.array([[-9.0, -9.0, 0.0], [9.0, -9.0, 0.0], [9.0, 9.0, 0.0], [2.0, 9.0, 0.0], [0.5, 1.5, 0.0], [-2.0, 9.0, 0.0],
                       [-9.0, 9.0, 0.0]])


def icp_fixture(seed=0, n_target=4097, n_source=2000):
    """A target cloud and a source that is a noisy subset of it under the inverse of a small similarity: ICP at threshold 0.3
    takes several iterations and its correspondence count changes on the way."""
    rng = np.random.default_rng(seed)
    target = (rng.random((n_target, 3)) * 10.0).astype(np.float32)
    S = similarity(1.01, [0.3, -0.5, 0.8], 0.6, [0.03, -0.02, 0.025])
    rows = rng.permutation(n_target)[:n_source]
    src = apply64(np.linalg.inv(S), target[rows].astype(np.float64)) + rng.normal(scale=0.01, size=(n_source, 3))
    return {"source": src.astype(np.float32), "target": target, "threshold": 0.3, "similarity": S}


def ellipsoid_instance(seed=0, n_gt=6000, noise=0.02):
    """The end-to-end case: the 1,280-triangle icosphere stretched to an ellipsoid (a sphere would leave ICP's rotation to the
    noise) and moved by the inverse of a known similarity, a noisy ground-truth cloud on the same ellipsoid, a concave crop
    polygon over XY with a Z range, and a first alignment that is off by a degree and a few centimetres."""
    rng = np.random.default_rng(seed)
    verts, tris = icosphere(3, 10.0)
    axes = np.array([1.0, 0.8, 0.6])
    S = similarity(1.03, [0.2, 0.9, -0.4], 25.0, [1.5, -2.0, 0.7])
    mesh_verts = apply64(np.linalg.inv(S), verts.astype(np.float64) * axes).astype(np.float32)
    d = rng.normal(size=(n_gt, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gt = (d * axes * (10.0 + rng.normal(scale=noise, size=(n_gt, 1)))).astype(np.float32)
    init = similarity(1.004, [0.5, 0.1, 0.7], 1.0, [0.08, -0.05, 0.06]) @ S
    crop = {"orthogonal_axis": "Z", "axis_min": -4.5, "axis_max": 5.25, "bounding_polygon": CONCAVE_XY}
    return {"verts": mesh_verts, "tris": tris, "gt_points": gt, "crop": crop, "tau": 0.5, "init": init, "similarity": S}


def write_tnt_instance(root, scene, inst, poses_gt, gt_trans):
    """The files load_tnt_instance reads, under root/scene/."""
    import json
    import os
    from gaussmart_amd.mesh import TriangleMesh
    d = os.path.join(root, scene)
    os.makedirs(d, exist_ok=True)
    TriangleMesh(np.asarray(inst["gt_points"], np.float32), None).write_ply(os.path.join(d, scene + ".ply"))
    crop = inst["crop"]
    with open(os.path.join(d, scene + ".json"), "w") as f:
        json.dump({"class_name": "SelectionPolygonVolume", "orthogonal_axis": crop["orthogonal_axis"], "axis_min": crop["axis_min"],
                   "axis_max": crop["axis_max"], "bounding_polygon": np.asarray(crop["bounding_polygon"]).tolist(),
                   "version_major": 1, "version_minor": 0}, f)
    np.savetxt(os.path.join(d, scene + "_trans.txt"), gt_trans)
    write_log(os.path.join(d, scene + "_COLMAP_SfM.log"), poses_gt)
    return d


def write_log(path, poses):
    with open(path, "w") as f:
        for k, m in enumerate(poses):
            f.write(f"{k} {k} 0\n")
            for row in np.asarray(m, np.float64):
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
