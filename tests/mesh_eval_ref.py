"""TEST-ONLY float64 restatement of the DTU evaluation rules EVAL_SAMPLE ... EVAL_MEAN (include/gsr.h), written for
readability: scalar loops, numpy and scipy's cKDTree for the searches, a plain sequential greedy loop.  The reference script
itself cannot be imported (it needs Open3D and runs under __main__)."""
import math

import numpy as np
from scipy.spatial import cKDTree

_CACHE = {}


def cached(key, fn):
    """Compute a reference once and share it among the tests that need it; the arrays are made read-only."""
    if key not in _CACHE:
        val = fn()
        for a in (val if isinstance(val, tuple) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


# ---------------------------------------------------------------- EVAL_SAMPLE
def tri_counts(verts, tri, thresh):
    """(n1, n2) of one triangle as floats, or None when the triangle gives nothing."""
    V = len(verts)
    if any(int(i) < 0 or int(i) >= V for i in tri):
        return None
    p0, p1, p2 = (np.asarray(verts[int(i)], np.float32).astype(np.float64) for i in tri)
    v1, v2 = p1 - p0, p2 - p0
    l1 = math.sqrt((v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2])
    l2 = math.sqrt((v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2])
    c = (v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0])
    area2 = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    if not area2 > 0:
        return None
    thr = thresh * math.sqrt(l1 * l2 / area2)
    return l1 / thr, l2 / thr, p0, v1, v2


def sample_triangle(verts, tri, thresh):
    """The kept (i, j) pairs and the float64 samples of one triangle."""
    s = tri_counts(verts, tri, thresh)
    if s is None:
        return [], np.zeros((0, 3))
    r1, r2, p0, v1, v2 = s
    n1, n2 = math.floor(r1), math.floor(r2)
    if n1 == 0 or n2 == 0:
        return [], np.zeros((0, 3))
    pairs, pts = [], []
    for i in range(n1 + 1):
        for j in range(n2 + 1):
            a, b = (i + 0.5) / n1, (j + 0.5) / n2
            if a + b < 1:
                pairs.append((i, j))
                pts.append((v1 * a + v2 * b) + p0)
    return pairs, np.array(pts, np.float64).reshape(-1, 3)


def integer_rule_pairs(n1, n2):
    return [(i, j) for i in range(n1 + 1) for j in range(n2 + 1) if (2 * i + 1) * n2 + (2 * j + 1) * n1 < 2 * n1 * n2]


def sample_mesh(verts, tris, thresh):
    """(cloud f32 [n,3] = vertices then samples in triangle order, per-triangle counts)."""
    verts = np.asarray(verts, np.float32)
    out, counts = [verts], []
    for tri in np.asarray(tris).reshape(-1, 3):
        _, pts = sample_triangle(verts, tri, thresh)
        counts.append(len(pts))
        out.append(pts.astype(np.float32))
    return np.concatenate(out, 0), np.array(counts, np.int64)


def min_integer_margin(verts, tris, thresh):
    """Smallest relative distance of l / thr from an integer over the triangles that are sampled (the floor must be safe)."""
    m = np.inf
    for tri in np.asarray(tris).reshape(-1, 3):
        s = tri_counts(np.asarray(verts, np.float32), tri, thresh)
        if s is None:
            continue
        for r in s[:2]:
            if r >= 0.5:
                m = min(m, abs(r - round(r)) / max(r, 1.0))
    return m


# ---------------------------------------------------------------- EVAL_DIST, EVAL_DOWNSAMPLE, EVAL_NN
def dist2(a, b):
    d = np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbour_lists(points, thresh):
    """Per point the sorted indices j (itself included) with d2 <= thresh^2 by EVAL_DIST."""
    p = np.asarray(points, np.float32).astype(np.float64)
    if len(p) == 0:
        return []
    lists = cKDTree(p).query_ball_point(p, thresh * (1 + 1e-9))
    t2 = thresh * thresh
    return [np.array(sorted(j for j in l if dist2(p[i], p[j]) <= t2), np.int64) for i, l in enumerate(lists)]


def greedy_keep(points, thresh):
    """The sequential rule: point i is kept iff no kept j < i has d2 <= thresh^2."""
    nb = neighbour_lists(points, thresh)
    keep = np.zeros(len(nb), bool)
    for i, l in enumerate(nb):
        keep[i] = not any(keep[j] for j in l if j < i)
    return keep


def pair_margin(points, thresh):
    """Smallest relative distance of a pair's d from thresh (pairs up to 2 thresh apart)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    pr = cKDTree(p).query_pairs(2 * thresh, output_type="ndarray")
    if len(pr) == 0:
        return np.inf
    return float(np.abs(np.sqrt(dist2(p[pr[:, 0]], p[pr[:, 1]])) / thresh - 1).min())


def nearest(query, cloud, k=2):
    """cKDTree's own distances and indices for the k nearest (float64 copies of the float32 points)."""
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    c = np.asarray(cloud, np.float32).astype(np.float64).reshape(-1, 3)
    k = min(k, len(c))
    d, i = cKDTree(c).query(q, k=k)
    return d.reshape(len(q), k), i.reshape(len(q), k)


# ---------------------------------------------------------------- EVAL_OBSMASK, EVAL_PLANE
def obs_filter(points, obs, bb, res, patch):
    p = np.asarray(points, np.float32).astype(np.float64)
    bb = np.asarray(bb, np.float32).astype(np.float64).reshape(2, 3)
    inbound, in_obs = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for k, x in enumerate(p):
        inbound[k] = all(x[a] >= bb[0, a] - patch and x[a] < bb[1, a] + patch * 2 for a in range(3))
        g = [float(np.around((x[a] - bb[0, a]) / res)) for a in range(3)]
        if inbound[k] and all(0 <= g[a] < obs.shape[a] for a in range(3)):
            in_obs[k] = obs[int(g[0]), int(g[1]), int(g[2])] != 0
    return inbound, in_obs


def plane_filter(points, plane):
    p = np.asarray(points, np.float32).astype(np.float64)
    P = np.asarray(plane, np.float64).reshape(4)
    return np.array([((P[0] * x[0] + P[1] * x[1]) + P[2] * x[2]) + P[3] > 0 for x in p], bool)


# ---------------------------------------------------------------- fixtures shared by the CPU and the GPU tests
def random_cloud(n, seed, thresh=0.2, neighbours=5.0):
    """n uniform points in a cube sized so that a ball of radius thresh holds `neighbours` of them on average."""
    side = (max(n, 1) * 4.0 / 3.0 * np.pi * thresh ** 3 / neighbours) ** (1.0 / 3.0)
    return (np.random.default_rng(seed).random((n, 3)) * side).astype(np.float32)


def lattice():
    g = np.arange(6, dtype=np.float32) * np.float32(0.25)          # dyadic: d2 == thresh^2 exactly between neighbours
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


# name -> (make the cloud, thresh, whether pair_margin is asserted first): the down-sampling cases of tests/test_gpu_mesh_eval.py,
# which tests/test_cloud_scale_ref_cpu.py also runs the fast reference over
DOWNSAMPLE = {f"n{n}": (lambda n=n: random_cloud(n, 100 + n), 0.2, True) for n in (0, 1, 63, 64, 65, 4097)}
DOWNSAMPLE.update({
    "random_3000": (lambda: random_cloud(3000, 7), 0.2, True),
    "lattice_6": (lattice, 0.25, False),
    "lattice_6_shuffled": (lambda: np.random.default_rng(3).permutation(lattice()), 0.25, False),
    "duplicates_200": (lambda: np.tile(np.array([[0.5, -1.0, 2.0]], np.float32), (200, 1)), 0.1, False),
    "sorted_line_2000": (lambda: np.stack([np.arange(2000) * 0.6 * 0.2, np.zeros(2000), np.zeros(2000)], 1).astype(np.float32),
                         0.2, True),
})


def icosphere(subdiv, radius):
    """Icosahedron subdivided `subdiv` times: 20 * 4^subdiv triangles (3 -> 1,280)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def sphere_instance(seed=0, n_gt=20000, radius=10.0, noise=0.05):
    """The end-to-end case: a 1,280-triangle sphere, a noisy ground-truth cloud, a small mask, a plane through the centre."""
    rng = np.random.default_rng(seed)
    verts, tris = icosphere(3, radius)
    d = rng.normal(size=(n_gt, 3))
    stl = (d / np.linalg.norm(d, axis=1, keepdims=True) * (radius + rng.normal(scale=noise, size=(n_gt, 1)))).astype(np.float32)
    obs = (rng.random((9, 13, 14)) < 0.8).astype(np.uint8)
    bb = np.array([[-11.0, -11.5, -12.0], [5.0, 10.0, 11.0]], np.float32)
    return {"verts": verts, "tris": tris, "stl_points": stl, "obs_mask": obs, "bb": bb, "res": 2.0,
            "plane": np.array([0.0, 0.0, 1.0, 0.0]), "patch_size": 1.5, "downsample_density": 0.5, "max_dist": 20.0}
