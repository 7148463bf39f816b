"""TEST-ONLY vectorised float64 restatements of EVAL_DOWNSAMPLE and TNT_VOXEL (include/gsr.h) for clouds of hundreds of
thousands of points, where the scalar loops of tests/mesh_eval_ref.py and tests/tnt_eval_ref.py take minutes.  They state the
same rules with the same float64 expressions; tests/test_cloud_scale_ref_cpu.py holds them to the scalar ones bit for bit on
every fixture of the two GPU modules.  (EVAL_NN needs nothing new: mesh_eval_ref.nearest is cKDTree's own query.)
fixed_order_sum states the one summation order of EVAL_MEAN, SEG_MEANSTD and TNT_ICP_SUMS, held to a scalar loop there too."""
import numpy as np
from scipy.spatial import cKDTree

from mesh_eval_ref import cached, dist2, nearest, pair_margin  # noqa: F401  (what the large cases need, in one place)


def greedy_keep_fast(points, thresh):
    """mesh_eval_ref.greedy_keep: point i is kept iff no kept j < i has d2 <= thresh^2 by EVAL_DIST.  The pairs come from one
    cKDTree.query_pairs (a little wider than thresh, then filtered by EVAL_DIST itself) and are grouped by their higher index;
    the decisions are one sequential pass, because keep[i] hangs on every earlier one."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    keep = np.ones(n, bool)
    if n < 2:
        return keep
    pairs = cKDTree(p).query_pairs(thresh * (1 + 1e-9), output_type="ndarray")
    pairs = pairs[dist2(p[pairs[:, 0]], p[pairs[:, 1]]) <= thresh * thresh]
    lower, higher = pairs.min(1), pairs.max(1)
    order = np.argsort(higher, kind="stable")
    lower, higher = lower[order], higher[order]
    start = np.searchsorted(higher, np.arange(n + 1))
    for i in np.unique(higher).tolist():
        keep[i] = not keep[lower[start[i]:start[i + 1]]].any()
    return keep


def voxel_fast(points, voxel_size):
    """tnt_eval_ref.voxel: (f32 [cells,3] in ascending (ix, iy, iz), int32 [n] output row of every point).  ValueError for an
    index outside [0, 2^21).  Every cell is summed sequentially in ascending input index -- np.add.at adds one element after
    the other in the order given, which a pairwise `sum` would not."""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    n = len(p)
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    lo = np.array([float(p32[:, a].min()) - 0.5 * voxel_size for a in range(3)])
    with np.errstate(all="ignore"):
        c = np.floor((p - lo[None, :]) / voxel_size)
    if not ((c >= 0) & (c < 2 ** 21)).all():
        raise ValueError("voxel_size")
    c = c.astype(np.int64)
    order = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))                 # stable: ascending input index inside a cell
    cs = c[order]
    head = np.ones(n, bool)
    head[1:] = (cs[1:] != cs[:-1]).any(1)
    row = np.empty(n, np.int64)
    row[order] = np.cumsum(head) - 1
    cells = int(head.sum())
    acc = np.zeros((cells, 3), np.float64)
    for a in range(3):
        np.add.at(acc[:, a], row, p[:, a])                          # unbuffered: element by element, k = 0, 1, 2, ...
    count = np.bincount(row, minlength=cells).astype(np.float64)
    return (acc / count[:, None]).astype(np.float32), row.astype(np.int32)


def wide_values(n, seed):
    """finite, non-negative, seventeen decades wide: the low bits of any sum depend on its order"""
    rng = np.random.default_rng(seed)
    return rng.random(n) * 10.0 ** rng.integers(-8, 9, size=n)


def _tree_256(acc):
    """acc [rows, 256] -> [rows]: column t += column t + d for d = 128, 64, ..., 1"""
    acc = acc.copy()
    d = 128
    while d:
        acc[:, :d] += acc[:, d:2 * d]
        d //= 2
    return acc[:, 0]


def fixed_order_sum(x):
    """The fixed-order float64 sum of the device (include/gsr.h, EVAL_MEAN): min(1024, ceil(n / 256)) workgroups of 256 threads,
    thread t of workgroup b adds x[b * 256 + t], x[b * 256 + t + blocks * 256], ... to 0.0 in that order; a tree adds the 256
    values of a workgroup; one workgroup adds the partials the same way (thread t takes partials t, t + 256, ...).  The
    missing elements of the last trip are +0.0, which changes no sum of values that are not -0.0."""
    x = np.asarray(x, np.float64).reshape(-1)
    n = len(x)
    blocks = min(1024, -(-n // 256))
    if blocks == 0:
        return 0.0

    def threads(v, width):                                  # [trips, width] added trip after trip
        trips = -(-len(v) // width)
        rows = np.concatenate([v, np.zeros(trips * width - len(v))]).reshape(trips, width)
        acc = np.zeros(width)
        for r in rows:
            acc = acc + r
        return acc

    partial = _tree_256(threads(x, blocks * 256).reshape(blocks, 256))
    return float(_tree_256(threads(partial, 256).reshape(1, 256))[0])
