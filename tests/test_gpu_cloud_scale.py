"""The point-cloud kernels beyond one trip of their capped grids and with more than one box on the top level of the search
tree, against the vectorised float64 references of tests/cloud_scale_ref.py (pinned to the scalar restatements bit for bit by
tests/test_cloud_scale_ref_cpu.py), cKDTree and numpy.  No bar here is new: each is the one the suite applies to the same
function at a smaller size, or exact equality.  N_TOP = 64^3 = 262 144 = 1 024 workgroups x 256 threads is both lines at once.

Where every capped grid and every level constant changes path, and the tests on either side of it
(ME = test_gpu_mesh_eval, TN = test_gpu_tnt_eval, SI = test_gpu_segment_init, KN = test_gpu_sort_knn, MV = test_gpu_mesh_vis,
here = this module):

  constant / grid                        path changes at                      below                             above
  -------------------------------------  -----------------------------------  --------------------------------  ------------------------------------
  cloud_common.h (one copy for knn.hip, mesh_eval.hip, tnt_eval.hip and seg_init.hip)
    cloud_bounds_kernel<true> on         262 145 points                       KN knn 200 000, here knn N_TOP,   here knn N_TOP + 1, 300 * 1024 + 1,
      gsr_partial_blocks, 1 024 x 256                                         here nearest N_TOP                nearest N_TOP + 1 (corner point last)
    cloud_bounds_kernel<false>           262 145 points                       TN voxel n20000                   here voxel N_TOP + 1, 2 N_TOP + 3
    gsr_block_sum_256: second thread     2 values                             here fixed_order_sums 1           here fixed_order_sums 255
      second workgroup                   257 values                           ME distance_mean 255, 256         here fixed_order_sums 257, ME distance_mean 257
      final workgroup's second trip      257 partials = 65 537 values         TN icp_sums 20000                 here fixed_order_sums 65 537, icp_sums N_TOP
      gsr_partial_blocks, 1 024 x 256    262 145 values                       ME distance_mean N_TOP            here fixed_order_sums N_TOP + 1; ME distance_mean
                                                                                                                N_TOP + 1, 300 001
  mesh_eval.hip
    ME_LEAF: second leaf                 65 points                            ME downsample n63, n64            ME downsample n65
    ME_LEAF^2: second node               4 097 points                         ME random_3000                    ME downsample n4097, nearest 4097 x 5000
    ME_LEAF^3: second top box            262 145 points (nt = 2)              here nearest N_TOP                here nearest / downsample N_TOP + 1
    ne = min(T.nn, ...): ragged last     a last top box that is not full      here nearest N_TOP (full box)     here nearest N_TOP + 1 (one node, one leaf,
      top box                                                                                                   one point), 2 N_TOP + 4096 + 65 (nt = 3)
    queries: m = max(n, nq), qorder      nq > n; 262 145 queries              ME nearest 4097 x 5000, 5000 x 1  here 300 000 queries x N_TOP + 1
    ME_MIS_BATCH: second read-back       9 rounds                             ME downsample n1 (one round)      ME sorted_line_2000 (>= 100 rounds)
    ext > 0 ? ... : 0 (flat axis)        an axis without extent               every other cloud                 here collapse flat_z, line_x; ME nearest 5000 x 1
  knn.hip
    KNN_BOX: second box                  1 025 points                         KN knn 4, 1000                    KN knn 3000, 20 000, 200 000
    ragged last box beyond one trip      300 * 1024 + 1 points                here knn N_TOP (full boxes)       here knn 300 * 1024 + 1
    ext > 0 ? ... : 0 (flat axis)        an axis without extent               every other cloud                 KN knn planar; here collapse flat_z, line_x
  tnt_eval.hip
    te_sums_kernel's own loop            262 145 source points                TN icp_sums 20000, here N_TOP     here icp_sums N_TOP + 1, 2 N_TOP + 257
    te_score_kernel, 1 024 x 256         262 145 distances                    TN score 20000                    here score N_TOP + 1, 2 N_TOP + 3
    TE_MAX_BINS                          4 097 bins (refused)                 TN score B = 4096                 TN score_refuses_too_many_bins
    TE_MAX_POLY                          257 vertices (refused)               TN crop_polygon_sizes 256         TN crop_polygon_sizes 257
    TE_CELL_LIMIT                        2^21 cells on an axis (refused)      TN voxel 10 / 2^20                TN voxel_refuses_too_many_cells
  seg_init.hip
    seg_sum_partial_kernel's own loop    262 145 distances                    SI mean_std filter (20 300)       SI mean_std_edges 300 000;
                                                                                                                here mean_std N_TOP + 1, 2 N_TOP + 3
    seg_box_kernel, 1 024 x 256          262 145 points                       SI project_points_sizes tyt       here project tyt N_TOP + 1, 2 N_TOP + 3
    seg_dtu_count_kernel, 1 024 x 256    262 145 points                       SI project_points_sizes dtu       here project dtu N_TOP + 1, 2 N_TOP + 3
    SEG_FACET_CHUNK                      513 facets                           SI hull gauss (600 points)        SI hull sphere, filter
  mesh_vis.hip
    MV_SMALL                             a pixel box of 9 x 8                 MV single_triangle 8 x 8          MV single_triangle 9 x 8
    MV_LARGE_BLOCKS                      2 049 large (triangle, view) pairs   MV two_spheres (a few large)      MV depth_interval_many_large_pairs
    MV_VOTE_VIEWS                        65 views                             MV vote n = 8                     MV vote_special_vertices (72 views)

The search results never depend on how good the Morton codes are -- only the time does -- so the far outlier and the flat
clouds hold that exactness to the same bars.  For the same reason no result of a search can tell whether
cloud_bounds_kernel<true> saw the whole cloud (a point outside the bounds is clamped into them): these cases run their second trip
with the box's corner in it, and hold what is computed from it to the bars; the voxel grid runs the same loop and does show it.
The second trips of cloud_bounds_kernel<false>, te_sums_kernel, te_score_kernel, seg_sum_partial_kernel, seg_box_kernel and
seg_dtu_count_kernel each decide a result here.  The last 200 points of the nearest-neighbour clouds are placed in the corner
cell of the box: they have the highest codes, so they are the ragged tail of the sorted order, which the test asserts."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import cloud_scale_ref as F
import mesh_eval_ref as R
import segment_cases as SC
import tnt_eval_ref as TN
from gaussmart_amd import segment_init as SI
from gaussmart_amd import tnt_eval as TE
from test_gpu_mesh_eval import _check_nearest, _dev, _random_cloud
from test_gpu_tnt_eval import check_icp_sums
from test_segment_init_cpu import G, camera  # noqa: F401  (G is a fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N_TOP = 64 ** 3
ULP = 2.0 ** -52
TAIL = 200


# ---------------------------------------------------------------- nearest neighbour: tree levels, query side
def _corner_tail_cloud(n, seed):
    """n uniform points of the unit cube whose last TAIL points lie in the corner cell at (1, 1, 1), the very last one on the
    corner itself: it alone has the highest code on all three axes."""
    rng = np.random.default_rng(seed)
    cloud = rng.random((n, 3)).astype(np.float32)
    cloud[-TAIL:] = (0.9992 + 0.0008 * rng.random((TAIL, 3))).astype(np.float32)
    cloud[-1] = 1.0
    # the tail's cell index is >= every other point's on every axis, and nobody else is in the tail's cell: whatever the
    # order of the interleaved bits, the tail sorts last
    q = np.floor((cloud - cloud.min(0)) / (cloud.max(0) - cloud.min(0)) * np.float32(1023.0))
    assert (q[-TAIL:] >= 1022).all() and not (q[:-TAIL] >= 1022).all(1).any() and (q[-1] == 1023).all()
    return cloud, rng


def _assert_tail_found(d, i, n):
    assert not d[-TAIL:].any() and np.array_equal(i[-TAIL:], np.arange(n - TAIL, n))


@pytest.mark.parametrize("n", [N_TOP, N_TOP + 1, 2 * N_TOP + 4096 + 65])
def test_nearest_tree_levels(n):
    cloud, rng = _corner_tail_cloud(n, 300 + n % 1000)
    far = (rng.random((300, 3)) * 2 - 1).astype(np.float32) * 100 + np.float32(0.5)
    query = np.concatenate([rng.random((5000, 3)).astype(np.float32), far, cloud[-TAIL:]], 0)
    d, i, _ = _check_nearest(query, cloud)
    assert np.isfinite(d).all()
    _assert_tail_found(d, i, n)
    cut_at = float(np.median(d)) * (1 + 1e-6)
    d, i, n_cut = _check_nearest(query, cloud, cut_at)
    assert abs(n_cut - len(query) / 2) <= 1
    _assert_tail_found(d, i, n)
    print(f"nearest {len(query)} x {n}: nt = {-(-n // N_TOP)}, median {np.median(d[np.isfinite(d)]):.5f}, {n_cut} cut at {cut_at:.5f}")


def test_nearest_more_queries_than_points():
    n, nq = N_TOP + 1, 300000
    cloud, rng = _corner_tail_cloud(n, 41)
    query = (rng.random((nq, 3)) * 1.2 - 0.1).astype(np.float32)           # a tenth of the box's side beyond it, all round
    query[-TAIL:] = cloud[-TAIL:]
    d, i, _ = _check_nearest(query, cloud)
    assert np.isfinite(d).all()
    _assert_tail_found(d, i, n)
    cut_at = float(np.median(d)) * (1 + 1e-6)
    _, _, n_cut = _check_nearest(query, cloud, cut_at)
    assert abs(n_cut - nq / 2) <= 1


# ---------------------------------------------------------------- down-sampling with a second top box
def test_downsample_second_top_box():
    """Seed 10: the point with the highest code (the only one of the second top box) is kept and is the only kept lower
    neighbour of two other points, so a traversal that stops after the first top box keeps two points too many."""
    from gaussmart_amd.mesh_eval import downsample_points
    pts, thresh = _random_cloud(N_TOP + 1, 10), 0.2
    assert R.pair_margin(pts, thresh) > 1e-9                # change the seed if this fails, never the bar
    ref = F.greedy_keep_fast(pts, thresh)
    p = _dev(pts)
    keep, rounds = downsample_points(p, thresh, return_rounds=True)
    keep = keep.cpu().numpy()
    print(f"downsample {len(pts)}: {int(ref.sum())} kept, {rounds} rounds, {int((keep != ref).sum())} differ")
    assert keep.dtype == bool and np.array_equal(keep, ref)
    assert np.array_equal(downsample_points(p, thresh).cpu().numpy(), keep)


# ---------------------------------------------------------------- Morton codes that say nothing
def _collapse_cloud(kind):
    """(cloud, thresh with about 5 neighbours per ball, the box the near queries are drawn from)"""
    rng = np.random.default_rng({"outlier": 1, "flat_z": 2, "line_x": 3}[kind])
    n, t = 20000, 0.2
    if kind == "outlier":                                   # every other point falls into one 10-bit cell per axis
        cloud = np.concatenate([rng.random((n, 3)), [[1e4, 1e4, 1e4]]], 0).astype(np.float32)
        return cloud, (5.0 * 3 / (4 * np.pi * n)) ** (1 / 3), np.ones(3)
    side = np.sqrt(n * np.pi * t * t / 5) if kind == "flat_z" else 2 * t * n / 5
    cloud = (rng.random((n, 3)) * side).astype(np.float32)
    cloud[:, (2 if kind == "flat_z" else 1):] = 0.0
    return cloud, t, np.array([side, side if kind == "flat_z" else 1.0, 1.0])


@pytest.mark.parametrize("kind", ["outlier", "flat_z", "line_x"])
def test_code_collapse_nearest(kind):
    cloud, _, box = _collapse_cloud(kind)
    rng = np.random.default_rng(50)
    far = (rng.random((300, 3)) * 2 - 1).astype(np.float32) * 100 * np.float32(box.max()) + np.float32(0.5)
    query = np.concatenate([((rng.random((2000, 3)) * 1.2 - 0.1) * box).astype(np.float32), far, cloud[-TAIL:]], 0)
    d, i, _ = _check_nearest(query, cloud)
    assert np.isfinite(d).all() and not d[-TAIL:].any()
    _, _, n_cut = _check_nearest(query, cloud, float(np.median(d)) * (1 + 1e-6))
    assert abs(n_cut - len(query) / 2) <= 1


@pytest.mark.parametrize("kind", ["outlier", "flat_z", "line_x"])
def test_code_collapse_downsample(kind):
    from gaussmart_amd.mesh_eval import downsample_points
    cloud, thresh, _ = _collapse_cloud(kind)
    assert R.pair_margin(cloud, thresh) > 1e-9
    ref = F.greedy_keep_fast(cloud, thresh)
    p = _dev(cloud)
    keep, rounds = downsample_points(p, thresh, return_rounds=True)
    keep = keep.cpu().numpy()
    print(f"downsample {kind}: {int(ref.sum())} of {len(cloud)} kept, {rounds} rounds")
    assert 0.2 * len(cloud) < ref.sum() < 0.8 * len(cloud)
    assert np.array_equal(keep, ref)
    assert np.array_equal(downsample_points(p, thresh).cpu().numpy(), keep)


def _check_knn(pts):
    from simple_knn._C import distCUDA2
    out = distCUDA2(torch.from_numpy(pts).to(DEV)).cpu().numpy()
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4)
    np.testing.assert_allclose(out, (d[:, 1:] ** 2).mean(1), rtol=2e-5, atol=1e-12)


@pytest.mark.parametrize("kind", ["outlier", "flat_z", "line_x"])
def test_code_collapse_knn(kind):
    _check_knn(_collapse_cloud(kind)[0])


# ---------------------------------------------------------------- KNN beyond one trip of the bounds grid
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("n", [N_TOP, N_TOP + 1, 300 * 1024 + 1])
def test_knn_beyond_one_grid_trip(n, kind):
    rng = np.random.default_rng(n)
    if kind == "uniform":
        pts = rng.uniform(-5, 5, size=(n, 3))
    else:
        pts = rng.normal(size=(n, 3)) * 0.01 + rng.integers(0, 5, size=(n, 1)) * 3.0
    pts[-1] = pts.max(0) + 0.25                             # the box's upper corner comes last: beyond the first trip
    _check_knn(pts.astype(np.float32))


# ---------------------------------------------------------------- voxel grid
@pytest.mark.parametrize("n,size", [(N_TOP + 1, 0.2), (2 * N_TOP + 3, 0.16)])
def test_voxel_beyond_one_grid_trip(n, size):
    pts = TN.cloud(n, 60 + n % 1000, 10.0)
    pts[-1] = pts.min(0) - np.array([0.37, 0.41, 0.29], np.float32)       # the grid's origin: seen by the second trip only
    assert (pts.argmin(0) >= N_TOP).all()
    want, row = F.voxel_fast(pts, size)
    print(f"voxel {n}: {len(want)} cells")
    assert n / 20 < len(want) < n / 2
    p = _dev(pts)
    got, cells = TE.voxel_down_sample(p, size, return_cells=True)
    got, cells = got.cpu().numpy(), cells.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cells, row)
    again, cells2 = TE.voxel_down_sample(p, size, return_cells=True)
    assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32)) and np.array_equal(cells2.cpu().numpy(), cells)
    host, hrow = TE.voxel_down_sample_host(pts, size, return_cells=True)
    assert np.array_equal(host.view(np.uint32), got.view(np.uint32)) and np.array_equal(hrow, row)


# ---------------------------------------------------------------- ICP sums
@pytest.mark.parametrize("n,pairs_from", [(N_TOP, 0), (N_TOP + 1, 0), (2 * N_TOP + 257, 0), (N_TOP + 5000, N_TOP)])
def test_icp_sums_beyond_one_grid_trip(n, pairs_from):
    pairs = check_icp_sums(n, pairs_from, pair_at_end=True)          # N_TOP + 1: the second trip's only point counts
    assert pairs > 0.6 * (n - pairs_from)


# ---------------------------------------------------------------- score
@pytest.mark.parametrize("B", [1, 499, 4096])
def test_score_beyond_one_grid_trip(B):
    rng = np.random.default_rng(80 + B)
    tau = 0.01
    edges = TE.score_edges(tau, 5) if B == 499 else np.sort(rng.random(B + 1)) * 0.05 + 0.001
    assert len(edges) == B + 1
    for n in (N_TOP + 1, 2 * N_TOP + 3):
        d = rng.random(n) * 0.06
        if n == N_TOP + 1:                                  # one value beyond the first trip: it decides a bin or the count
            d[N_TOP] = {1: np.nextafter(tau, 0), 499: edges[-1], 4096: edges[0]}[B]
        else:
            k, o = min(n // 4, B + 1), N_TOP
            d[o:o + k] = edges[rng.integers(0, B + 1, size=k)]                         # exactly on edges
            d[o + k:o + k + 5] = edges[-1]                                             # the last edge: in the last bin
            d[o + k + 5:o + k + 10] = np.nextafter(edges[-1], 1)                       # just above: in no bin
            d[o + k + 10:o + k + 15] = np.inf
            d[o + k + 15:o + k + 20] = [tau, np.nextafter(tau, 0), np.nextafter(tau, 1), edges[0], np.nextafter(edges[0], 0)]
        dd = _dev(d, np.float64)
        count, hist = TE.score_distances(dd, tau, edges)
        assert count == int((d < tau).sum())
        assert hist.dtype == np.int64 and np.array_equal(hist, np.histogram(d, edges)[0])
        if n > N_TOP + 1:
            assert hist[-1] >= 5 and hist.sum() < n
        assert TE.score_distances(dd, tau, edges)[1].tolist() == hist.tolist()
        assert TE.score_distances_host(d, tau, edges)[0] == count


# ---------------------------------------------------------------- one fixed-order sum behind EVAL_MEAN and SEG_MEANSTD
@pytest.mark.parametrize("n", [1, 255, 257, 65537, N_TOP + 1])
def test_fixed_order_sums_agree(n):
    """gsr_dist_mean and gsr_seg_mean_std add the same vector in the same order (gsr_block_sum_256): their means are one bit
    pattern, and it is the one of the restated order.  n: one thread, one short workgroup, two workgroups, 257 partials (the
    final workgroup's second trip), the capped grid's second trip."""
    from gaussmart_amd.mesh_eval import distance_mean
    x = F.wide_values(n, 501 + n)                          # change the seed if the last assertion fails, never the bar
    d = _dev(x, np.float64)
    mean, count = distance_mean(d)
    seg = float(SI.mean_std(d).cpu().numpy()[0])
    want = F.fixed_order_sum(x) / n
    bits = lambda v: int(np.float64(v).view(np.uint64))
    print(f"fixed order {n}: dist_mean {mean!r}, seg_mean_std {seg!r}, restated {want!r}, sequential {np.cumsum(x)[-1] / n!r}")
    assert count == n
    assert bits(mean) == bits(seg) == bits(want)
    if n >= 255:
        assert float(np.cumsum(x)[-1]) != F.fixed_order_sum(x)       # the vector tells one order from another


# ---------------------------------------------------------------- segment init: mean / std, bounding box, DTU in-view count
@pytest.mark.parametrize("n", [N_TOP + 1, 2 * N_TOP + 3])
def test_segment_mean_std_beyond_one_grid_trip(n):
    x = SC.uniform(n, 1, 3)[:, 0]
    x[N_TOP:] += 3.0                                        # the second trip's share moves both figures
    ms = SI.mean_std(_dev(x, np.float64)).cpu().numpy()
    ld = x.astype(np.longdouble)
    mean = ld.sum() / n
    std = np.sqrt(((ld - mean) ** 2).sum() / n)
    rel = 4.0 * 2.0 ** -53 * np.sqrt(n)
    assert abs(ms[0] - mean) <= rel * mean and abs(ms[1] - std) <= rel * std


def _check_projection(G, pts, cam, kind):
    """test_gpu_segment_init.py::test_project_points_sizes' bars for one cloud handed over as float64 and as float32 (pts holds
    float32 values, so both are the same points)."""
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts, equal_nan=True)
    uv_ld, z_ld = SC.project_ld(pts, SI.camera_terms(cam, kind))
    fin = np.isfinite(uv_ld.astype(np.float64)).all(axis=1) & np.isfinite(z_ld.astype(np.float64))
    big_mag = max(float(np.abs(uv_ld[fin]).max()), float(np.abs(z_ld[fin]).max()))
    tol = 4.0 * max(float(G[f"eref_proj_kind_{kind}"]), ULP * 2.0 ** np.floor(np.log2(big_mag)))
    a = SI.project_points(pts, cam, kind, device=DEV)
    uv, z = (t.cpu().numpy() for t in a)
    print(f"{kind} {len(pts)}: |uv - ld| {SC.max_dev(uv, uv_ld):.3g}, |z - ld| {SC.max_dev(z, z_ld):.3g}, tol {tol:.3g}")
    assert np.array_equal(np.isnan(z), np.isnan(z_ld.astype(np.float64)))
    assert SC.max_dev(uv, uv_ld) <= tol and SC.max_dev(z, z_ld) <= tol
    b = SI.project_points(pts.astype(np.float32), cam, kind, device=DEV)
    assert torch.equal(a[0].nan_to_num(7.0), b[0].nan_to_num(7.0)) and torch.equal(a[1].nan_to_num(7.0), b[1].nan_to_num(7.0))
    return uv, z


def _blob32(n):
    return (SC.blob(n, 8) * 0.6).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n", [N_TOP + 1, 2 * N_TOP + 3])
def test_segment_tyt_box_beyond_one_grid_trip(G, n):
    pts = _blob32(n)
    pts[17, 1] = np.nan                                     # a row with a NaN takes no part in the box
    first = pts[:N_TOP][np.isfinite(pts[:N_TOP]).all(1)]
    pts[-1] = (first.max(0) + 1.5).astype(np.float32)       # the box's upper corner and, for the larger cloud, its lower one:
    if n > N_TOP + 1:                                       # only the second trip sees them
        pts[-2] = (first.min(0) - 1.25).astype(np.float32)
    uv, _ = _check_projection(G, pts, camera(G, "tyt"), "tyt")
    w, h = (float(v) for v in np.asarray(camera(G, "tyt")["img_size"]).reshape(-1)[:2])
    assert abs(uv[-1, 0] - 0.9 * w) < 1e-6 and abs(uv[-1, 1] - 0.9 * h) < 1e-6       # the corner maps to the padded frame's corner


def _dtu_cloud(G, in_view):
    """A cloud whose row k projects into the 1554 x 1162 frame of the "dtu" camera iff in_view[k], each by more than 1e-3
    pixel in longdouble: rows of the blob where in_view, the blob moved 2.5 units (some 250 pixels) out of the frame elsewhere -- no farther, so that the
    largest coordinate, which sets the bar, stays that of the existing cases."""
    n = len(in_view)
    terms = SI.camera_terms(camera(G, "dtu"), "dtu")
    base = _blob32(n)
    pts = np.where(in_view[:, None], base, (base + np.array([-2.5, 0.0, 0.0])).astype(np.float32).astype(np.float64))
    for _ in range(2):                                      # the blob's few rows outside the frame: take a row that is inside
        uv, _z = SC.project_ld(pts, terms, fallback=False)
        u, v = uv[:, 0], uv[:, 1]
        inside = (u >= 1e-3) & (u < 1554 - 1e-3) & (v >= 1e-3) & (v < 1162 - 1e-3)
        outside = (u < -1e-3) | (u >= 1554 + 1e-3) | (v < -1e-3) | (v >= 1162 + 1e-3)
        wrong = np.nonzero(in_view & ~inside)[0]
        pts[wrong] = pts[np.nonzero(in_view & inside)[0][:len(wrong)]]
    assert np.array_equal(inside, in_view) and np.array_equal(outside, ~in_view)
    return pts


DTU_CASES = {
    # 0.1 n = 26 214.5: 26 215 rows in view keep the pinhole projection, and the last of them is row N_TOP
    "one_trip_plus_one_decides": (N_TOP + 1, lambda k: (k % 10 == 0) & (k < 262140) | (k == N_TOP), 26215, False),
    # the same without that row: 26 214 < 26 214.5, the view falls back to normalised rays
    "one_short_falls_back": (N_TOP + 1, lambda k: (k % 10 == 0) & (k < 262140), 26214, True),
    # 0.1 n = 52 429.1: every row in view lies beyond the first trip
    "all_in_view_rows_beyond_first_trip": (2 * N_TOP + 3, lambda k: (k >= N_TOP) & (k < N_TOP + 52430), 52430, False),
}


@pytest.mark.parametrize("name", list(DTU_CASES))
def test_segment_dtu_count_beyond_one_grid_trip(G, name):
    n, rule, count, fallback = DTU_CASES[name]
    in_view = rule(np.arange(n))
    assert in_view.sum() == count and (count < 0.1 * n) == fallback and abs(count - 0.1 * n) < 1
    pts = _dtu_cloud(G, in_view)
    cam = camera(G, "dtu")
    uv, _ = _check_projection(G, pts, cam, "dtu")
    # the decision itself: without the fallback the result is the pinhole projection, with it something else by many pixels
    pinhole = SC.project_ld(pts, SI.camera_terms(cam, "dtu"), fallback=False)[0]
    assert (SC.max_dev(uv, pinhole) > 100.0) == fallback
