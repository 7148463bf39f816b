"""Tanks-and-Temples evaluation without a device: the scalar restatement (tests/tnt_eval_ref.py) and the numpy host twins
(gaussmart_amd/tnt_eval.py) are shown to be the right rules -- the crossing rule against matplotlib, the voxel grid against
np.unique, Umeyama against a known similarity, the score against np.histogram and the reference's own comprehension, the
trajectory alignment against gross outliers, the whole host evaluation on a case whose answer is known, the loaders and the
command line."""
import json
import os

import numpy as np
import pytest

import tnt_eval_ref as R
from gaussmart_amd import tnt_eval as TE
from gaussmart_amd import tnt_eval_cli

CONVEX = np.array([[-3.0, -2.0, 0.0], [4.0, -3.0, 0.0], [5.0, 2.5, 0.0], [0.5, 4.0, 0.0], [-3.5, 1.0, 0.0]])


def _edge_distance(p2, poly2):
    """Smallest distance of every 2-D point to the polygon's edges."""
    best = np.full(len(p2), np.inf)
    for i in range(len(poly2)):
        a, b = poly2[i], poly2[(i + 1) % len(poly2)]
        ab = b - a
        t = np.clip(((p2 - a) @ ab) / (ab @ ab), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(p2 - (a + t[:, None] * ab), axis=1))
    return best


# ---------------------------------------------------------------- TNT_CROP
@pytest.mark.parametrize("name", ["convex", "concave"])
def test_crossing_rule_equals_matplotlib(name):
    mpath = pytest.importorskip("matplotlib.path")
    poly = CONVEX if name == "convex" else R.CONCAVE_XY
    rng = np.random.default_rng(3)
    pts = ((rng.random((3000, 3)) - 0.5) * (12 if name == "convex" else 24)).astype(np.float32)
    assert _edge_distance(pts[:, :2].astype(np.float64), poly[:, :2]).min() >= 1e-6      # the fixture's margin
    want = mpath.Path(poly[:, :2]).contains_points(pts[:, :2].astype(np.float64))
    assert 300 < want.sum() < 2700
    assert np.array_equal(R.crop_mask(pts, 2, -100.0, 100.0, poly), want)
    crop = {"orthogonal_axis": "Z", "axis_min": -100.0, "axis_max": 100.0, "bounding_polygon": poly}
    assert np.array_equal(TE.crop_mask_host(pts, crop), want)


def test_crop_host_twin_equals_restatement_on_every_axis():
    rng = np.random.default_rng(4)
    pts = ((rng.random((2000, 3)) - 0.5) * 24).astype(np.float32)
    for axis, name in enumerate("XYZ"):
        u, v = R.UV[axis]
        poly = np.zeros((len(R.CONCAVE_XY), 3))
        poly[:, u], poly[:, v] = R.CONCAVE_XY[:, 0], R.CONCAVE_XY[:, 1]
        crop = {"orthogonal_axis": name, "axis_min": 5.0, "axis_max": -6.0, "bounding_polygon": poly}     # min > max: swapped
        got = TE.crop_mask_host(pts, crop)
        assert np.array_equal(got, R.crop_mask(pts, axis, 5.0, -6.0, poly)) and 100 < got.sum() < 1500
        assert np.array_equal(TE.crop_points_host(pts, crop), pts[got])


# ---------------------------------------------------------------- TNT_VOXEL
def test_voxel_restatement_equals_unique_grouping():
    rng = np.random.default_rng(5)
    pts = ((rng.random((5000, 3)) - 0.3) * 4).astype(np.float32)
    size = 0.37
    out, row = R.voxel(pts, size)
    p = pts.astype(np.float64)
    cells = np.floor((p - (pts.min(0).astype(np.float64) - 0.5 * size)) / size).astype(np.int64)
    uniq, inv = np.unique(cells, axis=0, return_inverse=True)         # rows in lexicographic order: (ix, iy, iz) ascending
    inv = inv.reshape(-1)
    assert len(uniq) == len(out) and np.array_equal(inv, row)
    n = np.bincount(inv)
    assert n.max() > 3
    for a in range(3):
        mean = np.bincount(inv, p[:, a]) / n
        tol = n * 2.0 ** -53 * (np.bincount(inv, np.abs(p[:, a])) / n) + np.abs(mean) * 2.0 ** -24    # + the rounding to f32
        assert (np.abs(out[:, a].astype(np.float64) - mean) <= tol).all()
    host, hrow = TE.voxel_down_sample_host(pts, size, return_cells=True)
    assert np.array_equal(host, out) and np.array_equal(hrow, row)
    one = np.repeat(pts[:1], 300, 0)
    assert np.array_equal(TE.voxel_down_sample_host(one, size), R.voxel(one, size)[0])
    with pytest.raises(Exception, match="voxel_size"):
        TE.voxel_down_sample_host(pts, 1e-7)
    assert TE.voxel_down_sample_host(np.zeros((0, 3)), size).shape == (0, 3)


def test_uniform_down_sample_host():
    pts = np.arange(30, dtype=np.float32).reshape(10, 3)
    assert TE.uniform_stride(10, 4) == 2 and TE.uniform_stride(10, 10) == 0 and TE.uniform_stride(10, 2.5) == 4
    assert np.array_equal(TE.uniform_down_sample_host(pts, 4), pts[::2])
    assert np.array_equal(TE.uniform_down_sample_host(pts, 10), pts)


# ---------------------------------------------------------------- Umeyama
def test_umeyama_recovers_a_known_similarity():
    """Noise-free fp64 pairs t = S s.  What separates the result from S: the four sums carry a relative error of at most
    (n + 1) u each (u = 2^-53, n terms added, one product each); the SVD is backward stable, i.e. exact for a matrix within a
    few u of the cov it is given; the rotation is the orthogonal polar factor of cov = c R Scatter(s) / n, whose sensitivity to
    a relative perturbation e of cov is at most 2 kappa e with kappa the condition number of the centred source's scatter
    (R is orthogonal, so cov has Scatter's singular values times c).  With e <= (n + 16) u that gives
    |dR| <= 2 (n + 16) kappa u = (n + 16) kappa 2^-52; the scale is a ratio of two such sums (no kappa), and the translation
    t_mean - c R s_mean inherits (|dc| + c |dR|) |s_mean| plus its own rounding."""
    rng = np.random.default_rng(6)
    n = 200
    s = rng.normal(size=(n, 3)) * np.array([3.0, 1.0, 0.2]) + np.array([4.0, -2.0, 1.0])
    S = R.similarity(1.02, [0.4, 0.2, -0.9], 3.0, [0.5, -1.25, 2.0])
    t = R.apply64(S, s)
    ms, mt = s.mean(0), t.mean(0)
    ds, dt = s - ms, t - mt
    got = TE.umeyama_from_sums(n, ms, mt, dt.T @ ds, (ds * ds).sum())
    ev = np.linalg.eigvalsh(ds.T @ ds)
    kappa = ev[-1] / ev[0]
    tol = (n + 16) * kappa * 2.0 ** -52
    print(f"umeyama: kappa {kappa:.1f}, tol {tol:.2e}, error {np.abs(got - S).max():.2e}")
    assert kappa < 1e4
    assert np.abs(got[:3, :3] - S[:3, :3]).max() <= tol * 1.02
    assert np.abs(got[:3, 3] - S[:3, 3]).max() <= tol * 1.02 * (np.abs(ms).sum() + np.abs(mt).sum() + 1)
    assert np.array_equal(got[3], [0, 0, 0, 1])
    # a reflection is never returned, degenerate input gives the identity
    mirrored = TE.umeyama_from_sums(n, ms, mt, (dt * [1, 1, -1]).T @ ds, (ds * ds).sum())
    assert np.linalg.det(mirrored[:3, :3]) > 0
    assert np.array_equal(TE.umeyama_from_sums(2, ms, mt, dt.T @ ds, 1.0), np.eye(4))
    assert np.array_equal(TE.umeyama_from_sums(n, ms, mt, dt.T @ ds, 0.0), np.eye(4))


# ---------------------------------------------------------------- TNT_SCORE
def test_score_host_equals_histogram_and_the_comprehension():
    rng = np.random.default_rng(7)
    tau, stretch = 0.01, 5
    edges = TE.score_edges(tau, stretch)
    assert len(edges) == 500
    d = np.concatenate([rng.random(3000) * tau * 6, edges[[0, 1, 250, 498, 499]], [tau, np.nextafter(tau, 0), np.inf]])
    count, hist = TE.score_distances_host(d, tau, edges)
    assert count == sum(x < tau for x in d)                            # evaluation.py:183-186, literally
    assert np.array_equal(hist, np.histogram(d, edges)[0])
    rc, rh = R.score(d, tau, edges)
    assert rc == count and np.array_equal(rh, hist)
    assert hist[-1] >= 2 and hist.sum() < len(d)                       # the closed last bin, and values outside every bin


# ---------------------------------------------------------------- trajectories
def test_align_trajectories_ignores_gross_outliers():
    rng = np.random.default_rng(8)
    src = rng.normal(size=(30, 3)) * 3
    S = R.similarity(2.5, [0.1, 0.7, 0.3], 40.0, [3.0, 1.0, -2.0])
    dst = R.apply64(S, src)
    bad = [4, 17, 23]
    dst[bad] += rng.normal(size=(3, 3)) * 5 + 8
    T = TE.align_trajectories(src, dst)
    assert np.abs(T - S).max() < 1e-9
    assert np.abs(TE.align_trajectories(src, R.apply64(S, src)) - S).max() < 1e-9
    with pytest.raises(ValueError):
        TE.align_trajectories(src, dst[:-1])


def test_loaders_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    poses = np.tile(np.eye(4), (5, 1, 1))
    poses[:, :3, 3] = rng.normal(size=(5, 3))
    R.write_log(str(tmp_path / "t.log"), poses)
    assert np.array_equal(TE.read_trajectory_log(str(tmp_path / "t.log")), poses)
    assert np.array_equal(TE.camera_centres(poses), poses[:, :3, 3])
    inst = R.ellipsoid_instance(n_gt=50)
    gt_trans = R.similarity(1.0, [0, 0, 1], 10.0, [1.0, 2.0, 3.0])
    d = R.write_tnt_instance(str(tmp_path), "Barn", inst, poses, gt_trans)
    got = TE.load_tnt_instance(d)
    assert got["scene"] == "Barn" and np.array_equal(got["gt_points"], inst["gt_points"])
    assert got["crop"]["orthogonal_axis"] == "Z" and np.array_equal(got["crop"]["bounding_polygon"], R.CONCAVE_XY)
    assert np.allclose(got["gt_centres"], R.apply64(gt_trans, poses[:, :3, 3]), rtol=0, atol=1e-12)
    os.remove(os.path.join(d, "Barn_trans.txt"))
    with pytest.raises(FileNotFoundError):
        TE.load_tnt_instance(d)
    assert set(TE.SCENE_TAU) == {"Barn", "Caterpillar", "Church", "Courthouse", "Ignatius", "Meetingroom", "Truck"}
    assert TE.SCENE_TAU["Ignatius"] == 0.003 and TE.SCENE_TAU["Church"] == 0.025


# ---------------------------------------------------------------- ICP
def _icp_host():
    fx = R.icp_fixture()
    return fx, R.cached("icp_host", lambda: TE.registration_icp_host(fx["source"], fx["target"], fx["threshold"]))


def test_icp_host_converges_on_the_fixture():
    fx, h = _icp_host()
    assert 2 <= h["iterations"] < 20 and h["fitness"] == 1.0 and len(h["trace"]) == h["iterations"] + 1
    assert h["trace"][0][1] > 5 * h["inlier_rmse"]
    assert np.abs(h["transformation"] - fx["similarity"]).max() < 1e-3        # the noise of the fixture, 0.01 over 2,000 pairs
    empty = TE.registration_icp_host(fx["source"], fx["target"] + 100.0, fx["threshold"])
    assert empty["iterations"] == 0 and empty["fitness"] == 0.0 and np.array_equal(empty["transformation"], np.eye(4))
    none = TE.registration_icp_host(np.zeros((0, 3)), fx["target"], fx["threshold"])
    assert none["iterations"] == 0 and none["fitness"] == 0.0


def test_icp_sum_order_spread():
    """The noise floor of TNT_ICP_SUMS: the host twin over 20 random orders of adding the correspondences.  Measured here:
    2.0e-14 relative on the transformation's entries, 0 on the rmse; R.ICP_SPREAD records it and the device test holds the
    device to R.ICP_BAR_FACTOR x that.  A spread of 1e-9 or more would mean a badly conditioned fixture."""
    fx, h = _icp_host()
    spread = 0.0
    for k in range(20):
        g = TE.registration_icp_host(fx["source"], fx["target"], fx["threshold"], rng=np.random.default_rng(1000 + k))
        assert g["iterations"] == h["iterations"] and [c for c, _ in g["trace"]] == [c for c, _ in h["trace"]]
        spread = max(spread, np.abs(g["transformation"] - h["transformation"]).max() / np.abs(h["transformation"]).max(),
                     abs(g["inlier_rmse"] - h["inlier_rmse"]) / h["inlier_rmse"])
    print(f"icp spread over 20 orders: {spread:.3e} (recorded {R.ICP_SPREAD:.3e})")
    assert 0 < spread < 1e-9
    assert spread <= R.ICP_BAR_FACTOR * R.ICP_SPREAD


# ---------------------------------------------------------------- the whole evaluation, on a case whose answer is known
def test_host_evaluation_of_an_exact_subset():
    rng = np.random.default_rng(12)
    target = ((rng.random((20000, 3)) - 0.5) * 10).astype(np.float32)
    poly = np.array([[-3.0, -2.5, 0.0], [3.5, -3.0, 0.0], [3.0, 3.0, 0.0], [-2.5, 3.5, 0.0]])
    crop = {"orthogonal_axis": "Z", "axis_min": -3.0, "axis_max": 2.5, "bounding_polygon": poly}
    wide = {"orthogonal_axis": "Z", "axis_min": -3.5, "axis_max": 3.0, "bounding_polygon": poly * 1.15}
    # no point within 2e-5 of the crop volume's faces, 20 x the 1e-6 the alignment is held to below: the aligned source cannot
    # land on the other side of one
    t64 = target.astype(np.float64)
    assert _edge_distance(t64[:, :2], poly[:, :2]).min() > 2e-5 and np.abs(t64[:, 2:3] - [[-3.0, 2.5]]).min() > 2e-5
    inside, superset = TE.crop_mask_host(target, crop), TE.crop_mask_host(target, wide)
    assert 1000 < inside.sum() < superset.sum() < 20000 and (superset | ~inside).all()
    S = R.similarity(1.02, [0.3, 0.3, 0.9], 3.0, [0.4, -0.3, 0.2])
    source = R.apply64(np.linalg.inv(S), t64[superset]).astype(np.float32)
    init = R.similarity(1.0, [1, 0, 0], 0.0, [0.004, -0.003, 0.002]) @ S
    tau = 1e-3                                                         # f32 rounding of these coordinates: below 5e-7
    res = TE.evaluate_tnt_mesh_host(source, target, crop, tau, init)
    # (the first alignment is 5e-3 off, so the first registration's crop may differ near the faces; the last one's does not)
    assert res["registrations"][0]["fitness"] > 0.99 and res["registrations"][-1]["fitness"] == 1.0
    assert len(res["cloud_source"]) == len(res["cloud_target"]) == inside.sum()      # every point alone in its voxel
    assert res["precision"] == 1.0 and res["recall"] == 1.0 and res["fscore"] == 1.0
    assert np.abs(res["transformation"] - S).max() < 1e-6
    assert res["cum_source"][-1] == 1.0 and len(res["edges"]) == 500 and len(res["cum_target"]) == 499
    # an empty cloud: zeros, as the reference returns them
    far = TE.evaluate_histo_host(source + 100.0, target, init, crop, tau / 2, tau)
    assert (far["precision"], far["recall"], far["fscore"]) == (0.0, 0.0, 0.0)
    assert np.array_equal(far["edges"], [0]) and np.array_equal(far["cum_source"], [0])


# ---------------------------------------------------------------- command line
def _write_cli_case(tmp_path, scene):
    from gaussmart_amd.mesh import TriangleMesh
    inst = R.ellipsoid_instance(n_gt=1500)
    rng = np.random.default_rng(11)
    gt_trans = R.similarity(1.0, [0, 1, 0], 20.0, [0.5, 0.0, -0.5])
    # cameras around the ground truth; the COLMAP log holds them before gt_trans, the reconstruction's before `init`
    centres = rng.normal(size=(12, 3)) * 15
    poses_gt, poses_rec = np.tile(np.eye(4), (12, 1, 1)), np.tile(np.eye(4), (12, 1, 1))
    poses_gt[:, :3, 3] = R.apply64(np.linalg.inv(gt_trans), centres)
    poses_rec[:, :3, 3] = R.apply64(np.linalg.inv(inst["init"]), centres)
    d = R.write_tnt_instance(str(tmp_path), scene, inst, poses_gt, gt_trans)
    TriangleMesh(inst["verts"], inst["tris"]).write_ply(str(tmp_path / "mesh.ply"))
    R.write_log(str(tmp_path / "rec.log"), poses_rec)
    np.save(str(tmp_path / "rec.npy"), poses_rec)
    return inst, d


def test_cli_host_path_and_its_errors(tmp_path, capsys):
    from gaussmart_amd.mesh import TriangleMesh
    inst, d = _write_cli_case(tmp_path, "Sphere")
    common = ["--dataset-dir", d, "--ply-path", str(tmp_path / "mesh.ply"), "--host"]
    assert tnt_eval_cli.main(common + ["--traj-path", str(tmp_path / "rec.log")]) == 2
    err = capsys.readouterr().err
    assert "Sphere" in err and all(name in err for name in TE.SCENE_TAU)
    out = str(tmp_path / "out")
    assert tnt_eval_cli.main(common + ["--traj-path", str(tmp_path / "rec.log"), "--tau", "0.5", "--out-dir", out]) == 0
    with open(os.path.join(out, "results.json")) as f:
        res = json.load(f)
    init = TE.align_trajectories(TE.camera_centres(TE.read_trajectory_log(str(tmp_path / "rec.log"))),
                                 TE.load_tnt_instance(d)["gt_centres"])
    assert np.abs(init - inst["init"]).max() < 1e-9
    want = TE.evaluate_tnt_mesh_host(TriangleMesh(inst["verts"], inst["tris"]), inst["gt_points"], inst["crop"], 0.5, init)
    assert res["precision"] == want["precision"] and res["recall"] == want["recall"] and res["fscore"] == want["fscore"]
    assert 0.5 < res["fscore"] < 1.0 and res["tau"] == 0.5 and len(res["icp"]) == 3
    assert np.array_equal(np.array(res["transformation"]), want["transformation"])
    assert res["icp"][2]["trace"] == [[c, e] for c, e in want["registrations"][2]["trace"]]
    assert np.array_equal(np.loadtxt(os.path.join(out, "Sphere.precision.txt")), want["cum_source"])
    assert np.array_equal(np.loadtxt(os.path.join(out, "Sphere.recall.txt")), want["cum_target"])
    assert np.array_equal(np.loadtxt(os.path.join(out, "Sphere.prf_tau_plotstr.txt")),
                          [want["precision"], want["recall"], want["fscore"], 0.5, 5])
    # the .npy trajectory gives the same result in the default output directory; a .json trajectory is refused
    assert tnt_eval_cli.main(common + ["--traj-path", str(tmp_path / "rec.npy"), "--tau", "0.5"]) == 0
    with open(str(tmp_path / "evaluation" / "results.json")) as f:
        assert json.load(f) == res
    (tmp_path / "rec.json").write_text("{}")
    assert tnt_eval_cli.main(common + ["--traj-path", str(tmp_path / "rec.json"), "--tau", "0.5"]) == 2
    assert tnt_eval_cli.main(common + ["--traj-path", str(tmp_path / "missing.log"), "--tau", "0.5"]) == 2
