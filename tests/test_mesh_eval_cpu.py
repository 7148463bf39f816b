"""DTU mesh evaluation without a device: the float64 restatement (tests/mesh_eval_ref.py) against scikit-learn's greedy loop
and the integer sampling rule, the *_host functions against the restatement, and the command line with --host on a generated
instance."""
import json
import os

import numpy as np
import pytest

import mesh_eval_ref as R
from gaussmart_amd import mesh_eval as ME
from gaussmart_amd.mesh import TriangleMesh


def _random_cloud(n, seed, neighbours=5.0, thresh=0.2):
    """n points in a cube whose side gives about `neighbours` points within thresh of each."""
    side = (n * 4.0 / 3.0 * np.pi * thresh ** 3 / neighbours) ** (1.0 / 3.0)
    return (np.random.default_rng(seed).random((n, 3)) * side).astype(np.float32)


def _lattice(k=6, thresh=0.25):
    g = np.arange(k, dtype=np.float32) * np.float32(thresh)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_greedy_equals_sklearn_radius_neighbors_loop():
    skln = pytest.importorskip("sklearn.neighbors")
    for pts, thresh in ((_random_cloud(3000, 1), 0.2), (_lattice(), 0.25),
                        (np.random.default_rng(5).permutation(_lattice(5, 0.5)), 0.5)):
        assert R.pair_margin(pts, thresh) > 1e-9 or thresh != 0.2
        eng = skln.NearestNeighbors(n_neighbors=1, radius=thresh, algorithm="kd_tree")
        p64 = pts.astype(np.float64)
        eng.fit(p64)
        idxs = eng.radius_neighbors(p64, radius=thresh, return_distance=False)
        mask = np.ones(len(pts), bool)
        for cur, ix in enumerate(idxs):
            if mask[cur]:
                mask[ix] = False
                mask[cur] = True
        assert np.array_equal(R.greedy_keep(pts, thresh), mask)


def test_sampling_counts_equal_integer_rule():
    for n1 in range(1, 80, 3):
        for n2 in range(1, 80, 7):
            # a right triangle with legs n1 + 0.5 and n2 + 0.5 at thresh = sqrt(sin) = 1: l / thr = n + 0.5
            verts = np.array([[0, 0, 0], [n1 + 0.5, 0, 0], [0, n2 + 0.5, 0]], np.float32)
            pairs, _ = R.sample_triangle(verts, (0, 1, 2), 1.0)
            assert pairs == R.integer_rule_pairs(n1, n2), (n1, n2)


def _mesh_fixture():
    rng = np.random.default_rng(3)
    verts = rng.random((60, 3)).astype(np.float32) * 2
    tris = rng.integers(0, 60, (80, 3)).astype(np.int32)
    tris[5] = (1, 1, 2)            # zero area
    tris[6] = (0, 1, 99)           # index out of range
    return verts, tris


def test_host_sampling_equals_restatement():
    verts, tris = _mesh_fixture()
    ref, counts = R.sample_mesh(verts, tris, 0.11)
    got = ME.sample_mesh_points_host(TriangleMesh(verts, tris), 0.11)
    assert counts.sum() > 500 and counts[5] == 0 and counts[6] == 0
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), ref.view(np.int32))


def test_host_downsample_equals_restatement():
    for pts, thresh in ((_random_cloud(2000, 2), 0.2), (_lattice(), 0.25), (np.zeros((50, 3), np.float32), 0.1),
                        (np.zeros((0, 3), np.float32), 0.1), (np.ones((1, 3), np.float32), 0.1)):
        assert np.array_equal(ME.downsample_points_host(pts, thresh), R.greedy_keep(pts, thresh))


def test_host_nearest_equals_restatement():
    rng = np.random.default_rng(4)
    q, c = rng.random((500, 3)).astype(np.float32), rng.random((700, 3)).astype(np.float32)
    d, i = ME.nearest_distance_host(q, c)
    rd, ri = R.nearest(q, c)
    safe = rd[:, 1] > rd[:, 0] * (1 + 1e-9)
    assert safe.sum() > 490 and np.array_equal(i[safe], ri[safe, 0])
    assert np.array_equal(d, np.sqrt(R.dist2(q, c[i])))
    assert np.abs(d - rd[:, 0]).max() <= 4 * np.spacing(rd[:, 0]).max()
    cut = float(np.median(rd[:, 0]))
    d2, i2 = ME.nearest_distance_host(q, c, cut)
    far = d >= cut
    assert 200 < far.sum() < 300 and np.isinf(d2[far]).all() and (i2[far] == -1).all()
    assert np.array_equal(d2[~far], d[~far]) and np.array_equal(i2[~far], i[~far])
    # ties: the smallest index wins, however many there are
    same = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (40, 1))
    d3, i3 = ME.nearest_distance_host(q[:10], same)
    assert (i3 == 0).all() and np.array_equal(d3, np.sqrt(R.dist2(q[:10], same[:1])))


def test_host_filters_equal_restatement():
    rng = np.random.default_rng(6)
    obs = (rng.random((8, 9, 10)) < 0.5).astype(np.uint8)
    bb = np.array([[1.0, 2.0, 3.0], [12.0, 14.0, 16.5]], np.float32)
    pts = (rng.random((3000, 3)) * 30 - 6).astype(np.float32)
    a, b, inb, ino = ME.filter_by_obs_mask_host(pts, obs, bb, 1.5, 2.0)
    rin, rio = R.obs_filter(pts, obs, bb, 1.5, 2.0)
    assert np.array_equal(inb, rin) and np.array_equal(ino, rio) and 100 < rio.sum() < rin.sum() < 3000
    assert np.array_equal(a, pts[rin]) and np.array_equal(b, pts[rio])
    plane = np.array([0.3, -0.2, 0.9, -4.0])
    assert np.array_equal(ME.filter_by_plane_host(pts, plane), R.plane_filter(pts, plane))
    assert np.isnan(ME.distance_mean_host(np.array([np.inf]))[0])


def write_instance(root, scan, inst):
    """A DTU-shaped evaluation instance on disk: ObsMask/ObsMask{scan}_10.mat, ObsMask/Plane{scan}.mat, Points/stl/...ply."""
    from scipy.io import savemat
    os.makedirs(os.path.join(root, "ObsMask"))
    savemat(os.path.join(root, "ObsMask", f"ObsMask{scan}_10.mat"),
            {"ObsMask": inst["obs_mask"], "BB": inst["bb"].astype(np.float64), "Res": np.array([[inst["res"]]])})
    savemat(os.path.join(root, "ObsMask", f"Plane{scan}.mat"), {"P": inst["plane"].reshape(4, 1)})
    TriangleMesh(inst["stl_points"]).write_ply(os.path.join(root, "Points", "stl", f"stl{scan:03}_total.ply"))


def test_cli_host_writes_results(tmp_path):
    from gaussmart_amd import dtu_eval_cli
    inst = R.sphere_instance(n_gt=3000)
    write_instance(str(tmp_path / "dtu"), 7, inst)
    mesh_path = str(tmp_path / "mesh.ply")
    TriangleMesh(inst["verts"], inst["tris"]).write_ply(mesh_path)
    out = str(tmp_path / "out")
    rc = dtu_eval_cli.main(["--data", mesh_path, "--scan", "7", "--dataset_dir", str(tmp_path / "dtu"), "--vis_out_dir", out,
                            "--downsample_density", "0.5", "--patch_size", "1.5", "--host", "--write_vis"])
    assert rc == 0
    with open(os.path.join(out, "results.json")) as f:
        res = json.load(f)
    assert set(res) == {"mean_d2s", "mean_s2d", "overall"}
    loaded = ME.load_dtu_eval_instance(str(tmp_path / "dtu"), 7)
    assert np.array_equal(loaded["obs_mask"], inst["obs_mask"]) and np.array_equal(loaded["bb"], inst["bb"])
    ref = ME.evaluate_dtu_mesh_host(TriangleMesh(inst["verts"], inst["tris"]), downsample_density=0.5, patch_size=1.5, **loaded)
    assert res["mean_d2s"] == ref["mean_d2s"] and res["mean_s2d"] == ref["mean_s2d"]
    assert 0 < res["mean_d2s"] < 1 and 0 < res["mean_s2d"] < 1 and res["overall"] == (res["mean_d2s"] + res["mean_s2d"]) / 2
    assert len(ME.read_points_ply(os.path.join(out, "vis_007_d2s.ply"))) == int(ref["keep"].sum())
    assert dtu_eval_cli.main(["--data", str(tmp_path / "missing.ply"), "--scan", "7", "--dataset_dir", str(tmp_path / "dtu"),
                              "--vis_out_dir", out, "--host"]) == 2
