"""Tanks-and-Temples mesh evaluation on the device against the scalar restatement (tests/tnt_eval_ref.py) and the host twins:
face centres, transform, crop and voxel grid bit for bit, the ICP sums within the bound of their fixed-order reduction, the
score against np.histogram, ICP and the whole evaluation against the host twin on fixtures whose margins are asserted first,
the command line and the error paths."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import tnt_eval_ref as R
from gaussmart_amd import tnt_eval as TE

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES, _cloud = R.SIZES, R.cloud


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


# ---------------------------------------------------------------- 1. TNT_CLOUD, TNT_TRANSFORM
@pytest.mark.parametrize("n", SIZES)
def test_face_centres_and_transform_bit_for_bit(n):
    from gaussmart_amd.mesh import DeviceTriangleMesh, TriangleMesh
    rng = np.random.default_rng(20 + n)
    verts = _cloud(max(n // 2, 3), 30 + n)
    tris = rng.integers(0, len(verts), size=(n, 3)).astype(np.int32)
    want = np.concatenate([verts, R.face_centres(verts, tris)], 0)
    got = TE.mesh_to_cloud(DeviceTriangleMesh(_dev(verts), _dev(tris, np.int32)))
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(TE.mesh_to_cloud(TriangleMesh(verts, tris), device=DEV).cpu().numpy(), want)
    assert np.array_equal(TE.mesh_to_cloud_host(TriangleMesh(verts, tris)), want)
    T = R.similarity(1.02, [0.3, -0.2, 0.9], 33.0, [0.7, -11.0, 3.5])
    pts = _cloud(n, 40 + n)
    moved = TE.transform_points(_dev(pts), T).cpu().numpy()
    assert np.array_equal(moved.view(np.uint32), R.transform(pts, T).view(np.uint32))
    assert np.array_equal(TE.transform_points_host(pts, T), moved)


def test_cloud_and_transform_refuse_bad_input():
    from gaussmart_amd.mesh import DeviceTriangleMesh
    verts = _cloud(5, 1)
    for bad in ([[0, 1, 5]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match="outside"):
            TE.mesh_to_cloud(DeviceTriangleMesh(_dev(verts), _dev(bad, np.int32)))
    T = np.eye(4)
    T[3, 0] = 1e-3
    with pytest.raises(ValueError, match="last row"):
        TE.transform_points(_dev(verts), T)


# ---------------------------------------------------------------- 2. TNT_CROP
def _crop_points(axis, poly, lo, hi, seed):
    """Random points plus the cases of the rule: v equal to a vertex's v, points on axis_min / axis_max, points on an edge."""
    u, v = R.UV[axis]
    rng = np.random.default_rng(seed)
    pts = ((rng.random((4097, 3)) - 0.5) * 24).astype(np.float32)
    k = 0
    for vert in poly:                                   # v exactly a vertex's v, u on both sides: the `<` / `>=` pair
        for du in (-12.0, -0.75, 0.75, 12.0):
            pts[k, u], pts[k, v] = vert[u] + du, vert[v]
            k += 1
    pts[k:k + 200, axis] = lo                           # exactly on the two faces of the axis range
    pts[k + 200:k + 400, axis] = hi
    k += 400
    for i in range(len(poly)):                          # dyadic points exactly on an edge: the node equals p.u, not counted
        a, b = poly[i], poly[(i + 1) % len(poly)]
        for w in (0.25, 0.5, 0.75):
            q = a + w * (b - a)
            if np.array_equal(q.astype(np.float32).astype(np.float64), q):
                pts[k, u], pts[k, v] = q[u], q[v]
                k += 1
    return pts


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_crop_mask_exact(axis):
    u, v = R.UV[axis]
    poly = np.zeros((len(R.CONCAVE_XY), 3))
    poly[:, u], poly[:, v] = R.CONCAVE_XY[:, 0], R.CONCAVE_XY[:, 1]
    lo, hi = 6.5, -7.25                                 # handed over swapped: min / max are taken
    pts = _crop_points(axis, poly, lo, hi, 50 + axis)
    crop = {"orthogonal_axis": "XYZ"[axis], "axis_min": lo, "axis_max": hi, "bounding_polygon": poly}
    want = R.crop_mask(pts, axis, lo, hi, poly)
    out, keep = TE.crop_points(_dev(pts), crop, return_mask=True)
    keep = keep.cpu().numpy()
    print(f"crop axis {axis}: {int(want.sum())} of {len(pts)} kept, {int((keep != want).sum())} differ")
    assert 500 < want.sum() < 3000
    on_face = (pts[:, axis] == np.float32(lo)) | (pts[:, axis] == np.float32(hi))
    assert (want & on_face).sum() > 50                  # points on the faces are inside
    assert np.array_equal(keep, want)
    assert np.array_equal(out.cpu().numpy(), pts[want])
    assert np.array_equal(TE.crop_mask_host(pts, crop), want)


def test_crop_polygon_sizes():
    pts = _cloud(4097, 55, 24.0)
    tri = np.array([[-8.0, -7.0, 0.0], [9.0, -2.0, 0.0], [-1.0, 8.5, 0.0]])
    ang = 2 * np.pi * np.arange(256) / 256
    ring = np.stack([7.5 * np.cos(ang) * (1 + 0.3 * np.cos(5 * ang)), 7.5 * np.sin(ang) * (1 + 0.3 * np.cos(5 * ang)), 0 * ang], 1)
    for poly in (tri, ring):
        crop = {"orthogonal_axis": "Z", "axis_min": -100.0, "axis_max": 100.0, "bounding_polygon": poly}
        want = R.crop_mask(pts, 2, -100.0, 100.0, poly)
        assert 300 < want.sum() < 3500
        assert np.array_equal(TE.crop_points(_dev(pts), crop, return_mask=True)[1].cpu().numpy(), want)
    big = {"orthogonal_axis": "Z", "axis_min": -1.0, "axis_max": 1.0, "bounding_polygon": np.concatenate([ring, ring[:1]], 0)}
    with pytest.raises(TE._lib.GsrError, match="256"):
        TE.crop_points(_dev(pts), big)
    assert TE.crop_points(_dev(np.zeros((0, 3))), crop).shape == (0, 3)


# ---------------------------------------------------------------- 3. TNT_VOXEL
VOXEL = R.VOXEL          # (the table lives beside the reference: the CPU tests share it)


@pytest.mark.parametrize("name", list(VOXEL))
def test_voxel_bit_for_bit(name):
    make, size = VOXEL[name]
    pts = make()
    want, row = R.voxel(pts, size)
    got, cells = TE.voxel_down_sample(_dev(pts), size, return_cells=True)
    got, cells = got.cpu().numpy(), cells.cpu().numpy()
    print(f"voxel {name}: {len(pts)} points -> {len(want)} cells")
    if name in ("copies_of_one_point", "one_cell_distinct"):
        assert len(want) == 1
    elif len(pts) > 1:
        assert 1 < len(want) < len(pts)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cells, row)
    again, cells2 = TE.voxel_down_sample(_dev(pts), size, return_cells=True)
    assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32)) and np.array_equal(cells2.cpu().numpy(), cells)
    assert np.array_equal(TE.voxel_down_sample(_dev(pts), size).cpu().numpy().view(np.uint32), got.view(np.uint32))
    host, hrow = TE.voxel_down_sample_host(pts, size, return_cells=True)
    assert np.array_equal(host.view(np.uint32), got.view(np.uint32)) and np.array_equal(hrow, row)


def test_voxel_refuses_too_many_cells():
    pts = _cloud(300, 66)
    with pytest.raises(TE._lib.GsrError, match="voxel_size"):
        TE.voxel_down_sample(_dev(pts), 1e-6)
    with pytest.raises(ValueError, match="voxel_size"):
        TE.voxel_down_sample(_dev(pts), 0.0)
    assert TE.voxel_down_sample(_dev(pts), 10.0 / 2 ** 20).shape[0] == 300     # just below the limit: accepted


def test_uniform_down_sample():
    pts = _cloud(4097, 67)
    assert np.array_equal(TE.uniform_down_sample(_dev(pts), 1000).cpu().numpy(), pts[::4])
    assert np.array_equal(TE.uniform_down_sample(_dev(pts), 4097).cpu().numpy(), pts)
    assert np.array_equal(TE.uniform_down_sample(_dev(pts), 3000).cpu().numpy(), pts)          # k = round(1.37) = 1


# ---------------------------------------------------------------- 4. TNT_ICP_SUMS
def check_icp_sums(n, pairs_from=0, pair_at_end=False):
    """Both passes of the sums on n random pairs (three in ten without a correspondence; none below index `pairs_from`; the last
    point has one if `pair_at_end`) against numpy under the order-independent bound, twice for the same bits, and against the
    host twin.  tests/test_gpu_cloud_scale.py runs the same body beyond one trip of the grid."""
    rng = np.random.default_rng(70 + n)
    m = 500
    src, tgt = _cloud(n, 71 + n), _cloud(m, 72)
    idx = rng.integers(0, m, size=n).astype(np.int32)
    idx[rng.random(n) < 0.3] = -1
    idx[:pairs_from] = -1
    if pair_at_end:
        idx[-1] = m - 1
    dist = rng.random(n) * 0.3
    dist[idx < 0] = np.inf
    args = (_dev(src), _dev(tgt), _dev(dist, np.float64), _dev(idx, np.int32))
    rows = np.nonzero(idx >= 0)[0]
    s, t, d = src[rows].astype(np.float64), tgt[idx[rows]].astype(np.float64), dist[rows]
    p1 = TE.icp_sums(*args)
    assert p1[0] == len(rows) and p1[8] == 0 and p1[9] == 0
    terms1 = [s[:, 0], s[:, 1], s[:, 2], t[:, 0], t[:, 1], t[:, 2], d * d]
    for got, term in zip(p1[1:8], terms1):
        assert abs(got - term.sum()) <= len(rows) * 2.0 ** -53 * np.abs(term).sum()
    assert np.array_equal(TE.icp_sums(*args), p1)
    means = p1[1:7] / max(len(rows), 1)
    p2 = TE.icp_sums(*args, means=means)
    ds, dt = s - means[None, :3], t - means[None, 3:]
    terms2 = [dt[:, r] * ds[:, c] for r in range(3) for c in range(3)] + [(ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2]]
    for got, term in zip(p2, terms2):
        assert abs(got - term.sum()) <= len(rows) * 2.0 ** -53 * np.abs(term).sum()
    assert np.array_equal(TE.icp_sums(*args, means=means), p2)
    host1, host2 = TE.icp_sums_host(src, tgt, dist, idx), TE.icp_sums_host(src, tgt, dist, idx, means)
    assert host1[0] == p1[0] and np.allclose(host1, p1, rtol=1e-12, atol=1e-12) and np.allclose(host2, p2, rtol=1e-10, atol=1e-10)
    return len(rows)


@pytest.mark.parametrize("n", SIZES + (20000,))
def test_icp_sums_fixed_order(n):
    check_icp_sums(n)


def test_icp_sums_without_pairs():
    src, tgt = _cloud(257, 75), _cloud(100, 76)
    none = np.full(257, -1, np.int32)
    args = (_dev(src), _dev(tgt), _dev(np.full(257, np.inf), np.float64), _dev(none, np.int32))
    assert np.array_equal(TE.icp_sums(*args), np.zeros(10))
    assert np.array_equal(TE.icp_sums(*args, means=np.zeros(6)), np.zeros(10))
    # an index outside the target is no pair either (and is never read)
    wild = _dev(np.full(257, 100, np.int32), np.int32)
    assert np.array_equal(TE.icp_sums(args[0], args[1], args[2], wild), np.zeros(10))


# ---------------------------------------------------------------- 5. TNT_SCORE
@pytest.mark.parametrize("B", [1, 499, 4096])
def test_score_equals_numpy_histogram(B):
    rng = np.random.default_rng(80 + B)
    tau = 0.01
    edges = TE.score_edges(tau, 5) if B == 499 else np.sort(rng.random(B + 1)) * 0.05 + 0.001
    assert len(edges) == B + 1
    for n in SIZES + (20000,):
        d = rng.random(n) * 0.06
        if n >= 255:
            k = min(n // 4, B + 1)
            d[:k] = edges[rng.integers(0, B + 1, size=k)]                      # exactly on edges
            d[k:k + 5] = edges[-1]                                             # the last edge: in the last bin
            d[k + 5:k + 10] = np.nextafter(edges[-1], 1)                       # just above: in no bin
            d[k + 10:k + 15] = np.inf
            d[k + 15:k + 20] = [tau, np.nextafter(tau, 0), np.nextafter(tau, 1), edges[0], np.nextafter(edges[0], 0)]
        count, hist = TE.score_distances(_dev(d, np.float64), tau, edges)
        assert count == int((d < tau).sum())
        assert hist.dtype == np.int64 and np.array_equal(hist, np.histogram(d, edges)[0])
        if n == 4097:
            assert hist[-1] >= 5 and hist.sum() < n
            assert TE.score_distances(_dev(d, np.float64), tau, edges)[1].tolist() == hist.tolist()
    assert TE.score_distances_host(d, tau, edges)[0] == count


def test_score_refuses_too_many_bins():
    d = _dev(np.random.default_rng(1).random(100), np.float64)
    with pytest.raises(TE._lib.GsrError, match="4096"):
        TE.score_distances(d, 0.5, np.linspace(0, 1, 4098))
    with pytest.raises(ValueError):
        TE.score_distances(d, 0.0, np.linspace(0, 1, 10))
    with pytest.raises(TE._lib.GsrError, match="decrease"):
        TE.score_distances(d, 0.5, np.array([0.0, 0.5, 0.25]))


# ---------------------------------------------------------------- 6. ICP, device against host twin
class Margins:
    """The observer of a host run: asserts at every search that the device, whose sums differ in the last bits, must take the
    same decisions -- change the seed of a fixture that fails here, never the bar."""

    def __init__(self):
        self.searches = 0

    def __call__(self, query, cloud, max_dist):
        if len(query) == 0 or len(cloud) < 2:
            return
        d, _ = R.nearest(query, cloud, k=2)
        assert (d[:, 1] > (1 + 1e-6) * d[:, 0]).all(), "a query has two nearest points within 1e-6 relative"
        if np.isfinite(max_dist):
            assert (np.abs(d[:, 0] / max_dist - 1) > 1e-6).all(), "a distance lies within 1e-6 relative of the threshold"
        self.searches += 1


def _assert_stop_margins(reg, n_source, rel=1e-6):
    fit = [c / n_source for c, _ in reg["trace"]]
    rmse = [e for _, e in reg["trace"]]
    for k in range(1, len(fit)):
        for delta in (abs(fit[k] - fit[k - 1]), abs(rmse[k] - rmse[k - 1])):
            assert abs(delta / rel - 1) > 0.01, "a stopping test lies within 1 % of its threshold"


def _assert_same_registration(dev, host, label, bar=R.ICP_BAR_FACTOR * R.ICP_SPREAD):
    dT = np.abs(dev["transformation"] - host["transformation"]).max() / np.abs(host["transformation"]).max()
    dr = abs(dev["inlier_rmse"] - host["inlier_rmse"]) / host["inlier_rmse"]
    print(f"{label}: {host['iterations']} iterations, counts {[c for c, _ in host['trace']]}; transformation off by {dT:.3e}, "
          f"rmse by {dr:.3e} relative (bar {bar:.3e})")
    assert dev["iterations"] == host["iterations"]
    assert [c for c, _ in dev["trace"]] == [c for c, _ in host["trace"]]
    assert dev["fitness"] == host["fitness"]
    assert dT <= bar and dr <= bar


def test_registration_icp_equals_host_twin():
    """The bar on the transformation's entries and on inlier_rmse is 16 x the spread of the host twin over 20 random orders of
    adding the correspondences (tests/test_tnt_eval_cpu.py::test_icp_sum_order_spread): measured 2.03e-14 relative, so the bar
    is 3.25e-13 relative."""
    fx = R.icp_fixture()
    obs = Margins()
    host = R.cached("icp_host_observed", lambda: TE.registration_icp_host(fx["source"], fx["target"], fx["threshold"], observer=obs))
    assert obs.searches in (0, host["iterations"] + 1)
    _assert_stop_margins(host, len(fx["source"]))
    assert host["iterations"] >= 2
    dev = TE.registration_icp(_dev(fx["source"]), _dev(fx["target"]), fx["threshold"])
    _assert_same_registration(dev, host, "icp")
    again = TE.registration_icp(_dev(fx["source"]), _dev(fx["target"]), fx["threshold"])
    assert np.array_equal(again["transformation"], dev["transformation"]) and again["trace"] == dev["trace"]
    # nothing in reach: returned at once
    far = TE.registration_icp(_dev(fx["source"]), _dev(fx["target"] + 100.0), fx["threshold"])
    assert far["iterations"] == 0 and far["fitness"] == 0.0 and np.array_equal(far["transformation"], np.eye(4))


# ---------------------------------------------------------------- 7. end to end
def _host_e2e():
    from gaussmart_amd.mesh import TriangleMesh
    inst = R.ellipsoid_instance()
    assert len(inst["tris"]) == 1280

    def run():
        obs = Margins()
        res = TE.evaluate_tnt_mesh_host(TriangleMesh(inst["verts"], inst["tris"]), inst["gt_points"], inst["crop"], inst["tau"],
                                        inst["init"], observer=obs)
        assert obs.searches >= 8
        return res
    return inst, R.cached("tnt_e2e_host", run)


def test_end_to_end_equals_host_twin(tmp_path):
    from gaussmart_amd import tnt_eval_cli
    from gaussmart_amd.mesh import TriangleMesh
    inst, host = _host_e2e()
    mesh = TriangleMesh(inst["verts"], inst["tris"])
    for reg in host["registrations"]:
        _assert_stop_margins(reg, reg["n_source"])
    dev = TE.evaluate_tnt_mesh(mesh, inst["gt_points"], inst["crop"], inst["tau"], inst["init"], device=DEV)
    print(f"end to end: {len(host['cloud_source'])} / {len(host['cloud_target'])} points scored, precision {dev['precision']!r} / "
          f"{host['precision']!r}, recall {dev['recall']!r} / {host['recall']!r}, fscore {dev['fscore']!r}")
    for k, (d, h) in enumerate(zip(dev["registrations"], host["registrations"])):
        assert (d["n_source"], d["n_target"]) == (h["n_source"], h["n_target"])
        _assert_same_registration(d, h, f"registration {k}", bar=1e-9)      # (figures printed; the measured bar is the ICP test's)
    assert 0.5 < host["precision"] < 1.0 and 0.5 < host["recall"] < 1.0
    assert dev["precision"] == host["precision"] and dev["recall"] == host["recall"] and dev["fscore"] == host["fscore"]
    assert np.array_equal(dev["hist_source"], host["hist_source"]) and np.array_equal(dev["hist_target"], host["hist_target"])
    assert np.array_equal(dev["edges"], host["edges"]) and np.array_equal(dev["cum_source"], host["cum_source"])
    assert len(dev["cloud_source"]) == len(host["cloud_source"]) and len(dev["cloud_target"]) == len(host["cloud_target"])
    # a second device run: identical bits throughout
    again = TE.evaluate_tnt_mesh(mesh, inst["gt_points"], inst["crop"], inst["tau"], inst["init"], device=DEV)
    assert np.array_equal(again["transformation"], dev["transformation"])
    for key in ("dist_source", "dist_target", "cloud_source", "cloud_target"):
        assert torch.equal(again[key], dev[key]), key
    assert [r["trace"] for r in again["registrations"]] == [r["trace"] for r in dev["registrations"]]
    assert np.array_equal(again["hist_source"], dev["hist_source"]) and again["fscore"] == dev["fscore"]
    # the command line on the same instance written to disk
    poses = np.tile(np.eye(4), (4, 1, 1))
    d = R.write_tnt_instance(str(tmp_path), "Ellipsoid", inst, poses, np.eye(4))
    mesh.write_ply(str(tmp_path / "mesh.ply"))
    R.write_log(str(tmp_path / "rec.log"), poses)
    np.savetxt(str(tmp_path / "init.txt"), inst["init"])
    out = str(tmp_path / "out")
    rc = tnt_eval_cli.main(["--dataset-dir", d, "--traj-path", str(tmp_path / "rec.log"), "--ply-path", str(tmp_path / "mesh.ply"),
                            "--out-dir", out, "--tau", repr(inst["tau"]), "--init-transform", str(tmp_path / "init.txt"),
                            "--write_vis"])
    assert rc == 0
    with open(os.path.join(out, "results.json")) as f:
        res = json.load(f)
    assert (res["precision"], res["recall"], res["fscore"], res["tau"]) == (dev["precision"], dev["recall"], dev["fscore"], inst["tau"])
    assert np.array_equal(np.array(res["transformation"]), dev["transformation"])
    assert [r["trace"] for r in res["icp"]] == [[[c, e] for c, e in r["trace"]] for r in dev["registrations"]]
    assert np.array_equal(np.loadtxt(os.path.join(out, "Ellipsoid.precision.txt")), dev["cum_source"])
    assert np.array_equal(np.loadtxt(os.path.join(out, "Ellipsoid.recall.txt")), dev["cum_target"])
    assert np.array_equal(np.loadtxt(os.path.join(out, "Ellipsoid.prf_tau_plotstr.txt")),
                          [dev["precision"], dev["recall"], dev["fscore"], inst["tau"], 5])
    try:
        import matplotlib  # noqa: F401
        assert os.path.isfile(os.path.join(out, "Ellipsoid.precision.ply")) and os.path.isfile(os.path.join(out, "Ellipsoid.recall.ply"))
    except ImportError:
        assert not os.path.exists(os.path.join(out, "Ellipsoid.precision.ply"))


# ---------------------------------------------------------------- 8. argument checking through the ABI
def test_errors_come_before_any_launch():
    from gaussmart_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -4
    pts = _dev(_cloud(100, 90))
    tris = _dev(np.array([[0, 1, 2]] * 10), np.int32)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    big = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.full((200, 3), 7.0, device=DEV)
    keep = torch.full((100,), 7, dtype=torch.uint8, device=DEV)
    cells = torch.full((100,), 7, dtype=torch.int32, device=DEV)
    sums = torch.full((10,), 7.0, dtype=torch.float64, device=DEV)
    hist = torch.full((17,), 7, dtype=torch.int64, device=DEV)
    dist = _dev(np.random.default_rng(0).random(100), np.float64)
    idx = _dev(np.arange(100), np.int32)
    n64 = C.c_int64(5)

    def centres(F=10, V=100, v=p(pts), t=p(tris), o=p(out)):
        return L.gsr_mesh_face_centres(v, t, F, V, o, stream)
    assert [centres(F=-1), centres(V=-1), centres(v=None), centres(t=None), centres(o=None)] == [INVALID] * 5
    assert centres(F=2 ** 31) == UNSUPPORTED and centres(F=2 ** 30, V=2 ** 30) == UNSUPPORTED

    eye = np.eye(4)
    shear = np.eye(4)
    shear[3, 3] = 2.0

    def move(n=100, T=hp(eye), pp=p(pts), o=p(out)):
        return L.gsr_points_transform(pp, n, T, o, stream)
    assert [move(n=-1), move(T=None), move(T=hp(shear)), move(pp=None), move(o=None)] == [INVALID] * 5
    assert move(n=2 ** 31) == UNSUPPORTED

    poly = _dev(R.CONCAVE_XY, np.float64)

    def crop(n=100, axis=2, lo=-1.0, hi=1.0, m=7, pp=p(pts), pl=p(poly), k=p(keep)):
        return L.gsr_points_crop_polygon(pp, n, axis, lo, hi, pl, m, k, stream)
    assert [crop(n=-1), crop(axis=3), crop(axis=-1), crop(lo=float("nan")), crop(m=0), crop(m=-2), crop(pp=None), crop(pl=None),
            crop(k=None)] == [INVALID] * 9
    assert crop(m=257) == UNSUPPORTED and crop(n=2 ** 31) == UNSUPPORTED

    def vcount(n=100, size=0.5, ws=big.numel(), pp=p(pts)):
        return L.gsr_points_voxel_count(pp, n, size, p(big), ws, C.byref(n64), stream)
    assert [vcount(n=-1), vcount(size=0.0), vcount(size=-1.0), vcount(size=float("nan")), vcount(size=float("inf")), vcount(ws=64),
            vcount(pp=None)] == [INVALID] * 7
    assert vcount(n=2 ** 31) == UNSUPPORTED and n64.value == 0
    assert L.gsr_points_voxel_count(p(pts), 100, 0.5, p(big), big.numel(), None, stream) == INVALID

    def vemit(n=100, size=0.5, ws=big.numel(), pp=p(pts), o=p(out)):
        return L.gsr_points_voxel_emit(pp, n, size, p(big), ws, o, p(cells), stream)
    assert [vemit(n=-1), vemit(size=0.0), vemit(ws=64), vemit(pp=None), vemit(o=None)] == [INVALID] * 5

    mu = np.zeros(6)

    def isums(n=100, m=100, ws=big.numel(), s=p(pts), t=p(pts), d=p(dist), i=p(idx), o=p(sums), means=None):
        return L.gsr_icp_sums(s, n, t, m, d, i, means, p(big), ws, o, stream)
    assert [isums(n=-1), isums(m=-1), isums(ws=64), isums(s=None), isums(t=None), isums(d=None), isums(i=None), isums(o=None),
            isums(o=None, means=hp(mu))] == [INVALID] * 9
    assert isums(n=2 ** 31) == UNSUPPORTED and isums(m=2 ** 31) == UNSUPPORTED

    edges = np.linspace(0.0, 1.0, 17)
    down = edges[::-1].copy()
    nan = edges.copy()
    nan[3] = np.nan

    def score(n=100, B=16, tau=0.5, ws=big.numel(), d=p(dist), e=hp(edges), c=p(hist), h=p(hist[1:])):
        return L.gsr_dist_score(d, n, e, B, tau, p(big), ws, c, h, stream)
    assert [score(n=-1), score(B=0), score(tau=0.0), score(tau=-1.0), score(tau=float("nan")), score(ws=8), score(d=None),
            score(e=None), score(e=hp(down)), score(e=hp(nan)), score(c=None), score(h=None)] == [INVALID] * 12
    assert score(B=4097) == UNSUPPORTED and score(n=2 ** 31) == UNSUPPORTED
    assert "2147483648" in L.gsr_last_error().decode()
    torch.cuda.synchronize()
    # nothing ran
    assert not big.any() and (out == 7.0).all() and (keep == 7).all() and (cells == 7).all() and (sums == 7.0).all()
    assert (hist == 7).all()
    assert vcount(size=1e-7) == UNSUPPORTED and "voxel_size" in L.gsr_last_error().decode()
    assert vcount() == 0 and 1 < n64.value <= 100
