"""DTU mesh evaluation on the device against the float64 restatement (tests/mesh_eval_ref.py): sampling bit for bit, the
down-sampling's keep mask, the nearest-neighbour search against cKDTree, the ObsMask and plane filters against numpy, the whole
evaluation against its host twin, the command line and the error paths."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import mesh_eval_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ULP = 2.0 ** -52


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _mesh(verts, tris):
    from gaussmart_amd.mesh import DeviceTriangleMesh
    return DeviceTriangleMesh(_dev(verts), _dev(np.asarray(tris).reshape(-1, 3), np.int32))


# ---------------------------------------------------------------- 1. sampling
def _random_triangles(seed):
    rng = np.random.default_rng(seed)
    verts = (rng.random((300, 3)) * 2).astype(np.float32)
    return verts, rng.integers(0, 300, (500, 3)).astype(np.int32)


SAMPLING = {
    # legs 1.0 at thresh 0.25: n1 = n2 = 4 exactly, and a + b = 1 exactly for i + j = 3 (not kept)
    "right_ties": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 2]], 0.25, 6),
    "too_small": (np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]], np.float32), [[0, 1, 2]], 0.25, 0),
    "zero_area": (np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32), [[0, 1, 2], [0, 0, 1]], 0.25, 0),
    "bad_index": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 3], [-1, 1, 2], [0, 1, 2]], 0.25, 6),
    "sliver_1_200": (np.array([[5, 5, 5], [7, 5, 5], [5, 5.01, 5]], np.float32), [[0, 1, 2]], 0.003, None),
    "random_500": _random_triangles(11) + (0.1, None),
    "no_triangles": (np.array([[1, 2, 3]], np.float32), np.zeros((0, 3), np.int32), 0.25, 0),
}


@pytest.mark.parametrize("name", list(SAMPLING))
def test_sampling_bit_for_bit(name):
    from gaussmart_amd.mesh_eval import sample_mesh_points
    verts, tris, thresh, n_samples = SAMPLING[name]
    if name == "random_500":
        # the floors must not hang on the last bit: change the seed above if this fails, never the bar
        assert R.min_integer_margin(verts, tris, thresh) > 1e-9
    ref, counts = R.cached(("sample", name), lambda: R.sample_mesh(verts, tris, thresh))
    got = sample_mesh_points(_mesh(verts, tris), thresh).cpu().numpy()
    print(f"{name}: {len(verts)} vertices + {int(counts.sum())} samples, per-triangle maximum {int(counts.max()) if len(counts) else 0}")
    if n_samples is not None:
        assert counts.sum() == n_samples
    else:
        assert counts.sum() > 500
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))


def test_sampling_cap_names_the_density():
    from gaussmart_amd import _lib
    from gaussmart_amd.mesh_eval import sample_mesh_points
    big = np.array([[0, 0, 0], [100, 0, 0], [0, 100, 0]], np.float32)
    with pytest.raises(_lib.GsrError, match="downsample_density"):
        sample_mesh_points(_mesh(big, [[0, 1, 2]]), 0.01)          # n1 * n2 = 1e8 > 2^24


# ---------------------------------------------------------------- 2. down-sampling
_random_cloud, DOWNSAMPLE = R.random_cloud, R.DOWNSAMPLE          # (the table lives beside the reference: the CPU tests share it)


@pytest.mark.parametrize("name", list(DOWNSAMPLE))
def test_downsample_keep_mask(name):
    from gaussmart_amd.mesh_eval import downsample_points
    make, thresh, check_margin = DOWNSAMPLE[name]
    pts = make()
    if check_margin and len(pts) > 1:
        assert R.pair_margin(pts, thresh) > 1e-9
    ref = R.cached(("keep", name), lambda: R.greedy_keep(pts, thresh))
    keep, rounds = downsample_points(_dev(pts), thresh, return_rounds=True)
    keep = keep.cpu().numpy()
    print(f"{name}: {int(ref.sum())} of {len(pts)} kept, {rounds} rounds")
    assert keep.dtype == bool and np.array_equal(keep, ref)
    if name == "lattice_6":
        assert ref.sum() == 27 * 4          # the sequential rule keeps every other point per axis ... in lexicographic order
    if name == "duplicates_200":
        assert ref.sum() == 1 and ref[0]
    if name == "sorted_line_2000":
        assert ref.sum() == 1000 and 100 <= rounds <= 2008          # a chain: about one decision per round
    again = downsample_points(_dev(pts), thresh).cpu().numpy()
    assert np.array_equal(again, keep)


# ---------------------------------------------------------------- 3. nearest neighbour
def _check_nearest(query, cloud, max_dist=np.inf):
    from gaussmart_amd.mesh_eval import nearest_distance
    d, i = nearest_distance(_dev(query), _dev(cloud), max_dist)
    assert d.dtype == torch.float64 and i.dtype == torch.int32
    d, i = d.cpu().numpy(), i.cpu().numpy()
    rd, ri = R.nearest(query, cloud)
    cut = rd[:, 0] >= max_dist
    near_cut = np.abs(rd[:, 0] - max_dist) <= 4 * ULP * max_dist if np.isfinite(max_dist) else np.zeros(len(rd), bool)
    assert not near_cut.any()
    assert np.isinf(d[cut]).all() and (i[cut] == -1).all()
    ok = ~cut
    assert (np.abs(d[ok] - rd[ok, 0]) <= 4 * ULP * rd[ok, 0]).all(), float((np.abs(d[ok] - rd[ok, 0]) / (ULP * rd[ok, 0] + 1e-300)).max())
    safe = ok & (rd[:, 1] > rd[:, 0] * (1 + 1e-9)) if rd.shape[1] > 1 else ok
    assert np.array_equal(i[safe], ri[safe, 0])
    assert np.array_equal(d[ok], np.sqrt(R.dist2(query[ok], cloud[i[ok]])))     # EVAL_DIST itself
    return d, i, int(cut.sum())


@pytest.mark.parametrize("nq,nc", [(1, 65), (4097, 5000), (5000, 1)])
def test_nearest_sizes(nq, nc):
    rng = np.random.default_rng(nq + nc)
    query, cloud = rng.random((nq, 3)).astype(np.float32), (rng.random((nc, 3)) * np.array([1, 2, 0.5])).astype(np.float32)
    d, _, _ = _check_nearest(query, cloud)
    assert np.isfinite(d).all()
    cut_at = float(np.median(d)) * (1 + 1e-6) if nq > 1 else float(d[0]) * 2
    _, _, n_cut = _check_nearest(query, cloud, cut_at)
    assert nq == 1 or abs(n_cut - nq / 2) <= 1
    print(f"nearest {nq} x {nc}: median {np.median(d):.4f}, {n_cut} cut at {cut_at:.4f}")


def test_nearest_far_outside_identical_and_ties():
    from gaussmart_amd.mesh_eval import nearest_distance
    rng = np.random.default_rng(21)
    cloud = rng.random((5000, 3)).astype(np.float32)
    far = (rng.random((300, 3)) * 2 - 1).astype(np.float32) * 100 + np.float32(0.5)      # 100 box widths away, all round
    _check_nearest(far, cloud)
    _check_nearest(far, cloud, 60.0)
    same = np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (4097, 1))
    d, i = nearest_distance(_dev(far[:70]), _dev(same))
    assert (i.cpu().numpy() == 0).all()
    assert np.array_equal(d.cpu().numpy(), np.sqrt(R.dist2(far[:70], same[:70])))
    # exact ties: every cloud point twice, the copies first in reversed order; integer coordinates make d2 exact
    base = rng.integers(-20, 20, (700, 3)).astype(np.float32)
    base = np.unique(base, axis=0)
    tied = np.concatenate([base[::-1], base], 0)
    q = rng.integers(-25, 25, (1000, 3)).astype(np.float32)
    d, i = nearest_distance(_dev(q), _dev(tied))
    d, i = d.cpu().numpy(), i.cpu().numpy()
    d2 = R.dist2(q[:, None, :], tied[None, :, :])
    assert np.array_equal(i, d2.argmin(1)) and np.array_equal(d, np.sqrt(d2.min(1)))
    assert (i < len(base)).all()
    # an empty cloud, and no queries
    d, i = nearest_distance(_dev(q[:5]), _dev(np.zeros((0, 3))))
    assert torch.isinf(d).all() and (i == -1).all()
    d, i = nearest_distance(_dev(np.zeros((0, 3))), _dev(tied))
    assert d.numel() == 0 and i.numel() == 0


# ---------------------------------------------------------------- 4. ObsMask and plane
def test_obs_filter_and_plane_exact():
    from gaussmart_amd.mesh_eval import filter_by_obs_mask, filter_by_plane
    rng = np.random.default_rng(6)
    obs = (rng.random((8, 9, 10)) < 0.5).astype(np.uint8)
    bb = np.array([[1.0, 2.0, 3.0], [12.0, 14.0, 16.5]], np.float32)
    res, patch = 1.5, 2.0
    cells = np.stack(np.meshgrid(np.arange(-1, 9), np.arange(-1, 10), np.arange(-1, 11), indexing="ij"), -1).reshape(-1, 3)
    half = (bb[0].astype(np.float64) + (cells + 0.5) * res).astype(np.float32)          # exactly on half cells: half to even
    lo, hi = bb[0].astype(np.float64) - patch, bb[1].astype(np.float64) + 2 * patch
    edge = np.array([lo, hi, [lo[0], 5, 5], [hi[0], 5, 5], [5, lo[1], 5], [5, hi[1], 5], [5, 5, lo[2]], [5, 5, hi[2]],
                     np.nextafter(lo.astype(np.float32), np.float32(-100)), np.nextafter(hi.astype(np.float32), np.float32(-100))])
    outside = np.array([bb[0] - res, bb[0] + res * np.array(obs.shape), [1 - 0.76, 5, 5], [1 + 1.5 * 7.5, 5, 5]])
    pts = np.concatenate([(rng.random((3000, 3)) * 30 - 6), half, edge, outside], 0).astype(np.float32)
    assert np.array_equal(half.astype(np.float64), bb[0] + (cells + 0.5) * res)          # the fixture is exact in f32
    rin, rio = R.cached("obs", lambda: R.obs_filter(pts, obs, bb, res, patch))
    a, b, inb, ino = filter_by_obs_mask(_dev(pts), obs, bb, res, patch)
    assert np.array_equal(inb.cpu().numpy(), rin) and np.array_equal(ino.cpu().numpy(), rio)
    assert np.array_equal(a.cpu().numpy(), pts[rin]) and np.array_equal(b.cpu().numpy(), pts[rio])
    k = 3000 + len(half)
    assert rin[k] and not rin[k + 1] and list(rin[k + 2:k + 8]) == [True, False] * 3 and not rin[k + 8] and rin[k + 9]
    assert rin[k + 10:].all() and not rio[k + 10:k + 12].any()
    assert 100 < rio.sum() < rin.sum() < len(pts)
    for plane in ([0.3, -0.2, 0.9, -4.0], [0.0, 0.0, 1.0, -5.0], [0.0, 0.0, 0.0, 0.0]):
        got = filter_by_plane(_dev(pts), np.array(plane)).cpu().numpy()
        assert np.array_equal(got, R.plane_filter(pts, plane))
    e = filter_by_obs_mask(_dev(np.zeros((0, 3))), obs, bb, res, patch)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].numel() == 0


def test_distance_mean_fixed_order():
    from gaussmart_amd.mesh_eval import distance_mean
    rng = np.random.default_rng(9)
    for n in (0, 1, 255, 256, 257, 64 ** 3, 64 ** 3 + 1, 300001):      # 64^3 = 1024 x 256: the last size of one trip of the grid
        d = rng.random(n) * 20
        d[rng.random(n) < 0.3] = np.inf
        fin = d[np.isfinite(d)]
        m, c = distance_mean(_dev(d, np.float64))
        assert c == len(fin)
        if len(fin) == 0:
            assert np.isnan(m)
        else:
            assert abs(m - fin.mean()) <= len(fin) * 2.0 ** -53 * fin.mean()
            assert distance_mean(_dev(d, np.float64))[0] == m


# ---------------------------------------------------------------- 5. end to end
def _instance_kw(inst):
    return {k: inst[k] for k in ("stl_points", "obs_mask", "bb", "res", "plane", "patch_size", "downsample_density", "max_dist")}


def test_end_to_end_equals_host_twin(tmp_path):
    from gaussmart_amd import dtu_eval_cli
    from gaussmart_amd.mesh import TriangleMesh
    from gaussmart_amd.mesh_eval import evaluate_dtu_mesh, evaluate_dtu_mesh_host
    from test_mesh_eval_cpu import write_instance
    inst = R.sphere_instance()
    assert len(inst["tris"]) == 1280
    mesh = TriangleMesh(inst["verts"], inst["tris"])
    host = R.cached("e2e_host", lambda: evaluate_dtu_mesh_host(mesh, **_instance_kw(inst)))
    dev = evaluate_dtu_mesh(mesh, device=DEV, **_instance_kw(inst))
    print(f"end to end: {len(dev['keep'])} sampled, {int(host['keep'].sum())} kept in {dev['rounds']} rounds, "
          f"{int(host['inbound'].sum())} inbound, {int(host['in_obs'].sum())} in_obs, {int(host['above'].sum())} above; "
          f"d2s {dev['mean_d2s']!r} / {host['mean_d2s']!r}, s2d {dev['mean_s2d']!r} / {host['mean_s2d']!r}")
    for key in ("keep", "inbound", "in_obs", "above", "idx_d2s", "idx_s2d", "data_down"):
        assert np.array_equal(dev[key].cpu().numpy(), host[key]), key
    assert 0 < host["in_obs"].sum() < host["inbound"].sum() < host["keep"].sum() < len(host["keep"])
    assert 0 < host["above"].sum() < len(host["above"])
    for key, dkey in (("mean_d2s", "dist_d2s"), ("mean_s2d", "dist_s2d")):
        n = int(np.isfinite(host[dkey]).sum())
        assert n > 1000 and abs(dev[key] - host[key]) <= n * 2.0 ** -53 * host[key], key
        assert np.array_equal(dev[dkey].cpu().numpy(), host[dkey])
    assert dev["overall"] == (dev["mean_d2s"] + dev["mean_s2d"]) / 2
    again = evaluate_dtu_mesh(mesh, device=DEV, **_instance_kw(inst))
    for key in ("mean_d2s", "mean_s2d", "overall"):
        assert again[key] == dev[key]
    for key in ("dist_d2s", "dist_s2d", "idx_d2s", "idx_s2d", "keep"):
        assert torch.equal(again[key], dev[key])
    # the command line on the same instance written to disk
    write_instance(str(tmp_path / "dtu"), 3, inst)
    mesh.write_ply(str(tmp_path / "mesh.ply"))
    rc = dtu_eval_cli.main(["--data", str(tmp_path / "mesh.ply"), "--scan", "3", "--dataset_dir", str(tmp_path / "dtu"),
                            "--vis_out_dir", str(tmp_path / "out"), "--downsample_density", "0.5", "--patch_size", "1.5",
                            "--write_vis"])
    assert rc == 0
    with open(os.path.join(str(tmp_path / "out"), "results.json")) as f:
        res = json.load(f)
    assert res == {k: dev[k] for k in ("mean_d2s", "mean_s2d", "overall")}
    assert os.path.isfile(str(tmp_path / "out" / "vis_003_s2d.ply"))


# ---------------------------------------------------------------- 6. argument checking through the ABI
def test_errors_come_before_any_launch():
    from gaussmart_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -4
    verts, tris = _dev(SAMPLING["right_ties"][0]), _dev(np.array([[0, 1, 2]]), np.int32)
    pts = _dev(np.random.default_rng(0).random((100, 3)))
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    big = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.full((200, 3), 7.0, device=DEV)
    dist = torch.full((100,), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((100,), 7, dtype=torch.int32, device=DEV)
    keep = torch.full((100,), 7, dtype=torch.uint8, device=DEV)
    n64, n64b, r32 = C.c_int64(), C.c_int64(), C.c_int32()

    def sample(F=1, V=3, thresh=0.25, ws=big.numel(), v=p(verts), t=p(tris)):
        return L.gsr_mesh_sample_count(v, t, F, V, thresh, p(big), ws, C.byref(n64), stream)
    assert [sample(F=-1), sample(V=-1), sample(thresh=0.0), sample(thresh=-1.0), sample(thresh=float("nan")), sample(ws=8),
            sample(v=None), sample(t=None)] == [INVALID] * 8
    assert sample(F=2 ** 31) == UNSUPPORTED
    assert L.gsr_mesh_sample_emit(p(verts), p(tris), 1, 3, 0.25, p(big), big.numel(), None, stream) == INVALID

    def down(n=100, thresh=0.2, ws=big.numel(), pp=p(pts), k=p(keep)):
        return L.gsr_points_downsample(pp, n, thresh, p(big), ws, k, C.byref(r32), stream)
    assert [down(n=-1), down(thresh=0.0), down(thresh=-0.2), down(ws=64), down(pp=None), down(k=None)] == [INVALID] * 6
    assert down(n=2 ** 31) == UNSUPPORTED

    def near(nq=100, nc=100, md=1.0, ws=big.numel(), q=p(pts), c=p(pts), d=p(dist), i=p(idx)):
        return L.gsr_points_nearest(q, nq, c, nc, md, p(big), ws, d, i, stream)
    assert [near(nq=-1), near(nc=-1), near(md=0.0), near(md=-1.0), near(md=float("nan")), near(ws=64), near(q=None), near(c=None),
            near(d=None), near(i=None)] == [INVALID] * 10
    assert near(nq=2 ** 31) == UNSUPPORTED and near(nc=2 ** 31) == UNSUPPORTED

    obs = torch.ones(8, dtype=torch.uint8, device=DEV)
    shape, bb = np.array([2, 2, 2], np.int32), np.array([0, 0, 0, 1, 1, 1], np.float32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)

    def obsf(n=100, res=1.0, patch=1.0, ws=big.numel(), pp=p(pts), m=p(obs), sh=hp(shape)):
        return L.gsr_points_obs_filter_count(pp, n, m, sh, hp(bb), res, patch, p(big), ws, None, None, C.byref(n64),
                                             C.byref(n64b), stream)
    assert [obsf(n=-1), obsf(res=0.0), obsf(patch=-1.0), obsf(ws=64), obsf(pp=None), obsf(m=None), obsf(sh=None),
            obsf(sh=hp(np.array([2, 0, 2], np.int32)))] == [INVALID] * 8
    assert L.gsr_points_obs_filter_emit(p(pts), -1, p(big), big.numel(), p(out), p(out), stream) == INVALID
    assert L.gsr_points_obs_filter_emit(p(pts), 100, p(big), 64, p(out), p(out), stream) == INVALID
    plane = np.array([0.0, 0, 1, 0])
    assert L.gsr_points_plane_filter(p(pts), -1, hp(plane), p(keep), stream) == INVALID
    assert L.gsr_points_plane_filter(p(pts), 100, None, p(keep), stream) == INVALID
    assert L.gsr_points_plane_filter(None, 100, hp(plane), p(keep), stream) == INVALID
    assert L.gsr_points_gather(p(pts), 100, None, 5, p(out), stream) == INVALID
    assert L.gsr_points_gather(p(pts), -1, p(idx), 5, p(out), stream) == INVALID
    assert L.gsr_dist_mean(p(dist), -1, p(big), big.numel(), p(dist), None, stream) == INVALID
    assert L.gsr_dist_mean(None, 100, p(big), big.numel(), p(dist), None, stream) == INVALID
    assert L.gsr_dist_mean(p(dist), 100, p(big), 64, p(dist), None, stream) == INVALID
    assert L.gsr_dist_mean(p(dist), 100, p(big), big.numel(), None, None, stream) == INVALID
    torch.cuda.synchronize()
    # nothing ran
    assert not big.any() and (out == 7.0).all() and (dist == 7.0).all() and (idx == 7).all() and (keep == 7).all()
    assert "ws_bytes" in L.gsr_last_error().decode() or "mean_out" in L.gsr_last_error().decode()
    assert sample() == 0 and n64.value == 3 + 6
