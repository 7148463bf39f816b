"""Mesh culling by visibility without a GPU: the two measured constants of tests/mesh_vis_ref.py, the host path against the
float64 restatement under the interval test (depth) and the count bounds (vote), the camera and trajectory helpers, VIS_COMPACT,
the argument checks of gsr_mesh_depth_* / gsr_mesh_vis_* (they run before any device work) and the command line with --host."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mesh_vis_ref as R
from gaussmart_amd import _lib
from gaussmart_amd import mesh_visibility as MV
from gaussmart_amd.mesh import TriangleMesh

GSR_E_INVALID, GSR_E_UNSUPPORTED = -1, -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tnt_traj.npz")

# (scene, H, W, focal length, views used)
DEPTH_CASES = {"two_96x64": ("two", 64, 96, 60.0, 3), "two_33x17": ("two", 17, 33, 20.0, 3), "sub_96x64": ("sub", 64, 96, 60.0, 1)}


def _scene(name):
    return {"two": R.two_sphere_scene, "sub": R.subpixel_scene}[name]()


def _mesh(sc):
    return TriangleMesh(sc["verts"], sc["tris"], np.zeros_like(sc["verts"]))


def _five(case, view):
    name, H, W, f, _ = DEPTH_CASES[case]
    sc = _scene(name)
    return R.cached(("five", case, view), lambda: R.five_rasters(sc["verts"], sc["tris"], sc["w2c"][view], H, W, R.intrinsics(H, W, f)))


# ---------------------------------------------------------------- 1. the constants
def test_measured_constants_are_what_the_file_says():
    px, rel = [], []
    for case, (name, H, W, f, n) in DEPTH_CASES.items():
        sc, intr = _scene(name), R.intrinsics(H, W, f)
        px.append(R.measure_px(sc["verts"], sc["w2c"][:n], H, W, intr))
        rel.append(R.measure_rel(sc["verts"], sc["tris"], sc["w2c"][:n], H, W, intr))
        print(f"{case}: float32 vs float64 projection {px[-1]:.3e} px, depth {rel[-1]:.3e} relative")
    vs = R.vote_scene()
    px.append(R.measure_px(vs["verts"], vs["w2c"], vs["H"], vs["W"], vs["intr"]))
    print(f"vote scene: projection {px[-1]:.3e} px;  DELTA_PX {R.DELTA_PX:.3e}, TAU {R.TAU:.3e}")
    assert 0.9 * R.MEASURED_PX <= max(px) <= R.MEASURED_PX and R.DELTA_PX == 4 * R.MEASURED_PX
    assert 0.9 * R.MEASURED_REL <= max(rel) <= R.MEASURED_REL and R.TAU == 4 * R.MEASURED_REL


# ---------------------------------------------------------------- 2. host path: depth
@pytest.mark.parametrize("case", list(DEPTH_CASES))
def test_host_depth_passes_the_interval_test_and_has_no_cracks(case):
    name, H, W, f, n = DEPTH_CASES[case]
    sc, intr = _scene(name), R.intrinsics(H, W, f)
    got = MV.render_mesh_depth_host(_mesh(sc), sc["w2c"][:n], H, W, *intr)
    assert got.dtype == np.float32 and got.shape == (n, H, W)
    for i in range(n):
        five = _five(case, i)
        bad, mixed = R.depth_interval_errors(got[i], five)
        all_hit = (five > 0).all(0)
        print(f"{case} view {i}: hit {int((got[i] > 0).sum())} of {H * W}, five-sample disagreement at {int(mixed.sum())}, "
              f"outside the interval {int(bad.sum())}")
        assert not bad.any()
        assert (got[i][all_hit] > 0).all()              # a closed mesh has no cracks
        assert 0.1 < all_hit.mean() < 0.6               # silhouettes and background are in the picture


def test_host_depth_sees_the_near_sphere_in_front():
    sc = R.two_sphere_scene()
    H, W = 64, 96
    intr = R.intrinsics(H, W, 60.0)
    d, tri = R.raster64(sc["verts"], sc["tris"], sc["w2c"][0], H, W, intr)
    both = R.raster64(sc["verts"], sc["tris"][1196:], sc["w2c"][0], H, W, intr)[0]
    hidden = (tri >= 0) & (tri < 1196) & (both > 0)         # the far sphere would show here without the near one
    assert hidden.sum() > 50 and (d[hidden] < both[hidden]).all()


# ---------------------------------------------------------------- 3. host path: vote
def _vote_depths():
    vs = R.vote_scene()
    return R.cached("vote_depths_host", lambda: MV.render_mesh_depth_host(_mesh(vs), vs["w2c"], vs["H"], vs["W"], *vs["intr"]))


def test_vote_fixture_decides_99_percent_in_float64():
    vs = R.vote_scene()
    s, u, seen = R.cached("vote_bounds_host", lambda: R.vote_bounds(vs["verts"], vs["w2c"], _vote_depths(), vs["intr"]))
    print(f"vote scene: {int(u.sum())} unstable pairs of {seen.size}")
    for mv in (1, 3, 5):
        decided = (s >= mv) | (s + u < mv)
        kept = seen.sum(0) >= mv
        print(f"  min_views {mv}: {int((~decided).sum())} undecided vertices of {len(s)}, {int(kept.sum())} kept")
        assert decided.mean() >= 0.99
        assert 0.05 < kept.mean() < 0.95                # both outcomes occur


@pytest.mark.parametrize("min_views", [1, 3, 5])
def test_host_vote_lies_within_the_bounds(min_views):
    vs = R.vote_scene()
    s, u, seen = R.cached("vote_bounds_host", lambda: R.vote_bounds(vs["verts"], vs["w2c"], _vote_depths(), vs["intr"]))
    cnt = MV.visibility_counts_host(vs["verts"], vs["w2c"], _vote_depths(), *vs["intr"])
    assert cnt.dtype == np.int32 and ((cnt >= s) & (cnt <= s + u)).all()
    clamped = MV.visibility_counts_host(vs["verts"], vs["w2c"], _vote_depths(), *vs["intr"], min_views=min_views)
    assert np.array_equal(clamped, np.minimum(cnt, min_views))
    decided = (s >= min_views) | (s + u < min_views)
    assert np.array_equal((cnt >= min_views)[decided], (seen.sum(0) >= min_views)[decided])


def test_vote_special_vertices_and_empty_images():
    vs = R.vote_scene()
    H, W, intr = vs["H"], vs["W"], vs["intr"]
    verts = np.array([[0, 0, 0], [50, 0, 0], [0, 0, 9], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    zeros = np.zeros((len(vs["w2c"]), H, W), np.float32)
    cnt = MV.visibility_counts_host(verts, vs["w2c"], zeros, *intr)
    # a depth image of all zeros: every in-frustum vertex is seen; outside the frame, behind the camera, NaN and inf are not
    assert cnt.tolist() == [8, 0, 0, 0, 0]
    assert np.array_equal(R.vote64(verts, vs["w2c"], zeros, intr).sum(0), cnt)
    assert MV.visibility_counts_host(verts, vs["w2c"][:0], zeros[:0], *intr).tolist() == [0] * 5


# ---------------------------------------------------------------- 4. cameras and trajectories
def test_w2c_from_c2w_against_numpy_inverse():
    c2w = R.ring_cameras(5, seed=2)
    want = np.linalg.inv(c2w)[:, :3].astype(np.float32)
    assert np.array_equal(MV.w2c_from_c2w(c2w, opengl=False), want)
    assert np.array_equal(MV.w2c_from_c2w(c2w[:, :3], opengl=False), want)
    gl = c2w.copy()
    gl[:, :3, 1:3] *= -1
    got = MV.w2c_from_c2w(gl)                         # OpenGL poses: columns 1 and 2 negated first
    assert got.dtype == np.float32 and got.shape == (5, 3, 4) and np.array_equal(got, want)
    assert MV.w2c_from_c2w(np.zeros((0, 4, 4))).shape == (0, 3, 4)
    with pytest.raises(ValueError):
        MV.w2c_from_c2w(np.eye(4))


def test_load_trajectory_against_the_reference_helper(tmp_path):
    g = np.load(GOLDEN)
    c2w, order, want = g["c2w_in"], g["frame_order"], g["reference_out"]
    frames = [{"file_path": f"images/frame_{int(k) + 1:05d}.png", "transform_matrix": c2w[k].tolist()} for k in order]
    with open(tmp_path / "transforms.json", "w") as f:
        json.dump({"frames": frames}, f)
    got = MV.load_trajectory(str(tmp_path / "transforms.json"))
    assert got.dtype == np.float64 and got.shape == (12, 4, 4) and np.array_equal(got[:, 3], np.tile([0, 0, 0, 1.0], (12, 1)))
    diff = float(np.abs(got[:, :3] - want).max())
    print(f"load_trajectory vs the reference helper's float32 output: {diff:.2e}")
    assert diff <= 1e-6
    assert np.abs(got[:, :3, 3]).max() == 1.0
    np.save(tmp_path / "t44.npy", c2w)
    np.save(tmp_path / "t34.npy", c2w[:, :3])
    assert np.array_equal(MV.load_trajectory(str(tmp_path / "t44.npy"))[:, :3], c2w[:, :3])       # .npy: as they are
    assert np.array_equal(MV.load_trajectory(str(tmp_path / "t34.npy")), MV.load_trajectory(str(tmp_path / "t44.npy")))
    with pytest.raises(ValueError):
        MV.load_trajectory(str(tmp_path / "poses.txt"))


# ---------------------------------------------------------------- 5. VIS_COMPACT
def test_compaction_equals_plain_numpy():
    vs = R.vote_scene()
    rng = np.random.default_rng(1)
    cols = rng.random(vs["verts"].shape).astype(np.float32)
    tris = np.concatenate([vs["tris"], [[5, 5, 6], [7, 7, 7]]]).astype(np.int32)           # degenerate triangles stay
    keep = rng.random(len(vs["verts"])) < 0.8
    keep[[5, 6, 7]] = True
    got = MV.compact_host(TriangleMesh(vs["verts"], tris, cols), keep)
    v, c, t = R.compact_ref(vs["verts"], cols, tris, keep)
    assert got.vertices.tobytes() == v.tobytes() and got.vertex_colors.tobytes() == c.tobytes() and np.array_equal(got.triangles, t)
    assert 0 < len(t) < len(tris) and len(v) < keep.sum()                                    # kept but unused vertices go
    assert np.array_equal(np.unique(t), np.arange(len(v)))                                   # no unreferenced vertex
    none = MV.compact_host(TriangleMesh(vs["verts"], tris[:0], cols), keep)
    assert len(none.vertices) == 0 and len(none.triangles) == 0


# ---------------------------------------------------------------- 6. ABI rejections (no device work)
def _err():
    return _lib.lib().gsr_last_error().decode()


HOST = (C.c_int32 * 64)()          # never dereferenced: the checks return first


def _render(n_tris=5, n_verts=10, n_views=2, H=8, W=8, near=0.01, far=20.0, verts=HOST, tris=HOST, w2c=HOST, out=HOST, ws=HOST,
            ws_bytes=None, fx=10.0):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.gsr_mesh_depth_workspace_bytes(max(n_tris, 0), max(n_views, 0))
    return L.gsr_mesh_depth_render(verts, tris, n_tris, n_verts, w2c, n_views, H, W, fx, 10.0, 4.0, 4.0, near, far, out, ws,
                                   ws_bytes, None)


def test_depth_render_rejects_bad_arguments():
    for kw, word in ((dict(n_tris=-1), "n_tris"), (dict(n_verts=-1), "n_verts"), (dict(n_views=-1), "n_views"), (dict(H=0), "H "),
                     (dict(W=-2), "W "), (dict(near=20.0), "near"), (dict(near=30.0), "near"), (dict(near=0.0), "near"),
                     (dict(far=float("inf")), "far"), (dict(near=float("nan")), "near"), (dict(fx=0.0), "fx"),
                     (dict(out=None), "depth_out"), (dict(w2c=None), "w2c_host"), (dict(verts=None), "verts"),
                     (dict(tris=None), "verts"), (dict(n_verts=0), "n_verts"), (dict(ws=None), "ws_bytes"), (dict(ws_bytes=8), "ws_bytes")):
        assert _render(**kw) == GSR_E_INVALID, kw
        assert _err().startswith(word), (_err(), word)
    assert _render(n_tris=2 ** 31) == GSR_E_UNSUPPORTED and "n_tris" in _err()
    assert _render(n_tris=2 ** 30, n_verts=2 ** 30, n_views=4) == GSR_E_UNSUPPORTED and "fewer views" in _err()
    assert _render(n_views=0, out=None, w2c=None, ws=None, ws_bytes=0) == 0
    L = _lib.lib()
    assert L.gsr_mesh_depth_workspace_bytes(1000, 3) >= 4 * 3000 + 48 * 3 + 4


def test_vis_count_and_compact_reject_bad_arguments():
    L = _lib.lib()
    intr = (C.c_float * 4)(10, 10, 4, 4)
    def count(n_verts=10, n_views=2, H=8, W=8, verts=HOST, depths=HOST, w2c=HOST, k=intr, counts=HOST):
        return L.gsr_mesh_vis_count(verts, n_verts, depths, n_views, H, W, w2c, k, 0.005, 20, counts, None)
    for kw, word in ((dict(n_verts=-1), "n_verts"), (dict(n_views=-1), "n_views"), (dict(H=0), "H "), (dict(W=0), "W "),
                     (dict(k=None), "intrinsics"), (dict(verts=None), "verts"), (dict(depths=None), "depths"),
                     (dict(w2c=None), "w2c_host"), (dict(counts=None), "counts_inout")):
        assert count(**kw) == GSR_E_INVALID, kw
        assert _err().startswith(word), (_err(), word)
    assert count(n_verts=0, verts=None, counts=None) == 0 and count(n_views=0, depths=None, w2c=None) == 0
    need = L.gsr_mesh_vis_workspace_bytes(5, 10)
    def compact(n_tris=5, n_verts=10, tris=HOST, counts=HOST, ws=HOST, ws_bytes=need):
        nv, nt = C.c_int64(-7), C.c_int64(-7)
        rc = L.gsr_mesh_vis_compact_count(tris, n_tris, n_verts, counts, 20, ws, ws_bytes, None, C.byref(nv), C.byref(nt), None)
        return rc, nv.value, nt.value
    for kw, word in ((dict(n_tris=-1), "n_tris"), (dict(n_verts=-1), "n_verts"), (dict(n_verts=0), "n_verts"),
                     (dict(counts=None), "counts"), (dict(tris=None), "tris"), (dict(ws=None), "ws_bytes"),
                     (dict(ws_bytes=need - 1), "ws_bytes")):
        assert compact(**kw) == (GSR_E_INVALID, 0, 0), kw
        assert _err().startswith(word), (_err(), word)
    assert compact(n_tris=0, n_verts=0, tris=None, counts=None) == (0, 0, 0)
    assert L.gsr_mesh_vis_compact_count(HOST, 5, 10, HOST, 20, HOST, need, None, None, None, None) == GSR_E_INVALID
    def emit(n_tris=5, n_verts=10, verts=HOST, cols=HOST, tris=HOST, ws=HOST, ws_bytes=need, vo=HOST, co=HOST, to=HOST):
        return L.gsr_mesh_vis_emit(verts, cols, tris, n_tris, n_verts, ws, ws_bytes, vo, co, to, None)
    for kw in (dict(n_tris=-1), dict(n_verts=0), dict(verts=None), dict(tris=None), dict(vo=None), dict(to=None), dict(co=None),
               dict(ws=None), dict(ws_bytes=need - 1)):
        assert emit(**kw) == GSR_E_INVALID, kw
    assert emit(n_tris=0) == 0


def test_device_functions_have_no_cpu_path():
    import torch
    vs = R.vote_scene()
    with pytest.raises(ValueError, match="device="):
        MV.cull_mesh_by_visibility(_mesh(vs), R.ring_cameras(2), 8, 8, 10, 10, 4, 4)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        MV.visibility_counts(torch.zeros(3, 3), np.zeros((0, 3, 4)), torch.zeros(0, 8, 8), 10, 10, 4, 4)
    with pytest.raises(ValueError, match="near"):
        MV.render_mesh_depth_host(_mesh(vs), vs["w2c"], 8, 8, 10, 10, 4, 4, near=2.0, far=1.0)


# ---------------------------------------------------------------- 7. the whole host path and the command line
def _gl(c2w):
    gl = np.array(c2w)
    gl[:, :3, 1:3] *= -1
    return gl


def test_cull_host_end_to_end_and_cli(tmp_path, capsys):
    from gaussmart_amd import tnt_cull_cli
    vs = R.vote_scene()
    H, W, (fx, fy, cx, cy) = vs["H"], vs["W"], vs["intr"]
    c2w = _gl(R.ring_cameras(8, seed=7))
    cols = np.random.default_rng(2).random(vs["verts"].shape).astype(np.float32)
    mesh = TriangleMesh(vs["verts"], vs["tris"], cols)
    out, keep = MV.cull_mesh_by_visibility_host(mesh, c2w, H, W, fx, fy, cx, cy, min_views=3, return_keep=True)
    assert np.array_equal(MV.w2c_from_c2w(c2w), vs["w2c"])
    cnt = MV.visibility_counts_host(vs["verts"], vs["w2c"], _vote_depths(), fx, fy, cx, cy)
    assert np.array_equal(keep, cnt >= 3) and 0.05 < keep.mean() < 0.5
    v, c, t = R.compact_ref(vs["verts"], cols, vs["tris"], keep)
    assert out.vertices.tobytes() == v.tobytes() and out.vertex_colors.tobytes() == c.tobytes() and np.array_equal(out.triangles, t)
    assert (np.linalg.norm(out.vertices, axis=1) > 0.9).all()          # nothing of the hidden inner sphere is left
    mesh.write_ply(str(tmp_path / "m.ply"))
    np.save(tmp_path / "traj.npy", c2w)
    args = ["--traj-path", str(tmp_path / "traj.npy"), "--ply-path", str(tmp_path / "m.ply"), "--min-views", "3", "--host",
            "--intrinsics", str(fx), str(fy), str(cx), str(cy), "--size", str(W), str(H)]
    assert tnt_cull_cli.main(args) == 0
    text = capsys.readouterr().out
    got = TriangleMesh.read_ply(str(tmp_path / "m_cull.ply"))
    want = MV.cull_mesh_by_visibility_host(TriangleMesh.read_ply(str(tmp_path / "m.ply")), c2w, H, W, fx, fy, cx, cy, min_views=3)
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.triangles, want.triangles)
    assert f"num vertices culled {len(want.vertices)}, num triangles culled {len(want.triangles)}" in text and "8 camera views" in text
    assert tnt_cull_cli.main(args + ["--out", str(tmp_path / "other.ply")]) == 0 and os.path.isfile(tmp_path / "other.ply")
    capsys.readouterr()
    assert tnt_cull_cli.main(["--traj-path", str(tmp_path / "none.npy"), "--ply-path", str(tmp_path / "m.ply"), "--host"]) == 2
    assert "no such file" in capsys.readouterr().err
