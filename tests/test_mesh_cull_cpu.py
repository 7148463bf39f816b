"""Mesh culling by view masks without a GPU: the host half of CULL_PROJECT against a decomposition of P, the reference's float32
expression against the float64 restatement on the fixtures (with the stability rule and its DELTA checked), the host path, the
argument checks of gsr_mask_dilate_disk / gsr_mesh_cull_* (they run before any device work), and the loader and the command
line with --host."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_cull_ref as R
from gaussmart_amd import _lib
from gaussmart_amd.mesh import DeviceTriangleMesh, TriangleMesh

GSR_E_INVALID, GSR_E_UNSUPPORTED = -1, -4


# ---------------------------------------------------------------- 1. dtu_projection
def _random_camera(rng):
    f = rng.uniform(200, 3000)
    K = np.array([[f, rng.uniform(-2, 2), rng.uniform(100, 900)], [0, f * rng.uniform(0.9, 1.1), rng.uniform(100, 700)], [0, 0, 1]])
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = q, rng.uniform(-3, 3, 3)
    wm = np.eye(4)
    wm[:3, :4] = rng.uniform(0.01, 50) * (K @ w2c[:3, :4])
    sm = np.eye(4)
    sm[:3, :3] *= rng.uniform(0.2, 5)
    sm[:3, 3] = rng.uniform(-2, 2, 3)
    return wm.astype(np.float32), sm.astype(np.float32)


def test_dtu_projection_matches_the_decomposition():
    from gaussmart_amd.mesh_cull import dtu_projection
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(20):
        wm, sm = _random_camera(rng)
        P = (wm.astype(np.float64) @ sm.astype(np.float64))[:3, :4]
        intr, pose = R.decompose_P(P)
        assert (np.diag(intr)[:3] > 0).all() and intr[2, 2] == 1.0
        want = (intr @ np.linalg.inv(pose))[:3, :4]
        got = dtu_projection(wm, sm, dtype=np.float64)
        assert got.dtype == np.float64 and got.shape == (3, 4)
        rel = np.abs(got - want).max() / np.abs(want).max()
        worst = max(worst, rel)
        assert rel <= 1e-6, rel
        got32 = dtu_projection(wm, sm)
        assert got32.dtype == np.float32 and np.array_equal(got32, got.astype(np.float32))
        assert abs(np.linalg.norm(got[2, :3]) - 1) < 1e-12          # the third row carries camera depth
    print(f"dtu_projection vs rq decomposition: worst relative difference {worst:.3e}")


def test_dtu_projection_refuses_non_positive_determinant():
    from gaussmart_amd.mesh_cull import dtu_projection
    wm, sm = _random_camera(np.random.default_rng(2))
    neg = wm.copy()
    neg[:3] = -neg[:3]
    with pytest.raises(ValueError, match="det"):
        dtu_projection(neg, sm)
    flat = wm.copy()
    flat[2, :3] = flat[1, :3]
    with pytest.raises(ValueError, match="det"):
        dtu_projection(flat, sm)
    with pytest.raises(ValueError, match="4x4"):
        dtu_projection(wm[:3], sm)


# ---------------------------------------------------------------- 2. float32 expression vs float64 restatement
@pytest.mark.parametrize("name", ["hemi", "vote"])
def test_float32_expression_agrees_on_stable_vertices(name):
    fx = {"hemi": R.hemisphere_fixture, "vote": R.vote_fixture}[name]()
    r64 = R.fixture_restated(name)
    keep32, cx32, cy32 = R.reference_torch32(fx["verts"], fx["world_mats"], fx["scale_mats"], fx["masks"], fx["radius"],
                                             fx["norm_hw"])
    measured = R.measured_delta(r64, cx32, cy32)
    stable = R.stable_vertices(r64)
    share, kept = 1 - stable.mean(), r64["keep"].mean()
    print(f"{name}: float32 vs float64 pixel difference {measured:.3e} px, DELTA {R.DELTA:.3e}, unstable share {share:.4%}, "
          f"kept share {kept:.2%}, disagreements {(keep32 != r64['keep']).sum()}")
    # DELTA is what the docstring of mesh_cull_ref says it is
    assert measured <= R.MEASURED_F32_VS_F64 and 4 * R.MEASURED_F32_VS_F64 <= R.DELTA <= 4.2 * R.MEASURED_F32_VS_F64
    assert np.array_equal(keep32[stable], r64["keep"][stable])
    assert share <= 0.005
    if name == "hemi":
        assert 0.10 <= kept <= 0.90


def test_vote_fixture_has_every_case():
    fx, r = R.vote_fixture(), R.fixture_restated("vote")
    valid, sample, keeps = r["valid"], r["sample"], r["keeps"]
    for what, m in (("removed by the mask", valid & ~sample), ("kept because invalid", ~valid),
                    ("kept because inside the mask", valid & sample)):
        assert m.any(1).sum() >= 3, what
        assert m[:3].any(), what                        # ... already among the first three views
    assert np.array_equal(keeps, ~(valid & ~sample))
    P, v = fx["proj"].astype(np.float64), fx["verts"].astype(np.float64)
    finite = np.isfinite(v).all(1)
    depth2 = v[finite] @ P[2, 2, :3] + P[2, 2, 3]
    assert (depth2 < 0).any() and (depth2 > 0).any()          # view 2: part of the sphere behind the camera ...
    assert (valid[2][finite] & (depth2 < 0)).any()          # ... some of it mirrored into the frame, handled as the formula says
    assert 0.2 < (~valid[1]).mean() < 0.8                     # view 1: part outside the frame
    assert not np.isfinite(fx["verts"][0]).all() and not valid[:, 0].any() and r["keep"][0]        # the NaN vertex is kept
    assert fx["norm_hw"] != fx["masks"].shape[1:]
    assert len(np.unique(fx["masks"])) > 3                    # set pixels with values other than 1 / 255


def test_zero_views_keep_everything():
    v = R.sphere_vertices(50)
    r = R.restate64(v, np.zeros((0, 3, 4), np.float32), np.zeros((0, 4, 4), np.uint8), 24)
    assert r["keep"].all() and R.stable_vertices(r).all()


# ---------------------------------------------------------------- 3. host path
def _mesh_of(fx):
    v = fx["verts"]
    rng = np.random.default_rng(8)
    return TriangleMesh(v, R.neighbour_triangles(v), rng.random((len(v), 3)).astype(np.float32))


@pytest.mark.parametrize("name", ["hemi", "vote"])
def test_host_path_equals_restatement_and_its_own_compaction(name):
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks_host, dilate_masks_host
    fx = {"hemi": R.hemisphere_fixture, "vote": R.vote_fixture}[name]()
    r64 = R.fixture_restated(name)
    stable = R.stable_vertices(r64)
    assert np.array_equal(dilate_masks_host(fx["masks"], fx["radius"]), r64["dilated"])
    m = _mesh_of(fx)
    s, t = 2.5, np.array([0.25, -1.5, 3.0], np.float32)
    out, keep = cull_mesh_by_masks_host(m, fx["proj"], fx["masks"], fx["radius"], norm_size=fx["norm_hw"], scale=s, offset=t,
                                        return_keep=True)
    assert keep.dtype == np.bool_ and np.array_equal(keep[stable], r64["keep"][stable])
    v, c, tr = R.compact_ref(m.vertices, m.vertex_colors, m.triangles, keep, s, t)
    assert out.vertices.dtype == np.float32 and out.triangles.dtype == np.int32
    assert np.array_equal(out.triangles, tr) and np.array_equal(out.vertex_colors, c)
    assert np.array_equal(out.vertices, v, equal_nan=True)
    assert 0 < len(out.triangles) < len(m.triangles) and len(out.vertices) == int(keep.sum())
    # identity: the vertices are copied
    plain = cull_mesh_by_masks_host(m, fx["proj"], fx["masks"], fx["radius"], norm_size=fx["norm_hw"])
    assert plain.vertices.tobytes() == m.vertices[keep].tobytes()
    # zero views keep the mesh as it is
    same = cull_mesh_by_masks_host(m, np.zeros((0, 3, 4)), np.zeros((0, 240, 320), np.uint8))
    assert same.vertices.tobytes() == m.vertices.tobytes() and np.array_equal(same.triangles, m.triangles)


@pytest.mark.parametrize("r", R.DILATE_RADII)
def test_host_dilation_and_span_table(r):
    """The host path's dilation (an exact Euclidean feature transform) gives what scipy's binary_dilation gives on the
    dilation cases of the device test -- computed here or recorded (tests/golden), which this also checks from another side."""
    from gaussmart_amd.mesh_cull import dilate_masks_host, disk_spans
    for H, W in R.DILATE_SIZES:
        want = R.dilation_expected(H, W, r)
        assert want.shape == (6, H, W) and set(np.unique(want)) <= {0, 1}
        assert np.array_equal(dilate_masks_host(R.dilation_images(H, W), r), want), (H, W, r)
    assert np.array_equal(2 * disk_spans(r) + 1, R.disk(r).sum(1))


# ---------------------------------------------------------------- 4. ABI rejections (no device work)
def _err():
    return _lib.lib().gsr_last_error().decode()


HOST = (C.c_int32 * 64)()          # never dereferenced: the checks return first


def _cull_count(n_tris=5, n_verts=10, n_views=2, H=8, W=8, Wn=8, Hn=8, verts=HOST, tris=HOST, dilated=HOST, proj=HOST,
                ws=HOST, ws_bytes=None, keep=None):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.gsr_mesh_cull_workspace_bytes(max(n_tris, 0), max(n_verts, 0), max(n_views, 0))
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    rc = L.gsr_mesh_cull_count(verts, tris, n_tris, n_verts, dilated, n_views, H, W, Wn, Hn, proj, ws, ws_bytes, keep,
                               C.byref(nv), C.byref(nt), None)
    return rc, nv.value, nt.value


def test_dilate_rejects_bad_arguments():
    L = _lib.lib()
    need = L.gsr_mask_dilate_workspace_bytes(2, 8, 8)
    for args, word in (((HOST, -1, 8, 8, 3, HOST, HOST, need), "n "), ((HOST, 2, 0, 8, 3, HOST, HOST, need), "H "),
                       ((HOST, 2, 8, 0, 3, HOST, HOST, need), "W "), ((HOST, 2, 8, -4, 3, HOST, HOST, need), "W "),
                       ((HOST, 2, 8, 8, -1, HOST, HOST, need), "radius"), ((None, 2, 8, 8, 3, HOST, HOST, need), "masks"),
                       ((HOST, 2, 8, 8, 3, None, HOST, need), "out"), ((HOST, 2, 8, 8, 3, HOST, HOST, need - 1), "ws_bytes"),
                       ((HOST, 2, 8, 8, 3, HOST, None, need), "ws_bytes")):
        assert L.gsr_mask_dilate_disk(*args, None) == GSR_E_INVALID, args
        assert _err().startswith(word), (_err(), word)
    assert L.gsr_mask_dilate_disk(HOST, 2, 8, 8, 128, HOST, HOST, need, None) == GSR_E_UNSUPPORTED and "radius" in _err()
    assert L.gsr_mask_dilate_disk(None, 0, 8, 8, 127, None, None, 0, None) == 0


def test_cull_count_rejects_bad_arguments():
    for kw, word in ((dict(n_tris=-1), "n_tris"), (dict(n_verts=-2), "n_verts"), (dict(n_views=-1), "n_views"),
                     (dict(H=0), "H "), (dict(W=0), "W "), (dict(Wn=0), "Wn "), (dict(Hn=-3), "Hn "),
                     (dict(verts=None), "verts"), (dict(tris=None), "tris"), (dict(dilated=None), "dilated"),
                     (dict(proj=None), "proj_host"), (dict(ws=None), "ws_bytes"), (dict(n_verts=0), "n_verts")):
        rc, nv, nt = _cull_count(**kw)
        assert rc == GSR_E_INVALID and (nv, nt) == (0, 0), kw
        assert _err().startswith(word), (_err(), word)
    need = _lib.lib().gsr_mesh_cull_workspace_bytes(5, 10, 2)
    assert _cull_count(ws_bytes=need - 1)[0] == GSR_E_INVALID and "ws_bytes" in _err()
    assert _cull_count(n_verts=2 ** 31)[0] == GSR_E_UNSUPPORTED and "n_verts" in _err()
    assert _cull_count(n_tris=2 ** 31)[0] == GSR_E_UNSUPPORTED and "n_tris" in _err()
    L = _lib.lib()
    assert L.gsr_mesh_cull_count(HOST, HOST, 5, 10, HOST, 2, 8, 8, 8, 8, HOST, HOST, need, None, None, None, None) == GSR_E_INVALID
    assert "n_verts_out" in _err()
    # zero views need neither masks nor matrices: the next complaint is about something else
    assert _cull_count(n_views=0, dilated=None, proj=None, ws_bytes=0)[0] == GSR_E_INVALID and "ws_bytes" in _err()


def test_cull_emit_rejects_bad_arguments():
    L = _lib.lib()
    need = L.gsr_mesh_cull_workspace_bytes(5, 10, 0)

    def emit(verts=HOST, colors=HOST, tris=HOST, n_tris=5, n_verts=10, so=None, ws=HOST, ws_bytes=need, vo=HOST, co=HOST, to=HOST):
        return L.gsr_mesh_cull_emit(verts, colors, tris, n_tris, n_verts, so, ws, ws_bytes, vo, co, to, None)

    for kw, word in ((dict(n_tris=-3), "n_tris"), (dict(n_verts=-1), "n_verts"), (dict(verts=None), "verts "),
                     (dict(vo=None), "verts_out"), (dict(co=None), "colors_out"), (dict(tris=None), "tris "),
                     (dict(to=None), "tris_out"), (dict(ws_bytes=64), "ws_bytes"), (dict(ws=None), "ws_bytes"),
                     (dict(n_verts=0), "n_verts")):
        assert emit(**kw) == GSR_E_INVALID, kw
        assert _err().startswith(word), (_err(), word)
    assert emit(n_verts=2 ** 31) == GSR_E_UNSUPPORTED and "n_verts" in _err()


def test_cull_workspace_sizes_and_zero_counts():
    L = _lib.lib()
    a = L.gsr_mesh_cull_workspace_bytes(5, 10, 1)
    assert a > 0 and L.gsr_mesh_cull_workspace_bytes(0, 0, 0) > 0
    assert L.gsr_mesh_cull_workspace_bytes(50000, 10, 1) > a and L.gsr_mesh_cull_workspace_bytes(5, 100000, 1) > a
    assert L.gsr_mesh_cull_workspace_bytes(5, 10, 64) > a
    # the emit call knows no view count: its requirement is the view-independent part
    assert L.gsr_mesh_cull_workspace_bytes(5, 10, 0) <= a
    d = L.gsr_mask_dilate_workspace_bytes(1, 8, 8)
    assert d > 0 and L.gsr_mask_dilate_workspace_bytes(0, 8, 8) > 0
    assert L.gsr_mask_dilate_workspace_bytes(3, 240, 320) >= 3 * 240 * 320 > d
    assert L.gsr_mask_dilate_workspace_bytes(4, 240, 320) > L.gsr_mask_dilate_workspace_bytes(3, 240, 320)
    assert _cull_count(n_tris=0, n_verts=0, n_views=0, verts=None, tris=None, dilated=None, proj=None, ws=None, ws_bytes=0) == (0, 0, 0)
    assert _cull_count(n_tris=0, n_verts=0, n_views=3, verts=None, tris=None, ws=None, ws_bytes=0) == (0, 0, 0)
    assert L.gsr_mesh_cull_emit(None, None, None, 0, 0, None, None, 0, None, None, None, None) == 0


# ---------------------------------------------------------------- 5. loader and command line
def _scene(tmp_path, scan="24"):
    """A DTU directory around the hemisphere fixture, with a scale_mat that is not the identity."""
    fx = R.hemisphere_fixture()
    sm = np.eye(4, dtype=np.float32)
    sm[:3, :3] *= 2.0
    sm[:3, 3] = (0.5, -0.25, 1.0)
    inv = np.linalg.inv(sm.astype(np.float64))
    # the cameras live in world space: world_mat' = world_mat @ inverse(scale_mat), so that P is the fixture's
    wms = [(w.astype(np.float64) @ inv).astype(np.float32) for w in fx["world_mats"]]
    sms = [sm] * len(wms)
    R.write_dtu_dir(tmp_path / "masks", scan, wms, sms, fx["masks"])
    m = _mesh_of(fx)
    m.write_ply(str(tmp_path / "in.ply"))
    return fx, wms, sms, TriangleMesh.read_ply(str(tmp_path / "in.ply"))


def test_load_dtu_instance(tmp_path):
    from gaussmart_amd.mesh_cull import dtu_projection, load_dtu_instance
    fx, wms, sms, _ = _scene(tmp_path)
    inst = load_dtu_instance(str(tmp_path / "masks" / "scan24"))
    assert inst.masks.dtype == np.uint8 and np.array_equal(inst.masks, fx["masks"])          # RGB and single-channel files
    assert inst.proj.dtype == np.float32 and inst.proj.shape == (8, 3, 4)
    assert np.array_equal(inst.proj, np.stack([dtu_projection(w, s) for w, s in zip(wms, sms)]))
    assert np.abs(inst.proj - fx["proj"]).max() <= 2e-6 * np.abs(fx["proj"]).max()
    assert inst.scale == 2.0 and np.array_equal(inst.offset, np.array([0.5, -0.25, 1.0], np.float32))


def test_load_dtu_instance_errors(tmp_path):
    from PIL import Image
    from gaussmart_amd.mesh_cull import load_dtu_instance
    fx, wms, sms, _ = _scene(tmp_path)
    d = tmp_path / "masks" / "scan24"
    with pytest.raises(FileNotFoundError, match="cameras.npz"):
        load_dtu_instance(str(tmp_path / "masks" / "scan25"))
    Image.fromarray(np.zeros((100, 320), np.uint8)).save(d / "mask" / "003.png")
    with pytest.raises(ValueError, match="mask size 320x100 differs from 320x240"):
        load_dtu_instance(str(d))
    Image.fromarray(fx["masks"][3]).save(d / "mask" / "003.png")
    Image.fromarray(fx["masks"][3]).save(d / "mask" / "008.png")
    with pytest.raises(ValueError, match="9 masks but 8 cameras"):
        load_dtu_instance(str(d))


def test_cull_cli_host_end_to_end(tmp_path, capsys):
    from gaussmart_amd import cull_cli
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks_host, load_dtu_instance
    fx, wms, sms, mesh = _scene(tmp_path)
    out_dir = tmp_path / "out"
    args = ["--input_mesh", str(tmp_path / "in.ply"), "--scan_id", "24", "--mask_dir", str(tmp_path / "masks"),
            "--output_dir", str(out_dir), "--host"]
    assert cull_cli.main(args) == 0
    text = capsys.readouterr().out
    got = TriangleMesh.read_ply(str(out_dir / "culled_mesh.ply"))
    inst = load_dtu_instance(str(tmp_path / "masks" / "scan24"))
    want, keep = cull_mesh_by_masks_host(mesh, inst.proj, inst.masks, 24, scale=inst.scale, offset=inst.offset, return_keep=True)
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.triangles, want.triangles)
    assert np.array_equal(got.vertex_colors, want.vertex_colors)
    assert f"num vertices raw {len(mesh.vertices)}, num triangles raw {len(mesh.triangles)}" in text
    assert f"num vertices culled {len(want.vertices)}, num triangles culled {len(want.triangles)}" in text
    # the scene is the hemisphere fixture seen through another scale_mat: the same vertices stay (stable ones), in world space
    r64 = R.fixture_restated("hemi")
    stable = R.stable_vertices(r64)
    assert np.array_equal(keep[stable], r64["keep"][stable]) and 0 < keep.sum() < len(keep)
    assert np.allclose(got.vertices, mesh.vertices[keep] * 2.0 + np.array([0.5, -0.25, 1.0]), rtol=0, atol=1e-6)
    # another radius gives another mesh
    assert cull_cli.main(args[:-1] + ["--radius", "0", "--host"]) == 0
    assert len(TriangleMesh.read_ply(str(out_dir / "culled_mesh.ply")).vertices) < len(want.vertices)
    capsys.readouterr()


def test_cull_cli_errors(tmp_path, capsys):
    from PIL import Image
    from gaussmart_amd import cull_cli
    _scene(tmp_path)
    base = ["--scan_id", "24", "--mask_dir", str(tmp_path / "masks"), "--output_dir", str(tmp_path / "out"), "--host"]
    assert cull_cli.main(["--input_mesh", str(tmp_path / "missing.ply")] + base) != 0
    assert "missing.ply" in capsys.readouterr().err
    assert cull_cli.main(["--input_mesh", str(tmp_path / "in.ply"), "--scan_id", "99"] + base[2:]) != 0
    assert "cameras.npz" in capsys.readouterr().err
    Image.fromarray(np.zeros((10, 10), np.uint8)).save(tmp_path / "masks" / "scan24" / "mask" / "000.png")
    assert cull_cli.main(["--input_mesh", str(tmp_path / "in.ply")] + base) != 0
    assert "differs" in capsys.readouterr().err
    assert not (tmp_path / "out" / "culled_mesh.ply").exists()


def test_cull_mesh_by_masks_has_no_cpu_path():
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks, dilate_masks
    fx = R.hemisphere_fixture()
    m = _mesh_of(fx)
    with pytest.raises(ValueError, match="device="):
        cull_mesh_by_masks(m, fx["proj"], fx["masks"])
    d = DeviceTriangleMesh(torch.from_numpy(m.vertices), torch.from_numpy(m.triangles), torch.from_numpy(m.vertex_colors))
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        cull_mesh_by_masks(d, fx["proj"], fx["masks"])
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        dilate_masks(torch.from_numpy(fx["masks"]))
