"""Mesh culling by view masks on the device: the disk dilation against scipy.ndimage.binary_dilation (exactly), the vote against
the float64 restatement on stable vertices (tests/mesh_cull_ref.py), the compaction against numpy bit for bit, the hand-over
from marching cubes and the cluster filter, view chunking, and the command line."""
import contextlib
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_cull_ref as R
from test_gpu_mesh import _sphere_cams, _sphere_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _device_mesh(verts, tris, cols=None):
    from gaussmart_amd.mesh import DeviceTriangleMesh
    return DeviceTriangleMesh(torch.from_numpy(verts).to(DEV), torch.from_numpy(tris).to(DEV),
                              None if cols is None else torch.from_numpy(cols).to(DEV))


# ---------------------------------------------------------------- 1. dilation
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("r", R.DILATE_RADII)
@pytest.mark.parametrize("size", R.DILATE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dilation_equals_scipy(size, r, n):
    from gaussmart_amd.mesh_cull import dilate_masks
    H, W = size
    imgs = R.dilation_images(H, W)                      # zero, set, corner / border pixels, checkerboard, blobs, values > 1
    want = R.dilation_expected(H, W, r)
    dev = torch.from_numpy(imgs).to(DEV)
    for a in range(0, len(imgs), n):
        got = dilate_masks(dev[a:a + n], r)
        again = dilate_masks(dev[a:a + n].clone(), r)
        assert got.dtype == torch.uint8 and got.shape == (n, H, W) and got.device == DEV
        assert torch.equal(got, again)
        g = got.cpu().numpy()
        assert g.max(initial=0) <= 1
        assert np.array_equal(g, want[a:a + n]), (size, r, n, a, int((g != want[a:a + n]).sum()))


def test_dilation_rejects_a_radius_above_127():
    from gaussmart_amd import _lib
    from gaussmart_amd.mesh_cull import dilate_masks
    with pytest.raises(_lib.GsrError, match="radius"):
        dilate_masks(torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV), 128)
    assert dilate_masks(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV), 3).shape == (0, 8, 8)


# ---------------------------------------------------------------- 2. vote
@pytest.mark.parametrize("n", [0, 1, 3, 8])
@pytest.mark.parametrize("V", [0, 1, 63, 64, 65, 4097, 6000])
def test_vote_matches_float64_restatement(V, n):
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks
    fx = R.vote_fixture()
    verts = np.ascontiguousarray(fx["verts"][:V])
    proj, masks = fx["proj"][:n], fx["masks"][:n]
    r64 = R.fixture_restated("vote")
    want = r64["keeps"][:n, :V].all(0)
    sub = {k: (v[:n, :V] if k != "dilated" else v[:n]) for k, v in r64.items() if k != "keep"}
    stable = R.stable_vertices(sub)
    mesh = _device_mesh(verts, np.zeros((0, 3), np.int32))
    out, keep = cull_mesh_by_masks(mesh, proj, torch.from_numpy(masks).to(DEV), fx["radius"], norm_size=fx["norm_hw"],
                                   return_keep=True)
    keep = keep.cpu().numpy()
    assert keep.dtype == np.uint8 and keep.shape == (V,) and keep.max(initial=0) <= 1
    share = float((~stable).mean()) if V else 0.0
    print(f"vote V={V} n={n}: kept {int(keep.sum())}, unstable share {share:.4%}, "
          f"disagreements with float64 {int((keep.astype(bool) != want).sum())}")
    assert share <= 0.005
    assert np.array_equal(keep.astype(bool)[stable], want[stable])
    assert len(out.vertices) == int(keep.sum()) and len(out.triangles) == 0
    assert out.vertices.cpu().numpy().tobytes() == verts[keep.astype(bool)].tobytes()
    if n == 0:
        assert keep.all()
    if V == 6000 and n >= 3:
        # each way a view can decide occurs, and the device decides it the same way
        valid, sample = sub["valid"], sub["sample"]
        st = stable[None, :]
        removed, invalid, inside = valid & ~sample & st, ~valid & st, valid & sample & st
        assert removed.any() and invalid.any() and inside.any()
        assert not keep[removed.any(0)].any()                                # removed by the mask
        only_invalid = invalid.all(0)                                        # kept because invalid (in every view)
        assert only_invalid.any() and keep[only_invalid].all()
        kept_inside = (inside | invalid).all(0) & inside.any(0)              # kept because inside the mask
        assert kept_inside.any() and keep[kept_inside].all()
        behind = (np.nan_to_num(verts.astype(np.float64)) @ proj[2, 2, :3].astype(np.float64) + proj[2, 2, 3]) < 0
        assert (behind & valid[2]).any()                                     # view 2: behind the camera, inside the frame
        assert np.isnan(verts[0]).any() and keep[0] == 1                     # the NaN vertex


# ---------------------------------------------------------------- 3. compaction
def _fma32(a, s, t):
    return (a.astype(np.float64) * np.float64(np.float32(s)) + np.asarray(t, np.float32).astype(np.float64)).astype(np.float32)


def _compaction_mesh():
    fx = R.vote_fixture()
    verts = fx["verts"]
    tris = R.neighbour_triangles(verts)
    r64 = R.fixture_restated("vote")
    kept = np.nonzero(r64["keep"] & R.stable_vertices(r64) & np.isfinite(verts).all(1))[0]
    a, b = int(kept[0]), int(kept[1])
    tris = np.concatenate([tris[:100], np.array([[a, a, b], [b, b, b]], np.int32), tris[100:]])       # degenerate, and kept
    cols = np.random.default_rng(4).random((len(verts), 3)).astype(np.float32)
    return fx, verts, tris, cols, (a, b)


def test_compaction_matches_numpy_bit_for_bit():
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks
    fx, verts, tris, cols, (a, b) = _compaction_mesh()
    masks = torch.from_numpy(fx["masks"]).to(DEV)
    mesh = _device_mesh(verts, tris, cols)
    out, keep = cull_mesh_by_masks(mesh, fx["proj"], masks, fx["radius"], norm_size=fx["norm_hw"], return_keep=True)
    keep = keep.cpu().numpy().astype(bool)
    v, c, t = R.compact_ref(verts, cols, tris, keep)
    got = out.cpu()
    assert got.vertices.tobytes() == v.tobytes()                 # identity: the input's bytes (a NaN vertex among them)
    assert got.vertex_colors.tobytes() == c.tobytes() and np.array_equal(got.triangles, t)
    assert got.triangles.dtype == np.int32 and 0 < len(t) < len(tris)
    remap = np.cumsum(keep) - 1
    assert (got.triangles == [remap[a], remap[a], remap[b]]).all(1).any() and (got.triangles == remap[b]).all(1).any()
    referenced = np.zeros(len(v), bool)
    referenced[t.reshape(-1)] = True
    assert keep[0] and not referenced[remap[0]] and (~referenced).sum() > 1        # kept, although no triangle uses them
    # the input mesh is left as it was
    assert mesh.vertices.cpu().numpy().tobytes() == verts.tobytes() and np.array_equal(mesh.triangles.cpu().numpy(), tris)
    # CULL_TO_WORLD: fmaf(v, s, t) within 1 ulp of the float64 product rounded once; the rest unchanged
    s, off = 211.5, np.array([-4.25, 300.125, 0.001], np.float32)
    world = cull_mesh_by_masks(mesh, fx["proj"], masks, fx["radius"], norm_size=fx["norm_hw"], scale=s, offset=off).cpu()
    want = _fma32(v, s, off)
    fin = np.isfinite(want).all(1)
    assert np.array_equal(np.isfinite(world.vertices).all(1), fin)
    ulp = np.spacing(np.abs(want[fin]))
    assert (np.abs(world.vertices[fin].astype(np.float64) - want[fin].astype(np.float64)) <= ulp).all()
    print(f"to-world: {int((world.vertices[fin] != want[fin]).sum())} of {want[fin].size} components differ from the float64 product")
    assert world.vertex_colors.tobytes() == c.tobytes() and np.array_equal(world.triangles, t)
    # only a scale, only an offset
    assert np.array_equal(cull_mesh_by_masks(mesh, fx["proj"], masks, 24, norm_size=fx["norm_hw"], scale=2.0).cpu().vertices[fin],
                          v[fin] * np.float32(2))
    assert np.array_equal(cull_mesh_by_masks(mesh, fx["proj"], masks, 24, norm_size=fx["norm_hw"], offset=[0, 0, 0]).cpu().vertices[fin],
                          v[fin] + np.float32(0))


def test_compaction_without_triangles_and_without_colours():
    from gaussmart_amd import _lib
    import ctypes as C
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks, dilate_masks
    fx, verts, tris, cols, _ = _compaction_mesh()
    masks = torch.from_numpy(fx["masks"]).to(DEV)
    # F = 0 through the Python layer
    none = cull_mesh_by_masks(_device_mesh(verts, np.zeros((0, 3), np.int32), cols), fx["proj"], masks, 24, norm_size=fx["norm_hw"])
    full, keep = cull_mesh_by_masks(_device_mesh(verts, tris, cols), fx["proj"], masks, 24, norm_size=fx["norm_hw"], return_keep=True)
    assert none.triangles.shape == (0, 3) and torch.equal(none.vertices.view(torch.int32), full.vertices.view(torch.int32))
    assert torch.equal(none.vertex_colors, full.vertex_colors)
    # null colours through the C ABI: colors_out is not touched
    L = _lib.lib()
    V, F, n = len(verts), len(tris), len(masks)
    dv, dt = torch.from_numpy(verts).to(DEV), torch.from_numpy(tris).to(DEV)
    dil = dilate_masks(masks, 24)
    ws = torch.empty(L.gsr_mesh_cull_workspace_bytes(F, V, n), dtype=torch.uint8, device=DEV)
    nv, nt = C.c_int64(), C.c_int64()
    pj = np.ascontiguousarray(fx["proj"]).reshape(-1)
    Hn, Wn = fx["norm_hw"]
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(L.gsr_mesh_cull_count(C.c_void_p(dv.data_ptr()), C.c_void_p(dt.data_ptr()), F, V, C.c_void_p(dil.data_ptr()), n,
                                     240, 320, Wn, Hn, pj.ctypes.data_as(C.c_void_p), C.c_void_p(ws.data_ptr()), ws.numel(),
                                     None, C.byref(nv), C.byref(nt), stream))
    assert (nv.value, nt.value) == (len(full.vertices), len(full.triangles))
    vo = torch.empty((nv.value, 3), dtype=torch.float32, device=DEV)
    to = torch.empty((nt.value, 3), dtype=torch.int32, device=DEV)
    _lib.check(L.gsr_mesh_cull_emit(C.c_void_p(dv.data_ptr()), None, C.c_void_p(dt.data_ptr()), F, V, None,
                                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(vo.data_ptr()), None,
                                    C.c_void_p(to.data_ptr()), stream))
    assert torch.equal(vo.view(torch.int32), full.vertices.view(torch.int32)) and torch.equal(to, full.triangles)
    # null colours together with a scale and an offset: only the vertex kernel runs for the rows
    so = np.array([2.0, 1.0, -2.0, 0.5], np.float32)
    vw = torch.empty_like(vo)
    _lib.check(L.gsr_mesh_cull_emit(C.c_void_p(dv.data_ptr()), None, C.c_void_p(dt.data_ptr()), F, V, so.ctypes.data_as(C.c_void_p),
                                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(vw.data_ptr()), None,
                                    C.c_void_p(to.data_ptr()), stream))
    want = cull_mesh_by_masks(_device_mesh(verts, tris, cols), fx["proj"], masks, 24, norm_size=fx["norm_hw"], scale=2.0,
                              offset=[1.0, -2.0, 0.5])
    assert torch.equal(vw.view(torch.int32), want.vertices.view(torch.int32)) and torch.equal(to, full.triangles)
    fin = torch.isfinite(vo).all(1)
    assert torch.equal(vw[fin], vo[fin] * 2.0 + torch.tensor([1.0, -2.0, 0.5], device=DEV))       # the doubling is exact: one rounding either way


# ---------------------------------------------------------------- 4. hand-over from marching cubes and the cluster filter
def test_handover_from_extraction_and_cluster_filter():
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.mesh import DeviceTriangleMesh, GaussianExtractor, camera_intrinsics, post_process_mesh_device
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks, cull_mesh_by_masks_host, dtu_projection
    from gaussmart_amd.params import PipelineParams
    g = _sphere_model(6000)
    cams = _sphere_cams(12, 128, 128)
    pipe = PipelineParams(depth_ratio=1.0)
    ex = GaussianExtractor(g, render, pipe, bg_color=[0, 0, 0])
    ex.reconstruction(cams)
    dm = _quiet(ex.extract_mesh_bounded, voxel_size=0.02, sdf_trunc=0.08, depth_trunc=5, to_host=False)
    post = _quiet(post_process_mesh_device, dm, 1)
    assert isinstance(post, DeviceTriangleMesh) and len(post.triangles) > 1000
    # the masks: the upper half of the sphere (the surfels with z > 0) as three cameras near the equator see it
    top = g.get_xyz[:, 2] > 0
    half = GaussianModel(3, device=DEV)
    half.create_from_params({k: getattr(g, "_" + k).detach()[top].contiguous()
                             for k in ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity")})
    side = sorted(range(len(cams)), key=lambda i: abs(float(cams[i].camera_center[2])))[:3]
    bg = torch.zeros(3, device=DEV)
    masks, proj = [], []
    for i in side:
        alpha = render(cams[i], half, pipe=pipe, bg_color=bg)["rend_alpha"]
        masks.append(((alpha[0] > 0.5) * 255).to(torch.uint8))
        fx, fy, cx, cy = camera_intrinsics(cams[i])
        wm = np.eye(4)
        wm[:3, :4] = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]) @ cams[i].world_view_transform.T.cpu().numpy().astype(np.float64)[:3]
        proj.append(dtu_projection(wm, np.eye(4)))
    masks, proj = torch.stack(masks), np.stack(proj)
    assert 0.1 < float((masks > 0).float().mean()) < 0.5
    r = 3
    got, keep = cull_mesh_by_masks(post, proj, masks, r, return_keep=True)
    again, keep2 = cull_mesh_by_masks(post, proj, masks, r, return_keep=True)
    for a, b in ((got.vertices, again.vertices), (got.triangles, again.triangles), (got.vertex_colors, again.vertex_colors),
                 (keep, keep2)):
        assert a.shape == b.shape and torch.equal(a, b)
    assert 0 < len(got.vertices) < len(post.vertices) and 0 < len(got.triangles) < len(post.triangles)
    hp = post.cpu()
    host, hkeep = cull_mesh_by_masks_host(hp, proj, masks, r, return_keep=True)
    r64 = R.restate64(hp.vertices, proj, masks.cpu().numpy(), r)
    stable = R.stable_vertices(r64)
    keep = keep.cpu().numpy().astype(bool)
    print(f"hand-over: {len(hp.vertices)} -> {int(keep.sum())} vertices, {len(hp.triangles)} -> {len(got.triangles)} triangles, "
          f"unstable share {float((~stable).mean()):.4%}, device vs host disagreements {int((keep != hkeep).sum())}")
    assert (~stable).mean() <= 0.005
    assert np.array_equal(keep[stable], hkeep[stable]) and np.array_equal(keep[stable], r64["keep"][stable])
    if np.array_equal(keep, hkeep):
        gc = got.cpu()
        assert gc.vertices.tobytes() == host.vertices.tobytes() and np.array_equal(gc.triangles, host.triangles)
    # what is left is the upper half and a rim of the lower one
    z = got.vertices[:, 2]
    assert float(z.min()) > -0.35 and float(z.max()) > 0.95
    assert int((z > 0.1).sum()) >= 0.98 * int((post.vertices[:, 2] > 0.1).sum())


# ---------------------------------------------------------------- 5. view chunking
def test_view_chunks_give_the_same_mesh():
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks
    fx, verts, tris, cols, _ = _compaction_mesh()
    mesh = _device_mesh(verts, tris, cols)
    one, keep1 = cull_mesh_by_masks(mesh, fx["proj"], torch.from_numpy(fx["masks"]).to(DEV), 24, norm_size=fx["norm_hw"],
                                    return_keep=True)
    for masks, budget in ((torch.from_numpy(fx["masks"]).to(DEV), 1), (fx["masks"], 1), (fx["masks"], 3 * 3 * 240 * 320)):
        many, keepn = cull_mesh_by_masks(mesh, fx["proj"], masks, 24, norm_size=fx["norm_hw"], return_keep=True,
                                         chunk_bytes=budget)
        assert torch.equal(keep1, keepn)
        assert torch.equal(one.vertices.view(torch.int32), many.vertices.view(torch.int32))
        assert torch.equal(one.triangles, many.triangles) and torch.equal(one.vertex_colors, many.vertex_colors)
    assert 0 < int(keep1.sum()) < len(verts)


# ---------------------------------------------------------------- 6. command line
def test_cull_cli_on_the_device(tmp_path):
    from gaussmart_amd import _lib
    from gaussmart_amd.mesh import DeviceTriangleMesh, TriangleMesh
    from gaussmart_amd.mesh_cull import cull_mesh_by_masks, load_dtu_instance
    fx = R.hemisphere_fixture()
    sm = np.eye(4, dtype=np.float32)
    sm[:3, :3] *= 2.0
    sm[:3, 3] = (0.5, -0.25, 1.0)
    inv = np.linalg.inv(sm.astype(np.float64))
    wms = [(w.astype(np.float64) @ inv).astype(np.float32) for w in fx["world_mats"]]
    R.write_dtu_dir(tmp_path / "masks", "24", wms, [sm] * len(wms), fx["masks"])
    verts = fx["verts"]
    TriangleMesh(verts, R.neighbour_triangles(verts), np.random.default_rng(8).random((len(verts), 3))).write_ply(str(tmp_path / "in.ply"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussmart_amd.cull_cli", "--input_mesh", str(tmp_path / "in.ply"), "--scan_id", "24",
                        "--mask_dir", str(tmp_path / "masks"), "--output_dir", str(tmp_path / "out")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = TriangleMesh.read_ply(str(tmp_path / "out" / "culled_mesh.ply"))
    mesh = TriangleMesh.read_ply(str(tmp_path / "in.ply"))
    inst = load_dtu_instance(str(tmp_path / "masks" / "scan24"))
    want = cull_mesh_by_masks(mesh, inst.proj, inst.masks, 24, scale=inst.scale, offset=inst.offset, device=DEV).cpu()
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.triangles, want.triangles)
    assert np.array_equal(got.vertex_colors, want.vertex_colors)
    assert 0 < len(got.vertices) < len(mesh.vertices) and 0 < len(got.triangles) < len(mesh.triangles)
    assert f"num vertices culled {len(want.vertices)}, num triangles culled {len(want.triangles)}" in r.stdout
    d = DeviceTriangleMesh(torch.from_numpy(mesh.vertices), torch.from_numpy(mesh.triangles), torch.from_numpy(mesh.vertex_colors))
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        cull_mesh_by_masks(d, inst.proj, inst.masks)
