"""Mesh culling by visibility on the device: the depth images against the float64 restatement under the interval test (every
pixel), single triangles where float64 is unambiguous, bit-identity across runs, view chunks and triangle orders, the vote
against vote64 on the same device images, VIS_COMPACT against numpy bit for bit, the hand-over from the cluster filter, the
command line and the error paths (tests/mesh_vis_ref.py)."""
import contextlib
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_vis_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = {"1x1": (1, 1, 5.0), "33x17": (17, 33, 20.0), "96x64": (64, 96, 60.0)}       # H, W, focal length
IDENTITY = np.eye(4)[None, :3].astype(np.float32)                                     # a camera at the origin looking along +z


def _device_mesh(verts, tris, cols=None):
    from gaussmart_amd.mesh import DeviceTriangleMesh
    return DeviceTriangleMesh(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV),
                              torch.from_numpy(np.ascontiguousarray(tris, np.int32).reshape(-1, 3)).to(DEV),
                              None if cols is None else torch.from_numpy(cols).to(DEV))


def _render(verts, tris, w2c, H, W, intr, **kw):
    from gaussmart_amd.mesh_visibility import render_mesh_depth
    out = render_mesh_depth(_device_mesh(verts, tris), w2c, H, W, *intr, **kw)
    assert out.dtype == torch.float32 and out.shape == (len(w2c), H, W) and out.device == DEV
    return out


def _check_interval(got, verts, tris, w2c, H, W, intr, key, near=R.NEAR, far=R.FAR):
    """Every pixel of every view under the interval test; returns the number of pixels whose five samples disagree."""
    mixed_total = 0
    for i in range(len(w2c)):
        five = R.cached(("five",) + key + (i,), lambda: R.five_rasters(verts, tris, w2c[i], H, W, intr, near, far))
        bad, mixed = R.depth_interval_errors(got[i], five)
        assert not bad.any(), (key, i, int(bad.sum()), np.argwhere(bad)[:5].tolist())
        mixed_total += int(mixed.sum())
    return mixed_total


# ---------------------------------------------------------------- 1. depth images
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 2392])
def test_depth_interval_two_spheres(F, size, n):
    sc = R.two_sphere_scene()
    H, W, f = SIZES[size]
    intr = R.intrinsics(H, W, f)
    # the subsets start at triangle 6: the first of the near sphere that covers a pixel centre of every 96 x 64 view
    tris, w2c = (sc["tris"] if F == 2392 else sc["tris"][6:6 + F]), sc["w2c"][:n]
    got = _render(sc["verts"], tris, w2c, H, W, intr).cpu().numpy()
    mixed = _check_interval(got, sc["verts"], tris, w2c, H, W, intr, ("two", F, size))
    if size == "96x64" or F == 2392:
        assert (F == 0) == (not got.any()) and all(g.any() for g in got[:, None] if F)
    print(f"two spheres F={F} {size} n={n}: {int((got > 0).sum())} of {got.size} pixels hit, {mixed} with disagreeing samples")
    assert (got >= 0).all() and (F > 0 or not got.any())
    if F == 2392 and size == "96x64":
        assert 0.1 < (got > 0).mean() < 0.6


def test_depth_interval_subpixel_triangles():
    sc = R.subpixel_scene()
    H, W, f = SIZES["96x64"]
    intr = R.intrinsics(H, W, f)
    w2c = sc["w2c"][:1]
    got = _render(sc["verts"], sc["tris"], w2c, H, W, intr).cpu().numpy()
    _check_interval(got, sc["verts"], sc["tris"], w2c, H, W, intr, ("sub",))
    d, tri = R.raster64(sc["verts"], sc["tris"], w2c[0], H, W, intr)
    share = len(np.unique(tri[tri >= 0])) / len(sc["tris"])
    print(f"sub-pixel scene: {int((got > 0).sum())} pixels hit; {share:.2%} of the triangles are nearest at some pixel centre")
    assert share < 0.05 and (got > 0).sum() > 1000


def _large_pairs(verts, tris, w2c, H, W, intr):
    """The number of (triangle, view) pairs whose pixel box (VIS_COVER's guard, in float64) is wider or higher than 8."""
    fx, fy, cx, cy = intr
    total = 0
    for m in w2c:
        q = R.camera_space(verts, m)[tris]
        u, v = fx * q[:, :, 0] / q[:, :, 2] + cx, fy * q[:, :, 1] / q[:, :, 2] + cy
        x0, x1 = np.clip(np.ceil(u.min(1) - 1.5), 0, W), np.clip(np.floor(u.max(1) + 0.5), -1, W - 1)
        y0, y1 = np.clip(np.ceil(v.min(1) - 1.5), 0, H), np.clip(np.floor(v.max(1) + 0.5), -1, H - 1)
        ok = (q[:, :, 2] >= R.NEAR).all(1) & (x0 <= x1) & (y0 <= y1)
        total += int((ok & ((x1 - x0 >= 8) | (y1 - y0 >= 8))).sum())
    return total


def test_depth_interval_many_large_pairs():
    """The large path's fixed grid of 2,048 workgroups takes a second trip over its work list: two coarse spheres (280 triangles
    of some 6 x 9 pixels) in 16 views give about 3,000 large pairs; every pixel of every view under the interval test."""
    v, t = R.join(R.uv_sphere(10, 8, 0.5, (-0.25, 0.05, 0.45)), R.uv_sphere(10, 8, 0.7, (0.3, -0.1, -0.4)))
    w2c = R.w2c32(R.ring_cameras(16, seed=11))
    H, W, f = SIZES["96x64"]
    intr = R.intrinsics(H, W, f)
    n_large = _large_pairs(v, t, w2c, H, W, intr)
    assert n_large > 2048 + 512                              # well beyond one trip, whatever the last bit of a box says
    got = _render(v, t, w2c, H, W, intr).cpu().numpy()
    mixed = _check_interval(got, v, t, w2c, H, W, intr, ("coarse",))
    print(f"coarse spheres: {n_large} large pairs of {len(t) * len(w2c)}, {int((got > 0).sum())} of {got.size} pixels hit, "
          f"{mixed} with disagreeing samples")
    assert all(0.1 < (g > 0).mean() < 0.6 for g in got)


def _single(verts, tris, H=30, W=40, intr=(10.0, 10.0, 20.0, 15.0), near=R.NEAR, far=R.FAR, exact=True):
    """One view from the origin along +z, held to the interval test; exact=True: no pixel's five samples disagree, so the hit
    mask must be float64's exactly."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    got = _render(verts, tris, IDENTITY, H, W, intr, near=near, far=far).cpu().numpy()
    five = R.five_rasters(verts, tris, IDENTITY[0], H, W, intr, near, far)
    bad, mixed = R.depth_interval_errors(got[0], five)
    assert not bad.any(), np.argwhere(bad)[:5].tolist()
    if exact:
        assert not mixed.any() and np.array_equal(got[0] > 0, five[0] > 0)
    return got[0], five[0]


def test_single_triangle_cases():
    at = lambda u, v, z, k=(10.0, 10.0, 20.0, 15.0): [(u - k[2]) * z / k[0], (v - k[3]) * z / k[1], z]      # the point that projects to (u, v)
    # covers the whole image: the large path; the plane z = 2 gives exactly 2.0
    got, _ = _single([[-100, -100, 2], [100, -100, 2], [0, 100, 2]], [0, 1, 2])
    assert (got == 2.0).all()
    # a pixel box of 8 x 8 (looped over by its thread) and of 9 x 8 (through the work list): u in [10.25, 15.75] / [10.25, 16.75]
    for umax, width in ((15.75, 8), (16.75, 9)):
        got, want = _single([at(10.25, 5.25, 2), at(umax, 5.25, 2), at(10.25, 10.95, 2)], [0, 1, 2])
        assert (got[got > 0] == 2.0).all() and 10 < (got > 0).sum() < 40
        assert int(np.ceil(10.25 - 1.5)) == 9 and int(np.floor(umax + 0.5)) - 9 + 1 == width
    # crosses the camera plane (one vertex at z < 0): only the part with z >= near shows
    got, want = _single([[-1, -1, 3], [1, -1, 3], [0, 4, -1]], [0, 1, 2], exact=False)
    assert (got > 0).sum() > 100 and (got == 0).sum() > 100 and got[got > 0].min() >= R.NEAR and got[got > 0].max() <= 3.0 * (1 + R.TAU)
    # a near plane that cuts the triangle
    got, _ = _single([[-1, -1, 3], [1, -1, 3], [0, 4, -1]], [0, 1, 2], near=1.5, exact=False)
    assert (got > 0).sum() > 50 and got[got > 0].min() >= 1.5
    # entirely behind the camera; beyond far; nearer than near
    for z in (-2.0, 25.0, 0.005):
        got, _ = _single([[-z, -z, z], [z, -z, z], [0, z, z]], [0, 1, 2])
        assert not got.any()
    # zero area: collinear vertices, and a triangle that names a vertex twice
    got, _ = _single([[-1, 0, 2], [0, 0, 2], [1, 0, 2]], [[0, 1, 2], [0, 0, 2], [1, 1, 1]])
    assert not got.any()
    # edge-on: the triangle lies in the plane x = 0 through the camera, column 20 looks along it (cx = 20.5): n.d = 0
    got, _ = _single([[0, -1, 2], [0, 1, 2], [0, 0, 4]], [0, 1, 2], intr=(10.0, 10.0, 20.5, 15.0))
    assert not got.any()
    # back-facing: drawn, and the same bits as front-facing
    tri = [at(8.3, 4.2, 2), at(30.1, 6.7, 3), at(17.6, 25.4, 2.5)]
    front, _ = _single(tri, [0, 1, 2])
    back, _ = _single(tri, [0, 2, 1])
    assert (front > 0).sum() > 100 and front.tobytes() == back.tobytes()
    # a NaN and an infinite vertex: their triangles draw nothing, the others are unaffected
    verts = tri + [[np.nan, 0, 2], [0, np.inf, 2], at(12, 20, 1.5), at(25, 22, 1.5)]
    both, _ = _single(verts, [[0, 1, 2], [3, 5, 6], [5, 4, 6], [0, 3, 4]])
    assert both.tobytes() == front.tobytes()
    with_third, _ = _single(verts, [[0, 1, 2], [3, 5, 6], [5, 4, 6], [0, 5, 6]])
    assert with_third.tobytes() != front.tobytes()
    # an index outside the vertex array draws nothing
    outside = _render(np.asarray(tri, np.float32), np.array([[0, 1, 2], [0, 1, 3], [-1, 1, 2]], np.int32), IDENTITY, 30, 40,
                      (10.0, 10.0, 20.0, 15.0)).cpu().numpy()[0]
    assert outside.tobytes() == front.tobytes()


def test_depth_is_bit_identical_across_runs_chunks_and_triangle_orders():
    sc = R.two_sphere_scene()
    H, W, f = SIZES["96x64"]
    intr = R.intrinsics(H, W, f)
    # a triangle that fills the image from behind, so that the large path takes part
    verts = np.concatenate([sc["verts"], [[-40, -40, -3], [40, -40, -3], [0, 60, -3]]]).astype(np.float32)
    tris = np.concatenate([sc["tris"], [[len(sc["verts"]), len(sc["verts"]) + 1, len(sc["verts"]) + 2]]]).astype(np.int32)
    one = _render(verts, tris, sc["w2c"], H, W, intr)
    assert (one > 0).all() and 0.1 < float((one < 3.0).float().mean()) < 0.6
    again = _render(verts, tris, sc["w2c"], H, W, intr)
    per_view = _render(verts, tris, sc["w2c"], H, W, intr, chunk_bytes=1)
    reverse = _render(verts, tris[::-1].copy(), sc["w2c"], H, W, intr)
    for other in (again, per_view, reverse):
        assert torch.equal(one.view(torch.int32), other.view(torch.int32))
    for i in range(3):                                                           # a view alone gives its image of the batch
        assert torch.equal(_render(verts, tris, sc["w2c"][i:i + 1], H, W, intr)[0].view(torch.int32), one[i].view(torch.int32))


# ---------------------------------------------------------------- 2. vote
def _vote_fixture():
    """The device depth images of the vote scene and vote64's pairs on those same images."""
    def make():
        vs = R.vote_scene()
        depths = _render(vs["verts"], vs["tris"], vs["w2c"], vs["H"], vs["W"], vs["intr"])
        seen, stable = R.vote_pairs(vs["verts"], vs["w2c"], depths.cpu().numpy(), vs["intr"])
        return depths, seen, stable
    return R.cached("gpu_vote", make)


@pytest.mark.parametrize("n", [0, 1, 3, 8])
@pytest.mark.parametrize("V", [0, 1, 63, 64, 65, 4000])
def test_vote_counts_lie_within_the_float64_bounds(V, n):
    from gaussmart_amd.mesh_visibility import visibility_counts
    vs = R.vote_scene()
    depths, seen, stable = _vote_fixture()
    # the last V vertices: for small V these are around the inner sphere's south pole and the subset is all "hidden"; the
    # first ones are the outer sphere's north pole, seen by every view: take half of each
    idx = np.concatenate([np.arange((V + 1) // 2), np.arange(2000, 2000 + V // 2)]) if V < 4000 else np.arange(4000)
    verts = torch.from_numpy(np.ascontiguousarray(vs["verts"][idx])).to(DEV)
    s = (seen & stable)[:n][:, idx].sum(0)
    u = (~stable)[:n][:, idx].sum(0)
    truth = seen[:n][:, idx].sum(0)
    for mv in (1, 3, 9):
        cnt = visibility_counts(verts, vs["w2c"][:n], depths[:n], *vs["intr"], eps=R.EPS, min_views=mv)
        assert cnt.dtype == torch.int32 and cnt.shape == (len(idx),) and cnt.device == DEV
        cnt = cnt.cpu().numpy()
        assert ((cnt >= np.minimum(s, mv)) & (cnt <= np.minimum(s + u, mv))).all(), (V, n, mv)
        decided = (s >= mv) | (s + u < mv)
        assert np.array_equal((cnt >= mv)[decided], (truth >= mv)[decided])
        if V == 4000 and n == 8:
            print(f"vote min_views {mv}: kept {int((cnt >= mv).sum())} of 4000, unstable pairs {int(u.sum())}, "
                  f"undecided vertices {int((~decided).sum())}")
            assert decided.mean() >= 0.99
            assert (0.05 < (cnt >= mv).mean() < 0.95) if mv <= 3 else not (cnt >= mv).any()       # 9 > n: nobody is kept
    # chunks of views continue the same count
    if n == 8 and V:
        whole = visibility_counts(verts, vs["w2c"], depths, *vs["intr"], min_views=3)
        part = visibility_counts(verts, vs["w2c"][:5], depths[:5], *vs["intr"], min_views=3)
        part = visibility_counts(verts, vs["w2c"][5:], depths[5:], *vs["intr"], min_views=3, counts=part)
        assert torch.equal(whole, part)


def test_vote_special_vertices_and_empty_images():
    from gaussmart_amd.mesh_visibility import visibility_counts
    vs = R.vote_scene()
    H, W, intr = vs["H"], vs["W"], vs["intr"]
    verts = np.array([[0, 0, 0], [50, 0, 0], [0, 0, 9], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    zeros = torch.zeros((8, H, W), device=DEV)
    cnt = visibility_counts(torch.from_numpy(verts).to(DEV), vs["w2c"], zeros, *intr, min_views=20)
    # all-zero depth images: every in-frustum vertex is seen; outside the frame, behind the camera, NaN and inf are not
    assert cnt.tolist() == [8, 0, 0, 0, 0]
    assert visibility_counts(torch.from_numpy(verts).to(DEV), vs["w2c"], zeros, *intr, min_views=5).tolist() == [5, 0, 0, 0, 0]
    # more than 64 views: several launches continue one count
    many = visibility_counts(torch.from_numpy(verts).to(DEV), np.tile(vs["w2c"], (9, 1, 1)), zeros.repeat(9, 1, 1), *intr, min_views=70)
    assert many.tolist() == [70, 0, 0, 0, 0]


# ---------------------------------------------------------------- 3. end to end
def _gl(c2w):
    gl = np.array(c2w)
    gl[:, :3, 1:3] *= -1
    return gl


def test_cull_equals_numpy_compaction_of_the_device_keep_mask():
    from gaussmart_amd import _lib
    from gaussmart_amd.mesh import TriangleMesh
    from gaussmart_amd.mesh_visibility import cull_mesh_by_visibility, cull_mesh_by_visibility_host
    vs = R.vote_scene()
    H, W, intr = vs["H"], vs["W"], vs["intr"]
    c2w = _gl(R.ring_cameras(8, seed=7))
    cols = np.random.default_rng(2).random(vs["verts"].shape).astype(np.float32)
    tris = np.concatenate([vs["tris"], [[0, 0, 1], [2, 2, 2]]]).astype(np.int32)             # degenerate triangles stay
    mesh = _device_mesh(vs["verts"], tris, cols)
    out, keep = cull_mesh_by_visibility(mesh, c2w, H, W, *intr, min_views=3, return_keep=True)
    keep = keep.cpu().numpy().astype(bool)
    v, c, t = R.compact_ref(vs["verts"], cols, tris, keep)
    got = out.cpu()
    assert got.vertices.tobytes() == v.tobytes() and got.vertex_colors.tobytes() == c.tobytes() and np.array_equal(got.triangles, t)
    assert got.triangles.dtype == np.int32 and 0 < len(t) < len(tris) and len(v) < keep.sum() + 1
    assert np.array_equal(np.unique(t), np.arange(len(v)))                                   # no unreferenced vertex
    assert (t == [0, 0, 1]).all(1).any()                                                     # the north pole is seen by all
    assert (np.linalg.norm(v, axis=1) > 0.9).all()                                           # nothing of the inner sphere
    # the input is untouched; a host mesh with device=, one view per chunk, and a second run give the same bytes
    assert mesh.vertices.cpu().numpy().tobytes() == vs["verts"].tobytes()
    for kw in (dict(), dict(chunk_bytes=1)):
        other = cull_mesh_by_visibility(TriangleMesh(vs["verts"], tris, cols), c2w, H, W, *intr, min_views=3, device=DEV, **kw)
        assert torch.equal(other.vertices.view(torch.int32), out.vertices.view(torch.int32))
        assert torch.equal(other.triangles, out.triangles) and torch.equal(other.vertex_colors, out.vertex_colors)
    # the host path decides the same wherever float64 decides
    hkeep = cull_mesh_by_visibility_host(TriangleMesh(vs["verts"], tris, cols), c2w, H, W, *intr, min_views=3, return_keep=True)[1]
    print(f"cull: kept {int(keep.sum())} of {len(keep)} vertices, {len(t)} of {len(tris)} triangles; device vs host keep "
          f"disagreements {int((keep != hkeep).sum())}")
    assert (keep != hkeep).sum() <= 0.01 * len(keep)
    # no view, no triangle, min_views above the number of views: an empty mesh each time
    for m, poses, mv in ((mesh, c2w[:0], 3), (_device_mesh(vs["verts"], tris[:0], cols), c2w, 1), (mesh, c2w, 9)):
        e = cull_mesh_by_visibility(m, poses, H, W, *intr, min_views=mv)
        assert e.vertices.shape == (0, 3) and e.triangles.shape == (0, 3) and e.vertex_colors.shape == (0, 3)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        from gaussmart_amd.mesh import DeviceTriangleMesh
        cull_mesh_by_visibility(DeviceTriangleMesh(torch.from_numpy(vs["verts"]), torch.from_numpy(tris)), c2w, H, W, *intr)


def test_handover_from_the_cluster_filter():
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.mesh import DeviceTriangleMesh, GaussianExtractor, camera_intrinsics, post_process_mesh_device
    from gaussmart_amd.mesh_visibility import cull_mesh_by_visibility
    from gaussmart_amd.params import PipelineParams
    from test_gpu_mesh import _sphere_cams, _sphere_model
    g = _sphere_model(6000)
    cams = _sphere_cams(12, 128, 128)
    ex = GaussianExtractor(g, render, PipelineParams(depth_ratio=1.0), bg_color=[0, 0, 0])
    ex.reconstruction(cams)
    with contextlib.redirect_stdout(io.StringIO()):
        dm = ex.extract_mesh_bounded(voxel_size=0.02, sdf_trunc=0.08, depth_trunc=5, to_host=False)
        post = post_process_mesh_device(dm, 1)
    assert isinstance(post, DeviceTriangleMesh) and len(post.triangles) > 1000
    # the three cameras nearest to +z: what at least two of them see is the upper part of the sphere.  eps = 0.03: at 128 pixels
    # the half pixel between VIS_RAY and VIS_SAMPLE moves the sample by 0.009 scene units, which on a slanted surface is more
    # depth than the reference's 0.005 (chosen for 1920 x 1080) allows
    top = sorted(range(len(cams)), key=lambda i: -float(cams[i].camera_center[2]))[:3]
    c2w = np.stack([np.linalg.inv(cams[i].world_view_transform.T.cpu().numpy().astype(np.float64)) for i in top])
    fx, fy, cx, cy = camera_intrinsics(cams[top[0]])
    got, keep = cull_mesh_by_visibility(post, c2w, 128, 128, fx, fy, cx, cy, eps=0.03, min_views=2, opengl=False, return_keep=True)
    again = cull_mesh_by_visibility(post, c2w, 128, 128, fx, fy, cx, cy, eps=0.03, min_views=2, opengl=False)
    assert isinstance(got, DeviceTriangleMesh) and got.vertices.device == post.vertices.device
    assert torch.equal(got.vertices.view(torch.int32), again.vertices.view(torch.int32)) and torch.equal(got.triangles, again.triangles)
    hp = post.cpu()
    v, c, t = R.compact_ref(hp.vertices, hp.vertex_colors, hp.triangles, keep.cpu().numpy().astype(bool))
    gc = got.cpu()
    assert gc.vertices.tobytes() == v.tobytes() and gc.vertex_colors.tobytes() == c.tobytes() and np.array_equal(gc.triangles, t)
    print(f"hand-over: {len(hp.vertices)} -> {len(v)} vertices, {len(hp.triangles)} -> {len(t)} triangles")
    assert 0.1 * len(hp.vertices) < len(v) < 0.9 * len(hp.vertices)
    assert float(got.vertices[:, 2].min()) > -0.6 and float(got.vertices[:, 2].max()) > 0.95


def test_tnt_cull_cli_on_the_device(tmp_path):
    from gaussmart_amd.mesh import TriangleMesh
    from gaussmart_amd.mesh_visibility import cull_mesh_by_visibility
    vs = R.vote_scene()
    H, W, (fx, fy, cx, cy) = vs["H"], vs["W"], vs["intr"]
    c2w = _gl(R.ring_cameras(8, seed=7))
    TriangleMesh(vs["verts"], vs["tris"], np.random.default_rng(8).random(vs["verts"].shape)).write_ply(str(tmp_path / "in.ply"))
    np.save(tmp_path / "traj.npy", c2w[:, :3])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussmart_amd.tnt_cull_cli", "--traj-path", str(tmp_path / "traj.npy"), "--ply-path",
                        str(tmp_path / "in.ply"), "--min-views", "3", "--intrinsics", repr(fx), repr(fy), repr(cx), repr(cy),
                        "--size", str(W), str(H)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = TriangleMesh.read_ply(str(tmp_path / "in_cull.ply"))
    mesh = TriangleMesh.read_ply(str(tmp_path / "in.ply"))
    want = cull_mesh_by_visibility(mesh, c2w, H, W, fx, fy, cx, cy, min_views=3, device=DEV).cpu()
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.triangles, want.triangles)
    assert np.array_equal(got.vertex_colors, want.vertex_colors)
    assert 0 < len(got.vertices) < len(mesh.vertices) and 0 < len(got.triangles) < len(mesh.triangles)
    assert f"num vertices culled {len(want.vertices)}, num triangles culled {len(want.triangles)}" in r.stdout


# ---------------------------------------------------------------- 4. error paths
def test_errors_come_before_any_launch():
    from gaussmart_amd import _lib
    from gaussmart_amd.mesh_visibility import render_mesh_depth, visibility_counts
    L = _lib.lib()
    sc = R.two_sphere_scene()
    mesh = _device_mesh(sc["verts"], sc["tris"])
    F, V = len(sc["tris"]), len(sc["verts"])
    out = torch.full((1, 8, 8), 7.0, device=DEV)
    ws = torch.zeros(L.gsr_mesh_depth_workspace_bytes(F, 1), dtype=torch.uint8, device=DEV)
    m = np.ascontiguousarray(sc["w2c"][:1]).reshape(-1)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    def call(H=8, W=8, near=0.01, far=20.0, F=F, ws_bytes=ws.numel()):
        return L.gsr_mesh_depth_render(C.c_void_p(mesh.vertices.data_ptr()), C.c_void_p(mesh.triangles.data_ptr()), F, V,
                                       m.ctypes.data_as(C.c_void_p), 1, H, W, 10.0, 10.0, 4.0, 4.0, near, far,
                                       C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, stream)
    for kw in (dict(H=0), dict(W=-1), dict(near=20.0), dict(near=21.0), dict(near=0.0), dict(F=-1), dict(ws_bytes=16)):
        assert call(**kw) == -1, kw                                              # GSR_E_INVALID
    torch.cuda.synchronize()
    assert (out == 7.0).all() and not ws.any()                                   # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == 7.0).any()
    with pytest.raises(ValueError, match="near"):
        render_mesh_depth(mesh, sc["w2c"], 8, 8, 10, 10, 4, 4, near=1.0, far=0.5)
    with pytest.raises(ValueError, match="matrices"):
        visibility_counts(mesh.vertices, sc["w2c"][:2], torch.zeros((3, 8, 8), device=DEV), 10, 10, 4, 4)
    with pytest.raises(ValueError, match="depths"):
        visibility_counts(mesh.vertices, sc["w2c"], torch.zeros((3, 8, 8), dtype=torch.float64, device=DEV), 10, 10, 4, 4)
