"""Mesh post-processing on the device: cluster labels against scipy, the cluster filter against the host post_process_mesh
(bit for bit), determinism, the hand-over from marching cubes, the depth AABB kernel against a float64 restatement, and the
command line with and without --host_post_process."""
import contextlib
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_post_fixtures as Fx
from test_gpu_mesh import _fib, _look_at_w2c, _sphere_cams, _sphere_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FIXTURES = {"mixed": Fx.mixed, "holed_grid": Fx.holed_grid, "snake": Fx.snake}


def _device_mesh(m):
    from gaussmart_amd.mesh import DeviceTriangleMesh
    return DeviceTriangleMesh(torch.from_numpy(m.vertices).to(DEV), torch.from_numpy(m.triangles).to(DEV),
                              torch.from_numpy(m.vertex_colors).to(DEV))


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ---------------------------------------------------------------- 1. labels
@pytest.mark.parametrize("name", ["mixed", "holed_grid", "snake"])
def test_cluster_labels_match_scipy(name):
    from gaussmart_amd.mesh import mesh_clusters_device
    m = FIXTURES[name]()
    labels, sizes = mesh_clusters_device(torch.from_numpy(m.triangles).to(DEV), len(m.vertices))
    ref_labels, ref_sizes = Fx.reference_labels(m.triangles, len(m.vertices))
    got_labels, got_sizes = labels.cpu().numpy(), sizes.cpu().numpy()
    assert got_labels.dtype == np.int32 and got_sizes.dtype == np.int32
    assert np.array_equal(got_labels, ref_labels)
    assert np.array_equal(got_sizes, ref_sizes)


def test_cluster_labels_single_triangle_and_large_indices():
    from gaussmart_amd.mesh import mesh_clusters_device
    labels, sizes = mesh_clusters_device(torch.tensor([[4, 2, 9]], dtype=torch.int32, device=DEV), 10)
    assert labels.tolist() == [0] and sizes.tolist() == [1]
    # vertex indices up to 2^31 - 2 (every bit of the two sort keys in use); triangles 1 and 3 share edge (top - 1, top)
    top = 2 ** 31 - 2
    tris = np.array([[0, 1, 2], [top, top - 1, 5], [7, 8, 9], [top - 1, top, top - 2]], dtype=np.int32)
    labels, sizes = mesh_clusters_device(torch.from_numpy(tris).to(DEV), 2 ** 31 - 1)
    assert labels.tolist() == [0, 1, 2, 1] and sizes.tolist() == [1, 2, 1, 2]


# ---------------------------------------------------------------- 2. filter
@pytest.mark.parametrize("name", ["mixed", "holed_grid", "snake"])
def test_filter_matches_host(name, capsys):
    from gaussmart_amd.mesh import DeviceTriangleMesh, post_process_mesh_device
    m = FIXTURES[name]()
    d = _device_mesh(m)
    for k in Fx.KEEP:
        want = Fx.host_filtered(name, k)
        capsys.readouterr()
        got = post_process_mesh_device(d, k)
        out = capsys.readouterr().out.splitlines()
        assert out == [f"post processing the mesh to have {k} clusterscluster_to_kep", f"num vertices raw {len(m.vertices)}",
                       f"num vertices post {len(want.vertices)}"]
        assert isinstance(got, DeviceTriangleMesh) and got.vertices.device == DEV
        Fx.assert_same_mesh(got.cpu(), want)
        expected = {"mixed": Fx.MIXED_EXPECTED, "holed_grid": Fx.HOLED_GRID_EXPECTED}.get(name, {})
        if k in expected:
            assert (len(got.vertices), len(got.triangles)) == expected[k]
    # the input mesh is left as it was
    Fx.assert_same_mesh(d.cpu(), m)


def test_filter_from_host_mesh_and_all_clusters_below_50():
    from gaussmart_amd.mesh import post_process_mesh_device
    m = Fx.mixed(False)
    got = _quiet(post_process_mesh_device, m, 1, device=DEV).cpu()
    want = Fx.host_filtered("mixed", 1, False)
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and got.vertex_colors.shape == (0, 3)
    Fx.assert_same_mesh(got, want)
    Fx.assert_same_mesh(_quiet(post_process_mesh_device, Fx.mixed(), 2, device=DEV).cpu(), Fx.host_filtered("mixed", 2))


# ---------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("name,k", [("snake", 1), ("holed_grid", 3)])
def test_labels_and_filter_are_bitwise_deterministic(name, k):
    from gaussmart_amd.mesh import mesh_clusters_device, post_process_mesh_device
    m = FIXTURES[name]()
    d = _device_mesh(m)
    runs = []
    for _ in range(5):
        labels, sizes = mesh_clusters_device(d.triangles, len(m.vertices))
        post = _quiet(post_process_mesh_device, d, k)
        runs.append((labels, sizes, post.vertices, post.triangles, post.vertex_colors))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------- 4. hand-over from marching cubes
def _two_sphere_volume():
    from gaussmart_amd.tsdf import TSDFVolume
    n = 40
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    c = (n - 1) / 2
    s1 = np.sqrt((x - 12.0) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 8.3      # the larger sphere: x in [3.7, 20.3]
    s2 = np.sqrt((x - 30.0) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 5.2      # the smaller one: x in [24.8, 35.2]
    f = (np.minimum(s1, s2) / 5).astype(np.float32)
    colour = np.random.default_rng(5).integers(0, 256, f.shape + (3,)).astype(np.float32)
    return TSDFVolume.from_dense(0.01, 0.05, f, np.ones_like(f), colour, device=DEV)


def test_handover_from_marching_cubes():
    from gaussmart_amd.mesh import DeviceTriangleMesh, TriangleMesh, post_process_mesh, post_process_mesh_device
    vol = _two_sphere_volume()
    dm = vol.extract_triangle_mesh(to_host=False)
    hm = vol.extract_triangle_mesh()
    assert isinstance(dm, DeviceTriangleMesh) and dm.vertices.device == DEV and isinstance(hm, TriangleMesh)
    Fx.assert_same_mesh(dm.cpu(), hm)
    Fx.assert_same_mesh(vol.extract_triangle_mesh(to_host=True), hm)
    assert repr(dm) == repr(hm)
    got = _quiet(post_process_mesh_device, dm, 1).cpu()
    want = _quiet(post_process_mesh, hm, 1)
    Fx.assert_same_mesh(got, want)
    # exactly the larger sphere: every vertex on its side of the gap (x = 22.5 voxels), and every such vertex / triangle kept
    mid = (22.5 + 0.5) * 0.01
    left = hm.vertices[:, 0] < mid
    assert 0 < left.sum() < len(left)
    assert (got.vertices[:, 0] < mid).all() and len(got.vertices) == int(left.sum())
    assert len(got.triangles) == int(left[hm.triangles[:, 0]].sum()) > len(hm.triangles) // 2
    e = np.unique(np.sort(np.concatenate([got.triangles[:, [0, 1]], got.triangles[:, [1, 2]], got.triangles[:, [2, 0]]]), 1),
                  axis=0)
    assert len(got.vertices) - len(e) + len(got.triangles) == 2


# ---------------------------------------------------------------- 6. depth AABB
TRUNC = 3.0


def _aabb_views():
    rng = np.random.default_rng(21)
    views = []
    for H, W in ((48, 64), (67, 129), (1, 1)):
        depth = (rng.random((H, W)) * 4).astype(np.float32)
        depth[rng.random((H, W)) < 0.3] = 0.0
        mask = rng.random((H, W)) < 0.6
        if H * W == 1:          # the single pixel is a valid one, so that the 1 x 1 launch has something to reduce
            depth[:], mask[:] = 1.75, True
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = q, rng.uniform(-5, 5, 3)
        c2w = c2w.astype(np.float32)
        intr = (float(W) * 0.75 + 2.0, float(W) * 0.75 + 2.0, (W - 1) / 2, (H - 1) / 2)     # exact in fp32
        views.append((depth, mask, intr, c2w))
    return views


def _aabb_ref64(depth, mask, intr, c2w):
    """float64 restatement: (lo, hi, S) of the valid pixels' world points; S = max|t| + 3 max ||pc||_inf."""
    fx, fy, cx, cy = intr
    ok = (depth > 0) & (depth <= np.float32(TRUNC)) & mask
    v, u = np.nonzero(ok)
    z = depth[v, u].astype(np.float64)
    pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    M = c2w.astype(np.float64)
    pw = pc @ M[:3, :3].T + M[:3, 3]
    return pw.min(0), pw.max(0), np.abs(M[:3, 3]).max() + 3 * np.abs(pc).max()


def _aabb_torch(depth, mask, intr, c2w):
    """The torch pass of GaussianExtractor.block_aabb on one view (fp32 on the device), for the printed comparison."""
    fx, fy, cx, cy = intr
    d = torch.from_numpy(np.where(mask, depth, np.float32(0))).to(DEV)
    H, W = d.shape
    v, u = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32),
                          indexing="ij")
    ok = (d > 0) & (d <= TRUNC)
    z = d[ok]
    pc = torch.stack([(u[ok] - cx) * z / fx, (v[ok] - cy) * z / fy, z], 1)
    M = torch.from_numpy(c2w).to(DEV)
    pw = pc @ M[:3, :3].T + M[:3, 3]
    return pw.min(0).values.cpu().numpy(), pw.max(0).values.cpu().numpy()


def _bounds_of(views):
    from gaussmart_amd.tsdf import DepthBounds
    b = DepthBounds(DEV)
    for depth, mask, intr, c2w in views:
        b.add(torch.from_numpy(depth), intr, c2w, TRUNC, mask=torch.from_numpy(mask))
    return b


def test_depth_aabb_matches_float64_restatement():
    views = _aabb_views()
    singles = []
    for depth, mask, intr, c2w in views:
        lo64, hi64, S = _aabb_ref64(depth, mask, intr, c2w)
        tol = 32 * 2.0 ** -24 * S
        lo, hi = _bounds_of([(depth, mask, intr, c2w)]).read()
        assert lo.dtype == np.float32 and hi.dtype == np.float32
        dist = max(np.abs(lo - lo64).max(), np.abs(hi - hi64).max())
        tlo, thi = _aabb_torch(depth, mask, intr, c2w)
        tdist = max(np.abs(tlo - lo64).max(), np.abs(thi - hi64).max())
        print(f"depth AABB {depth.shape[1]}x{depth.shape[0]}: kernel {dist:.3e}, torch pass {tdist:.3e}, bound {tol:.3e} (S {S:.3f})")
        assert dist <= tol, (dist, tol)
        singles.append((lo, hi))
    # accumulating the three views = min / max of the three single-view results, exactly
    lo, hi = _bounds_of(views).read()
    assert np.array_equal(lo, np.min([s[0] for s in singles], 0)) and np.array_equal(hi, np.max([s[1] for s in singles], 0))


def test_depth_aabb_invalid_view_and_truncation_edge():
    from gaussmart_amd.tsdf import DepthBounds
    depth, mask, intr, c2w = _aabb_views()[0]
    # no valid pixel: zero depth, depth beyond the truncation, a mask of zeros -- the words stay as initialised
    b = DepthBounds(DEV)
    init = b.words.clone()
    b.add(torch.zeros(48, 64), intr, c2w, TRUNC)
    b.add(torch.full((48, 64), 3.5), intr, c2w, TRUNC)
    b.add(torch.from_numpy(depth), intr, c2w, TRUNC, mask=torch.zeros(48, 64, dtype=torch.bool))
    assert torch.equal(b.words, init) and init.cpu().numpy().view(np.uint32).tolist() == [0xFFFFFFFF] * 3 + [0] * 3
    assert b.read() is None
    # ... and untouched by an invalid view after a valid one
    b = _bounds_of([(depth, mask, intr, c2w)])
    before = b.words.clone()
    b.add(torch.zeros(48, 64), intr, c2w, TRUNC)
    assert torch.equal(b.words, before)
    # d == depth_trunc counts, the next float above does not
    above = np.nextafter(np.float32(TRUNC), np.float32(10))
    edge = np.array([[TRUNC, above]], dtype=np.float32)
    only = np.array([[TRUNC, 0.0]], dtype=np.float32)
    intr2 = (4.0, 4.0, 0.5, 0.0)
    ones = np.ones((1, 2), bool)
    lo, hi = _bounds_of([(edge, ones, intr2, c2w)]).read()
    lo1, hi1 = _bounds_of([(only, ones, intr2, c2w)]).read()
    lo64, hi64, S = _aabb_ref64(only, ones, intr2, c2w)
    assert np.array_equal(lo, lo1) and np.array_equal(hi, hi1) and np.array_equal(lo, hi)
    assert np.abs(lo - lo64).max() <= 32 * 2.0 ** -24 * S
    assert _bounds_of([(np.array([[above, above]], dtype=np.float32), ones, intr2, c2w)]).read() is None


# ---------------------------------------------------------------- 7. the AABB pass does not change the mesh
def test_aabb_pass_does_not_change_the_mesh(tmp_path):
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.mesh import GaussianExtractor, camera_intrinsics
    from gaussmart_amd.params import PipelineParams
    from gaussmart_amd.tsdf import BLOCK, block_aabb_of_points
    vs, st, dt = 0.02, 0.08, 5
    ex = GaussianExtractor(_sphere_model(6000), render, PipelineParams(depth_ratio=1.0), bg_color=[0, 0, 0])
    ex.reconstruction(_sphere_cams(12, 128, 128))
    dev_aabb = ex.block_aabb_device(vs, st, dt)
    torch_aabb = ex.block_aabb(vs, st, dt)
    print(f"block AABB device {dev_aabb}, torch {torch_aabb}")
    # float64 extents of the back-projected valid depth
    lo64, hi64 = np.full(3, np.inf), np.full(3, -np.inf)
    for i, cam in enumerate(ex.viewpoint_stack):
        d = ex._masked_depth(i, True)[0].cpu().numpy().astype(np.float64)
        fx, fy, cx, cy = camera_intrinsics(cam)
        v, u = np.nonzero((d > 0) & (d <= dt))
        z = d[v, u]
        pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        c2w = np.linalg.inv(cam.world_view_transform.T.cpu().numpy().astype(np.float64))
        pw = pc @ c2w[:3, :3].T + c2w[:3, 3]
        lo64, hi64 = np.minimum(lo64, pw.min(0)), np.maximum(hi64, pw.max(0))
    bl = BLOCK * vs
    lo, hi = np.array(dev_aabb[0]), np.array(dev_aabb[1])
    assert (lo * bl <= lo64 - st).all() and (hi * bl >= hi64 + st).all()
    rlo, rhi = (np.array(a) for a in block_aabb_of_points(lo64, hi64, vs, st))
    assert (lo >= rlo - 1).all() and (hi <= rhi + 1).all()
    files = {}
    for aabb in ("device", "torch"):
        mesh = _quiet(ex.extract_mesh_bounded, voxel_size=vs, sdf_trunc=st, depth_trunc=dt, aabb=aabb)
        mesh.write_ply(str(tmp_path / f"{aabb}.ply"))
        files[aabb] = (tmp_path / f"{aabb}.ply").read_bytes()
        assert len(mesh.triangles) > 1000
    assert files["device"] == files["torch"]
    # the device mesh of the same extraction writes the same bytes
    dm = _quiet(ex.extract_mesh_bounded, voxel_size=vs, sdf_trunc=st, depth_trunc=dt, to_host=False)
    dm.write_ply(str(tmp_path / "dm.ply"))
    assert (tmp_path / "dm.ply").read_bytes() == files["device"]


def test_block_aabb_device_without_valid_depth():
    from gaussmart_amd.mesh import GaussianExtractor
    ex = GaussianExtractor.__new__(GaussianExtractor)
    cams = _sphere_cams(2, 32, 32)
    ex.viewpoint_stack, ex.depthmaps = cams, [torch.zeros(1, 32, 32, device=DEV) for _ in cams]
    assert ex.block_aabb_device(0.02, 0.08, 5) == ([0, 0, 0], [0, 0, 0]) == ex.block_aabb(0.02, 0.08, 5)


# ---------------------------------------------------------------- 8. command line
def test_render_cli_device_and_host_post_process_write_the_same_files(tmp_path):
    from PIL import Image
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.scene_io import Scene
    src, model = tmp_path / "src", tmp_path / "model"
    (src / "train").mkdir(parents=True)
    W = H = 96
    frames = []
    for i, d in enumerate(_fib(10)):
        c2w = np.linalg.inv(_look_at_w2c(3.0 * d, [0, 0, 0]))
        c2w[:3, 1:3] *= -1                         # COLMAP axes -> Blender axes
        img = np.zeros((H, W, 4), np.uint8)
        img[..., :3], img[..., 3] = 128, 255
        Image.fromarray(img, "RGBA").save(src / "train" / f"r_{i}.png")
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": c2w.tolist()})
    for split in ("train", "test"):
        with open(src / f"transforms_{split}.json", "w") as f:
            json.dump({"camera_angle_x": math.radians(60), "frames": frames if split == "train" else frames[:2]}, f)
    scene = Scene(str(src), GaussianModel(3, device=DEV), model_path=str(model), data_device=DEV, shuffle=False)
    scene.gaussians = _sphere_model(6000)
    scene.save(7)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = model / "train" / "ours_7"
    written = {}
    for flags in ((), ("--host_post_process",)):
        r = subprocess.run([sys.executable, "-m", "gaussmart_amd.render_cli", "-s", str(src), "-m", str(model), "--depth_ratio",
                            "1", "--num_cluster", "1", "--voxel_size", "0.03", "--skip_train", "--skip_test", *flags],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "num vertices post" in r.stdout
        written[flags] = {n: (out / n).read_bytes() for n in ("fuse.ply", "fuse_post.ply")}
        for n in written[flags]:
            os.remove(out / n)
    a, b = written[()], written[("--host_post_process",)]
    assert len(a["fuse.ply"]) > 1000 and len(a["fuse_post.ply"]) > 1000
    assert a["fuse.ply"] == b["fuse.ply"] and a["fuse_post.ply"] == b["fuse_post.ply"]
