"""Developer probe: time each part of the bounded mesh export (gaussmart_amd.mesh) on a unit-sphere surfel scene at the DTU
flags (--voxel_size 0.004 --sdf_trunc 0.016 --depth_trunc 3.0, depth_ratio 1): rendering the views, the block AABB,
TSDF touch + integrate, marching cubes and post-processing.  The AABB pass, the extraction and the post-processing are timed
on the host path (torch AABB, mesh copied to the host, numpy + scipy filter) and on the device path (gsr_depth_aabb, mesh kept
on the device, gsr_mesh_filter_*) in the same run; both must give equal arrays.  Prints one JSON line.

With --cull the post-processed mesh is then culled against one synthetic ellipse mask per view (gaussmart_amd.mesh_cull: the
DTU evaluation's cull_scan, disk radius 24) on the device and on the host path in the same run; the two keep masks must be
equal outside the unstable set (a vertex whose vote changes within DELTA pixels, scaled to the frame width, of its float64 position:
tests/mesh_cull_ref.py); a second JSON
line with the times goes to --cull_out (default profiles/r07_mesh_cull_bench.json).  cull_device_ms starts from masks on
the device, cull_host_ms from masks in host memory; the comparison the script asserts adds mask_upload_ms to the device side.

With --vis the post-processed mesh is culled by visibility from the same cameras (gaussmart_amd.mesh_visibility: the
Tanks-and-Temples step): wall times of the depth rendering, the vote and the compaction, with the bytes the small-box rasterizer
has to move next to them; the JSON line goes to --vis_out (default profiles/r08_mesh_vis_bench.json).  There is no host side to
this comparison: the numpy path is far too slow at this size.

    python scripts/mesh_bench.py [--surfels 300000] [--views 49] [--width 1600] [--height 1200]
    python scripts/mesh_bench.py --cull
    python scripts/mesh_bench.py --vis
    python scripts/mesh_bench.py --eval
    python scripts/mesh_bench.py --tnt
    python scripts/mesh_bench.py --unbounded [--mesh_res 1024] [--mesh_crop 512]

With --unbounded nothing of the above runs: a ground plane z = -1 is added under the sphere so that the field leaves the unit
ball, and the unbounded mesh export (gaussmart_amd.mesh_unbounded) is timed per stage on the device (pass 1 with the
allocation, pass 2, marching cubes, vertex finishing, colouring) at --mesh_res.  The same field is then evaluated on the same
GPU in the shape the reference computes it (utils/mesh_utils.py:197-248, utils/mcube_utils.py:42-68): per crop a
torch.linspace lattice, 256^3 chunks, one pass per view over state in memory, torch.nn.functional.grid_sample -- with the maps
already on the device, which favours it.  The reference's marching cubes run on the host (scikit-image) and are not part of
that figure.  One JSON line goes to --unbounded_out (default profiles/unbounded_mesh_bench.json).

With --eval the post-processed mesh is scored like a DTU scan (gaussmart_amd.mesh_eval: sampling, shuffle, greedy down-sampling,
ObsMask and plane filters, the two nearest-neighbour searches, the means) against a ground-truth cloud sampled from the analytic
sphere, on the device and on the host path (numpy + cKDTree) in the same run; masks, indices and distances must be equal and the
means within the summation bound.  Wall times per stage of both paths go to --eval_out (default
profiles/r09_mesh_eval_bench.json).

With --tnt the post-processed mesh, moved by the inverse of a known similarity, is scored like a Tanks-and-Temples scene
(gaussmart_amd.tnt_eval: the mesh as a cloud, crop, voxel grid, three ICP refinements, histograms and F-score) against the
analytic sphere cloud, on the device and on the host path in the same run; ICP iteration counts, correspondence counts and
fitness, precision, recall and the histograms must be equal.  Wall times per stage of both paths go to --tnt_out (default
profiles/r10_tnt_eval_bench.json).
"""
import argparse
import contextlib
import io
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))          # mesh_cull_ref: the stability rule of the culling comparison


def fib(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--surfels", type=int, default=300_000)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--voxel_size", type=float, default=0.004)
    ap.add_argument("--sdf_trunc", type=float, default=0.016)
    ap.add_argument("--depth_trunc", type=float, default=3.0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cull", action="store_true", help="also time the mask culling of the post-processed mesh")
    ap.add_argument("--cull_radius", type=int, default=24)
    ap.add_argument("--cull_out", type=str, default=os.path.join(ROOT, "profiles", "r07_mesh_cull_bench.json"),
                    help="the culling JSON line is written to this file as well")
    ap.add_argument("--vis", action="store_true", help="also time the culling by visibility of the post-processed mesh")
    ap.add_argument("--vis_min_views", type=int, default=12,
                    help="views that must see a vertex (a camera at distance 2.5 sees 30 %% of the unit sphere: about 14 of 49)")
    ap.add_argument("--vis_out", type=str, default=os.path.join(ROOT, "profiles", "r08_mesh_vis_bench.json"))
    ap.add_argument("--eval", action="store_true", help="also score the post-processed mesh against an analytic ground truth")
    ap.add_argument("--eval_density", type=float, default=0.002, help="downsample_density in scene units (half the voxel size)")
    ap.add_argument("--eval_gt_points", type=int, default=1_000_000)
    ap.add_argument("--eval_out", type=str, default=os.path.join(ROOT, "profiles", "r09_mesh_eval_bench.json"))
    ap.add_argument("--tnt", action="store_true", help="also score the post-processed mesh like a Tanks-and-Temples scene")
    ap.add_argument("--tnt_tau", type=float, default=0.004, help="distance threshold in scene units (the voxel size)")
    ap.add_argument("--tnt_gt_points", type=int, default=1_000_000)
    ap.add_argument("--tnt_out", type=str, default=os.path.join(ROOT, "profiles", "r10_tnt_eval_bench.json"))
    ap.add_argument("--unbounded", action="store_true", help="time the unbounded mesh export instead (sphere on a ground plane)")
    ap.add_argument("--mesh_res", type=int, default=1024)
    ap.add_argument("--mesh_crop", type=int, default=512)
    ap.add_argument("--torch_res", type=int, default=-1, help="resolution of the reference-shaped torch run (-1: --mesh_res)")
    ap.add_argument("--unbounded_out", type=str, default=os.path.join(ROOT, "profiles", "unbounded_mesh_bench.json"))
    args = ap.parse_args()
    if args.unbounded:
        ub = unbounded_bench(args)
        print(json.dumps(ub))
        if args.unbounded_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.unbounded_out)), exist_ok=True)
            with open(args.unbounded_out, "w") as f:
                f.write(json.dumps(ub) + "\n")
        return
    from gaussmart_amd.camera import look_at_camera
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.mesh import GaussianExtractor, camera_intrinsics, post_process_mesh, post_process_mesh_device
    from gaussmart_amd.params import PipelineParams
    from gaussmart_amd.tsdf import TSDFVolume
    dev = torch.device("cuda", 0)
    n = args.surfels
    p = fib(n)
    z = np.array([0.0, 0.0, 1.0])
    axis = np.cross(z, p)
    s = np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.arctan2(s[:, 0], p @ z)
    axis = np.where(s > 1e-9, axis / np.maximum(s, 1e-12), np.array([1.0, 0, 0]))
    q = np.concatenate([np.cos(ang / 2)[:, None], axis * np.sin(ang / 2)[:, None]], 1)
    spacing = math.sqrt(4 * math.pi / n)
    params = dict(xyz=torch.tensor(p), features_dc=torch.zeros(n, 1, 3), features_rest=torch.zeros(n, 15, 3),
                  scaling=torch.full((n, 2), math.log(0.8 * spacing)), rotation=torch.tensor(q),
                  opacity=torch.full((n, 1), math.log(0.99 / 0.01)))
    g = GaussianModel(3, device=dev)
    g.create_from_params({k: v.float().to(dev).contiguous() for k, v in params.items()})
    g.active_sh_degree = 0
    cams = []
    for i, d in enumerate(fib(args.views)):
        up = (0, 0, 1) if abs(d[2]) < 0.95 else (0, 1, 0)
        cams.append(look_at_camera(2.5 * d, (0, 0, 0), up, math.radians(50), args.width, args.height, device=dev, uid=i))
    ex = GaussianExtractor(g, render, PipelineParams(depth_ratio=1.0), bg_color=[0, 0, 0])
    sync = torch.cuda.synchronize
    res = {}
    for rep in range(args.repeats):
        sync(); t0 = time.perf_counter()
        ex.reconstruction(cams)
        sync(); t1 = time.perf_counter()
        aabb = ex.block_aabb(args.voxel_size, args.sdf_trunc, args.depth_trunc)
        sync(); t2 = time.perf_counter()
        aabb_dev = ex.block_aabb_device(args.voxel_size, args.sdf_trunc, args.depth_trunc)
        sync(); t2d = time.perf_counter()
        vol = TSDFVolume(args.voxel_size, args.sdf_trunc, aabb_dev, device=dev)
        touched = [vol.integrate(ex._masked_depth(i, True), ex.rgbmaps[i], camera_intrinsics(c), c.world_view_transform.T,
                                 args.depth_trunc) for i, c in enumerate(cams)]
        sync(); t3 = time.perf_counter()
        mesh = vol.extract_triangle_mesh()
        sync(); t4 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            post = post_process_mesh(mesh, 1)
        t5 = time.perf_counter()
        dmesh = vol.extract_triangle_mesh(to_host=False)
        sync(); t6 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            dpost = post_process_mesh_device(dmesh, 1)
        sync(); t7 = time.perf_counter()
        dmesh_host, dpost_host = dmesh.cpu(), dpost.cpu()      # what writing fuse.ply and fuse_post.ply copies
        t8 = time.perf_counter()
        for a, b in ((mesh, dmesh_host), (post, dpost_host)):
            for f in ("vertices", "triangles", "vertex_colors"):
                x, y = getattr(a, f), getattr(b, f)
                assert x.dtype == y.dtype and np.array_equal(x, y), f"host and device path differ in {f}"
        ti = 1e3 * (t3 - t2d)
        res = {"surfels": n, "views": args.views, "width": args.width, "height": args.height,
               "voxel_size": args.voxel_size, "sdf_trunc": args.sdf_trunc, "depth_trunc": args.depth_trunc,
               "grid_blocks": vol.n_blocks, "allocated_blocks": vol.n_alloc, "mean_touched_per_view": float(np.mean(touched)),
               "vertices": len(mesh.vertices), "triangles": len(mesh.triangles), "post_vertices": len(post.vertices),
               "block_aabb": aabb, "block_aabb_device": aabb_dev,
               "render_ms": 1e3 * (t1 - t0), "aabb_ms": 1e3 * (t2 - t1), "aabb_device_ms": 1e3 * (t2d - t2),
               "touch_integrate_ms": ti, "marching_cubes_ms": 1e3 * (t4 - t3), "extract_device_ms": 1e3 * (t6 - t5),
               "post_process_ms": 1e3 * (t5 - t4), "post_process_device_ms": 1e3 * (t7 - t6),
               "device_to_host_ms": 1e3 * (t8 - t7), "integrate_plus_extract_ms": 1e3 * (t4 - t2d),
               "export_total_ms_host": 1e3 * ((t2 - t1) + (t5 - t3)) + ti,
               "export_total_ms_device": 1e3 * ((t2d - t2) + (t8 - t5)) + ti, "repeat": rep}
    print(json.dumps(res))
    if args.cull:
        cull = cull_bench(args, cams, dpost, dev)
        print(json.dumps(cull))
        if args.cull_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.cull_out)), exist_ok=True)
            with open(args.cull_out, "w") as f:
                f.write(json.dumps(cull) + "\n")


    if args.vis:
        vis = vis_bench(args, cams, dpost, dev)
        print(json.dumps(vis))
        if args.vis_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.vis_out)), exist_ok=True)
            with open(args.vis_out, "w") as f:
                f.write(json.dumps(vis) + "\n")
    if args.eval:
        ev = eval_bench(args, dpost, dev)
        print(json.dumps(ev))
        if args.eval_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.eval_out)), exist_ok=True)
            with open(args.eval_out, "w") as f:
                f.write(json.dumps(ev) + "\n")
    if args.tnt:
        tn = tnt_bench(args, dpost, dev)
        print(json.dumps(tn))
        if args.tnt_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.tnt_out)), exist_ok=True)
            with open(args.tnt_out, "w") as f:
                f.write(json.dumps(tn) + "\n")


def surfel_params(p, normals, spacing):
    """Flat surfels at p [n,3] facing normals [n,3], grey, nearly opaque (create_from_params' dictionary)."""
    n = len(p)
    z = np.array([0.0, 0.0, 1.0])
    axis = np.cross(z, normals)
    s = np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.arctan2(s[:, 0], normals @ z)
    axis = np.where(s > 1e-9, axis / np.maximum(s, 1e-12), np.array([1.0, 0, 0]))
    q = np.concatenate([np.cos(ang / 2)[:, None], axis * np.sin(ang / 2)[:, None]], 1)
    return dict(xyz=torch.tensor(p), features_dc=torch.zeros(n, 1, 3), features_rest=torch.zeros(n, 15, 3),
                scaling=torch.full((n, 2), math.log(0.8 * spacing)), rotation=torch.tensor(q),
                opacity=torch.full((n, 1), math.log(0.99 / 0.01)))


def torch_reference_field(views, center, radius, R, resolution, crop, dev):
    """The reference's formulation of the field on the device: per crop torch.linspace, 256^3 chunks, one pass per view,
    grid_sample.  Returns (points evaluated, negative values found)."""
    import torch.nn.functional as F
    n = resolution // crop
    xs = np.linspace(-R, R, n + 1)
    voxel = 2 * radius / resolution
    cen = torch.as_tensor(center, dtype=torch.float32, device=dev)
    total = neg = 0
    for i in range(n):
        for j in range(n):
            for k in range(n):
                x, y, z = (torch.linspace(xs[a], xs[a + 1], crop, device=dev) for a in (i, j, k))
                pts = torch.stack(torch.meshgrid(x, y, z, indexing="ij"), -1).reshape(-1, 3)
                for samples in torch.split(pts, 256 ** 3, dim=0):
                    m = torch.linalg.norm(samples, dim=-1)
                    trunc = 5 * voxel * torch.ones_like(samples[:, 0])
                    mask = m > 1
                    trunc[mask] *= 1 / (2 - m[mask].clamp(max=1.9))
                    mag = m[:, None]
                    w_pts = torch.where(mag < 1, samples, (1 / (2 - mag)) * (samples / mag)) * radius + cen
                    tsdf = torch.ones_like(samples[:, 0])
                    wgt = torch.ones_like(samples[:, 0])
                    hom = torch.cat([w_pts, torch.ones_like(w_pts[:, :1])], -1)
                    for M, depth, _ in views:
                        p = hom @ M
                        zc = p[:, -1:]
                        pix = p[:, :2] / zc
                        ok = ((pix > -1.0) & (pix < 1.0) & (zc > 0)).all(-1)
                        d = F.grid_sample(depth[None], pix[None, None], mode="bilinear", padding_mode="border",
                                          align_corners=True).reshape(-1)
                        sdf = d - zc[:, 0]
                        ok = ok & (sdf > -trunc)
                        t = torch.clamp(sdf / trunc, min=-1.0, max=1.0)[ok]
                        w = wgt[ok]
                        tsdf[ok] = (tsdf[ok] * w + t) / (w + 1)
                        wgt[ok] = w + 1
                    total += len(samples)
                    neg += int((tsdf < 0).sum())
    return total, neg


def unbounded_bench(args):
    from gaussmart_amd import mesh_unbounded as MU
    from gaussmart_amd.camera import look_at_camera
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.params import PipelineParams
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    n = args.surfels
    p = fib(n)
    sp = math.sqrt(4 * math.pi / n)
    half = 6.0
    fstep = 2 * half / math.ceil(2 * half / sp / 4)          # the plane is seen from further away: four times the spacing
    gx, gy = np.meshgrid(np.arange(-half, half + 1e-9, fstep), np.arange(-half, half + 1e-9, fstep))
    fl = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -1.0)], 1)
    a, b = surfel_params(p, p, sp), surfel_params(fl, np.tile([0.0, 0.0, 1.0], (len(fl), 1)), fstep)
    g = GaussianModel(3, device=dev)
    g.create_from_params({k: torch.cat([a[k], b[k]]).float().to(dev).contiguous() for k in a})
    g.active_sh_degree = 0
    dirs = fib(2 * args.views)
    dirs = dirs[dirs[:, 2] > 0][:args.views]
    cams = [look_at_camera(2.5 * d, (0, 0, 0), (0, 0, 1) if abs(d[2]) < 0.95 else (0, 1, 0), math.radians(50), args.width,
                           args.height, device=dev, uid=i) for i, d in enumerate(dirs)]
    ex = MU.UnboundedExtractor(g, render, PipelineParams(depth_ratio=1.0), bg_color=[0, 0, 0])
    with contextlib.redirect_stdout(io.StringIO()):
        ex.reconstruction(cams)
    R = MU.quantile_radius(g.get_xyz, ex.center, ex.radius)
    views = ex.views()
    res, crop = args.mesh_res, args.mesh_crop
    G, nb = MU.lattice_size(res, crop)
    runs = []
    for rep in range(max(args.repeats, 2)):
        stages, last = {}, [0.0]

        def tick(name):
            sync()
            now = time.perf_counter()
            stages[name + "_ms"] = 1e3 * (now - last[0])
            last[0] = now
        sync()
        last[0] = t0 = time.perf_counter()
        tab = MU.ViewTable(views, dev)
        mesh = MU.marching_cubes_contracted(tab, ex.center, ex.radius, R, res, crop, to_host=False, timer=tick)
        sync()
        stages["total_ms"] = 1e3 * (time.perf_counter() - t0)
        runs.append(stages)
        if rep:
            assert torch.equal(mesh.vertices, first), "the vertices differ between two runs"
        first = mesh.vertices
    best = {k: min(r[k] for r in runs[1:]) for k in runs[0]}
    flags = MU.block_flags(tab, ex.center, ex.radius, R, res, crop)
    n_alloc = int(MU.alloc_set_host(flags.cpu().reshape(nb, nb, nb).permute(2, 1, 0)).sum())
    tres = args.mesh_res if args.torch_res < 0 else args.torch_res
    tviews = [(M.to(dev), d.float(), c) for M, d, c in views]
    sync(); t0 = time.perf_counter()
    tpoints, tneg = torch_reference_field(tviews, ex.center, ex.radius, R, tres, crop, dev)
    sync(); torch_ms = 1e3 * (time.perf_counter() - t0)
    dev_field_ms = best["pass1_ms"] + best["pass2_ms"]
    out = {"surfels": len(p), "plane_surfels": len(fl), "views": len(cams), "width": args.width, "height": args.height,
           "mesh_res": res, "mesh_crop": crop, "R": R, "radius": ex.radius, "lattice_points_per_axis": G,
           "lattice_blocks": nb ** 3, "allocated_blocks": n_alloc, "vertices": len(mesh.vertices),
           "triangles": len(mesh.triangles), "device_ms": best, "device_first_run_ms": runs[0],
           "device_field_ms": dev_field_ms, "device_lattice_points": G ** 3,
           "torch_reference_res": tres, "torch_reference_points": tpoints, "torch_reference_negative_points": tneg,
           "torch_reference_field_ms": torch_ms}
    if tres == res:
        out["field_speedup_vs_torch_reference"] = torch_ms / dev_field_ms
    return out


def tnt_bench(args, dpost, dev):
    from gaussmart_amd import tnt_eval as TE
    from gaussmart_amd.mesh import DeviceTriangleMesh
    from tnt_eval_ref import similarity
    rng = np.random.default_rng(0)
    n_gt, tau = args.tnt_gt_points, args.tnt_tau
    gt = (fib(n_gt) * (1.0 + rng.normal(scale=0.25 * tau, size=(n_gt, 1)))).astype(np.float32)
    S = similarity(1.01, [0.3, -0.5, 0.8], 2.0, [0.01, -0.02, 0.015])
    init = similarity(1.0005, [0.6, 0.2, -0.4], 0.1, [0.5 * tau, -0.4 * tau, 0.3 * tau]) @ S
    moved = DeviceTriangleMesh(TE.transform_points(dpost.vertices, np.linalg.inv(S)), dpost.triangles)
    crop = {"orthogonal_axis": "Z", "axis_min": -0.7, "axis_max": 0.9,
            "bounding_polygon": np.array([[-0.9, -0.8, 0.0], [0.85, -0.9, 0.0], [0.9, 0.8, 0.0], [0.1, 0.3, 0.0], [-0.8, 0.9, 0.0]])}
    dev_runs = []
    for rep in range(max(args.repeats, 2)):
        td = {}
        t0 = time.perf_counter()
        d = TE.evaluate_tnt_mesh(moved, gt, crop, tau, init, device=dev, timings=td)
        td["total_ms"] = 1e3 * (time.perf_counter() - t0)
        dev_runs.append(td)
        if rep:
            assert np.array_equal(d["transformation"], first), "the transformation differs between two runs"
        first = d["transformation"]
    th = {}
    t0 = time.perf_counter()
    h = TE.evaluate_tnt_mesh_host(moved.cpu(), gt, crop, tau, init, timings=th)
    th["total_ms"] = 1e3 * (time.perf_counter() - t0)
    for k, (a, b) in enumerate(zip(d["registrations"], h["registrations"])):
        assert a["iterations"] == b["iterations"], f"registration {k}: {a['iterations']} against {b['iterations']} iterations"
        assert [c for c, _ in a["trace"]] == [c for c, _ in b["trace"]], f"registration {k}: correspondence counts differ"
        assert a["fitness"] == b["fitness"], f"registration {k}: fitness differs"
    for key in ("precision", "recall", "fscore"):
        assert d[key] == h[key], f"{key}: {d[key]!r} against {h[key]!r}"
    for key in ("hist_source", "hist_target"):
        assert np.array_equal(d[key], h[key]), f"host and device path differ in {key}"
    best = {k: min(r[k] for r in dev_runs[1:]) for k in dev_runs[0]}
    stages = [k for k in best if k != "total_ms"]
    regs = d["registrations"]
    return {"vertices": len(dpost.vertices), "triangles": len(dpost.triangles), "tau": tau, "gt_points": n_gt,
            "icp_points": [[r["n_source"], r["n_target"]] for r in regs], "icp_iterations": [r["iterations"] for r in regs],
            "icp_fitness": [r["fitness"] for r in regs], "icp_rmse": [r["inlier_rmse"] for r in regs],
            "scored_points": [len(d["cloud_source"]), len(d["cloud_target"])],
            "precision": d["precision"], "recall": d["recall"], "fscore": d["fscore"],
            "transformation_error": float(np.abs(d["transformation"] - S).max()),
            "host_transformation_diff": float(np.abs(d["transformation"] - h["transformation"]).max()),
            "device_ms": best, "device_first_run_ms": dev_runs[0], "host_ms": th,
            "slowest_device_stage": max(stages, key=lambda k: best[k]), "slowest_host_stage": max(stages, key=lambda k: th[k])}


def eval_bench(args, dpost, dev):
    from gaussmart_amd.mesh_eval import evaluate_dtu_mesh, evaluate_dtu_mesh_host
    rng = np.random.default_rng(0)
    n_gt, thresh = args.eval_gt_points, args.eval_density
    gt = (fib(n_gt) * (1.0 + rng.normal(scale=0.5 * thresh, size=(n_gt, 1)))).astype(np.float32)
    obs = np.ones((45, 45, 45), np.uint8)
    obs[:22, :22, :22] = 0                                   # one octant of the volume was not observed
    kw = dict(stl_points=gt, obs_mask=obs, bb=np.array([[-1.1] * 3, [1.1] * 3], np.float32), res=0.05,
              plane=np.array([0.0, 0.0, 1.0, 0.0]), downsample_density=thresh, patch_size=0.1, max_dist=100 * thresh)
    dev_runs = []
    for rep in range(max(args.repeats, 2)):
        td = {}
        t0 = time.perf_counter()
        d = evaluate_dtu_mesh(dpost, timings=td, **kw)
        td["total_ms"] = 1e3 * (time.perf_counter() - t0)
        dev_runs.append(td)
        if rep:
            assert (d["mean_d2s"], d["mean_s2d"]) == first, "the means differ between two runs"
        first = (d["mean_d2s"], d["mean_s2d"])
    th = {}
    t0 = time.perf_counter()
    h = evaluate_dtu_mesh_host(dpost.cpu(), timings=th, **kw)
    th["total_ms"] = 1e3 * (time.perf_counter() - t0)
    for key in ("keep", "inbound", "in_obs", "above", "idx_d2s", "idx_s2d", "dist_d2s", "dist_s2d"):
        assert np.array_equal(d[key].cpu().numpy(), h[key]), f"host and device path differ in {key}"
    for key, dk in (("mean_d2s", "dist_d2s"), ("mean_s2d", "dist_s2d")):
        n = int(np.isfinite(h[dk]).sum())
        assert abs(d[key] - h[key]) <= n * 2.0 ** -53 * h[key], f"{key}: {d[key]!r} against {h[key]!r}"
    best = {k: min(r[k] for r in dev_runs[1:]) for k in dev_runs[0]}
    stages = [k for k in best if k != "total_ms"]
    return {"vertices": len(dpost.vertices), "triangles": len(dpost.triangles), "density": thresh, "gt_points": n_gt,
            "sampled_points": len(h["keep"]), "kept_points": int(h["keep"].sum()), "rounds": d["rounds"],
            "inbound": int(h["inbound"].sum()), "in_obs": int(h["in_obs"].sum()), "gt_above": int(h["above"].sum()),
            "mean_d2s": d["mean_d2s"], "mean_s2d": d["mean_s2d"], "overall": d["overall"],
            "host_mean_d2s": h["mean_d2s"], "host_mean_s2d": h["mean_s2d"],
            "device_ms": best, "device_first_run_ms": dev_runs[0], "host_ms": th,
            "slowest_device_stage": max(stages, key=lambda k: best[k]), "slowest_host_stage": max(stages, key=lambda k: th[k])}


def vis_bench(args, cams, dpost, dev):
    from gaussmart_amd.mesh import camera_intrinsics
    from gaussmart_amd.mesh_visibility import compact_by_counts, render_mesh_depth, visibility_counts, w2c_from_c2w
    sync = torch.cuda.synchronize
    c2w = np.stack([np.linalg.inv(c.world_view_transform.T.cpu().numpy().astype(np.float64)) for c in cams])
    w2c = w2c_from_c2w(c2w, opengl=False)
    intr = camera_intrinsics(cams[0])
    H, W, n, mv = args.height, args.width, len(cams), args.vis_min_views
    F, V = len(dpost.triangles), len(dpost.vertices)
    runs = []
    for rep in range(max(args.repeats, 3)):
        sync(); t0 = time.perf_counter()
        depths = render_mesh_depth(dpost, w2c, H, W, *intr)
        sync(); t1 = time.perf_counter()
        counts = visibility_counts(dpost.vertices, w2c, depths, *intr, min_views=mv)
        sync(); t2 = time.perf_counter()
        culled, keep = compact_by_counts(dpost, counts, mv, return_keep=True)
        sync(); t3 = time.perf_counter()
        runs.append((1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
        if rep == 0:
            first = depths.clone()
        else:
            assert torch.equal(first.view(torch.int32), depths.view(torch.int32)), "depth images differ between two runs"
    kept = int(keep.sum())
    assert 0 < kept < V, f"{kept} of {V} vertices kept: not a culling workload"
    hit = float((depths > 0).float().mean())
    best = [min(r[k] for r in runs[1:]) for k in range(3)]
    # what mv_raster_small has to move: every (triangle, view) pair reads its 12-byte index row; the vertex rows (12 bytes) are
    # gathered three per pair, from HBM at least once per call and at most once per view; every hit pixel is at least one
    # 4-byte atomic.  The image itself is written by the fill before and read and written by the resolve pass after.
    return {"views": n, "width": W, "height": H, "vertices": V, "triangles": F, "pairs": F * n, "min_views": mv,
            "kept_vertices": kept, "culled_vertices": len(culled.vertices), "culled_triangles": len(culled.triangles),
            "hit_pixel_share": hit, "depth_render_ms": best[0], "vote_ms": best[1], "compact_ms": best[2],
            "first_run_ms": list(runs[0]), "all_runs_ms": [list(r) for r in runs],
            "raster_small_index_bytes": 12 * F * n, "raster_small_vertex_bytes_once": 12 * V,
            "raster_small_vertex_bytes_per_view": 12 * V * n, "raster_small_gathered_bytes": 36 * F * n,
            "hit_pixel_atomic_bytes_min": int(4 * hit * n * H * W), "image_bytes": 4 * n * H * W}


def cull_views(cams, width, height):
    """One projection and one ellipse mask per camera.  The ellipse sits on the sphere's image, a little wider and a little
    flatter than it and shifted sideways: every view cuts slivers off the limb, and all views together leave about 60 % of the
    sphere (ellipses smaller than the image would leave nothing: every vertex is on some view's limb)."""
    from gaussmart_amd.mesh import camera_intrinsics
    from gaussmart_amd.mesh_cull import dtu_projection
    proj, masks = [], []
    y, x = np.mgrid[0:height, 0:width]
    for i, cam in enumerate(cams):
        fx, fy, cx, cy = camera_intrinsics(cam)
        wm = np.eye(4)
        wm[:3, :4] = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]) @ cam.world_view_transform.T.cpu().numpy().astype(np.float64)[:3]
        proj.append(dtu_projection(wm, np.eye(4)))
        r_img = fx / math.sqrt(2.5 ** 2 - 1.0)                 # the unit sphere's image radius from distance 2.5
        a, b = r_img * (1.10 + 0.05 * math.sin(i)), r_img * (0.95 + 0.05 * math.cos(2 * i))
        masks.append(((((x - cx - 0.1 * r_img * math.sin(3 * i)) / a) ** 2 + ((y - cy) / b) ** 2) <= 1).astype(np.uint8) * 255)
    return np.stack(proj), np.stack(masks)


def unstable_vertices(verts, proj, dilated, delta):
    """bool [V]: the stability rule of tests/mesh_cull_ref.py (its vote_at and pixel_positions64, nothing restated here), one view
    at a time to keep the arrays small: some view's vote differs among the four positions (cx +- delta, cy +- delta) around the
    float64 pixel position, and no view whose vote is the same at all four removes the vertex."""
    import mesh_cull_ref as R
    n, H, W = dilated.shape
    unstable_any = np.zeros(len(verts), bool)
    stable_remove = np.zeros(len(verts), bool)
    for i in range(n):
        cx, cy = R.pixel_positions64(verts, proj[i:i + 1], (H, W), (H, W))
        votes = np.stack([R.vote_at(cx + sx, cy + sy, dilated[i:i + 1])[0][0] for sx in (-delta, delta) for sy in (-delta, delta)])
        same = (votes == votes[0]).all(0)
        unstable_any |= ~same
        stable_remove |= same & ~votes[0]
    return unstable_any & ~stable_remove


def cull_bench(args, cams, dpost, dev):
    from gaussmart_amd.mesh_cull import compact_host, cull_mesh_by_masks, dilate_masks, dilate_masks_host, vote_host
    import mesh_cull_ref as R
    sync = torch.cuda.synchronize
    proj, masks = cull_views(cams, args.width, args.height)
    hpost = dpost.cpu()
    r = args.cull_radius
    out = {}
    for rep in range(args.repeats):
        sync(); t0 = time.perf_counter()
        dmasks = torch.from_numpy(masks).to(dev)
        sync(); t1 = time.perf_counter()
        dil = dilate_masks(dmasks, r)
        sync(); t2 = time.perf_counter()
        dculled, dkeep = cull_mesh_by_masks(dpost, proj, dmasks, r, return_keep=True)      # dilates again: the whole step
        sync(); t3 = time.perf_counter()
        hdil = dilate_masks_host(masks, r)                     # the three steps of cull_mesh_by_masks_host
        t4 = time.perf_counter()
        hkeep = vote_host(hpost.vertices, proj, hdil)
        hculled = compact_host(hpost, hkeep)
        t5 = time.perf_counter()
        assert np.array_equal(dil.cpu().numpy(), hdil), "device and host dilation differ"
        dk = dkeep.cpu().numpy().astype(bool)
        # DELTA was measured on 320-pixel-wide frames; the pixel error of the fp32 projection grows with the coordinates
        unstable = unstable_vertices(hpost.vertices, proj, hdil, R.DELTA * args.width / 320)
        differ = dk != hkeep
        assert not (differ & ~unstable).any(), f"{int((differ & ~unstable).sum())} stable vertices differ between the paths"
        assert len(hculled.vertices) == int(hkeep.sum())
        assert 0.1 < dk.mean() < 0.9, f"the masks leave {dk.mean():.1%} of the vertices: not a culling workload"
        # both paths from masks in host memory: the device side pays the upload as well
        assert (t1 - t0) + (t3 - t2) <= (t5 - t3), "the device path is slower than the host path"
        out = {"views": len(cams), "width": args.width, "height": args.height, "radius": r,
               "vertices": len(hpost.vertices), "triangles": len(hpost.triangles),
               "culled_vertices": int(dk.sum()), "culled_triangles": len(dculled.triangles),
               "host_culled_vertices": int(hkeep.sum()), "unstable_vertices": int(unstable.sum()),
               "differing_vertices": int(differ.sum()),
               "mask_upload_ms": 1e3 * (t1 - t0), "dilate_device_ms": 1e3 * (t2 - t1), "cull_device_ms": 1e3 * (t3 - t2),
               "cull_device_with_upload_ms": 1e3 * ((t1 - t0) + (t3 - t2)),
               "dilate_host_ms": 1e3 * (t4 - t3), "cull_host_ms": 1e3 * (t5 - t3), "repeat": rep}
    return out


if __name__ == "__main__":
    main()
