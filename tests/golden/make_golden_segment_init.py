"""Regenerate tests/golden/segment_init.npz: what the reference's own functions compute on the inputs of
tests/segment_cases.py, on the CPU.

    python tests/golden/make_golden_segment_init.py /path/to/reference/checkout

identification/pc_projection.py (project_points_to_view, assign_segment_indices_simple and its view loop
process_all_views_with_mask_size, which states the loop of identification/main.py:114-148 without that file's SAM imports),
filter/hull_removal.py (HullRemoval.filtering, compute_hull_distances) and scene/gaussian_model.py
(calculate_segment_covariance, then MultivariateNormal(mean, cov).scale_tril) are loaded by file path; open3d, cv2,
matplotlib and plyfile are stubbed in sys.modules, simple_knn comes from this repository.  Beside each float result the same
formulas are evaluated in np.longdouble (float64 for the torch parts) and the reference's largest deviation from them is
recorded (`eref_*`): the reference's own rounding error is on file.  Masks are bit-packed."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _load(ref_root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stubs():
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.ModuleType("open3d.geometry")
    o3d.geometry.PointCloud = type("PointCloud", (), {})
    for name, mod in (("open3d", o3d), ("open3d.geometry", o3d.geometry), ("cv2", types.ModuleType("cv2")),
                      ("matplotlib", types.ModuleType("matplotlib")), ("matplotlib.pyplot", types.ModuleType("matplotlib.pyplot"))):
        sys.modules.setdefault(name, mod)
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = object
    sys.modules.setdefault("plyfile", ply)


def _rot(ax, ay):
    ca, sa, cb, sb = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])


def _dtu_cam(R, t, fx, cx, cy):
    world = np.eye(4)
    world[:3, :3], world[:3, 3] = R, t
    world[3] = world[2]                                     # w = depth: u = fx X / Z + cx
    scale = np.diag([1.1, 1.1, 1.1, 1.0])
    scale[:3, 3] = [0.02, -0.03, 0.01]
    return {"world_mat": world, "scale_mat": scale, "camera_mat": np.array([[fx, 0, cx, 0], [0, fx, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])}


def _rt_cam(R, t, fx, cx, cy, **extra):
    world = np.eye(4)
    world[:3, :3], world[:3, 3] = R, t
    cam = {"world_mat": world, "scale_mat": np.eye(4), "camera_mat": np.array([[fx, 0, cx, 0], [0, fx, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])}
    cam.update(extra)
    return cam


CAM_KEYS = ("world_mat", "scale_mat", "camera_mat")


def main(ref_root):
    _stubs()
    import torch
    from torch.distributions import MultivariateNormal
    import segment_cases as SC
    from gaussmart_amd import segment_init as SI
    sys.path.insert(0, ref_root)
    proj = _load(ref_root, "identification/pc_projection.py", "ref_pc_projection")
    hull = _load(ref_root, "filter/hull_removal.py", "ref_hull_removal")
    gm = _load(ref_root, "scene/gaussian_model.py", "ref_gaussian_model")
    out = {}

    # ------------------------------------------------------------ projection
    pts = SC.blob(600, 7) * 0.6
    out["proj_points"] = pts
    t4 = np.array([0.05, -0.02, 4.0])
    cams = {
        "dtu": ("dtu", _dtu_cam(_rot(0.1, -0.15), t4, 300.0, 80.0, 60.0)),
        "dtu_fb": ("dtu", _dtu_cam(_rot(0.0, 0.0), t4, 300.0, -9000.0, 60.0)),
        "dtu2": ("dtu", _dtu_cam(_rot(-0.2, 0.1), t4, 280.0, 78.0, 56.0)),
        "nerf": ("nerf", _rt_cam(_rot(0.12, 0.2), t4, 300.0, 80.0, 60.0)),
        "nerf2": ("nerf", _rt_cam(_rot(-0.1, -0.25), t4, 280.0, 78.0, 56.0)),
        "behind": ("nerf", _rt_cam(_rot(0.0, np.pi), -t4, 300.0, 80.0, 60.0)),
        "tyt": ("tyt", _rt_cam(_rot(0.1, 0.1), t4, 300.0, 80.0, 60.0, img_size=np.array([160, 120]))),
    }
    pts_nan = pts.copy()
    pts_nan[17, 1] = np.nan
    out["proj_points_nan_row"] = np.int64(17)
    eref = {}
    for name, (kind, cam) in list(cams.items()) + [("tyt_nan", ("tyt", cams["tyt"][1]))]:
        p = pts_nan if name == "tyt_nan" else pts
        uv, z = proj.project_points_to_view(p.copy(), cam, kind)
        uv_ld, z_ld = SC.project_ld(p, SI.camera_terms(cam, kind))
        e = max(SC.max_dev(uv, uv_ld), SC.max_dev(z, z_ld))
        eref[name] = e
        out[f"proj_{name}_uv"], out[f"proj_{name}_z"], out[f"eref_proj_{name}"] = uv, z, np.float64(e)
        out[f"proj_{name}_kind"] = np.array(kind)
        if name != "tyt_nan":
            for k in CAM_KEYS:
                out[f"cam_{name}_{k}"] = cam[k]
            if "img_size" in cam:
                out[f"cam_{name}_img_size"] = cam["img_size"]
    for kind in ("dtu", "nerf", "tyt"):
        out[f"eref_proj_kind_{kind}"] = np.float64(max(e for n, e in eref.items() if str(out[f"proj_{n}_kind"]) == kind))
    # the fallback view is a fallback, the others are not
    inb = lambda uv: ((uv[:, 0] >= 0) & (uv[:, 0] < 1554) & (uv[:, 1] >= 0) & (uv[:, 1] < 1162)).sum()
    main_fb = SC.project_ld(pts, SI.camera_terms(cams["dtu_fb"][1], "dtu"), fallback=False)[0]
    assert inb(main_fb) < 0.1 * len(pts) and inb(SC.project_ld(pts, SI.camera_terms(cams["dtu"][1], "dtu"), fallback=False)[0]) > 0.5 * len(pts)
    assert (out["proj_behind_z"] < 0).all()

    # ------------------------------------------------------------ assignment
    cases = {
        "dtu": ("dtu", ["dtu", "dtu2", "dtu2", "dtu_fb"], [SC.rect_masks(7, 120, 160, 0), None, SC.rect_masks(130, 113, 157, 1),
                                                              SC.centre_masks(1162, 1554)]),
        "nerf": ("nerf", ["nerf", "behind", "nerf2"], [SC.rect_masks(1, 120, 160, 3), SC.rect_masks(7, 113, 157, 4),
                                                        SC.rect_masks(7, 113, 157, 5)]),
        "tyt": ("tyt", ["tyt", "tyt"], [SC.rect_masks(7, 120, 160, 6), SC.rect_masks(1, 113, 157, 7)]),
    }
    for name, (kind, cam_names, masks) in cases.items():
        p = pts_nan if name == "tyt" else pts
        all_masks = [[] if m is None else [{"segmentation": plane} for plane in m] for m in masks]
        cam_dict = {f"camera_{i:03d}": cams[c][1] for i, c in enumerate(cam_names)}
        labels, areas = proj.process_all_views_with_mask_size(p.copy(), all_masks, cam_dict, kind)
        out[f"assign_{name}_labels"] = np.asarray(labels, np.int64)
        out[f"assign_{name}_area_keys"] = np.array(sorted(areas), np.int64)
        out[f"assign_{name}_area_values"] = np.array([areas[k] for k in sorted(areas)], np.int64)
        out[f"assign_{name}_cams"] = np.array(cam_names)
        for i, m in enumerate(masks):
            if m is not None:
                out[f"assign_{name}_masks_{i}"] = np.packbits(m, axis=None)
                out[f"assign_{name}_shape_{i}"] = np.array(m.shape, np.int64)
        assert (labels >= 0).mean() > 0.2, name
        # the same views on the large cloud of the GPU tests (tests/segment_cases.py:large_cloud)
        big = SC.large_cloud(nan_row=name == "tyt")
        out[f"assign_large_{name}_labels"] = np.asarray(proj.process_all_views_with_mask_size(big, all_masks, cam_dict, kind)[0], np.int16)
    # the fallback view alone puts at least 20 % of the points inside its masks
    fb_masks = cases["dtu"][2][3]
    uv_fb = out["proj_dtu_fb_uv"]
    one = proj.assign_segment_indices_simple(np.clip(uv_fb, [0, 0], [1553, 1161]), list(fb_masks))
    vis = (uv_fb[:, 0] >= 0) & (uv_fb[:, 0] < 1554) & (uv_fb[:, 1] >= 0) & (uv_fb[:, 1] < 1162) & (out["proj_dtu_fb_z"] > 0)
    assert (vis & (one >= 0)).mean() >= 0.2, (vis & (one >= 0)).mean()
    # assign_segment_indices_simple on its own: the 130 masks of view 2 on that view's clipped coordinates
    uv2 = np.clip(out["proj_dtu2_uv"], [0, 0], [156, 112])
    out["simple_dtu2_labels"] = np.asarray(proj.assign_segment_indices_simple(uv2, list(cases["dtu"][2][2])), np.int64)

    # ------------------------------------------------------------ hull
    for name, cloud in (("gauss", SC.hull_gauss()), ("sphere", SC.hull_sphere()), ("filter", SC.filter_cloud()),
                        ("corners", SC.cube_corners())):
        hr = hull.HullRemoval(None)
        with np.errstate(all="ignore"):
            keep, h = hr.filtering(cloud)
            d = hr.compute_hull_distances(cloud, h)
        d_ld, _ = SC.hull_distances_ld(cloud, h.equations)
        mean_ld = d_ld.sum() / len(d_ld)
        std_ld = np.sqrt(((d_ld - mean_ld) ** 2).sum() / len(d_ld))
        out[f"hull_{name}_keep"] = np.packbits(keep)
        out[f"hull_{name}_n_facets"] = np.int64(len(h.equations))
        out[f"hull_{name}_mean_std"] = np.array([np.mean(d), np.std(d)])
        out[f"hull_{name}_mean_std_ld"] = np.array([mean_ld, std_ld], np.float64)
        out[f"eref_hull_{name}"] = np.float64(SC.max_dev(d, d_ld))
        if name != "filter":
            out[f"hull_{name}_d"] = d
        if name in ("gauss", "corners"):
            out[f"hull_{name}_equations"] = h.equations
        print(f"hull {name}: {len(cloud)} points, {len(h.equations)} facets, removed {(~keep).sum()}, std {np.std(d):.3g}")
        if name == "filter":
            with np.errstate(all="ignore"):
                zs = (d_ld - mean_ld) / std_ld
            assert 290 <= (~keep).sum() <= 310 and not (np.abs(zs + 1.96) < 1e-9).any()
        if name == "corners":
            assert np.std(d) == 0.0 and not keep.any()

    # ------------------------------------------------------------ per-segment statistics
    spts, scol, slab = SC.stats_cloud()
    model = gm.GaussianModel.__new__(gm.GaussianModel)
    n_labels = int(slab.max()) + 1
    ref32, ref64 = np.full((n_labels, 27), np.nan, np.float32), np.full((n_labels, 27), np.nan)
    for dt, dst in ((torch.float32, ref32), (torch.float64, ref64)):
        P, Cc = torch.from_numpy(spts).to(dt), torch.from_numpy(scol).to(dt)
        for l in range(n_labels):
            sel = torch.from_numpy(slab == l)
            k = int(sel.sum())
            if k == 0:
                continue
            seg = P[sel]
            dst[l, 0:3] = seg.mean(dim=0).numpy()
            dst[l, 15:18] = Cc[sel].mean(dim=0).numpy()
            if k < 2:
                continue
            dst[l, 3:12] = torch.cov(seg.T).reshape(-1).numpy()
            dst[l, 12:15] = seg.std(dim=0).numpy()
            try:
                mean, scaled = model.calculate_segment_covariance(seg)
                dst[l, 18:27] = MultivariateNormal(mean, scaled).scale_tril.reshape(-1).numpy()
            except Exception as e:                          # the reference's except branch: diag(0.5 std)
                print(f"segment {l} ({dt}): {type(e).__name__}")
                dst[l, 18:27] = torch.diag(0.5 * seg.std(dim=0)).reshape(-1).numpy()
    out["stats_ref32"], out["stats_ref64"] = ref32, ref64

    path = os.path.join(HERE, "segment_init.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    print("e_ref:", {k: float(v) for k, v in out.items() if k.startswith("eref_")})


if __name__ == "__main__":
    main(sys.argv[1])
