"""The numpy twins of gaussmart_amd.segment_init (the `*_host` functions, the planning and the file plumbing) against what
the reference's own functions computed (tests/golden/segment_init.npz, written by tests/golden/make_golden_segment_init.py).

create_from_pcd with mask areas on device="cpu" is ROUTED to the host twins (it is not refused): a model on the CPU was
already supported, and the twins state the same rules."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_cases as SC  # noqa: E402
from gaussmart_amd import _lib, segment_cli  # noqa: E402
from gaussmart_amd import segment_init as SI  # noqa: E402
from gaussmart_amd.gaussian_model import GaussianModel  # noqa: E402
from gaussmart_amd.scene_io import BasicPointCloud, fetchPly, storePly  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment_init.npz")
ULP = 2.0 ** -52
F32_ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def camera(G, name):
    cam = {k: G[f"cam_{name}_{k}"] for k in ("world_mat", "scale_mat", "camera_mat")}
    if f"cam_{name}_img_size" in G:
        cam["img_size"] = G[f"cam_{name}_img_size"]
    return cam


def assign_case(G, name):
    """(kind, points, cameras, masks per view or None, reference labels, reference areas)"""
    kind = {"dtu": "dtu", "nerf": "nerf", "tyt": "tyt"}[name]
    pts = G["proj_points"].copy()
    if name == "tyt":
        pts[int(G["proj_points_nan_row"]), 1] = np.nan
    cams, masks = [], []
    for i, c in enumerate(G[f"assign_{name}_cams"]):
        cams.append(camera(G, str(c)))
        if f"assign_{name}_masks_{i}" in G:
            shape = tuple(int(v) for v in G[f"assign_{name}_shape_{i}"])
            masks.append(np.unpackbits(G[f"assign_{name}_masks_{i}"])[:int(np.prod(shape))].reshape(shape).astype(bool))
        else:
            masks.append(None)
    areas = dict(zip(G[f"assign_{name}_area_keys"].tolist(), G[f"assign_{name}_area_values"].tolist()))
    return kind, pts, cams, masks, G[f"assign_{name}_labels"], areas


def proj_tol(G, name, uv, z):
    big = max(float(np.nanmax(np.abs(uv))), float(np.nanmax(np.abs(z))))
    return 4.0 * max(float(G[f"eref_proj_{name}"]), ULP * 2.0 ** np.floor(np.log2(big)))


def comparable(G, name, kind, pts, cams, masks):
    views = []
    for cam, m in zip(cams, masks):
        if m is None:
            views.append(None)
            continue
        uv, z = SC.project_ld(pts, SI.camera_terms(cam, kind))
        views.append((uv, z, m.shape[2], m.shape[1]))
    near = SC.near_boundary(views)
    assert near.mean() <= 1e-3
    return ~near


# ---------------------------------------------------------------- projection
@pytest.mark.parametrize("name", ["dtu", "dtu_fb", "dtu2", "nerf", "nerf2", "behind", "tyt", "tyt_nan"])
def test_project_points_host(G, name):
    pts = G["proj_points"].copy()
    if name == "tyt_nan":
        pts[int(G["proj_points_nan_row"]), 1] = np.nan
    kind = str(G[f"proj_{name}_kind"])
    uv, z = SI.project_points_host(pts, camera(G, "tyt" if name == "tyt_nan" else name), kind)
    ref_uv, ref_z = G[f"proj_{name}_uv"], G[f"proj_{name}_z"]
    tol = proj_tol(G, name, ref_uv, ref_z)
    print(f"{name}: e_ref {float(G[f'eref_proj_{name}']):.3g}, |uv - ref| {SC.max_dev(uv, ref_uv):.3g}, |z - ref| {SC.max_dev(z, ref_z):.3g}, tol {tol:.3g}")
    assert np.array_equal(np.isnan(uv), np.isnan(ref_uv)) and np.array_equal(np.isnan(z), np.isnan(ref_z))
    assert SC.max_dev(uv, ref_uv) <= tol and SC.max_dev(z, ref_z) <= tol


def test_project_tyt_all_nan_is_zero():
    cam = {"world_mat": np.eye(4), "camera_mat": np.eye(4)}
    uv, z = SI.project_points_host(np.full((5, 3), np.nan), cam, "tyt")
    assert not uv.any() and not z.any()


# ---------------------------------------------------------------- label maps, assignment
def test_label_map_host_highest_index_and_areas():
    masks = SC.rect_masks(7, 113, 157, 0)
    label, area = SI.build_label_map_host(masks)
    assert label.dtype == np.int16 and area.dtype == np.int64 and area[0] == 0
    want = np.full((113, 157), -1)
    for m in range(7):
        want[masks[m]] = m
    assert np.array_equal(label, want) and np.array_equal(area, masks.reshape(7, -1).sum(1))
    empty, none = SI.build_label_map_host(np.zeros((0, 4, 5), bool))
    assert (empty == -1).all() and empty.shape == (4, 5) and len(none) == 0
    with pytest.raises(_lib.GsrError):
        SI.build_label_map_host(torch.zeros((32768, 1, 1), dtype=torch.uint8))


def test_merge_mask_areas_keys_by_per_view_index():
    assert SI.merge_mask_areas([np.array([5, 9]), np.array([7, 2, 4]), np.array([], np.int64)]) == {0: 7, 1: 9, 2: 4}
    assert SI.merge_mask_areas([]) == {}


@pytest.mark.parametrize("name", ["dtu", "nerf", "tyt"])
def test_label_points_host_matches_reference(G, name):
    kind, pts, cams, masks, ref_labels, ref_areas = assign_case(G, name)
    labels, areas = SI.label_points_host(pts, cams, kind, masks)
    ok = comparable(G, name, kind, pts, cams, masks)
    assert np.array_equal(labels[ok], ref_labels[ok]) and areas == ref_areas
    assert (labels >= 0).mean() > 0.2 and (labels == -1).any()
    if name == "tyt":
        assert labels[int(G["proj_points_nan_row"])] == ref_labels[int(G["proj_points_nan_row"])]


def test_assign_simple_reference_is_the_label_map_lookup(G):
    _, pts, cams, masks, _, _ = assign_case(G, "dtu")
    label, _ = SI.build_label_map_host(masks[2])
    uv = np.clip(G["proj_dtu2_uv"], [0, 0], [156, 112])
    mine = label[np.rint(uv[:, 1]).astype(int), np.rint(uv[:, 0]).astype(int)]
    assert np.array_equal(mine, G["simple_dtu2_labels"]) and mine.max() > 127


# ---------------------------------------------------------------- hull
@pytest.mark.parametrize("name,cloud", [("gauss", SC.hull_gauss), ("sphere", SC.hull_sphere), ("filter", SC.filter_cloud),
                                        ("corners", SC.cube_corners)])
def test_hull_filter_host(G, name, cloud):
    pts = cloud()
    eq = SI.hull_equations(pts)
    assert len(eq) == int(G[f"hull_{name}_n_facets"])
    d = SI.hull_distances_host(pts, eq)
    d_ld, bound = SC.hull_distances_ld(pts, eq)
    assert (np.abs(d - d_ld) <= bound).all()
    if f"hull_{name}_d" in G:
        assert (np.abs(d - G[f"hull_{name}_d"]) <= bound).all()
    ms, ms_ld = SI.mean_std_host(d), G[f"hull_{name}_mean_std_ld"]
    rel = 4.0 * 2.0 ** -53 * np.sqrt(len(pts))
    assert abs(ms[0] - ms_ld[0]) <= rel * abs(ms_ld[0]) and abs(ms[1] - ms_ld[1]) <= rel * abs(ms_ld[1])
    with np.errstate(all="ignore"):
        keep, kept, col, _ = SI.hull_filter_host(pts, colors=np.arange(len(pts)), equations=eq)
        zs = (d_ld - d_ld.sum() / len(d_ld)) / np.sqrt(((d_ld - d_ld.sum() / len(d_ld)) ** 2).sum() / len(d_ld))
        ok = ~(np.abs(zs + 1.96) < 1e-9)
    ref_keep = np.unpackbits(G[f"hull_{name}_keep"])[:len(pts)].astype(bool)
    assert (~ok).mean() <= 1e-3 and np.array_equal(keep[ok], ref_keep[ok])
    assert len(kept) == keep.sum() == len(col) and np.array_equal(kept, pts[keep])
    if name == "corners":
        assert ms[1] == 0.0 and not keep.any()              # std = 0: z is NaN, nothing is kept
    if name == "filter":
        assert 290 <= (~keep).sum() <= 310


def test_hull_argument_checks():
    with pytest.raises(ValueError, match="at least 4 points"):
        SI.hull_filter_host(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="degenerate"):
        SI.hull_filter_host(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0]]))
    with pytest.raises(ValueError, match="equations"):
        SI.hull_distances_host(np.zeros((5, 3)), np.zeros((0, 4)))
    with pytest.raises(_lib.GsrError, match="device"):
        SI.hull_distances(torch.zeros((5, 3)), np.ones((1, 4)))
    with pytest.raises(_lib.GsrError, match="device"):
        SI.project_points(torch.zeros((5, 3)), {"world_mat": np.eye(4)}, "nerf")
    with pytest.raises(ValueError, match="dataset type"):
        SI.project_points_host(np.zeros((5, 3)), {"world_mat": np.eye(4)}, "llff")


# ---------------------------------------------------------------- statistics, factors, plan, emit
def stats_tol(ref32, ref64, cols):
    """per label: max(the reference's f32 deviation from f64, two f32 ulps of the largest magnitude) over the columns"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # labels without a reference value are all-NaN rows
        dev = np.nanmax(np.abs(ref32[:, cols].astype(np.float64) - ref64[:, cols]), axis=1)
        big = np.nanmax(np.abs(ref64[:, cols]), axis=1)
    return np.maximum(dev, 2.0 * F32_ULP * 2.0 ** np.floor(np.log2(np.maximum(big, 1e-300))))


STAT_COLS = {"mean": slice(0, 3), "cov": slice(3, 12), "std": slice(12, 15), "mean_color": slice(15, 18)}


def check_stats(G, stats, tril):
    ref32, ref64 = G["stats_ref32"], G["stats_ref64"]
    _, _, lab = SC.stats_cloud()
    counts = np.bincount(lab[lab >= 0], minlength=8)
    assert np.array_equal(stats["count"].cpu().numpy(), counts) and counts.tolist() == [0, 1, 4, 5, 6, 8, 6, 10000]
    with np.errstate(all="ignore"):
        for key, cols in STAT_COLS.items():
            got = stats[key].cpu().numpy().reshape(8, -1).astype(np.float64)
            assert stats[key].dtype == torch.float32
            tol = stats_tol(ref32, ref64, cols)
            for l in range(8):
                if counts[l] == 0 or (counts[l] < 2 and key in ("cov", "std")):
                    assert np.isnan(got[l]).all(), (key, l)
                else:
                    assert (np.abs(got[l] - ref64[l, cols]) <= tol[l]).all(), (key, l, got[l], ref64[l, cols], tol[l])
        tol = stats_tol(ref32, ref64, slice(18, 27))
        L = tril.numpy().reshape(-1, 9).astype(np.float64)
        for l in range(2, 8):
            assert (np.abs(L[l] - ref64[l, 18:27]) <= tol[l]).all(), (l, L[l], ref64[l, 18:27], tol[l])
        for l in (5, 6):                                    # collinear, coincident: the eigenvalue clamp
            M = L[l].reshape(3, 3)
            assert np.linalg.eigvalsh(M @ M.T).min() >= 0.25e-6 * (1 - 1e-3)


def test_segment_stats_host(G):
    pts, col, lab = SC.stats_cloud()
    stats = SI.segment_stats_host(pts, col, lab, 8)
    check_stats(G, stats, SI.segment_factors(stats))


def test_segment_factors_fallback_is_half_std():
    s64 = torch.full((2, 18), float("nan"), dtype=torch.float64)
    s64[1, 3:12] = torch.eye(3, dtype=torch.float64).reshape(-1) * 4.0
    s64[:, 12:15] = torch.tensor([[2.0, 4.0, 6.0], [2.0, 2.0, 2.0]], dtype=torch.float64)
    tril = SI.segment_factors({"f64": s64})
    assert torch.equal(tril[0], torch.diag(torch.tensor([1.0, 2.0, 3.0]))) and torch.allclose(tril[1], torch.eye(3))


def test_plan_augmentation():
    areas = {1: 40000, 2: 10 ** 6, 3: 90000, 7: 100}
    counts = np.array([50, 4, 5, 31, 6, 9, 12, 9])
    labels, add = SI.plan_augmentation(counts, areas)
    median = np.median(list(areas.values()))                # 65000: int(sqrt) * 0.1 = 25
    want = {}
    for l, c in enumerate(counts):
        t = max(int(np.sqrt(areas.get(l, median)) * 0.1), 10)
        if c >= 5 and t - c > 0:
            want[l] = t - c
    assert dict(zip(labels.tolist(), add.tolist())) == want == {2: 95, 4: 19, 5: 16, 6: 13, 7: 1}
    assert list(labels) == sorted(labels)
    assert len(SI.plan_augmentation(counts, {})[0]) == 0 and len(SI.plan_augmentation([], areas)[0]) == 0


def test_augment_emit_host():
    eps = torch.randn((7, 3), generator=torch.Generator().manual_seed(1))
    mean, tril = torch.tensor([[1.0, 2, 3], [4, 5, 6], [7, 8, 9]]), torch.tril(torch.rand((3, 3, 3), generator=torch.Generator().manual_seed(2)))
    col, labels = torch.rand((3, 3), generator=torch.Generator().manual_seed(3)), torch.tensor([4, 9, 11])
    xyz, c, lab = SI.augment_emit_host(eps, [0, 3, 3, 7], mean, tril, col, labels)
    seg = [0, 0, 0, 2, 2, 2, 2]
    assert lab.tolist() == [4, 4, 4, 11, 11, 11, 11] and torch.equal(c, col[seg])
    want = mean[seg].double() + torch.einsum("nij,nj->ni", tril[seg].double(), eps.double())
    assert torch.allclose(xyz.double(), want, rtol=0, atol=4 * F32_ULP * 16)


# ---------------------------------------------------------------- model, files, command
def test_create_from_pcd_cpu_is_routed_to_the_host_twins(G):
    pts, col, lab = SC.stats_cloud()
    areas = {2: 10 ** 5, 3: 250000, 4: 10 ** 6, 5: 40000, 6: 40000, 7: 100}
    pcd = BasicPointCloud(pts.astype(np.float64), np.clip(col * 0.5 + 0.5, 0, 1).astype(np.float64), np.zeros_like(pts), lab, areas)
    dist2 = lambda p: torch.full((len(p),), 0.01)
    labels, add = SI.plan_augmentation(np.bincount(lab[lab >= 0]), areas)
    assert labels.tolist() == [3, 4, 5, 6] and add.tolist() == [45, 94, 12, 14]
    models = []
    for _ in range(2):
        m = GaussianModel(1, device="cpu")
        m.create_from_pcd(pcd, 1.0, dist2_fn=dist2, generator=torch.Generator().manual_seed(5))
        models.append(m)
    m = models[0]
    n, total = len(pts), int(add.sum())
    assert m.get_xyz.shape == (n + total, 3) and m._segments.shape == (n + total,) and m._scaling.shape == (n + total, 2)
    assert torch.equal(m._segments[:n], torch.from_numpy(lab)) and m._segments[n:].tolist() == np.repeat(labels, add).tolist()
    assert torch.equal(m.get_xyz[:n], torch.from_numpy(pts)) and torch.isfinite(m.get_xyz).all()
    assert torch.equal(models[0].get_xyz, models[1].get_xyz) and torch.equal(models[0]._features_dc, models[1]._features_dc)
    # the new points of the coincident segment stay within a few sigma = 0.5 sqrt(1e-6) of it
    six = m.get_xyz[n:][m._segments[n:] == 6]
    assert (six - torch.tensor([1.25, -0.75, 3.5])).abs().max() < 6 * 0.5e-3
    # no mask areas, no uniform upsampling: nothing is added; uniform upsampling adds max(int(0.1 n), 10) points labelled 0
    plain = GaussianModel(1, device="cpu")
    plain.create_from_pcd(pcd._replace(mask_areas={}), 1.0, dist2_fn=dist2)
    assert plain.get_xyz.shape[0] == n and torch.equal(plain._segments, torch.from_numpy(lab))
    uni = GaussianModel(1, uniform_upsampling=True, device="cpu")
    uni.create_from_pcd(pcd._replace(mask_areas={}), 1.0, dist2_fn=dist2, generator=torch.Generator().manual_seed(5))
    assert uni.get_xyz.shape[0] == n + int(0.1 * n) == uni._segments.shape[0] and not uni._segments[n:].any()


def test_fetch_ply_segmentation_dir(tmp_path):
    xyz = SC.cube(10, 0)
    storePly(str(tmp_path / "p.ply"), xyz, np.full((10, 3), 128), np.arange(10, dtype=np.int32))
    assert fetchPly(str(tmp_path / "p.ply")).mask_areas == {} and BasicPointCloud(1, 2, 3, 4).mask_areas == {}
    seg = tmp_path / "seg"
    seg.mkdir()
    np.save(seg / "segment_indices.npy", np.array([3, -1, 2, 2, 0, 1, 1], np.int64))
    np.save(seg / "mask_areas.npy", {0: 11, 3: 500})
    pcd = fetchPly(str(tmp_path / "p.ply"), str(seg))
    assert len(pcd.points) == len(pcd.colors) == len(pcd.normals) == 7 and pcd.segments.tolist() == [3, -1, 2, 2, 0, 1, 1]
    assert pcd.mask_areas == {0: 11, 3: 500}
    np.save(seg / "segment_indices.npy", np.arange(12))
    assert len(fetchPly(str(tmp_path / "p.ply"), str(seg)).segments) == 10
    with pytest.raises(FileNotFoundError):
        fetchPly(str(tmp_path / "p.ply"), str(tmp_path / "nothing"))


def write_scan(G, root):
    """A tiny scan directory of the fixture's dtu case, as segment_cli reads it.  Returns (--views, reference labels, areas)."""
    kind, pts, cams, masks, ref_labels, ref_areas = assign_case(G, "dtu")
    os.makedirs(root)
    segment_cli.write_cloud_ply(os.path.join(root, "points.ply"), pts, np.full((len(pts), 3), 200, np.uint8))
    views = [4, 2, 7, 5]                                    # camera indices in the file, in the order of the mask files
    mats = {}
    for i, cam in zip(views, cams):
        for k in ("world_mat", "scale_mat", "camera_mat"):
            mats[f"{k}_{i}"] = cam[k]
    np.savez(os.path.join(root, "cameras.npz"), **mats)
    os.makedirs(os.path.join(root, "masks"))
    for k, m in enumerate(masks):
        np.savez_compressed(os.path.join(root, "masks", f"segments_{k:03d}.npz"), masks=np.zeros((0, 4, 4), bool) if m is None else m)
    return views, ref_labels, ref_areas


def test_segment_cli_host(G, tmp_path, capsys):
    scan, out = str(tmp_path / "scan"), str(tmp_path / "out")
    views, ref_labels, ref_areas = write_scan(G, scan)
    segment_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--masks", os.path.join(scan, "masks"), "--views", *map(str, views),
                      "--host", "--dump_projection", "0"])
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    d = os.path.join(out, "segments", "point_cloud")
    labels = np.load(os.path.join(d, "segment_indices.npy"))
    areas = np.load(os.path.join(d, "mask_areas.npy"), allow_pickle=True).item()
    assert info["points"] == 600 == len(labels) and info["host"] and labels.dtype == np.int64
    kind, pts, cams, masks, _, _ = assign_case(G, "dtu")
    ok = comparable(G, "dtu", kind, pts, cams, masks)
    assert areas == ref_areas and np.array_equal(labels[ok], ref_labels[ok]) and (labels >= 0).sum() == info["labelled"] > 100
    for f in ("raw_pc.ply", "segmented_point_cloud.ply", "projection_000.npz"):
        assert os.path.exists(os.path.join(d, f))
    # the written directory is what --segmentation_dir reads, and the cloud goes round
    pcd = fetchPly(os.path.join(d, "segmented_point_cloud.ply"), d)
    assert np.array_equal(pcd.segments, labels) and pcd.mask_areas == areas and np.array_equal(pcd.points, G["proj_points"])
    # --clean filters first (the blob has nothing to remove at 1.96 sigma below the mean, a far shell does)
    segment_cli.main(["-s", scan, "-o", out + "2", "-t", "dtu", "--masks", os.path.join(scan, "masks"), "--views", *map(str, views),
                      "--host", "--clean"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["points"] <= 600
    with pytest.raises(SystemExit):
        segment_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--masks", os.path.join(scan, "masks"), "--views", "4", "2", "9", "--host"])
