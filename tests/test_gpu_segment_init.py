"""The gsr_seg_* kernels (gaussmart_amd.segment_init) against the reference's recorded results
(tests/golden/segment_init.npz), the np.longdouble restatements of tests/segment_cases.py and the numpy twins.

Tolerances, none of them measured on the device: hull distances 8 2^-53 (sum |n_k p_k| + |o|) / |n| of the minimising facet
(both sides round a three-term dot product and one addition); mean / std 4 2^-53 sqrt(N) relative; projections 4 max(e_ref,
one float64 ulp of the view's largest |u|, |v|, |z|) with e_ref the reference's own deviation from longdouble (on file);
statistics and factors max(the reference's float32 deviation from float64, two float32 ulps of the largest magnitude); the new
points two float32 ulps of |mean| + |L| |eps|.  Labels and the keep mask are equal to the reference's on every point that
is not within 1e-6 pixel / 1e-9 of a decision boundary in longdouble (at most 0.1 % of a case)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_cases as SC  # noqa: E402
from test_segment_init_cpu import G, assign_case, camera, check_stats, comparable, proj_tol, write_scan  # noqa: E402,F401
from gaussmart_amd import _lib, segment_cli  # noqa: E402
from gaussmart_amd import segment_init as SI  # noqa: E402
from gaussmart_amd.gaussian_model import GaussianModel  # noqa: E402
from gaussmart_amd.scene_io import BasicPointCloud  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 20000)
ULP, F32_ULP = 2.0 ** -52, 2.0 ** -23


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------- label maps
@pytest.mark.parametrize("H,W", [(120, 160), (113, 157)])
@pytest.mark.parametrize("M", [0, 1, 7, 130])
def test_label_map_equals_host_twin(gpu_device, H, W, M):
    masks = SC.rect_masks(M, H, W, M)
    want_label, want_area = SI.build_label_map_host(masks)
    if M == 130:
        assert want_label.max() > 127
    variants = {"bool": dev_t(masks, gpu_device), "uint8 (values 1..255)": dev_t(masks.astype(np.uint8) * 200, gpu_device)}
    # an odd base address: no plane of this copy starts on a 16-byte boundary
    buf = torch.zeros(M * H * W + 16, dtype=torch.uint8, device=gpu_device)
    buf[3:3 + M * H * W] = dev_t(masks.astype(np.uint8), gpu_device).reshape(-1)
    variants["odd base"] = buf[3:3 + M * H * W].view(M, H, W)
    for name, m in variants.items():
        label, area = SI.build_label_map(m)
        assert label.dtype == torch.int16 and area.dtype == torch.int64
        assert np.array_equal(label.cpu().numpy(), want_label) and np.array_equal(area.cpu().numpy(), want_area), name
    # host masks, uploaded in chunks of two planes
    label, area = SI.build_label_map(masks, device=gpu_device, chunk_bytes=2 * H * W)
    assert np.array_equal(label.cpu().numpy(), want_label) and np.array_equal(area.cpu().numpy(), want_area)


def test_label_map_refusals(gpu_device):
    with pytest.raises(_lib.GsrError):
        SI.build_label_map(torch.zeros((32768, 1, 1), dtype=torch.uint8, device=gpu_device))
    with pytest.raises(_lib.GsrError):
        SI.build_label_map(np.zeros((2, 4, 4), bool))
    L = _lib.lib()
    assert L.gsr_seg_label_map(None, 32768, 1, 1, None, None, None) != 0 and b"32767" in L.gsr_last_error()


# ---------------------------------------------------------------- hull
@pytest.fixture(scope="module")
def hull_cases(G):
    out = {}
    for name, cloud in (("gauss", SC.hull_gauss), ("sphere", SC.hull_sphere), ("filter", SC.filter_cloud)):
        pts = cloud()
        eq = SI.hull_equations(pts)
        assert len(eq) == int(G[f"hull_{name}_n_facets"])
        out[name] = (pts, eq) + SC.hull_distances_ld(pts, eq)
    return out


@pytest.mark.parametrize("name", ["gauss", "sphere"])
def test_hull_distances(gpu_device, G, hull_cases, name):
    pts, eq, d_ld, bound = hull_cases[name]
    d = SI.hull_distances(pts, eq, device=gpu_device).cpu().numpy()
    err, err_ref = np.abs(d - d_ld), np.abs(d - G[f"hull_{name}_d"])
    print(f"{name}: {len(eq)} facets, max |d - ld| / bound {float((err / bound).max()):.3g}, max |d - ref| / bound {float((err_ref / bound).max()):.3g}")
    assert (err <= bound).all() and (err_ref <= bound).all()
    assert np.array_equal(d, SI.hull_distances_host(pts, eq))           # the twin states the same operations
    for n in SIZES[:5]:
        dn = SI.hull_distances(pts[:n], eq, device=gpu_device).cpu().numpy()
        assert dn.shape == (n,) and np.array_equal(dn, d[:n])
    # float32 points are widened on load
    p32 = pts.astype(np.float32)
    d32 = SI.hull_distances(p32, eq, device=gpu_device).cpu().numpy()
    assert np.array_equal(d32, SI.hull_distances_host(p32.astype(np.float64), eq))


@pytest.mark.parametrize("name", ["gauss", "sphere", "filter"])
def test_mean_std(gpu_device, G, hull_cases, name):
    pts, eq, d_ld, _ = hull_cases[name]
    d = SI.hull_distances(pts, eq, device=gpu_device)
    ms, ms_ld = SI.mean_std(d).cpu().numpy(), G[f"hull_{name}_mean_std_ld"]
    rel = 4.0 * 2.0 ** -53 * np.sqrt(len(pts))
    print(f"{name}: mean rel err {abs(ms[0] - ms_ld[0]) / ms_ld[0]:.3g}, std rel err {abs(ms[1] - ms_ld[1]) / ms_ld[1]:.3g}, bound {rel:.3g}")
    assert abs(ms[0] - ms_ld[0]) <= rel * abs(ms_ld[0]) and abs(ms[1] - ms_ld[1]) <= rel * abs(ms_ld[1])


def test_mean_std_edges(gpu_device):
    assert torch.isnan(SI.mean_std(torch.zeros(0, dtype=torch.float64, device=gpu_device))).all()
    one = SI.mean_std(torch.tensor([0.3], dtype=torch.float64, device=gpu_device)).cpu().numpy()
    assert one[0] == 0.3 and one[1] == 0.0
    for n in (63, 64, 65, 300000):
        d = dev_t(SC.uniform(n, 1, 3)[:, 0], gpu_device)
        ms = SI.mean_std(d).cpu().numpy()
        ld = d.cpu().numpy().astype(np.longdouble)
        mean = ld.sum() / n
        std = np.sqrt(((ld - mean) ** 2).sum() / n)
        rel = 4.0 * 2.0 ** -53 * np.sqrt(n)
        assert abs(ms[0] - mean) <= rel * mean and abs(ms[1] - std) <= rel * std


def test_hull_filter(gpu_device, G, hull_cases):
    pts, eq, d_ld, _ = hull_cases["filter"]
    keep, kept, col, nrm = SI.hull_filter(pts, colors=np.arange(len(pts)), device=gpu_device, equations=eq)
    mean = d_ld.sum() / len(d_ld)
    zs = (d_ld - mean) / np.sqrt(((d_ld - mean) ** 2).sum() / len(d_ld))
    ok = ~(np.abs(zs + 1.96) < 1e-9)
    ref_keep = np.unpackbits(G["hull_filter_keep"])[:len(pts)].astype(bool)
    keep = keep.cpu().numpy()
    assert (~ok).mean() <= 1e-3 and np.array_equal(keep[ok], ref_keep[ok]) and 290 <= (~keep).sum() <= 310
    assert nrm is None and np.array_equal(kept.cpu().numpy(), pts[keep]) and np.array_equal(col.cpu().numpy(), np.arange(len(pts))[keep])
    # every point on the hull: std = 0, z is NaN, nothing is kept
    keep, kept, _, _ = SI.hull_filter(SC.cube_corners(), device=gpu_device)
    assert not keep.any() and kept.shape == (0, 3)
    with pytest.raises(ValueError, match="at least 4 points"):
        SI.hull_filter(np.zeros((3, 3)), device=gpu_device)
    with pytest.raises(ValueError, match="degenerate"):
        SI.hull_filter(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0]]), device=gpu_device)


# ---------------------------------------------------------------- projection
@pytest.mark.parametrize("name", ["dtu", "dtu_fb", "dtu2", "nerf", "nerf2", "behind", "tyt", "tyt_nan"])
def test_project_points_against_reference(gpu_device, G, name):
    pts = G["proj_points"].copy()
    if name == "tyt_nan":
        pts[int(G["proj_points_nan_row"]), 1] = np.nan
    kind = str(G[f"proj_{name}_kind"])
    uv, z = (t.cpu().numpy() for t in SI.project_points(pts, camera(G, "tyt" if name == "tyt_nan" else name), kind, device=gpu_device))
    ref_uv, ref_z = G[f"proj_{name}_uv"], G[f"proj_{name}_z"]
    tol = proj_tol(G, name, ref_uv, ref_z)
    print(f"{name}: e_ref {float(G[f'eref_proj_{name}']):.3g}, |uv - ref| {SC.max_dev(uv, ref_uv):.3g}, |z - ref| {SC.max_dev(z, ref_z):.3g}, tol {tol:.3g}")
    assert np.array_equal(np.isnan(uv), np.isnan(ref_uv)) and np.array_equal(np.isnan(z), np.isnan(ref_z))
    assert SC.max_dev(uv, ref_uv) <= tol and SC.max_dev(z, ref_z) <= tol


@pytest.mark.parametrize("name", ["dtu", "dtu_fb", "nerf", "behind", "tyt"])
def test_project_points_sizes(gpu_device, G, name):
    kind = str(G[f"proj_{name}_kind"])
    cam = camera(G, name)
    big = SC.large_cloud(nan_row=name == "tyt")
    for n in SIZES:
        pts = big[:n]
        uv, z = (t.cpu().numpy() for t in SI.project_points(pts, cam, kind, device=gpu_device))
        assert uv.shape == (n, 2) and z.shape == (n,)
        if n == 0:
            continue
        uv_ld, z_ld = SC.project_ld(pts, SI.camera_terms(cam, kind))
        fin = np.isfinite(uv_ld.astype(np.float64)).all(axis=1) & np.isfinite(z_ld.astype(np.float64))
        big_mag = max(float(np.abs(uv_ld[fin]).max()), float(np.abs(z_ld[fin]).max()))
        tol = 4.0 * max(float(G[f"eref_proj_kind_{kind}"]), ULP * 2.0 ** np.floor(np.log2(big_mag)))
        assert np.array_equal(np.isnan(z), np.isnan(z_ld.astype(np.float64)))
        assert SC.max_dev(uv, uv_ld) <= tol and SC.max_dev(z, z_ld) <= tol, (n, SC.max_dev(uv, uv_ld), SC.max_dev(z, z_ld), tol)
        # float32 points are widened on load: the same as their float64 copies
        p32 = pts.astype(np.float32)
        a = SI.project_points(p32, cam, kind, device=gpu_device)
        b = SI.project_points(p32.astype(np.float64), cam, kind, device=gpu_device)
        assert torch.equal(a[0].nan_to_num(7.0), b[0].nan_to_num(7.0)) and torch.equal(a[1].nan_to_num(7.0), b[1].nan_to_num(7.0))
    uv, z = SI.project_points(np.full((5, 3), np.nan), cam, kind, device=gpu_device)
    if kind == "tyt":
        assert not uv.any() and not z.any()                 # every point has a NaN: all zeros


# ---------------------------------------------------------------- assignment
@pytest.mark.parametrize("name", ["dtu", "nerf", "tyt"])
def test_label_points_against_reference(gpu_device, G, name):
    kind, pts, cams, masks, ref_labels, ref_areas = assign_case(G, name)
    labels, areas = SI.label_points(pts, cams, kind, masks, device=gpu_device)
    assert labels.dtype == torch.int32
    labels = labels.cpu().numpy()
    ok = comparable(G, name, kind, pts, cams, masks)
    assert np.array_equal(labels[ok], ref_labels[ok]) and areas == ref_areas
    if name == "dtu":
        assert labels.max() > 127 and (ref_labels == -1).any()
    # the large cloud, and prefixes of it (each has its own DTU in-bounds count and TYT bounds)
    big = SC.large_cloud(nan_row=name == "tyt")
    ref_big = G[f"assign_large_{name}_labels"].astype(np.int64)
    maps = [None if m is None else SI.build_label_map(dev_t(m, gpu_device))[0] for m in masks]
    got = SI.assign_segments(big, cams, kind, maps, device=gpu_device).cpu().numpy()
    ok = comparable(G, name, kind, big, cams, masks)
    assert np.array_equal(got[ok], ref_big[ok]) and (got >= 0).mean() > 0.2
    host_maps = [None if m is None else SI.build_label_map_host(m)[0] for m in masks]
    for n in SIZES[:5]:
        part = SI.assign_segments(big[:n], cams, kind, maps, device=gpu_device).cpu().numpy()
        want = SI.assign_segments_host(big[:n], cams, kind, host_maps)
        ok = comparable(G, name, kind, big[:n], cams, masks) if n else np.zeros(0, bool)
        assert part.shape == (n,) and np.array_equal(part[ok], want[ok])


def test_assign_refusals(gpu_device, G):
    _, pts, cams, masks, _, _ = assign_case(G, "nerf")
    with pytest.raises(_lib.GsrError):
        SI.assign_segments(torch.from_numpy(pts), cams, "nerf", [None] * 3)
    with pytest.raises(_lib.GsrError):
        SI.assign_segments(pts, cams, "nerf", [torch.zeros((4, 4), dtype=torch.int16)] * 3, device=gpu_device)
    # a view whose map would lie outside label_maps is refused before anything is launched
    L = _lib.lib()
    arr = SI._seg_views(cams[:1], "nerf", [(1, 120, 160, 5)])
    p = dev_t(pts, gpu_device)
    ws = torch.empty(L.gsr_seg_views_workspace_bytes(1), dtype=torch.uint8, device=gpu_device)
    rc = L.gsr_seg_views_prepare(SI._ptr(p), 1, len(p), arr, 1, 120 * 160, SI._ptr(ws), ws.numel(), SI._stream(gpu_device))
    assert rc != 0 and b"label_offset" in L.gsr_last_error()


# ---------------------------------------------------------------- statistics, emit
def test_segment_stats(gpu_device, G):
    pts, col, lab = SC.stats_cloud()
    stats = SI.segment_stats(dev_t(pts, gpu_device), dev_t(col, gpu_device), dev_t(lab, gpu_device), 8)
    check_stats(G, stats, SI.segment_factors(stats))
    empty = SI.segment_stats(torch.zeros((0, 3), device=gpu_device), torch.zeros((0, 3), device=gpu_device),
                             torch.zeros(0, dtype=torch.int64, device=gpu_device), 2)
    assert empty["count"].tolist() == [0, 0] and torch.isnan(empty["mean"]).all()
    with pytest.raises(_lib.GsrError):
        SI.segment_stats(torch.from_numpy(pts), torch.from_numpy(col), torch.from_numpy(lab), 8)


def test_augment_emit(gpu_device):
    g = torch.Generator().manual_seed(4)
    add = np.array([5, 0, 300, 1, 64])
    S, total = len(add), int(add.sum())
    eps = torch.randn((total, 3), generator=g)
    mean, tril = torch.randn((S, 3), generator=g) * 3, torch.tril(torch.randn((S, 3, 3), generator=g))
    col, labels = torch.rand((S, 3), generator=g), torch.tensor([2, 3, 7, 40000, 41])
    off = SI._offsets(add)
    xyz, c, lab = SI.augment_emit(eps.to(gpu_device), off, mean, tril, col, labels)
    seg = np.repeat(np.arange(S), add)
    assert lab.cpu().tolist() == labels[seg].tolist() and torch.equal(c.cpu(), col[seg])
    e, Lm, m = eps.double().numpy(), tril.double().numpy()[seg], mean.double().numpy()[seg]
    want = m + np.einsum("nij,nj->ni", Lm, e)
    mag = np.abs(m) + np.einsum("nij,nj->ni", np.abs(Lm), np.abs(e))
    tol = 2.0 * F32_ULP * 2.0 ** np.floor(np.log2(mag))
    assert (np.abs(xyz.cpu().double().numpy() - want) <= tol).all()
    hx, hc, hl = SI.augment_emit_host(eps, off, mean, tril, col, labels)
    assert torch.equal(hx, xyz.cpu()) and torch.equal(hc, c.cpu()) and torch.equal(hl, lab.cpu())
    none = SI.augment_emit(torch.zeros((0, 3), device=gpu_device), [0], torch.zeros((0, 3)), torch.zeros((0, 3, 3)), torch.zeros((0, 3)),
                           torch.zeros(0, dtype=torch.int64))
    assert none[0].shape == (0, 3)
    with pytest.raises(ValueError):
        SI.augment_emit(eps.to(gpu_device), [0, 1, 2, 3, 4, 5], mean, tril, col, labels)


# ---------------------------------------------------------------- end to end
def test_create_from_pcd_augments_on_the_device(gpu_device, G):
    from gaussmart_amd.knn import distCUDA2
    kind, pts, cams, masks, _, _ = assign_case(G, "dtu")
    labels, areas = SI.label_points(pts, cams, kind, masks, device=gpu_device)
    labels = labels.cpu().numpy()
    areas = {k: v * 400 for k, v in areas.items()}          # areas of full-size images: targets above the counts
    colors = SC.uniform(len(pts), 3, 5)
    pcd = BasicPointCloud(pts, colors, np.zeros_like(pts), labels, areas)
    want_labels, add = SI.plan_augmentation(np.bincount(labels[labels >= 0]), areas)
    total = int(add.sum())
    assert total > 0 and len(want_labels) >= 3
    models = []
    for _ in range(2):
        m = GaussianModel(1, device=gpu_device)
        m.create_from_pcd(pcd, 1.0, generator=torch.Generator(device=gpu_device).manual_seed(11))
        models.append(m)
    m, n = models[0], len(pts)
    assert m.get_xyz.shape == (n + total, 3) and m._segments.shape == (n + total,) and m._features_dc.shape == (n + total, 1, 3)
    assert m._segments[n:].cpu().tolist() == np.repeat(want_labels, add).tolist() and torch.isfinite(m.get_xyz).all()
    scales = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(m.get_xyz.detach()), 0.0000001)))[..., None].repeat(1, 2)
    assert torch.equal(m._scaling.detach(), scales)
    for a, b in zip((models[0]._xyz, models[0]._features_dc, models[0]._scaling, models[0]._segments),
                    (models[1]._xyz, models[1]._features_dc, models[1]._scaling, models[1]._segments)):
        assert torch.equal(a, b)
    # the new points of a segment carry its mean SH colour and lie around its mean
    stats = SI.segment_stats(m.get_xyz.detach()[:n], m._features_dc.detach()[:n, 0], m._segments[:n], int(want_labels.max()) + 1)
    l0 = int(want_labels[0])
    new = m._segments[n:] == l0
    assert torch.equal(m._features_dc.detach()[n:, 0][new], stats["mean_color"][l0].expand(int(new.sum()), 3))
    spread = float(stats["std"][l0].max())
    assert float((m.get_xyz.detach()[n:][new] - stats["mean"][l0]).abs().max()) < 6 * 0.5 * spread + 1e-2
    # uniform upsampling: one segment, the new points are labelled 0
    uni = GaussianModel(1, uniform_upsampling=True, device=gpu_device)
    uni.create_from_pcd(pcd._replace(mask_areas={}), 1.0, generator=torch.Generator(device=gpu_device).manual_seed(11))
    assert uni.get_xyz.shape[0] == n + int(0.1 * n) == uni._segments.shape[0] and not uni._segments[n:].any()


def test_segment_cli_device_equals_host(gpu_device, G, tmp_path, capsys):
    scan = str(tmp_path / "scan")
    views, ref_labels, ref_areas = write_scan(G, scan)
    outs = []
    for extra in ([], ["--host"]):
        out = str(tmp_path / ("host" if extra else "dev"))
        segment_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--masks", os.path.join(scan, "masks"), "--views", *map(str, views),
                          "--clean", *extra])
        info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        d = os.path.join(out, "segments", "point_cloud")
        outs.append((np.load(os.path.join(d, "segment_indices.npy")), np.load(os.path.join(d, "mask_areas.npy"), allow_pickle=True).item(), info))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] == ref_areas
    assert outs[0][2]["points"] == outs[1][2]["points"] and not outs[0][2]["host"] and outs[1][2]["host"]


def test_run_to_run_bits(gpu_device, G, hull_cases):
    """every gsr_seg_* result of the large cases has the same bits on a second call"""
    def twice(fn):
        a, b = fn(), fn()
        a, b = (a if isinstance(a, (tuple, list)) else [a]), (b if isinstance(b, (tuple, list)) else [b])
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8) if x.is_floating_point() else x, y.view(torch.uint8) if y.is_floating_point() else y)
        return a
    pts, eq, _, _ = hull_cases["filter"]
    p = dev_t(pts, gpu_device)
    d = twice(lambda: SI.hull_distances(p, eq))[0]
    twice(lambda: SI.mean_std(d))
    kind, _, cams, masks, _, _ = assign_case(G, "dtu")
    big = dev_t(SC.large_cloud(), gpu_device)
    m130 = dev_t(masks[2], gpu_device)
    twice(lambda: SI.build_label_map(m130))
    twice(lambda: SI.project_points(big, cams[3], kind))
    maps = [None if m is None else SI.build_label_map(dev_t(m, gpu_device))[0] for m in masks]
    twice(lambda: SI.assign_segments(big, cams, kind, maps))
    sp, sc, sl = (dev_t(a, gpu_device) for a in SC.stats_cloud())
    twice(lambda: [SI.segment_stats(sp, sc, sl, 8)[k] for k in ("count", "f64")])
    eps = torch.randn((5000, 3), generator=torch.Generator().manual_seed(1)).to(gpu_device)
    twice(lambda: SI.augment_emit(eps, [0, 1000, 5000], torch.ones((2, 3)), torch.eye(3).expand(2, 3, 3), torch.zeros((2, 3)), [3, 4]))
