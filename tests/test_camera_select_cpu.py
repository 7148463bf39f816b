"""gaussmart_amd.camera_select and gaussmart_amd.identify_cli without a device: the numpy twin against the golden file of the
reference's CameraClustering and against scikit-learn, KMeans' choice among its initialisations, the Tanks-and-Temples mapping,
the refusals, the header, and the command with --host on an 8-camera scan."""
import json
import os
import re

import numpy as np
import pytest

import camera_select_cases as KC
from conftest import ROOT
from gaussmart_amd import _lib
from gaussmart_amd import camera_select as CS


@pytest.mark.parametrize("name", KC.SETS)
def test_twin_equals_the_reference(name):
    g, details = KC.golden(), {}
    res = CS.select_representative_cameras(KC.views_of(name), details=details)
    assert details["best_k"] == int(g[f"{name}_best_k"])
    assert np.array_equal(details["labels"], g[f"{name}_labels"])
    assert res["selected_indices"] == g[f"{name}_selected"].tolist()           # and their order: the cluster label order
    ks = g[f"{name}_ks"].tolist()
    assert sorted(details["scores"]) == ks
    np.testing.assert_allclose([details["inertia"][k] for k in ks], g[f"{name}_inertia"], rtol=1e-9, atol=0)
    np.testing.assert_allclose([details["scores"][k] for k in ks], g[f"{name}_score"], rtol=1e-9, atol=0)
    np.testing.assert_allclose([res["cluster_info"][c]["score"] for c in range(details["best_k"])], g[f"{name}_rep_score"], rtol=1e-9, atol=0)
    assert [res["cluster_info"][c]["selected"] for c in range(details["best_k"])] == res["selected_indices"]
    assert sorted(sum((res["cluster_info"][c]["members"] for c in range(details["best_k"])), [])) == list(range(len(g[f"{name}_labels"])))


def test_small_sets_stop_at_four_clusters():
    g = KC.golden()
    assert g["dome7_ks"].tolist() == g["dome8_ks"].tolist() == [3, 4] and g["dome31_ks"].tolist() == list(range(3, 16))


@pytest.mark.parametrize("name", ("ring49", "blob120"))
def test_twin_labels_equal_scikit_learn(name):
    cluster = pytest.importorskip("sklearn.cluster")
    X, _, _ = CS.normalize_positions(CS.camera_centres_dirs(KC.views_of(name))[0])
    ks = list(range(3, 16))
    fits = CS.kmeans_many(X, ks)
    for k in ks:
        km = cluster.KMeans(n_clusters=k, n_init=10, random_state=42)
        assert np.array_equal(km.fit_predict(X), fits[k][0]), k
        assert abs(km.inertia_ - fits[k][2]) <= 1e-9 * km.inertia_
        np.testing.assert_allclose(fits[k][1], km.cluster_centers_, rtol=0, atol=1e-12)
    labels, centres, inertia = CS.kmeans(X, 5)
    assert np.array_equal(labels, fits[5][0]) and inertia == fits[5][2] and centres.shape == (5, 3)


def test_an_equal_partition_does_not_replace_the_best_fit():
    first = np.array([0, 0, 1, 1, 2, 2])
    permuted = np.array([2, 2, 0, 0, 1, 1])            # the same partition under other names
    other = np.array([0, 1, 1, 2, 2, 0])
    assert CS.is_same_clustering(first, permuted, 3) and not CS.is_same_clustering(first, other, 3)
    assert CS.pick_best(np.stack([first, permuted]), np.array([2.0, 1.0]), 3) == 0       # lower inertia, same partition: stays
    assert CS.pick_best(np.stack([first, other]), np.array([2.0, 1.0]), 3) == 1          # lower inertia, another partition
    assert CS.pick_best(np.stack([first, other]), np.array([2.0, 2.0]), 3) == 0          # not strictly lower
    assert CS.pick_best(np.stack([first, permuted, other]), np.array([2.0, 1.0, 1.5]), 3) == 2


def test_kmeans_plus_plus_follows_the_random_stream():
    X = KC.cloud(40, 3)
    a, b = np.random.RandomState(42), np.random.RandomState(42)
    first = [CS.kmeans_pp_init(X, 5, a) for _ in range(2)]
    # what one initialisation draws: one choice, then 2 + int(log 5) = 3 uniforms per further centre
    b.choice(40, p=np.full(40, 1 / 40))
    for _ in range(4):
        b.uniform(size=3)
    again = CS.kmeans_pp_init(X, 5, b)
    assert np.array_equal(again, first[1]) and not np.array_equal(first[0], first[1])
    assert all((c[:, None, :] == X[None]).all(-1).any(1).all() for c in first)             # every centre is a point


def test_host_twin_status_and_shapes():
    X = KC.cloud(65, 1)
    ks = [3, 15, 1, 0, 17]
    c0 = np.zeros((5, _lib.GSR_CK_KMAX, 3))
    c0[:3] = KC.inits(X, [3, 15, 1])
    res = CS.lloyd_batch_host(X, c0, ks, KC.tolerance(X))
    assert res["status"].tolist() == [0, 0, 0, 2, 2] and res["labels"][3:].tolist() == [[-1] * 65] * 2
    assert res["labels"].dtype == np.int32 and res["n_iter"].dtype == np.int32 and res["centres"].shape == (5, 16, 3)
    assert (res["centres"][0, 3:] == 0).all() and set(res["labels"][1]) == set(range(15))
    # one cluster: its centre is the mean in the rule's order and the inertia is the summed squared norm
    np.testing.assert_allclose(res["centres"][2, 0], 0.0, atol=1e-15)
    np.testing.assert_allclose(res["inertia"][2], (X ** 2).sum(), rtol=1e-12)
    far = KC.inits(X, [3])
    far[0, 2] = 1e6                                             # a centre no point is nearest to
    lost = CS.lloyd_batch_host(X, far, [3], KC.tolerance(X))
    assert lost["status"].tolist() == [1] and lost["n_iter"].tolist() == [1] and np.array_equal(lost["centres"][0], far[0])
    # the Python layer redoes such a fit with scikit-learn's relocation: three clusters come back
    redone = CS.lloyd_batch_host(X, far, [3], KC.tolerance(X), relocate=True)
    assert redone["status"].tolist() == [0] and set(redone["labels"][0]) == {0, 1, 2}


def test_tyt_keeps_half_the_rows_and_maps_indices(tmp_path):
    g = KC.golden()
    path = str(tmp_path / "poses_bounds.npy")
    np.save(path, g["tyt20_poses"])
    assert len(g["tyt20_poses"]) == 40
    selected, views = CS.select_views(path, "tyt")
    assert sorted(views) == list(range(20))
    np.testing.assert_allclose(np.stack([views[i]["world_mat"] for i in range(20)]), g["tyt20_world_mat"], rtol=0, atol=1e-12)
    assert selected == g["tyt20_mapped"].tolist() == (g["tyt20_selected"] // 2).tolist()
    assert len(set(selected)) < len(selected) or max(g["tyt20_selected"]) >= 2          # the mapping is not the identity here
    everything, _ = CS.select_views(path, "tyt", cluster=False)
    assert everything == [i // 2 for i in range(20)]                                   # duplicates included
    images = tmp_path / "images"
    images.mkdir()
    (images / "00003.jpg").write_bytes(b"x")
    (images / "000007.jpg").write_bytes(b"x")
    assert os.path.basename(CS.image_path(str(images), "tyt", 3)) == "00003.jpg"
    assert os.path.basename(CS.image_path(str(images), "tyt", 7)) == "000007.jpg"
    with pytest.raises(FileNotFoundError, match="00004.jpg"):
        CS.image_path(str(images), "tyt", 4)


def test_hidden_files_are_skipped(tmp_path):
    for name in (".DS_Store", "._0000.png", "0001.png", "0000.png", "0002.png"):
        (tmp_path / name).write_bytes(b"x")
    assert CS.list_images(str(tmp_path)) == ["0000.png", "0001.png", "0002.png"]
    assert os.path.basename(CS.image_path(str(tmp_path), "dtu", 1)) == "0001.png"
    with pytest.raises(FileNotFoundError, match="view 3"):
        CS.image_path(str(tmp_path), "nerf", 3)


def test_refusals():
    views = KC.views_of("dome8")
    with pytest.raises(ValueError, match="ascending"):
        CS.camera_centres_dirs({k: views[k] for k in (1, 0, 2, 3, 4)})
    with pytest.raises(ValueError, match="ascending"):
        CS.camera_centres_dirs({k + 1: v for k, v in views.items()})
    with pytest.raises(ValueError, match="neither c2w nor world_mat"):
        CS.camera_centres_dirs({0: {"camera_mat": np.eye(4)}})
    with pytest.raises(ValueError, match="at least 4 cameras"):
        CS.select_representative_cameras({k: views[k] for k in range(3)})
    with pytest.raises(ValueError, match="does not fit"):
        CS.select_representative_cameras(views, max_cameras=9)
    with pytest.raises(_lib.GsrError, match="lloyd_batch_host"):
        CS.lloyd_batch(KC.cloud(8, 0), np.zeros((1, 16, 3)), [3], 0.0, device=None)
    c2w = {i: {"c2w": np.linalg.inv(v["world_mat"]), "world_mat": np.eye(4)} for i, v in views.items()}      # c2w comes first
    assert CS.select_representative_cameras(c2w)["selected_indices"] == KC.golden()["dome8_selected"].tolist()


def test_load_cameras_moved_and_is_re_exported():
    from gaussmart_amd import segment_cli
    assert segment_cli.load_cameras is CS.load_cameras and segment_cli.TYT_IMG_WH == CS.TYT_IMG_WH == (979, 543)


def test_header_declares_the_kernel_under_abi_18():
    text = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert re.search(r"#define GSR_ABI_VERSION 18\b", text) and _lib.ABI_VERSION == 18
    assert re.search(r"int32_t gsr_cam_lloyd\(const double\* x, int32_t n,", text) and "gsr_cam_lloyd_workspace_bytes(int32_t n, int32_t n_fits)" in text
    assert "CK_LLOYD" in text
    for name, value in (("GSR_CK_KMAX", 16), ("GSR_CK_CHUNK", 64), ("GSR_CK_MAX_CAMERAS", _lib.GSR_CK_MAX_CAMERAS)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value == getattr(_lib, name)
    assert _lib.GSR_CK_MAX_CAMERAS >= 4096 and _lib.GSR_CK_MAX_CAMERAS * 24 <= 96 * 1024
    makefile = open(os.path.join(ROOT, "gaussmart_amd", "csrc", "Makefile")).read()
    assert "cam_cluster.hip" in makefile and re.search(r"\$\(BUILD\)/cam_cluster\.o: EXTRA := -ffp-contract=off", makefile)
    L = _lib.lib()
    assert L.gsr_abi_version() == 18 and L.gsr_cam_lloyd_workspace_bytes(300, 130) == 0
    # refused before anything is launched: no device is needed to see it
    for kw, rc in ((dict(n=0), -1), (dict(n=_lib.GSR_CK_MAX_CAMERAS + 1), -4), (dict(fits=-1), -1), (dict(max_iter=0), -1),
                   (dict(tol=-1.0), -1), (dict(tol=float("nan")), -1), (dict(ptr=None), -1)):
        a = dict(n=8, fits=1, max_iter=300, tol=0.0, ptr=8)
        a.update(kw)
        assert L.gsr_cam_lloyd(a["ptr"], a["n"], 8, 8, a["fits"], a["tol"], a["max_iter"], 8, 8, 8, 8, 8, None, 0, None) == rc, kw
    assert L.gsr_cam_lloyd(8, _lib.GSR_CK_MAX_CAMERAS + 1, 8, 8, 1, 0.0, 300, 8, 8, 8, 8, 8, None, 0, None) == -4
    assert "lloyd_batch_host" in L.gsr_last_error().decode()


def test_identify_cli_on_the_host(tmp_path, capsys):
    from gaussmart_amd import identify_cli, segment_init as SI
    scan, out = str(tmp_path / "scan"), str(tmp_path / "out")
    pts = KC.scan8(scan)
    argv = ["-s", scan, "-o", out, "-t", "dtu", "--host"]
    identify_cli.main(argv, generator=KC.StubGenerator())
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l.get("step") for l in lines] == [1, 2, 3, 4, 5, None] and all(l["ms"] >= 0 for l in lines[:5])
    want = KC.golden()["dome8_selected"].tolist()
    assert lines[-1]["selected_views"] == want and lines[0]["best_k"] == 4 and lines[-1]["images"] == [f"{i:04d}.png" for i in want]
    base = os.path.join(out, "segments")
    assert sorted(os.listdir(base)) == ["cameras", "embeddings", "images", "masks", "point_cloud"]
    assert sorted(os.listdir(os.path.join(base, "images"))) == sorted(f"{i:04d}.png" for i in want)
    assert sorted(os.listdir(os.path.join(base, "masks"))) == [f"segments_{k:03d}.npz" for k in range(4)]
    assert sorted(os.listdir(os.path.join(base, "point_cloud"))) == ["mask_areas.npy", "raw_pc.ply", "segment_indices.npy", "segmented_point_cloud.ply"]
    assert os.listdir(os.path.join(base, "embeddings")) == []
    with np.load(os.path.join(base, "cameras", "selected_cameras.npz"), allow_pickle=True) as z:
        assert sorted(z.files) == ["cameras_dict", "selected_indices"] and z["selected_indices"].tolist() == want
        cams = z["cameras_dict"].item()
    all_cams = CS.load_cameras(os.path.join(scan, "cameras.npz"), "dtu")
    assert list(cams) == [f"camera_{k:03d}" for k in range(4)]
    for k, i in enumerate(want):
        assert set(cams[f"camera_{k:03d}"]) == {"world_mat", "camera_mat", "scale_mat"}
        assert np.array_equal(cams[f"camera_{k:03d}"]["world_mat"], all_cams[i]["world_mat"])
    # the labels are those of the twins on the same masks, first view first
    from PIL import Image
    stub = KC.StubGenerator()
    masks = [stub.generate_segments(np.asarray(Image.open(os.path.join(scan, "images", f"{i:04d}.png")).convert("RGB")))[1]["masks"] for i in want]
    labels, areas = SI.label_points_host(pts, [all_cams[i] for i in want], "dtu", masks)
    got = np.load(os.path.join(base, "point_cloud", "segment_indices.npy"))
    assert got.dtype == np.int64 and np.array_equal(got, labels) and (got >= 0).sum() > 100
    assert np.load(os.path.join(base, "point_cloud", "mask_areas.npy"), allow_pickle=True).item() == areas
    with np.load(os.path.join(base, "masks", "segments_002.npz")) as z:
        assert np.array_equal(z["masks"], masks[2]) and z["masks"].dtype == bool and z["boxes"].shape == (3, 4) and z["areas"].dtype == np.int64
    # an existing tree is refused, and left alone, without --overwrite
    marker = os.path.join(base, "images", "keep.txt")
    open(marker, "w").close()
    with pytest.raises(SystemExit, match="--overwrite"):
        identify_cli.main(argv, generator=KC.StubGenerator())
    assert os.path.exists(marker)
    identify_cli.main(argv + ["--overwrite", "--skip_camera_clustering", "--clean"], generator=KC.StubGenerator())
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert not os.path.exists(marker) and lines[-1]["selected_views"] == list(range(8)) and lines[0]["best_k"] is None
    assert lines[2]["clean"] and lines[2]["points"] <= lines[2]["points_in"] == 300


def test_identify_cli_refuses_too_few_cameras_and_a_missing_image(tmp_path):
    from gaussmart_amd import identify_cli
    scan, out = str(tmp_path / "scan"), str(tmp_path / "out")
    KC.scan8(scan)
    os.remove(os.path.join(scan, "images", "0007.png"))                  # view 7 is selected and now has no picture
    with pytest.raises(SystemExit, match="view 7 has no image"):
        identify_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--host"], generator=KC.StubGenerator())
    assert not os.path.exists(os.path.join(out, "segments"))
    with np.load(os.path.join(scan, "cameras.npz")) as z:
        three = {k: z[k] for k in z.files if int(k.rsplit("_", 1)[1]) < 3}
    np.savez(os.path.join(scan, "cameras.npz"), **three)
    with pytest.raises(SystemExit, match="at least 4 cameras"):
        identify_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--host"], generator=KC.StubGenerator())
    with pytest.raises(SystemExit, match="--sam_checkpoint is required"):
        identify_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--host", "--skip_camera_clustering"])
