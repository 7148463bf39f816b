"""csrc/cam_cluster.hip on the device: gsr_cam_lloyd against its numpy twin BIT FOR BIT (labels, centres, inertia, n_iter,
status) at the shapes where its paths part (one chunk, a chunk boundary, several chunks, the cap, many fits of mixed k, ties, an
empty cluster, the final relabelling), the view selection against the twin and the reference's golden file, and
gaussmart_amd.identify_cli against sam_cli followed by segment_cli on the views it selected, and train_cli --run_segmentation."""
import json
import os

import numpy as np
import pytest

import camera_select_cases as KC
from gaussmart_amd import _lib
from gaussmart_amd import camera_select as CS

pytestmark = pytest.mark.gpu
CAP = _lib.GSR_CK_MAX_CAMERAS


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(X, c0, ks, tol, dev, max_iter=300):
    got = CS.lloyd_batch(X, c0, ks, tol, max_iter, device=dev)
    want = CS.lloyd_batch_host(X, c0, ks, tol, max_iter)
    for key in ("status", "n_iter", "labels", "centres", "inertia"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, got[key], want[key])
    return got


@pytest.mark.parametrize("n,ks", [(4, [3, 4]), (7, [3, 4, 7]), (63, [15]), (64, [15]), (65, [15]), (257, [15, 16, 1])])
def test_lloyd_equals_the_twin_bit_for_bit(gpu_device, n, ks):
    X = KC.cloud(n, n)
    got = same_bits(X, KC.inits(X, ks), ks, KC.tolerance(X), gpu_device)
    assert (got["status"] == 0).all() and (got["n_iter"] >= 1).all()
    for f, k in enumerate(ks):
        assert set(got["labels"][f]) == set(range(k)) and (got["centres"][f, k:] == 0).all()
    if n == 4:      # k = 4: every point is its own cluster and nothing is left over
        assert sorted(got["labels"][1]) == [0, 1, 2, 3] and got["inertia"][1] == 0.0 and got["inertia"][0] > 0.0


def test_lloyd_at_the_cap_and_past_it(gpu_device):
    X = KC.cloud(CAP, 5)
    ks = [16, 3]
    got = same_bits(X, KC.inits(X, ks), ks, KC.tolerance(X), gpu_device)
    assert (got["status"] == 0).all() and set(got["labels"][0]) == set(range(16))
    X1 = KC.cloud(CAP + 1, 6)
    with pytest.raises(_lib.GsrError, match="lloyd_batch_host"):
        CS.lloyd_batch(X1, KC.inits(X1, [3]), [3], KC.tolerance(X1), device=gpu_device)
    # the Python layer takes the twin there by itself
    assert not CS._use_device(gpu_device, CAP + 1, [3]) and CS._use_device(gpu_device, CAP, [16]) and not CS._use_device(gpu_device, 8, [17])


def test_one_launch_of_130_fits_and_a_single_fit(gpu_device):
    X = KC.cloud(120, 9)
    ks = [k for k in range(3, 16) for _ in range(10)]
    c0 = KC.inits(X, ks)
    many = same_bits(X, c0, ks, KC.tolerance(X), gpu_device)
    assert len(ks) == 130 and len(set(many["n_iter"].tolist())) > 3                 # the fits end at different iterations
    one = same_bits(X, c0[77:78], ks[77:78], KC.tolerance(X), gpu_device)
    for key in one:
        assert np.array_equal(bits(one[key][0]), bits(many[key][77])), key          # a fit does not depend on its neighbours


def test_ties_go_to_the_lowest_cluster(gpu_device):
    X = np.array([[-1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [0, 1.0, 0]])            # the last two: alike, and as far from either centre
    c0 = np.zeros((1, 16, 3))
    c0[0, 0], c0[0, 1] = (-1.0, 0, 0), (1.0, 0, 0)
    got = same_bits(X, c0, [2], 0.0, gpu_device)
    assert got["labels"][0].tolist() == [0, 1, 0, 0] and got["status"][0] == 0


def test_an_empty_cluster_ends_the_fit_with_status_one(gpu_device):
    X = KC.cloud(65, 1)
    c0 = KC.inits(X, [3, 3])
    c0[0, 2] = 1e6                                      # no point is nearest to it
    got = same_bits(X, c0, [3, 3], KC.tolerance(X), gpu_device)
    assert got["status"].tolist() == [1, 0] and got["n_iter"][0] == 1 and np.array_equal(got["centres"][0], c0[0])
    assert set(got["labels"][0]) == {0, 1}
    # the Python layer redoes it on the host with scikit-learn's relocation; k outside 1 .. 16 is status 2
    bad = same_bits(X, c0, [0, 17], KC.tolerance(X), gpu_device)
    assert bad["status"].tolist() == [2, 2] and (bad["labels"] == -1).all()


def test_max_iter_one_relabels_against_the_final_centres(gpu_device):
    X = KC.cloud(257, 2)
    ks = [5, 15]
    c0 = KC.inits(X, ks)
    got = same_bits(X, c0, ks, KC.tolerance(X), gpu_device, max_iter=1)
    assert got["n_iter"].tolist() == [1, 1]
    first = np.argmin(CS._sqdist(X, c0[0, :5]), axis=1)
    assert not np.array_equal(got["labels"][0], first)                              # labelled again, against the moved centres
    assert np.array_equal(got["labels"][0], np.argmin(CS._sqdist(X, got["centres"][0, :5]), axis=1))
    two = same_bits(X, c0, ks, 1e30, gpu_device)                                    # the tolerance stop takes the same path
    assert two["n_iter"].tolist() == [1, 1] and np.array_equal(two["labels"], got["labels"])


@pytest.mark.parametrize("name", KC.SETS)
def test_selection_on_the_device_equals_twin_and_reference(gpu_device, name):
    g, host, dev = KC.golden(), {}, {}
    views = KC.views_of(name)
    want = CS.select_representative_cameras(views, details=host)
    got = CS.select_representative_cameras(views, device=gpu_device, details=dev)
    assert got == want and got["selected_indices"] == g[f"{name}_selected"].tolist()
    assert dev["best_k"] == host["best_k"] == int(g[f"{name}_best_k"]) and np.array_equal(dev["labels"], g[f"{name}_labels"])
    for k in host["fits"]:
        for a, b in zip(dev["fits"][k], host["fits"][k]):
            assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))), k
    assert dev["scores"] == host["scores"]


def same_file(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        return fa.read() == fb.read()


@pytest.mark.parametrize("sam2", (False, True), ids=("sam", "sam2-hip"))
def test_identify_cli_equals_sam_cli_then_segment_cli(gpu_device, tmp_path, capsys, sam2):
    from gaussmart_amd import identify_cli, sam_cli, segment_cli
    scan, out, two, ckpt = (str(tmp_path / d) for d in ("scan", "out", "two", "ckpt"))
    KC.scan8(scan)
    if sam2:
        import sam2_decoder_cases as K2
        from gaussmart_amd import sam2 as S2
        S2.save_sam2_weights(K2.weights("K1"), ckpt)
        flavour = ["--sam2", "--decoder", "hip"]
    else:
        import sam_decoder_cases as DC
        from gaussmart_amd import sam as S
        S.save_sam_weights(DC.weights("D1"), ckpt)
        flavour = []
    sam_args = ["--sam_checkpoint", ckpt, "--points_per_side", "4", "--device", str(gpu_device), "--pred_iou_thresh", "-100",
                "--stability_score_thresh", "0.0"] + flavour
    identify_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--clean"] + sam_args)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    views = lines[-1]["selected_views"]
    assert views == KC.golden()["dome8_selected"].tolist() and [l.get("step") for l in lines] == [1, 2, 3, 4, 5, None]
    assert not lines[0]["host"] and all(v["masks"] > 0 for v in lines[1]["views"]) and lines[3]["labelled"] > 0
    sam_cli.main(["-s", scan, "-o", two, "--views"] + [str(v) for v in views] + sam_args)
    segment_cli.main(["-s", scan, "-o", two, "-t", "dtu", "--clean", "--masks", os.path.join(two, "segments", "masks"), "--views"] +
                     [str(v) for v in views] + ["--device", str(gpu_device)])
    capsys.readouterr()
    # the .npz container carries its entries' time of writing; what it stores is compared byte for byte, entry by entry
    for k in range(len(views)):
        with np.load(os.path.join(out, "segments", "masks", f"segments_{k:03d}.npz")) as a, \
                np.load(os.path.join(two, "segments", "masks", f"segments_{k:03d}.npz")) as b:
            assert a.files == b.files == ["masks", "boxes", "areas"]
            for key in a.files:
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (k, key)
    for name in ("segment_indices.npy", "mask_areas.npy", "raw_pc.ply", "segmented_point_cloud.ply"):
        assert same_file(os.path.join(out, "segments", "point_cloud", name), os.path.join(two, "segments", "point_cloud", name)), name
    assert sorted(os.listdir(os.path.join(out, "segments", "images"))) == sorted(os.listdir(os.path.join(two, "segments", "images")))


def test_train_cli_run_segmentation(gpu_device, tmp_path, monkeypatch):
    """train.py --run_segmentation: the pipeline runs in-process into MODEL/segmentation before training, and the run trains from
    its labels (--segmentation_dir is set to the result).  The masks are the stub generator's: this is about the plumbing."""
    import torch
    from PIL import Image
    from gaussmart_amd import sam_cli, train_cli
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.params import PipelineParams
    from gaussmart_amd.scene_io import storePly
    from gaussmart_amd.synthetic import make_scene, jittered_cameras
    root, out = tmp_path / "scan", tmp_path / "model"
    pts = KC.scan8(str(root))                               # cameras.npz, images/, points.ply: what the identification reads
    os.makedirs(root / "train")
    W, H = 96, 64
    params, _ = make_scene(300, W, H, seed=3, radius_px=5.0)
    m = GaussianModel(3, device=gpu_device)
    m.create_from_params(params)
    frames = []
    for i, cam in enumerate(jittered_cameras(4, W, H, seed=3, device=gpu_device, amount=0.2)):
        with torch.no_grad():
            img = render(cam, m, PipelineParams(), torch.zeros(3, device=gpu_device), surface_maps=False)["render"].clamp(0, 1)
        rgba = np.concatenate([(img.permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], -1)
        Image.fromarray(rgba, "RGBA").save(root / "train" / f"r_{i}.png")
        c2w = np.linalg.inv(cam.world_view_transform.T.cpu().numpy().astype(np.float64))
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": c2w.tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.8, "frames": frames if split == "train" else []}, open(root / f"transforms_{split}.json", "w"))
    storePly(str(root / "points3d.ply"), params["xyz"].numpy(), np.full((300, 3), 128))     # what the training reads: as many points
    seen = {}

    def stub(args):
        seen.update(sam2=args.sam2, checkpoint=args.sam_checkpoint, device=args.device)
        return KC.StubGenerator(), None
    monkeypatch.setattr(sam_cli, "make_generator", stub)
    train_cli.main(["-s", str(root), "-m", str(out), "--iterations", "30", "--save_iterations", "30", "--log_every", "0",
                    "--run_segmentation", "--dataset_type", "dtu", "--sam2", "--clean", "--sam_checkpoint", "nowhere"])
    seg = out / "segmentation" / "segments"
    assert seen == dict(sam2=True, checkpoint="nowhere", device=str(gpu_device))
    with np.load(seg / "cameras" / "selected_cameras.npz", allow_pickle=True) as z:
        assert z["selected_indices"].tolist() == KC.golden()["dome8_selected"].tolist()
    labels = np.load(seg / "point_cloud" / "segment_indices.npy")
    assert 0 < len(labels) <= len(pts) and (labels >= 0).sum() > 50
    res = json.load(open(out / "results.json"))
    assert res["iterations"] == 30 and res["points"] >= len(labels)             # the cloud was cut to the labels (fetchPly), then augmented
    # a second run finds its own earlier tree and replaces it
    train_cli.main(["-s", str(root), "-m", str(out), "--iterations", "5", "--save_iterations", "5", "--log_every", "0",
                    "--run_segmentation", "--dataset_type", "dtu", "--skip_camera_clustering", "--sam_checkpoint", "nowhere"])
    with np.load(seg / "cameras" / "selected_cameras.npz", allow_pickle=True) as z:
        assert z["selected_indices"].tolist() == list(range(8))
