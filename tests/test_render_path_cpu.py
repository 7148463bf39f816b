"""The trajectory export without a GPU: the camera path against the reference's own functions (tests/golden/render_path.npz),
generate_path's cameras, the numpy twins of the u8 and turbo frames, the generated colour tables, the Motion-JPEG writer
and create_videos on a directory of synthetic frames."""
import io
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLDEN


# ---------------------------------------------------------------- 1. camera path
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "render_path.npz"))


def test_golden_reaches_both_branches(golden):
    br = np.stack([golden[f"branches_{k}"] for k in range(3)])
    assert [len(golden[f"c2ws_{k}"]) for k in range(3)] == [3, 12, 49]
    assert br[:, 0].any() and not br[:, 0].all(), "negative PCA determinant: one side only"
    assert br[:, 1].any() and not br[:, 1].all(), "y-flip: one side only"


@pytest.mark.parametrize("k", [0, 1, 2])
def test_path_matches_reference(golden, k):
    from gaussmart_amd.render_path import generate_ellipse_path, pad_poses, path_c2ws, transform_poses_pca, unpad_poses
    c2ws = golden[f"c2ws_{k}"]
    poses = c2ws[:, :3, :] @ np.diag([1, -1, -1, 1])
    recentered, transform = transform_poses_pca(poses)
    assert recentered.dtype == np.float64 and transform.shape == (4, 4)
    assert np.abs(recentered - golden[f"recentered_{k}"]).max() <= 1e-9
    assert np.abs(transform - golden[f"transform_{k}"]).max() <= 1e-9
    assert np.array_equal(unpad_poses(pad_poses(poses)), poses) and pad_poses(poses).shape == (len(poses), 4, 4)
    for frames in (8, 240):
        path = generate_ellipse_path(poses=recentered, n_frames=frames)
        assert path.shape == (frames, 3, 4)
        assert np.abs(path - golden[f"ellipse_{k}_{frames}"]).max() <= 1e-9
        warped = np.linalg.inv(transform) @ pad_poses(path)
        assert np.abs(warped - golden[f"warped_{k}_{frames}"]).max() <= 1e-9
        assert np.abs(path_c2ws(c2ws, frames) - golden[f"warped_{k}_{frames}"] @ np.diag([1, -1, -1, 1])).max() <= 1e-9


def test_normalize_and_viewmatrix():
    from gaussmart_amd.render_path import normalize, viewmatrix
    assert np.allclose(np.linalg.norm(normalize(np.array([3.0, 4.0, 12.0]))), 1.0, atol=1e-15)
    m = viewmatrix(np.array([0.0, 0.0, 2.0]), np.array([0.0, 1.0, 0.0]), np.array([1.0, 2.0, 3.0]))
    assert m.shape == (3, 4) and np.allclose(m, np.concatenate([np.eye(3), [[1.0], [2.0], [3.0]]], 1), atol=1e-15)


def test_generate_path_cameras():
    from gaussmart_amd.camera import look_at_camera
    from gaussmart_amd.render_path import generate_path
    rng = np.random.default_rng(3)
    cams = []
    for i in range(7):
        a = 2 * np.pi * i / 7
        eye = np.array([3 * np.cos(a), 3 * np.sin(a), 0.4 * rng.normal()])
        img = torch.rand(3, 95, 97) if i == 0 else None
        cams.append(look_at_camera(eye, (0, 0, 0), (0, 0, 1), np.radians(55), 97, 95, device="cpu", image=img, uid=i))
    before = {k: v.clone() for k, v in vars(cams[0]).items() if isinstance(v, torch.Tensor)}
    traj = generate_path(cams, 6, device="cpu")
    assert len(traj) == 6
    for cam in traj:
        assert (cam.image_width, cam.image_height) == (96, 94)
        assert cam.original_image is None and cam.gt_alpha_mask is None
        assert cam.FoVx == cams[0].FoVx and cam.FoVy == cams[0].FoVy
        w = cam.world_view_transform
        assert w.dtype == torch.float32 and w.shape == (4, 4)
        assert torch.equal(cam.full_proj_transform, w @ cams[0].projection_matrix)
        assert torch.equal(cam.camera_center, w.inverse()[3, :3])
        c2w = np.linalg.inv(w.T.numpy().astype(np.float64))
        assert np.allclose(c2w[:3, :3] @ c2w[:3, :3].T, np.eye(3), atol=1e-5), "the view matrix is not a rigid motion"
        assert np.allclose(c2w[:3, 3], cam.camera_center.numpy(), atol=1e-5)
        # the camera looks at the scene: its +z axis points from its centre towards the origin the cameras surround
        to_origin = -c2w[:3, 3] / np.linalg.norm(c2w[:3, 3])
        assert c2w[:3, 2] @ to_origin > 0.95
    # camera 0 is not modified
    assert cams[0].original_image is not None and (cams[0].image_width, cams[0].image_height) == (97, 95)
    for k, v in before.items():
        assert torch.equal(getattr(cams[0], k), v), k
    assert len({tuple(c.camera_center.tolist()) for c in traj}) == 6


# ---------------------------------------------------------------- 2. u8 and turbo twins
def _depth_frame():
    rng = np.random.default_rng(1)
    d = rng.uniform(2.0, 4.0, (131, 257)).astype(np.float32)
    d[rng.integers(0, 131, 40), rng.integers(0, 257, 40)] = 0.0
    d[5, 7], d[60, 200] = np.nan, np.inf
    return d


def test_to_u8_host_is_save_img_u8():
    from gaussmart_amd.frames import to_u8_host
    rng = np.random.default_rng(0)
    img = rng.uniform(-0.5, 1.5, (3, 9, 13)).astype(np.float32)
    k = (np.arange(256, dtype=np.float32) / np.float32(255))
    edge = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                           np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)])
    img.reshape(-1)[:len(edge)] = edge[:img.size]
    hwc = np.moveaxis(img, 0, -1)
    want = (np.clip(np.nan_to_num(hwc), 0.0, 1.0) * 255.0).astype(np.uint8)       # mesh._save_img_u8's expression
    got = to_u8_host(img)
    assert got.dtype == np.uint8 and got.shape == (9, 13, 3) and np.array_equal(got, want)
    assert np.array_equal(to_u8_host(torch.from_numpy(img)[None])[0], want)


def test_depth_to_turbo_host_is_create_videos_expression():
    matplotlib = pytest.importorskip("matplotlib")
    from gaussmart_amd.frames import depth_limits_host, depth_to_turbo_host
    d = _depth_frame()
    clean, frame = depth_to_turbo_host(d, *depth_limits_host(d))
    # utils/render_utils.py:215-221 and 262-266, with this machine's numpy and matplotlib
    depth_frame = np.nan_to_num(d).astype(np.float32)          # what save_img_f32 wrote and load_img reads
    assert clean.dtype == np.float32 and np.array_equal(clean, depth_frame)
    distance_limits = np.percentile(depth_frame.flatten(), [3, 97])
    lo, hi = [np.log(x) for x in distance_limits]
    assert (lo, hi) == depth_limits_host(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        img = np.log(depth_frame)
        img = np.clip((img - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1)
    assert img.dtype == np.float64, "numpy 2 promotes the normalisation through the float64 limits"
    img = matplotlib.colormaps["turbo"](img)[..., :3]
    want = (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)
    assert frame.dtype == np.uint8 and frame.shape == (131, 257, 3) and np.array_equal(frame, want)
    # zeros and the NaN (cleaned to 0) sit at the lower end of the table, the cleaned inf at the upper
    from gaussmart_amd.colormaps import turbo_u8
    assert np.array_equal(frame[5, 7], turbo_u8()[0]) and np.array_equal(frame[60, 200], turbo_u8()[255])
    assert (frame[d == 0] == turbo_u8()[0]).all()


def test_fp32_log_picks_the_fp64_bins():
    """The float32 log of the twin and a float64 evaluation of the same formula choose the same table row at every pixel of
    the 131 x 257 frame: a last-bit difference of the log moves t by ~1e-7 of a bin 1/256 wide."""
    from gaussmart_amd.frames import depth_limits_host, depth_turbo_index_host
    d = _depth_frame()
    lo, hi = depth_limits_host(d)
    i32, i64 = depth_turbo_index_host(d, lo, hi)[1], depth_turbo_index_host(d, lo, hi, log_dtype=np.float64)[1]
    assert np.array_equal(i32, i64) and i32.min() == 0 and i32.max() == 255


def test_depth_to_turbo_host_degenerate_limits():
    matplotlib = pytest.importorskip("matplotlib")
    from gaussmart_amd.frames import depth_to_turbo_host
    d = np.array([[3.0, 3.0, 2.0, 4.0, 0.0, -1.0]], np.float32)
    lo = hi = float(np.log(np.float32(3.0)))
    _, frame = depth_to_turbo_host(d, lo, hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip((np.log(d) - np.minimum(np.float64(lo), np.float64(hi))) / np.abs(np.float64(hi) - np.float64(lo)), 0, 1)
    want = (np.clip(np.nan_to_num(matplotlib.colormaps["turbo"](t)[..., :3]), 0., 1.) * 255.).astype(np.uint8)
    assert np.array_equal(frame, want)
    assert not frame[0, 0].any() and not frame[0, 5].any(), "0 / 0 and the log of a negative depth are black"


def test_colormap_tables_are_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    from gaussmart_amd import colormaps
    colors = np.asarray(matplotlib.colormaps["turbo"].colors, np.float64)
    assert np.array_equal(np.asarray(colormaps.TURBO, np.float64), colors)
    assert np.array_equal(colormaps.turbo_f32(), colors.astype(np.float32)) and colormaps.turbo_f32().dtype == np.float32
    assert np.array_equal(colormaps.turbo_u8(), (colors * 255.).astype(np.uint8)) and colormaps.turbo_u8().dtype == np.uint8
    assert np.array_equal(matplotlib.colormaps["turbo"](np.arange(256))[:, :3], colors)


def test_colormap_tables_are_consistent():
    from gaussmart_amd import colormaps
    t = np.asarray(colormaps.TURBO, np.float64)
    assert t.shape == (256, 3) and t.min() >= 0 and t.max() <= 1
    assert np.array_equal(colormaps.turbo_u8(), (t * 255.).astype(np.uint8))


def test_gradient_and_colormap_hosts():
    from gaussmart_amd.frames import colormap_host, gradient_map_host
    from gaussmart_amd import colormaps
    img = torch.zeros(3, 5, 6)
    img[:, :, 3:] = 1.0                                    # a vertical step: |gx| = 1 on both sides of it and at the zero-padded border
    g = gradient_map_host(img)
    assert g.shape == (1, 5, 6)
    assert torch.allclose(g[0, 2], torch.tensor([0.0, 0, 1, 1, 0, 1]) * 3 ** 0.5, atol=1e-6)
    m = torch.linspace(0, 1, 30).reshape(1, 5, 6)
    c = colormap_host(m)
    table = torch.from_numpy(colormaps.turbo_f32())
    assert c.shape == (3, 5, 6) and torch.equal(c[:, 0, 0], table[0]) and torch.equal(c[:, 4, 5], table[255])
    assert torch.equal(colormap_host(torch.full((1, 4, 4), 2.5)), table[0].reshape(3, 1, 1).expand(3, 4, 4))


# ---------------------------------------------------------------- 3. Motion-JPEG AVI
def read_avi(path):
    """A RIFF reader for what MJPEGWriter writes: {'avih', 'strh', 'strf', 'frames' (the 00dc payloads), 'idx1'}."""
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out = {"frames": [], "offsets": []}

    def walk(lo, hi, movi_at=None):
        p = lo
        while p < hi:
            cid, size = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
            body = p + 8
            if cid == b"LIST":
                kind = data[body:body + 4]
                walk(body + 4, body + size, movi_at=body if kind == b"movi" else None)
            elif cid == b"00dc":
                out["frames"].append(data[body:body + size])
                out["offsets"].append((p - movi_at, size))
            else:
                out[cid.decode()] = data[body:body + size]
            p = body + size + size % 2
        assert p == hi, "a chunk runs past its list"

    walk(12, len(data))
    return out


def avi_info(path):
    r = read_avi(path)
    avih = struct.unpack("<14I", r["avih"])
    assert r["strh"][:8] == b"vidsMJPG"
    strh = struct.unpack("<IHHIIIIIIII4H", r["strh"][8:])
    strf = struct.unpack("<IiiHH4sIiiII", r["strf"])
    idx = [struct.unpack("<4sIII", r["idx1"][i:i + 16]) for i in range(0, len(r["idx1"]), 16)]
    assert [(o, s) for _, _, o, s in idx] == r["offsets"] and all(c == b"00dc" for c, _, _, _ in idx)
    return {"frames": r["frames"], "total_frames": avih[4], "streams": avih[6], "width": avih[8], "height": avih[9],
            "usec_per_frame": avih[0], "scale": strh[4], "rate": strh[5], "length": strh[7], "bi_width": strf[1],
            "bi_height": strf[2], "compression": strf[5]}


def _pil_jpeg(frame, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


@pytest.mark.parametrize("quality,fps", [(95, 60), (70, 24)])
def test_mjpeg_writer(tmp_path, quality, fps):
    from gaussmart_amd.video import MJPEGWriter
    rng = np.random.default_rng(quality)
    frames = [rng.integers(0, 256, (34, 50, 3), dtype=np.uint8) for _ in range(5)]
    frames.append(np.full((34, 50, 3), 77, np.uint8))      # a flat frame: a short chunk, odd or even
    path = tmp_path / "v.avi"
    with MJPEGWriter(str(path), (34, 50), fps=fps, quality=quality) as w:
        for f in frames:
            w.add_image(f)
        assert w.num_frames == 6
    info = avi_info(str(path))
    assert info["total_frames"] == info["length"] == len(info["frames"]) == 6 and info["streams"] == 1
    assert (info["width"], info["height"], info["bi_width"], info["bi_height"]) == (50, 34, 50, 34)
    assert (info["scale"], info["rate"], info["usec_per_frame"]) == (1, fps, 1000000 // fps)
    assert info["compression"] == b"MJPG"
    for got, f in zip(info["frames"], frames):
        assert got == _pil_jpeg(f, quality)
    with pytest.raises(ValueError, match="frame is"):
        with MJPEGWriter(str(tmp_path / "w.avi"), (34, 50)) as w:
            w.add_image(np.zeros((10, 10, 3), np.uint8))


# ---------------------------------------------------------------- 4. create_videos
def test_create_videos_from_files(tmp_path, capsys):
    from PIL import Image
    from gaussmart_amd.frames import depth_limits_host, depth_to_turbo_host
    from gaussmart_amd.video import create_videos
    rng = np.random.default_rng(2)
    src = tmp_path / "in"
    (src / "renders").mkdir(parents=True)
    (src / "vis").mkdir()
    colours, depths = [], []
    for i in range(6):
        c = rng.integers(0, 256, (20, 28, 3), dtype=np.uint8)
        d = rng.uniform(2.0, 4.0, (20, 28)).astype(np.float32)
        d[i, i] = 0.0
        Image.fromarray(c).save(src / "renders" / f"{i:05d}.png", "PNG")
        Image.fromarray(d).save(src / "vis" / f"depth_{i:05d}.tiff", "TIFF")
        colours.append(c)
        depths.append(d)
    out = tmp_path / "out"
    create_videos(base_dir=str(out), input_dir=str(src), out_name="render_traj", num_frames=6)
    text = capsys.readouterr().out
    assert "Images missing for tag normal" in text and "Video shape is (20, 28)" in text
    assert sorted(p.name for p in out.iterdir()) == ["render_traj_color.avi", "render_traj_depth.avi"]
    colour, depth = avi_info(str(out / "render_traj_color.avi")), avi_info(str(out / "render_traj_depth.avi"))
    lo, hi = depth_limits_host(depths[0])
    for info in (colour, depth):
        assert info["total_frames"] == len(info["frames"]) == 6 and info["rate"] == 60
        assert (info["width"], info["height"]) == (28, 20)
    for i in range(6):
        assert colour["frames"][i] == _pil_jpeg(colours[i], 95)
        assert depth["frames"][i] == _pil_jpeg(depth_to_turbo_host(depths[i], lo, hi)[1], 95)
