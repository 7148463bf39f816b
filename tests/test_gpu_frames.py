"""Frame kernels (gsr_frame_*) against their host twins, the device and the host route of export_image / export_trajectory,
and `render_cli --render_path`."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import frames_ref
from test_gpu_mesh import DEV, _fib, _look_at_w2c, _sphere_cams, _sphere_model
from test_render_path_cpu import avi_info

pytestmark = pytest.mark.gpu

SHAPES_HW = [(1, 1), (3, 5), (16, 64), (33, 257)]


def _edge_values():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.concatenate([np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), k, np.nextafter(k, np.float32(2)),
                           np.nextafter(k, np.float32(-1))])


# ---------------------------------------------------------------- to_u8
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (1, 3, 3, 5), (2, 3, 7, 64), (1, 1, 5, 8), (3, 4, 2, 4), (1, 3, 33, 257)])
def test_to_u8_is_the_host_expression(shape):
    """Vector path (W % 4 == 0) and scalar path, a tail, several workgroups, B > 1; every k / 255 with both neighbours,
    NaN, +-inf and -0 wherever they fit (all of them on (2,3,7,64), vector, and (1,3,33,257), scalar)."""
    from gaussmart_amd.frames import to_u8, to_u8_host
    rng = np.random.default_rng(sum(shape))
    x = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
    e = _edge_values()
    x.reshape(-1)[:len(e)] = e[:x.size]
    if x.size > 2 * len(e):
        x.reshape(-1)[-len(e):] = e                    # the same values again at other lanes and bytes of the dwords
    got = to_u8(torch.from_numpy(x).to(DEV))
    want = to_u8_host(x)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0], shape[2], shape[3], shape[1])
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(to_u8(torch.from_numpy(x[0]).to(DEV)).cpu().numpy(), want[0])
    assert np.array_equal(want, (np.clip(np.nan_to_num(np.moveaxis(x, 1, -1)), 0.0, 1.0) * 255.0).astype(np.uint8))


def test_to_u8_refuses_host_tensors_and_odd_channels():
    from gaussmart_amd import _lib
    from gaussmart_amd.frames import to_u8
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        to_u8(torch.zeros(3, 4, 4))
    with pytest.raises(_lib.GsrError, match="channels must be 1, 3 or 4"):
        to_u8(torch.zeros(2, 4, 4, device=DEV))


# ---------------------------------------------------------------- order statistics
def _stats_values(n):
    rng = np.random.default_rng(n)
    x = rng.uniform(2.0, 4.0, n).astype(np.float32)
    if n >= 255:
        x[rng.integers(0, n, n // 8)] = x[rng.integers(0, n, n // 8)]      # duplicates
        x[rng.integers(0, n, n // 20)] = 0.0
        x[rng.integers(0, n, n // 30)] = -rng.uniform(0.0, 3.0, n // 30).astype(np.float32)
        x[n // 2], x[n // 3], x[n // 5] = np.nan, np.inf, -np.inf
    return x


@pytest.mark.parametrize("n", [1, 2, 255, 257, 131 * 257])
def test_order_stats_are_the_sorted_elements(n):
    from gaussmart_amd.frames import order_stats
    x = _stats_values(n)
    srt = np.sort(np.nan_to_num(x))
    for ranks in ([0], [n - 1, 0], [0, n // 3, n // 2, n - 1], list(np.linspace(0, n - 1, 8).astype(int))):
        got = order_stats(torch.from_numpy(x).to(DEV), ranks)
        assert got.dtype == np.float32 and np.array_equal(got, srt[ranks]), (ranks, got, srt[ranks])


@pytest.mark.parametrize("n", [1, 2, 255, 257, 131 * 257])
def test_depth_limits_are_numpys_percentiles(n):
    from gaussmart_amd.frames import depth_limits, depth_limits_host
    x = np.abs(_stats_values(n))          # depth: zeros, duplicates, a NaN and an inf, nothing negative
    with np.errstate(divide="ignore"):
        want = np.log(np.percentile(np.nan_to_num(x), [3, 97]))
    got = depth_limits(torch.from_numpy(x).to(DEV).reshape(1, 1, -1), p=3)
    print(f"depth_limits n={n}: device {got}, numpy {tuple(want)}")
    np.testing.assert_allclose(np.array(got), want, rtol=1e-12, atol=0)
    assert got == depth_limits_host(x)


def test_order_stats_arguments():
    from gaussmart_amd import _lib
    from gaussmart_amd.frames import order_stats
    x = torch.arange(10, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.GsrError, match="outside"):
        order_stats(x, [10])
    with pytest.raises(_lib.GsrError, match="k must be"):
        order_stats(x, list(range(9)))


# ---------------------------------------------------------------- depth frame
def _depth(h, w, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(2.0, 4.0, (h, w)).astype(np.float32)
    n = h * w
    d.reshape(-1)[rng.choice(n, max(2, n // 50), replace=False)] = 0.0
    d.reshape(-1)[n // 2], d.reshape(-1)[n // 3] = np.nan, np.inf
    return d


def check_depth_frame(frame, d, lo, hi):
    """The depth_vis condition: black exactly where the twin is black; elsewhere the twin's table row, or a neighbouring
    row at no more than 1e-3 of the pixels.  Returns the share of pixels on a neighbouring row."""
    from gaussmart_amd.colormaps import turbo_u8
    from gaussmart_amd.frames import depth_turbo_index_host
    _, idx = depth_turbo_index_host(d, lo, hi)
    tab = turbo_u8()
    bad = idx < 0
    assert not frame[bad].any(), "a NaN pixel is not black"
    i = idx[~bad]
    f = frame[~bad]
    same = (f == tab[i]).all(-1)
    near = (f == tab[np.minimum(i + 1, 255)]).all(-1) | (f == tab[np.maximum(i - 1, 0)]).all(-1)
    assert (same | near).all(), f"{int((~(same | near)).sum())} pixels are more than one table row away"
    share = float((~same).mean()) if same.size else 0.0
    assert share <= 1e-3, share
    return share


@pytest.mark.parametrize("h,w", [(3, 5), (7, 64), (131, 257)])
def test_depth_vis(h, w):
    """Measured on the MI355X: no pixel of any of the three frames (nor of the constant one below) left the twin's table
    row, share 0.0 (expected order 256 * 2^-24 * |log d| / |hi - lo| ~ 2e-5 of the pixels)."""
    from gaussmart_amd.frames import depth_limits_host, depth_to_turbo, depth_to_turbo_host
    d = _depth(h, w, h * w)
    lo, hi = depth_limits_host(d)
    for shape in ((1, 1, h, w), (h, w)):
        clean, frame = depth_to_turbo(torch.from_numpy(d).to(DEV).reshape(shape), lo, hi)
        assert clean.dtype == torch.float32 and tuple(clean.shape) == shape
        assert tuple(frame.shape) == ((1, h, w, 3) if len(shape) == 4 else (h, w, 3)) and frame.dtype == torch.uint8
        assert np.array_equal(clean.cpu().numpy().reshape(h, w).view(np.uint32), np.nan_to_num(d).view(np.uint32))
        share = check_depth_frame(frame.cpu().numpy().reshape(h, w, 3), d, lo, hi)
        print(f"depth_vis {h}x{w}: share of pixels one table row off {share:.2e}")
    # the limits the other way round give the same frame; without the cleaned depth too
    none, swapped = depth_to_turbo(torch.from_numpy(d).to(DEV), hi, lo, want_clean=False)
    assert none is None and torch.equal(swapped, frame)
    assert np.array_equal(depth_to_turbo_host(d, lo, hi)[1], depth_to_turbo_host(d, hi, lo)[1])


def test_depth_vis_batch_and_constant_frame():
    from gaussmart_amd.frames import clean_depth, depth_limits, depth_to_turbo, depth_to_turbo_host
    d = np.stack([_depth(7, 9, s) for s in range(3)])[:, None]
    lo, hi = math.log(2.2), math.log(3.7)
    clean, frame = depth_to_turbo(torch.from_numpy(d).to(DEV), lo, hi)
    assert tuple(frame.shape) == (3, 7, 9, 3)
    for b in range(3):
        check_depth_frame(frame[b].cpu().numpy(), d[b, 0], lo, hi)
    assert np.array_equal(clean_depth(torch.from_numpy(d).to(DEV)).cpu().numpy().view(np.uint32),
                          np.nan_to_num(d).view(np.uint32))
    # hi == lo: (log d - lo) / 0 is +-inf or NaN, as numpy gives it.  The constant is 1: its log is exactly 0 in float32 and
    # in float64, so every constant pixel is 0 / 0 whatever the last bit of a log function (at any other constant the sign
    # of logf(d) - log(d) would pick the first or the last table row)
    c = np.full((5, 8), 1.0, np.float32)
    c[0, :4] = [2.0, 4.0, 0.0, -1.0]
    lim = depth_limits(torch.from_numpy(np.full((5, 8), 1.0, np.float32)).to(DEV))
    assert lim == (0.0, 0.0)
    _, frame = depth_to_turbo(torch.from_numpy(c).to(DEV), *lim)
    assert np.array_equal(frame.cpu().numpy(), depth_to_turbo_host(c, *lim)[1])
    assert not frame[1:].any() and not frame[0, 3].any() and frame[0, 0].any() and frame[0, 1].any()


# ---------------------------------------------------------------- gradient_map
@pytest.mark.parametrize("hw", SHAPES_HW)
@pytest.mark.parametrize("channels", [1, 3])
def test_gradient_map(channels, hw):
    """Bitwise the numpy restatement in the kernel's order (tests/frames_ref.py); within 4e-6 of torch's conv2d: five
    roundings of partial sums <= 1 per response, two summation orders, sqrt(2) for the magnitude and sqrt(3) for the channel
    norm come to ~1.5e-6."""
    from gaussmart_amd.frames import gradient_map, gradient_map_host
    x = np.random.default_rng(channels * 1000 + hw[1]).uniform(0.0, 1.0, (channels,) + hw).astype(np.float32)
    got = gradient_map(torch.from_numpy(x).to(DEV))
    assert tuple(got.shape) == (1,) + hw and got.dtype == torch.float32
    g = got.cpu().numpy()
    assert np.array_equal(g.view(np.uint32), frames_ref.sobel_ordered(x).view(np.uint32))
    err = float((got.cpu() - gradient_map_host(torch.from_numpy(x))).abs().max())
    print(f"gradient_map C={channels} {hw}: max |device - conv2d| {err:.2e}")
    assert err <= 4e-6


# ---------------------------------------------------------------- colormap
@pytest.mark.parametrize("hw", SHAPES_HW)
def test_colormap(hw):
    from gaussmart_amd.frames import colormap, colormap_host
    rng = np.random.default_rng(hw[1])
    for x in (rng.uniform(0.5, 7.0, (1,) + hw).astype(np.float32), rng.normal(size=hw).astype(np.float32) * 1e-3,
              np.full((1,) + hw, 2.5, np.float32)):
        got = colormap(torch.from_numpy(x).to(DEV))
        want = colormap_host(torch.from_numpy(x))
        assert tuple(got.shape) == (3,) + hw and torch.equal(got.cpu(), want)


def test_colormap_halfway_indices_round_to_even():
    from gaussmart_amd.frames import colormap, colormap_host
    # min 0, max 255: (x - 0) / 255 * 255 lands on k + 0.5 for many k; rint and torch.round both go to even
    x = np.concatenate([np.arange(256, dtype=np.float32), np.arange(255, dtype=np.float32) + 0.5, [0.0]]).reshape(1, 16, 32)
    assert torch.equal(colormap(torch.from_numpy(x).to(DEV)).cpu(), colormap_host(torch.from_numpy(x)))


# ---------------------------------------------------------------- the sphere: render_net_image and the exports
@pytest.fixture(scope="module")
def sphere():
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.mesh import GaussianExtractor
    from gaussmart_amd.params import PipelineParams
    g = _sphere_model(6000)
    return g, GaussianExtractor(g, render, PipelineParams(depth_ratio=1.0), bg_color=[0, 0, 0])


def test_render_net_image(sphere):
    from gaussmart_amd.frames import RENDER_ITEMS, colormap, gradient_map, render_net_image, render_net_image_host
    g, ex = sphere
    cam = _sphere_cams(3, 100, 76)[1]
    with torch.no_grad():
        pkg = ex.render(cam, g)
    assert RENDER_ITEMS == ['RGB', 'Alpha', 'Normal', 'Depth', 'Edge', 'Curvature']
    normal01 = (pkg["rend_normal"] + 1) / 2
    parts = {"RGB": pkg["render"], "Alpha": colormap(pkg["rend_alpha"]), "Normal": normal01,
             "Depth": colormap(pkg["surf_depth"]), "Edge": colormap(gradient_map(pkg["render"])),
             "Curvature": colormap(gradient_map(normal01))}
    for mode, name in enumerate(RENDER_ITEMS):
        img = render_net_image(pkg, RENDER_ITEMS, mode, cam)
        assert tuple(img.shape) == (3, 76, 100) and img.dtype == torch.float32 and img.is_cuda
        assert torch.equal(img, parts[name]), name
        if name != "RGB":
            assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
        if name in ("RGB", "Alpha", "Normal", "Depth"):      # no gradient_map inside: the host twin gives the same bits
            assert torch.equal(img.cpu(), render_net_image_host(pkg, RENDER_ITEMS, mode, cam)), name
    # an unknown item falls through to the RGB render, as in the reference
    assert torch.equal(render_net_image(pkg, ["Other"], 0, cam), pkg["render"])


def test_export_image_routes_write_the_same_files(sphere, tmp_path):
    _, ex = sphere
    cams = _sphere_cams(4, 96, 96)
    cams[0].original_image = torch.rand(3, 96, 96, device=DEV)
    ex.reconstruction(cams)
    ex.depthmaps[1][0, 5, 7], ex.depthmaps[1][0, 6, 7] = float("nan"), float("inf")
    ex.export_image(str(tmp_path / "dev"))
    ex.export_image(str(tmp_path / "host"), host=True)
    names = sorted(str(p.relative_to(tmp_path / "host")) for p in (tmp_path / "host").rglob("*") if p.is_file())
    assert len(names) == 4 + 4 + 1 and "gt/00000.png" in names
    assert names == sorted(str(p.relative_to(tmp_path / "dev")) for p in (tmp_path / "dev").rglob("*") if p.is_file())
    for n in names:
        assert (tmp_path / "dev" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), n


def test_export_trajectory_routes(sphere, tmp_path, monkeypatch):
    from gaussmart_amd import video
    from gaussmart_amd.frames import depth_limits_host, depth_to_turbo_host
    from gaussmart_amd.render_path import generate_path
    _, ex = sphere
    taken = {}

    class Recorder(video.MJPEGWriter):
        def add_image(self, frame):
            taken.setdefault(self.path, []).append(np.array(frame))
            super().add_image(frame)

    monkeypatch.setattr(video, "MJPEGWriter", Recorder)
    ex.reconstruction(generate_path(_sphere_cams(9, 97, 97), 6))
    assert tuple(ex.rgbmaps[0].shape) == (3, 96, 96)
    for route, host in (("dev", False), ("host", True)):
        video.export_trajectory(ex, str(tmp_path / route), "render_traj", host=host)
    names = sorted(str(p.relative_to(tmp_path / "host")) for p in (tmp_path / "host").rglob("*") if p.is_file())
    assert names == sorted(str(p.relative_to(tmp_path / "dev")) for p in (tmp_path / "dev").rglob("*") if p.is_file())
    assert len(names) == 6 + 6 + 2 and not any(n.startswith("gt") for n in names)
    for n in names:
        if not n.endswith("_depth.avi"):
            assert (tmp_path / "dev" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), n
    d0 = np.nan_to_num(ex.depthmaps[0][0].cpu().numpy())
    lo, hi = depth_limits_host(d0)
    dev_frames, host_frames = (taken[str(tmp_path / r / "render_traj_depth.avi")] for r in ("dev", "host"))
    assert len(dev_frames) == len(host_frames) == 6
    for i in range(6):
        d = ex.depthmaps[i][0].cpu().numpy()
        assert np.array_equal(host_frames[i], depth_to_turbo_host(d, lo, hi)[1])
        share = check_depth_frame(dev_frames[i], d, lo, hi)
        print(f"trajectory depth frame {i}: share of pixels one table row off {share:.2e}")
    for r in ("dev", "host"):
        for k in ("color", "depth"):
            info = avi_info(str(tmp_path / r / f"render_traj_{k}.avi"))
            assert info["total_frames"] == len(info["frames"]) == 6 and (info["width"], info["height"]) == (96, 96)


# ---------------------------------------------------------------- the command
def test_render_cli_render_path(tmp_path):
    from PIL import Image
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.scene_io import Scene
    src, model = tmp_path / "src", tmp_path / "model"
    (src / "train").mkdir(parents=True)
    W = H = 97
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
    r = subprocess.run([sys.executable, "-m", "gaussmart_amd.render_cli", "-s", str(src), "-m", str(model), "--depth_ratio", "1",
                        "--skip_train", "--skip_test", "--skip_mesh", "--render_path", "--n_frames", "6"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = model / "traj" / "ours_7"
    pngs, tiffs = sorted((out / "renders").glob("*.png")), sorted((out / "vis").glob("depth_*.tiff"))
    assert len(pngs) == 6 and len(tiffs) == 6 and not list((out / "gt").glob("*"))
    for p, t in zip(pngs, tiffs):
        img, depth = np.array(Image.open(p)), np.array(Image.open(t))
        assert img.shape == (96, 96, 3) and img.dtype == np.uint8 and depth.shape == (96, 96) and depth.dtype == np.float32
        # the path looks at the scene: the centre pixel shows the sphere's grey (SH dc 0 -> 0.5) at a finite depth
        assert np.abs(img[48, 48].astype(np.float64) - 127.5).max() <= 2.0, img[48, 48]
        assert 0.5 < depth[48, 48] < 6.0
    for k in ("color", "depth"):
        info = avi_info(str(out / f"render_traj_{k}.avi"))
        assert info["total_frames"] == len(info["frames"]) == 6 and (info["width"], info["height"]) == (96, 96)
    colour = avi_info(str(out / "render_traj_color.avi"))
    import io
    for p, jpeg in zip(pngs, colour["frames"]):
        buf = io.BytesIO()
        Image.fromarray(np.array(Image.open(p))).save(buf, "JPEG", quality=95)
        assert jpeg == buf.getvalue()
