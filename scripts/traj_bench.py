"""Developer probe: time every stage of the trajectory export (gaussmart_amd.video.export_trajectory) on the unit-sphere surfel
scene of scripts/mesh_bench.py, 240 frames at 1600 x 1200 on the ellipse through 49 cameras, for both routes, stage by stage:

  device route   render | kernels (to_u8, depth_vis; once: the depth limits) | copy of the u8 frames and the cleaned fp32 depth |
                 PNG | TIFF | JPEG (both videos)
  host route     render | copy of the fp32 maps | numpy conversion (u8, nan_to_num; for the videos: / 255 * 255 and log,
                 normalise, turbo) | PNG | TIFF | reading the files back (create_videos works from the files) | JPEG

The stages are the same code the two routes of export_trajectory run, called one by one with a stream synchronisation
between them, so the sums are the routes' wall times without overlap.  Frame 0's files of the two routes are compared.
Writes a table to profiles/traj_export_bench.txt and prints one JSON line.

    python scripts/traj_bench.py [--surfels 300000] [--views 49] [--frames 240] [--width 1600] [--height 1200]
"""
import argparse
import contextlib
import io
import json
import math
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fib(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def sphere_model(n, dev):
    from gaussmart_amd.gaussian_model import GaussianModel
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
    return g


class Clock:
    def __init__(self):
        self.t = {}

    @contextlib.contextmanager
    def __call__(self, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yield
        torch.cuda.synchronize()
        self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0


def device_route(ex, out, clk):
    from PIL import Image
    from gaussmart_amd.frames import depth_limits, depth_to_turbo, to_u8
    from gaussmart_amd.video import MJPEGWriter
    H, W = ex.depthmaps[0].shape[-2:]
    for d in ("renders", "vis"):
        os.makedirs(os.path.join(out, d), exist_ok=True)
    with clk("limits"):
        lo, hi = depth_limits(ex.depthmaps[0], p=3)
    nbytes = 0
    with MJPEGWriter(os.path.join(out, "c.avi"), (H, W)) as cw, MJPEGWriter(os.path.join(out, "d.avi"), (H, W)) as dw:
        for i in range(len(ex.rgbmaps)):
            with clk("convert"):
                rgb = to_u8(ex.rgbmaps[i])
                clean, turbo = depth_to_turbo(ex.depthmaps[i], lo, hi)
            with clk("copy"):
                rgb, clean, turbo = rgb.cpu().numpy(), clean.reshape(H, W).cpu().numpy(), turbo.cpu().numpy()
            nbytes += rgb.nbytes + clean.nbytes + turbo.nbytes
            with clk("png"):
                Image.fromarray(rgb).save(os.path.join(out, "renders", f"{i:05d}.png"), "PNG")
            with clk("tiff"):
                Image.fromarray(clean).save(os.path.join(out, "vis", f"depth_{i:05d}.tiff"), "TIFF")
            with clk("jpeg"):
                cw.add_image(rgb)
                dw.add_image(turbo)
    return nbytes


def host_route(ex, out, clk):
    from PIL import Image
    from gaussmart_amd.frames import depth_limits_host, depth_to_turbo_host
    from gaussmart_amd.video import MJPEGWriter, load_img
    H, W = ex.depthmaps[0].shape[-2:]
    for d in ("renders", "vis"):
        os.makedirs(os.path.join(out, d), exist_ok=True)
    nbytes = 0
    n = len(ex.rgbmaps)
    for i in range(n):                                   # export_image(host=True)
        with clk("copy"):
            rgb, depth = ex.rgbmaps[i].permute(1, 2, 0).cpu().numpy(), ex.depthmaps[i][0].cpu().numpy()
        nbytes += rgb.nbytes + depth.nbytes
        with clk("convert"):
            rgb = (np.clip(np.nan_to_num(rgb), 0.0, 1.0) * 255.0).astype(np.uint8)
            depth = np.nan_to_num(depth).astype(np.float32)
        with clk("png"):
            Image.fromarray(rgb).save(os.path.join(out, "renders", f"{i:05d}.png"), "PNG")
        with clk("tiff"):
            Image.fromarray(depth).save(os.path.join(out, "vis", f"depth_{i:05d}.tiff"), "TIFF")
    with clk("read"):                                    # create_videos
        frame0 = load_img(os.path.join(out, "vis", "depth_00000.tiff"))
    with clk("limits"):
        lo, hi = depth_limits_host(frame0, p=3)
    with MJPEGWriter(os.path.join(out, "d.avi"), (H, W)) as dw:
        for i in range(n):
            with clk("read"):
                img = load_img(os.path.join(out, "vis", f"depth_{i:05d}.tiff"))
            with clk("convert"):
                frame = depth_to_turbo_host(img, lo, hi)[1]
            with clk("jpeg"):
                dw.add_image(frame)
    with MJPEGWriter(os.path.join(out, "c.avi"), (H, W)) as cw:
        for i in range(n):
            with clk("read"):
                img = load_img(os.path.join(out, "renders", f"{i:05d}.png"))
            with clk("convert"):
                frame = (np.clip(np.nan_to_num(img / 255.), 0., 1.) * 255.).astype(np.uint8)
            with clk("jpeg"):
                cw.add_image(frame)
    return nbytes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--surfels", type=int, default=300_000)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "traj_export_bench.txt"))
    ap.add_argument("--tmp", type=str, default=None, help="directory for the frames and videos (default: a temporary one)")
    args = ap.parse_args()
    from gaussmart_amd.camera import look_at_camera
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.mesh import GaussianExtractor
    from gaussmart_amd.params import PipelineParams
    from gaussmart_amd.render_path import generate_path
    dev = torch.device("cuda", 0)
    g = sphere_model(args.surfels, dev)
    cams = []
    for i, d in enumerate(fib(args.views)):
        up = (0, 0, 1) if abs(d[2]) < 0.95 else (0, 1, 0)
        cams.append(look_at_camera(2.5 * d, (0, 0, 0), up, math.radians(50), args.width, args.height, device=dev, uid=i))
    traj = generate_path(cams, n_frames=args.frames)
    ex = GaussianExtractor(g, render, PipelineParams(depth_ratio=1.0), bg_color=[0, 0, 0])
    with contextlib.redirect_stdout(io.StringIO()):
        ex.reconstruction(traj[:2])                      # warm-up: library load, allocator
    render_clk = Clock()
    with render_clk("render"), contextlib.redirect_stdout(io.StringIO()):
        ex.reconstruction(traj)
    tmp = args.tmp or tempfile.mkdtemp(prefix="traj_bench_")
    routes = {}
    try:
        for name, fn in (("device", device_route), ("host", host_route)):
            clk = Clock()
            moved = fn(ex, os.path.join(tmp, name), clk)
            routes[name] = dict(clk.t, bytes_to_host=moved)
        same = all(open(os.path.join(tmp, "device", f), "rb").read() == open(os.path.join(tmp, "host", f), "rb").read()
                   for f in ("renders/00000.png", "vis/depth_00000.tiff", "c.avi"))
        sizes = {f: os.path.getsize(os.path.join(tmp, "device", f)) for f in ("c.avi", "d.avi")}
    finally:
        if not args.tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    n = args.frames
    res = {"surfels": args.surfels, "views": args.views, "frames": n, "width": traj[0].image_width,
           "height": traj[0].image_height, "render_s": render_clk.t["render"], "routes": routes,
           "frame0_files_and_colour_video_identical": bool(same), "video_bytes": sizes}
    dvc, hst = routes["device"], routes["host"]
    dev_cc, host_cc = dvc["convert"] + dvc["copy"] + dvc["limits"], hst["convert"] + hst["copy"] + hst["limits"]
    lines = [f"trajectory export, {n} frames {res['width']} x {res['height']}, {args.surfels} surfels, path through {args.views} cameras",
             f"render (shared by both routes)            {res['render_s']:9.3f} s   {1e3 * res['render_s'] / n:8.2f} ms/frame", "",
             f"{'stage':<34}{'device route':>16}{'host route':>16}      (seconds, all frames)"]
    for key, label in (("limits", "depth limits (once)"), ("convert", "conversion"), ("copy", "device-to-host copy"),
                       ("png", "PNG encoding"), ("tiff", "TIFF encoding"), ("read", "reading the files back"),
                       ("jpeg", "JPEG encoding (two videos)")):
        lines.append(f"{label:<34}{dvc.get(key, 0.0):16.3f}{hst.get(key, 0.0):16.3f}")
    tot_d = sum(v for k, v in dvc.items() if k != "bytes_to_host")
    tot_h = sum(v for k, v in hst.items() if k != "bytes_to_host")
    enc_d, enc_h = dvc["png"] + dvc["tiff"] + dvc["jpeg"], hst["png"] + hst["tiff"] + hst["jpeg"]
    lines += [f"{'sum without render':<34}{tot_d:16.3f}{tot_h:16.3f}",
              f"{'bytes copied to the host':<34}{dvc['bytes_to_host'] / 1e9:13.3f} GB{hst['bytes_to_host'] / 1e9:13.3f} GB", "",
              f"conversion + copy + limits: device {dev_cc:.3f} s, host {host_cc:.3f} s: the device route is "
              f"{'faster' if dev_cc < host_cc else 'NOT faster'} ({host_cc / dev_cc:.2f} x)",
              f"encoding (PNG + TIFF + JPEG) is {100 * enc_d / tot_d:.1f} % of the device route and {100 * enc_h / tot_h:.1f} % of "
              f"the host route: {'the host-side encoders bound both routes' if enc_d > 0.5 * tot_d and enc_h > 0.5 * tot_h else 'see the rows above for what bounds each route'}",
              f"frame 0's PNG and TIFF and the colour video of the two routes identical: {same}"]
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
