"""Times the device path and the host path of every part of gaussmart_amd.segment_init on a synthetic instance: a cloud of
--points points (default 1 M) with a hull of a few thousand facets, --views views (default 15) of 1554 x 1162 with --masks masks
each (default 100).  The host twins run on a cloud and a view count scaled down by --host_scale (default 0.05; their
per-point cost is what is compared, printed per million points / per view).  Writes a plain-text table.

    python scripts/segment_bench.py --out profiles/segment_init_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussmart_amd import segment_init as SI  # noqa: E402


def cloud(n, rng):
    """A ball with a sphere shell of 2 000 points: the shell gives the hull its few thousand facets."""
    shell = rng.normal(size=(2000, 3))
    shell /= np.linalg.norm(shell, axis=1, keepdims=True)
    inside = rng.normal(size=(max(n - 2000, 0), 3)) * 0.25
    inside *= np.minimum(1.0, 0.95 / np.linalg.norm(inside, axis=1, keepdims=True))     # strictly inside the shell
    return np.concatenate([shell, inside])[:max(n, 4)]


def blobs(m, h, w, rng):
    """m rectangular masks, uint8 [m,h,w]."""
    out = np.zeros((m, h, w), np.uint8)
    for k in range(m):
        x0, y0 = int(rng.integers(0, w - 40)), int(rng.integers(0, h - 40))
        out[k, y0:y0 + int(rng.integers(30, h // 3)), x0:x0 + int(rng.integers(30, w // 3))] = 1
    return out


def camera(k, n_views):
    a = 2 * np.pi * k / n_views
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    world = np.eye(4)
    world[:3, :3], world[:3, 3] = R, [0, 0, 3.0]
    return {"world_mat": world, "scale_mat": np.eye(4), "camera_mat": np.array([[900.0, 0, 777, 0], [0, 900, 581, 0], [0, 0, 1, 0], [0, 0, 0, 1]])}


def timed(fn, sync, repeat=1):
    fn()                                                    # warm-up (allocations, first launch)
    sync()
    best = float("inf")
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        sync()
        best = min(best, time.perf_counter() - t)
    return best * 1e3, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--masks", type=int, default=100)
    ap.add_argument("--size", type=int, nargs=2, default=[1554, 1162], metavar=("W", "H"))
    ap.add_argument("--host_scale", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_init_bench.txt"))
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    W, H = args.size
    n, nh = args.points, max(int(args.points * args.host_scale), 4000)
    vh = max(int(round(args.views * args.host_scale)), 1)
    pts = cloud(n, rng)
    n = len(pts)
    sync, nosync = (lambda: torch.cuda.synchronize(dev)), (lambda: None)
    rows = []

    def row(part, dev_ms, dev_units, host_ms, host_units, unit):
        rows.append((part, dev_ms, dev_ms / dev_units, host_ms, host_ms / host_units, unit))

    t = time.perf_counter()
    eq = SI.hull_equations(pts)
    qhull_ms = (time.perf_counter() - t) * 1e3
    p_d = torch.from_numpy(pts).to(dev)
    d_ms, d = timed(lambda: SI.hull_distances(p_d, eq), sync, args.repeat)
    h_ms, dh = timed(lambda: SI.hull_distances_host(pts[:nh], eq), nosync)
    row(f"hull distances ({len(eq)} facets)", d_ms, n / 1e6, h_ms, nh / 1e6, "ms per M points")
    d_ms, _ = timed(lambda: SI.mean_std(d), sync, args.repeat)
    h_ms, _ = timed(lambda: SI.mean_std_host(dh), nosync)
    row("mean / std", d_ms, n / 1e6, h_ms, nh / 1e6, "ms per M points")

    masks = blobs(args.masks, H, W, rng)
    m_d = torch.from_numpy(masks).to(dev)
    d_ms, (lm, _) = timed(lambda: SI.build_label_map(m_d), sync, args.repeat)
    h_ms, _ = timed(lambda: SI.build_label_map_host(masks), nosync)
    row(f"label map ({args.masks} masks, {W} x {H}), masks on the device", d_ms, 1, h_ms, 1, "ms per view")
    u_ms, _ = timed(lambda: SI.build_label_map(masks, device=dev), sync, args.repeat)
    row("label map, masks uploaded from the host", u_ms, 1, h_ms, 1, "ms per view")

    cams = [camera(k, args.views) for k in range(args.views)]
    maps = [lm] * args.views
    d_ms, _ = timed(lambda: SI.assign_segments(p_d, cams, "nerf", maps), sync, args.repeat)
    lm_h = lm.cpu().numpy()
    h_ms, _ = timed(lambda: SI.assign_segments_host(pts[:nh], cams[:vh], "nerf", [lm_h] * vh), nosync)
    row(f"projection + assignment ({args.views} views)", d_ms, n / 1e6 * args.views, h_ms, nh / 1e6 * vh, "ms per M points and view")

    lab = SI.assign_segments(p_d, cams, "nerf", maps).to(torch.int64)
    n_labels = args.masks
    p32, c32 = p_d.float(), torch.rand((n, 3), device=dev)
    d_ms, stats = timed(lambda: SI.segment_stats(p32, c32, lab, n_labels), sync, args.repeat)
    h_ms, _ = timed(lambda: SI.segment_stats_host(p32[:nh].cpu(), c32[:nh].cpu(), lab[:nh].cpu(), n_labels), nosync)
    row(f"segment statistics ({n_labels} labels)", d_ms, n / 1e6, h_ms, nh / 1e6, "ms per M points")
    areas = {k: 10 ** 10 for k in range(n_labels)}
    d_ms, new = timed(lambda: SI.augment_point_cloud(p32, c32, lab, areas, generator=torch.Generator(device=dev).manual_seed(0)), sync,
                      args.repeat)
    h_ms, _ = timed(lambda: SI.augment_point_cloud_host(p32[:nh].cpu(), c32[:nh].cpu(), lab[:nh].cpu(), areas,
                                                       generator=torch.Generator().manual_seed(0)), nosync)
    row(f"augmentation, whole ({len(new[0])} new points on the device)", d_ms, 1, h_ms, 1, "ms per call")

    lines = [f"segment_init on {torch.cuda.get_device_name(dev)}: {n} points, {args.views} views of {W} x {H}, {args.masks} masks each",
             f"host twins on {nh} points and {vh} view(s) (numpy float64, one thread); Qhull on the host: {qhull_ms:.0f} ms for {n} points",
             "", f"{'part':72s} {'device ms':>10s} {'per unit':>10s} {'host ms':>10s} {'per unit':>10s}  unit"]
    for part, dm, du, hm, hu, unit in rows:
        lines.append(f"{part:72s} {dm:10.3f} {du:10.3f} {hm:10.1f} {hu:10.1f}  {unit}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
