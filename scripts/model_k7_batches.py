#!/usr/bin/env python3
"""CPU model of render_bwd's batch loop (K7, gaussmart_amd/csrc/render_bwd.hip): how many loop iterations, staged records
and batches a frame costs when a wave's batch is 64 CONSECUTIVE list entries (the kernel before the compacting scan front)
and when it is the next B entries the forward blended into the wave's own 8x8 quad (the kernel now).

Oracle only, no GPU: the scene comes from gaussmart_amd.synthetic.make_scene, geometry and tile lists from
oracle.surfel_ref.preprocess / bin_tiles, and the touch nibbles (entry blended into >= 1 pixel of a 4x4 block) from an fp32
evaluation of the oracle's pair formulas.  Per quad the model walks the list backwards from the deepest entry any of its
pixels blended, as the kernel does, and counts
    iterations : sum over batches of max over the four 4x4 blocks of the block's to-do entries in that batch
    records    : entries gathered and staged (every entry of a consecutive batch; touched entries only when compacted)
    batches    : gather + stage + four ballots + wave barriers each
The defaults are the headline's density (1 M Gaussians at 1920x1080, radius_px 6) shrunk to 480x272.
Usage: python3 scripts/model_k7_batches.py [--width 480 --height 272 --gaussians 62962 --radius-px 6 --batch 64 128]"""
import argparse
import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE = 16


def touched_blocks(px, py, Tm, xy, opa, O):
    """[L, 256 pixels] bool: the forward blends list entry i into the pixel (oracle.surfel_ref._tile_eval's decisions)."""
    Tu, Tv, Tw = Tm[:, 0, :], Tm[:, 1, :], Tm[:, 2, :]
    pxb, pyb = px[None, :], py[None, :]
    k = [pxb * Tw[:, i:i + 1] - Tu[:, i:i + 1] for i in range(3)]
    l = [pyb * Tw[:, i:i + 1] - Tv[:, i:i + 1] for i in range(3)]
    p0, p1, p2 = k[1] * l[2] - k[2] * l[1], k[2] * l[0] - k[0] * l[2], k[0] * l[1] - k[1] * l[0]
    valid = p2 != 0
    p2s = torch.where(valid, p2, torch.ones_like(p2))
    sx, sy = p0 / p2s, p1 / p2s
    dx, dy = xy[:, 0:1] - pxb, xy[:, 1:2] - pyb
    rho2d = O.FILTER_INV_SQUARE * (dx * dx + dy * dy)
    rho3d = sx * sx + sy * sy
    use3d = rho3d <= rho2d
    depth = torch.where(use3d, sx * Tw[:, 0:1] + sy * Tw[:, 1:2] + Tw[:, 2:3], Tw[:, 2:3].expand_as(sx))
    power = -0.5 * torch.where(use3d, rho3d, rho2d)
    alpha = torch.clamp_max(opa[:, None] * torch.exp(power), O.ALPHA_MAX)
    valid = valid & (depth >= O.NEAR_N) & ~(power > 0) & (alpha >= O.ALPHA_MIN)
    cum = torch.cumprod(1 - torch.where(valid, alpha, torch.zeros_like(alpha)), dim=0)
    term = valid & (cum < O.T_EPS)
    L, P = alpha.shape
    first = torch.where(term.any(0), term.to(torch.uint8).argmax(0), torch.full((P,), L))
    return valid & (torch.arange(L)[:, None] < first[None, :])


def quad_counts(nib, batches):
    """nib: bool [n, 4] touch bits of ONE quad for list entries 0..n-1 (n = deepest blended entry + 1).  -> dict of
    (iterations, records, batches) for consecutive 64-entry batches, for every compacted batch size, and without boundary."""
    n = nib.shape[0]
    out = {}
    rev = nib[::-1]                                           # deep -> shallow, as the kernel walks
    pad = (-n) % 64
    c = np.concatenate([rev, np.zeros((pad, 4), bool)]).reshape(-1, 64, 4).sum(1)
    out["now"] = (int(c.max(1).sum()), n, c.shape[0])
    t = rev[rev.any(1)]
    u = t.shape[0]
    for B in batches:
        pad = (-u) % B
        c = np.concatenate([t, np.zeros((pad, 4), bool)]).reshape(-1, B, 4).sum(1)
        out[B] = (int(c.max(1).sum()), u, c.shape[0])
    out["none"] = (int(t.sum(0).max()) if u else 0, u, 1 if u else 0)
    out["union"] = u
    out["busy"] = int(nib.sum())                              # row-iterations that do work
    return out


def tile_job(args):
    (t, gx, W, H, Tm, xy, opa, batches) = args
    from oracle import surfel_ref as O
    torch.set_num_threads(1)
    ty, tx = divmod(t, gx)
    yy, xx = torch.meshgrid(torch.arange(ty * TILE, ty * TILE + TILE), torch.arange(tx * TILE, tx * TILE + TILE), indexing="ij")
    inside = ((yy < H) & (xx < W)).reshape(-1)
    contrib = touched_blocks(xx.reshape(-1).float(), yy.reshape(-1).float(), Tm, xy, opa, O) & inside[None, :]
    L = contrib.shape[0]
    # pixel (y, x) of the tile -> quad (y // 8) * 2 + x // 8, block ((y % 8) // 4) * 2 + (x % 8) // 4
    c = contrib.reshape(L, 2, 2, 4, 2, 2, 4).permute(0, 1, 4, 2, 5, 3, 6).reshape(L, 4, 4, 16).any(-1).numpy()
    tot = {}
    for q in range(4):
        nz = np.nonzero(c[:, q].any(1))[0]
        if nz.size == 0:
            continue
        r = quad_counts(c[:nz[-1] + 1, q], batches)
        for k, v in r.items():
            tot[k] = tuple(a + b for a, b in zip(tot.get(k, (0, 0, 0)), v)) if isinstance(v, tuple) else tot.get(k, 0) + v
    return tot, L, int(c.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=272)
    ap.add_argument("--gaussians", type=int, default=62962)
    ap.add_argument("--radius-px", type=float, default=6.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    from gaussmart_amd.synthetic import make_scene, activate
    from oracle import surfel_ref as O
    W, H = a.width, a.height
    p, cam = make_scene(a.gaussians, W, H, seed=a.seed, radius_px=a.radius_px)
    act = activate(p)
    S = O.Settings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.zeros(3), 1.0,
                   cam.world_view_transform.cpu().float(), cam.full_proj_transform.cpu().float(), 3, cam.camera_center.cpu().float())
    with torch.no_grad():
        g = O.preprocess(act["means3D"], act["scales"], act["rotations"], act["opacities"], None, None, None, S)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    N = a.gaussians
    depth_all = np.zeros(N, np.float32)
    depth_all[g.vis_idx.numpy()] = g.depth.numpy()
    keys, point_list = O.bin_tiles(None, g.radii.numpy(), g.rect.numpy(), depth_all, gx)
    ranges = O.tile_ranges(keys, gx * gy).astype(np.int64)
    D = int(point_list.size)
    slot = np.full(N, -1, np.int64)
    slot[g.vis_idx.numpy()] = np.arange(g.vis_idx.numel())
    opa = act["opacities"].reshape(-1)[g.vis_idx]
    jobs = []
    for t in range(gx * gy):
        ids = torch.from_numpy(slot[point_list[ranges[t, 0]:ranges[t, 1]].astype(np.int64)])
        if ids.numel():
            jobs.append((t, gx, W, H, g.Tm[ids], g.xy[ids], opa[ids], tuple(a.batch)))
    tot, rows = {}, 0
    with ProcessPoolExecutor(a.workers) as ex:
        for r, L, n_rows in ex.map(tile_job, jobs, chunksize=4):
            rows += n_rows
            for k, v in r.items():
                tot[k] = tuple(x + y for x, y in zip(tot.get(k, (0, 0, 0)), v)) if isinstance(v, tuple) else tot.get(k, 0) + v
    lens = ranges[:, 1] - ranges[:, 0]
    print(f"{N} Gaussians at {W}x{H}, radius_px {a.radius_px}: D = {D} instances, tile list mean {lens.mean():.1f} (max {lens.max()}), "
          f"{rows / max(D, 1):.2f} gradient rows per instance")
    now = tot["now"]
    print(f"iterations / |union of the four block lists| = {now[0] / max(tot['union'], 1):.3f}; a row is busy in "
          f"{tot['busy'] / (4 * now[0]):.0%} of the iterations now")
    print(f"{'':34s} {'iterations':>12s} {'records':>12s} {'batches':>10s}")
    labels = [("now", "now (64 consecutive entries)")] + [(B, f"{B} touched entries per batch") for B in a.batch] + \
             [("none", "no batch boundary at all")]
    for k, name in labels:
        it, rec, nb = tot[k]
        print(f"{name:34s} {it:12d} {rec:12d} {nb:10d}   x{it / now[0]:.3f}  x{rec / now[1]:.3f}  x{nb / now[2]:.3f}"
              + (f"   (row busy {tot['busy'] / (4 * it):.0%})" if it else ""))


if __name__ == "__main__":
    main()
