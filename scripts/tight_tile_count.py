"""Instance count D of a synthetic scene with the reference tile rect and with GSR_FLAG_TIGHT_TILES, on the CPU.

A float32 torch transcription of the two boxes preprocess_one (gaussmart_amd/csrc/preprocess_fwd.hip) computes per
Gaussian -- the square of the major 3-sigma extent, and the conservative pixel box of {alpha >= 1/255} -- and of the
integer intersection gsr_clip_tile_rect (gsr_common.h) applies under the flag.  Statement order follows the kernel;
the CPU does not contract multiply-adds the way the GPU compiler does, so a box edge may round the other way for a
handful of Gaussians in a million: good for counts and for checking that a test scene is not vacuous, not a bit-exact
oracle of the lists.

    python scripts/tight_tile_count.py                   # seed 0 of every bench.py preset
    python scripts/tight_tile_count.py --preset scan24
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE, CUTOFF, FILTER_SIZE, NEAR, MIN_EXT2 = 16, 3.0, 0.707106, 0.2, 1e-4


def tile_rects(params, cam, width, height, scale_modifier=1.0):
    """Raw parameters (synthetic.make_scene layout) + camera -> dict of int64 tensors [N]:
    ref = (x0, y0, x1, y1) of the reference tile rect, tight = the same after the intersection with the alpha box,
    box = (x0, x1, y0, y1) of the alpha box in pixels, radii (0: culled)."""
    f = lambda t: t.detach().to("cpu", torch.float32)
    xyz, scaling, rot, opa_raw = f(params["xyz"]), f(params["scaling"]), f(params["rotation"]), f(params["opacity"]).reshape(-1)
    V, P = f(cam.world_view_transform), f(cam.full_proj_transform)
    W, H = int(width), int(height)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    px, py, pz = xyz.unbind(1)
    vx = px * V[0, 0] + py * V[1, 0] + pz * V[2, 0] + V[3, 0]
    vy = px * V[0, 1] + py * V[1, 1] + pz * V[2, 1] + V[3, 1]
    vz = px * V[0, 2] + py * V[1, 2] + pz * V[2, 2] + V[3, 2]
    alive = vz > NEAR

    q = rot * torch.rsqrt((rot * rot).sum(1, keepdim=True))
    qw, qx, qy, qz = q.unbind(1)
    r00, r10, r20 = 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy + qw * qz), 2 * (qx * qz - qw * qy)
    r01, r11, r21 = 2 * (qx * qy - qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz + qw * qx)
    r02, r12, r22 = 2 * (qx * qz + qw * qy), 2 * (qy * qz - qw * qx), 1 - 2 * (qx * qx + qy * qy)
    sx, sy = torch.exp(scaling[:, 0]) * scale_modifier, torch.exp(scaling[:, 1]) * scale_modifier
    one, zero = torch.ones_like(px), torch.zeros_like(px)
    rows = ((r00 * sx, r10 * sx, r20 * sx, zero), (r01 * sy, r11 * sy, r21 * sy, zero), (px, py, pz, one))
    hw, hh, cw, ch = 0.5 * W, 0.5 * H, 0.5 * (W - 1), 0.5 * (H - 1)
    Tu, Tv, Tw = [], [], []
    for a, b, c, e in rows:
        h0 = a * P[0, 0] + b * P[1, 0] + c * P[2, 0] + e * P[3, 0]
        h1 = a * P[0, 1] + b * P[1, 1] + c * P[2, 1] + e * P[3, 1]
        h3 = a * P[0, 3] + b * P[1, 3] + c * P[2, 3] + e * P[3, 3]
        Tu.append(h0 * hw + h3 * cw); Tv.append(h1 * hh + h3 * ch); Tw.append(h3)
    nx = r02 * V[0, 0] + r12 * V[1, 0] + r22 * V[2, 0]
    ny = r02 * V[0, 1] + r12 * V[1, 1] + r22 * V[2, 1]
    nz = r02 * V[0, 2] + r12 * V[1, 2] + r22 * V[2, 2]
    alive &= -(vx * nx + vy * ny + vz * nz) != 0

    # AABB of the 3-sigma ellipse, the reference's square tile rect
    t0 = CUTOFF * CUTOFF
    d = t0 * Tw[0] * Tw[0] + t0 * Tw[1] * Tw[1] - Tw[2] * Tw[2]
    alive &= d != 0
    inv_d = 1.0 / d
    f0, f1, f2 = t0 * inv_d, t0 * inv_d, -inv_d
    cx = f0 * Tu[0] * Tw[0] + f1 * Tu[1] * Tw[1] + f2 * Tu[2] * Tw[2]
    cy = f0 * Tv[0] * Tw[0] + f1 * Tv[1] * Tw[1] + f2 * Tv[2] * Tw[2]
    h0x = cx * cx - (f0 * Tu[0] * Tu[0] + f1 * Tu[1] * Tu[1] + f2 * Tu[2] * Tu[2])
    h0y = cy * cy - (f0 * Tv[0] * Tv[0] + f1 * Tv[1] * Tv[1] + f2 * Tv[2] * Tv[2])
    ex, ey = torch.sqrt(h0x.clamp_min(MIN_EXT2)), torch.sqrt(h0y.clamp_min(MIN_EXT2))
    radius = torch.ceil(torch.maximum(torch.maximum(ex, ey), torch.tensor(CUTOFF * FILTER_SIZE)))
    alive &= torch.isfinite(cx) & torch.isfinite(cy) & torch.isfinite(radius)
    cx_, cy_, rad_ = (torch.where(alive, t, zero) for t in (cx, cy, radius))
    trunc = lambda t: torch.trunc(t).long()     # (int) casts truncate toward zero
    x0 = trunc((cx_ - rad_) / TILE).clamp(0, gx); x1 = trunc((cx_ + rad_ + (TILE - 1)) / TILE).clamp(0, gx)
    y0 = trunc((cy_ - rad_) / TILE).clamp(0, gy); y1 = trunc((cy_ + rad_ + (TILE - 1)) / TILE).clamp(0, gy)
    alive &= (x1 - x0) * (y1 - y0) > 0
    z64 = torch.zeros_like(x0)
    ref = tuple(torch.where(alive, t, z64) for t in (x0, y0, x1, y1))

    # alpha box: [-32768, 32767] = never culled, x0 = 32767 > x1 = -32768 = cannot reach 1/255
    opa = 1.0 / (1.0 + torch.exp(-opa_raw))
    c2 = ((2.0 * torch.log(255.0 * opa)).clamp_min(0.0) + 0.05) * 1.02
    dd = c2 * (Tw[0] * Tw[0] + Tw[1] * Tw[1]) - Tw[2] * Tw[2]
    idd = 1.0 / dd
    g0, g2 = c2 * idd, -idd
    bqx = g0 * (Tu[0] * Tw[0] + Tu[1] * Tw[1]) + g2 * Tu[2] * Tw[2]
    bqy = g0 * (Tv[0] * Tw[0] + Tv[1] * Tw[1]) + g2 * Tv[2] * Tw[2]
    hx = torch.sqrt((bqx * bqx - (g0 * (Tu[0] * Tu[0] + Tu[1] * Tu[1]) + g2 * Tu[2] * Tu[2])).clamp_min(0.0))
    hy = torch.sqrt((bqy * bqy - (g0 * (Tv[0] * Tv[0] + Tv[1] * Tv[1]) + g2 * Tv[2] * Tv[2])).clamp_min(0.0))
    r2 = torch.sqrt(0.5 * c2)
    lox, hix = torch.minimum(bqx - hx, cx - r2), torch.maximum(bqx + hx, cx + r2)
    loy, hiy = torch.minimum(bqy - hy, cy - r2), torch.maximum(bqy + hy, cy + r2)
    mx, my = 1.0 + 0.01 * (hix - lox), 1.0 + 0.01 * (hiy - loy)
    lox, hix, loy, hiy = lox - mx, hix + mx, loy - my, hiy + my
    boxed = (dd < 0) & torch.isfinite(lox) & torch.isfinite(hix) & torch.isfinite(loy) & torch.isfinite(hiy)
    faint = 255.0 * opa < 0.999
    i16 = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).clamp(-32768.0, 32767.0).long()
    full_lo, full_hi = torch.full_like(x0, -32768), torch.full_like(x0, 32767)
    bx0 = torch.where(faint, full_hi, torch.where(boxed, i16(torch.floor(lox)), full_lo))
    bx1 = torch.where(faint, full_lo, torch.where(boxed, i16(torch.ceil(hix)), full_hi))
    by0 = torch.where(faint, full_hi, torch.where(boxed, i16(torch.floor(loy)), full_lo))
    by1 = torch.where(faint, full_lo, torch.where(boxed, i16(torch.ceil(hiy)), full_hi))

    # gsr_clip_tile_rect: a tile stays iff one of its four 8x8 quads passes gsr_rect_overlaps_quad
    tx0, tx1 = torch.maximum(ref[0], bx0 >> 4), torch.minimum(ref[2], (bx1 >> 4) + 1)
    ty0, ty1 = torch.maximum(ref[1], by0 >> 4), torch.minimum(ref[3], (by1 >> 4) + 1)
    keep = alive & (tx1 > tx0) & (ty1 > ty0)
    tight = tuple(torch.where(keep, t, z64) for t in (tx0, ty0, tx1, ty1))
    return dict(ref=ref, tight=tight, box=(bx0, bx1, by0, by1), radii=torch.where(alive, radius, zero).long())


def count(rect):
    return int(((rect[2] - rect[0]) * (rect[3] - rect[1])).sum())


def main():
    import bench
    from gaussmart_amd.synthetic import make_scene, jittered_cameras
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--preset", choices=sorted(bench.PRESETS), action="append")
    args = ap.parse_args()
    for name in args.preset or ("headline", "scan24", "bicycle", "truck"):
        p = bench.PRESETS[name]
        N, W, H = p["gaussians"], p["width"], p["height"]
        params, _ = make_scene(N, W, H, seed=0, device="cpu", radius_px=p["radius_px"])
        cam = jittered_cameras(1, W, H, seed=0, device="cpu")[0]          # the view bench.py renders on one GPU
        r = tile_rects(params, cam, W, H)
        d_ref, d_tight = count(r["ref"]), count(r["tight"])
        untiled = int(((r["radii"] > 0) & (count_per(r["tight"]) == 0)).sum())
        print(f"{name}: N={N} {W}x{H}  D_reference={d_ref}  D_tight={d_tight}  ({100.0 * (d_tight / d_ref - 1.0):+.1f} %)  "
              f"visible without a tile: {untiled}", flush=True)


def count_per(rect):
    return (rect[2] - rect[0]) * (rect[3] - rect[1])


if __name__ == "__main__":
    main()
