"""Test-only restatement of the reference's unbounded field (utils/mesh_utils.py:184-279: contract, uncontract,
compute_sdf_perframe, compute_unbounded_tsdf) on torch CPU ops, written afresh from the rules of include/gsr.h (UNB_*).  It
calls torch.nn.functional.grid_sample itself and runs in float32 or float64.  Besides the field it reports, per point,
whether any decision on the way was close (`unstable`): u or v near +-1, z near 0, sdf near -trunc, |s| near 1, 1.9 or 2, a
clamp bound of sdf / trunc.  Two correct implementations may decide such a point differently, so comparisons leave it out.

Fixtures shared by tests/test_unbounded_cpu.py and tests/test_gpu_unbounded.py live here too."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def contract(x):
    mag = torch.linalg.norm(x, ord=2, dim=-1)[..., None]
    return torch.where(mag < 1, x, (2 - (1 / mag)) * (x / mag))


def uncontract(y):
    mag = torch.linalg.norm(y, ord=2, dim=-1)[..., None]
    return torch.where(mag < 1, y, (1 / (2 - mag)) * (y / mag))


def lattice_coords(R, resolution, crop, dtype=torch.float32):
    """UNB_LATTICE: formed in fp64; rounded to fp32 first even for the fp64 run (the fp32 coordinate IS the lattice point)."""
    G = (resolution // crop) * (crop - 1) + 1
    s = -float(R) + np.arange(G, dtype=np.float64) * (2.0 * float(R) / (G - 1))
    return torch.from_numpy(s.astype(np.float32)).to(dtype)


def lattice_points(R, resolution, crop, lo=None, dims=None, dtype=torch.float32):
    s = lattice_coords(R, resolution, crop, dtype)
    G = len(s)
    lo = (0, 0, 0) if lo is None else lo
    dims = (G, G, G) if dims is None else dims
    ax = [s[l:l + d] for l, d in zip(lo, dims)]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def field(points, views, center, radius, voxel_size, contracted=True, dtype=torch.float32, eps=1e-4):
    """(tsdf [n], rgb [n,3], unstable bool [n]) of compute_unbounded_tsdf.  eps: how close (relative to the quantity's scale)
    a decision has to be to count as unstable."""
    s = points.to(dtype)
    center = torch.as_tensor(center, dtype=torch.float32).to(dtype)
    unstable = torch.zeros(len(s), dtype=torch.bool)
    trunc0 = torch.tensor(np.float32(5.0 * float(voxel_size))).to(dtype)   # 5 voxel_size * ones_like(f32): rounded to f32
    if contracted:
        m = torch.linalg.norm(s, dim=-1)
        trunc = trunc0 * torch.ones_like(m)
        mask = m > 1
        trunc[mask] = trunc[mask] * (1 / (2 - m[mask].clamp(max=1.9)))
        x = uncontract(s) * float(np.float32(radius)) + center
        for edge in (1.0, 1.9, 2.0):
            unstable |= (m - edge).abs() < eps
    else:
        x, trunc = s, trunc0 * torch.ones(len(s), dtype=dtype)
    tsdf = torch.ones(len(s), dtype=dtype)
    rgbs = torch.zeros((len(s), 3), dtype=dtype)
    w = torch.ones(len(s), dtype=dtype)
    for M, depth, rgb in views:
        M, depth, rgb = M.to(dtype), depth.to(dtype).reshape(1, *depth.shape[-2:]), rgb.to(dtype)
        p = torch.cat([x, torch.ones_like(x[:, :1])], -1) @ M
        z = p[:, -1:]
        pix = p[:, :2] / z
        ok = ((pix > -1.0) & (pix < 1.0) & (z > 0)).all(-1)
        grid = torch.nan_to_num(pix, nan=0.0, posinf=2.0, neginf=-2.0)[None, None]
        d = F.grid_sample(depth[None], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(-1)
        c = F.grid_sample(rgb[None], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(3, -1).T
        sdf = d - z[:, 0]
        fin = torch.isfinite(pix).all(-1) & torch.isfinite(z[:, 0])
        near_proj = fin & (((pix.abs() - 1).abs() < eps).any(-1) | (z[:, 0].abs() < eps))
        in_view = fin & ((pix.abs() < 1 + eps).all(-1)) & (z[:, 0] > -eps)
        q = sdf / trunc
        near_sdf = in_view & (((q + 1).abs() < eps) | ((q - 1).abs() < eps))
        unstable |= near_proj | near_sdf
        ok = ok & (sdf > -trunc)
        t = q.clamp(-1.0, 1.0)
        wp = w + 1
        tsdf = torch.where(ok, (tsdf * w + t) / wp, tsdf)
        rgbs = torch.where(ok[:, None], (rgbs * w[:, None] + c) / wp[:, None], rgbs)
        w = torch.where(ok, wp, w)
    return tsdf, rgbs, unstable


def finish(verts_index, R, resolution, crop, center, radius, max_range=32.0, dtype=torch.float64):
    """UNB_VERTEX: index-space vertices (lattice position + 0.5) -> world."""
    G = (resolution // crop) * (crop - 1) + 1
    s = -float(R) + (verts_index.double() - 0.5) * (2.0 * float(R) / (G - 1))
    s = s.float().to(dtype)
    x = uncontract(s) * float(np.float32(radius)) + torch.as_tensor(center, dtype=torch.float32).to(dtype)
    return x.clamp(-max_range, max_range)


# ------------------------------------------------------------------------------------------------ fixtures
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world_view_transform in the rasterizer's row-vector convention (p_cam = [x, 1] @ V), camera looking down +z."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    if np.linalg.norm(r) < 1e-6:
        r = np.cross(f, np.array([0.0, 1.0, 0.0]))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    Rm = np.stack([r, d, f], 1)            # world -> camera rotation as columns
    V = np.eye(4)
    V[:3, :3] = Rm
    V[3, :3] = -eye @ Rm
    return V


def full_proj(eye, target, fovx, fovy, znear=0.01, zfar=100.0):
    """full_proj_transform [4,4] float32 (row-vector convention), the camera.py projection: p.w = camera z."""
    V = look_at(eye, target)
    tx, ty = math.tan(fovx / 2), math.tan(fovy / 2)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 1 / tx, 1 / ty
    P[2, 2], P[2, 3] = zfar / (zfar - znear), 1.0
    P[3, 2] = -zfar * znear / (zfar - znear)
    return torch.from_numpy((V @ P).astype(np.float32)), V


def render_analytic(eye, target, fovx, fovy, H, W, sphere_c, sphere_r, floor_z=None, holes=True, grey=0.6, shell=None):
    """One view of an analytic sphere (plus a ground plane z = floor_z seen from above): (M, depth [1,H,W], rgb [3,H,W]).
    depth is camera z of the first hit; no hit -> 0, or with shell the inside of a sphere of that radius around sphere_c (a
    room: free space then gets positive votes, as in a scene with a background); with holes a few rows of zero depth are
    punched in.  The pixel grid is the align_corners one: pixel i sits at ndc -1 + 2 i / (W - 1)."""
    M, V = full_proj(eye, target, fovx, fovy)
    Rm = V[:3, :3]
    u = np.linspace(-1, 1, W) if W > 1 else np.zeros(1)
    v = np.linspace(-1, 1, H) if H > 1 else np.zeros(1)
    uu, vv = np.meshgrid(u, v)
    dirs_cam = np.stack([uu * math.tan(fovx / 2), vv * math.tan(fovy / 2), np.ones_like(uu)], -1)   # z = 1
    dirs = dirs_cam @ Rm.T
    o = np.asarray(eye, np.float64)
    depth = np.full((H, W), np.inf)
    oc = o - np.asarray(sphere_c, np.float64)
    a = (dirs * dirs).sum(-1)
    b = 2 * (dirs @ oc)
    c = oc @ oc - sphere_r ** 2
    disc = b * b - 4 * a * c
    t = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
    hit = (disc > 0) & (t > 0)
    depth[hit] = t[hit]
    if floor_z is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            tf = (floor_z - o[2]) / dirs[..., 2]
        hf = np.isfinite(tf) & (tf > 0) & (tf < depth)
        depth[hf] = tf[hf]
    if shell is not None:
        ts = (-b + np.sqrt(np.maximum(b * b - 4 * a * (oc @ oc - shell ** 2), 0))) / (2 * a)
        miss = ~np.isfinite(depth)
        depth[miss] = ts[miss]
    depth[~np.isfinite(depth)] = 0.0
    if holes:
        depth[H // 3:H // 3 + 2, W // 4:W // 2] = 0.0
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([grey + 0.3 * np.sin(0.37 * xx), grey + 0.3 * np.cos(0.23 * yy), grey + 0.2 * np.sin(0.11 * (xx + yy))])
    return M, torch.from_numpy(depth[None].astype(np.float32)), torch.from_numpy(rgb.astype(np.float32))


CENTER = (0.05, -0.02, 0.1)
RADIUS = 1.3


def parity_views():
    """The field-parity fixture: five views of 40x30 and 33x47 (W x H) around a sphere of radius 0.45 on a ground plane;
    view 1 stands inside the lattice region (many points with z <= 0), view 2 looks past the scene (part of the lattice
    off-frame); zero-depth holes in every map."""
    sc, sr, fz = (0.1, 0.0, 0.15), 0.45, -0.4
    cams = [((2.6, 0.3, 1.2), sc, 0.9, 0.7, 30, 40),
            ((0.4, 0.5, 0.6), sc, 1.0, 1.2, 47, 33),
            ((-2.2, 1.9, 1.5), (0.9, 0.8, 0.0), 0.6, 0.8, 47, 33),
            ((-1.0, -2.8, 2.0), sc, 0.8, 0.6, 30, 40),
            ((0.3, 0.2, 3.5), sc, 0.9, 0.9, 30, 40)]
    return [render_analytic(e, t, fx, fy, H, W, sc, sr, fz) for e, t, fx, fy, H, W in cams]


def ring_views(n, H, W, sphere_c, sphere_r, dist, floor_z=None, fov=0.9, grey=0.6, holes=False, shell=None):
    """n views on two rings around the sphere, all looking at its centre from above the floor."""
    out = []
    for i in range(n):
        a = 2 * math.pi * i / n
        el = 0.35 if i % 2 == 0 else 0.9
        eye = (sphere_c[0] + dist * math.cos(a) * math.cos(el), sphere_c[1] + dist * math.sin(a) * math.cos(el),
               sphere_c[2] + dist * math.sin(el))
        out.append(render_analytic(eye, sphere_c, fov, fov, H, W, sphere_c, sphere_r, floor_z, holes=holes, grey=grey, shell=shell))
    return out


def fib_dirs(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def around_views(n, H, W, sphere_c, sphere_r, dist, fov=0.9, shell=None):
    """n views from all around the sphere (Fibonacci directions), so that every part of it is seen from the front."""
    c = np.asarray(sphere_c, np.float64)
    return [render_analytic(tuple(c + dist * d), sphere_c, fov, fov, H, W, sphere_c, sphere_r, holes=False, shell=shell)
            for d in fib_dirs(n)]
