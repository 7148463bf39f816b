"""What the visibility-culling tests hold gaussmart_amd.mesh_visibility to (helper, no tests):

  * raster_np / raster64   the rules VIS_CAMERA ... VIS_RANGE of include/gsr.h in plain numpy of one dtype (float64: the
                           reference; float32: the restatement the two constants below are measured with), every candidate
                           (pixel, triangle) pair evaluated, returning the depth image and the nearest triangle per pixel;
  * vote64                 VIS_PROJECT ... VIS_VOTE in float64 on given depth images;
  * depth_interval_errors  the interval test of the depth images: every pixel, nothing excluded;
  * vote_pairs, vote_bounds  per pair whether it is stable; per vertex the stable seeing views s and the unstable pairs u;
  * compact_ref            VIS_COMPACT in plain numpy;
  * the fixtures of tests/test_mesh_vis_cpu.py and tests/test_gpu_mesh_vis.py.
"""
import numpy as np

# DELTA_PX = 4 x the largest |float32 - float64| difference in projected pixel position (VIS_PROJECT's u, v) over the (vertex,
# view) pairs of the fixtures below that lie within one pixel of the frame.  TAU = 4 x the largest relative depth difference
# between raster_np(float32) and raster64 at the pixels where both hit the same triangle.  The factor 4: the device sums in
# another order (fmaf chains) than numpy.  Measured (tests/test_mesh_vis_cpu.py prints and checks both):
#   two-sphere scene at 96 x 64 7.5e-6 px / 1.23e-6, at 33 x 17 3.3e-6 px / 1.24e-6; sub-pixel scene 1.07e-5 px / 1.29e-6;
#   vote scene 1.40e-5 px  ->  DELTA_PX = 4 x 1.41e-5 = 5.64e-5 px, TAU = 4 x 1.3e-6 = 5.2e-6.
# (Both are smaller than a guess from the formats would be: the fixtures sit within a few units of the origin at f <= 100.)
MEASURED_PX = 1.41e-5
MEASURED_REL = 1.3e-6
DELTA_PX = 4 * MEASURED_PX
TAU = 4 * MEASURED_REL

NEAR, FAR, EPS = 0.01, 20.0, 0.005
_BOX = 8


# ---------------------------------------------------------------- VIS_CAMERA ... VIS_RANGE
def camera_space(verts, w2c, dtype=np.float64):
    v = np.asarray(verts, np.float32).astype(dtype).reshape(-1, 3)
    m = np.asarray(w2c, np.float32).astype(dtype).reshape(3, 4)
    with np.errstate(all="ignore"):
        return v[:, 0:1] * m[:, 0] + v[:, 1:2] * m[:, 1] + v[:, 2:3] * m[:, 2] + m[:, 3]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _edge(pa, ia, pb, ib):
    return np.where((ia <= ib)[:, None], _cross(pa, pb), -_cross(pb, pa))


def _hit_depth(c0, c1, c2, n, np0, dx, dy, near, far):
    def dot(c):
        return c[:, 0:1] * dx + c[:, 1:2] * dy + c[:, 2:3]
    b0, b1, b2 = dot(c0), dot(c1), dot(c2)
    pos = (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
    neg = (b0 <= 0) & (b1 <= 0) & (b2 <= 0)
    nd = dot(n)
    z = np0[:, None] / nd
    return np.where((pos ^ neg) & (nd != 0) & (z >= near) & (z <= far), z, np.inf)


def raster_np(verts, tris, w2c, H, W, intr, near=NEAR, far=FAR, shift=(0.0, 0.0), dtype=np.float64):
    """(depth [H,W] of `dtype`, 0 = no hit; nearest triangle int64 [H,W], -1 = none) of ONE view.  Pixel (i, j) asks the ray
    through (i + 0.5 + shift[0], j + 0.5 + shift[1]).  Candidates: every pixel of the image for a triangle that crosses the
    near plane, every pixel within two pixels of the projected bounding box otherwise (in exact arithmetic a hit lies inside
    the box; |shift| stays far below one pixel)."""
    t = dtype
    fx, fy, cx, cy = (t(a) for a in intr)
    near, far = t(near), t(far)
    depth = np.zeros((H, W), dtype)
    tri_id = np.full((H, W), -1, np.int64)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    if not len(tris):
        return depth, tri_id
    with np.errstate(all="ignore"):
        p = camera_space(verts, w2c, dtype)
        i0, i1, i2 = tris[:, 0], tris[:, 1], tris[:, 2]
        p0, p1, p2 = p[i0], p[i1], p[i2]
        zs = np.stack([p0[:, 2], p1[:, 2], p2[:, 2]], 1)
        ok = np.isfinite(p0).all(1) & np.isfinite(p1).all(1) & np.isfinite(p2).all(1) & ~(zs < near).all(1)
        front = ok & (zs >= near).all(1)
        x0, x1 = np.zeros(len(tris), np.int64), np.full(len(tris), W - 1, np.int64)
        y0, y1 = np.zeros(len(tris), np.int64), np.full(len(tris), H - 1, np.int64)
        q = [a[front] for a in (p0, p1, p2)]
        u = np.stack([fx * a[:, 0] / a[:, 2] + cx for a in q], 1)
        v = np.stack([fy * a[:, 1] / a[:, 2] + cy for a in q], 1)
        x0[front] = np.clip(np.ceil(u.min(1) - 2.5), 0, W).astype(np.int64)
        x1[front] = np.clip(np.floor(u.max(1) + 1.5), -1, W - 1).astype(np.int64)
        y0[front] = np.clip(np.ceil(v.min(1) - 2.5), 0, H).astype(np.int64)
        y1[front] = np.clip(np.floor(v.max(1) + 1.5), -1, H - 1).astype(np.int64)
        ok &= (x0 <= x1) & (y0 <= y1)
        c0, c1, c2 = _edge(p1, i1, p2, i2), _edge(p2, i2, p0, i0), _edge(p0, i0, p1, i1)
        n = _cross(p1 - p0, p2 - p0)
        np0 = n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1] + n[:, 2] * p0[:, 2]
        rx = ((np.arange(W).astype(t) + t(0.5) + t(shift[0])) - cx) / fx
        ry = ((np.arange(H).astype(t) + t(0.5) + t(shift[1])) - cy) / fy
        pix, zz, who = [], [], []
        small = ok & (x1 - x0 < _BOX) & (y1 - y0 < _BOX)
        oy, ox = (a.reshape(-1) for a in np.mgrid[0:_BOX, 0:_BOX])
        ids = np.nonzero(small)[0]
        for a in range(0, len(ids), 16384):
            k = ids[a:a + 16384]
            px, py = x0[k, None] + ox[None, :], y0[k, None] + oy[None, :]
            valid = (px <= x1[k, None]) & (py <= y1[k, None])
            px, py = np.minimum(px, W - 1), np.minimum(py, H - 1)
            z = _hit_depth(c0[k], c1[k], c2[k], n[k], np0[k], rx[px], ry[py], near, far)
            hit = valid & np.isfinite(z)
            pix.append((py * W + px)[hit]); zz.append(z[hit]); who.append(np.broadcast_to(k[:, None], z.shape)[hit])
        for k in np.nonzero(ok & ~small)[0]:
            yy, xx = np.mgrid[y0[k]:y1[k] + 1, x0[k]:x1[k] + 1]
            yy, xx = yy.reshape(1, -1), xx.reshape(1, -1)
            s = slice(k, k + 1)
            z = _hit_depth(c0[s], c1[s], c2[s], n[s], np0[s], rx[xx], ry[yy], near, far)
            hit = np.isfinite(z)
            pix.append((yy * W + xx)[hit]); zz.append(z[hit]); who.append(np.full(int(hit.sum()), k))
    if pix:
        pix, zz, who = np.concatenate(pix), np.concatenate(zz), np.concatenate(who)
        order = np.lexsort((who, zz, pix))
        pix, zz, who = pix[order], zz[order], who[order]
        first = np.ones(len(pix), bool)
        first[1:] = pix[1:] != pix[:-1]
        depth.reshape(-1)[pix[first]] = zz[first]
        tri_id.reshape(-1)[pix[first]] = who[first]
    return depth, tri_id


def raster64(verts, tris, w2c, H, W, intr, near=NEAR, far=FAR, shift=(0.0, 0.0)):
    return raster_np(verts, tris, w2c, H, W, intr, near, far, shift, np.float64)


def five_rasters(verts, tris, w2c, H, W, intr, near=NEAR, far=FAR, delta=None):
    """raster64 depth at the pixel centre and at (+-delta, +-delta): float64 [5,H,W]."""
    d = DELTA_PX if delta is None else delta
    return np.stack([raster64(verts, tris, w2c, H, W, intr, near, far, s)[0]
                     for s in ((0, 0), (-d, -d), (-d, d), (d, -d), (d, d))])


def depth_interval_errors(got, five, tau=None):
    """The interval test for one view: got [H,W] against five [5,H,W].  Returns (bad pixels bool [H,W], pixels whose five samples
    disagree about hitting).  All five hit: got in [min (1 - tau), max (1 + tau)].  None hits: got == 0.  Otherwise: got == 0
    or inside the widened interval of the samples that hit."""
    tau = TAU if tau is None else tau
    got = np.asarray(got, np.float64)
    hit = five > 0
    lo = np.where(hit, five, np.inf).min(0) * (1 - tau)
    hi = np.where(hit, five, -np.inf).max(0) * (1 + tau)
    inside = (got >= lo) & (got <= hi)
    all_hit, none_hit = hit.all(0), ~hit.any(0)
    good = np.where(all_hit, inside, np.where(none_hit, got == 0, (got == 0) | inside))
    return ~good, ~(all_hit | none_hit)


# ---------------------------------------------------------------- VIS_PROJECT ... VIS_VOTE
def project(verts, w2c, intr, dtype=np.float64):
    """(u, v, z) of VIS_PROJECT in `dtype`."""
    t = dtype
    fx, fy, cx, cy = (t(a) for a in intr)
    with np.errstate(all="ignore"):
        p = camera_space(verts, w2c, dtype)
        z = p[:, 2] + t(np.float32(1e-8))
        return (fx * p[:, 0] + cx * p[:, 2]) / z, (fy * p[:, 1] + cy * p[:, 2]) / z, z


def vote64(verts, w2c, depths, intr, eps=EPS, shift=(0.0, 0.0), zscale=1.0):
    """seen bool [n,V]: VIS_PROJECT ... VIS_VOTE in float64 on the depth images `depths` [n,H,W], with the projected position
    moved by `shift` pixels and z multiplied by zscale."""
    depths = np.asarray(depths).astype(np.float64)
    n, H, W = depths.shape
    V = len(np.asarray(verts).reshape(-1, 3))
    seen = np.zeros((n, V), bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            u, v, z = project(verts, w2c[i], intr)
            u, v, z = u + shift[0], v + shift[1], z * zscale
            ok = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
            k = np.nonzero(ok)[0]
            uu, vv = u[k], v[k]
            x0, y0 = np.floor(uu).astype(np.int64), np.floor(vv).astype(np.int64)
            ax, ay = uu - x0, vv - y0
            xr, yd = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)      # weight 0 where clamped
            img = depths[i]
            ds = img[y0, x0] * (1 - ax) * (1 - ay) + img[y0, xr] * ax * (1 - ay) + img[yd, x0] * (1 - ax) * ay + img[yd, xr] * ax * ay
            seen[i, k] = np.where(ds > 0, z[k] < ds + np.float64(np.float32(eps)), True)
    return seen


def vote_pairs(verts, w2c, depths, intr, eps=EPS, delta=None, tau=None):
    """(seen, stable) bool [n,V]: vote64, and whether the pair is stable: vote64 gives the same answer at the centre and at the
    four positions (+-delta, +-delta), each with z (1 + tau) and z (1 - tau)."""
    d = DELTA_PX if delta is None else delta
    tau = TAU if tau is None else tau
    seen = vote64(verts, w2c, depths, intr, eps)
    stable = np.ones(seen.shape, bool)
    for sx in (-d, d):
        for sy in (-d, d):
            for zs in (1 - tau, 1 + tau):
                stable &= vote64(verts, w2c, depths, intr, eps, (sx, sy), zs) == seen
    return seen, stable


def vote_bounds(verts, w2c, depths, intr, eps=EPS, delta=None, tau=None):
    """(s, u, seen): per vertex the number of STABLE views that see it and the number of unstable (vertex, view) pairs."""
    seen, stable = vote_pairs(verts, w2c, depths, intr, eps, delta, tau)
    return (seen & stable).sum(0), (~stable).sum(0), seen


def compact_ref(verts, colors, tris, keep):
    """VIS_COMPACT in plain numpy: (vertices, colours, triangles int32)."""
    keep = np.asarray(keep, bool)
    tk = keep[tris].all(1) if len(tris) else np.zeros(0, bool)
    used = np.zeros(len(keep), bool)
    used[tris[tk].reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], colors[used], remap[tris[tk]].reshape(-1, 3).astype(np.int32)


# ---------------------------------------------------------------- fixtures
def uv_sphere(segments, rings, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A closed, welded sphere: segments * (rings - 1) + 2 vertices, 2 * segments * (rings - 1) triangles, outward winding."""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segments))], -1)
    verts = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]])
    idx = lambda r, s: 1 + r * segments + (s % segments)
    south = len(verts) - 1
    tris = []
    for s in range(segments):
        tris.append([0, idx(0, s), idx(0, s + 1)])
        for r in range(rings - 2):
            tris.append([idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)])
            tris.append([idx(r, s), idx(r + 1, s + 1), idx(r, s + 1)])
        tris.append([south, idx(rings - 2, s + 1), idx(rings - 2, s)])
    return (verts * radius + np.asarray(centre)).astype(np.float32), np.asarray(tris, np.int32)


def join(*meshes):
    verts, tris, base = [], [], 0
    for v, t in meshes:
        verts.append(v); tris.append(t + base); base += len(v)
    return np.concatenate(verts), np.concatenate(tris).astype(np.int32)


def look_at_c2w(eye, target=(0.0, 0.0, 0.0)):
    """An OpenCV camera-to-world pose [4,4] float64 (x right, y down, z forward)."""
    eye = np.asarray(eye, float)
    fwd = np.asarray(target, float) - eye
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.95 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, eye
    return m


def ring_cameras(n, distance=2.5, spread=0.5, seed=5):
    """n OpenCV camera-to-world poses at `distance` from the origin, within `spread` rad of +z, looking at the origin."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        t, p = (0.0, 0.0) if k == 0 else (spread * np.sqrt(rng.random()), 2 * np.pi * rng.random())
        out.append(look_at_c2w(distance * np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])))
    return np.stack(out)


def w2c32(c2w):
    from gaussmart_amd.mesh_visibility import w2c_from_c2w
    return w2c_from_c2w(c2w, opengl=False)


_CACHE = {}


def two_sphere_scene():
    """2,392 triangles: a sphere of radius 0.5 in front of, and partly hiding, one of radius 0.7 (occlusion, silhouettes);
    three views.  dict(verts, tris, w2c)."""
    if "two" not in _CACHE:
        v, t = join(uv_sphere(26, 24, 0.5, (-0.25, 0.05, 0.45)), uv_sphere(26, 24, 0.7, (0.3, -0.1, -0.4)))
        _CACHE["two"] = dict(verts=v, tris=t, w2c=w2c32(ring_cameras(3, seed=11)))
    return _CACHE["two"]


def subpixel_scene():
    """80,000 triangles on the same two spheres: at 96 x 64 and f = 60 most of them cover no pixel centre."""
    if "sub" not in _CACHE:
        v, t = join(uv_sphere(200, 101, 0.5, (-0.25, 0.05, 0.45)), uv_sphere(200, 101, 0.7, (0.3, -0.1, -0.4)))
        _CACHE["sub"] = dict(verts=v, tris=t, w2c=w2c32(ring_cameras(3, seed=11)))
    return _CACHE["sub"]


def intrinsics(H, W, f):
    return (float(f), float(f) * 1.03, W / 2 - 0.3, H / 2 + 0.2)


def vote_scene():
    """Two nested spheres (radius 1 and 0.6) of 2,000 vertices each, eight 96 x 72 views at distance 2.5 within 0.5 rad of +z,
    f = 100.  The inner sphere is hidden; of the outer one each view sees the near cap.  dict(verts, tris, w2c, H, W, intr)."""
    if "vote" not in _CACHE:
        v, t = join(uv_sphere(54, 38, 1.0), uv_sphere(54, 38, 0.6))
        _CACHE["vote"] = dict(verts=v, tris=t, w2c=w2c32(ring_cameras(8, seed=7)), H=72, W=96, intr=intrinsics(72, 96, 100.0))
    return _CACHE["vote"]


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def measure_px(verts, w2c, H, W, intr):
    """Largest |float32 - float64| of VIS_PROJECT's (u, v) over the pairs within one pixel of the frame."""
    worst = 0.0
    for m in w2c:
        u64, v64, z64 = project(verts, m, intr)
        u32, v32, _ = project(verts, m, intr, np.float32)
        with np.errstate(all="ignore"):
            near = (u64 > -1) & (u64 < W) & (v64 > -1) & (v64 < H) & (z64 > 0)
            d = np.maximum(np.abs(u32 - u64), np.abs(v32 - v64))
        if near.any():
            worst = max(worst, float(d[near].max()))
    return worst


def measure_rel(verts, tris, w2c, H, W, intr):
    """Largest relative depth difference raster_np(float32) against raster64 where both hit the same triangle."""
    worst = 0.0
    for m in w2c:
        d64, t64 = raster64(verts, tris, m, H, W, intr)
        d32, t32 = raster_np(verts, tris, m, H, W, intr, dtype=np.float32)
        same = (t64 >= 0) & (t64 == t32)
        if same.any():
            worst = max(worst, float((np.abs(d32[same].astype(np.float64) - d64[same]) / d64[same]).max()))
    return worst
