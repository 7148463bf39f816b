"""What the mesh-culling tests hold gaussmart_amd.mesh_cull to (helper, no tests):

  * restate64          the rules CULL_MASK_BINARISE ... CULL_TO_WORLD of include/gsr.h in float64 (the dilation with
                       scipy.ndimage.binary_dilation and the disk dx^2 + dy^2 <= r^2);
  * reference_torch32  the reference's own expression (scripts/eval_dtu/evaluate_single_scene.py: cull_scan) in torch float32
                       on the CPU: K4 @ inverse(pose) @ verts from a decomposition of P, the normalisation, the real
                       F.grid_sample on the scipy dilation.  scipy.linalg.rq stands where the reference calls
                       cv2.decomposeProjectionMatrix;
  * stable_vertices    which vertices a comparison may be held to: a (vertex, view) pair is stable when the vote of CULL_VOTE
                       is the same at the four positions (cx +- DELTA, cy +- DELTA) around its float64 pixel position, each with
                       its own validity test; a vertex is stable when every view is stable or some stable view removes it;
  * the fixtures of tests/test_mesh_cull_cpu.py and tests/test_gpu_mesh_cull.py.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from scipy import linalg, ndimage

# 4 x the largest pixel-coordinate difference between reference_torch32 and restate64 over the fixtures' own (vertex, view)
# pairs that lie within one pixel of the frame (elsewhere both call the pair invalid, whatever the position).  The factor 4:
# the device sums in another order than torch's matmul.  Measured (tests/test_mesh_cull_cpu.py prints and checks it):
# hemisphere fixture 5.6e-5 px, vote fixture 7.6e-5 px (mask pixels, 320 wide; the largest is a vertex 0.3 in front of the
# camera that sits inside the sphere) -> 4 x 7.6e-5 = 3.04e-4.
MEASURED_F32_VS_F64 = 7.6e-5
DELTA = 3.1e-4


# ---------------------------------------------------------------- rules 1, 2
def disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return x * x + y * y <= r * r


def dilate_ref(masks, r):
    masks = np.asarray(masks)
    return np.stack([ndimage.binary_dilation(m != 0, structure=disk(r)) for m in masks]).astype(np.uint8) \
        if len(masks) else np.zeros(masks.shape, np.uint8)


# ---------------------------------------------------------------- rules 3 - 5 in float64
def pixel_positions64(verts, proj, mask_hw, norm_hw):
    """Continuous mask-pixel position (cx, cy) [n,V] float64 of every (view, vertex): cx = (gx + 1) / 2 (W - 1)."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    P = np.asarray(proj, np.float32).astype(np.float64).reshape(-1, 3, 4)
    (H, W), (Hn, Wn) = mask_hw, norm_hw
    with np.errstate(all="ignore"):
        p = np.einsum("nij,vj->niv", P[:, :, :3], v) + P[:, :, 3:4]
        den = p[:, 2] + np.float64(np.float32(1e-6))
        gx = (p[:, 0] / den / (Wn - 1) - 0.5) * 2
        gy = (p[:, 1] / den / (Hn - 1) - 0.5) * 2
        return (gx + 1) / 2 * (W - 1), (gy + 1) / 2 * (H - 1)


def vote_at(cx, cy, dilated):
    """CULL_SAMPLE + CULL_VOTE per (view, vertex) at the mask-pixel positions (cx, cy) [n,V]: (keeps, valid, sample).  In mask
    pixels the validity test -1 < gx < 1 reads 0 < cx < W - 1."""
    n, H, W = dilated.shape
    with np.errstate(all="ignore"):
        valid = (cx > 0) & (cx < W - 1) & (cy > 0) & (cy < H - 1)
        ix, iy = np.rint(cx), np.rint(cy)
        inside = valid & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
    sample = np.zeros(cx.shape, bool)
    vi, pi = np.nonzero(inside)
    sample[vi, pi] = dilated[vi, iy[vi, pi].astype(np.int64), ix[vi, pi].astype(np.int64)] != 0
    return sample | ~valid, valid, sample


def restate64(verts, proj, masks, radius, norm_hw=None):
    """dict(keep [V], cx, cy, keeps [n,V], valid, sample, dilated): rules 1 - 5 in float64."""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    norm_hw = (H, W) if norm_hw is None else norm_hw
    dil = dilate_ref(masks, radius)
    cx, cy = pixel_positions64(verts, proj, (H, W), norm_hw)
    keeps, valid, sample = vote_at(cx, cy, dil)
    return dict(keep=keeps.all(0), cx=cx, cy=cy, keeps=keeps, valid=valid, sample=sample, dilated=dil)


def stable_vertices(r64, delta=DELTA):
    """bool [V] per the rule in this file's docstring."""
    cx, cy, dil = r64["cx"], r64["cy"], r64["dilated"]
    stable = np.ones(cx.shape, bool)
    first = None
    for sx in (-delta, delta):
        for sy in (-delta, delta):
            k = vote_at(cx + sx, cy + sy, dil)[0]
            first = k if first is None else first
            stable &= k == first
    removes = stable & ~r64["keeps"]
    return stable.all(0) | removes.any(0)


def compact_ref(verts, colors, tris, keep, scale=None, offset=None):
    """Rules 6 and 7 in plain numpy: (vertices f32, colours f32, triangles i32); the product v s + t in float64, rounded once."""
    keep = np.asarray(keep, bool)
    tk = keep[tris].all(1) if len(tris) else np.zeros(0, bool)
    remap = np.cumsum(keep) - 1
    v = verts[keep]
    if scale is not None or offset is not None:
        s = np.float64(np.float32(1.0 if scale is None else scale))
        t = np.zeros(3) if offset is None else np.asarray(offset, np.float32).astype(np.float64)
        v = (v.astype(np.float64) * s + t).astype(np.float32)
    return v, colors[keep], remap[tris[tk]].reshape(-1, 3).astype(np.int32)


# ---------------------------------------------------------------- the reference's expression in torch float32
def decompose_P(P):
    """K (positive diagonal, K[2,2] = 1 after the division), camera-to-world pose: load_K_Rt_from_P with scipy.linalg.rq in the
    place of cv2.decomposeProjectionMatrix.  float64 4x4 intrinsics and pose."""
    P = np.asarray(P, np.float64)
    K, R = linalg.rq(P[:, :3])
    S = np.diag(np.sign(np.diag(K)))
    K, R = K @ S, S @ R
    c = -np.linalg.solve(P[:, :3], P[:, 3])          # camera centre
    intr = np.eye(4)
    intr[:3, :3] = K / K[2, 2]
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R.T, c
    return intr, pose


def reference_torch32(verts, world_mats, scale_mats, masks, radius, norm_hw=None):
    """(keep bool [V], cx, cy [n,V]) by the arithmetic of the reference's cull_scan, restated: everything in torch float32 on the
    CPU, in the reference's order of operations --
      homogeneous vertices [4,V];  (K4 @ inverse(pose)) @ vertices with torch's matmul;  x, y divided by (z + 1e-6);
      x / (Wn - 1), y / (Hn - 1);  (g - 0.5) * 2;  valid = -1 < g < 1 on both axes;
      torch's grid_sample (nearest, zero padding, align_corners) on the dilated mask;  a view's vote = sample + (1 - valid) > 0."""
    masks = np.asarray(masks)
    n_views, H, W = masks.shape
    Hn, Wn = (H, W) if norm_hw is None else norm_hw
    xyz = torch.from_numpy(np.ascontiguousarray(verts, np.float32))
    n_verts = xyz.shape[0]
    homog = torch.ones((4, n_verts), dtype=torch.float32)
    homog[:3] = xyz.T
    dilated = dilate_ref(masks, radius)
    votes = torch.ones((n_views, n_verts), dtype=torch.bool)
    cx = np.zeros((n_views, n_verts))
    cy = np.zeros((n_views, n_verts))
    for view in range(n_views):
        P32 = (np.asarray(world_mats[view], np.float32) @ np.asarray(scale_mats[view], np.float32))[:3, :4]
        K4, c2w = decompose_P(P32)
        K4 = torch.tensor(K4, dtype=torch.float32)
        world_to_cam = torch.linalg.inv(torch.tensor(c2w.astype(np.float32)))
        projected = torch.matmul(torch.matmul(K4, world_to_cam), homog)
        depth = projected[2] + 1e-6
        grid = torch.stack((projected[0] / depth, projected[1] / depth), dim=1)         # [V,2] pixel coordinates
        grid[:, 0] = grid[:, 0] / (Wn - 1)
        grid[:, 1] = grid[:, 1] / (Hn - 1)
        grid = (grid - 0.5) * 2
        in_frame = (grid[:, 0] > -1) & (grid[:, 0] < 1) & (grid[:, 1] > -1) & (grid[:, 1] < 1)
        image = torch.from_numpy(dilated[view].astype(np.float32)).reshape(1, 1, H, W)
        sample = F.grid_sample(image, grid.reshape(1, 1, n_verts, 2), mode="nearest", padding_mode="zeros",
                               align_corners=True).reshape(n_verts)
        votes[view] = (sample + (1 - in_frame.float())) > 0
        cx[view] = ((grid[:, 0].double() + 1) / 2 * (W - 1)).numpy()
        cy[view] = ((grid[:, 1].double() + 1) / 2 * (H - 1)).numpy()
    return votes.all(dim=0).numpy(), cx, cy


def measured_delta(r64, cx32, cy32):
    """Largest |float32 - float64| pixel-coordinate difference over the pairs within one pixel of the frame."""
    n, H, W = r64["dilated"].shape
    cx, cy = r64["cx"], r64["cy"]
    with np.errstate(all="ignore"):
        near = (cx > -1) & (cx < W) & (cy > -1) & (cy < H)
        d = np.maximum(np.abs(cx32 - cx), np.abs(cy32 - cy))
    return float(d[near].max()) if near.any() else 0.0


# ---------------------------------------------------------------- fixtures
def fib(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def look_at_w2c(eye, target):
    eye = np.asarray(eye, float)
    fwd = np.asarray(target, float) - eye
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.95 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], 0)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ eye
    return w2c


def world_mat(f, W, H, w2c, factor=1.0):
    """DTU's world_mat: [K [R|t]; 0 0 0 1] up to a factor (any multiple of P is the same camera)."""
    K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1.0]])
    M = np.eye(4)
    M[:3, :4] = factor * (K @ w2c[:3, :4])
    return M.astype(np.float32)


def ellipse_mask(H, W, cx, cy, a, b, value=255):
    y, x = np.mgrid[0:H, 0:W]
    return (((x - cx) / a) ** 2 + ((y - cy) / b) ** 2 <= 1).astype(np.uint8) * np.uint8(value)


def sphere_vertices(n=6000, radius=0.5, seed=3):
    """n Fibonacci points on a sphere in a fixed shuffled order (every prefix is spread over the whole sphere)."""
    return (radius * fib(n))[np.random.default_rng(seed).permutation(n)].astype(np.float32)


def projections(world_mats, scale_mats):
    from gaussmart_amd.mesh_cull import dtu_projection
    return np.stack([dtu_projection(w, s) for w, s in zip(world_mats, scale_mats)]) if len(world_mats) \
        else np.zeros((0, 3, 4), np.float32)


_CACHE = {}


def hemisphere_fixture():
    """The CPU fixture: 6,000 vertices on a sphere of radius 0.5, eight 320 x 240 views at distance 2.5 clustered around +z,
    ellipse masks of 30 x 22 px half-axes, r = 24.  dict(verts, world_mats, scale_mats, proj, masks, radius)."""
    if "hemi" not in _CACHE:
        W, H, f = 320, 240, 340.0
        dirs = [np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])
                for t, p in [(0.0, 0.0)] + [(0.2, 2 * np.pi * k / 7) for k in range(7)]]
        wms = [world_mat(f, W, H, look_at_w2c(2.5 * d, [0, 0, 0]), factor=(1.0, 3.7, 0.02, 250.0)[i % 4]) for i, d in enumerate(dirs)]
        sms = [np.eye(4, dtype=np.float32)] * len(wms)
        masks = np.stack([ellipse_mask(H, W, (W - 1) / 2, (H - 1) / 2, 30, 22) for _ in wms])
        _CACHE["hemi"] = dict(verts=sphere_vertices(), world_mats=wms, scale_mats=sms, proj=projections(wms, sms), masks=masks,
                              radius=24, norm_hw=None)
    return _CACHE["hemi"]


def vote_fixture():
    """The device vote fixture: the same sphere with vertex 0 made NaN and vertex 1 infinite; eight views of a 640 x 480 camera
    (norm_size) whose masks are 320 x 240; view 0 regular, view 1 looks past the sphere (part of it outside the frame), view 2
    sits inside the sphere (part of it behind the camera), the others regular from other sides; r = 24."""
    if "vote" not in _CACHE:
        Wn, Hn, W, H, f = 640, 480, 320, 240, 680.0
        verts = sphere_vertices().copy()
        verts[0, 0] = np.nan
        verts[1, 2] = np.inf
        cams = [look_at_w2c([0, 0, 2.5], [0, 0, 0]), look_at_w2c([0.3, 0, 2.5], [1.0, 0.2, 0]),
                look_at_w2c([0, 0.05, -0.2], [0, 0, 1.0])]
        cams += [look_at_w2c(2.5 * np.array(d), [0, 0, 0]) for d in
                 ([0.3, 0.1, 0.95], [-0.2, 0.25, 0.95], [0.1, -0.3, 0.95], [-0.3, -0.2, 0.93], [0.25, 0.3, 0.92])]
        wms = [world_mat(f, Wn, Hn, c, factor=(1.0, 0.5, 7.0)[i % 3]) for i, c in enumerate(cams)]
        sms = [np.eye(4, dtype=np.float32)] * len(wms)
        masks = np.stack([ellipse_mask(H, W, (W - 1) / 2, (H - 1) / 2, 30, 22, value=(255, 1, 128)[i % 3]) for i in range(len(wms))])
        masks[1] = ellipse_mask(H, W, 40, 100, 45, 60)             # where view 1 sees the sphere's edge
        masks[2] = ellipse_mask(H, W, (W - 1) / 2, (H - 1) / 2, 120, 90, value=7)
        _CACHE["vote"] = dict(verts=verts, world_mats=wms, scale_mats=sms, proj=projections(wms, sms), masks=masks, radius=24,
                              norm_hw=(Hn, Wn))
    return _CACHE["vote"]


def fixture_restated(name):
    """restate64 of a fixture (all its views), computed once."""
    key = name + "_r64"
    if key not in _CACHE:
        fx = {"hemi": hemisphere_fixture, "vote": vote_fixture}[name]()
        _CACHE[key] = restate64(fx["verts"], fx["proj"], fx["masks"], fx["radius"], fx["norm_hw"])
    return _CACHE[key]


def neighbour_triangles(verts):
    """One triangle (v, nearest, second nearest) per finite vertex, int32 [F,3]: a mesh whose triangles are spatially coherent,
    so that a cull keeps a good part of them."""
    from scipy.spatial import cKDTree
    ok = np.nonzero(np.isfinite(verts).all(1))[0]
    _, nn = cKDTree(verts[ok]).query(verts[ok], k=3)
    return ok[nn].astype(np.int32)


def write_dtu_dir(root, scan_id, world_mats, scale_mats, masks, rgb=(True, False)):
    """root/scan<id>/cameras.npz and mask/NNN.png (RGB when rgb[i % len(rgb)], single-channel otherwise)."""
    from PIL import Image
    d = os.path.join(str(root), f"scan{scan_id}")
    os.makedirs(os.path.join(d, "mask"), exist_ok=True)
    cams = {}
    for i, (w, s) in enumerate(zip(world_mats, scale_mats)):
        cams[f"world_mat_{i}"], cams[f"scale_mat_{i}"] = np.asarray(w, np.float64), np.asarray(s, np.float64)
        cams[f"world_mat_inv_{i}"] = np.linalg.inv(cams[f"world_mat_{i}"])
    np.savez(os.path.join(d, "cameras.npz"), **cams)
    for i, m in enumerate(masks):
        img = np.repeat(m[:, :, None], 3, 2) if rgb[i % len(rgb)] else m
        if img.ndim == 3:
            img = img.copy()
            img[..., 1:] = 0          # only channel 0 carries the mask
        Image.fromarray(img).save(os.path.join(d, "mask", f"{i:03d}.png"))
    return d


# ---------------------------------------------------------------- dilation cases
DILATE_SIZES = [(1, 1), (10, 300), (97, 150), (240, 320), (64, 64)]
DILATE_RADII = [0, 1, 5, 24, 127]
# scipy's binary_dilation visits the whole (2r + 1)^2 footprint for every pixel without a set neighbour: 16 ns a visit, a
# minute for one empty 320 x 240 image at r = 127.  Cases above this many visits per image are compared with scipy's result
# recorded in tests/golden/mesh_cull_dilate.npz (tests/golden/make_golden_mesh_cull.py writes it with the same call); the others
# run scipy in the test.
DILATE_LIVE_VISITS = 5e7
DILATE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_cull_dilate.npz")


def dilation_images(H, W):
    """uint8 [6,H,W]: all zero; all set; single pixels in each corner and on each border; a checkerboard; random blobs; set
    pixels with values other than 0 / 1."""
    rng = np.random.default_rng(1000 * H + W)
    m = np.zeros((6, H, W), np.uint8)
    m[1] = 1
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)):
        m[2, y, x] = 1
    m[3] = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8)
    for _ in range(4):
        cy, cx, a, b = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, 0.2 * W + 2), rng.uniform(1, 0.2 * H + 2)
        m[4] |= ellipse_mask(H, W, cx, cy, a, b, value=1)
    m[5] = np.where(rng.random((H, W)) < 0.01, rng.integers(2, 256, (H, W)), 0).astype(np.uint8)
    return m


def dilation_case_is_live(H, W, r):
    return H * W * (2 * r + 1) ** 2 <= DILATE_LIVE_VISITS


def dilation_expected(H, W, r):
    """scipy.ndimage.binary_dilation of dilation_images(H, W) with disk(r): computed here, or scipy's recorded result."""
    key = ("dil", H, W, r)
    if key not in _CACHE:
        imgs = dilation_images(H, W)
        if dilation_case_is_live(H, W, r):
            _CACHE[key] = dilate_ref(imgs, r)
        else:
            import zlib
            with np.load(DILATE_GOLDEN) as g:
                name = f"{H}x{W}_r{r}"
                assert int(g[name + "_input_crc"]) == zlib.crc32(imgs.tobytes()), "dilation_images changed: regenerate the golden file"
                _CACHE[key] = np.unpackbits(g[name])[:imgs.size].reshape(imgs.shape)
    return _CACHE[key]
