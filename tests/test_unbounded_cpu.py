"""Unbounded mesh export without a device: the fp32 host twins of gaussmart_amd/mesh_unbounded.py against the restatement of
the reference (tests/unbounded_ref.py), quantile_radius against np.quantile, the single-lattice rule against the reference's
per-crop torch.linspace, the UNB_ALLOC set on synthetic flag grids, argument rejection of the gsr_unb_* C ABI, and
UnboundedExtractor routed to the twins on a CPU model.

No golden file of the reference's own extract_mesh_unbounded exists: utils/mesh_utils.py imports Open3D at the top and calls
.cuda(), so it cannot run where these fixtures were made.  The restatement stands in for it."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from gaussmart_amd import _lib
from gaussmart_amd import mesh_unbounded as MU
from gaussmart_amd.mesh import GaussianExtractor, TriangleMesh
import unbounded_ref as UR

R_PAR, RES_PAR, CROP_PAR = 1.9, 48, 24
VS_PAR = 2 * UR.RADIUS / RES_PAR


@pytest.fixture(scope="module")
def parity():
    views = UR.parity_views()
    pts = UR.lattice_points(R_PAR, RES_PAR, CROP_PAR)
    f32, c32, u32 = UR.field(pts, views, UR.CENTER, UR.RADIUS, VS_PAR, dtype=torch.float32)
    f64, c64, u64 = UR.field(pts, views, UR.CENTER, UR.RADIUS, VS_PAR, dtype=torch.float64)
    return dict(views=views, pts=pts, f32=f32, f64=f64, c64=c64, stable=~(u32 | u64))


def test_fixture_is_usable(parity):
    """The conditions the GPU parity test relies on, checked on the fp32 restatement alone: every regime of the contraction
    occurs, both signs occur, at most 1 % of the lattice is unstable, no NaN leaves the field, and no stable point changes
    sign between fp32 and fp64."""
    m = parity["pts"].norm(dim=-1)
    assert (m < 1).any() and ((m > 1) & (m < 1.9)).any() and ((m > 1.9) & (m < 2)).any() and (m > 2).any()
    st = parity["stable"]
    assert (~st).float().mean() <= 0.01
    assert torch.isfinite(parity["f32"]).all() and torch.isfinite(parity["f64"]).all()
    assert (parity["f64"] < 0).sum() > 1000 and (parity["f64"] == 1).sum() > 1000
    assert not ((parity["f32"] < 0) != (parity["f64"] < 0))[st].any()


def test_host_twin_matches_restatement(parity):
    """Bar: 16 x e_ref, e_ref = max |fp32 restatement - fp64 restatement| on the stable points (the factor the suite gives an
    fp32 implementation over a measured fp32 floor, as tests/test_gpu_tnt_eval.py)."""
    st = parity["stable"]
    e_ref = float((parity["f32"].double() - parity["f64"])[st].abs().max())
    f, c = MU.unbounded_field_host(parity["pts"], parity["views"], UR.CENTER, UR.RADIUS, VS_PAR, return_rgb=True)
    err = float((f.double() - parity["f64"])[st].abs().max())
    err_c = float((c.double() - parity["c64"])[st].abs().max())
    print(f"host twin: e_ref {e_ref:.3e}, twin vs fp64 {err:.3e}, rgb {err_c:.3e}")
    assert 0 < e_ref < 1e-3
    assert err <= 16 * e_ref and err_c <= 16 * e_ref
    assert torch.isfinite(f).all() and torch.isfinite(c).all()
    G = len(UR.lattice_coords(R_PAR, RES_PAR, CROP_PAR))
    box = MU.lattice_field_host(R_PAR, RES_PAR, CROP_PAR, (3, 20, 30), (5, 9, 17), parity["views"], UR.CENTER, UR.RADIUS)
    assert torch.equal(box, f.reshape(G, G, G)[3:8, 20:29, 30:47])


def test_host_twin_world_points(parity):
    """contracted=False: world points, plain truncation, colours."""
    g = torch.Generator().manual_seed(3)
    pts = (torch.rand((4000, 3), generator=g) - 0.5) * 2.4
    f64, c64, u64 = UR.field(pts, parity["views"], UR.CENTER, UR.RADIUS, VS_PAR, contracted=False, dtype=torch.float64)
    f32, c32, u32 = UR.field(pts, parity["views"], UR.CENTER, UR.RADIUS, VS_PAR, contracted=False, dtype=torch.float32)
    st = ~(u32 | u64)
    e_ref = max(float((f32.double() - f64)[st].abs().max()), float((c32.double() - c64)[st].abs().max()))
    f, c = MU.unbounded_field_host(pts, parity["views"], UR.CENTER, UR.RADIUS, VS_PAR, contracted=False, return_rgb=True)
    assert float((f.double() - f64)[st].abs().max()) <= 16 * e_ref
    assert float((c.double() - c64)[st].abs().max()) <= 16 * e_ref
    assert (c64.sum(1) > 0).sum() > 100


def test_contract_roundtrip_and_edge_magnitudes():
    x = torch.tensor([[0.3, 0.1, -0.2], [3.0, -4.0, 12.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    assert torch.allclose(MU.uncontract(MU.contract(x)), x, atol=1e-12)
    y = torch.tensor([[2.0, 0.0, 0.0], [0.0, 2.5, 0.0]])
    out = MU.uncontract(y)
    assert not torch.isfinite(out[0]).all()              # m == 2: torch's arithmetic gives a non-finite point
    assert torch.isfinite(out[1]).all() and out[1, 1] < 0    # m > 2: a mirrored point


def test_quantile_radius():
    g = torch.Generator().manual_seed(1)
    for n in (1, 2, 7, 1000, 4001):
        xyz = torch.randn((n, 3), generator=g) * 2.0
        c, r = torch.tensor([0.1, -0.2, 0.3]), 1.7
        norms = UR.contract((xyz - c) / r).norm(dim=-1).numpy()
        want = min(float(np.quantile(norms, q=0.95)) + 0.01, 1.9)
        got = MU.quantile_radius(xyz, c, r)
        # np.quantile of a float32 array interpolates in float32 or float64 depending on the numpy version: one f32 rounding
        assert abs(got - want) <= 2.0 ** -23 * 2.0, (n, got, want)
    far = torch.full((10, 3), 50.0)
    assert MU.quantile_radius(far, (0, 0, 0), 1.0) == 1.9
    with pytest.raises(ValueError):
        MU.quantile_radius(torch.zeros((0, 3)), (0, 0, 0), 1.0)


@pytest.mark.parametrize("R,resolution,crop", [(1.5, 64, 32), (1.9, 48, 24), (0.8, 30, 10)])
def test_lattice_is_the_union_of_the_crops(R, resolution, crop):
    """UNB_LATTICE against the reference's construction: np.linspace crop bounds, torch.linspace(x_min, x_max, crop) per crop.
    The crops share their boundary points, and every crop coordinate is the lattice coordinate to within the roundings of the
    fp32 linspace: half an ulp of its result, half an ulp of the lattice's, and the fp32 step's error (half an ulp of the
    step) carried over at most crop / 2 steps (torch.linspace runs from both ends).  |s| < 2, so ulp = 2^-23 * 2 at most."""
    n = resolution // crop
    s = MU.lattice_coords(R, resolution, crop)
    G, nb = MU.lattice_size(resolution, crop)
    assert len(s) == G == n * (crop - 1) + 1 and nb == -(-G // 16)
    assert torch.equal(s, UR.lattice_coords(R, resolution, crop))
    xs = np.linspace(-R, R, n + 1)
    step = 2 * R / (G - 1)
    ulp = 2.0 ** -23 * (2.0 if R > 1 else 1.0)
    bound = ulp + (crop / 2) * (2.0 ** -24 * 2.0 ** math.ceil(math.log2(step)))
    worst = 0.0
    for i in range(n):
        c = torch.linspace(xs[i], xs[i + 1], crop)
        mine = s[i * (crop - 1): i * (crop - 1) + crop]
        worst = max(worst, float((c.double() - mine.double()).abs().max()))
    print(f"lattice vs per-crop linspace: worst difference {worst:.2e}, bound {bound:.2e}")
    assert worst <= bound
    assert s[0] == np.float32(-R) and s[-1] == np.float32(R)


def _alloc_brute(flags):
    nx, ny, nz = flags.shape
    get = lambda x, y, z: int(flags[x, y, z]) if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz else 0
    offs = list(itertools.product((0, 1), repeat=3))
    anchor = np.zeros(flags.shape, bool)
    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):
        u = 0
        for o in offs:
            u |= get(x + o[0], y + o[1], z + o[2])
        anchor[x, y, z] = u == 3
    alloc = np.zeros(flags.shape, bool)
    for x, y, z in zip(*np.nonzero(anchor)):
        for o in offs:
            if x + o[0] < nx and y + o[1] < ny and z + o[2] < nz:
                alloc[x + o[0], y + o[1], z + o[2]] = True
    return alloc


def test_alloc_set_on_synthetic_flags():
    rng = np.random.default_rng(5)
    for shape, p in (((3, 3, 3), 0.3), ((5, 4, 6), 0.1), ((4, 4, 4), 0.9)):
        flags = np.where(rng.random(shape) < p, 1, 2).astype(np.uint8)
        flags[rng.random(shape) < 0.2] = 3
        assert np.array_equal(MU.alloc_set_host(flags), _alloc_brute(flags))
    one_sign = np.full((3, 3, 3), 2, np.uint8)
    assert not MU.alloc_set_host(one_sign).any()
    # the only sign change lies between block (1,1,1) and block (2,1,1): anchors are the blocks whose +{0,1}^3 holds both
    f = np.full((4, 4, 4), 2, np.uint8)
    f[2, 1, 1] = 1
    alloc = MU.alloc_set_host(f)
    want = np.zeros((4, 4, 4), bool)
    want[1:3, 0:2, 0:2] = True          # anchors (1..2, 0..1, 0..1) ...
    want[1:4, 0:3, 0:3] = True          # ... dilated by +{0,1}^3
    assert np.array_equal(alloc, want)
    # flags from a dense field: a sign change between voxel 15 of one block and voxel 0 of the next
    dense = torch.ones((40, 40, 40))
    dense[16:, :, :] = -1
    fl = MU.block_flags_of_dense(dense).numpy()
    assert (fl[0] == 2).all() and (fl[1:] == 1).all()
    assert MU.alloc_set_host(fl)[0:2].all() and not MU.alloc_set_host(fl)[2].any()


def test_c_entries_reject_bad_arguments():
    """Every check happens on the host before anything touches the device (GSR_E_INVALID = -1), so this runs without one."""
    L = _lib.lib()
    cen = (C.c_float * 3)(0, 0, 0)
    lo, dims, empty = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(2, 0, 2)
    fake = C.c_void_p(0x1000)   # never dereferenced: a later check fails first
    inval = -1
    assert L.gsr_unb_points(None, 1, fake, 4, cen, 1.0, 0.1, 1, fake, None, None) == inval
    assert "table" in L.gsr_last_error().decode()
    assert L.gsr_unb_points(fake, 0, fake, 4, cen, 1.0, 0.1, 1, fake, None, None) == inval
    assert "no views" in L.gsr_last_error().decode()
    assert L.gsr_unb_points(fake, 1, None, 4, cen, 1.0, 0.1, 1, fake, None, None) == inval
    assert L.gsr_unb_points(fake, 1, fake, 4, cen, 0.0, 0.1, 1, fake, None, None) == inval
    assert L.gsr_unb_points(fake, 1, fake, -1, cen, 1.0, 0.1, 1, fake, None, None) == inval
    assert L.gsr_unb_points(fake, 1, None, 0, cen, 1.0, 0.1, 1, None, None, None) == 0      # n == 0: nothing to do
    assert L.gsr_unb_lattice_box(None, 1, 1.5, 48, 24, lo, dims, cen, 1.0, 0.1, fake, None) == inval
    assert L.gsr_unb_lattice_box(fake, 1, 1.5, 50, 24, lo, dims, cen, 1.0, 0.1, fake, None) == inval
    assert "multiple of crop" in L.gsr_last_error().decode()
    assert L.gsr_unb_lattice_box(fake, 1, 1.5, 48, 24, lo, empty, cen, 1.0, 0.1, fake, None) == inval
    assert "empty box" in L.gsr_last_error().decode()
    assert L.gsr_unb_lattice_box(fake, 1, 1.5, 48, 24, (C.c_int32 * 3)(46, 0, 0), dims, cen, 1.0, 0.1, fake, None) == inval
    assert L.gsr_unb_lattice_box(fake, 0, 1.5, 48, 24, lo, dims, cen, 1.0, 0.1, fake, None) == inval
    assert L.gsr_unb_block_flags(None, 1, 1.5, 48, 24, cen, 1.0, 0.1, fake, None) == inval
    assert L.gsr_unb_block_flags(fake, 1, 1.5, 48, 7, cen, 1.0, 0.1, fake, None) == inval
    assert L.gsr_unb_block_flags(fake, 0, 1.5, 48, 24, cen, 1.0, 0.1, fake, None) == inval
    v = _lib.GsrTsdfVolume()
    v.voxel_size = v.sdf_trunc = 1.0
    v.block_hi[:] = (2, 2, 2)            # the lattice of (48, 24) needs [0, 3)^3
    assert L.gsr_unb_alloc(C.byref(v), 48, 24, fake, None) == inval
    assert L.gsr_unb_fill(C.byref(v), None, 1, 1.5, 48, 24, cen, 1.0, 0.1, None) == inval
    assert L.gsr_unb_fill(C.byref(v), fake, 1, 1.5, 48, 5, cen, 1.0, 0.1, None) == inval
    assert L.gsr_unb_finish(fake, 3, 1.5, 48, 5, cen, 1.0, 32.0, None) == inval
    assert L.gsr_unb_finish(None, 3, 1.5, 48, 24, cen, 1.0, 32.0, None) == inval
    g, nb = C.c_int32(), C.c_int32()
    assert L.gsr_unb_lattice_size(2048, 512, C.byref(g), C.byref(nb)) == 0 and (g.value, nb.value) == (2045, 128)
    assert L.gsr_unb_lattice_size(100, 512, C.byref(g), C.byref(nb)) == inval
    with pytest.raises(_lib.GsrError):
        MU.unbounded_field(torch.zeros((2, 3)), [], (0, 0, 0), 1.0, 0.1)     # CPU points: no quiet fall-back to torch


class _Cam:
    def __init__(self, eye, target, H, W, sc, sr):
        M, depth, rgb = UR.render_analytic(eye, target, 0.9, 0.9, H, W, sc, sr, holes=False, shell=8.0)
        _, V = UR.full_proj(eye, target, 0.9, 0.9)
        self.full_proj_transform = M
        self.world_view_transform = torch.from_numpy(V.astype(np.float32))
        self.depth, self.rgb = depth, rgb


class _Model:
    def __init__(self, xyz):
        self.get_xyz = xyz


def test_extractor_on_cpu_runs_the_twins():
    sc, sr = (0.0, 0.0, 0.0), 0.3       # smaller than the truncation (5 voxel_size = 0.39): no unobserved interior
    cams = []
    for i in range(8):
        a = 2 * math.pi * i / 8
        el = 0.3 if i % 2 else -0.5
        cams.append(_Cam((2.5 * math.cos(a) * math.cos(el), 2.5 * math.sin(a) * math.cos(el), 2.5 * math.sin(el)), sc, 40, 40,
                         sc, sr))
    g = torch.Generator().manual_seed(0)
    d = torch.randn((500, 3), generator=g)
    xyz = sr * d / d.norm(dim=1, keepdim=True)
    xyz[::5] *= 1.4                    # the 95 % quantile, and with it the lattice, reaches past the sphere
    model = _Model(xyz)
    render = lambda cam, gaussians, pipe, bg_color: {"render": cam.rgb, "surf_depth": cam.depth}
    ex = MU.UnboundedExtractor(model, render, None)
    ex.reconstruction(cams)
    mesh = ex.extract_mesh_unbounded(resolution=64, crop=32)
    assert isinstance(mesh, TriangleMesh) and len(mesh.triangles) > 100
    r = np.linalg.norm(mesh.vertices.astype(np.float64), axis=1)
    voxel = 2 * ex.radius / 64         # the reference's voxel_size (the lattice itself is finer: R < 1)
    assert np.abs(r - sr).max() < voxel, (np.abs(r - sr).max(), voxel)
    assert mesh.vertex_colors.min() >= 0 and mesh.vertex_colors.max() <= 1 and mesh.vertex_colors.max() > 0.2
    e = np.sort(np.concatenate([mesh.triangles[:, [0, 1]], mesh.triangles[:, [1, 2]], mesh.triangles[:, [2, 0]]]), 1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    assert (cnt == 2).all() and len(mesh.vertices) - len(ue) + len(mesh.triangles) == 2
    with pytest.raises(NotImplementedError, match="follow-up"):     # the base class keeps its stub
        GaussianExtractor.extract_mesh_unbounded(ex)
