"""loss.hip and regularizer.hip on the device, pixel by pixel, through the C ABI: gsr_loss_forward / _backward, gsr_regularizer_forward /
_backward / _backward_partials, gsr_surface_maps_forward / _backward and gsr_objective_finish against the fp64 twins of
tests/objective_cases.py, each quantity held to the bar derived there (tests/test_objective_cpu.py proves every bar reachable and
tight without a GPU).  Every output is pre-filled with NaN: a slot or a pixel nobody writes shows.
GSR_OBJECTIVE_PARITY_REPORT=<file>: the measured errors and bars are appended there (profiles/objective_parity.txt and
profiles/surface_maps_parity.txt are such runs)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import objective_cases as OC
from objective_cases import E, U32, TINY32, bar, ratio
from gaussmart_amd import _lib
from gaussmart_amd._dev import ptr, stream

pytestmark = pytest.mark.gpu


def report(line):
    out = os.environ.get("GSR_OBJECTIVE_PARITY_REPORT")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


@pytest.fixture
def held():
    """held(case, what, got, truth): max over the elements of |got - truth.v| / bar(truth) must be <= 1.  Every figure is printed
    before it is asserted; the case's worst quantity is reported -- one line per case -- whether the case holds or not."""
    rows = []

    def check(case, what, got, truth, where=None):
        got, want, b = got.detach().double().cpu(), truth.v, bar(truth)
        if where is not None:
            got, want, b = got[where], want[where], b[where]
        err = (got - want).abs()
        use = ratio(err, b)
        rows.append((use, what, float(err.max()) if err.numel() else 0.0, float(b.max()) if b.numel() else 0.0, case))
        print(f"{case} {what}: max err {rows[-1][2]:.3e}, max bar {rows[-1][3]:.3e}, worst err/bar {use:.3f}")
        assert bool(torch.isfinite(got).all()) and use <= 1.0, (case, what, use)

    yield check
    if rows:
        use, what, err, b, case = max(rows)
        report(f"{case}: {len(rows)} quantities, worst err/bar {use:.3f} at {what} (max err {err:.3e}, max bar {b:.3e})")


def nans(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ photometric loss
@pytest.mark.parametrize("content,shape", OC.LOSS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_loss_forward_and_backward_per_pixel(gpu_device, held, content, shape):
    L, dev = _lib.lib(), gpu_device
    Cn, H, W = shape
    name = f"loss {content} {Cn}x{H}x{W}"
    xh, yh = OC.loss_inputs(content, shape)
    x, y = xh.to(dev), yh.to(dev)
    fwd, bwd = OC.loss_truth(content, shape)
    n_slots = OC.num_slots(H, W)
    assert L.gsr_loss_num_partials(H, W) == 2 * n_slots
    maps, partials = nans((3, Cn, H, W), dev), nans((n_slots, 2), dev)
    _lib.check(L.gsr_loss_forward(ptr(x), ptr(y), Cn, H, W, ptr(maps), ptr(partials), stream(dev)))
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(maps).all()) and bool(torch.isfinite(partials).all())        # every pixel and every slot was written
    for k, what in enumerate(("dS/dmu1", "dS/dE[x2]", "dS/dE[xy]")):
        held(name, what, maps[k], fwd["maps"][k])
    g16y, g16x = -(-H // 16), -(-W // 16)
    slots = partials.reshape(g16y, g16x, 2).cpu()
    top_left = torch.zeros(g16y, g16x, dtype=torch.bool)
    top_left[::2, ::2] = True
    for k, what in enumerate(("sum S", "sum |x-y|")):
        held(name, f"{what} per tile", slots[..., k], fwd["slots"][k], where=top_left)
        assert bool((slots[..., k][~top_left] == 0.0).all()), what           # a tile's other cells hold exactly 0
        total = E(fwd["slots"][k].v.sum(), fwd["slots"][k].b.sum())
        held(name, f"{what} total", slots[..., k].double().sum(), total)

    same = (xh == yh)
    runs = {}
    for (lam, gs), truth in bwd.items():
        scale = torch.tensor([gs], dtype=torch.float32, device=dev)
        out = []
        for _ in range(2):
            dimg = nans((Cn, H, W), dev)
            _lib.check(L.gsr_loss_backward(ptr(x), ptr(y), ptr(maps), Cn, H, W, lam, ptr(scale), ptr(dimg), stream(dev)))
            out.append(dimg)
        torch.cuda.synchronize(dev)
        held(name, f"dimg lambda {lam} scale {gs}", out[0], truth)
        assert torch.equal(out[0], out[1])                                   # the same call twice: the same bits
        runs[(lam, gs)] = out[0].cpu()
    # sign(0) = 0: where x == y the L1 part is exactly absent.  With lambda = 0 nothing is left; otherwise what is left is the
    # lambda = 1 run's value times lambda: k_ssim = (-lambda / n) gs against (-1 / n) gs and one product each, five roundings
    if bool(same.any()):
        for gs in OC.LOSS_GRAD_SCALES:
            assert float(runs[(0.0, gs)][same].abs().max()) == 0.0
            ref = OC.f32(0.2) * runs[(1.0, gs)][same].double()
            assert bool(((runs[(0.2, gs)][same].double() - ref).abs() <= 6 * U32 * ref.abs() + TINY32).all())


# ------------------------------------------------------------------------------------------------ surface regularizers
@pytest.mark.parametrize("case", OC.REG_CASES, ids=OC.reg_case_id)
def test_regularizer_forward_and_backward_per_pixel(gpu_device, held, case):
    L, dev = _lib.lib(), gpu_device
    kind, size, r, (ln, ld) = case
    H, W = size
    name = "reg " + OC.reg_case_id(case)
    amh = OC.reg_allmap(kind, size)
    am = amh.to(dev)
    kinv = (C.c_float * 9)(*OC.reg_kinv(size).reshape(-1).tolist())
    truth = OC.reg_truth(case)
    n_slots = OC.num_slots(H, W)
    gs = OC.REG_GRAD_SCALE
    scale = torch.tensor([gs], dtype=torch.float32, device=dev)
    p_fwd, p_bwd = nans((n_slots, 2), dev), nans((n_slots, 2), dev)
    dam, dam_p = nans((7, H, W), dev), nans((7, H, W), dev)
    _lib.check(L.gsr_regularizer_forward(ptr(am), H, W, kinv, r, ptr(p_fwd), stream(dev)))
    _lib.check(L.gsr_regularizer_backward(ptr(am), H, W, kinv, r, ln, ld, ptr(scale), ptr(dam), stream(dev)))
    _lib.check(L.gsr_regularizer_backward_partials(ptr(am), H, W, kinv, r, ln, ld, ptr(scale), ptr(dam_p), ptr(p_bwd), stream(dev)))
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(p_fwd).all()) and bool(torch.isfinite(dam).all())             # every slot, every pixel, holes included
    assert torch.equal(p_fwd, p_bwd) and torch.equal(dam, dam_p)
    slots = p_fwd.reshape(-(-H // 16), -(-W // 16), 2).cpu()
    held(name, "sum error per tile", slots[..., 0], truth["sums"][0])
    held(name, "sum distortion per tile", slots[..., 1], truth["sums"][1])
    lit = amh[1] > 0
    got = dam.cpu()
    for c in range(7):
        held(name, f"d_allmap[{c}] lit", got[c], truth["dam"][c], where=lit)
        held(name, f"d_allmap[{c}] holes", got[c], truth["dam"][c], where=~lit)
    # the contract at pixels without a splat: (finite, above) zero in channels 0 and 1, channel 6 = kd -- at every pixel, to the bit
    assert float(got[0][~lit].abs().sum()) == 0.0 and float(got[1][~lit].abs().sum()) == 0.0
    kd = np.float32(np.float32(ld) * (np.float32(1.0) / (np.float32(W) * np.float32(H)))) * np.float32(gs)
    assert bool((got[6] == float(kd)).all())
    if kind == "island":
        # the lit pixel's cross product is exactly 0 (all four neighbours are holes): reg_bwd_kernel hands nothing to them
        assert float(got[[0, 1, 5]].abs().sum()) == 0.0
    if kind == "micro":
        # a lit surface whose every cross product is below 1e-12: the same, at every pixel
        assert float(got[[0, 1, 5]].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ surface maps
def _c9(t):
    return (C.c_float * 9)(*t.reshape(-1).tolist())


def _maps_forward(L, am, rays, rot, r):
    out = nans(tuple(am.shape), am.device)
    _, H, W = am.shape
    _lib.check(L.gsr_surface_maps_forward(ptr(am), H, W, rays, rot, r, ptr(out), stream(am.device)))
    return out


def _maps_backward(L, am, rays, rot, r, gout):
    dam = nans(tuple(am.shape), am.device)
    _, H, W = am.shape
    _lib.check(L.gsr_surface_maps_backward(ptr(am), H, W, rays, rot, r, ptr(gout), ptr(dam), stream(am.device)))
    return dam


@pytest.mark.parametrize("case", OC.MAPS_CASES, ids=OC.maps_case_id)
def test_surface_maps_forward_and_backward_per_pixel(gpu_device, held, case):
    L, dev = _lib.lib(), gpu_device
    kind, size, r, _ = case
    H, W = size
    name = "maps " + OC.maps_case_id(case)
    amh, gh = OC.reg_allmap(kind, size), OC.maps_gout(case)
    am, gout = amh.to(dev), gh.to(dev)
    rays, rot = (_c9(t) for t in OC.maps_rays(size))
    truth = OC.maps_truth(case)
    outs = [_maps_forward(L, am, rays, rot, r) for _ in range(2)]
    dams = [_maps_backward(L, am, rays, rot, r, gout) for _ in range(2)]
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(outs[0]).all()) and bool(torch.isfinite(dams[0]).all())      # every element was written
    assert torch.equal(outs[0], outs[1]) and torch.equal(dams[0], dams[1])                  # the same call twice: the same bits
    out, dam = outs[0].cpu(), dams[0].cpu()
    lit = amh[1] > 0
    for which, sel in (("lit", lit), ("holes", ~lit)):
        for c in range(7):
            held(name, f"out[{c}] {which}", out[c], truth["out"][c], where=sel)
            held(name, f"d_allmap[{c}] {which}", dam[c], truth["dam"][c], where=sel)
    # exact facts.  surf_normal is 0 on the border, everywhere when there is no interior; rend_dist is outside this node; no
    # gradient passes where there is no splat
    border = torch.ones(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        border[1:-1, 1:-1] = False
    assert float(out[4:7][:, border].abs().sum()) == 0.0
    assert float(dam[6].abs().sum()) == 0.0
    assert float(dam[0][~lit].abs().sum()) == 0.0 and float(dam[1][~lit].abs().sum()) == 0.0
    # surf_depth where D / A or the median is not a number the reference keeps: nan_to_num(., 0, 0) stands in, to the bit (one
    # of the two products is with an exact 0, so a contracted multiply-add gives the same bits)
    e, med = amh[0] / amh[1], amh[5]
    replaced = ~torch.isfinite(e) | ~torch.isfinite(med)
    if bool(replaced.any()):
        r32 = torch.tensor(r, dtype=torch.float32)
        want = (1.0 - r32) * torch.nan_to_num(e, 0.0, 0.0) + r32 * torch.nan_to_num(med, 0.0, 0.0)
        both = torch.isfinite(e) & torch.isfinite(med)
        assert not bool((replaced & both).any()) and torch.equal(out[3][replaced], want[replaced])
    if kind == "nonfinite" and H * W >= 9:
        assert bool(((amh[1] == 0) & (amh[0] > 0)).any()) and bool(torch.isnan(med).any()) and bool(torch.isinf(med).any())
    # the gradient of surf_normal on the border is never read (the border is a constant): NaN there changes no bit
    poisoned = gh.clone()
    poisoned[4:7][:, border] = float("nan")
    dam_p = _maps_backward(L, am, rays, rot, r, poisoned.to(dev))
    cleared = gh.clone()
    cleared[4:7][:, border] = 0.0
    dam_c = _maps_backward(L, am, rays, rot, r, cleared.to(dev))
    torch.cuda.synchronize(dev)
    assert torch.equal(dam_p, dam_c) and torch.equal(dam_c, dams[0])


WRAPPER_CASES = [next(c for c in OC.MAPS_CASES if c[0] == kind and c[1] == size)
                 for kind, size in zip(OC.REG_KINDS, [(17, 33), (31, 18), (48, 40)] * 4)]


@pytest.mark.parametrize("case", WRAPPER_CASES, ids=OC.maps_case_id)
def test_surface_maps_node_passes_partial_gradients(gpu_device, case):
    """fused_surface_maps.surface_maps: whichever of its three outputs is consumed, allmap.grad holds the bits of the direct call
    with zeros for the gradients that did not arrive; a non-contiguous allmap gives the bits of its contiguous copy."""
    from gaussmart_amd.fused_surface_maps import surface_maps
    L, dev = _lib.lib(), gpu_device
    kind, size, r, _ = case
    H, W = size
    cam = OC.reg_camera(size, rotated=True)
    am, gout = OC.reg_allmap(kind, size).to(dev), OC.maps_gout(case).to(dev)
    rays, rot = (_c9(t) for t in OC.maps_rays(size))
    out = _maps_forward(L, am, rays, rot, r)
    planes = {"rend_normal": slice(0, 3), "surf_depth": slice(3, 4), "surf_normal": slice(4, 7)}
    wide = torch.zeros(7, H + 2, W + 5, device=dev)
    wide[:, 1:H + 1, 3:W + 3] = am
    for used in (["surf_depth"], ["surf_normal"], ["rend_normal"], list(planes)):
        seen = torch.zeros_like(gout)
        for k in used:
            seen[planes[k]] = gout[planes[k]]
        want = _maps_backward(L, am, rays, rot, r, seen)
        for leaf in (am.clone().requires_grad_(True), wide[:, 1:H + 1, 3:W + 3].detach().requires_grad_(True)):
            maps = dict(zip(planes, surface_maps(leaf, cam, r)))
            for k, s in planes.items():
                assert torch.equal(maps[k], out[s]), (used, k)
            sum((maps[k] * gout[planes[k]]).sum() for k in used).backward()
            assert torch.equal(leaf.grad, want), used
    assert not wide[:, 1:H + 1, 3:W + 3].is_contiguous()


def test_moved_camera_gives_the_new_pose(gpu_device):
    """The per-camera caches follow the pose: after a camera was moved in place, the fused maps and the fused regularizer give the
    bits of a fresh camera at the new pose."""
    from gaussmart_amd.fused_regularizer import surface_regularizer
    from gaussmart_amd.fused_surface_maps import surface_maps
    from gaussmart_amd.synthetic import jittered_cameras
    dev = gpu_device
    H, W = 31, 18
    am = OC.reg_allmap("sphere", (H, W)).to(dev)

    def run(cam):
        a = am.clone().requires_grad_(True)
        maps = surface_maps(a, cam, 0.3)
        loss, nm, dm = surface_regularizer(a, cam, 0.3, 0.05, 100.0)
        (sum(m.sum() for m in maps) + loss).backward()
        return [m.detach().clone() for m in maps] + [loss.detach().clone(), nm.clone(), dm.clone(), a.grad.clone()]

    cam_a, cam_b = jittered_cameras(3, W, H, seed=5, device=dev, amount=0.4)[1:]
    before = run(cam_a)
    cam_a.world_view_transform.copy_(cam_b.world_view_transform)
    cam_a.full_proj_transform.copy_(cam_b.full_proj_transform)
    moved, fresh = run(cam_a), run(jittered_cameras(3, W, H, seed=5, device=dev, amount=0.4)[2])
    assert all(torch.equal(x, y) for x, y in zip(moved, fresh))
    assert not torch.equal(moved[0], before[0]) and not torch.equal(moved[2], before[2])


# ------------------------------------------------------------------------------------------------ objective finish
@pytest.mark.parametrize("with_reg", [False, True], ids=["loss", "loss+reg"])
@pytest.mark.parametrize("n", OC.FINISH_N)
def test_objective_finish_on_synthetic_partials(gpu_device, held, n, with_reg):
    """It reads only counts from C, H, W: H = 16, W = 16 n gives n partial pairs; 2048 pairs make one round of the summation loop."""
    L, dev = _lib.lib(), gpu_device
    Cn, H, W = 3, 16, 16 * n
    lam, ln, ld = 0.2, 0.05, 100.0
    assert L.gsr_loss_num_partials(H, W) == 2 * n
    plh, prh = OC.finish_partials(n, with_reg)
    pl, pr = plh.to(dev), (prh.to(dev) if with_reg else None)
    out = nans((5,), dev)
    _lib.check(L.gsr_objective_finish(ptr(pl), Cn, H, W, ptr(pr), lam, ln, ld, ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    truth = OC.finish_truth(plh, prh, Cn, H, W, lam, ln, ld)
    for k, what in enumerate(("total", "l1", "ssim", "normal", "dist")):
        held(f"finish n {n} {'with' if with_reg else 'without'} reg", what, out[k], truth[k])
    if n == 2049:
        # the same five scalars from the workgroup that rides along with loss_bwd_kernel
        img, maps, dimg, out2 = torch.zeros(Cn, H, W, device=dev), torch.zeros(3, Cn, H, W, device=dev), nans((Cn, H, W), dev), nans((5,), dev)
        scale = torch.ones(1, device=dev)
        _lib.check(L.gsr_loss_backward_finish(ptr(img), ptr(img), ptr(maps), Cn, H, W, lam, ptr(scale), ptr(dimg), ptr(pl), ptr(pr),
                                              ln, ld, ptr(out2), None, stream(dev)))
        torch.cuda.synchronize(dev)
        assert torch.equal(out, out2) and bool(torch.isfinite(dimg).all())
