"""The twins and bars of tests/objective_cases.py without a GPU: the fp64 twins against oracle/loss_ref.py and
oracle/regularizer_ref.py, the reachability of every bar (the kernel's formulation in torch fp32 uses at most half of it on every
case and quantity) and its tightness (each wrong reading of a kernel listed there moves some quantity of some case beyond ten
bars).  tests/test_gpu_objective_parity.py holds the kernels to the same bars.  The same three for the surface maps (maps_chain
against oracle/regularizer_ref.surface_maps), and the per-camera caches of rays and intrinsics on a camera that moves."""
import pytest
import torch

import objective_cases as OC
from objective_cases import bar, ratio
from oracle import loss_ref
from oracle import regularizer_ref as R


def worst(pairs):
    """pairs of (got, E) -> the largest |got - truth| / bar."""
    return max(ratio((g.double() - e.v).abs(), bar(e)) for g, e in pairs)


# ------------------------------------------------------------------------------------------------ photometric loss
def test_the_kernel_window_is_the_references_within_a_few_roundings():
    # the two 1-D windows differ by the order of an 11-term fp32 sum -- one ulp of the sum here, 2 roundings per factor -- and the
    # reference rounds the product of its two factors: 2 * 2 + 1 = 5, one to spare (the bars use the measured k, whatever it is)
    w = OC.WINDOW
    assert w.k <= 6 and abs(float(w.w1.double().sum()) - 1.0) < 4 * OC.U32
    assert torch.equal(w.w2.float(), loss_ref.gaussian_window(11, 1.5, 1)[0, 0])


def test_cases_cover_what_they_claim():
    for content in OC.LOSS_CONTENTS:
        assert sum(c == content for c, _ in OC.LOSS_CASES) >= 2, content
    for shape in OC.LOSS_SHAPES:
        assert sum(s == shape for _, s in OC.LOSS_CASES) >= 2, shape
    x, y = OC.loss_inputs("ulp", (3, 37, 70))
    assert torch.equal(x[..., :35], y[..., :35]) and bool((x[..., 35:] != y[..., 35:]).all())
    assert float((x - y).abs().max()) <= 2.0 ** -23
    x, _ = OC.loss_inputs("outside", (3, 33, 31))
    assert float(x.min()) < 0 and float(x.max()) > 1
    for size in OC.REG_SIZES:
        for kind in OC.REG_KINDS:
            assert sum(c[0] == kind and c[1] == size for c in OC.REG_CASES) == 1
    for kind in OC.REG_KINDS:
        assert {c[2] for c in OC.REG_CASES if c[0] == kind} == set(OC.REG_RATIOS)
        assert {c[3] for c in OC.REG_CASES if c[0] == kind} == set(OC.REG_LAMBDAS)
    am = OC.reg_allmap("nonfinite", (17, 33))
    assert bool(torch.isnan(am[5]).any()) and bool(torch.isinf(am[5]).any()) and bool(((am[1] == 0) & (am[0] > 0)).any())
    assert int((OC.reg_allmap("island", (31, 18))[1] > 0).sum()) == 1 and int((OC.reg_allmap("one_hole", (31, 18))[1] == 0).sum()) == 1


@pytest.mark.parametrize("content,shape", OC.LOSS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_loss_fp64_twin_is_the_oracle(content, shape):
    x, y = (t.double() for t in OC.loss_inputs(content, shape))
    fwd, bwd = OC.loss_truth(content, shape)
    assert float((fwd["S"].v - loss_ref.ssim_map(x, y)).abs().max()) <= 1e-12
    C, H, W = shape
    for (lam, gs), d in bwd.items():
        xo = x.clone().requires_grad_(True)
        (gs * loss_ref.photometric_loss(xo, y, OC.f32(lam))[0]).backward()
        assert float((d.v - xo.grad).abs().max()) <= 1e-12, (lam, gs)
    # the slots: a 32x32 tile's sums in its top-left 16x16 cell, zeros in its other cells, nothing lost
    s, l = fwd["slots"]
    assert s.v.numel() == OC.num_slots(H, W)
    for t_, full in ((s.v, fwd["S"].v), (l.v, (x - y).abs())):
        assert abs(float(t_.sum() - full.sum())) <= 1e-9 * max(1.0, float(full.abs().sum()))
        assert float(t_[1::2].abs().sum()) == 0.0 and float(t_[:, 1::2].abs().sum()) == 0.0
        assert abs(float(t_[0, 0] - full[:, :32, :32].sum())) <= 1e-9 * max(1.0, float(full.abs().sum()))


@pytest.mark.parametrize("content,shape", OC.LOSS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_loss_bars_are_reachable(content, shape):
    """The kernel's formulation in torch fp32 stays within half of every bar."""
    x, y = OC.loss_inputs(content, shape)
    fwd, bwd = OC.loss_truth(content, shape)
    got = OC.loss_forward(x, y)
    use = {"S": worst([(got["S"], fwd["S"])]), "maps": worst(zip(got["maps"], fwd["maps"])), "slots": worst(zip(got["slots"], fwd["slots"]))}
    for (lam, gs), d in bwd.items():
        use[f"dimg {lam} {gs}"] = worst([(OC.loss_backward(x, y, got["maps"], OC.f32(lam), gs), d)])
    print(content, shape, {k: round(v, 3) for k, v in use.items()})
    assert max(use.values()) <= 0.5, use


def _beyond(got, e, factor=10.0):
    d = (got - e.v).abs()
    return bool((~torch.isfinite(d)).any()) or bool((d > factor * bar(e)).any())


@pytest.mark.parametrize("name", list(OC.LOSS_MUTATIONS))
def test_loss_bars_are_tight(name):
    """A wrong reading of the kernel moves some checked quantity of some case beyond ten bars."""
    caught = []
    for content, shape in OC.LOSS_CASES:
        fwd, bwd = OC.loss_truth(content, shape)
        m, d = OC.loss_mutant(content, shape, name, 0.2, 3.0)
        hit = _beyond(m["S"], fwd["S"]) or any(_beyond(a, b) for a, b in zip(m["maps"], fwd["maps"])) or \
            any(_beyond(a, b) for a, b in zip(m["slots"], fwd["slots"])) or _beyond(d, bwd[(0.2, 3.0)])
        if hit:
            caught.append((content, shape))
    print(name, "caught by", len(caught), "of", len(OC.LOSS_CASES), "cases")
    assert caught, name


# ------------------------------------------------------------------------------------------------ surface regularizers
@pytest.mark.parametrize("case", OC.REG_CASES, ids=OC.reg_case_id)
def test_reg_fp64_twin_is_the_oracle(case):
    """On a rotated camera: the oracle works in world space, the twin in camera space with K^-1."""
    kind, size, r, (ln, ld) = case
    H, W = size
    am = OC.reg_allmap(kind, size).double()
    wvt, full = OC.reg_camera_f64(size, rotated=True)
    kinv = OC.reg_kinv(size, rotated=True, dtype=torch.float64)
    gs = OC.REG_GRAD_SCALE
    t = OC.reg_chain(am, kinv, r, ln, ld, gs)
    err_a, sums_a, grad_a = OC.reg_autograd64(am, kinv, r, ln, ld, gs)
    ao = am.clone().requires_grad_(True)
    lo, nmo, dmo = R.regularizer_loss(ao, wvt, full, r, ln, ld)
    (gs * lo).backward()
    nmo, dmo = nmo.detach(), dmo.detach()
    lit = am[1] > 0
    # `micro` is lit and all of it has |cross| <= 1e-12: there reg_bwd_kernel lets nothing through the normalisation, by its
    # contract (reg_chain), and autograd of F.normalize scales by 1e12.  The oracle's depth gradients are not the twin's then
    through = [2, 3, 4, 6] if kind == "micro" else list(range(7))
    for nm, dm, grad in ((t["err"].mean(), t["sums"][1].sum() / (H * W), torch.stack(t["dam"])), (err_a.mean(), sums_a[1].sum() / (H * W), grad_a)):
        assert abs(float(nm - nmo)) <= 1e-10 and abs(float(dm - dmo)) <= 1e-10
        if bool(lit.any()):
            assert float((grad - ao.grad)[through][:, lit].abs().max()) <= 1e-10
        if kind == "micro":
            assert float(grad[[0, 1, 5]].abs().sum()) == 0.0
            assert min(size) < 3 or ln == 0.0 or float(ao.grad[[0, 1, 5]].abs().max()) > 0.0
    assert abs(float(t["sums"][0].sum() - t["err"].sum())) <= 1e-10 * H * W
    # the two formulations of the twin agree everywhere, holes included
    assert float((torch.stack(t["dam"]) - grad_a).abs().max()) <= 1e-10 and float((t["err"] - err_a).abs().max()) <= 1e-12


def reg_contract(dam, am, kd):
    """What the kernels promise at pixels without a splat: finite values, zero in channels 0 and 1, channel 6 = kd."""
    hole = am[1] == 0
    assert bool(torch.isfinite(dam).all())
    assert float(dam[0][hole].abs().sum()) == 0.0 and float(dam[1][hole].abs().sum()) == 0.0
    assert bool((dam[6] == kd).all())


@pytest.mark.parametrize("case", OC.REG_CASES, ids=OC.reg_case_id)
def test_reg_bars_are_reachable(case):
    kind, size, r, (ln, ld) = case
    am = OC.reg_allmap(kind, size)
    truth = OC.reg_truth(case)
    got = OC.reg_chain(am, OC.reg_kinv(size), OC.f32(r), OC.f32(ln), OC.f32(ld), OC.REG_GRAD_SCALE)
    lit = am[1] > 0
    use = {"err": worst([(got["err"], truth["err"])]), "sums": worst(zip(got["sums"], truth["sums"])),
           "dam": worst((g[lit], t[lit]) for g, t in zip(got["dam"], truth["dam"])),
           "dam holes": worst((g[~lit], t[~lit]) for g, t in zip(got["dam"], truth["dam"]))}
    print(OC.reg_case_id(case), {k: round(v, 3) for k, v in use.items()})
    assert max(use.values()) <= 0.5, use
    for dam in (torch.stack(got["dam"]), torch.stack([t.v for t in truth["dam"]]).float()):
        reg_contract(dam, am, dam[6, 0, 0])
    assert float(truth["dam"][6].v[0, 0]) == pytest.approx(OC.f32(ld) * OC.REG_GRAD_SCALE / (size[0] * size[1]), rel=1e-12)
    if kind in ("island", "micro"):   # |cross| = 0 at the lit pixel and around it, |cross| < 1e-12 everywhere: reg_bwd lets nothing
        assert float(torch.stack(got["dam"])[[0, 1, 5]].abs().sum()) == 0.0        # through (maps_bwd scales by 1e12)
    if kind == "plane" and min(size) >= 3:
        assert float(truth["err"].v[1:-1, 1:-1].abs().max()) < 1e-6


@pytest.mark.parametrize("name", OC.REG_MUTATIONS)
def test_reg_bars_are_tight(name):
    caught = []
    for case in OC.REG_CASES:
        kind, size, r, (ln, ld) = case
        am = OC.reg_allmap(kind, size)
        truth = OC.reg_truth(case)
        err, sums, grad = OC.reg_autograd64(am, OC.reg_kinv(size), OC.f32(r), OC.f32(ln), OC.f32(ld), OC.REG_GRAD_SCALE, mut=name)
        lit = am[1] > 0
        if any(_beyond(a, b) for a, b in zip(sums, truth["sums"])) or any(_beyond(grad[c][lit], truth["dam"][c][lit]) for c in range(7)):
            caught.append(OC.reg_case_id(case))
    print(name, "caught by", len(caught), "of", len(OC.REG_CASES), "cases")
    assert caught, name


# ------------------------------------------------------------------------------------------------ surface maps
def _split(am):
    lit = am[1] > 0
    return (("lit", lit), ("holes", ~lit))


def test_maps_cases_cover_what_they_claim():
    for size in OC.MAPS_SIZES:
        for kind in OC.REG_KINDS:
            assert sum(c[0] == kind and c[1] == size for c in OC.MAPS_CASES) == 1
    for kind in OC.REG_KINDS:
        assert {c[2] for c in OC.MAPS_CASES if c[0] == kind} == set(OC.REG_RATIOS)
        assert sum(c[3] == "delta" for c in OC.MAPS_CASES if c[0] == kind) == 1
    assert OC.REG_CASES[:36] == [(kind, size, OC.REG_RATIOS[(i + j) % 3], OC.REG_LAMBDAS[(i + 2 * j + (i // 3)) % 3])
                                 for i, size in enumerate(OC.REG_SIZES) for j, kind in enumerate(OC.REG_NOISE_KINDS)]
    for case in OC.MAPS_CASES:
        kind, (H, W), r, pattern = case
        am, gout, truth = OC.reg_allmap(kind, (H, W)), OC.maps_gout(case), OC.maps_truth(case)
        assert bool(((am[1] == 0) | (am[1] >= 0.05)).all()) and float(am[1].max()) <= 1.0
        if pattern == "delta":
            hit = (gout != 0).any(0)
            assert int(hit.sum()) == 1 and bool(hit[1:-1, 1:-1].any()) and bool((gout[:, hit] != 0).all())
        # no pixel stands near the threshold between the two regimes of the normalisation: |cross| of the truth lies farther
        # than ten of its own bars from 1e-12, so the kernel and the truth take the same branch at every pixel
        ln = truth["len"]
        assert bool(((ln.v - 1e-12).abs() > 10.0 * bar(ln)).all()), OC.maps_case_id(case)
        if kind == "micro":                                  # all of it in the eps regime
            assert ln.v.numel() == max(H - 2, 0) * max(W - 2, 0) and bool((ln.v < 1e-12).all())
            assert min(H, W) < 3 or float(ln.v.min()) > 0.0
        if kind == "grazing" and H > 2:
            assert bool((am[1] == 0).any()) and bool((am[1] > 0).any())
    lit = OC.reg_allmap("sphere", (48, 40))[1] > 0           # a silhouette inside one 16x16 tile
    assert any(bool(t.any()) and not bool(t.all()) for t in (lit[y:y + 16, x:x + 16] for y in (0, 16, 32) for x in (0, 16, 32)))
    step = OC.reg_allmap("step", (17, 33))
    assert float((step[0] / step[1])[:, :16].max()) < 2.02 and float((step[0] / step[1])[:, 16:].min()) >= 9.0
    assert float((OC.reg_allmap("far", (17, 33))[0] / OC.reg_allmap("far", (17, 33))[1]).min()) > 2000.0


@pytest.mark.parametrize("case", OC.MAPS_CASES, ids=OC.maps_case_id)
def test_maps_fp64_twin_is_the_oracle(case):
    """maps_chain in fp64 on the fp64 rays of the rotated camera against oracle/regularizer_ref.surface_maps and autograd."""
    kind, size, r, _ = case
    am, gout = OC.reg_allmap(kind, size).double(), OC.maps_gout(case).double()
    wvt, full = OC.reg_camera_f64(size, rotated=True)
    rays9, rot9 = OC.maps_rays(size, torch.float64)
    t = OC.maps_chain(am, rays9, rot9, r, gout)
    out, dam = torch.stack(t["out"]), torch.stack(t["dam"])
    ao = am.clone().requires_grad_(True)
    m = R.surface_maps(ao, wvt, full, r)
    oracle = torch.cat([m["rend_normal"], m["surf_depth"], m["surf_normal"]])
    (oracle * gout).sum().backward()
    assert float((out - oracle.detach()).abs().max()) <= 1e-10
    lit = am[1] > 0
    grad_o = ao.grad
    if kind == "micro":
        # the eps regime multiplies the gradient by 1e12: it reaches 4e6 here, where fp64 resolves 1e-9, and the oracle's own
        # points, depth * ray + camera centre, lose the differences of 3e-8 .. 2e-7 to the centre's 1e-16: 7.5e-10 of the
        # gradient at 80x112.  So for this kind the oracle sees the same camera with its centre at the world origin (the maps do
        # not depend on it), and the 1e-10 is relative to the channel's largest gradient
        ao = am.clone().requires_grad_(True)
        m = R.surface_maps(ao, *OC.reg_camera_f64(size, rotated=True, centred=True), r)
        centred = torch.cat([m["rend_normal"], m["surf_depth"], m["surf_normal"]])
        (centred * gout).sum().backward()
        assert float((out - centred.detach()).abs().max()) <= 1e-10
        scale = ao.grad.abs().amax((1, 2), keepdim=True).clamp_min(1.0)
        dam, grad_o = dam / scale, ao.grad / scale
        if min(size) >= 3:
            assert float(scale.max()) > 1e3
    if bool(lit.any()):                                      # torch leaves 0 / 0 at the holes
        assert float((dam - grad_o)[:, lit].abs().max()) <= 1e-10
    # the two formulations of the twin agree everywhere, and both keep the contract at the holes (where a lit pixel between two
    # holes is in the eps regime, the holes' median channel receives 1e12 times its gradient: relative to the value there)
    out_a, grad_a = OC.maps_autograd64(am, rays9, rot9, r, gout)
    dam = torch.stack(t["dam"])
    assert float((out - out_a).abs().max()) <= 1e-10 and bool(((dam - grad_a).abs() <= 1e-10 * grad_a.abs().clamp_min(1.0)).all())
    for d in (dam, grad_a):
        maps_contract(d, am)


def maps_contract(dam, am):
    """What the kernels promise at pixels without a splat: finite values, zero in channels 0 and 1; channel 6 is zero everywhere."""
    hole = am[1] == 0
    assert bool(torch.isfinite(dam).all())
    assert float(dam[0][hole].abs().sum()) == 0.0 and float(dam[1][hole].abs().sum()) == 0.0
    assert float(dam[6].abs().sum()) == 0.0


@pytest.mark.parametrize("case", OC.MAPS_CASES, ids=OC.maps_case_id)
def test_maps_bars_are_reachable(case):
    """The kernels' formulation in torch fp32 stays within half of every bar: every plane, every channel, lit pixels and holes."""
    kind, size, r, _ = case
    am, truth = OC.reg_allmap(kind, size), OC.maps_truth(case)
    got = OC.maps_chain(am, *OC.maps_rays(size), OC.f32(r), OC.maps_gout(case))
    use = {}
    for which, sel in _split(am):
        for name in ("out", "dam"):
            for c in range(7):
                use[f"{name}[{c}] {which}"] = worst([(got[name][c][sel], truth[name][c][sel])])
    top = max(use, key=use.get)
    print(OC.maps_case_id(case), top, round(use[top], 3))
    assert use[top] <= 0.5, use
    maps_contract(torch.stack(got["dam"]), am)
    border = torch.ones(size, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    if min(size) < 3:
        border[:] = True
    assert float(torch.stack(got["out"][4:7])[:, border].abs().sum()) == 0.0


@pytest.mark.parametrize("name", OC.MAPS_MUTATIONS)
def test_maps_bars_are_tight(name):
    """A wrong reading of maps_fwd_kernel / maps_bwd_kernel moves some plane or channel of some case beyond ten bars."""
    caught = []
    for case in OC.MAPS_CASES:
        kind, size, r, _ = case
        truth = OC.maps_truth(case)
        out, grad = OC.maps_autograd64(OC.reg_allmap(kind, size), *OC.maps_rays(size), OC.f32(r), OC.maps_gout(case), mut=name)
        if any(_beyond(out[c], truth["out"][c]) or _beyond(grad[c], truth["dam"][c]) for c in range(7)):
            caught.append(OC.maps_case_id(case))
    print(name, "caught by", len(caught), "of", len(OC.MAPS_CASES), "cases")
    assert caught, name
    if name == "eps_passes_nothing":
        assert any(c.startswith("micro-") for c in caught), caught


# ------------------------------------------------------------------------------------------------ the per-camera caches
def _cache_functions():
    from gaussmart_amd.fused_regularizer import camera_kinv
    from gaussmart_amd.fused_surface_maps import camera_world_rays
    from gaussmart_amd.gaussian_renderer import _camera_rays
    bits = lambda v: v.clone() if isinstance(v, torch.Tensor) else torch.tensor(list(v), dtype=torch.float32)
    return {"camera_kinv": (camera_kinv, lambda v: [bits(v)]),
            "camera_world_rays": (camera_world_rays, lambda v: [bits(x) for x in v]),
            "_camera_rays": (lambda cam: _camera_rays(cam, torch.device("cpu"), torch.float32), lambda v: [bits(x) for x in v])}


@pytest.mark.parametrize("how", ["copy_", "assignment"])
@pytest.mark.parametrize("which", ["camera_kinv", "camera_world_rays", "_camera_rays"])
def test_camera_caches_follow_the_pose(which, how):
    """What is cached on a camera belongs to its pose: after the pose tensors were written in place or replaced, the camera gives
    the numbers of a fresh camera at the new pose; an unchanged camera gives the cached objects themselves."""
    from gaussmart_amd.synthetic import jittered_cameras
    fn, numbers = _cache_functions()[which]
    same = lambda a, b: all(x is y for x, y in zip(a, b)) if isinstance(a, tuple) else a is b
    cam_a, cam_b = jittered_cameras(3, 40, 24, seed=3, amount=0.4)[1:]
    fresh_b = numbers(fn(jittered_cameras(3, 40, 24, seed=3, amount=0.4)[2]))
    first = fn(cam_a)
    old_a = numbers(first)
    assert same(fn(cam_a), first)
    if how == "copy_":
        cam_a.world_view_transform.copy_(cam_b.world_view_transform)
        cam_a.full_proj_transform.copy_(cam_b.full_proj_transform)
    else:
        cam_a.world_view_transform = cam_b.world_view_transform.clone()
        cam_a.full_proj_transform = cam_b.full_proj_transform.clone()
    moved = fn(cam_a)
    assert all(torch.equal(x, y) for x, y in zip(numbers(moved), fresh_b))
    assert not all(torch.equal(x, y) for x, y in zip(numbers(moved), old_a))
    assert same(fn(cam_a), moved)


# ------------------------------------------------------------------------------------------------ objective finish
@pytest.mark.parametrize("n", OC.FINISH_N)
def test_finish_bar_is_reachable(n):
    """The kernel's order in torch fp32: 256 threads, thread t adds the partials t, t + 256, ... one after the other, then a tree."""
    C, H, W = 3, 16, 16 * n
    for with_reg in (False, True):
        pl, pr = OC.finish_partials(n, with_reg)
        truth = OC.finish_truth(pl, pr, C, H, W, 0.2, 0.05, 100.0)

        def tree(col):
            acc = torch.zeros(256)
            padded = torch.cat([col, torch.zeros(-n % 256)]).reshape(-1, 256)
            for row in padded:
                acc = acc + row
            d = 128
            while d > 0:
                acc = acc[:d] + acc[d:2 * d]
                d //= 2
            return acc[0]

        inv_img, inv_pix = torch.tensor(1.0) / torch.tensor(float(C * H * W)), torch.tensor(1.0) / torch.tensor(float(H * W))
        ssim, l1 = tree(pl[:, 0]) * inv_img, tree(pl[:, 1]) * inv_img
        nrm, dst = (tree(pr[:, 0]) * inv_pix, tree(pr[:, 1]) * inv_pix) if with_reg else (torch.tensor(0.0), torch.tensor(0.0))
        lam, ln, ld = torch.tensor(0.2), torch.tensor(0.05 if with_reg else 0.0), torch.tensor(100.0 if with_reg else 0.0)
        tot = (1.0 - lam) * l1 + lam * (1.0 - ssim) + ln * nrm + ld * dst
        use = worst(zip((tot, l1, ssim, nrm, dst), truth))
        print(n, with_reg, round(use, 3))
        assert use <= 0.5
        # a typical partial left out, or counted twice, is far beyond the bar
        assert float(pl[:, 0].abs().median()) / (C * H * W) > 10 * float(bar(truth[2]))
