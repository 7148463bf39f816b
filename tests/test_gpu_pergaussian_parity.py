"""The per-Gaussian kernels on the device, Gaussian by Gaussian and field by field, against the fp64 chains of
tests/pergaussian_cases.py, each quantity held to the bar derived there (tests/test_pergaussian_cpu.py proves every bar reachable
and tight without a GPU):
  1. K1 geometry (preprocess_fwd_kernel): the record, depth key, radius, tile rect and tile count of every Gaussian;
  2. every producer of the SH colour: rgb, clamp bits and d(rgb)/d(dir);
  3. the view-direction term of dL/dmean, isolated by a twin run without SH whose geometry gradient has the same bits;
  4. the K8 chain dL/dT -> (mean, scale, quaternion), isolated by a twin run with transmat_precomp.
GSR_PERGAUSSIAN_PARITY_REPORT=<file>: the measured errors and bars are appended there (profiles/pergaussian_parity.txt is such a
run)."""
import ctypes as C
import os

import pytest
import torch

import pergaussian_cases as PC
from conftest import hip_settings
from objective_cases import U32, bar

pytestmark = pytest.mark.gpu
GEOM = PC.geom_cases()


def report(line):
    out = os.environ.get("GSR_PERGAUSSIAN_PARITY_REPORT")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


@pytest.fixture
def held():
    """held(case, what, got, want, b, where=None, excused=0): max |got - want| / b over the elements (of the rows `where`) must be
    <= 1.  Every figure is printed before it is asserted; one line per case and field is reported, whether it holds or not (the
    runs of one case at several sizes N, "case ... N n", are reported together: the worst of them)."""
    rows = {}

    def check(case, what, got, want, b, where=None, excused=0):
        got = got.detach().double().cpu()
        if where is not None:
            got, want, b = got[where], want[where], b[where]
        err = (got - want).abs()
        use = PC.ratio(err, b)
        e_max, b_max, cnt = (float(err.max()), float(b.max()), err.shape[0]) if err.numel() else (0.0, 0.0, 0)
        print(f"{case} | {what}: max err {e_max:.3e}, max bar {b_max:.3e}, worst err/bar {use:.3f}, excused {int(excused)} of {cnt}")
        r = rows.setdefault((case.split(" N ")[0], what), [0.0, 0.0, 0.0, 0, 0])
        rows[(case.split(" N ")[0], what)] = [max(r[0], e_max), max(r[1], b_max), max(r[2], use), r[3] + int(excused), r[4] + cnt]
        assert bool(torch.isfinite(got).all()) and use <= 1.0, (case, what, use)

    yield check
    for (case, what), (e_max, b_max, use, excused, cnt) in rows.items():
        report(f"{case} | {what}: max err {e_max:.3e}, max bar {b_max:.3e}, worst err/bar {use:.3f}, excused {excused} of {cnt}")


def held_E(held, case, what, got, truth, where=None, excused=0):
    held(case, what, got, truth.v, bar(truth), where, excused)


def to(dev, t):
    return None if t is None else t.to(dev).contiguous()


def clamp_bits(words):
    w = words.detach().cpu().to(torch.int64)
    return torch.stack([(w >> c) & 1 for c in range(3)], -1).bool()


def misaligned(t, dev):
    """A contiguous copy of `t` on the device that starts 4 bytes into its allocation (neither _f32c nor _pack_reference copies a
    contiguous float32 tensor, so the kernels see this address)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def debug(dev, rs, means, opac, **kw):
    """rasterize_debug -> clones of the fields the tests read (the views alias pooled buffers)."""
    from gaussmart_amd import rasterizer as R
    res = R.rasterize_debug(means, opac, raster_settings=rs, **kw)
    out = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in res.items() if k != "_lease"}
    del res
    return out


# ------------------------------------------------------------------------------------------------ 1. K1 geometry
@pytest.mark.parametrize("name", list(GEOM))
def test_geometry_per_gaussian(gpu_device, held, name):
    dev = gpu_device
    c = GEOM[name]()
    n = c["means"].shape[0]
    truth = PC.geom_run("bar", c)
    rs = hip_settings(c["cam"], deg=3, device=dev, scale_modifier=c["mod"])
    if c["raw"]:
        d = debug(dev, rs, to(dev, c["means"]), to(dev, c["opac"]), scales=to(dev, c["scales"]), rotations=to(dev, c["rots"]),
                  raw_features=(to(dev, c["f_dc"]), to(dev, c["f_rest"])))
    elif c["precomp"] is not None:
        d = debug(dev, rs, to(dev, c["means"]), to(dev, c["opac"]), colors_precomp=torch.full((n, 3), 0.5, device=dev),
                  cov3D_precomp=to(dev, c["precomp"]))
    else:
        d = debug(dev, rs, to(dev, c["means"]), to(dev, c["opac"]), colors_precomp=torch.full((n, 3), 0.5, device=dev),
                  scales=to(dev, c["scales"]), rotations=to(dev, c["rots"]))
    radii, tiles, key = d["radii"].cpu(), d["tiles_touched"].cpu().long(), d["depth_key"].cpu()
    tr = d["tile_rect"].cpu().long()
    rect = torch.stack([tr[:, 0] & 0xFFFF, tr[:, 0] >> 16, (tr[:, 0] & 0xFFFF) + (tr[:, 1] & 0xFFFF), (tr[:, 0] >> 16) + (tr[:, 1] >> 16)], -1)
    vis = radii > 0
    ex = truth["excused"]
    n_ex = int((ex["radius"] | ex["rect"]).sum())
    # discrete results: equal to fp64 wherever the deciding quantity's margin exceeds its bar
    assert torch.equal(vis[~ex["vis"]], truth["vis"][~ex["vis"]])
    assert torch.equal(radii[~ex["radius"]], truth["radii"][~ex["radius"]])
    assert torch.equal(rect[~ex["rect"]], truth["rect"][~ex["rect"]])
    # what K1 wrote hangs together, excused or not
    assert torch.equal(tiles, (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]))
    assert d["num_rendered"] == int(tiles.sum())
    assert bool((tiles[~vis] == 0).all()) and bool((key[~vis] == -1).all()) and bool((tr[~vis] == 0).all())      # 0xFFFFFFFF
    assert bool((tiles[vis] > 0).all())
    if "labels" in c:
        assert n_ex == 0                                             # an edge Gaussian stands a stated distance from its threshold
    # the record, for the Gaussians visible here and in fp64 (`clamped` and the record are never written for a culled one)
    both = vis & truth["vis"]
    fields = PC.record_fields(d["splat"].cpu(), key)
    for k in PC.GEOM_FIELDS:
        held_E(held, f"geometry {name}", k, fields[k], truth[k], both, n_ex)
    if not c["raw"]:
        assert bool((d["clamped"].cpu()[vis] == 0).all())            # precomputed colours clamp nothing
    report(f"geometry {name} | decisions: {n} Gaussians, {int(vis.sum())} visible, {n_ex} excused "
           f"({', '.join(f'{k} {int(v.sum())}' for k, v in ex.items())})")


# ------------------------------------------------------------------------------------------------ 2. colour producers
def check_colour(held, case, rgb, words, J, truth, rows=None):
    """rgb within its bar and exactly 0 where clamped; clamp bits as fp64 wherever |v + 0.5| exceeds its bar; J within its bar."""
    rgb, bits = rgb.detach().cpu(), clamp_bits(words)
    decided = truth["v"].v.abs() > bar(truth["v"])
    rows = torch.ones(rgb.shape[0], dtype=torch.bool) if rows is None else rows
    held_E(held, case, "rgb", rgb, truth["rgb"], rows, int((~decided[rows]).sum()))
    assert bool((rgb[rows][bits[rows]] == 0).all())
    assert bool((words.detach().cpu()[rows] >> 3 == 0).all())
    assert torch.equal(bits[rows][decided[rows]], truth["clamp"][rows][decided[rows]])
    if J is not None:
        held_E(held, case, "J", J.reshape(-1, 3, 3), truth["J"], rows)


def colour_settings(dev, s, deg):
    return hip_settings(s["cam"], deg=deg, device=dev)._replace(campos=s["campos"].to(dev))


PRODUCERS = ("16-lane joint", "16-lane split", "staged", "unstaged")


@pytest.mark.parametrize("producer", PRODUCERS)
@pytest.mark.parametrize("deg,M", PC.COLOR_GRID)
def test_colour_pass_per_gaussian(gpu_device, held, monkeypatch, deg, M, producer):
    dev = gpu_device
    if producer in ("staged", "unstaged"):
        monkeypatch.setenv("GSR_COLOR_STAGED", "1")
    else:
        monkeypatch.delenv("GSR_COLOR_STAGED", raising=False)
    for n in PC.COLOR_NS:
        s = PC.color_scene(deg, M, n)
        truth = PC.color_truth(deg, M, n)
        rs = colour_settings(dev, s, deg)
        case = f"colour {producer} deg {deg} M {M} N {n}"
        if producer == "16-lane split":
            d = debug(dev, rs, to(dev, s["means"]), to(dev, s["opac_raw"]), scales=to(dev, s["scales_raw"]), rotations=to(dev, s["rots"]),
                      raw_features=(to(dev, s["sh"][:, :1]), to(dev, s["sh"][:, 1:])))
        else:
            shs = misaligned(s["sh"], dev) if producer == "unstaged" else to(dev, s["sh"])
            d = debug(dev, rs, to(dev, s["means"]), to(dev, s["opac"]), shs=shs, scales=to(dev, s["scales"]), rotations=to(dev, s["rots"]))
        assert bool((d["radii"] > 0).all())                          # the scene was built for that: every Gaussian has a colour
        J = d["color_jac"] if producer.startswith("16-lane") else None      # (the staged forms leave none)
        check_colour(held, case, d["splat"][:, 15:18], d["clamped"], J, truth)


def cache_step(dev, s, deg, ranges=None):
    """FusedAdam.step_sh_factored with an all-zero record and the next view = this view -> (cache [13 N], the coefficients after
    the step [N,M,3]).  ranges: [(first, count), ...] through the C ABI (step_sh_factored builds a cache only for the whole
    range)."""
    from gaussmart_amd import _lib
    from gaussmart_amd.fused_adam import FusedAdam
    n = s["means"].shape[0]
    f_dc = torch.nn.Parameter(to(dev, s["sh"][:, :1]))
    f_rest = torch.nn.Parameter(to(dev, s["sh"][:, 1:]))
    opt = FusedAdam([{"params": [f_dc], "lr": 0.0025, "name": "f_dc"}, {"params": [f_rest], "lr": 0.000125, "name": "f_rest"}],
                    lr=0.0, eps=1e-15)
    xyz, campos = to(dev, s["means"]), to(dev, s["campos"])
    rec = torch.zeros(3 * n + 4, dtype=torch.float32, device=dev)
    if ranges is None:
        opt.step_sh_factored(f_dc, f_rest, xyz, rec, 1, 3 * n + 4, deg, next_view=(campos, deg), xyz_next=xyz)
        cache = opt.color_cache[1]
    else:
        cache = torch.full((13 * n,), float("nan"), dtype=torch.float32, device=dev)
        st = [opt._state_of(p) for p in (f_dc, f_rest)]
        stream = torch.cuda.current_stream(dev).cuda_stream
        for first, count in ranges:
            a = [C.c_void_p(t.data_ptr()) for t in (f_dc, st[0]["exp_avg"], st[0]["exp_avg_sq"])]
            b = [C.c_void_p(t.data_ptr()) for t in (f_rest, st[1]["exp_avg"], st[1]["exp_avg_sq"])]
            _lib.check(_lib.lib().gsr_adam_sh_factored_next(
                first, count, s["sh"].shape[1], deg, C.c_void_p(xyz.data_ptr()), 1, C.c_void_p(rec.data_ptr()), 3 * n + 4,
                C.c_void_p(rec.data_ptr() + 12 * n), 3 * n + 4, 1.0, *a, 0.025, 31.6, *b, 0.00125, 31.6, 0.9, 0.999, 1e-15,
                C.c_void_p(xyz.data_ptr()), C.c_void_p(campos.data_ptr()), deg, n, C.c_void_p(cache.data_ptr()), C.c_void_p(stream)))
    torch.cuda.synchronize(dev)
    return cache.clone(), torch.cat([f_dc.detach(), f_rest.detach()], 1).cpu()


@pytest.mark.parametrize("deg,M", PC.COLOR_GRID)
def test_colour_cache_per_gaussian(gpu_device, held, deg, M):
    dev = gpu_device
    for n in PC.COLOR_NS:
        s = PC.color_scene(deg, M, n)
        cache, sh_after = cache_step(dev, s, deg)
        assert torch.equal(sh_after, s["sh"])                        # a zero gradient on zero moments moves nothing
        truth = PC.color_chain("bar", deg, sh_after, s["means"], s["campos"])
        check_colour(held, f"colour cache deg {deg} M {M} N {n}", cache[:3 * n].view(n, 3), cache[3 * n:4 * n].view(torch.int32),
                     cache[4 * n:], truth)
        if n > 64:      # ranges that start off a multiple of 64 write the same cache
            parts, sh_parts = cache_step(dev, s, deg, ranges=[(0, 37), (37, n - 37 - 5), (n - 5, 5)])
            assert torch.equal(parts, cache) and torch.equal(sh_parts, sh_after)


# ------------------------------------------------------------------------------------------------ 3. view-direction term
def backward_of(color, allmap, normals=True):
    wc, wa = PC.image_weights(color.shape, allmap.shape, normals)
    ((color * wc.to(color.device)).sum() + (allmap * wa.to(color.device)).sum()).backward()


def run_reference(dev, rs, s, *, shs=None, colors=None, precomp=None, opac=None, normals=True, wc_channels=None):
    """The reference signature with autograd -> images, radii and the gradients of the leaves."""
    from gaussmart_amd import rasterizer as R
    leaf = lambda t: None if t is None else t.detach().clone().to(dev).requires_grad_(True)
    means, op = leaf(s["xyz"]), leaf(s["opac"] if opac is None else opac)
    sc, q = (None, None) if precomp is not None else (leaf(s["scales"]), leaf(s["rots"]))
    col, pre = leaf(colors), leaf(precomp)
    m2d = torch.zeros_like(means, requires_grad=True)
    color, radii, allmap = R.rasterize_gaussians(means, m2d, shs, col, op, sc, q, pre, rs)
    wc, wa = PC.image_weights(color.shape, allmap.shape, normals)
    if wc_channels is not None:
        wc = wc * torch.tensor(wc_channels, dtype=torch.float32)[:, None, None]
        wa = wa * 0.0
    ((color * wc.to(dev)).sum() + (allmap * wa.to(dev)).sum()).backward()
    g = lambda t: None if t is None or t.grad is None else t.grad.detach().clone()
    return dict(color=color.detach(), allmap=allmap.detach(), radii=radii, dmean=g(means), dopac=g(op), dscales=g(sc), drots=g(q),
                dcolors=g(col), dT=g(pre))


def run_raw(dev, rs, s, *, cache=None, f_rest=None):
    """The raw signature, factored -> images, radii, the gradients and the factored record [N,3]."""
    from gaussmart_amd import rasterizer as R
    leaf = lambda t: t.detach().clone().to(dev).requires_grad_(True)
    p = {k: leaf(s[k]) for k in ("xyz", "f_dc", "opacity", "scaling", "rotation")}
    p["f_rest"] = leaf(s["f_rest"] if f_rest is None else f_rest)
    m2d = torch.zeros_like(p["xyz"], requires_grad=True)
    state = R.RasterState()
    color, radii, allmap = R.rasterize_gaussians_raw(p["xyz"], m2d, p["f_dc"], p["f_rest"], p["opacity"], p["scaling"], p["rotation"], rs,
                                                     factored_sh_grad=True, color_cache=cache, state=state)
    backward_of(color, allmap)
    n = s["xyz"].shape[0]
    rec = state.take_color_grad()
    return dict(color=color.detach(), allmap=allmap.detach(), radii=radii, dmean=p["xyz"].grad.clone(), dopac=p["opacity"].grad.clone(),
                dscales=p["scaling"].grad.clone(), drots=p["rotation"].grad.clone(), g=rec.record[:3 * n].view(n, 3).clone())


def assert_twins(main, twin, planes=slice(None)):
    """The preconditions: same pixels, same gradients of everything the view direction does not reach."""
    assert torch.equal(main["radii"], twin["radii"])
    assert torch.equal(main["color"], twin["color"]) and torch.equal(main["allmap"][planes], twin["allmap"][planes])
    for k in ("dopac", "dscales", "drots"):
        if main[k] is not None and twin[k] is not None:
            assert torch.equal(main[k], twin[k]), k


def term_reference(s, deg, g, words):
    c = PC.color_chain("bar", deg, s["sh"], s["xyz"], s["campos"])
    return PC.term_chain("bar", g.detach().cpu(), clamp_bits(words), c["J"], c["dir"], c["il"]), c


TERM_FORMS = ("unfactored staged", "unfactored misaligned", "raw factored", "raw factored staged", "raw factored cached")
TERM_DEGREES = [(3, 16), (2, 9), (1, 4), (0, 16)]


@pytest.mark.parametrize("form", TERM_FORMS)
@pytest.mark.parametrize("deg,M", TERM_DEGREES)
def test_view_direction_term_per_gaussian(gpu_device, held, monkeypatch, deg, M, form):
    dev = gpu_device
    monkeypatch.delenv("GSR_COLOR_STAGED", raising=False)
    s = PC.term_scene(deg, M)
    n = s["xyz"].shape[0]
    rs = hip_settings(s["cam"], deg=deg, device=dev)
    raw_args = dict(scales=to(dev, s["scaling"]), rotations=to(dev, s["rotation"]), raw_features=(to(dev, s["f_dc"]), to(dev, s["f_rest"])))
    if form.startswith("unfactored"):
        shs = misaligned(s["sh"], dev) if form.endswith("misaligned") else to(dev, s["sh"])
        d = debug(dev, rs, to(dev, s["xyz"]), to(dev, s["opac"]), shs=shs, scales=to(dev, s["scales"]), rotations=to(dev, s["rots"]))
        rgb = torch.where((d["radii"] > 0)[:, None], d["splat"][:, 15:18], torch.zeros(n, 3, device=dev))
        main = run_reference(dev, rs, s, shs=shs)
        twin = run_reference(dev, rs, s, colors=rgb)
        g = twin["dcolors"]
    else:
        if form.endswith("staged"):
            # the Jacobian path must be off (gsr_color_jac_available): leave a WRONG Jacobian in the pooled GEOM buffer first
            run_raw(dev, rs, s, f_rest=-s["f_rest"])
            monkeypatch.setenv("GSR_COLOR_STAGED", "1")
        cache = None
        if form.endswith("cached"):
            cs = dict(sh=s["sh"], means=s["xyz"], campos=s["campos"])
            cache, sh_after = cache_step(dev, cs, deg)
            assert torch.equal(sh_after, s["sh"])
            d = debug(dev, rs, to(dev, s["xyz"]), to(dev, s["opacity"]), color_cache=cache, **raw_args)
        else:
            d = debug(dev, rs, to(dev, s["xyz"]), to(dev, s["opacity"]), **raw_args)
        visible = d["radii"] > 0
        fake = torch.zeros(13 * n, dtype=torch.float32, device=dev)          # rgb, clamp words, J = 0
        fake[:3 * n] = torch.where(visible[:, None], d["splat"][:, 15:18], torch.zeros(n, 3, device=dev)).reshape(-1)
        fake[3 * n:4 * n] = torch.where(visible, d["clamped"], torch.zeros_like(d["clamped"])).view(torch.float32)
        main = run_raw(dev, rs, s, cache=cache)
        twin = run_raw(dev, rs, s, cache=fake)
        g = main["g"]
        assert torch.equal(main["g"], twin["g"])
    assert_twins(main, twin)
    vis = (d["radii"] > 0).cpu()
    term = (main["dmean"] - twin["dmean"]).cpu()
    truth, c = term_reference(s, deg, g, d["clamped"])
    if not form.startswith("unfactored"):
        # the record is the masked gradient already: masked channels are exactly 0
        assert bool((main["g"].cpu()[clamp_bits(d["clamped"]) & vis[:, None]] == 0).all())
    b = bar(truth) + U32 * (main["dmean"].abs().cpu().double() + twin["dmean"].abs().cpu().double())      # the final addition
    held(f"term {form} deg {deg} M {M}", "dL/dmean(main) - dL/dmean(twin)", term, truth.v, b, vis)
    assert bool((term[~vis] == 0).all())
    if deg == 0:
        assert float(term.abs().max()) == 0.0                        # no direction in the colour: the term is exactly zero
    else:
        assert float(truth.v[vis].abs().max()) > 100 * float(b[vis].max())       # loud: the term stands far above its bar


@pytest.mark.parametrize("form", ("unfactored staged", "raw factored"))
def test_a_clamped_channel_contributes_nothing(gpu_device, monkeypatch, form):
    """Channel 2 clamps on every Gaussian; with image weights on that channel alone the whole term is exactly zero."""
    dev = gpu_device
    monkeypatch.delenv("GSR_COLOR_STAGED", raising=False)
    s = PC.term_scene(3, 16, clamped_channel=2)
    n = s["xyz"].shape[0]
    rs = hip_settings(s["cam"], deg=3, device=dev)
    d = debug(dev, rs, to(dev, s["xyz"]), to(dev, s["opac"]), shs=to(dev, s["sh"]), scales=to(dev, s["scales"]), rotations=to(dev, s["rots"]))
    vis = d["radii"] > 0
    assert bool((d["clamped"][vis] & 4 == 4).all()) and bool((d["splat"][vis, 17] == 0).all()) and int(vis.sum()) > 500
    rgb = torch.where(vis[:, None], d["splat"][:, 15:18], torch.zeros(n, 3, device=dev))
    if form == "unfactored staged":
        main = run_reference(dev, rs, s, shs=to(dev, s["sh"]), wc_channels=(0.0, 0.0, 1.0))
        twin = run_reference(dev, rs, s, colors=rgb, wc_channels=(0.0, 0.0, 1.0))
        assert float(twin["dcolors"][:, 2].abs().max()) > 0          # the channel does receive a gradient; the clamp stops it
        assert_twins(main, twin)
        assert torch.equal(main["dmean"], twin["dmean"])
    else:
        # the raw operator has one set of image weights; the channel's own contribution: zero its entry of the record's gradient
        main = run_raw(dev, rs, s)
        assert bool((main["g"][:, 2] == 0).all()) and float(main["g"][:, :2].abs().max()) > 0
        g2 = torch.zeros(n, 3)
        truth, _ = term_reference(s, 3, g2, d["clamped"])
        assert float(truth.v.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. K8 chain
K8_CASES = {"facing": ("facing s0", False), "free": ("free s0", False), "modifier 0.7": ("facing s2 modifier 0.7", False),
            "free raw": ("free s3 raw", True), "facing raw": ("facing s4 raw", True)}


@pytest.mark.parametrize("name", list(K8_CASES))
def test_k8_chain_per_gaussian(gpu_device, held, monkeypatch, name):
    dev = gpu_device
    monkeypatch.delenv("GSR_COLOR_STAGED", raising=False)
    from gaussmart_amd import rasterizer as R
    key, raw = K8_CASES[name]
    c = dict(PC.random_case(key, 600, 128, 96))
    n = c["means"].shape[0]
    rs = hip_settings(c["cam"], deg=3, device=dev, scale_modifier=c["mod"])
    gen = torch.Generator().manual_seed(5)
    leaf = lambda t: t.detach().clone().to(dev).requires_grad_(True)
    if raw:
        c["rots"] = c["rots"].clone()
        c["rots"][7] *= 1e-13 / float(c["rots"][7].norm())           # |q|^2 = 1e-26: the kernel's qn2 < 1e-24 branch
        sh = torch.cat([c["f_dc"], 0.5 * torch.randn(n, 15, 3, generator=gen)], 1)
        raw_args = dict(scales=to(dev, c["scales"]), rotations=to(dev, c["rots"]), raw_features=(to(dev, sh[:, :1]), to(dev, sh[:, 1:])))
        d = debug(dev, rs, to(dev, c["means"]), to(dev, c["opac"]), **raw_args)
        p = dict(xyz=leaf(c["means"]), f_dc=leaf(sh[:, :1]), f_rest=leaf(sh[:, 1:]), opacity=leaf(c["opac"]), scaling=leaf(c["scales"]),
                 rotation=leaf(c["rots"]))
        m2d = torch.zeros_like(p["xyz"], requires_grad=True)
        color, radii, allmap = R.rasterize_gaussians_raw(p["xyz"], m2d, p["f_dc"], p["f_rest"], p["opacity"], p["scaling"], p["rotation"], rs)
        backward_of(color, allmap, normals=False)
        main = dict(color=color.detach(), allmap=allmap.detach(), radii=radii, dmean=p["xyz"].grad, dscales=p["scaling"].grad,
                    drots=p["rotation"].grad, dopac=None)
    else:
        col = torch.rand(n, 3, generator=gen)
        d = debug(dev, rs, to(dev, c["means"]), to(dev, c["opac"]), colors_precomp=to(dev, col), scales=to(dev, c["scales"]),
                  rotations=to(dev, c["rots"]))
        s = dict(xyz=c["means"], opac=c["opac"], scales=c["scales"], rots=c["rots"])
        main = run_reference(dev, rs, s, colors=col, normals=False)
    vis_d = d["radii"] > 0
    vis = vis_d.cpu()
    z = lambda t: torch.where(vis_d.reshape(-1, *[1] * (t.dim() - 1)), t, torch.zeros_like(t))
    # the twin: the record's own nine floats as transmat_precomp, its opacity and colour; its dL_dtransmat is the device's dT
    s_t = dict(xyz=c["means"], opac=z(d["splat"][:, 14:15]))
    twin = run_reference(dev, rs, s_t, colors=z(d["splat"][:, 15:18]), precomp=z(d["splat"][:, 0:9]), normals=False)
    assert_twins(main, dict(twin, dopac=None), planes=[0, 1, 5, 6])
    dT = twin["dT"].cpu()
    assert bool((dT[~vis] == 0).all()) and float(dT[vis].abs().max()) > 0
    truth = PC.bwd_chain("bar", dT, c["means"], c["scales"], c["rots"], c["view"], c["proj"], c["W"], c["H"], mod=c["mod"], raw=raw)
    case = f"K8 {name}"
    held_E(held, case, "dL/dscales", main["dscales"], truth["dscales"], vis)
    held_E(held, case, "dL/drotations", main["drots"], truth["drotations"], vis)
    want, b = truth["dmean"].v, bar(truth["dmean"])
    if raw:
        # with shs the mean also receives the view-direction term: the reference of part 3 on the device's own g, and its bar
        cc = PC.color_chain("bar", 3, sh, c["means"], c["campos"])
        term = PC.term_chain("bar", twin["dcolors"].cpu(), clamp_bits(d["clamped"]), cc["J"], cc["dir"], cc["il"])
        b = b + bar(term) + U32 * (want.abs() + term.v.abs())
        want = want + term.v
        assert float(main["drots"][7].abs().max()) > 1e6 * float(main["drots"][8].abs().max())
    held(case, "dL/dmean", main["dmean"], want, b, vis)
    for k in ("dmean", "dscales", "drots"):
        assert bool((main[k].cpu()[~vis] == 0).all()), k
