"""The chains and bars of tests/pergaussian_cases.py without a GPU: the fp64 chains against oracle/surfel_ref.py and autograd, the
reachability of every bar (the kernels' formulations in torch fp32 stay within it on every case and field), its tightness (each
wrong reading of a kernel listed there, applied to the fp32 twin, leaves a bar on some case of its part) and the conditions the
inputs were chosen for (clamp share, share of excused decisions).  tests/test_gpu_pergaussian_parity.py holds the kernels to the
same bars.  GSR_PERGAUSSIAN_PARITY_REPORT=<file>: one line per mutation is appended there."""
import os

import pytest
import torch
import torch.nn.functional as F

import pergaussian_cases as PC
from conftest import oracle_settings
from objective_cases import bar, f32
from oracle import surfel_ref as O

GEOM = PC.geom_cases()


def report(line):
    out = os.environ.get("GSR_PERGAUSSIAN_PARITY_REPORT")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


def activated64(c):
    """The case's parameters as the oracle takes them, in fp64."""
    sc, q, o = c["scales"].double(), c["rots"].double(), c["opac"].double()
    if c["raw"]:
        sc, q, o = torch.exp(sc), F.normalize(q), torch.sigmoid(o)
    return c["means"].double(), sc, q, o.reshape(-1, 1)


# ------------------------------------------------------------------------------------------------ K1 geometry
@pytest.mark.parametrize("name", list(GEOM))
def test_geom_fp64_chain_is_the_oracle(name):
    c = GEOM[name]()
    n = c["means"].shape[0]
    d = PC.geom_run("f64", c)
    S = oracle_settings(c["cam"], 3, torch.float64, scale_modifier=f32(c["mod"]))
    m, sc, q, o = activated64(c)
    pre = c["precomp"].double() if c["precomp"] is not None else None
    g = O.preprocess(m, sc, q, o, None, torch.zeros(n, 3, dtype=torch.float64), pre, S)
    vi = g.vis_idx
    assert torch.equal(torch.nonzero(d["vis"]).flatten(), vi)
    assert torch.equal(d["radii"], g.radii) and torch.equal(d["rect"].int(), g.rect)
    Tm = torch.stack([d["Tu"], d["Tv"], d["Tw"]], 1)[vi]
    scale = g.Tm.abs().amax((1, 2))                                  # relative to the Gaussian's own matrix
    assert float(((Tm - g.Tm).abs().amax((1, 2)) / scale).max()) <= 1e-12
    # the centre is a cancelling quotient: relative to the magnitude of its terms sum |f_i T_i Tw_i| >= |c|
    t9 = torch.tensor([9.0, 9.0, -1.0], dtype=torch.float64)
    fi = t9 / (t9 * g.Tm[:, 2] ** 2).sum(-1, keepdim=True)
    mag = torch.stack([(fi * g.Tm[:, 0] * g.Tm[:, 2]).abs().sum(-1), (fi * g.Tm[:, 1] * g.Tm[:, 2]).abs().sum(-1)], -1)
    assert float(((d["xy"][vi] - g.xy).abs() / mag.clamp_min(1.0)).max()) <= 1e-12
    assert float((d["normal"][vi] - g.normal).abs().max()) <= 1e-12
    assert float(((d["depth"][vi] - g.depth).abs() / g.depth.abs()).max()) <= 1e-12          # the float whose bits are depth_key
    assert float((d["opacity"][vi] - o[vi, 0]).abs().max()) <= 1e-12


def geom_use(got, truth):
    """Worst err / bar per field over the Gaussians visible in both runs, and the discrete mismatches outside the excused."""
    both = truth["vis"] & got["vis"]
    use = {k: PC.use_of(got[k], truth[k], both)[0] for k in PC.GEOM_FIELDS}
    ex = truth["excused"]
    wrong = dict(vis=int((got["vis"] != truth["vis"])[~ex["vis"]].sum()),
                 radius=int((got["radii"] != truth["radii"])[~ex["radius"]].sum()),
                 rect=int((got["rect"] != truth["rect"]).any(1)[~ex["rect"]].sum()))
    return use, wrong


@pytest.mark.parametrize("name", list(GEOM))
def test_geom_bars_are_reachable_and_cases_decided(name):
    """The kernel's formulation in torch fp32 stays within every bar and takes every decision that is not excused as fp64 does;
    at most 2 % of a random case, and nothing of an edge case, is excused."""
    c = GEOM[name]()
    n = c["means"].shape[0]
    truth = PC.geom_run("bar", c)
    use, wrong = geom_use(PC.geom_run("f32", c), truth)
    share = {k: int(v.sum()) / n for k, v in truth["excused"].items()}
    print(name, {k: round(v, 3) for k, v in use.items()}, wrong, share)
    assert max(use.values()) <= 1.0 and not any(wrong.values()), (use, wrong)
    if name.startswith("random"):
        assert max(share.values()) <= 0.02, share
        assert 0.8 * n <= int(truth["vis"].sum()) < n                # most are visible, some are culled
    elif name.startswith("edges"):
        bad = [c["labels"][i] for i in torch.nonzero(truth["excused"]["radius"] | truth["excused"]["rect"]).flatten().tolist()]
        assert not bad, bad
        assert 150 <= n <= 250
    else:
        assert max(share.values()) == 0.0


def test_edge_cases_reach_the_edges_they_name():
    for w, h in PC.EDGE_SIZES:
        c = PC.edge_case(w, h)
        t = PC.geom_run("bar", c)
        lab = c["labels"]
        sel = lambda s: torch.tensor([s in l for l in lab])
        vis, radii, rect = t["vis"], t["radii"], t["rect"]
        near = sel("near plane")
        z = t["depth"].v[near]
        assert bool((vis[near] == (z > 0.2)).all()) and bool((z > 0.2).any()) and bool((z < 0).any())
        assert float((z[(z > 0) & (z < 0.2)] / 0.2 - 1).abs().max()) < 2.0 ** -9
        for side in ("left", "right", "top", "bottom"):
            assert bool(vis[sel(f"{side} border +2")].all()) and not bool(vis[sel(f"{side} border -2")].any()), side
        assert not bool(vis[sel("off screen")].any())
        assert bool((radii[sel("sub-pixel")] == 3).all())
        big = sel("radius ")
        assert int(radii[big].max()) == 100001 and int(radii[big].min()) == w + h + 1
        assert bool((rect[big] == torch.tensor([0, 0, (w + 15) // 16, (h + 15) // 16])).all())
        corners = t["xy"].v[sel("tile corner")]
        assert float((corners / 16 - torch.round(corners / 16)).abs().max()) < 1e-6
        tilt = sel("tilt 89.9")
        cosn = t["normal"].v[tilt, 2].abs()                          # the view ray is +z there
        assert float(cosn.max()) < 2e-3 and bool(vis[tilt].all())
        plane = sel("from the camera")
        to_centre = c["means"][plane].double()                       # the camera sits at the origin
        assert float(((to_centre * t["normal"].v[plane]).sum(-1).abs() - 1e-3).abs().max()) < 1e-5
        dz = sel("z^2 from zero")
        Tw = t["Tw"].v[dz]
        dval = 9 * (Tw[:, 0] ** 2 + Tw[:, 1] ** 2) - Tw[:, 2] ** 2
        assert float(((dval / Tw[:, 2] ** 2).abs() - 0.1).abs().max()) < 0.02 and bool((dval > 0).any()) and bool((dval < 0).any())
        qn = c["rots"][sel("quaternion norm")].norm(dim=1)
        assert float(qn.min()) < 1.1e-3 and float(qn.max()) > 0.9e3


def _geom_mutant_factor(name, mut):
    """(the largest error of the mutated fp32 twin / bar over the fields of one case, its wrong decisions outside the excused)."""
    c = GEOM[name]()
    truth = PC.geom_run("bar", c)
    use, wrong = geom_use(PC.geom_run("f32", c, mut=(mut,)), truth)
    return max(use.values()), sum(wrong.values())


@pytest.mark.parametrize("mut", PC.GEOM_MUTATIONS)
def test_geom_bars_are_tight(mut):
    both = {name: _geom_mutant_factor(name, mut) for name in GEOM}
    factors = {name: (float("inf") if w else f) for name, (f, w) in both.items()}
    best = max(both, key=lambda k: (both[k][0] if both[k][0] == both[k][0] else 0.0, both[k][1]))
    if mut == "aabb_min_ext2_dropped":
        # an equivalent mutant (see pergaussian_cases.GEOM_MUTATIONS): the record and every decision are those of the kernel's text
        for name in GEOM:
            c = GEOM[name]()
            a, b = PC.geom_run("f32", c), PC.geom_run("f32", c, mut=(mut,))
            assert all(torch.equal(a[k], b[k]) for k in PC.GEOM_FIELDS + ("vis", "radii", "rect")), name
        report(f"mutation geom {mut}: equivalent -- GSR_AABB_MIN_EXT2 (0.01 px) lies below the radius floor, no output depends on it")
        return
    report(f"mutation geom {mut}: caught by {sum(f > 1 for f in factors.values())} of {len(factors)} cases, worst '{best}': a field at "
           f"{both[best][0]:.3g} bars, {both[best][1]} decided results differ")
    assert max(factors.values()) > 1.0, factors


# ------------------------------------------------------------------------------------------------ SH colour
def _color_runs(deg, M, n, **kw):
    sh, means, campos = PC.color_case(deg, M, n)
    return PC.color_chain(kw.pop("mode", "f32"), deg, sh, means, campos, **kw)


@pytest.mark.parametrize("deg,M", PC.COLOR_GRID)
def test_color_fp64_chain_is_the_oracle_and_autograd(deg, M):
    clamped = total = 0
    for n in PC.COLOR_NS:
        sh, means, campos = PC.color_case(deg, M, n)
        c = PC.color_chain("f64", deg, sh, means, campos)
        rgb, cl = O.eval_sh_rgb(deg, sh.double(), means.double(), campos.double())
        assert float((c["rgb"] - rgb).abs().max()) <= 1e-12 and torch.equal(c["clamp"], cl)
        clamped, total = clamped + int(cl.sum()), total + cl.numel()
        # J against autograd of the written polynomials, x, y, z independent leaves
        x, y, z = (t.detach().clone().requires_grad_(True) for t in c["dir"])
        n_act = min(M, (deg + 1) ** 2)
        b, _, _, _ = PC.sh_polynomials("f64", x, y, z, n_act)
        v = sum(b[k][:, None] * sh[:, k].double() for k in range(n_act))
        for ch in range(3):
            gr = torch.autograd.grad(v[:, ch].sum(), (x, y, z), retain_graph=True, allow_unused=True)
            gr = torch.stack([g if g is not None else torch.zeros_like(x) for g in gr], -1)
            assert float((c["J"][:, ch] - gr).abs().max()) <= 1e-12, ch
        # J (I - d d^T) / |o| against autograd of the oracle's unclamped colour with respect to the mean
        mm = means.double().clone().requires_grad_(True)
        out_rgb = O.eval_sh_rgb(deg, sh.double(), mm, campos.double())[0] + 0.0 * mm.sum()       # (degree 0 does not depend on it)
        mx = lambda t_: float(t_.max()) if t_.numel() else 0.0
        for ch in range(3):
            keep = ~cl[:, ch]
            gm = torch.autograd.grad(out_rgb[:, ch].sum(), mm, retain_graph=True)[0]
            onehot = torch.zeros(n, 3, dtype=torch.float64); onehot[:, ch] = 1.0
            t = PC.term_chain("f64", onehot, torch.zeros(n, 3, dtype=torch.bool), c["J"], c["dir"], c["il"])
            assert mx((t[keep] - gm[keep]).abs()) <= 1e-11 * max(1.0, float(c["il"].max())), ch
            assert mx(gm[~keep].abs()) == 0.0                                  # a clamped channel has no gradient
    print(deg, M, "clamped", clamped, "of", total)
    assert 0.2 <= clamped / total <= 0.6


def test_color_cases_hold_the_directions_they_name():
    for n in PC.COLOR_NS:
        sh, means, campos = PC.color_case(3, 16, n)
        o = (means - campos).double()
        if n > 5:
            d = o / o.norm(dim=1, keepdim=True)
            for axis in range(3):
                assert bool(((d[:, axis].abs() - 1).abs() < 1e-6).any()), axis
            assert bool(((o[:, 0] - o[:, 1]).abs() < 1e-6).any())
        assert bool(((o.norm(dim=1) - 0.25).abs() < 1e-3).any())
        assert float(sh[:, 1:].std()) > 0.4 if n > 30 else True


def _color_use(got, truth):
    use = {"rgb": PC.use_of(got["rgb"], truth["rgb"])[0], "J": PC.use_of(got["J"], truth["J"])[0]}
    decided = (truth["v"].v.abs() > bar(truth["v"]))
    wrong = int((got["clamp"] != truth["clamp"])[decided].sum())
    zero = bool((got["rgb"][got["clamp"]] == 0).all())
    return use, wrong, zero, int((~decided).sum())


@pytest.mark.parametrize("form", ["written", "table"])
@pytest.mark.parametrize("deg,M", PC.COLOR_GRID)
def test_color_bars_are_reachable(deg, M, form):
    """Both fp32 formulations -- the written polynomials summed in sequence, and the 16-lane kernel's table form summed by its
    DPP tree -- stay within the bars of rgb and J; the clamp decisions agree wherever |v + 0.5| exceeds its bar."""
    for n in PC.COLOR_NS:
        truth = PC.color_truth(deg, M, n)
        use, wrong, zero, undecided = _color_use(_color_runs(deg, M, n, form=form), truth)
        print(deg, M, n, form, {k: round(v, 3) for k, v in use.items()}, "undecided clamps", undecided)
        assert max(use.values()) <= 1.0 and wrong == 0 and zero, (n, use, wrong)


@pytest.mark.parametrize("mut", PC.COLOR_MUTATIONS)
def test_color_bars_are_tight(mut):
    factors = {}
    for deg, M in PC.COLOR_GRID:
        for n in PC.COLOR_NS:
            use, wrong, _, _ = _color_use(_color_runs(deg, M, n, mut=(mut,)), PC.color_truth(deg, M, n))
            factors[(deg, M, n)] = (max(use.values()), wrong)
    best = max(factors, key=factors.get)
    caught = sum(f > 1 or w > 0 for f, w in factors.values())
    report(f"mutation colour {mut}: caught by {caught} of {len(factors)} cases, worst (deg, M, N) = {best}: rgb or J at "
           f"{factors[best][0]:.3g} bars, {factors[best][1]} decided clamp bits differ")
    assert factors[best][0] > 1.0


# ------------------------------------------------------------------------------------------------ view-direction term
def _term_inputs(deg, M, n):
    g = torch.Generator().manual_seed(31 * deg + M + n)
    return torch.randn(n, 3, generator=g) * 1e-3


def _term(mode, deg, M, n, mut=(), clamp_from=None):
    sh, means, campos = PC.color_case(deg, M, n)
    c = PC.color_chain(mode, deg, sh, means, campos, mut=tuple(m for m in mut if m in PC.COLOR_MUTATIONS and m != "jac_transposed"))
    clamp = c["clamp"] if clamp_from is None else clamp_from
    return PC.term_chain(mode, _term_inputs(deg, M, n), clamp, c["J"], c["dir"], c["il"], mut=mut), c["clamp"]


@pytest.mark.parametrize("deg,M", PC.COLOR_GRID)
def test_term_bars_are_reachable(deg, M):
    for n in PC.COLOR_NS:
        truth, clamp = _term("bar", deg, M, n)
        got, _ = _term("f32", deg, M, n, clamp_from=clamp)
        use = PC.use_of(got, truth)[0]
        print(deg, M, n, round(use, 3))
        assert use <= 1.0
        if deg == 0:
            assert float(truth.v.abs().max()) == 0.0 and float(got.abs().max()) == 0.0      # no direction, no term


@pytest.mark.parametrize("mut", PC.TERM_MUTATIONS)
def test_term_bars_are_tight(mut):
    factors = {}
    for deg, M in PC.COLOR_GRID:
        for n in PC.COLOR_NS:
            truth, clamp = _term("bar", deg, M, n)
            got, _ = _term("f32", deg, M, n, mut=(mut,), clamp_from=clamp)
            factors[(deg, M, n)] = PC.use_of(got, truth)[0]
    best = max(factors, key=factors.get)
    report(f"mutation term {mut}: caught by {sum(f > 1 for f in factors.values())} of {len(factors)} cases, worst (deg, M, N) = {best} at {factors[best]:.3g} bars")
    assert factors[best] > 1.0


# ------------------------------------------------------------------------------------------------ K8 chain
BWD_CASES = ["facing s0", "free s0", "facing s2 modifier 0.7", "free s3 raw", "facing s4 raw"]


def bwd_case(name, n=600):
    c = dict(PC.random_case(name, n, 128, 96))
    if c["raw"]:
        c["rots"] = c["rots"].clone()
        c["rots"][7] *= 1e-13 / float(c["rots"][7].norm())           # below the 1e-12 of F.normalize: the kernel's qn2 < 1e-24 branch
    g = torch.Generator().manual_seed(n + len(name))
    c["dT"] = torch.randn(n, 9, generator=g) * torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 30.0, 30.0, 30.0]) * 1e-3
    return c


def _bwd(mode, c, mut=()):
    return PC.bwd_chain(mode, c["dT"], c["means"], c["scales"], c["rots"], c["view"], c["proj"], c["W"], c["H"], mod=c["mod"],
                        raw=c["raw"], mut=mut)


@pytest.mark.parametrize("name", BWD_CASES)
def test_bwd_fp64_chain_is_autograd_of_the_geometry_chain(name):
    c = bwd_case(name)
    m, sc, q = (c[k].double().clone().requires_grad_(True) for k in ("means", "scales", "rots"))
    sa, qa = (torch.exp(sc), F.normalize(q)) if c["raw"] else (sc, q)          # scene/gaussian_model.py:37-43
    t = PC.preprocess_one("f64", m, sa, qa, c["opac"], c["view"], c["proj"], c["W"], c["H"], mod=c["mod"])
    T = torch.cat([t["Tu"], t["Tv"], t["Tw"]], 1)
    gm, gs, gq = torch.autograd.grad((T * c["dT"].double()).sum(), (m, sc, q))
    got = _bwd("f64", c)
    for k, want in (("dmean", gm), ("dscales", gs), ("drotations", gq)):
        scale = want.abs().amax(1, keepdim=True).clamp_min(1e-30)
        assert float(((got[k] - want).abs() / scale).max()) <= 1e-9, k
    if c["raw"]:
        assert float(gq[7].abs().max()) > 1e6 * float(gq[8].abs().max())         # the tiny quaternion: a gradient of 1 / |q|


@pytest.mark.parametrize("name", BWD_CASES)
def test_bwd_bars_are_reachable(name):
    c = bwd_case(name)
    truth, got = _bwd("bar", c), _bwd("f32", c)
    use = {k: PC.use_of(got[k], truth[k])[0] for k in truth}
    print(name, {k: round(v, 3) for k, v in use.items()})
    assert max(use.values()) <= 1.0


@pytest.mark.parametrize("mut", PC.BWD_MUTATIONS)
def test_bwd_bars_are_tight(mut):
    factors = {}
    for name in BWD_CASES:
        c = bwd_case(name)
        truth, got = _bwd("bar", c), _bwd("f32", c, mut=(mut,))
        factors[name] = max(PC.use_of(got[k], truth[k])[0] for k in truth)
    best = max(factors, key=factors.get)
    report(f"mutation K8 {mut}: caught by {sum(f > 1 for f in factors.values())} of {len(factors)} cases, worst '{best}' at {factors[best]:.3g} bars")
    assert factors[best] > 1.0
