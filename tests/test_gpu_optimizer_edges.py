"""The optimiser kernels (gaussmart_amd/csrc/adam.hip) against the float64 reference of tests/adam_ref.py, one step at a
time, at the shapes and values where they can go wrong:

  D1-D4  dense step: slices off the 16-byte grid, sizes around the vector width and the block, a tensor that takes the
         grid-stride loop round twice, chunks of 8 tensors, two batch keys, gradients from 1e-30 to 1e15, keep_old;
  F1-F4  factored SH step: 16 / 9 / 4 / 1 coefficients, every active degree, waves with 1, 63, 64 and 65 Gaussians,
         1 / 3 / 16 views, ranges, zero gradients;
  C1-C2  the colour cache of the next view, evaluated from the coefficients the device wrote.

Every buffer a kernel writes lies between 64 guard floats; what a call must not touch is compared bit for bit.  The bars
are those of adam_ref (4 x the recorded fp32 level, tests/golden/adam_bars.json).  With GSR_ADAM_BARS_REPORT set, the
worst measured use of every bar per case group is written to that file."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu
G = A.GUARD


@pytest.fixture(scope="module", autouse=True)
def _bars_report():
    yield
    if A.USAGE:
        text = A.usage_report()
        out = os.environ.get("GSR_ADAM_BARS_REPORT")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                f.write(text + "\n")
        print("\n[optimiser bars]\n" + text)


def guarded(host, dev, shape=None):
    """(buffer, view): the host values between two runs of 64 sentinel floats, 16-byte aligned."""
    n = host.numel()
    buf = A.sentinel(n + 2 * G).to(dev)
    view = buf[G:G + n].view(host.shape if shape is None else shape)
    view.copy_(host.reshape(view.shape))
    assert view.data_ptr() % 16 == 0          # whole tensors take the 16-byte path, slices off the grid the scalar one
    return buf, view


def guards_intact(buf, what):
    n = buf.numel() - 2 * G
    A.check_untouched(A.sentinel(G), buf[:G], f"{what}: guard floats below")
    A.check_untouched(A.sentinel(G), buf[G + n:], f"{what}: guard floats above")


def dense_setup(cases, dev, shapes=None, groups=None):
    """FusedAdam over one guarded parameter per case, state and step count as the case says; gradients parked in s.g."""
    from gaussmart_amd.fused_adam import FusedAdam
    s = SimpleNamespace(cases=cases, bufs=[], p=[], g=[], m=[], v=[])
    for i, c in enumerate(cases):
        shape = None if shapes is None else shapes[i]
        for name, host in (("p", c.p), ("g", c.g), ("m", c.m), ("v", c.v)):
            buf, view = guarded(host, dev, shape)
            s.bufs.append((f"{c.name} {name}", buf))
            getattr(s, name).append(torch.nn.Parameter(view) if name == "p" else view)
    if groups is None:
        groups = [{"params": list(s.p), "lr": cases[0].lr, "betas": cases[0].betas, "eps": cases[0].eps}]
    else:
        groups = [{"params": [s.p[i] for i in idx], **kw} for idx, kw in groups]
    s.opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    for c, p, m, v in zip(cases, s.p, s.m, s.v):
        s.opt.state[p] = {"step": torch.tensor(float(c.t - 1)), "exp_avg": m, "exp_avg_sq": v}
    return s


def dense_read(s, i):
    return tuple(x[i].detach().cpu().reshape(-1) for x in (s.p, s.m, s.v))


def all_guards(s):
    torch.cuda.synchronize()
    for what, buf in s.bufs:
        guards_intact(buf, what)


# ------------------------------------------------------------------------------------------------------ dense step
@pytest.mark.parametrize("start", A.D1_STARTS)
def test_d1_slices(gpu_device, start):
    c = A.d1_case()
    s = dense_setup([c], gpu_device)
    p, old = s.p[0], (c.p, c.m, c.v)
    p.grad = s.g[0]
    for length in A.D1_LENGTHS:
        with torch.no_grad():
            p.copy_(c.p); s.m[0].copy_(c.m); s.v[0].copy_(c.v)
        s.opt.state[p]["step"] = torch.tensor(float(c.t - 1))
        cuts = (start, start + length, start + length + 5)
        before = old
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):          # the second slice of the iteration does not count
            s.opt.step_slice(p, a, b, count_step=k == 0)
            new = dense_read(s, 0)
            what = f"D1 [{a}, {b})"
            A.check_dense([x[a:b] for x in before], [x[a:b] for x in new], c.g[a:b], c.lr, c.t, c.betas, c.eps, "D1 slices", what)
            for name, x0, x1 in zip("pmv", before, new):
                A.check_untouched(x0[:a], x1[:a], f"{what}: {name} below the slice")
                A.check_untouched(x0[b:], x1[b:], f"{what}: {name} above the slice")
            assert float(s.opt.state[p]["step"]) == c.t
            before = new
    all_guards(s)


def test_d2_sizes_chunks_and_batch_keys(gpu_device):
    ca, cb = A.d2_cases(), A.d2_other_cases()
    na = len(ca)
    assert na == 13 and ca[-1].n == 4197379
    ia, ib = list(range(na)), list(range(na, na + len(cb)))
    s = dense_setup(ca + cb, gpu_device, shapes=list(A.D2_SHAPES) + list(A.D2_OTHER),
                    groups=[(ia, {"lr": ca[0].lr}), (ib, {"lr": cb[0].lr, "betas": cb[0].betas, "eps": cb[0].eps})])
    host = [(c.p, c.m, c.v) for c in s.cases]
    for first, idx in enumerate((ia, ib)):           # step 1: 13 tensors, launches of 8 and 5; step 2: the other batch key
        for i, p in enumerate(s.p):
            p.grad = s.g[i] if i in idx else None
        s.opt.step()
        for i, c in enumerate(s.cases):
            new = dense_read(s, i)
            if i in idx:
                A.check_dense(host[i], new, c.g, c.lr, c.t, c.betas, c.eps, "D2 sizes", f"{c.name} ({c.n} elements)")
                assert float(s.opt.state[s.p[i]]["step"]) == c.t
                host[i] = new
            else:
                for name, x0, x1 in zip("pmv", host[i], new):
                    A.check_untouched(x0, x1, f"{c.name}: {name} of a parameter without gradient")
        all_guards(s)


def test_d3_values(gpu_device):
    for c in A.d3_cases():
        assert c.n % 4 == 3 and float(c.g.abs().max()) >= 9e14 and float(c.g[c.g != 0].abs().min()) <= 2e-30
        s = dense_setup([c], gpu_device)
        s.p[0].grad = s.g[0]
        s.opt.step()
        new = dense_read(s, 0)
        A.check_dense((c.p, c.m, c.v), new, c.g, c.lr, c.t, c.betas, c.eps, "D3 values", c.name)
        assert all(bool(torch.isfinite(x).all()) for x in new)
        assert float(s.opt.state[s.p[0]]["step"]) == c.t
        all_guards(s)


def test_d3_fresh_state_zero_gradient(gpu_device):
    from gaussmart_amd.fused_adam import FusedAdam
    host = torch.randn(1027, generator=torch.Generator().manual_seed(5))
    buf, view = guarded(host, gpu_device)
    p = torch.nn.Parameter(view)
    p.grad = torch.zeros_like(p)
    opt = FusedAdam([p], lr=1e-3, eps=1e-15)
    opt.step()
    A.check_untouched(host, p, "p after a zero gradient on a fresh state")
    for k in ("exp_avg", "exp_avg_sq"):
        assert bool(torch.isfinite(opt.state[p][k]).all()) and float(opt.state[p][k].abs().max()) == 0.0
    guards_intact(buf, "p")


def _d4_run(dev, rows, with_grad=True):
    cases = A.d4_cases(rows)
    s = dense_setup(cases, dev, shapes=[(c.n,) for c in cases[:-1]] + [(rows, 3)])
    for i, p in enumerate(s.p):
        p.grad = s.g[i]
    if not with_grad:
        s.p[-1].grad = None
    s.old_buf, s.old = guarded(torch.zeros(rows, 3), dev)
    s.old.view(torch.int32).fill_(A.SENTINEL)
    s.opt.step(keep_old=(s.p[-1], s.old))
    torch.cuda.synchronize()
    return s


@pytest.mark.parametrize("rows", A.D4_ROWS)
def test_d4_keep_old(gpu_device, rows):
    s = _d4_run(gpu_device, rows)
    kept = s.cases[-1]
    assert len(s.cases) == 9                                   # the kept parameter is alone in the second launch
    A.check_untouched(kept.p, s.old.reshape(-1), "old: the parameter before the step")
    assert not torch.equal(s.p[-1].detach().cpu().reshape(-1), kept.p)
    for i, c in enumerate(s.cases):
        A.check_dense((c.p, c.m, c.v), dense_read(s, i), c.g, c.lr, c.t, c.betas, c.eps, "D4 keep_old", c.name)
    guards_intact(s.old_buf, "old")
    all_guards(s)
    again = _d4_run(gpu_device, rows)                          # two identical runs: the same bits
    for i in range(len(s.cases)):
        for name, x0, x1 in zip("pmv", dense_read(s, i), dense_read(again, i)):
            A.check_untouched(x0, x1, f"{s.cases[i].name}: {name} of a second identical run")
    A.check_untouched(s.old, again.old, "old of a second identical run")


def test_d4_keep_old_without_gradient_copies(gpu_device):
    s = _d4_run(gpu_device, 5, with_grad=False)
    kept = s.cases[-1]
    A.check_untouched(kept.p, s.old.reshape(-1), "old: copy of a parameter that took no update")
    for name, x0, x1 in zip("pmv", (kept.p, kept.m, kept.v), dense_read(s, len(s.cases) - 1)):
        A.check_untouched(x0, x1, f"{name} of the parameter without gradient")
    guards_intact(s.old_buf, "old")
    all_guards(s)


# ------------------------------------------------------------------------------------------------ factored SH step
def sh_setup(c, dev, cache=False):
    from gaussmart_amd.fused_adam import FusedAdam
    s = SimpleNamespace(case=c, bufs=[])
    parts = {}
    for name, host in (("p", c.p), ("m", c.m), ("v", c.v)):
        for part, sl in (("dc", slice(0, 1)), ("rest", slice(1, None))):
            buf, view = guarded(host[:, sl].contiguous(), dev)
            s.bufs.append((f"{c.name} {name}_{part}", buf))
            parts[name, part] = view
    s.parts = parts
    s.f_dc, s.f_rest = torch.nn.Parameter(parts["p", "dc"]), torch.nn.Parameter(parts["p", "rest"])
    s.opt = FusedAdam([{"params": [s.f_dc], "lr": c.lr_dc}, {"params": [s.f_rest], "lr": c.lr_rest}], lr=0.0, eps=c.eps)
    sh_reset(s)
    s.xyz, s.records = c.xyz.to(dev), c.records.to(dev)
    if cache:
        s.cache_buf, s.cache = guarded(A.sentinel(13 * c.N), dev)
        s.bufs.append((f"{c.name} cache", s.cache_buf))
        s.xyz_next, s.campos_next = c.xyz_next.to(dev), c.campos_next.to(dev)
    return s


def sh_reset(s):
    """The state of the case again: parameters, moments, step count t - 1."""
    c = s.case
    with torch.no_grad():
        for name, host in (("p", c.p), ("m", c.m), ("v", c.v)):
            s.parts[name, "dc"].copy_(host[:, :1])
            s.parts[name, "rest"].copy_(host[:, 1:])
    for q, part in ((s.f_dc, "dc"), (s.f_rest, "rest")):
        s.opt.state[q] = {"step": torch.tensor(float(c.t - 1)), "exp_avg": s.parts["m", part], "exp_avg_sq": s.parts["v", part]}


def sh_read(s):
    torch.cuda.synchronize()
    return tuple(A.sh_pack(s.parts[name, "dc"], s.parts[name, "rest"]) for name in "pmv")


def sh_step(s, first=0, count=None, **kw):
    c = s.case
    s.opt.step_sh_factored(s.f_dc, s.f_rest, s.xyz, s.records, c.views, c.stride, c.deg, c.grad_scale, first=first,
                           count=count, **kw)
    assert float(s.opt.state[s.f_dc]["step"]) == c.t and float(s.opt.state[s.f_rest]["step"]) == c.t


@pytest.mark.parametrize("M,N", [(M, N) for M, sizes in A.F1_SIZES.items() for N in sizes])
def test_f1_coefficients_and_sizes(gpu_device, M, N):
    cases = A.f1_cases(M, N)
    assert len(cases) == 3 * (A.SH_DEGREE_OF[M] + 1)
    for c in cases:
        s = sh_setup(c, gpu_device)
        sh_step(s)
        A.check_factored(c, (c.p, c.m, c.v), sh_read(s), group=f"F1 M{M}", what=c.name)
        all_guards(s)


@pytest.mark.parametrize("M", list(A.F1_SIZES))
def test_f2_ranges(gpu_device, M):
    c = A.f2_case(M)
    s = sh_setup(c, gpu_device)
    old = (c.p, c.m, c.v)
    for first in A.F2_FIRSTS:
        for count in A.f2_counts(first):
            sh_reset(s)
            sh_step(s, first, count)
            new = sh_read(s)
            what = f"{c.name} [{first}, {first + count})"
            A.check_factored(c, old, new, slice(first, first + count), f"F2 M{M}", what)
            for name, x0, x1 in zip("pmv", old, new):
                A.check_untouched(x0[:first], x1[:first], f"{what}: {name} below the range")
                A.check_untouched(x0[first + count:], x1[first + count:], f"{what}: {name} above the range")
    all_guards(s)


def test_f3_zero_gradients(gpu_device):
    c = A.factored_case(257, 16, 3, 3, 5300, name="F3")
    s = sh_setup(c, gpu_device)
    sh_step(s)
    p1, m1, v1 = sh_read(s)
    idx = torch.arange(c.N)
    g = c.records.view(c.views, c.stride)[:, :3 * c.N].view(c.views, c.N, 3)
    never = idx[(g == 0).all(dim=2).all(dim=0)]
    once = idx[(g == 0).all(dim=2).sum(dim=0) == 1]
    assert never.numel() >= 50 and once.numel() >= 40
    for rows, what in ((never, "no gradient in any view"), (once, "no gradient in one view")):
        A.check_factored(c, (c.p, c.m, c.v), (p1, m1, v1), rows, "F3 zero gradients", what)
    # without a gradient the moments decay and the parameter moves by momentum
    assert bool((m1[never].abs() < c.m[never].abs()).all()) and bool((v1[never] < c.v[never]).all())
    assert bool((p1[never] != c.p[never]).all())
    all_guards(s)


def test_f4_one_coefficient(gpu_device):
    """features_rest of shape [N, 0, 3]: either the step is right or it is refused; nothing in between."""
    from gaussmart_amd import _lib
    c = A.f4_case()
    s = sh_setup(c, gpu_device)
    assert s.f_rest.shape == (c.N, 0, 3)
    try:
        sh_step(s)
    except _lib.GsrError:
        for name, x0, x1 in zip("pmv", (c.p, c.m, c.v), sh_read(s)):
            A.check_untouched(x0, x1, f"{name} after a refused step")
        return
    A.check_factored(c, (c.p, c.m, c.v), sh_read(s), group="F4 M1", what=c.name)
    all_guards(s)


# ---------------------------------------------------------------------------------------------------- colour cache
@pytest.mark.parametrize("M,N", [(M, N) for M in A.F1_SIZES for N in A.C1_SIZES])
def test_c1_cached_colours(gpu_device, M, N):
    cases = A.c1_cases(M, N)
    assert len(cases) == 2 * A.SH_DEGREE_OF[M] + 1
    for c in cases:
        s = sh_setup(c, gpu_device, cache=True)
        s.opt._cache_buf = s.cache
        sh_step(s, next_view=(s.campos_next, c.deg_next), xyz_next=s.xyz_next)
        assert s.opt.color_cache is not None and s.opt.color_cache[1].data_ptr() == s.cache.data_ptr()
        assert s.opt.lookup_color_cache(s.campos_next, c.deg_next, s.xyz_next, s.f_dc, s.f_rest) is not None
        new = sh_read(s)
        A.check_factored(c, (c.p, c.m, c.v), new, group=f"C1 M{M}", what=c.name)
        A.check_cache(s.cache, new[0], c.xyz_next, c.campos_next, c.deg_next, exact_rows=c.exact_rows, group=f"C1 M{M}",
                      what=c.name)
        all_guards(s)


@pytest.mark.parametrize("M", list(A.F1_SIZES))
def test_c2_cache_of_a_sub_range(gpu_device, M):
    from gaussmart_amd import _lib
    c = A.c2_case(M)
    assert (c.first, c.count, c.N) == (64, 65, 257)
    s = sh_setup(c, gpu_device, cache=True)
    b1, b2 = c.betas
    ss = lambda lr: lr / (1.0 - b1 ** c.t)
    ib = 1.0 / math.sqrt(1.0 - b2 ** c.t)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    P = s.parts
    with torch.cuda.device(gpu_device):
        _lib.check(_lib.lib().gsr_adam_sh_factored_next(
            c.first, c.count, c.M, c.deg, ptr(s.xyz), c.views, ptr(s.records), c.stride,
            C.c_void_p(s.records.data_ptr() + 12 * c.N), c.stride, c.grad_scale,
            ptr(P["p", "dc"]), ptr(P["m", "dc"]), ptr(P["v", "dc"]), ss(c.lr_dc), ib,
            ptr(P["p", "rest"]), ptr(P["m", "rest"]), ptr(P["v", "rest"]), ss(c.lr_rest), ib,
            b1, b2, c.eps, ptr(s.xyz_next), ptr(s.campos_next), c.deg_next, c.N, ptr(s.cache),
            C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)))
    old, new = (c.p, c.m, c.v), sh_read(s)
    rows = slice(c.first, c.first + c.count)
    A.check_factored(c, old, new, rows, f"C2 M{M}", c.name)
    for name, x0, x1 in zip("pmv", old, new):
        A.check_untouched(x0[:c.first], x1[:c.first], f"{c.name}: {name} below the range")
        A.check_untouched(x0[c.first + c.count:], x1[c.first + c.count:], f"{c.name}: {name} above the range")
    A.check_cache(s.cache, new[0], c.xyz_next, c.campos_next, c.deg_next, c.first, c.count, before=A.sentinel(13 * c.N),
                  exact_rows=c.exact_rows, group=f"C2 M{M}", what=c.name)
    all_guards(s)
