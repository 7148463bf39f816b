"""Float64 reference of the optimiser kernels (gaussmart_amd/csrc/adam.hip) and the checkers every optimiser test shares.

What is compared, and on which scale (the figures a checker returns are already divided by these):

  one step, never a trajectory   the reference starts from the fp32 state the side under test started from;
  moments against the gradient   m: max(|m_old|, G) + FLT_MIN;  v: v_new + (1 - b2) G^2 + FLT_MIN, with G = |g| for the
                                 dense step and G = grad_scale * sum_views |basis_k| |g_view|, the cancellation-free
                                 magnitude of the sum, for the factored SH step;
  parameter against the moments  p_ref = p_old - step_size * m / (sqrt(v) * inv_bc2_sqrt + eps) in float64 from the m, v
                                 the side under test STORED; scale 2^-24 |p_old| + 2^-23 |update|.  The ill-conditioned
                                 m / sqrt(v) of near-zero gradients never enters a comparison: "moments follow the
                                 gradient" plus "parameter follows the moments" is the whole step;
  colour cache                   rgb: sum_k |basis_k sh_k| + 0.5;  J: sum_k |d basis_k| |sh_k|;  clamp bits equal wherever
                                 |sum + 0.5| of the reference exceeds the rgb bar, the band inside it is counted;
  untouched                      bit-identical (compared as int32).
A scale of exactly zero (a Jacobian at degree 0, a zero parameter that takes no update) admits no error at all.

The bars are 4 x the level at which plain fp32 torch (torch.optim.Adam(foreach=False), sh_basis in fp32) restates the
same operations on exactly the inputs below (tests/golden/make_adam_bars.py -> tests/golden/adam_bars.json).  The kernels
order a handful of roundings differently (m + (g - m)(1 - b1) against lerp, a product with 1 / sqrt(1 - b2^t) against a
quotient, contracted multiply-adds): about one level each.  What has to be caught sits far above: 1 - b2 formed in fp32 is
off by 1.3e-5 relative.  The factor was fixed before the kernels were ever measured against these bars.

The inputs of every case are built here, on the host, from seeds: the generator, the GPU tests
(tests/test_gpu_optimizer_edges.py) and the CPU tests of the checkers (tests/test_adam_ref_cpu.py) see the same numbers.
"""
import json
import math
import os
from types import SimpleNamespace

import torch

from gaussmart_amd.sh import sh_basis

FLT_MIN = 1.1754943508222875e-38
BARS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_bars.json")
QUANTITIES = ("m", "v", "p", "m_sh", "v_sh", "rgb", "J")
MARGIN = 4.0
with open(BARS_FILE) as _f:
    LEVELS = json.load(_f)["levels"]
BARS = {q: MARGIN * float(LEVELS[q]) for q in QUANTITIES}

# worst (error / bar) per case group and quantity of this process: what the GPU run reports (usage_report)
USAGE = {}


def _note(group, q, err):
    if group is not None:
        u = USAGE.setdefault(group, {})
        use = err / BARS[q]
        u[q] = use if use != use else max(u.get(q, 0.0), use)      # a NaN stays visible


def usage_report():
    lines = ["bars (4 x recorded fp32 level): " + "  ".join(f"{q} {BARS[q]:.3e}" for q in QUANTITIES),
             "worst measured error / bar per case group:"]
    for group in sorted(USAGE):
        lines.append(f"  {group:<24s} " + "  ".join(f"{q} {USAGE[group][q]:.3f}" for q in QUANTITIES if q in USAGE[group]))
    return "\n".join(lines)


def _host(x, dtype=torch.float64):
    return x.detach().cpu().to(dtype)


def _scaled(diff, scale):
    """Largest diff / scale; where the scale is exactly zero any difference is infinite.  NaN propagates."""
    if diff.numel() == 0:
        return 0.0
    inf = torch.full_like(diff, math.inf)
    err = torch.where(scale > 0, diff / scale, torch.where(diff == 0, torch.zeros_like(diff), inf))
    return float(err.max())


# ---------------------------------------------------------------------------------------------------- references
def dense_step(p, g, m, v, lr, t, betas, eps):
    """One torch-Adam step (no weight decay, no amsgrad) in float64 from fp32 inputs -> (p, m, v)."""
    b1, b2 = betas
    p, g, m, v = (_host(x) for x in (p, g, m, v))
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    return p - (lr / (1.0 - b1 ** t)) * m / denom, m, v


def _view_grad(xyz, g, campos, deg, coeffs, dtype):
    """([N,coeffs,3] basis x g, [N,coeffs,3] |basis| x |g|) of one view; rows whose g is all zero contribute nothing."""
    d = xyz.detach().to(dtype) - campos.to(dtype)
    b = sh_basis(deg, d / d.norm(dim=1, keepdim=True))
    k = min(b.shape[1], coeffs)
    full = torch.zeros(xyz.shape[0], coeffs, dtype=dtype, device=xyz.device)
    full[:, :k] = b[:, :k]
    seen = (g != 0).any(dim=1)[:, None, None]
    zero = torch.zeros((), dtype=dtype, device=xyz.device)
    return (torch.where(seen, full[:, :, None] * g[:, None, :], zero),
            torch.where(seen, full.abs()[:, :, None] * g.abs()[:, None, :], zero))


def _sh_grad_from_record(xyz, record, n, deg, coeffs=16):
    """[N,coeffs,3] = basis(normalize(xyz - campos)) x g, float64."""
    return _view_grad(xyz, record[:3 * n].view(n, 3).double(), record[3 * n:3 * n + 3], deg, coeffs, torch.float64)[0]


def factored_grad(xyz, records, n_views, view_stride, campos_stride, deg, M, grad_scale, dtype=torch.float64, magnitude=False):
    """[N,M,3] SH gradient the factored step applies: grad_scale * sum over the views, in view order, of
    basis_k(dir_view) * g_view.  View r has its [N,3] colour gradient at records[r * view_stride] and its camera centre at
    records[3 N + r * campos_stride].  `magnitude`: also return G = grad_scale * sum |basis_k| |g_view|."""
    xyz, rec = _host(xyz, torch.float32), _host(records, torch.float32).reshape(-1)
    n = xyz.shape[0]
    total = torch.zeros(n, M, 3, dtype=dtype)
    mag = torch.zeros(n, M, 3, dtype=dtype)
    for r in range(n_views):
        g = rec[r * view_stride:r * view_stride + 3 * n].view(n, 3).to(dtype)
        campos = rec[3 * n + r * campos_stride:3 * n + r * campos_stride + 3]
        a, b = _view_grad(xyz, g, campos, deg, M, dtype)
        total, mag = total + a, mag + b
    total, mag = total * grad_scale, mag * grad_scale
    return (total, mag) if magnitude else total


def colour_cache(sh_new, xyz_next, campos_next, deg_next, dtype=torch.float64):
    """What gsr_adam_sh_factored_next caches for the next view, from coefficients sh_new [N,M,3]:
    rgb [N,3] = max(sum_k basis_k sh_k + 0.5, 0); bits [N], bit c set where the sum + 0.5 is below 0;
    J [N,9], J[3c + j] = sum_k d basis_k / d dir_j * sh[k][c] with the direction components independent (autograd through
    sh_basis on a normalised, detached direction).  Also t = sum + 0.5 and the two error scales."""
    sh = _host(sh_new, dtype)
    n, M = sh.shape[0], sh.shape[1]
    d = _host(xyz_next, dtype) - _host(campos_next, dtype).reshape(1, 3)
    d = (d / d.norm(dim=1, keepdim=True)).detach().requires_grad_(True)
    b = sh_basis(deg_next, d)[:, :M]
    K = b.shape[1]
    db = torch.zeros(n, K, 3, dtype=dtype)
    if b.requires_grad:
        for k in range(K):
            gk = torch.autograd.grad(b[:, k].sum(), d, retain_graph=True, allow_unused=True)[0]
            if gk is not None:
                db[:, k] = gk
    b = b.detach()
    s = torch.zeros(n, 3, dtype=dtype)
    s_abs = torch.zeros(n, 3, dtype=dtype)
    J = torch.zeros(n, 3, 3, dtype=dtype)
    J_abs = torch.zeros(n, 3, 3, dtype=dtype)
    for k in range(K):
        term = b[:, k, None] * sh[:, k]
        s, s_abs = s + term, s_abs + term.abs()
        jt = sh[:, k, :, None] * db[:, k, None, :]            # [N, c, j]
        J, J_abs = J + jt, J_abs + jt.abs()
    t = s + 0.5
    bits = ((t < 0).to(torch.int32) * torch.tensor([1, 2, 4], dtype=torch.int32)).sum(dim=1).to(torch.int32)
    return SimpleNamespace(rgb=t.clamp_min(0), bits=bits, J=J.reshape(n, 9), t=t, rgb_scale=s_abs + 0.5,
                           J_scale=J_abs.reshape(n, 9))


# ------------------------------------------------------------------------------------------------------ checkers
def check_step(old, new, g_ref, G, lr, t, betas, eps, keys=("m", "v", "p"), group=None, what=""):
    """One Adam step of the side under test: old = (p, m, v) before, new = (p, m, v) after (fp32, any shape), g_ref / G the
    float64 gradient and its magnitude, lr a number or a tensor that broadcasts.  Returns {key: scaled error}; asserts
    each against its bar."""
    b1, b2 = betas
    p0, m0, v0 = (_host(x) for x in old)
    p1, m1, v1 = (_host(x) for x in new)
    g_ref, G = _host(g_ref), _host(G)
    m_ref = m0 + (g_ref - m0) * (1.0 - b1)
    v_ref = b2 * v0 + (1.0 - b2) * g_ref * g_ref
    upd = (lr / (1.0 - b1 ** t)) * m1 / (v1.sqrt() * (1.0 / math.sqrt(1.0 - b2 ** t)) + eps)
    errs = {keys[0]: _scaled((m1 - m_ref).abs(), torch.maximum(m0.abs(), G) + FLT_MIN),
            keys[1]: _scaled((v1 - v_ref).abs(), v_ref + (1.0 - b2) * G * G + FLT_MIN),
            keys[2]: _scaled((p1 - (p0 - upd)).abs(), 2.0 ** -24 * p0.abs() + 2.0 ** -23 * upd.abs())}
    for q, e in errs.items():
        _note(group, q, e)
    for q, e in errs.items():
        assert e <= BARS[q], f"{what}: {q} is {e:.3e} of its scale, bar {BARS[q]:.3e} ({e / BARS[q]:.2f} x)"
    return errs


def check_dense(old, new, g, lr, t, betas, eps, group=None, what=""):
    return check_step(old, new, _host(g), _host(g).abs(), lr, t, betas, eps, ("m", "v", "p"), group, what)


def sh_pack(f_dc, f_rest):
    """[N,1,3] and [N,M-1,3] -> [N,M,3] on the host, fp32."""
    return torch.cat([_host(f_dc, torch.float32), _host(f_rest, torch.float32)], dim=1)


def check_factored(case, old, new, rows=slice(None), group=None, what=""):
    """Factored SH step of `case` (factored_case) on the Gaussians `rows`: old / new = (p, m, v), each [N,M,3]."""
    g_ref, G = factored_grad(case.xyz, case.records, case.views, case.stride, case.stride, case.deg, case.M,
                             case.grad_scale, magnitude=True)
    lr = torch.full((1, case.M, 1), case.lr_rest, dtype=torch.float64)
    lr[0, 0, 0] = case.lr_dc
    return check_step([x[rows] for x in old], [x[rows] for x in new], g_ref[rows], G[rows], lr, case.t, case.betas,
                      case.eps, ("m_sh", "v_sh", "p"), group, what)


def check_untouched(before, after, what=""):
    """Bit-identical, NaN patterns included."""
    a, b = (x.detach().cpu().contiguous().view(torch.int32) for x in (before, after))
    assert a.shape == b.shape, what
    bad = (a != b).reshape(-1).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {a.numel()} words changed, first at {int(bad[0])}"


SENTINEL = 0x7FC0BEEF          # a quiet NaN no kernel computes


def sentinel(n, device="cpu"):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def split_cache(cache, n_total):
    """f32[13 n_total] -> (rgb [n,3] f32, bits [n] int32, J [n,9] f32) views on the host."""
    c = cache.detach().cpu().contiguous()
    return (c[:3 * n_total].view(n_total, 3), c[3 * n_total:4 * n_total].view(torch.int32),
            c[4 * n_total:13 * n_total].view(n_total, 9))


def exact_clamp_bits(sh_new):
    """Clamp bits of Gaussians whose only non-zero coefficients are those of k = 0: every fp32 evaluation order gives
    t = fl(fl(Y00 * sh_0) + 0.5) there, so the bits are known exactly, the case t == 0 (not below 0: bit clear) included."""
    y00 = torch.tensor(0.28209479177387814, dtype=torch.float32)
    t = _host(sh_new, torch.float32)[:, 0] * y00 + 0.5
    return ((t < 0).to(torch.int32) * torch.tensor([1, 2, 4], dtype=torch.int32)).sum(dim=1).to(torch.int32)


def cache_errors(cache, sh_new, xyz_next, campos_next, deg_next, first=0, count=None):
    """({"rgb", "J"}: scaled error over the Gaussians of the range, the reference, the three sections of the cache)."""
    n = sh_new.shape[0]
    count = n - first if count is None else count
    ref = colour_cache(sh_new, xyz_next, campos_next, deg_next)
    rgb, bits, J = split_cache(cache, n)
    sel = slice(first, first + count)
    errs = {"rgb": _scaled((rgb[sel].double() - ref.rgb[sel]).abs(), ref.rgb_scale[sel]),
            "J": _scaled((J[sel].double() - ref.J[sel]).abs(), ref.J_scale[sel])}
    return errs, ref, (rgb, bits, J)


def check_cache(cache, sh_new, xyz_next, campos_next, deg_next, first=0, count=None, before=None, exact_rows=None,
                group=None, what=""):
    """The colour cache f32[13 n_total] against colour_cache(sh_new ...) on the Gaussians [first, first + count); outside
    them the cache must equal `before` bit for bit.  sh_new are the coefficients the side under test wrote.
    `exact_rows`: indices of Gaussians with only k = 0 coefficients (exact_clamp_bits): their bits are held to the exact
    fp32 value and they do not count towards the band."""
    n = sh_new.shape[0]
    count = n - first if count is None else count
    sel = slice(first, first + count)
    errs, ref, (rgb, bits, J) = cache_errors(cache, sh_new, xyz_next, campos_next, deg_next, first, count)
    for q, e in errs.items():
        _note(group, q, e)
    for q, e in errs.items():
        assert e <= BARS[q], f"{what}: {q} is {e:.3e} of its scale, bar {BARS[q]:.3e} ({e / BARS[q]:.2f} x)"
    in_band = ref.t.abs() <= BARS["rgb"] * ref.rgb_scale                      # [n,3]
    want = ref.bits.clone()
    if exact_rows is not None and len(exact_rows):
        assert not bool(_host(sh_new)[exact_rows, 1:].any()), f"{what}: the k = 0 Gaussians took other coefficients"
        in_band[exact_rows] = False
        want[exact_rows] = exact_clamp_bits(sh_new[exact_rows])
    got = bits[sel]
    assert int(((got < 0) | (got > 7)).sum()) == 0, f"{what}: clamp words with bits above 2"
    for c in range(3):
        differ = (((got >> c) & 1) != ((want[sel] >> c) & 1)) & ~in_band[sel, c]
        assert int(differ.sum()) == 0, f"{what}: clamp bit {c} wrong on Gaussians {(differ.nonzero().reshape(-1) + first).tolist()[:8]}"
    n_band = int(in_band[sel].sum())
    assert n_band <= 0.01 * 3 * count, f"{what}: {n_band} of {3 * count} clamp entries inside the rounding band"
    if n <= 257:
        assert n_band == 0, f"{what}: {n_band} clamp entries inside the rounding band of a small case"
    if before is not None:
        r0, b0, j0 = split_cache(before, n)
        for name, a, b in (("rgb", r0, rgb), ("clamp bits", b0.view(torch.float32), bits.view(torch.float32)), ("J", j0, J)):
            check_untouched(a[:first], b[:first], f"{what}: cached {name} below the range")
            check_untouched(a[first + count:], b[first + count:], f"{what}: cached {name} above the range")
    errs["band"] = n_band
    return errs


# ---------------------------------------------------------------------------------------- inputs of the cases
GUARD = 64
DEFAULT_BETAS = (0.9, 0.999)
SH_DEGREE_OF = {16: 3, 9: 2, 4: 1, 1: 0}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dense_case(n, seed, t=3, wide=False, lr=1e-3, betas=DEFAULT_BETAS, eps=1e-15, name=None):
    """Host fp32 p, g, m, v of `n` elements for the step that takes the count to `t`.  The moments come from min(t - 1, 3)
    float64 reference steps from zero, rounded to fp32, so that m and v belong together.  Every 7th gradient is zero, at
    another phase in each step: zero gradients meet zero and non-zero moments.  `wide`: gradients +-10^e, e in [-30, 15]
    (g^2 from zero over denormal to 1e30); else unit normals times 10^e, e in [-3, 1]."""
    gen = _gen(seed)

    def grad(phase):
        if wide:
            e = torch.randint(-30, 16, (n,), generator=gen).double()
            g = 10.0 ** e * (torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1)
        else:
            g = torch.randn(n, generator=gen).double() * 10.0 ** torch.randint(-3, 2, (n,), generator=gen).double()
        g[phase::7] = 0
        return g.float()

    p = torch.randn(n, generator=gen)
    m = torch.zeros(n, dtype=torch.float64)
    v = torch.zeros(n, dtype=torch.float64)
    for s in range(min(t - 1, 3)):
        _, m, v = dense_step(m, grad(s + 1), m, v, 0.0, s + 1, betas, eps)
    return SimpleNamespace(name=name or f"n{n}-t{t}{'-wide' if wide else ''}", n=n, p=p, g=grad(0), m=m.float(), v=v.float(),
                           lr=lr, t=t, betas=betas, eps=eps)


D1_N, D1_STARTS, D1_LENGTHS = 4133, (0, 1, 2, 3, 5), (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1027)
D2_SHAPES = ((0,), (1,), (2,), (3,), (4,), (5,), (255,), (256,), (257,), (1023,), (1025,), (1366, 3),
             (4 * 256 * 4096 + 4 * 256 * 3 + 3,))
D2_OTHER = ((5,), (257,), (1025,))                     # the group with betas (0.8, 0.99), eps 1e-8
D3_N, D3_STEPS = 1027, (1, 2, 1000, 30000)
D4_ROWS = (1, 5, 1366)


def _numel(shape):
    return int(math.prod(shape))


def d1_case():
    return dense_case(D1_N, 101, name="D1")


def d2_cases():
    return [dense_case(_numel(s), 200 + i, name=f"D2-{i}") for i, s in enumerate(D2_SHAPES)]


def d2_other_cases():
    return [dense_case(_numel(s), 250 + i, betas=(0.8, 0.99), eps=1e-8, name=f"D2-other-{i}") for i, s in enumerate(D2_OTHER)]


def d3_cases():
    return [dense_case(D3_N, 300 + i, t=t, wide=True, name=f"D3-t{t}") for i, t in enumerate(D3_STEPS)]


def d4_cases(rows):
    """Nine tensors of one step; the kept (rows, 3) parameter is the last: the second launch."""
    return [dense_case(s, 400 + 10 * rows + i, name=f"D4-{rows}-{i}") for i, s in enumerate((7, 64, 3, 1025, 5, 256, 33, 129, 3 * rows))]


def dense_bar_cases():
    out = [d1_case()] + d2_cases() + d2_other_cases() + d3_cases()
    for rows in D4_ROWS:
        out += d4_cases(rows)
    return out


def exact_zero_dc():
    """(a, b): fp32 values with fl(Y00 * a) + 0.5 == 0 exactly and fl(Y00 * b) + 0.5 the next value below 0."""
    y00 = torch.tensor(0.28209479177387814, dtype=torch.float32)
    a = torch.tensor(-0.5, dtype=torch.float32) / y00
    lo = torch.tensor(-4.0, dtype=torch.float32)
    hi = torch.tensor(0.0, dtype=torch.float32)
    for _ in range(8):                                  # walk to a value whose product rounds to -0.5 exactly
        if float(a * y00) == -0.5:
            break
        a = torch.nextafter(a, hi if float(a * y00) < -0.5 else lo)
    assert float(a * y00 + 0.5) == 0.0
    b = a.clone()
    while float(b * y00 + 0.5) >= 0.0:
        b = torch.nextafter(b, lo)
    return float(a), float(b)


def factored_case(N, M, views, deg, seed, lr_dc=0.0025, lr_rest=0.0025 / 20, dark=False, name=None):
    """Host inputs of one factored SH step: positions, `views` records of [N,3] colour gradient + camera centre (stride
    3 N + 4), coefficients ~ N(0, 0.3), moments from one float64 step from zero (t = 2).  Gaussians n % 5 == 0 have a zero
    gradient in every view, n % 5 == 1 in view n % views only.  `dark` (N >= 64): the last two Gaussians have only k = 0
    coefficients, zero moments and no gradient, so the step leaves them alone, and sit on the clamp: channel 0 gives
    sum + 0.5 == 0 exactly in fp32, channel 1 the next value below, channel 2 (and all of the last Gaussian) well below."""
    gen = _gen(seed)
    stride = 3 * N + 4
    xyz = torch.randn(N, 3, generator=gen) * 3
    rec = torch.zeros(views, stride)
    g = torch.randn(views, N, 3, generator=gen) * 1e-3
    idx = torch.arange(N)
    g[:, idx % 5 == 0] = 0
    for r in range(views):
        g[r, (idx % 5 == 1) & (idx % views == r)] = 0
    rec[:, :3 * N] = g.reshape(views, 3 * N)
    rec[:, 3 * N:3 * N + 3] = torch.randn(views, 3, generator=gen) * 0.3 + torch.tensor([0.0, 0.0, -6.0])
    p = torch.randn(N, M, 3, generator=gen) * 0.3
    g0 = torch.randn(N, M, 3, generator=gen) * 1e-3
    _, m, v = dense_step(p, g0, torch.zeros_like(p), torch.zeros_like(p), 0.0, 1, DEFAULT_BETAS, 1e-15)
    m, v = m.float(), v.float()
    exact_rows = []
    if dark and N >= 64:
        a, b = exact_zero_dc()
        exact_rows = [N - 2, N - 1]
        p[exact_rows] = 0
        p[N - 2, 0] = torch.tensor([a, b, -3.0])
        p[N - 1, 0] = torch.tensor([-2.5, b, a])
        m[exact_rows] = 0
        v[exact_rows] = 0
        rec[:, :3 * N].view(views, N, 3)[:, exact_rows] = 0
    return SimpleNamespace(name=name or f"N{N}-M{M}-views{views}-deg{deg}", N=N, M=M, views=views, deg=deg, stride=stride,
                           xyz=xyz, records=rec.reshape(-1).contiguous(), p=p, m=m, v=v, t=2, betas=DEFAULT_BETAS, eps=1e-15,
                           lr_dc=lr_dc, lr_rest=lr_rest, grad_scale=1.0 / views, exact_rows=exact_rows)


F1_SIZES = {16: (1, 63, 64, 65, 257), 9: (65, 257), 4: (65, 257)}
F_VIEWS = (1, 3, 16)
F2_N, F2_FIRSTS = 257, (0, 1, 2, 3, 64, 129)


def f2_counts(first):
    return sorted({1, 63, 64, 65, F2_N - first})


def f1_cases(M, N):
    return [factored_case(N, M, views, deg, 1000 * M + 10 * N + 3 * deg + views)
            for deg in range(SH_DEGREE_OF[M] + 1) for views in F_VIEWS]


def f2_case(M):
    return factored_case(F2_N, M, 3, SH_DEGREE_OF[M], 5000 + M, name=f"F2-M{M}")


def f4_case():
    return factored_case(65, 1, 3, 0, 6001, name="F4-M1")


C1_SIZES = (1, 64, 65, 257)


def degree_pairs(M):
    """(active degree of the step, degree of the next view): equal, or one more (the iteration the SH ramp steps up)."""
    D = SH_DEGREE_OF[M]
    return [(d, d) for d in range(D + 1)] + [(d, d + 1) for d in range(D)]


def cache_case(N, M, deg, deg_next, first=0, count=None):
    """A factored step with lr = 0.05 (colours of the coefficients before the update miss the rgb bar by orders of
    magnitude) and the next view: positions after their own update and another camera centre."""
    c = factored_case(N, M, 3, deg, 7000 + 100 * M + 10 * deg + deg_next + N, lr_dc=0.05, lr_rest=0.05, dark=True,
                      name=f"N{N}-M{M}-deg{deg}-next{deg_next}")
    gen = _gen(8000 + N + M)
    c.xyz_next = c.xyz + torch.randn(N, 3, generator=gen) * 1.6e-2
    c.campos_next = torch.randn(3, generator=gen) * 0.3 + torch.tensor([0.5, -0.4, -6.0])
    c.deg_next, c.first, c.count = deg_next, first, N - first if count is None else count
    return c


def c1_cases(M, N):
    return [cache_case(N, M, d, dn) for d, dn in degree_pairs(M)]


def c2_case(M):
    return cache_case(257, M, SH_DEGREE_OF[M], SH_DEGREE_OF[M], first=64, count=65)


def factored_bar_cases():
    out = [c for M, sizes in F1_SIZES.items() for N in sizes for c in f1_cases(M, N)]
    return out + [f2_case(M) for M in F1_SIZES] + [f4_case()]


def cache_bar_cases():
    return [c for M in F1_SIZES for N in C1_SIZES for c in c1_cases(M, N)] + [c2_case(M) for M in F1_SIZES]


# -------------------------------------------------------------------- the fp32 restatement the levels are measured on
def torch_adam_step(p, g, m, v, lr, t, betas, eps):
    """One step of fp32 torch.optim.Adam(foreach=False) on the host from the given state -> (p, m, v)."""
    q = torch.nn.Parameter(p.detach().clone().float())
    q.grad = g.detach().clone().float()
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.detach().clone().float(),
                    "exp_avg_sq": v.detach().clone().float()}
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


def torch_factored_step(case):
    """fp32 restatement of the factored step of `case` -> (p, m, v), each [N,M,3]: gradient sum in plain fp32 torch, then
    torch.optim.Adam on the two tensors."""
    g = factored_grad(case.xyz, case.records, case.views, case.stride, case.stride, case.deg, case.M, case.grad_scale,
                      dtype=torch.float32)
    parts = []
    for sl, lr in ((slice(0, 1), case.lr_dc), (slice(1, None), case.lr_rest)):
        if case.M == 1 and sl.start == 1:
            continue
        parts.append(torch_adam_step(case.p[:, sl].contiguous(), g[:, sl].contiguous(), case.m[:, sl].contiguous(),
                                     case.v[:, sl].contiguous(), lr, case.t, case.betas, case.eps))
    return tuple(torch.cat([q[i] for q in parts], dim=1) for i in range(3))


def pack_cache(col, n_total=None, into=None, first=0, count=None):
    """A colour_cache result as the f32[13 n] layout of the kernel (rows [first, first + count) written into `into`)."""
    n = col.rgb.shape[0]
    count = n - first if count is None else count
    out = sentinel(13 * n) if into is None else into.clone()
    rgb, bits, J = (out[:3 * n].view(n, 3), out[3 * n:4 * n].view(torch.int32), out[4 * n:].view(n, 9))
    sel = slice(first, first + count)
    rgb[sel], bits[sel], J[sel] = col.rgb[sel].float(), col.bits[sel], col.J[sel].float()
    return out
