"""Shared cases, twins and bar arithmetic for tests/test_objective_cpu.py and tests/test_gpu_objective_parity.py: the photometric
loss (csrc/loss.hip) and the surface regularizers (csrc/regularizer.hip) pixel by pixel.

One chain, three arithmetics.  loss_forward / loss_backward / reg_chain are written once, in the order of the kernel text, and run
  * on fp64 tensors: the truth (the "fp64 twin"),
  * on fp32 tensors: the kernel's own formulation on the CPU (the "fp32 twin": the proof that a bar can be reached),
  * on E objects: the fp64 value together with a first-order bound of what fp32 rounding can do to it (the "bar").
E charges U32 * |result| for every rounding the kernel text has (U32 = 2^-24, the unit roundoff of fp32) and carries the bars of
the operands through the absolute partial derivatives of the operation: d(a b) = |a| db + |b| da, d(a / b) = (da + |a/b| db) / |b|,
d(sqrt a) = da / (2 sqrt a).  A contracted multiply-add rounds once instead of twice, so the separate count also bounds it.
The bars that the tests use are 2 * E.b (the fixed factor 2 covers the second order) + TINY32.  No constant here is fitted.

The photometric loss: what is counted, from the kernel text of loss_fwd_kernel / loss_bwd_kernel
  * the window.  The truth filters with the reference's 11x11 window, the fp32-rounded outer product of the fp32 1-D window
    (oracle/loss_ref.py); the kernel filters separably with its own 1-D window (make_window: fp32 sum in index order).  The two
    differ by Window.k roundings per tap at the most, measured on the two windows themselves (4 where this was written).
  * a filtered plane: 11 taps horizontally and 11 vertically, each a sequential chain `acc += w * v` from 0: every term passes
    through 11 roundings per pass at the most, 22 + Window.k in all: (22 + k) * U32 * filter(|plane|), plus filter(plane's own bar).
  * the planes: x and y are exact, x^2 + y^2 is fmaf(x, x, y * y) (two roundings; E counts three), x y is one.
  * C1 and C2 are fp32 constants (one rounding each); the reciprocal of B1 B2 is v_rcp_f32 and a Newton step (<= 1 ulp = 2 U32).
  * a tile's sums: a thread adds 4 C values, the wave tree is 6 levels, the four waves are 2 more: every term passes through
    4 C + 8 roundings at the most: n * U32 * sum|term| plus the sum of the pixels' bars.
  * lambda and grad_scale arrive as fp32; the twins take the fp32 values, so the truth is the truth of what the kernel was given.

The regularizers: reg_chain is reg_fwd_kernel / reg_bwd_kernel in camera space with the nine fp32 numbers of camera_kinv.
Every intermediate carries the magnitudes of its terms (the cross products and the normalisation are where they matter).
A tile's sums: wave tree 6 levels + 2: 8 roundings.

The surface maps: maps_chain is maps_fwd_kernel / maps_bwd_kernel with the world-space rays and the rotation of
fused_surface_maps.camera_world_rays, for an arbitrary upstream gradient of the seven output planes (MAPS_CASES: every kind of
allmap at every size, on the rotated camera).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_ref

U32 = 2.0 ** -24
TINY32 = 2.0 ** -126          # below this fp32 is subnormal: no relative bound holds


# ------------------------------------------------------------------------------------------------ the bar arithmetic
class E:
    """fp64 value v and a first-order bound b >= 0 of the error an fp32 evaluation of the same expression can have."""
    __slots__ = ("v", "b")

    def __init__(self, v, b=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.b = torch.zeros_like(self.v) if b is None else b

    @staticmethod
    def of(a):
        return a if isinstance(a, E) else E(a)

    shape = property(lambda s: s.v.shape)

    def __getitem__(s, i):
        return E(s.v[i], s.b[i])

    def __neg__(s):
        return E(-s.v, s.b)

    def __add__(s, o):
        o = E.of(o); v = s.v + o.v
        return E(v, s.b + o.b + U32 * v.abs())

    def __sub__(s, o):
        o = E.of(o); v = s.v - o.v
        return E(v, s.b + o.b + U32 * v.abs())

    def __mul__(s, o):
        o = E.of(o); v = s.v * o.v
        return E(v, s.v.abs() * o.b + o.v.abs() * s.b + U32 * v.abs())

    def __truediv__(s, o):
        o = E.of(o); v = s.v / o.v
        return E(v, (s.b + v.abs() * o.b) / o.v.abs() + U32 * v.abs())

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(s, o):
        return E.of(o) - s

    def __rtruediv__(s, o):
        return E.of(o) / s


def val(a):
    return a.v if isinstance(a, E) else a


def bar(a):
    """The bar the tests hold a quantity to: twice the first-order bound, and fp32's underflow threshold."""
    return 2.0 * a.b + TINY32


def mode_of(a):
    return "bar" if isinstance(a, E) else ("f32" if a.dtype == torch.float32 else "f64")


def scalar(mode, c, exact=True):
    """A scalar of the chain.  exact: c is an fp32 number already; otherwise the kernel holds fl32(c): one rounding."""
    if mode == "bar":
        return E(c, None if exact else torch.as_tensor(U32 * abs(c), dtype=torch.float64))
    return torch.tensor(c, dtype=torch.float32 if mode == "f32" else torch.float64)


def lift(mode, t):
    return E(t.double()) if mode == "bar" else t


def mul2(a):                      # a multiplication by two is exact
    return E(2.0 * a.v, 2.0 * a.b) if isinstance(a, E) else 2.0 * a


def absval(a):
    return E(a.v.abs(), a.b) if isinstance(a, E) else a.abs()


def sqrt(a):
    if not isinstance(a, E):
        return torch.sqrt(a)
    v = torch.sqrt(a.v)
    return E(v, torch.where(v > 0, a.b / (2.0 * v.clamp_min(1e-300)), torch.sqrt(a.b)) + U32 * v)


def rcp(a, roundings):
    if not isinstance(a, E):
        return 1.0 / a
    v = 1.0 / a.v
    return E(v, a.b * v * v + roundings * U32 * v.abs())


def maxc(a, c):
    return E(a.v.clamp_min(c), a.b) if isinstance(a, E) else a.clamp_min(c)


def where(cond, a, b):
    if isinstance(a, E) or isinstance(b, E):
        a = a if isinstance(a, E) else E(torch.full_like(b.v, float(a)))
        b = b if isinstance(b, E) else E(torch.full_like(a.v, float(b)))
        return E(torch.where(cond, a.v, b.v), torch.where(cond, a.b, b.b))
    a = a if isinstance(a, torch.Tensor) else torch.full_like(b, float(a))
    b = b if isinstance(b, torch.Tensor) else torch.full_like(a, float(b))
    return torch.where(cond, a, b)


def _embed(t, H, W, fill):
    out = torch.full((H, W), fill, dtype=t.dtype)
    if H >= 3 and W >= 3:
        out[1:-1, 1:-1] = t
    return out


def embed(a, H, W, fill=0.0):
    """An array of the interior pixels [H-2,W-2] -> the whole image, `fill` on the border (exact there)."""
    return E(_embed(a.v, H, W, fill), _embed(a.b, H, W, 0.0)) if isinstance(a, E) else _embed(a, H, W, fill)


def _shift(t, dy, dx):
    H, W = t.shape
    return F.pad(t, (1, 1, 1, 1))[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def shift(a, dy, dx):
    """out[y, x] = a[y + dy, x + dx], zero outside (|dy|, |dx| <= 1)."""
    return E(_shift(a.v, dy, dx), _shift(a.b, dy, dx)) if isinstance(a, E) else _shift(a, dy, dx)


def _tiles(t, tile, g16, corner):
    if t.dim() == 3:
        t = t.sum(0)
    H, W = t.shape
    ty, tx = -(-H // tile), -(-W // tile)
    s = F.pad(t, (0, tx * tile - W, 0, ty * tile - H)).reshape(ty, tile, tx, tile).sum((1, 3))
    out = torch.zeros(g16, dtype=t.dtype)
    step = tile // 16
    if corner == "top_left":
        out[::step, ::step] = s
    else:                                                   # the mutation: the bottom-right cell the tile still covers
        iy = torch.clamp(torch.arange(ty) * step + step - 1, max=g16[0] - 1)
        ix = torch.clamp(torch.arange(tx) * step + step - 1, max=g16[1] - 1)
        out[iy[:, None], ix[None, :]] = s
    return out


def tile_slots(a, tile, roundings, corner="top_left"):
    """Sums over the channels and over tile x tile pixels, laid out in 16x16-cell slots [ceil(H/16), ceil(W/16)]: a tile's sums
    stand in its top-left cell, its other cells hold 0."""
    H, W = a.shape[-2:]
    g16 = (-(-H // 16), -(-W // 16))
    if isinstance(a, E):
        return E(_tiles(a.v, tile, g16, corner), _tiles(a.b, tile, g16, corner) + roundings * U32 * _tiles(a.v.abs(), tile, g16, corner))
    return _tiles(a, tile, g16, corner)


def num_slots(H, W):
    return -(-H // 16) * -(-W // 16)


def f32(c):
    """The fp32 number the C ABI hands to the kernel for a Python float."""
    return float(np.float32(c))


# ------------------------------------------------------------------------------------------------ photometric loss
class Window:
    """w1: the kernel's 1-D window (make_window: fp32 values, fp32 sum in index order, fp32 division).  w2: the reference's 2-D
    window in fp64 (fp32-rounded outer product).  k: how many roundings per tap the two differ by, measured on the windows."""

    def __init__(self, sigma=1.5):
        g = np.array([np.float32(math.exp(-float((i - 5) * (i - 5)) / (2.0 * sigma * sigma))) for i in range(11)], dtype=np.float32)
        s = np.float32(0.0)
        for v in g:
            s = np.float32(s + v)
        self.w1 = torch.from_numpy((g / s).astype(np.float32))
        self.w2 = loss_ref.gaussian_window(11, sigma, 1, torch.float64)[0, 0].contiguous()
        outer = self.w1.double()[:, None] * self.w1.double()[None, :]
        self.k = int(math.ceil(float(((outer - self.w2).abs() / self.w2).max()) / U32))


WINDOW = Window()


def _conv64(p, w2, pad):
    C = p.shape[0]
    pp = F.pad(p[None], (5, 5, 5, 5), mode="replicate" if pad == "replicate" else "constant")
    return F.conv2d(pp, w2.expand(C, 1, 11, 11), groups=C)[0]


def _sep32(p, w1):
    """The kernel's filter: horizontal pass, then vertical pass, zero padding, each a chain `acc += w[k] * v[k]` from 0."""
    H, W = p.shape[-2:]
    pp, acc = F.pad(p, (5, 5)), torch.zeros_like(p)
    for k in range(11):
        acc = acc + w1[k] * pp[..., k:k + W]
    pp, out = F.pad(acc, (0, 0, 5, 5)), torch.zeros_like(p)
    for k in range(11):
        out = out + w1[k] * pp[..., k:k + H, :]
    return out


def filt(a, win, pad="zero"):
    if isinstance(a, E):
        return E(_conv64(a.v, win.w2, pad), _conv64(a.b, win.w2, pad) + (22 + win.k) * U32 * _conv64(a.v.abs(), win.w2, pad))
    if a.dtype == torch.float32:
        return _sep32(a, win.w1)
    return _conv64(a, win.w2, pad)


def loss_forward(x, y, win=WINDOW, *, pad="zero", c2=0.03 ** 2, corner="top_left"):
    """loss_fwd_kernel on [C,H,W]: S, the three maps dS/dmu1, dS/dE[x^2], dS/dE[xy] with (mu1, E[x^2], E[xy]) as the independent
    variables, and the slots of the sums of S and of |x - y| (32x32 tiles in 16x16 cells)."""
    mode = mode_of(x)
    C = x.shape[0]
    ss, xy = x * x + y * y, x * y
    mu1, mu2, ess, e12 = (filt(p, win, pad) for p in (x, y, ss, xy))
    C1, C2 = scalar(mode, 0.01 ** 2, exact=False), scalar(mode, c2, exact=False)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s12 = e12 - mu12
    A1, A2 = mul2(mu12) + C1, mul2(s12) + C2
    B1, B2 = (mu1_sq + mu2_sq) + C1, ((ess - mu1_sq) - mu2_sq) + C2
    if mode != "f32":
        # B2 cancels 1.6 down to 9e-4 on a flat bright image: two fp64 evaluations in different associations differ by 2.6e-12
        # there.  The VALUE of the truth follows the reference's association (two second-moment planes), so that it is the
        # oracle's to the last digits; the BAR stays the one of the kernel's association above.
        ref = ((filt(x * x, win, pad) - mu1_sq) + (filt(y * y, win, pad) - mu2_sq)) + C2
        B2 = E(ref.v, B2.b) if mode == "bar" else ref
    inv = rcp(B1 * B2, 2)
    S = (A1 * A2) * inv
    m0 = (mul2(mu2) * (A2 - A1)) * inv - (mul2(mu1) * S) * ((B2 - B1) * inv)
    m1 = -(S * (B1 * inv))
    m2 = mul2(A1) * inv
    l1 = absval(x - y)
    n = 4 * C + 8
    return dict(S=S, maps=(m0, m1, m2), l1=l1, slots=(tile_slots(S, 32, n, corner), tile_slots(l1, 32, n, corner)))


def loss_backward(x, y, maps, lam, gs, win=WINDOW, *, pad="zero", sign0=0.0, xy_times="y"):
    """loss_bwd_kernel: dL/dx of gs * [(1 - lam) mean|x - y| + lam (1 - mean S)] from the forward's maps.  lam, gs: fp32 numbers."""
    mode = mode_of(x)
    C, H, W = x.shape
    g0, g1, g2 = (filt(m, win, pad) for m in maps)
    inv_n = scalar(mode, 1.0 / (C * H * W), exact=False)             # C H W is exact in fp32 at every size used
    lam_, gs_ = scalar(mode, lam), scalar(mode, gs)
    k_ssim = ((-lam_) * inv_n) * gs_
    k_l1 = ((1.0 - lam_) * inv_n) * gs_
    d = val(x) - val(y)                                              # its sign is exact in any precision
    sgn = torch.where(d == 0, torch.full_like(d, sign0), torch.sign(d))
    other = y if xy_times == "y" else x
    return k_ssim * ((g0 + mul2(x) * g1) + other * g2) + k_l1 * sgn


# cases: (C, H, W) -> the edge it reaches
LOSS_SHAPES = {(1, 1, 1): "single pixel", (3, 5, 7): "smaller than the window", (1, 32, 32): "one tile",
               (3, 33, 31): "one-pixel remainders, four tiles, odd 16-grid", (3, 37, 70): "2x3 tiles, 3x5 cells",
               (4, 70, 70): "nine tiles, 16 workgroups, even channel count"}
LOSS_CONTENTS = ("rand", "flat_same", "flat_off", "flat_noise", "zeros", "ramp", "step", "outside", "ulp")
LOSS_LAMBDAS = (0.2, 0.0, 1.0)
LOSS_GRAD_SCALES = (1.0, 3.0)
# every content at two shapes or more, every shape at two contents or more
LOSS_CASES = [("rand", (1, 1, 1)), ("rand", (3, 5, 7)), ("rand", (3, 33, 31)), ("rand", (4, 70, 70)),
              ("flat_same", (1, 32, 32)), ("flat_same", (3, 33, 31)), ("flat_off", (3, 5, 7)), ("flat_off", (3, 37, 70)),
              ("flat_noise", (1, 32, 32)), ("flat_noise", (4, 70, 70)), ("zeros", (1, 1, 1)), ("zeros", (3, 33, 31)),
              ("ramp", (3, 5, 7)), ("ramp", (3, 37, 70)), ("step", (3, 37, 70)), ("step", (4, 70, 70)),
              ("outside", (1, 32, 32)), ("outside", (3, 33, 31)), ("ulp", (3, 33, 31)), ("ulp", (3, 37, 70)), ("ulp", (1, 1, 1))]


@functools.lru_cache(maxsize=None)
def loss_inputs(content, shape):
    """-> (x, y) fp32 [C,H,W]."""
    C, H, W = shape
    g = torch.Generator().manual_seed(1000 * LOSS_CONTENTS.index(content) + 100 * C + H + W)
    if content == "rand":
        x = torch.rand(shape, generator=g)
        y = (x + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif content == "flat_same":
        x, y = torch.full(shape, 0.9), torch.full(shape, 0.9)
    elif content == "flat_off":
        x, y = torch.full(shape, 0.9), torch.full(shape, 0.88)
    elif content == "flat_noise":
        x = torch.full(shape, 0.9)
        y = 0.9 + 1e-3 * torch.randn(shape, generator=g)
    elif content == "zeros":
        x, y = torch.zeros(shape), torch.zeros(shape)
    elif content == "ramp":
        x = (torch.arange(W, dtype=torch.float32) / max(W - 1, 1)).expand(C, H, W).contiguous()
        y = (x + 0.02 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif content == "step":                                  # 0 -> 1 at column 32 (x) and at row 32 (y)
        x = (torch.arange(W) >= 32).float().expand(C, H, W).contiguous()
        y = (torch.arange(H) >= 32).float()[:, None].expand(C, H, W).contiguous()
    elif content == "outside":                               # the render is not clamped
        x = -0.1 + 1.6 * torch.rand(shape, generator=g)
        y = torch.rand(shape, generator=g)
    elif content == "ulp":                                   # x == y on the left half, y = x -+ 1 ulp on the right
        y = 0.05 + 0.9 * torch.rand(shape, generator=g)
        up = (torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2 == 0
        moved = torch.where(up, torch.nextafter(y, torch.tensor(2.0)), torch.nextafter(y, torch.tensor(-1.0)))
        x = torch.where(torch.arange(W) < (W + 1) // 2, y, moved)
    else:
        raise KeyError(content)
    return x.float().contiguous(), y.float().contiguous()


@functools.lru_cache(maxsize=None)
def loss_truth(content, shape):
    """-> (forward in E arithmetic, {(lam, gs): backward in E arithmetic from the forward's maps})."""
    x, y = (E(t.double()) for t in loss_inputs(content, shape))
    fwd = loss_forward(x, y)
    return fwd, {(lam, gs): loss_backward(x, y, fwd["maps"], f32(lam), gs) for lam in LOSS_LAMBDAS for gs in LOSS_GRAD_SCALES}


LOSS_MUTATIONS = {"replicate_padding": (dict(pad="replicate"), {}), "c2_not_squared": (dict(c2=0.03), {}),
                  "sigma_1_4": (dict(win=Window(1.4)), {}), "sign0_is_1": ({}, dict(sign0=1.0)),
                  "xy_map_times_x": ({}, dict(xy_times="x")), "sums_in_bottom_right_cell": (dict(corner="bottom_right"), {})}


def loss_mutant(content, shape, name, lam, gs):
    """fp64 twin of one wrong reading of the kernel -> (forward dict, dimg)."""
    fkw, bkw = LOSS_MUTATIONS[name]
    x, y = (t.double() for t in loss_inputs(content, shape))
    fwd = loss_forward(x, y, **fkw)
    bk = dict(bkw)
    if "win" in fkw:
        bk["win"] = fkw["win"]
    if "pad" in fkw:
        bk["pad"] = fkw["pad"]
    return fwd, loss_backward(x, y, fwd["maps"], f32(lam), gs, **bk)


# ------------------------------------------------------------------------------------------------ surface regularizers
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def reg_chain(am, kinv, r, ln, ld, gs, bars=False):
    """reg_fwd_kernel and reg_bwd_kernel on allmap [7,H,W] (fp32 or fp64; bars: fp64 in E arithmetic) with K^-1 = kinv [3,3]:
    the normal error per pixel, the 16x16 tile sums of it and of the distortion, and the seven channels of d_allmap for
    gs * (ln * mean error + ld * mean distortion).  r, ln, ld, gs: fp32 numbers.

    Pixels without a splat (alpha == 0).  D / A is 0 / 0 or D / 0 there: surf_depth takes 0 for it (NaN and +inf become 0, as
    torch.nan_to_num(v, 0, 0) does; -inf does not occur: depth is positive), and no gradient passes: channels 0 and 1 get exactly
    0.  A NaN or infinite median passes none either.  Every channel is finite, channel 6 is kd = ld * gs / (H W) at every pixel.
    Where |cross| <= 1e-12 the normal is cross * 1e12 and reg_bwd_kernel lets NO gradient through it (maps_bwd_kernel scales by
    1e12 there instead, as autograd of F.normalize does).  Short of a surface seen exactly edge-on (parallel differences), the
    cross product of a pixel vanishes only when one of its finite differences does, which -- the two rays differ -- needs both
    neighbours at depth 0, that is both to be holes, and those two are the only pixels that finite difference hands a gradient
    to.  It can be below 1e-12 without vanishing, though: on a surface closer than about 1e-6 W (the `micro` kind) every pixel is,
    and the difference reaches lit pixels there.  This twin follows reg_bwd_kernel: zero."""
    mode = "bar" if bars else mode_of(am)
    H, W = am.shape[-2:]
    D, A, M, Dist = am[0], am[1], am[5], am[6]
    ok_e, ok_m = torch.isfinite(D / A), torch.isfinite(M)
    Dc, Ac, Mc = where(ok_e, D, 0.0), where(ok_e, A, 1.0), where(ok_m, M, 0.0)
    L = lambda t: lift(mode, t)
    r_ = scalar(mode, r)
    sd = (1.0 - r_) * (L(Dc) / L(Ac)) + r_ * L(Mc)
    xs = L(torch.arange(W, dtype=am.dtype)[None, :].expand(H, W).contiguous())
    ys = L(torch.arange(H, dtype=am.dtype)[:, None].expand(H, W).contiguous())
    m = [[scalar(mode, float(kinv[i, j])) for j in range(3)] for i in range(3)]
    R = [(m[k][0] * xs + m[k][1] * ys) + m[k][2] for k in range(3)]
    up, dn, rt, lf, mid = (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None)), \
        (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(1, -1))
    dx = [sd[up] * R[k][up] - sd[dn] * R[k][dn] for k in range(3)]
    dy = [sd[rt] * R[k][rt] - sd[lf] * R[k][lf] for k in range(3)]
    c = _cross(dx, dy)
    ln_c = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    inv = rcp(maxc(ln_c, 1e-12), 1)
    alpha, N = L(A)[mid], [L(am[2 + k])[mid] for k in range(3)]
    dotp = (((N[0] * c[0] + N[1] * c[1]) + N[2] * c[2]) * inv) * alpha
    err = embed(1.0 - dotp, H, W, fill=1.0)
    sums = (tile_slots(err, 16, 8), tile_slots(L(Dist), 16, 8))
    # backward
    inv_n = scalar(mode, 1.0 / (W * H), exact=False)
    kn, kd = (scalar(mode, ln) * inv_n) * scalar(mode, gs), (scalar(mode, ld) * inv_n) * scalar(mode, gs)
    big = val(ln_c) > 1e-12
    il = rcp(where(big, ln_c, 1.0), 1)
    s = [c[k] * il for k in range(3)]
    g = [((-kn) * alpha) * N[k] for k in range(3)]
    sg = (s[0] * g[0] + s[1] * g[1]) + s[2] * g[2]
    gc = [(g[k] - s[k] * sg) * il for k in range(3)]
    gdx = [embed(where(big, v, 0.0), H, W) for v in _cross(dy, gc)]
    gdy = [embed(where(big, v, 0.0), H, W) for v in _cross(gc, dx)]
    gP = [((shift(gdx[k], -1, 0) - shift(gdx[k], 1, 0)) + shift(gdy[k], 0, -1)) - shift(gdy[k], 0, 1) for k in range(3)]
    g_sd = (gP[0] * R[0] + gP[1] * R[1]) + gP[2] * R[2]
    g_e = (1.0 - r_) * g_sd
    dam = [None] * 7
    dam[0] = where(ok_e, g_e / L(Ac), 0.0)
    dam[1] = where(ok_e, ((-g_e) * L(Dc)) / (L(Ac) * L(Ac)), 0.0)
    dam[5] = where(ok_m, r_ * g_sd, 0.0)
    dam[6] = kd * L(torch.ones(H, W, dtype=am.dtype))
    for k in range(3):
        dam[2 + k] = (-kn) * embed((c[k] * inv) * alpha, H, W)
    return dict(err=err, sums=sums, dam=dam)


REG_MUTATIONS = ("forward_differences", "border_normal_kept", "alpha_attached", "inf_kept", "ratio_exchanged", "half_pixel_rays")


def _surf64(a, m, r, mut=None, eps_passes=False):
    """surf_depth [H,W] and surf_normal * alpha [H,W,3] of allmap `a` (fp64, possibly an autograd leaf) with the rays m [x, y, 1],
    written for autograd with the guards of the contract of reg_chain, and one wrong reading of it per `mut`.  eps_passes: where
    |cross| <= 1e-12 the gradient passes through the scaling by 1e12 (F.normalize, maps_bwd_kernel) or not at all (reg_bwd_kernel)."""
    H, W = a.shape[-2:]
    D, A, M = a[0], a[1], a[5]
    q = (D / A).detach()
    ok_e = ~torch.isnan(q) if mut == "inf_kept" else torch.isfinite(q)
    ok_m = ~torch.isnan(M.detach()) if mut == "inf_kept" else torch.isfinite(M.detach())
    e = torch.where(ok_e, D / torch.where(ok_e, A, torch.ones_like(A)), torch.zeros_like(D))
    med = torch.where(ok_m, M, torch.zeros_like(M))
    r1, r2 = (r, 1.0 - r) if mut == "ratio_exchanged" else (1.0 - r, r)
    sd = r1 * e + r2 * med
    off = 0.5 if mut == "half_pixel_rays" else 0.0
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float64) + off, torch.arange(W, dtype=torch.float64) + off, indexing="ij")
    rays = torch.stack([gx, gy, torch.ones_like(gx)], -1) @ m.double().T
    P = sd[..., None] * rays
    if mut == "border_normal_kept":
        P = F.pad(P.permute(2, 0, 1)[None], (1, 1, 1, 1), mode="replicate")[0].permute(1, 2, 0)
    if mut == "forward_differences":
        dx, dy = P[2:, 1:-1] - P[1:-1, 1:-1], P[1:-1, 2:] - P[1:-1, 1:-1]
    else:
        dx, dy = P[2:, 1:-1] - P[:-2, 1:-1], P[1:-1, 2:] - P[1:-1, :-2]
    c = torch.cross(dx, dy, dim=-1)
    ln_c = c.norm(dim=-1, keepdim=True)
    n = c / ln_c.clamp_min(1e-12)
    if not eps_passes:
        n = torch.where(ln_c > 1e-12, n, n.detach())
    if mut == "border_normal_kept":
        sn = n
    else:
        sn = torch.zeros(H, W, 3, dtype=torch.float64)
        if H >= 3 and W >= 3:
            sn = F.pad(n.permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)
    if mut != "no_alpha":
        sn = sn * (A if mut == "alpha_attached" else A.detach())[..., None]
    return sd, sn


def reg_autograd64(am, kinv, r, ln, ld, gs, mut=None):
    """The same objective written for autograd in fp64 (the oracle's formulation in camera space, with the guards of the contract
    above), and one wrong reading of it per REG_MUTATIONS -> (err [H,W], (tile sums), d_allmap [7,H,W])."""
    a = am.double().clone().requires_grad_(True)
    _, sn = _surf64(a, kinv, r, mut)
    err = 1.0 - (a[2:5].permute(1, 2, 0) * sn).sum(-1)
    (gs * (ln * err.mean() + ld * a[6].mean())).backward()
    err = err.detach()
    return err, (tile_slots(err, 16, 8), tile_slots(a[6].detach(), 16, 8)), a.grad


REG_SIZES = {(2, 7): "no interior pixel", (3, 3): "one interior pixel", (16, 16): "one tile", (17, 33): "tile straddling",
             (31, 18): "tile straddling", (48, 40): "nine tiles"}
REG_NOISE_KINDS = ("full", "holes", "island", "one_hole", "plane", "nonfinite")
# structured depth, what every real render has: the cross product of the two finite differences has to cancel
REG_SURFACE_KINDS = ("sphere", "far", "micro", "grazing", "step")
REG_KINDS = REG_NOISE_KINDS + REG_SURFACE_KINDS
REG_RATIOS = (0.0, 0.3, 1.0)
REG_LAMBDAS = ((0.05, 100.0), (1.0, 0.0), (0.0, 1.0))
REG_GRAD_SCALE = 2.5


def _reg_rotation(i, j):
    return REG_RATIOS[(i + j) % 3], REG_LAMBDAS[(i + 2 * j + (i // 3)) % 3]


# every kind at every size; the ratio and the lambdas rotate so that each kind and each size meets every one of them.  The
# structured kinds are appended: the cases of the noise kinds keep their places, ratios and lambdas
REG_CASES = [(kind, size) + _reg_rotation(i, j) for i, size in enumerate(REG_SIZES) for j, kind in enumerate(REG_NOISE_KINDS)] + \
            [(kind, size) + _reg_rotation(i, len(REG_NOISE_KINDS) + j) for i, size in enumerate(REG_SIZES)
             for j, kind in enumerate(REG_SURFACE_KINDS)]


def reg_case_id(case):
    kind, (H, W), r, (ln, ld) = case
    return f"{kind}-{H}x{W}-r{r}-ln{ln}-ld{ld}"


@functools.lru_cache(maxsize=None)
def reg_camera(size, rotated=False):
    from gaussmart_amd.synthetic import jittered_cameras
    H, W = size
    return jittered_cameras(2, W, H, seed=H + W, amount=0.4)[1 if rotated else 0]


def reg_camera_f64(size, rotated=False, centred=False):
    """-> (world_view_transform, full_proj_transform) in fp64 from the camera's fp64 R and T.  The camera's own fp32 matrices are
    orthogonal to 4e-8 only, and the rotation drops out of the normal error no better than that.  centred: the same rotation and
    intrinsics with the camera centre at the world origin."""
    cam = reg_camera(size, rotated)
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3] = torch.as_tensor(cam.R, dtype=torch.float64).T
    if not centred:
        w2c[:3, 3] = torch.as_tensor(cam.T, dtype=torch.float64)
    wvt = w2c.T.contiguous()
    return wvt, wvt @ cam.projection_matrix.double().cpu()


def reg_kinv(size, rotated=False, dtype=torch.float32):
    """The nine numbers of fused_regularizer.camera_kinv as a [3,3] tensor (float32: through camera_kinv itself; float64: the same
    derivation in fp64, what the oracle works with)."""
    cam = reg_camera(size, rotated)
    if dtype == torch.float32:
        from gaussmart_amd.fused_regularizer import camera_kinv
        return torch.tensor(list(camera_kinv(cam)), dtype=torch.float32).reshape(3, 3)
    H, W = size
    wvt, full = reg_camera_f64(size, rotated)
    c2w = wvt.T.inverse()
    ndc2pix = torch.tensor([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], dtype=torch.float64).T
    return ((c2w.T @ full) @ ndc2pix)[:3, :3].T.inverse()


def _surface_depth(kind, size, g):
    """The z-depth [H,W] (fp64) of a surface seen through the camera-space rays of reg_kinv(size) (z = 1), and where it is hit.
      sphere   centre (0, 0, 6), radius 2: a silhouette, holes around it
      far      the plane of `plane` through (0, 0, 3000)
      micro    the same plane through (0, 0, 1.5e-6): every cross product is below F.normalize's eps, 1e-12.  The rays of two
               neighbours differ by about 1.15 / W (60 degrees across the width), so below W = 16 the plane comes closer by W / 16
      grazing  a plane through (0, 0, 6) whose normal is 85 degrees from the view axis; holes where the ray misses it or the depth
               exceeds 1e6
      step     depth 2 on the left half, 9 on the right, plus 0.01 * noise"""
    H, W = size
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    rays = torch.stack([gx, gy, torch.ones_like(gx)], -1) @ reg_kinv(size).double().T
    if kind == "sphere":
        centre, radius = torch.tensor([0.0, 0.0, 6.0], dtype=torch.float64), 2.0
        b, a = rays @ centre, (rays * rays).sum(-1)
        disc = b * b - a * (centre @ centre - radius * radius)
        return (b - torch.sqrt(disc.clamp_min(0.0))) / a, disc > 0
    if kind == "step":
        left = (torch.arange(W) < W // 2)[None, :].expand(H, W)
        depth = torch.where(left, 2.0, 9.0).double() + 0.01 * torch.rand(H, W, generator=g).double()
        return depth, torch.ones(H, W, dtype=torch.bool)
    n = torch.tensor([0.0, -1.0, -0.0875] if kind == "grazing" else [0.3, -0.2, -1.0], dtype=torch.float64)
    n = n / n.norm()
    z0 = {"far": 3000.0, "micro": 1.5e-6 * min(1.0, W / 16.0), "grazing": 6.0}[kind]
    depth = (n[2] * z0) / (rays @ n)
    return depth, (depth > 0) & (depth < 1e6)


@functools.lru_cache(maxsize=None)
def reg_allmap(kind, size):
    """-> allmap fp32 [7,H,W]: alpha * depth, alpha, alpha * normal, median depth, distortion (as tests/test_gpu_surface_maps.py).
    alpha is 0 or in [0.05, 1]: D / A is finite in fp32 wherever it is in fp64.  REG_NOISE_KINDS draw the depth per pixel (but
    `plane`); REG_SURFACE_KINDS (_surface_depth) are surfaces, with a random rendered normal and a median within 2 % of the depth."""
    H, W = size
    g = torch.Generator().manual_seed(100 * REG_KINDS.index(kind) + 7 * H + W)
    alpha = 0.05 + 0.95 * torch.rand(1, H, W, generator=g)
    depth = 0.5 + 19.5 * torch.rand(1, H, W, generator=g)
    cy, cx = H // 2, W // 2
    if kind in ("holes", "nonfinite"):
        alpha = torch.where(torch.rand(1, H, W, generator=g) < 0.3, torch.zeros_like(alpha), alpha)
    elif kind == "island":
        lit = torch.zeros(1, H, W, dtype=torch.bool)
        lit[0, cy, cx] = True
        alpha = torch.where(lit, alpha, torch.zeros_like(alpha))
    elif kind == "one_hole":
        alpha[0, cy, cx] = 0.0
    if kind in REG_SURFACE_KINDS:
        depth, lit = _surface_depth(kind, size, g)
        alpha = torch.where(lit[None], alpha, torch.zeros_like(alpha))
        depth = torch.where(lit, depth, torch.zeros_like(depth))[None].float()
    nrm = torch.randn(3, H, W, generator=g) * alpha
    if kind == "plane":                                     # the rendered normal IS the surface normal: error ~ 0, 1 - dot cancels
        kinv = reg_kinv(size).double()
        gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        rays = torch.stack([gx, gy, torch.ones_like(gx)], -1) @ kinv.T
        n = torch.tensor([0.3, -0.2, -1.0], dtype=torch.float64)
        n = n / n.norm()
        depth = ((n[2] * 6.0) / (rays @ n))[None].float()    # the plane through (0, 0, 6); rays have z = 1, so this is the z-depth
        alpha = torch.ones(1, H, W)
        nrm = n.float()[:, None, None].expand(3, H, W)
    spread = 0.04 if kind in REG_SURFACE_KINDS else 0.4      # the structured kinds stay surfaces at every depth ratio
    med = torch.where(alpha > 0, depth * ((1.0 - spread / 2) + spread * torch.rand(1, H, W, generator=g)), torch.zeros_like(depth))
    if kind == "plane":
        med = depth
    am = torch.cat([alpha * depth, alpha, nrm, med, alpha * torch.rand(1, H, W, generator=g)]).float().contiguous()
    if kind == "nonfinite":
        flat = torch.randperm(H * W, generator=g)[:min(9, H * W)]
        ys, xs = flat // W, flat % W
        for i, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
            if i % 3 == 0:                                   # A = 0 with D > 0: D / A = +inf
                am[:, y, x] = 0.0
                am[0, y, x] = 1.5
            elif i % 3 == 1:
                am[5, y, x] = float("nan")
            else:
                am[5, y, x] = float("inf")
    return am


@functools.lru_cache(maxsize=None)
def reg_truth(case):
    kind, size, r, (ln, ld) = case
    return reg_chain(reg_allmap(kind, size).double(), reg_kinv(size).double(), f32(r), f32(ln), f32(ld), REG_GRAD_SCALE, bars=True)


# ------------------------------------------------------------------------------------------------ surface maps
def maps_chain(am, rays9, rot9, r, gout, bars=False):
    """maps_fwd_kernel and maps_bwd_kernel on allmap [7,H,W] (fp32 or fp64; bars: fp64 in E arithmetic) with the world-space rays
    rays9 [3,3] = c2w[:3,:3] K^-1 and the rotation rot9 [3,3] = world_view_transform[:3,:3], the numbers of
    fused_surface_maps.camera_world_rays: the seven output planes (rend_normal, surf_depth, surf_normal * alpha) and, for the
    upstream gradient gout [7,H,W], the seven channels of d_allmap.  `len` is |cross| at the interior pixels.

    What differs from reg_chain: the rays carry the rotation; out[0:3] = rot . n and d_allmap[2:5] = rot^T . gout[0:3], three
    products and two additions each; the gradient of surf_normal is whatever arrives, times alpha (detached); surf_depth has a
    gradient of its own; d_allmap[6] = 0; and where |cross| <= 1e-12 the normal is cross * 1e12 with the gradient gout * 1e12, as
    autograd of F.normalize has it.  1e-12 and 1e12 are fp32 constants there: one rounding each, which shows only in that regime.
    The contract at pixels without a splat is reg_chain's: finite everywhere, channels 0 and 1 exactly 0."""
    mode = "bar" if bars else mode_of(am)
    H, W = am.shape[-2:]
    D, A, M = am[0], am[1], am[5]
    ok_e, ok_m = torch.isfinite(D / A), torch.isfinite(M)
    Dc, Ac, Mc = where(ok_e, D, 0.0), where(ok_e, A, 1.0), where(ok_m, M, 0.0)
    L = lambda t: lift(mode, t)
    r_ = scalar(mode, r)
    sd = (1.0 - r_) * (L(Dc) / L(Ac)) + r_ * L(Mc)
    xs = L(torch.arange(W, dtype=am.dtype)[None, :].expand(H, W).contiguous())
    ys = L(torch.arange(H, dtype=am.dtype)[:, None].expand(H, W).contiguous())
    m = [[scalar(mode, float(rays9[i, j])) for j in range(3)] for i in range(3)]
    rot = [[scalar(mode, float(rot9[i, j])) for j in range(3)] for i in range(3)]
    R = [(m[k][0] * xs + m[k][1] * ys) + m[k][2] for k in range(3)]
    up, dn, rt, lf, mid = (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None)), \
        (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(1, -1))
    dx = [sd[up] * R[k][up] - sd[dn] * R[k][dn] for k in range(3)]
    dy = [sd[rt] * R[k][rt] - sd[lf] * R[k][lf] for k in range(3)]
    c = _cross(dx, dy)
    ln_c = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    big = val(ln_c) > 1e-12
    inv = rcp(where(big, ln_c, scalar(mode, 1e-12, exact=False)), 1)
    alpha, N = L(A)[mid], [L(am[2 + k]) for k in range(3)]
    out = [(rot[j][0] * N[0] + rot[j][1] * N[1]) + rot[j][2] * N[2] for j in range(3)] + [sd] + \
          [embed((c[k] * inv) * alpha, H, W) for k in range(3)]
    # backward
    G = [L(gout[k]) for k in range(4)]
    g = [L(gout[4 + k][mid]) * alpha for k in range(3)]
    il = rcp(where(big, ln_c, 1.0), 1)
    s = [c[k] * il for k in range(3)]
    sg = (s[0] * g[0] + s[1] * g[1]) + s[2] * g[2]
    e12 = scalar(mode, 1e12, exact=False)
    gc = [where(big, (g[k] - s[k] * sg) * il, g[k] * e12) for k in range(3)]
    gdx = [embed(v, H, W) for v in _cross(dy, gc)]
    gdy = [embed(v, H, W) for v in _cross(gc, dx)]
    gP = [((shift(gdx[k], -1, 0) - shift(gdx[k], 1, 0)) + shift(gdy[k], 0, -1)) - shift(gdy[k], 0, 1) for k in range(3)]
    g_sd = ((gP[0] * R[0] + gP[1] * R[1]) + gP[2] * R[2]) + G[3]
    g_e = (1.0 - r_) * g_sd
    dam = [None] * 7
    dam[0] = where(ok_e, g_e / L(Ac), 0.0)
    dam[1] = where(ok_e, ((-g_e) * L(Dc)) / (L(Ac) * L(Ac)), 0.0)
    dam[5] = where(ok_m, r_ * g_sd, 0.0)
    dam[6] = L(torch.zeros(H, W, dtype=am.dtype))
    for k in range(3):
        dam[2 + k] = (rot[0][k] * G[0] + rot[1][k] * G[1]) + rot[2][k] * G[2]
    return dict(out=out, dam=dam, len=ln_c)


MAPS_MUTATIONS = ("camera_space_rays", "rotation_not_transposed_back", "rotation_transposed_forward", "alpha_attached", "no_alpha",
                  "eps_passes_nothing", "depth_gradient_dropped", "forward_differences", "border_normal_kept", "ratio_exchanged",
                  "inf_kept", "half_pixel_rays", "dist_gradient_not_zero")


def maps_autograd64(am, rays9, rot9, r, gout, mut=None):
    """The same maps written for autograd in fp64 (the oracle's formulation on the rays the kernel was given, with the guards of
    the contract), and one wrong reading of the kernels per MAPS_MUTATIONS -> (out [7,H,W], d_allmap [7,H,W] of sum(out * gout))."""
    a = am.double().clone().requires_grad_(True)
    rays, rot, go = rays9.double(), rot9.double(), gout.double()
    if mut == "camera_space_rays":
        rays = rot.T @ rays
    sd, sn = _surf64(a, rays, r, mut, eps_passes=mut != "eps_passes_nothing")
    rn = torch.einsum("ij,jhw->ihw" if mut != "rotation_transposed_forward" else "ji,jhw->ihw", rot, a[2:5])
    out = torch.cat([rn, sd[None], sn.permute(2, 0, 1)])
    seen = go.clone()
    if mut == "depth_gradient_dropped":
        seen[3] = 0.0
    (out * seen).sum().backward()
    grad = a.grad.clone()
    if mut == "rotation_not_transposed_back":
        grad[2:5] = torch.einsum("ij,jhw->ihw", rot, go[0:3])
    if mut == "dist_gradient_not_zero":                      # reg_bwd_kernel's channel 6 with unit weights
        grad[6] = 1.0 / (am.shape[-2] * am.shape[-1])
    return out.detach(), grad


MAPS_SIZES = dict(REG_SIZES)
MAPS_SIZES.update({(1, 1): "a single pixel", (80, 112): "35 tiles: not a multiple of the eight tile bands, idle workgroups, a ragged last band"})
# the sizes at which a kind's upstream gradient is a single interior pixel (one size per kind, in turn)
_DELTA_SIZES = [size for size in MAPS_SIZES if min(size) >= 3]
# every kind at every size on the rotated camera; the depth ratio rotates as in REG_CASES
MAPS_CASES = [(kind, size, REG_RATIOS[(i + j) % 3], "delta" if size == _DELTA_SIZES[j % len(_DELTA_SIZES)] else "randn")
              for i, size in enumerate(MAPS_SIZES) for j, kind in enumerate(REG_KINDS)]


def maps_case_id(case):
    kind, (H, W), r, pattern = case
    return f"{kind}-{H}x{W}-r{r}-{pattern}"


def maps_rays(size, dtype=torch.float32):
    """-> (rays9, rot9) as [3,3] tensors for the rotated camera.  float32: the numbers fused_surface_maps.camera_world_rays hands
    to the kernels; float64: the same derivation from the camera's fp64 matrices, what the oracle works with."""
    if dtype == torch.float32:
        from gaussmart_amd.fused_surface_maps import camera_world_rays
        rays, rot = camera_world_rays(reg_camera(size, rotated=True))
        return tuple(torch.tensor(list(v), dtype=torch.float32).reshape(3, 3) for v in (rays, rot))
    wvt, _ = reg_camera_f64(size, rotated=True)
    return wvt.T.inverse()[:3, :3] @ reg_kinv(size, rotated=True, dtype=torch.float64), wvt[:3, :3].clone()


@functools.lru_cache(maxsize=None)
def maps_gout(case):
    """-> the upstream gradient of the seven output planes, fp32 [7,H,W].  randn: every pixel; delta: zero but at one interior
    pixel (lit, and on a 16x16 tile's edge where there is one), so that a gradient landing on the wrong neighbour cannot hide."""
    kind, (H, W), r, pattern = case
    g = torch.Generator().manual_seed(5000 + 100 * REG_KINDS.index(kind) + 7 * H + W)
    gout = torch.randn(7, H, W, generator=g)
    if pattern == "delta":
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        inner = (ys >= 1) & (ys <= H - 2) & (xs >= 1) & (xs <= W - 2)
        edge = ((ys % 16 == 0) | (ys % 16 == 15) | (xs % 16 == 0) | (xs % 16 == 15))
        lit = reg_allmap(kind, (H, W))[1] > 0
        for cand in (inner & lit & edge, inner & lit, inner):
            if bool(cand.any()):
                break
        at = cand.nonzero()[int(torch.randint(int(cand.sum()), (1,), generator=g))]
        keep = torch.zeros(H, W, dtype=torch.bool)
        keep[at[0], at[1]] = True
        gout = torch.where(keep, gout, torch.zeros_like(gout))
    return gout.contiguous()


@functools.lru_cache(maxsize=None)
def maps_truth(case):
    kind, size, r, _ = case
    rays9, rot9 = maps_rays(size)
    return maps_chain(reg_allmap(kind, size).double(), rays9.double(), rot9.double(), f32(r), maps_gout(case).double(), bars=True)


# ------------------------------------------------------------------------------------------------ objective finish
FINISH_N = (1, 255, 256, 257, 2048, 2049, 4100)


def finish_truth(pl, pr, C, H, W, lam, ln, ld):
    """objective_finish_body on fp32 partial pairs pl [n,2] (SSIM, L1) and pr [n,2] or None (normal error, distortion): the five
    scalars in E arithmetic.  A thread adds ceil(n / 256) values one after the other, the tree is 8 levels: every partial passes
    through n / 256 + 8 roundings at the most, and the product with 1 / (C H W) is the ninth."""
    n = pl.shape[0]

    def total(col):
        v = col.double()
        return E(v.sum(), (n / 256 + 8) * U32 * v.abs().sum())

    zero = E(torch.zeros((), dtype=torch.float64))
    inv_img, inv_pix = scalar("bar", 1.0 / (C * H * W), exact=False), scalar("bar", 1.0 / (H * W), exact=False)
    ssim, l1 = total(pl[:, 0]) * inv_img, total(pl[:, 1]) * inv_img
    nrm, dst = (total(pr[:, 0]) * inv_pix, total(pr[:, 1]) * inv_pix) if pr is not None else (zero * inv_pix, zero * inv_pix)
    lam_ = scalar("bar", f32(lam))
    ln_, ld_ = (scalar("bar", f32(ln)), scalar("bar", f32(ld))) if pr is not None else (zero, zero)
    tot = (((1.0 - lam_) * l1 + lam_ * (1.0 - ssim)) + ln_ * nrm) + ld_ * dst
    return [tot, l1, ssim, nrm, dst]


def finish_partials(n, with_reg):
    g = torch.Generator().manual_seed(n)
    pl = torch.randn(n, 2, generator=g) * 200.0
    pr = torch.randn(n, 2, generator=g) * 50.0 if with_reg else None
    return pl, pr


def ratio(err, b):
    """max err / bar, with 0 / 0 = 0 and anything not finite = inf."""
    q = torch.where(err == 0, torch.zeros_like(err), err / b)
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))
    return float(q.max()) if q.numel() else 0.0
