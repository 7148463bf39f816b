"""Shared cases, chains and mutations for tests/test_pergaussian_cpu.py and tests/test_gpu_pergaussian_parity.py: the per-Gaussian
kernels -- preprocess_fwd.hip (K1 geometry and the SH colour passes), the colour cache of adam.hip and the per-Gaussian half of
preprocess_bwd.hip (K8) -- Gaussian by Gaussian and field by field.

One chain, three arithmetics, exactly as tests/objective_cases.py (whose E, bar and helpers are imported, not copied): every chain
is written once in the order of the kernel text and run on fp64 tensors (the truth), on fp32 tensors (the fp32 twin: the proof
that a bar can be reached) and on E objects (the fp64 value with a first-order bound of what fp32 rounding can do to it).  The
only bar is 2 * E.b + TINY32.  No constant here is fitted.

What is counted, from the kernel text
  * preprocess_one (K1 geometry): every product and every sum of the view transform, of the quaternion's rotation, of the three
    rows through `proj` and of the (W-1)/2 pixel convention is one rounding (a contracted multiply-add rounds once, so the
    separate count bounds it); rsqrtf, expf and a division are charged one ulp (2 U32: the documented bound of the device's
    functions; a correctly rounded division is within it).  The centre is the cancelling quotient sum f_i Tu_i Tw_i with
    f = t / d: E carries |f_i Tu_i Tw_i| and the bar of d through it, so the bar of (cx, cy) grows with the conditioning of each
    Gaussian and is not a figure relative to a column's maximum.  The constants 0.2f (near plane), 0.707106f and 1e-4f are the
    kernel's fp32 literals.  A discrete result (visibility, radius, tile rect) is compared only where the fp64 margin of the
    quantity that decides it exceeds that quantity's bar: `decisions` lists them, `excused` marks the others.
  * color_chain (every colour producer): direction o / |o| (three roundings for |o|^2, one sqrt, one ulp for the reciprocal), the
    sixteen written polynomials, their sum over k < min(M, (deg+1)^2), + 0.5 and the clamp.  The producers add the same terms in
    different orders (nested sequential in sh_to_rgb, a four-level DPP tree in the 16-lane kernel, a chain of fmaf in the colour
    cache), so the sum is charged order-independently: n_active roundings on the sum of the terms' magnitudes.  J[c][a] is the
    derivative of the written polynomials with the direction components independent, summed the same way.
  * term_chain (the view-direction term of dL/dmean): dd = sum_c g_c J[c][:] (the unfactored kernel forms the same double sum
    in the other order: the same magnitudes), dotp = d . dd, (dd - d dotp) / |o|.
  * bwd_chain (step 3b of preprocess_bwd_kernel): the matrix M3 = proj @ ndc2pix per row, dT -> (dtu, dtv, dmean), the rotation
    as the forward, dscale, dL/dR column-wise, the four quaternion sums, times rsqrt(|q|^2); raw: times exp(scale) and the
    projection of the normalisation (not below |q|^2 = 1e-24).
"""
import functools
import math

import numpy as np
import torch

from objective_cases import E, val, bar, scalar, lift, sqrt, rcp, where, U32, TINY32, f32
from oracle import surfel_ref as O

TILE = 16
NEAR32 = f32(0.2)                                  # GSR_NEAR_N
FLOOR32 = float(np.float32(3.0) * np.float32(0.707106))     # GSR_CUTOFF * GSR_FILTER_SIZE, the fp32 product
MIN_EXT2_32 = f32(1e-4)                            # GSR_AABB_MIN_EXT2
SH_C = [O.SH_C0, -O.SH_C1, O.SH_C1, -O.SH_C1] + list(O.SH_C2) + list(O.SH_C3)       # with the signs of the basis functions


# ------------------------------------------------------------------------------------------------ arithmetic helpers
def conv(mode, t):
    """An fp32 input tensor (or an fp64 autograd leaf) in the arithmetic of `mode`."""
    if mode == "bar":
        return lift(mode, t.detach())
    return t.float() if mode == "f32" else t.double()


def stack(items, dim=-1):
    if any(isinstance(a, E) for a in items):
        items = [E.of(a) for a in items]
        vs = torch.broadcast_tensors(*[a.v for a in items])
        bs = [b.expand_as(v) for b, v in zip([a.b for a in items], vs)]
        return E(torch.stack(vs, dim), torch.stack(bs, dim))
    return torch.stack(torch.broadcast_tensors(*items), dim)


def esum(terms, roundings=None):
    """Sum of `terms` in any order: every term passes through `roundings` additions at the most (default: one fewer than terms)."""
    n = len(terms) - 1 if roundings is None else roundings
    if isinstance(terms[0], E):
        v = sum(t.v for t in terms)
        return E(v, sum(t.b for t in terms) + n * U32 * sum(t.v.abs() for t in terms))
    out = terms[0]
    for t in terms[1:]:
        out = out + t
    return out


def emax(a, b):
    """fmaxf: the larger one, a NaN ignored.  Its bound: where one operand stays below the other even when both move by their
    bars (2 E.b), the result is the other one and carries that one's bound alone; elsewhere the larger of the two bounds."""
    if isinstance(a, E) or isinstance(b, E):
        a, b = E.of(a), E.of(b)
        shape = (a.v + b.v).shape
        av, ab, bv, bb = a.v.expand(shape), a.b.expand(shape), b.v.expand(shape), b.b.expand(shape)
        bound = torch.where(av + 2 * ab < bv - 2 * bb, bb, torch.where(bv + 2 * bb < av - 2 * ab, ab, torch.maximum(ab, bb)))
        return E(torch.fmax(av, bv), bound)
    return torch.fmax(a, b if isinstance(b, torch.Tensor) else torch.full_like(a, b))


def sqrt_interval(a):
    """sqrtf of a quantity whose bound may exceed its value (the extents of a sub-pixel splat: 1e-4 with a bound of 1e-2): the
    first-order b / (2 sqrt v) of objective_cases.sqrt overstates that a hundredfold, so the bound is the image of
    [v - b, v + b] itself, and one rounding."""
    if not isinstance(a, E):
        return torch.sqrt(a)
    v = torch.sqrt(a.v)
    up, down = torch.sqrt(a.v + a.b) - v, v - torch.sqrt((a.v - a.b).clamp_min(0.0))
    return E(v, torch.maximum(up, down) + U32 * v)


def extent2(c, f, Ta, Tw):
    """h0 = c^2 - sum f_i Ta_i^2 with c = sum f_i Ta_i Tw_i (Ta = Tu or Tv).  c^2 and the sum cancel (a splat of 8 px at
    x = 240 px: 57600 - 57536), and most of what moves the one moves the other: an operator-by-operator bound counts the two
    separately and overstates the bound of the radius tenfold.  So the bound is taken of h0 as ONE function of the computed
    (f, Ta, Tw): the absolute partial derivatives times the bounds of those, and the roundings of the operations in between
    (c: two products a term and the sum, 4; c c: 1; the second sum: 4; the difference: 1) at their sensitivities."""
    terms = [(f[i] * Ta[i]) * Ta[i] for i in range(3)]
    h = c * c - esum(terms)
    if not isinstance(c, E):
        return h
    b = U32 * c.v * c.v + 4 * U32 * sum(t.v.abs() for t in terms) + U32 * h.v.abs() \
        + 2 * c.v.abs() * 4 * U32 * sum((f[i].v * Ta[i].v * Tw[i].v).abs() for i in range(3))
    for i in range(3):
        b = b + (2 * c.v * Ta[i].v * Tw[i].v - Ta[i].v ** 2).abs() * f[i].b \
              + (2 * f[i].v * (c.v * Tw[i].v - Ta[i].v)).abs() * Ta[i].b + (2 * c.v * f[i].v * Ta[i].v).abs() * Tw[i].b
    return E(h.v, b)


def expe(a):                                       # expf: one ulp
    if not isinstance(a, E):
        return torch.exp(a)
    v = torch.exp(a.v)
    return E(v, v * a.b + 2 * U32 * v)


def rsqrte(a):                                     # rsqrtf: one ulp
    if not isinstance(a, E):
        return torch.rsqrt(a)
    v = torch.rsqrt(a.v)
    return E(v, 0.5 * v * a.b / a.v + 2 * U32 * v)


def detach(a):
    return a if isinstance(a, E) else a.detach()


def cols(a, n):
    return [a[..., i] for i in range(n)]


# ------------------------------------------------------------------------------------------------ K1 geometry
GEOM_MUTATIONS = ("cw_is_half_width", "normal_sign_kept", "radius_floor_dropped", "aabb_min_ext2_dropped", "centre_weights_1_1_m1")
# aabb_min_ext2_dropped is an equivalent mutant: sqrt(1e-4) = 0.01 lies below the radius floor 3 * 0.707106 and fmaxf ignores
# the NaN of sqrtf(negative), so no output of the kernel depends on that constant.  The CPU test asserts exactly that.


def quat_rotation(q, mode):
    """rsqrt(|q|^2), |q|^2, the normalised quaternion and the nine entries r[row][col] of its rotation, as the kernel forms them."""
    qw, qx, qy, qz = cols(q, 4)
    n2 = esum([qw * qw, qx * qx, qy * qy, qz * qz])
    s = detach(rsqrte(n2))                          # (the operator's own normalisation carries no gradient)
    qw, qx, qy, qz = qw * s, qx * s, qy * s, qz * s
    r = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
         [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
         [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]
    return s, n2, (qw, qx, qy, qz), r


def preprocess_one(mode, means, scales, rots, opac, view, proj, W, H, *, mod=1.0, raw=False, tprecomp=None, mut=()):
    """preprocess_one of preprocess_fwd.hip for all Gaussians at once.  means [N,3], scales [N,2], rots [N,4], opac [N,1] or [N],
    view / proj: the 16 fp32 numbers each; tprecomp [N,9] or None.  -> dict of the record's fields, the discrete results and,
    in the bar arithmetic, the decisions with their margins."""
    m, V, P = conv(mode, means), conv(mode, view.reshape(16)), conv(mode, proj.reshape(16))
    px, py, pz = cols(m, 3)
    vx = px * V[0] + py * V[4] + pz * V[8] + V[12]
    vy = px * V[1] + py * V[5] + pz * V[9] + V[13]
    vz = px * V[2] + py * V[6] + pz * V[10] + V[14]
    near = scalar(mode, NEAR32)
    if tprecomp is None:
        _, _, _, r = quat_rotation(conv(mode, rots), mode)
        sc = conv(mode, scales)
        sx, sy = cols(sc, 2)
        if raw:
            sx, sy = expe(sx), expe(sy)
        mod_ = scalar(mode, f32(mod))
        sx, sy = sx * mod_, sy * mod_
        rows = [(r[0][0] * sx, r[1][0] * sx, r[2][0] * sx, False), (r[0][1] * sy, r[1][1] * sy, r[2][1] * sy, False),
                (px, py, pz, True)]
        hw, hh = 0.5 * W, 0.5 * H
        cw, ch = (hw if "cw_is_half_width" in mut else 0.5 * (W - 1)), 0.5 * (H - 1)
        Tu, Tv, Tw = [], [], []
        for a, b, c, one in rows:
            h0 = a * P[0] + b * P[4] + c * P[8]
            h1 = a * P[1] + b * P[5] + c * P[9]
            h3 = a * P[3] + b * P[7] + c * P[11]
            if one:
                h0, h1, h3 = h0 + P[12], h1 + P[13], h3 + P[15]
            Tu.append(h0 * hw + h3 * cw)
            Tv.append(h1 * hh + h3 * ch)
            Tw.append(h3)
        nrm = [r[0][2] * V[0 + j] + r[1][2] * V[4 + j] + r[2][2] * V[8 + j] for j in range(3)]
    else:
        t = conv(mode, tprecomp)
        Tu, Tv, Tw = [t[:, i] for i in range(3)], [t[:, 3 + i] for i in range(3)], [t[:, 6 + i] for i in range(3)]
        zero = 0.0 * vz
        nrm = [zero, zero, zero + 1.0]
        if mode == "bar":
            nrm = [E(n.v) for n in nrm]
    cosv = -(vx * nrm[0] + vy * nrm[1] + vz * nrm[2])
    flip = val(cosv) > 0 if "normal_sign_kept" not in mut else torch.ones_like(val(cosv), dtype=torch.bool)
    nrm = [where(flip, n, -n) for n in nrm]

    t9 = 1.0 if "centre_weights_1_1_m1" in mut else 9.0
    tt = (t9, t9, -1.0)
    d = esum([(tt[i] * Tw[i]) * Tw[i] for i in range(3)])
    dv = val(d)
    dsafe = where(dv != 0, d, 1.0)
    inv_d = rcp(dsafe, 2) if mode == "bar" else 1.0 / dsafe
    f = [tt[i] * inv_d for i in range(3)]
    cx = esum([(f[i] * Tu[i]) * Tw[i] for i in range(3)])
    cy = esum([(f[i] * Tv[i]) * Tw[i] for i in range(3)])
    h0x, h0y = extent2(cx, f, Tu, Tw), extent2(cy, f, Tv, Tw)
    if "aabb_min_ext2_dropped" in mut:
        ex, ey = sqrt_interval(h0x), sqrt_interval(h0y)                # (NaN below zero, as sqrtf)
    else:
        ex, ey = sqrt_interval(emax(h0x, MIN_EXT2_32)), sqrt_interval(emax(h0y, MIN_EXT2_32))
    rad_f = emax(ex, ey)
    if "radius_floor_dropped" not in mut:
        rad_f = emax(rad_f, FLOOR32)
    rad_f = detach(rad_f)
    radius = torch.ceil(val(rad_f))
    radius = torch.where(torch.isfinite(radius), radius, torch.zeros_like(radius))
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    cxd, cyd = detach(cx), detach(cy)
    q = [(cxd - radius) * (1.0 / TILE), (cyd - radius) * (1.0 / TILE),
         (cxd + radius + float(TILE) - 1.0) * (1.0 / TILE), (cyd + radius + float(TILE) - 1.0) * (1.0 / TILE)]
    lim = (gx, gy, gx, gy)
    rect = torch.stack([torch.trunc(val(q[i])).clamp(0, lim[i]) for i in range(4)], -1).to(torch.int64)
    tiles = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    vis = (val(vz) > val(near)) & (val(cosv) != 0) & (dv != 0) & (tiles > 0) & torch.isfinite(val(cx)) & torch.isfinite(val(cy))

    o = conv(mode, opac.reshape(-1))
    if raw:
        den = 1.0 + expe(-o)
        opacity = rcp(den, 2) if mode == "bar" else 1.0 / den
    else:
        opacity = o
    out = dict(vis=vis, Tu=stack(Tu), Tv=stack(Tv), Tw=stack(Tw), xy=stack([cx, cy]), normal=stack(nrm), opacity=opacity,
               depth=vz, rad_f=rad_f, radii=torch.where(vis, radius, torch.zeros_like(radius)).to(torch.int32),
               rect=torch.where(vis[:, None], rect, torch.zeros_like(rect)), tiles=torch.where(vis, tiles, torch.zeros_like(tiles)))
    if mode == "bar":
        # the decisions: (fp64 margin, bar of the deciding quantity).  A decision whose margin does not exceed its bar may fall
        # either way in fp32 and is excused; the decisions behind it are excused with it.
        inf = torch.full_like(dv, float("inf"))
        passed = val(vz) > val(near)
        dec = {"vz - NEAR": ((vz.v - near.v).abs(), bar(vz - near))}
        dec["|cosv|"] = (torch.where(passed, cosv.v.abs(), inf), bar(cosv))
        dec["|d|"] = (torch.where(passed, dv.abs(), inf), bar(d))
        alive = passed & (cosv.v != 0) & (dv != 0)
        up = torch.ceil(rad_f.v)
        dec["radius"] = (torch.where(alive, torch.minimum(up - rad_f.v, rad_f.v - (up - 1.0)), inf), bar(rad_f))
        for i, name in enumerate(("(cx - r)/16", "(cy - r)/16", "(cx + r + 15)/16", "(cy + r + 15)/16")):
            k = torch.round(q[i].v).clamp(1, lim[i])           # the integers at which trunc-and-clamp changes: 1 .. grid
            dec[name] = (torch.where(alive, (q[i].v - k).abs(), inf), bar(q[i]))
        out["decisions"] = dec
        late = lambda name, extra=0.0: ~(dec[name][0] > dec[name][1] + extra)
        ex_early = late("vz - NEAR") | late("|cosv|") | late("|d|")
        ex_rad = ex_early | late("radius")
        # a radius that may fall either way moves the rect's quantities by its own uncertainty: one step and its bar
        slack = torch.where(late("radius") & alive, (torch.ceil(bar(rad_f)) + 1.0) / TILE, torch.zeros_like(dv))
        ex_rect = ex_early.clone()
        for name in list(dec)[4:]:
            ex_rect |= late(name, slack)
        # visibility hangs on the early culls and on the rect being empty; the radius is compared where the Gaussian is
        # visible beyond doubt (a culled one has radius 0 whatever its extents)
        out["excused"] = dict(vis=ex_rect, rect=ex_rect, radius=ex_rect | (ex_rad & vis))
    return out


GEOM_FIELDS = ("Tu", "Tv", "Tw", "xy", "normal", "opacity", "depth")


def record_fields(splat, depth_key):
    """The device's record [N,20] and depth keys as the chain's fields."""
    return dict(Tu=splat[:, 0:3], Tv=splat[:, 3:6], Tw=splat[:, 6:9], xy=splat[:, 9:11], normal=splat[:, 11:14],
                opacity=splat[:, 14], depth=depth_key.view(torch.float32))


# ------------------------------------------------------------------------------------------------ SH colour
COLOR_MUTATIONS = ("poly13_sign", "dbz13_sign", "jac_transposed", "degree_cut_ignored")
TERM_MUTATIONS = ("projection_dropped", "inv_norm_dropped", "clamp_mask_ignored", "jac_transposed", "dbz13_sign")

# the eight numbers per basis function of k_sh_basis_rows: C x^fx y^fy z^fz (al xx + be yy + ga zz + de)
BASIS_ROWS = [(0, 0, 0, 0, 0, 0, 1), (0, 1, 0, 0, 0, 0, 1), (0, 0, 1, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0, 1), (1, 1, 0, 0, 0, 0, 1),
              (0, 1, 1, 0, 0, 0, 1), (0, 0, 0, -1, -1, 2, 0), (1, 0, 1, 0, 0, 0, 1), (0, 0, 0, 1, -1, 0, 0), (0, 1, 0, 3, -1, 0, 0),
              (1, 1, 1, 0, 0, 0, 1), (0, 1, 0, -1, -1, 4, 0), (0, 0, 1, -3, -3, 2, 0), (1, 0, 0, -1, -1, 4, 0), (0, 0, 1, 1, -1, 0, 0),
              (1, 0, 0, 1, -3, 0, 0)]


def sh_polynomials(mode, x, y, z, n, mut=()):
    """The first n written polynomials of utils/sh_utils.py:57-112 with their constants, and their derivatives with x, y, z
    independent (sh_basis16_grad; None: identically zero) -> (basis [n], dbx [n], dby [n], dbz [n])."""
    C = [scalar(mode, c, exact=False) for c in SH_C]
    one = 0.0 * x + 1.0
    if mode == "bar":
        one = E(one.v)
    b, dx, dy, dz = [C[0] * one], [None], [None], [None]
    if n > 1:
        b += [C[1] * y, C[2] * z, C[3] * x]
        dx += [None, None, C[3] * one]; dy += [C[1] * one, None, None]; dz += [None, C[2] * one, None]
    if n > 4:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [C[4] * xy, C[5] * yz, C[6] * (2.0 * zz - xx - yy), C[7] * xz, C[8] * (xx - yy)]
        dx += [C[4] * y, None, C[6] * -2.0 * x, C[7] * z, C[8] * 2.0 * x]
        dy += [C[4] * x, C[5] * z, C[6] * -2.0 * y, None, C[8] * -2.0 * y]
        dz += [None, C[5] * y, C[6] * 4.0 * z, C[7] * x, None]
    if n > 9:
        p13 = (4.0 * zz - xx + yy) if "poly13_sign" in mut else (4.0 * zz - xx - yy)
        b += [C[9] * y * (3.0 * xx - yy), C[10] * xy * z, C[11] * y * (4.0 * zz - xx - yy), C[12] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy),
              C[13] * x * p13, C[14] * z * (xx - yy), C[15] * x * (xx - 3.0 * yy)]
        dx += [C[9] * 6.0 * xy, C[10] * yz, C[11] * -2.0 * xy, C[12] * -6.0 * xz, C[13] * (4.0 * zz - 3.0 * xx - yy), C[14] * 2.0 * xz,
               C[15] * (3.0 * xx - 3.0 * yy)]
        dy += [C[9] * (3.0 * xx - 3.0 * yy), C[10] * xz, C[11] * (4.0 * zz - xx - 3.0 * yy), C[12] * -6.0 * yz, C[13] * -2.0 * xy,
               C[14] * -2.0 * yz, C[15] * -6.0 * xy]
        dz += [None, C[10] * xy, C[11] * 8.0 * yz, C[12] * (6.0 * zz - 3.0 * xx - 3.0 * yy),
               C[13] * (-8.0 if "dbz13_sign" in mut else 8.0) * xz, C[14] * (xx - yy), None]
    n = min(n, len(b))
    return b[:n], dx[:n], dy[:n], dz[:n]


def sh_polynomials_table(x, y, z, n):
    """The same values as preprocess_color16_kernel forms them in fp32: C mono poly from the table, fmaf by fmaf (torch has no
    fused multiply-add on fp32: each is formed in fp64 and rounded once, which is what fmaf does)."""
    def fma(a, b, c):
        a, b, c = (torch.as_tensor(t).double() for t in (a, b, c))
        return (a * b + c).float()
    b, dx, dy, dz = [], [], [], []
    for k in range(n):
        fx, fy, fz, al, be, ga, de = [float(v) for v in BASIS_ROWS[k]]
        C = torch.tensor(SH_C[k], dtype=torch.float32)
        poly = fma(al, x * x, fma(be, y * y, fma(ga, z * z, de + 0.0 * x)))
        ux, uy, uz = fma(fx, x, 1.0 - fx), fma(fy, y, 1.0 - fy), fma(fz, z, 1.0 - fz)
        mono = ux * uy * uz
        b.append(C * mono * poly)
        cm, cp = C * mono, C * poly
        dx.append(fma(cp, fx * uy * uz, cm * 2.0 * al * x))
        dy.append(fma(cp, fy * ux * uz, cm * 2.0 * be * y))
        dz.append(fma(cp, fz * ux * uy, cm * 2.0 * ga * z))
    return b, dx, dy, dz


def direction(mode, means, campos):
    m, c = conv(mode, means), conv(mode, campos.reshape(3))
    o = [m[:, i] - c[i] for i in range(3)]
    n = sqrt(esum([o[0] * o[0], o[1] * o[1], o[2] * o[2]]))
    il = rcp(n, 2) if mode == "bar" else 1.0 / n
    return [o[i] * il for i in range(3)], il


def color_chain(mode, deg, sh, means, campos, *, mut=(), form="written"):
    """Every colour producer: sh [N,M,3] -> rgb [N,3], the clamp decisions, v + 0.5 before the clamp, J [N,3,3] (J[c][a] =
    d rgb[c] / d dir[a], not masked by the clamp), the direction and 1 / |o|.  form="table" (fp32 only): the 16-lane kernel's
    arithmetic, DPP tree included."""
    M = sh.shape[1]
    n_act = M if "degree_cut_ignored" in mut else min(M, (deg + 1) ** 2)
    (x, y, z), il = direction(mode, means, campos)
    s = conv(mode, sh)
    if form == "table":
        assert mode == "f32"
        b, dbx, dby, dbz = sh_polynomials_table(x, y, z, n_act)
        zero = torch.zeros_like(x)[:, None].expand(-1, 3)

        def tree(terms):                          # quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
            v = list(terms) + [zero] * (16 - len(terms))
            for perm in ([1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14], [2, 3, 0, 1, 6, 7, 4, 5, 10, 11, 8, 9, 14, 15, 12, 13],
                         [7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8], list(range(15, -1, -1))):
                v = [v[i] + v[perm[i]] for i in range(16)]
            return v[0]
        total = tree([b[k][:, None] * s[:, k] for k in range(n_act)])
        J = torch.stack([tree([d[k][:, None] * s[:, k] for k in range(n_act)]) for d in (dbx, dby, dbz)], -1)
    else:
        b, dbx, dby, dbz = sh_polynomials(mode, x, y, z, n_act, mut)
        total = esum([b[k][:, None] * s[:, k] for k in range(n_act)], n_act)
        zero = 0.0 * (b[0][:, None] * s[:, 0])
        if mode == "bar":
            zero = E(zero.v)
        J = stack([esum([d[k][:, None] * s[:, k] for k in range(n_act) if d[k] is not None] or [zero], n_act)
                   for d in (dbx, dby, dbz)], -1)
    if "jac_transposed" in mut:
        J = E(J.v.transpose(1, 2), J.b.transpose(1, 2)) if mode == "bar" else J.transpose(1, 2)
    v = total + 0.5
    clamp = val(v) < 0
    return dict(rgb=where(clamp, 0.0, v), clamp=clamp, v=v, J=J, dir=(x, y, z), il=il)


def term_chain(mode, g, clamp, J, dirs, il, *, mut=()):
    """The view-direction term of dL/dmean: (I - d d^T) / |o| applied to sum_c g_c J[c][:], g masked by the clamp decisions.
    g [N,3]: dL/drgb as the device holds it (exact); clamp [N,3] bool; J, dirs, il from color_chain in the same arithmetic."""
    gg = conv(mode, g)
    if "clamp_mask_ignored" not in mut:
        gg = where(clamp, 0.0, gg)
    if "jac_transposed" in mut:
        J = E(J.v.transpose(1, 2), J.b.transpose(1, 2)) if mode == "bar" else J.transpose(1, 2)
    dd = [esum([gg[:, c] * J[:, c, a] for c in range(3)]) for a in range(3)]
    x, y, z = dirs
    dotp = esum([x * dd[0], y * dd[1], z * dd[2]])
    if "projection_dropped" in mut:
        out = dd
    else:
        out = [dd[0] - x * dotp, dd[1] - y * dotp, dd[2] - z * dotp]
    if "inv_norm_dropped" not in mut:
        out = [t * il for t in out]
    return stack(out)


# ------------------------------------------------------------------------------------------------ K8: dL/dT -> parameters
BWD_MUTATIONS = ("dscale_without_modifier", "quaternion_projection_dropped")


def bwd_chain(mode, dT, means, scales, rots, view, proj, W, H, *, mod=1.0, raw=False, mut=()):
    """Step 3b of preprocess_bwd_kernel with dn = 0: dT [N,9] (rows dTu, dTv, dTw: the device's own values after the AABB-centre
    step, exact) -> dL/dmean [N,3] (without the view-direction term), dL/dscales [N,2], dL/drotations [N,4]."""
    P = conv(mode, proj.reshape(16))
    g = conv(mode, dT)
    hw, hh, cw, ch = 0.5 * W, 0.5 * H, 0.5 * (W - 1), 0.5 * (H - 1)
    dtu, dtv, dmean = [], [], []
    for r in range(3):
        m0 = P[4 * r + 0] * hw + P[4 * r + 3] * cw
        m1 = P[4 * r + 1] * hh + P[4 * r + 3] * ch
        m2 = P[4 * r + 3]
        dtu.append(g[:, 0] * m0 + g[:, 3] * m1 + g[:, 6] * m2)
        dtv.append(g[:, 1] * m0 + g[:, 4] * m1 + g[:, 7] * m2)
        dmean.append(g[:, 2] * m0 + g[:, 5] * m1 + g[:, 8] * m2)
    s, n2, (qw, qx, qy, qz), R = quat_rotation(conv(mode, rots), mode)
    sx, sy = cols(conv(mode, scales), 2)
    if raw:
        sx, sy = expe(sx), expe(sy)
    mod_ = scalar(mode, f32(mod))
    sx, sy = sx * mod_, sy * mod_
    ds0 = dtu[0] * R[0][0] + dtu[1] * R[1][0] + dtu[2] * R[2][0]
    ds1 = dtv[0] * R[0][1] + dtv[1] * R[1][1] + dtv[2] * R[2][1]
    if "dscale_without_modifier" not in mut:
        ds0, ds1 = ds0 * mod_, ds1 * mod_
    d00, d10, d20 = dtu[0] * sx, dtu[1] * sx, dtu[2] * sx
    d01, d11, d21 = dtv[0] * sy, dtv[1] * sy, dtv[2] * sy
    gr = 2.0 * esum([-(qz * d01), qz * d10, -(qy * d20), qx * d21])
    gx = 2.0 * esum([qy * d01, qy * d10, -(2.0 * qx * d11), qz * d20, qw * d21])
    gy = 2.0 * esum([-(2.0 * qy * d00), qx * d01, qx * d10, -(qw * d20), qz * d21])
    gz = 2.0 * esum([-(2.0 * qz * d00), -(qw * d01), qw * d10, -(2.0 * qz * d11), qx * d20, qy * d21])
    gq = [gr, gx, gy, gz]
    dq = [t * s for t in gq]
    if raw:
        ds0, ds1 = ds0 * (sx / mod_), ds1 * (sy / mod_)
        if "quaternion_projection_dropped" not in mut:
            qd = esum([qw * gr, qx * gx, qy * gy, qz * gz])
            proj_ = [(gq[i] - (qw, qx, qy, qz)[i] * qd) * s for i in range(4)]
            small = val(n2) < f32(1e-24)
            dq = [where(small, dq[i], proj_[i]) for i in range(4)]
    return dict(dmean=stack(dmean), dscales=stack([ds0, ds1]), drotations=stack(dq))


# ------------------------------------------------------------------------------------------------ cases
def settings_of(cam):
    """The 16 + 16 + 3 fp32 numbers the kernels are handed for a camera, and its size."""
    return dict(view=cam.world_view_transform.detach().cpu().float().contiguous(),
                proj=cam.full_proj_transform.detach().cpu().float().contiguous(),
                campos=cam.camera_center.detach().cpu().float().contiguous(), W=int(cam.image_width), H=int(cam.image_height))


def _conftest():
    import conftest
    return conftest


# name -> (kind, seed, options)
RANDOM_CASES = {"facing s0": ("facing", 0, {}), "facing s1": ("facing", 1, {}), "free s0": ("free", 0, {}), "free s1": ("free", 1, {}),
                "facing s2 modifier 0.7": ("facing", 2, dict(mod=0.7)), "free s2 off-axis camera": ("free", 2, dict(cam=1)),
                "free s3 raw": ("free", 3, dict(raw=True)), "facing s4 raw": ("facing", 4, dict(raw=True)),
                "facing s3 transmat_precomp": ("facing", 3, dict(precomp=True))}
SIZES = (1, 63, 64, 65, 255, 257)
EDGE_SIZES = ((33, 17), (256, 160))


@functools.lru_cache(maxsize=None)
def random_case(name, n=1000, w=250, h=130):
    """-> dict(inputs of preprocess_one as fp32 CPU tensors, cam, options)."""
    from gaussmart_amd.synthetic import make_scene, activate, jittered_cameras
    kind, seed, opt = RANDOM_CASES[name]
    params, cam = (_conftest().facing_scene if kind == "facing" else make_scene)(n, w, h, seed=seed)
    if "cam" in opt:
        cam = jittered_cameras(3, w, h, seed=seed)[opt["cam"]]
    raw = bool(opt.get("raw"))
    a = activate(params)
    c = dict(means=params["xyz"], scales=params["scaling"] if raw else a["scales"], rots=params["rotation"] if raw else a["rotations"],
             opac=params["opacity"] if raw else a["opacities"], f_dc=params["features_dc"], f_rest=params["features_rest"],
             cam=cam, mod=opt.get("mod", 1.0), raw=raw, precomp=None, **settings_of(cam))
    if opt.get("precomp"):
        t = preprocess_one("f64", c["means"], c["scales"], c["rots"], c["opac"], c["view"], c["proj"], c["W"], c["H"])
        c["precomp"] = torch.cat([t["Tu"], t["Tv"], t["Tw"]], 1).float().contiguous()      # the fp64 Tm rounded to fp32
    return c


@functools.lru_cache(maxsize=None)
def size_case(n):
    params, cam = _conftest().facing_scene(n, 33, 17, seed=40 + n)
    from gaussmart_amd.synthetic import activate
    a = activate(params)
    return dict(means=params["xyz"], scales=a["scales"], rots=a["rotations"], opac=a["opacities"], cam=cam, mod=1.0, raw=False,
                precomp=None, **settings_of(cam))


def _rot_x(theta):
    return [math.cos(theta / 2), math.sin(theta / 2), 0.0, 0.0]


@functools.lru_cache(maxsize=None)
def edge_case(w, h):
    """About 200 constructed Gaussians, each a stated distance from the threshold it is named after (camera at the origin looking
    down +z; pixel = ndc * W/2 + (W-1)/2).  -> the case dict with `labels`."""
    from gaussmart_amd.camera import look_at_camera
    fovx = math.radians(60.0)
    cam = look_at_camera(eye=(0, 0, 0), target=(0, 0, 1), up=(0, -1, 0), fovx=fovx, width=w, height=h, device="cpu")
    S = settings_of(cam)
    P = S["proj"].double()
    # a point (x, y, z, 1) @ proj = (ax x, ay y, ., z): ndc = (ax x / z, ay y / z)
    ax, ay = float(P[0, 0]), float(P[1, 1])
    gx, gy = (w + 15) // 16, (h + 15) // 16
    rows, labels = [], []

    def at_pixel(u, v, z):
        return [(u - 0.5 * (w - 1)) / (0.5 * w) * z / ax, (v - 0.5 * (h - 1)) / (0.5 * h) * z / ay, z]

    def scale_for(radius_px, z):                    # a fronto-parallel surfel of this scale has extents 3 s ax (W/2) / z
        return radius_px / 3.0 * z / (ax * 0.5 * w)

    def add(label, pos, s, q=(1.0, 0.0, 0.0, 0.0), opa=0.8):
        s = (s, s) if not isinstance(s, tuple) else s
        rows.append(list(pos) + list(s) + list(q) + [opa])
        labels.append(label)

    cu, cv = 0.5 * (w - 1), 0.5 * (h - 1)
    for k, z in enumerate((0.2 * (1 + 2.0 ** -10), 0.2 * (1 - 2.0 ** -10), -1.0, -0.2)):
        for du in (0.0, 3.25, -5.0):
            add(f"near plane z={z:.6f}", at_pixel(cu + du, cv, z) if z > 0 else [0.01 * du, 0.0, z], 0.004)
    for z in (2.0, 5.0, 9.0):
        r = 4.5                                     # un-ceiled 4.5: radius 5, half a pixel from both integers
        sc = scale_for(r, z)
        for cross in (2.0, -2.0):                   # the rect's decision: (c + r + 15) / 16 >= 1 and (c - r) / 16 < grid
            add(f"left border {cross:+}", at_pixel(1.0 + cross - 5.0, cv, z), sc)
            add(f"right border {cross:+}", at_pixel(16.0 * gx - cross + 5.0, cv, z), sc)
            add(f"top border {cross:+}", at_pixel(cu, 1.0 + cross - 5.0, z), sc)
            add(f"bottom border {cross:+}", at_pixel(cu, 16.0 * gy - cross + 5.0, z), sc)
        for tu in range(0, gx + 1):
            for tv in range(0, gy + 1):
                if w < 64 or (tu + tv + int(z)) % 7 == 0:
                    add(f"tile corner ({tu},{tv})", at_pixel(16.0 * tu, 16.0 * tv, z), sc)
        for u, v in ((-100.0, -100.0), (3.0 * w, cv), (cu, -60.0), (cu, 4.0 * h), (-2000.0, 5000.0)):
            add("off screen", at_pixel(u, v, z), sc)
        for s in (1e-5, 1e-7, 3e-4):
            add(f"sub-pixel scale {s}", at_pixel(cu + 2.25, cv - 1.75, z), s)
            add(f"sub-pixel scale {s}, anisotropic", at_pixel(3.25, 2.75, z), (s, 1e-3 * s))
        # (up to 1e5 px: at 9e5 the bar of the un-ceiled radius is 1.9 px, so no placement there is decided)
        for r_px in (w + h + 0.5, 1e3 + 0.5, 1e4 + 0.5, 3e4 + 0.5, 1e5 + 0.5):
            add(f"radius {r_px:.0f} px", at_pixel(cu + 1.5, cv + 0.5, z), scale_for(r_px, z))
        for deg_ in (80.0, 89.0, 89.9):
            for sgn in (1.0, -1.0):
                add(f"tilt {deg_} deg", [0.0, 0.0, z], (0.05 * z, 0.02 * z), _rot_x(sgn * math.radians(deg_)))
        # the surfel's plane passes 1e-3 from the camera centre: p . n = z cos(theta) = 1e-3
        for dist in (1e-3, -1e-3):
            add(f"plane {dist} from the camera", [0.0, 0.0, z], 0.01 * z, _rot_x(math.acos(dist / z)))
        # d = 9 (Tw0^2 + Tw1^2) - Tw2^2 five per cent either side of zero: 3 sy sin(theta) = z (1 +- 0.05) at theta = 60 degrees
        for off in (0.05, -0.05):
            th = math.radians(60.0)
            add(f"d {off:+} z^2 from zero", [0.0, 0.0, z], (0.01 * z, z * (1 + off) / (3 * math.sin(th))), _rot_x(th))
        q = np.array([0.8, 0.3, -0.4, 0.2]); q /= np.linalg.norm(q)
        for norm in (1e-3, 1e3, 1.0):
            add(f"quaternion norm {norm}", at_pixel(cu - 3.0, cv + 2.0, z), (scale_for(6.3, z), scale_for(2.2, z)), tuple(q * norm))
    t = torch.tensor(rows, dtype=torch.float64).float()
    return dict(means=t[:, 0:3].contiguous(), scales=t[:, 3:5].contiguous(), rots=t[:, 5:9].contiguous(), opac=t[:, 9:10].contiguous(),
                cam=cam, mod=1.0, raw=False, precomp=None, labels=labels, **S)


def geom_run(mode, c, mut=()):
    return preprocess_one(mode, c["means"], c["scales"], c["rots"], c["opac"], c["view"], c["proj"], c["W"], c["H"], mod=c["mod"],
                          raw=c["raw"], tprecomp=c["precomp"], mut=mut)


def geom_cases():
    """name -> thunk of the case dict, every case of part 1."""
    out = {f"random {k}": functools.partial(random_case, k) for k in RANDOM_CASES}
    out.update({f"edges {w}x{h}": functools.partial(edge_case, w, h) for w, h in EDGE_SIZES})
    out.update({f"sizes N={n}": functools.partial(size_case, n) for n in SIZES})
    return out


# colour: (deg, M) x N
COLOR_GRID = [(0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16)]
COLOR_NS = (1, 31, 32, 33, 65, 257)
COLOR_CAMPOS = (0.3, -0.2, 0.1)


@functools.lru_cache(maxsize=None)
def color_case(deg, M, n):
    """Loud coefficients (all M drawn with sigma 0.5, so that |J| is of order 1) and directions that include each coordinate
    axis, x = y and |o| = 0.25 -> (sh [n,M,3], means [n,3], campos [3]) fp32.  The DC coefficient is drawn around -1.5: v + 0.5
    then has mean 0.08 and a fifth to three fifths of the channels clamp at every degree (around 0, degree 0 would clamp 0.02 %)."""
    g = torch.Generator().manual_seed(7000 + 100 * deg + 10 * M + n)
    sh = 0.5 * torch.randn(n, M, 3, generator=g)
    sh[:, 0] -= 1.5
    campos = torch.tensor(COLOR_CAMPOS)
    o = torch.randn(n, 3, generator=g) * torch.tensor([2.0, 1.5, 4.0])
    special = torch.tensor([[3.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 5.0], [1.5, 1.5, -2.0], [0.15, -0.1, 0.1732050808]])
    k = min(n, special.shape[0])
    first = (n * 7 // 13) % n if n > special.shape[0] else 0          # (not always lane 0 of a row)
    idx = [(first + i) % n for i in range(k)]
    o[idx] = special[:k] if n > 1 else special[4:5]
    return sh.contiguous(), (o + campos).contiguous(), campos


def color_truth(deg, M, n):
    sh, means, campos = color_case(deg, M, n)
    return color_chain("bar", deg, sh, means, campos)


# ------------------------------------------------------------------------------------------------ comparison
def ratio(err, b):
    q = torch.where(err == 0, torch.zeros_like(err), err / b)
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))
    return float(q.max()) if q.numel() else 0.0


def use_of(got, truth, where_=None):
    """max |got - truth| / bar(truth) over the elements (of the rows `where_`)."""
    got, want, b = got.detach().double().cpu(), truth.v, bar(truth)
    if where_ is not None:
        got, want, b = got[where_], want[where_], b[where_]
    err = (got - want).abs()
    return ratio(err, b), (float(err.max()) if err.numel() else 0.0), (float(b.max()) if b.numel() else 0.0)


# ------------------------------------------------------------------------------------------------ scenes of the device tests
@functools.lru_cache(maxsize=None)
def color_scene(deg, M, n):
    """color_case as a scene every Gaussian of which is visible (the colour passes skip culled ones): small camera-facing surfels
    seen by a camera 70 units back, while the view direction is taken from COLOR_CAMPOS -- the kernels read the camera centre
    and the matrices as separate inputs.  Activated and raw parameters of the same surfels."""
    from gaussmart_amd.camera import look_at_camera
    sh, means, campos = color_case(deg, M, n)
    cam = look_at_camera(eye=(0, 0, -70), target=(0, 0, 0), up=(0, -1, 0), fovx=math.radians(60.0), width=64, height=48, device="cpu")
    g = torch.Generator().manual_seed(n)
    q = torch.tensor([1.0, 0.0, 0.0, 0.0]) + 0.2 * torch.randn(n, 4, generator=g)
    return dict(sh=sh, means=means, campos=campos, cam=cam, rots=q.contiguous(), scales=torch.full((n, 2), 0.2), opac=torch.full((n, 1), 0.8),
                scales_raw=torch.full((n, 2), math.log(0.2)), opac_raw=torch.full((n, 1), math.log(0.8 / 0.2)), mod=1.0, raw=False,
                precomp=None, **{k: v for k, v in settings_of(cam).items() if k != "campos"})


@functools.lru_cache(maxsize=None)
def term_scene(deg, M, seed=0, clamped_channel=None, n=600, w=128, h=96):
    """The scene of parts 3 and 4: make_scene's geometry (raw parameters), loud coefficients as color_case; clamped_channel: that
    channel's DC coefficient at -12, so that it clamps on every Gaussian."""
    from gaussmart_amd.synthetic import make_scene
    params, cam = make_scene(n, w, h, seed=seed)
    g = torch.Generator().manual_seed(900 + 10 * deg + seed)
    sh = 0.5 * torch.randn(n, M, 3, generator=g)
    sh[:, 0] -= 1.5
    if clamped_channel is not None:
        sh[:, 0, clamped_channel] = -12.0
    s = dict(xyz=params["xyz"], scaling=params["scaling"], rotation=params["rotation"], opacity=params["opacity"],
             f_dc=sh[:, :1].contiguous(), f_rest=sh[:, 1:].contiguous(), sh=sh.contiguous(), cam=cam, deg=deg, M=M, **settings_of(cam))
    s["scales"], s["rots"], s["opac"] = torch.exp(s["scaling"]), torch.nn.functional.normalize(s["rotation"]), torch.sigmoid(s["opacity"])
    return s


def image_weights(shape_c, shape_a, normals=True):
    """The image weights of tests/test_gpu_factored_sh.py; normals=False: zero on the normal planes of allmap (dn = 0)."""
    gen = torch.Generator().manual_seed(11)
    wc = torch.randn(shape_c, generator=gen)
    wa = torch.randn(shape_a, generator=gen) * 0.1
    if not normals:
        wa[2:5] = 0.0
    return wc, wa
