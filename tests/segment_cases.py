"""Inputs of the segment-initialisation tests, shared by tests/golden/make_golden_segment_init.py (which records what the
reference computes on them) and the tests.  Everything here is built from IEEE multiplications, additions, square roots
and integer arithmetic only, so it has the same bits on every machine; nothing depends on a random generator's stream.
Also the np.longdouble restatement of the projection and hull formulas the tolerances are measured against."""
import numpy as np

_PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
LD = np.longdouble


def uniform(n, dims, seed=0):
    """[n, dims] in [0, 1): Weyl sequences frac(i sqrt(prime) + offset)."""
    i = np.arange(1, n + 1, dtype=np.float64)
    cols = []
    for d in range(dims):
        a = np.modf(np.sqrt(np.float64(_PRIMES[(d + seed) % len(_PRIMES)])))[0]
        cols.append(np.modf(i * a + (0.137 * (seed + 1) + 0.31 * d))[0])
    return np.stack(cols, axis=1)


def blob(n, seed=0):
    """A bell-shaped cloud (sum of three uniforms per axis), roughly within radius 1."""
    u = uniform(n, 9, seed)
    return (u[:, 0:3] + u[:, 3:6] + u[:, 6:9]) - 1.5


def cube(n, seed=0):
    return uniform(n, 3, seed) - 0.5


def sphere(n, seed=0):
    v = uniform(n, 3, seed) * 2.0 - 1.0
    return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]


def hull_gauss():
    return blob(600, 1)


def hull_sphere():
    return np.concatenate([sphere(2000, 2), 0.9 * cube(3000, 3)])


def filter_cloud():
    return np.concatenate([10.0 * sphere(300, 4), cube(20000, 5)])


def large_cloud(nan_row=False):
    """The 20 000 points of the large projection / assignment case (row 17 has a NaN on request)."""
    p = blob(20000, 8) * 0.6
    if nan_row:
        p[17, 1] = np.nan
    return p


def cube_corners():
    return np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])


def rect_masks(M, H, W, seed=0):
    """M rectangles as a bool [M,H,W] stack, from integer arithmetic; mask 0 of seed 0 is empty when M >= 3 (area 0)."""
    out = np.zeros((M, H, W), bool)
    for m in range(M):
        k = 7919 * (m + 1) + 104729 * (seed + 1)
        x0, y0 = (k * 31) % W, (k * 17) % H
        w, h = 8 + (k * 13) % max(W // 3, 9), 8 + (k * 11) % max(H // 3, 9)
        if M >= 3 and m == 0 and seed == 0:
            continue
        out[m, y0:y0 + h, x0:x0 + w] = True
    return out


def centre_masks(H, W):
    """Three overlapping rectangles around the image centre, bool [3,H,W]."""
    out = np.zeros((3, H, W), bool)
    cx, cy = W // 2, H // 2
    out[0, cy - 100:cy + 100, cx - 120:cx - 20] = True
    out[1, cy - 60:cy + 20, cx - 40:cx + 60] = True
    out[2, cy - 100:cy + 100, cx + 30:cx + 110] = True
    return out


def stats_cloud():
    """(points f32 [n,3], sh colours f32 [n,3], labels int64 [n]): label 0 has no point, 1: one, 2: four, 3: five, 4: six,
    5: eight collinear points, 6: six coincident points, 7: 10 000; -1: 50 unlabelled; all interleaved."""
    parts, labels = [], []
    sizes = {1: 1, 2: 4, 3: 5, 4: 6, 7: 10000, -1: 50}
    for lab, k in sizes.items():
        parts.append(blob(k, 10 + lab) * (0.3 + 0.1 * abs(lab)) + np.array([lab, 0.5 * lab, -lab], np.float64))
        labels += [lab] * k
    t = np.arange(8, dtype=np.float64)[:, None]
    parts.append(np.array([0.5, -1.0, 2.0]) + t * np.array([0.25, 0.5, -0.125]))
    labels += [5] * 8
    parts.append(np.tile(np.array([[1.25, -0.75, 3.5]]), (6, 1)))
    labels += [6] * 6
    pts = np.concatenate(parts).astype(np.float32)
    labels = np.array(labels, np.int64)
    n = len(pts)
    perm = (np.arange(n, dtype=np.int64) * 7919) % n          # 7919 is prime and n is not a multiple of it: a permutation
    assert len(np.unique(perm)) == n
    col = (uniform(n, 3, 3) * 2.0 - 1.0).astype(np.float32)
    return pts[perm], col, labels[perm]


# ---------------------------------------------------------------- np.longdouble restatements
def hull_distances_ld(points, equations):
    """(d, bound) in longdouble: the distance to the nearest facet and the issue's bound 8 2^-53 (sum |n_k p_k| + |o|) / |n|
    of the minimising facet."""
    p, eq = np.asarray(points, LD), np.asarray(equations, LD)
    best = np.full(len(p), np.inf, LD)
    bound = np.zeros(len(p), LD)
    for a, b, c, o in eq:
        norm = np.sqrt(a * a + b * b + c * c)
        d = np.abs(a * p[:, 0] + b * p[:, 1] + c * p[:, 2] + o) / norm
        mag = (np.abs(a * p[:, 0]) + np.abs(b * p[:, 1]) + np.abs(c * p[:, 2]) + np.abs(o)) / norm
        better = d < best
        best = np.where(better, d, best)
        bound = np.where(better, mag, bound)
    return best, LD(8.0) * LD(2.0) ** -53 * bound


def project_ld(points, terms, fallback=None):
    """SEG_PROJ_* in longdouble from gaussmart_amd.segment_init.camera_terms: (uv [n,2], z [n]).  fallback: the DTU decision
    (None: decided here from the longdouble coordinates)."""
    p = np.asarray(points, LD)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    Wm, K, S = (np.asarray(terms[k], LD) for k in ("world_mat", "camera_mat", "scale_mat"))
    pos = np.asarray(terms["cam_pos"], LD)
    with np.errstate(all="ignore"):
        if terms["kind"] == 0:
            s = [S[r, 0] * x + S[r, 1] * y + S[r, 2] * z + S[r, 3] for r in range(4)]
            c = [Wm[r, 0] * s[0] + Wm[r, 1] * s[1] + Wm[r, 2] * s[2] + Wm[r, 3] * s[3] for r in range(4)]
            u, v, depth = K[0, 0] * (c[0] / c[3]) + K[0, 2], K[1, 1] * (c[1] / c[3]) + K[1, 2], c[2]
            if fallback is None:
                fallback = float(((u >= 0) & (u < 1554) & (v >= 0) & (v < 1162)).sum()) < 0.1 * len(p)
            if fallback:
                d = p - pos
                r = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
                u = r[:, 0] / (r[:, 2] + LD(1e-10)) * (LD(1554) / 3) + LD(777)
                v = r[:, 1] / (r[:, 2] + LD(1e-10)) * (LD(1162) / 3) + LD(581)
        elif terms["kind"] == 1:
            c = [Wm[r, 0] * x + Wm[r, 1] * y + Wm[r, 2] * z + Wm[r, 3] for r in range(3)]
            q = [K[r, 0] * c[0] + K[r, 1] * c[1] + K[r, 2] * c[2] for r in range(3)]
            u, v, depth = q[0] / q[2], q[1] / q[2], c[2]
        else:
            ok = ~np.isnan(p).any(axis=1)
            if not ok.any():
                return np.zeros((len(p), 2), LD), np.zeros(len(p), LD)
            lo, hi = p[ok].min(axis=0), p[ok].max(axis=0)
            pad, span = LD(0.1), LD(1) - 2 * LD(0.1)
            u = (pad + span * (x - lo[0]) / (hi[0] - lo[0] + LD(1e-10))) * LD(terms["img_w"])
            v = (pad + span * (y - lo[1]) / (hi[1] - lo[1] + LD(1e-10))) * LD(terms["img_h"])
            u, v = np.where(np.isnan(u), LD(0), u), np.where(np.isnan(v), LD(0), v)
            d = p - pos
            depth = d[:, 0] * Wm[2, 0] + d[:, 1] * Wm[2, 1] + d[:, 2] * Wm[2, 2]
    return np.stack([u, v], axis=1), depth


def max_dev(a, b):
    """largest |a - b| over the entries where both are finite, as a float"""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a - b)[ok].max()) if ok.any() else 0.0


def near_boundary(views_uvz, margin_px=1e-6, margin_z=1e-9):
    """Points within reach of a decision boundary of SEG_ASSIGN.  views_uvz: per view, in order, (uv, z, W, H) in longdouble
    or None for a view without masks.  A conservative superset of the issue's set: every view counts, not only those up to
    the one that labels the point."""
    near = None
    for item in views_uvz:
        if item is None:
            continue
        uv, z, W, H = item
        u, v = np.asarray(uv[:, 0], LD), np.asarray(uv[:, 1], LD)
        with np.errstate(invalid="ignore"):
            half = lambda a: np.abs((a - np.floor(a)) - LD(0.5)) < margin_px
            border = (np.abs(u) < margin_px) | (np.abs(u - W) < margin_px) | (np.abs(v) < margin_px) | (np.abs(v - H) < margin_px)
            here = half(u) | half(v) | border | (np.abs(np.asarray(z, LD)) < margin_z)
            here &= ~(np.isnan(u) | np.isnan(v) | np.isnan(np.asarray(z, LD)))     # a NaN decides (b) or (c) by itself
        near = here if near is None else (near | here)
    return near
