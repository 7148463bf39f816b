"""Test-only restatement of the mesh-export rules of include/gsr.h in float64 (torch / numpy): TSDF touch + integrate and
marching cubes with the generated case table.  Slow and simple; tests/test_gpu_mesh.py compares the kernels against it."""
import importlib.util
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 16
STRIDE = 4
BORDER = 1e-4


def mc_table():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "scripts", "gen_mc_tables.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class RefVolume:
    """Sparse volume: {block (3 ints): [5, 4096] float64 (tsdf, weight, r, g, b)}; voxel (x, y, z) of a block is entry
    x + 16 (y + 16 z).  `unstable_blocks`: blocks whose allocation decision lay within `eps_block` of a block boundary."""

    def __init__(self, voxel_size, sdf_trunc, eps_block=1e-6):
        self.vs, self.st, self.eps = float(voxel_size), float(sdf_trunc), eps_block
        self.blocks = {}
        self.unstable_blocks = set()
        self.unstable_voxels = {}   # block -> bool [4096]

    def touch(self, depth, intr, w2c, depth_trunc, mask=None):
        fx, fy, cx, cy = (float(v) for v in intr)
        depth_trunc = float(np.float32(depth_trunc))   # the library takes depth_trunc as a float: 0 < d <= it is exact
        d = torch.as_tensor(depth, dtype=torch.float64).reshape(depth.shape[-2:])
        H, W = d.shape
        vv, uu = torch.meshgrid(torch.arange(0, H, STRIDE, dtype=torch.float64), torch.arange(0, W, STRIDE, dtype=torch.float64),
                                indexing="ij")
        dd = d[::STRIDE, ::STRIDE]
        ok = (dd > 0) & (dd <= depth_trunc)
        if mask is not None:
            ok &= torch.as_tensor(mask).reshape(H, W)[::STRIDE, ::STRIDE].bool()
        z = dd[ok]
        pc = torch.stack([(uu[ok] - cx) * z / fx, (vv[ok] - cy) * z / fy, z], 1)
        c2w = torch.linalg.inv(torch.as_tensor(w2c, dtype=torch.float64))
        pw = pc @ c2w[:3, :3].T + c2w[:3, 3]
        bl = B * self.vs
        out = set()
        lo = torch.floor((pw - self.st) / bl).long()
        hi = torch.floor((pw + self.st) / bl).long()
        qlo, qhi = (pw - self.st) / bl, (pw + self.st) / bl
        amb_lo = (qlo - torch.round(qlo)).abs() < self.eps
        amb_hi = (qhi - torch.round(qhi)).abs() < self.eps
        span = int((hi - lo).max()) + 1 if len(lo) else 0
        for dz in range(span):
            for dy in range(span):
                for dx in range(span):
                    off = torch.tensor([dx, dy, dz])
                    b = lo + off
                    sel = (b <= hi).all(1)
                    # a block on the edge of a sample's range whose floor decision is within eps of a boundary
                    edge = ((off == 0) & amb_lo) | ((b == hi) & amb_hi)
                    for bb, e in zip(b[sel].tolist(), edge[sel].any(1).tolist()):
                        out.add(tuple(bb))
                        if e:
                            self.unstable_blocks.add(tuple(bb))
        # also the blocks just beyond an ambiguous bound (the float kernel may include them)
        for i in torch.nonzero(amb_lo.any(1)).flatten().tolist():
            for a in range(3):
                if amb_lo[i, a]:
                    self._mark_neighbours(lo[i], hi[i], a, -1)
        for i in torch.nonzero(amb_hi.any(1)).flatten().tolist():
            for a in range(3):
                if amb_hi[i, a]:
                    self._mark_neighbours(lo[i], hi[i], a, +1)
        for bb in out:
            if bb not in self.blocks:
                self.blocks[bb] = torch.zeros(5, B ** 3, dtype=torch.float64)
                self.unstable_voxels[bb] = torch.zeros(B ** 3, dtype=torch.bool)
        return out

    def _mark_neighbours(self, lo, hi, axis, side):
        lo, hi = lo.clone(), hi.clone()
        if side < 0:
            lo[axis] -= 1
            hi[axis] = lo[axis]
        else:
            hi[axis] += 1
            lo[axis] = hi[axis]
        for z in range(int(lo[2]), int(hi[2]) + 1):
            for y in range(int(lo[1]), int(hi[1]) + 1):
                for x in range(int(lo[0]), int(hi[0]) + 1):
                    self.unstable_blocks.add((x, y, z))

    def integrate(self, depth, rgb, intr, w2c, depth_trunc, mask=None, touched=None):
        fx, fy, cx, cy = (float(v) for v in intr)
        depth_trunc = float(np.float32(depth_trunc))
        d = torch.as_tensor(depth, dtype=torch.float64).reshape(depth.shape[-2:])
        H, W = d.shape
        col = torch.as_tensor(rgb, dtype=torch.float64).reshape(3, H, W)
        m = torch.ones(H, W, dtype=torch.bool) if mask is None else torch.as_tensor(mask).reshape(H, W).bool()
        M = torch.as_tensor(w2c, dtype=torch.float64)
        blocks = sorted(touched if touched is not None else self.blocks)
        if not blocks:
            return
        l = torch.arange(B ** 3)
        loc = torch.stack([l % B, (l // B) % B, l // (B * B)], 1)
        bt = torch.tensor(blocks)
        g = bt[:, None, :] * B + loc[None]
        p = (g.double() + 0.5) * self.vs
        pc = p @ M[:3, :3].T + M[:3, 3]
        x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
        zs = torch.where(z > 0, z, torch.ones_like(z))
        uf = fx * x / zs + cx + 0.5
        vf = fy * y / zs + cy + 0.5
        inside = (z > 0) & (uf >= BORDER) & (uf < W - BORDER) & (vf >= BORDER) & (vf < H - BORDER)

        def at(uu, vv):
            """(updated?, sdf, depth) of every voxel if it read pixel (uu, vv)."""
            ok_px = inside & (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            uu, vv = uu.clamp(0, W - 1), vv.clamp(0, H - 1)
            dv = d[vv, uu]
            mult = torch.sqrt(1 + ((uu.double() - cx) / fx) ** 2 + ((vv.double() - cy) / fy) ** 2)
            sdf = (dv - z) * mult
            return ok_px & (dv > 0) & (dv <= depth_trunc) & m[vv, uu] & (sdf > -self.st), sdf, dv

        u = torch.where(inside, uf, torch.zeros_like(uf)).long().clamp(0, W - 1)
        v = torch.where(inside, vf, torch.zeros_like(vf)).long().clamp(0, H - 1)
        ok, sdf, dv = at(u, v)
        t = torch.clamp(sdf / self.st, max=1.0)
        rgb8 = torch.floor(col.clamp(0, 1)[:, v, u] * 255)
        # decision stability of this view: near a rounding boundary the float kernel may read the neighbouring pixel; that
        # matters when the voxel is updated from either of the two
        frac = lambda q: (q - torch.round(q)).abs()
        step = lambda q, i: torch.where(q - torch.floor(q) < 0.5, i - 1, i + 1)
        near_u, near_v = frac(uf) < 1e-4, frac(vf) < 1e-4
        ok_u = at(step(uf, u), v)[0]
        ok_v = at(u, step(vf, v))[0]
        ok_uv = at(step(uf, u), step(vf, v))[0]   # near both boundaries: the diagonal neighbour is a candidate too
        unstable = (z > 0) & ((near_u & (ok | ok_u)) | (near_v & (ok | ok_v)) | (near_u & near_v & ok_uv) | (((sdf + self.st).abs() < 1e-6) & inside) |
                              ((uf - (W - BORDER)).abs() < 1e-4) |
                              ((vf - (H - BORDER)).abs() < 1e-4) | ((uf - BORDER).abs() < 1e-4) | ((vf - BORDER).abs() < 1e-4))
        for i, bb in enumerate(blocks):
            s = self.blocks[bb]
            k = ok[i]
            w = s[1, k]
            s[0, k] = (s[0, k] * w + t[i, k]) / (w + 1)
            for c in range(3):
                s[2 + c, k] = (s[2 + c, k] * w + rgb8[c, i, k]) / (w + 1)
            s[1, k] = w + 1
            self.unstable_voxels[bb] |= unstable[i]


def mc_dense(tsdf, weight, colour=None, voxel_size=1.0, origin=(0, 0, 0)):
    """Marching cubes of a dense [X,Y,Z] field with the generated table and the rules of include/gsr.h (float64, numpy).
    Returns (vertices [V,3], triangles [F,3], colours [V,3], vertex keys [(x, y, z, axis)]); vertices are one per crossing
    edge used by a valid cube, in key order."""
    T = mc_table()
    table = T.build_table()
    f = np.asarray(tsdf, np.float64)
    w = np.asarray(weight, np.float64)
    X, Y, Z = f.shape
    col = np.zeros(f.shape + (3,)) if colour is None else np.asarray(colour, np.float64)
    neg = f < 0
    valid = np.zeros((X - 1, Y - 1, Z - 1), bool)
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    allw = np.ones_like(valid)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, c >> 2
        sl = (slice(ox, X - 1 + ox), slice(oy, Y - 1 + oy), slice(oz, Z - 1 + oz))
        allw &= w[sl] > 0
        case |= neg[sl].astype(np.int64) << c
    valid = allw
    tris_e = []
    for idx in zip(*np.nonzero(valid & (case != 0) & (case != 255))):
        for tri in table[case[idx]]:
            keys = []
            for e in tri:
                c0, _, a = T.EDGES[e]
                keys.append((idx[0] + (c0 & 1), idx[1] + ((c0 >> 1) & 1), idx[2] + (c0 >> 2), a))
            tris_e.append(keys)
    keys = sorted({k for t in tris_e for k in t})
    index = {k: i for i, k in enumerate(keys)}
    verts = np.zeros((len(keys), 3))
    cols = np.zeros((len(keys), 3))
    org = np.asarray(origin, np.float64)
    for i, (x, y, z, a) in enumerate(keys):
        n = [x, y, z]
        n[a] += 1
        f0, f1 = abs(f[x, y, z]), abs(f[tuple(n)])
        p = (np.array([x, y, z], np.float64) + org + 0.5) * voxel_size
        p[a] += f0 / (f0 + f1) * voxel_size
        verts[i] = p
        cols[i] = (col[x, y, z] * f1 + col[tuple(n)] * f0) / (f0 + f1) / 255.0
    tris = np.array([[index[k] for k in t] for t in tris_e], np.int64).reshape(-1, 3)
    return verts, tris, cols, keys


def flat_wall_expected(voxel_centres, intr, wall_z, sdf_trunc, W, H):
    """Independent statement of the flat-wall case (camera at the origin looking down +z, wall at z = wall_z): the TSDF of a
    voxel is its distance to the wall along the ray of its pixel, / sdf_trunc, clipped at 1; NaN where not updated."""
    fx, fy, cx, cy = intr
    out = np.full(len(voxel_centres), np.nan)
    for i, (x, y, z) in enumerate(np.asarray(voxel_centres, np.float64)):
        if z <= 0:
            continue
        uf, vf = fx * x / z + cx + 0.5, fy * y / z + cy + 0.5
        if not (BORDER <= uf < W - BORDER and BORDER <= vf < H - BORDER):
            continue
        u, v = math.floor(uf), math.floor(vf)
        ray = np.array([(u - cx) / fx, (v - cy) / fy, 1.0])
        dist = (wall_z - z) * np.linalg.norm(ray)   # the ray's length between the voxel's depth and the wall's
        if dist <= -sdf_trunc:
            continue
        out[i] = min(1.0, dist / sdf_trunc)
    return out


def edge_keys(verts_index):
    """(x, y, z, axis) of the lattice edge each marching-cubes vertex lies on (vertex positions in voxel-index coordinates:
    two integral coordinates, one strictly between two integers)."""
    v = np.asarray(verts_index, np.float64)
    off = np.abs(v - np.round(v))
    axis = np.argmax(off, axis=1)
    base = np.round(v).astype(np.int64)
    rows = np.arange(len(v))
    base[rows, axis] = np.floor(v[rows, axis]).astype(np.int64)
    return [tuple(b) + (int(a),) for b, a in zip(base.tolist(), axis.tolist())]


def polygons(tris, keys):
    """The polygons a triangulated marching-cubes mesh was cut from: triangles merged across their in-cube diagonals (mesh
    edges whose two vertices do not lie on a common cube face).  Independent of which diagonals a case table chose."""
    import collections
    parent = list(range(len(tris)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    emap = collections.defaultdict(list)
    for t, tri in enumerate(np.asarray(tris).tolist()):
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            emap[(min(a, b), max(a, b))].append(t)
    for (a, b), ts in emap.items():
        ka, kb = keys[a], keys[b]
        on_face = any(ka[3] != c and kb[3] != c and ka[c] == kb[c] for c in range(3))
        if not on_face:
            for t in ts[1:]:
                parent[find(t)] = find(ts[0])
    groups = collections.defaultdict(set)
    for t, tri in enumerate(np.asarray(tris).tolist()):
        groups[find(t)].update(tri)
    return {frozenset(g) for g in groups.values()}
