"""Generate gaussmart_amd/csrc/mc_tables.h, the marching-cubes case table of gaussmart_amd/csrc/mcubes.hip.

    python scripts/gen_mc_tables.py            # rewrites the header
    python scripts/gen_mc_tables.py --check    # exit 1 if the committed header differs

The table is derived here, not typed in:
  - corner i of a cube sits at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1); bit i of a case is set when corner i is
    negative (tsdf < 0, behind the observed surface);
  - edge 4 a + k runs along axis a from the corner with bit a clear (the k-th such corner in increasing order) to that
    corner + e_a.  The voxel at the edge's first corner owns the edge (one mesh vertex per crossing edge);
  - on each of the six faces, walked counter-clockwise seen from outside the cube, every maximal run of negative corners
    gives one segment from the edge where the walk leaves the run to the edge where it entered it.  A face with two
    negative corners on a diagonal (ambiguous) therefore cuts off each negative corner on its own: a rule that depends on
    the face's four signs only, so the two cubes sharing a face agree and the glued surface has no cracks;
  - every crossing edge is left by exactly one segment and entered by exactly one (the two faces of an edge walk it in
    opposite directions), so the segments link into closed loops; each loop is fan-triangulated from its smallest edge
    whose diagonals stay off the cube's faces (a diagonal in a face would be shared with the neighbouring cube);
  - the orientation is fixed once, from the one-negative-corner case: triangle normals (v1-v0)x(v2-v0) point away from
    the negative corners, toward positive tsdf.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gaussmart_amd", "csrc", "mc_tables.h")
MAX_TRIS = 5


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edges():
    """[(corner0, corner1, axis)] for the 12 edges, edge index 4 axis + k."""
    out = []
    for a in range(3):
        for c in range(8):
            if not (c >> a) & 1:
                out.append((c, c | (1 << a), a))
    return out


EDGES = edges()
EDGE_OF = {frozenset((c0, c1)): i for i, (c0, c1, _) in enumerate(EDGES)}


def faces():
    """Six faces as corner cycles, counter-clockwise seen from outside the cube."""
    out = []
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        for s in (0, 1):
            cyc = []
            for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):   # CCW seen from +a (u x w = a)
                cyc.append((s << a) | (du << u) | (dw << w))
            out.append(cyc if s == 1 else cyc[::-1])
    return out


FACES = faces()


def face_segments(case, cyc):
    neg = [(case >> c) & 1 for c in cyc]
    if all(neg) or not any(neg):
        return []
    segs = []
    for i in range(4):
        if neg[i] and not neg[i - 1]:          # a negative run starts at position i
            j = i
            while neg[(j + 1) % 4]:
                j = (j + 1) % 4
            entry = EDGE_OF[frozenset((cyc[i - 1], cyc[i]))]
            leave = EDGE_OF[frozenset((cyc[j], cyc[(j + 1) % 4]))]
            segs.append((leave, entry))
    return segs


def is_ambiguous_face(case, cyc):
    neg = [(case >> c) & 1 for c in cyc]
    return neg in ([1, 0, 1, 0], [0, 1, 0, 1])


def case_loops(case):
    nxt = {}
    for cyc in FACES:
        for a, b in face_segments(case, cyc):
            assert a not in nxt, (case, a)
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def edge_faces(e):
    c0, _, a = EDGES[e]
    return {(b, (c0 >> b) & 1) for b in range(3) if b != a}


def fan_start(loop):
    """The smallest edge of the loop from which no fan diagonal lies in a cube face: such a diagonal would also be drawn
    by the neighbouring cube and make a mesh edge of four triangles."""
    k = len(loop)
    for s in sorted(loop):
        i = loop.index(s)
        if all(not (edge_faces(s) & edge_faces(loop[(i + j) % k])) for j in range(2, k - 1)):
            return i
    raise AssertionError(f"no fan start without a face diagonal in loop {loop}")


def _tris(case, flip):
    tris = []
    for loop in case_loops(case):
        if flip:
            loop = [loop[0]] + loop[1:][::-1]
        i = fan_start(loop)
        loop = loop[i:] + loop[:i]
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def _mid(e):
    c0, c1, _ = EDGES[e]
    p, q = corner_pos(c0), corner_pos(c1)
    return [(p[i] + q[i]) / 2 for i in range(3)]


def _normal(t):
    a, b, c = (_mid(e) for e in t)
    u = [b[i] - a[i] for i in range(3)]
    v = [c[i] - a[i] for i in range(3)]
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def build_table():
    # orientation from the one-negative-corner case: the normal must point away from corner 0, toward (1, 1, 1)
    (t,) = _tris(1, False)
    flip = sum(_normal(t)) < 0
    (t,) = _tris(1, flip)
    assert sum(_normal(t)) > 0
    table = [_tris(c, flip) for c in range(256)]
    worst = max(len(t) for t in table)
    assert worst <= MAX_TRIS, f"a case needs {worst} triangles > {MAX_TRIS}: widen the table"
    return table


def render_header(table):
    lines = [
        "// Generated by scripts/gen_mc_tables.py -- do not edit.  Marching-cubes case table of mcubes.hip (see the script for",
        "// the corner / edge numbering and the ambiguous-face rule).",
        "#pragma once",
        "#include <stdint.h>",
        "",
        f"#define MC_MAX_TRIS {MAX_TRIS}",
        "",
        "// edge e: from corner mc_edge_corner[e] along axis mc_edge_axis[e]; corner c at offset (c & 1, c >> 1 & 1, c >> 2 & 1)",
        "__constant__ uint8_t mc_edge_corner[12] = {" + ", ".join(str(c0) for c0, _, _ in EDGES) + "};",
        "__constant__ uint8_t mc_edge_axis[12] = {" + ", ".join(str(a) for _, _, a in EDGES) + "};",
        "",
        "// triangles of case c (bit i set: corner i has tsdf < 0)",
        "__constant__ uint8_t mc_num_tris[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(table[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append(f"__constant__ int8_t mc_tri_edges[256][{3 * MAX_TRIS}] = {{")
    for c in range(256):
        flat = [e for t in table[c] for e in t]
        flat += [-1] * (3 * MAX_TRIS - len(flat))
        lines.append("    {" + ", ".join(str(e) for e in flat) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args(argv)
    text = render_header(build_table())
    if args.check:
        ok = os.path.exists(args.out) and open(args.out).read() == text
        print("mc_tables.h up to date" if ok else "mc_tables.h differs from the generator")
        return 0 if ok else 1
    with open(args.out, "w") as f:
        f.write(text)
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
