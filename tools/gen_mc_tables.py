"""Generate latent-nerf-test_amd/csrc/mc_tables.h: the marching-cubes case tables, derived from first principles.

    python tools/gen_mc_tables.py           # (re)write the header
    python tools/gen_mc_tables.py --check   # exit 1 if the committed header differs from what this script writes

Convention (repeated in the header):
  * corner c = x + 2y + 4z of the unit cube, (x, y, z) in {0, 1}^3;
  * edges 0-3 run along x, 4-7 along y, 8-11 along z.  Edge 4*a + k (axis a) joins corner c0 and c0 + 2^a, where
    the two coordinates other than a are the bits of k, lower axis first;
  * a corner is INSIDE iff its value > iso (so NaN is outside).
Construction, per case (the 8 inside bits):
  1. on each of the 6 cube faces the surface crosses the face edges whose corners differ; the crossings are joined into
     segments by one fixed rule -- inside corners of an ambiguous face (two inside corners on a diagonal) are never
     connected, i.e. every maximal run of inside corners around the face gets its own segment.  The segments of a
     face therefore depend on that face's 4 corner signs only, which is what makes neighbouring cells join without
     cracks;
  2. each segment is directed so that, seen from outside the cube, the inside corners lie on its RIGHT; then every
     crossed edge has exactly one segment leaving it and one entering it, and the segments chain into closed loops;
  3. every loop is fan-triangulated from the first vertex (the loop starts at its smallest edge) whose fan diagonals
     do not lie in a cube face, so the only triangle edges on the cube's surface are the face segments;
  4. with that direction the triangles' normals (b - a) x (c - a) point from inside to outside.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "latent-nerf-test_amd", "csrc", "mc_tables.h")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e):
    """(c0, c1) of edge e, c1 = c0 + 2^axis."""
    a, k = divmod(e, 4)
    others = [b for b in range(3) if b != a]
    c0 = ((k & 1) << others[0]) | (((k >> 1) & 1) << others[1])
    return c0, c0 | (1 << a)


EDGES = [edge_corners(e) for e in range(12)]
EDGE_OF = {frozenset(p): e for e, p in enumerate(EDGES)}


def edge_faces(e):
    """The two cube faces (axis, side) an edge lies on."""
    a = e // 4
    c0 = EDGES[e][0]
    return {(b, (c0 >> b) & 1) for b in range(3) if b != a}


def face_cycle(a, s):
    """The 4 corners of face (axis a, side s) in cyclic order, and its outward normal."""
    b, c = (a + 1) % 3, (a + 2) % 3
    cyc = []
    for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
        cyc.append((s << a) | (u << b) | (v << c))
    n = [0, 0, 0]
    n[a] = 1 if s else -1
    return cyc, n


def _sub(p, q):
    return [p[i] - q[i] for i in range(3)]


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def _dot(p, q):
    return sum(p[i] * q[i] for i in range(3))


def mid(e):
    p, q = corner_pos(EDGES[e][0]), corner_pos(EDGES[e][1])
    return [(p[i] + q[i]) / 2.0 for i in range(3)]


def face_segments(case, a, s):
    """Directed segments (edge_from, edge_to) of one face: one per maximal run of inside corners around it."""
    cyc, n = face_cycle(a, s)
    ins = [(case >> c) & 1 for c in cyc]
    segs = []
    for i in range(4):
        if ins[i] and not ins[i - 1]:                       # a run of inside corners starts at i
            j = i
            while ins[(j + 1) % 4]:
                j = (j + 1) % 4
            e_in = EDGE_OF[frozenset((cyc[i - 1], cyc[i]))]
            e_out = EDGE_OF[frozenset((cyc[j], cyc[(j + 1) % 4]))]
            q = corner_pos(cyc[i])
            p0, p1 = mid(e_in), mid(e_out)
            left = _dot(n, _cross(_sub(p1, p0), _sub(q, p0))) > 0
            segs.append((e_out, e_in) if left else (e_in, e_out))   # inside corners on the right
    return segs


def case_loops(case):
    nxt = {}
    for a in range(3):
        for s in range(2):
            for e0, e1 in face_segments(case, a, s):
                assert e0 not in nxt, (case, e0)
                nxt[e0] = e1
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


def share_face(e0, e1):
    return bool(edge_faces(e0) & edge_faces(e1))


def fan(loop):
    k = len(loop)
    for a in range(k):
        if all(not share_face(loop[a], loop[(a + j) % k]) for j in range(2, k - 1)):
            return [(loop[a], loop[(a + j) % k], loop[(a + j + 1) % k]) for j in range(1, k - 1)]
    raise RuntimeError("no fan apex without a diagonal in a cube face for loop %s" % loop)


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        tris.extend(fan(loop))
    return tris


def tables():
    return [case_triangles(c) for c in range(256)]


def _check_orientation(tabs):
    # a single inside corner: every triangle's normal points away from it
    for c in range(8):
        q = corner_pos(c)
        for t in tabs[1 << c]:
            p = [mid(e) for e in t]
            nrm = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
            assert _dot(nrm, _sub(p[0], q)) > 0, (c, t)


def render_header():
    tabs = tables()
    _check_orientation(tabs)
    maxt = max(len(t) for t in tabs)
    out = []
    w = out.append
    w("// mc_tables.h -- GENERATED by tools/gen_mc_tables.py; do not edit (tests check it byte for byte).")
    w("//")
    w("// Marching-cubes case tables of csrc/isosurface.hip.")
    w("//   corner c = x + 2y + 4z of the unit cube;  a corner is INSIDE iff value > iso (NaN is outside);")
    w("//   case index = sum over corners of inside(c) << c;")
    w("//   edge 4a + k runs along axis a (0 = x, 1 = y, 2 = z) from corner MC_EDGE_CORNERS[e][0] to")
    w("//   MC_EDGE_CORNERS[e][0] + 2^a; the two other coordinates are the bits of k, lower axis first.")
    w("// Each case's triangles come from the cube-face segments: on every face each maximal run of inside corners gets")
    w("// its own segment (inside corners of an ambiguous face are never connected), so a face's segments depend on its")
    w("// 4 corner signs alone and neighbouring cells join without cracks.  The segments chain into closed loops, each")
    w("// fanned from the first vertex whose diagonals lie in no cube face.  Triangle (a, b, c) has its normal")
    w("// (b - a) x (c - a) pointing from inside to outside.")
    w("#pragma once")
    w("#include <stdint.h>")
    w("")
    w("// storage qualifier of the tables (csrc/isosurface.hip puts them in __constant__ memory)")
    w("#ifndef MC_TABLE_ATTR")
    w("#define MC_TABLE_ATTR")
    w("#endif")
    w("")
    w("#define MC_MAX_TRIS %d" % maxt)
    w("")
    w("static MC_TABLE_ATTR const int8_t MC_EDGE_CORNERS[12][2] = {")
    for e in range(12):
        w("    {%d, %d},%s" % (EDGES[e][0], EDGES[e][1], "  // axis %d" % (e // 4) if e % 4 == 0 else ""))
    w("};")
    w("")
    w("static MC_TABLE_ATTR const uint8_t MC_TRI_COUNT[256] = {")
    for r in range(16):
        w("    " + " ".join("%d," % len(tabs[16 * r + i]) for i in range(16)))
    w("};")
    w("")
    w("// MC_TRIS[case][3 t + j]: edge of corner j of triangle t (-1 past MC_TRI_COUNT[case])")
    w("static MC_TABLE_ATTR const int8_t MC_TRIS[256][%d] = {" % (3 * maxt))
    for c in range(256):
        flat = [e for t in tabs[c] for e in t]
        flat += [-1] * (3 * maxt - len(flat))
        w("    {" + ", ".join("%d" % e for e in flat) + "},  // %d" % c)
    w("};")
    return "\n".join(out) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args(argv)
    text = render_header()
    if args.check:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("mc_tables.h is %s" % ("current" if same else "STALE"))
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main())
