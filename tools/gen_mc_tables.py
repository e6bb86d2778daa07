#!/usr/bin/env python3
"""Generate level-s2fm_official_amd/csrc/mc_tables.h: the marching-cubes case table of ls2fm_marching_cubes_*.

The table is derived from one rule rather than typed in, so that the extracted mesh is crack-free by construction:

  corner q of a cell sits at offset (q & 1, q >> 1 & 1, q >> 2 & 1) along (axis 0, axis 1, axis 2); corner q is BELOW iff its
  value < level (strict: a NaN is not below); case bit q = below(q).  Edge e runs along axis a = e >> 2 from the corner whose
  offsets along the two other axes (b < c) are (e & 1, e >> 1 & 1) and 0 along a; it CROSSES iff exactly one end is below.

  face rule: on each of the 6 faces, the crossing edges (0, 2 or 4) are joined into segments -- 2 edges: one segment; 4 edges
  (an ambiguous face): each below corner is cut off on its own (the above corners stay connected across the face).  The rule
  reads only the face's 4 corners, so two cells sharing a face produce the same segments on it.  Each segment is oriented so
  that (outward face normal) x (segment direction) points, within the face, to the above side; the neighbour across the face
  has the opposite normal and walks the segment the other way, so shared boundaries cancel.

  loops: the oriented segments close into loops on the cube surface (every crossing edge has one segment in, one out); each loop
  is fan-triangulated from its first edge (in loop order from its smallest) whose fan draws no diagonal between two edges of one
  face, and right-hand triangle normals then point to the above side (increasing values).

This is simpler than scikit-image's Lewiner tables (asymptotic decider, MC33): topology in ambiguous cells may differ.

  python tools/gen_mc_tables.py [out.h]          (default: the committed header)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, "level-s2fm_official_amd", "csrc", "mc_tables.h")


def corner_offset(q):
    return (q & 1, (q >> 1) & 1, (q >> 2) & 1)


def corner_index(o):
    return o[0] | (o[1] << 1) | (o[2] << 2)


def edge_axis_offset(e):
    """(axis, offset of the lower end) of edge e"""
    a = e >> 2
    b, c = [x for x in range(3) if x != a]
    o = [0, 0, 0]
    o[b] = e & 1
    o[c] = (e >> 1) & 1
    return a, tuple(o)


def edge_corners(e):
    a, o = edge_axis_offset(e)
    hi = list(o)
    hi[a] = 1
    return corner_index(o), corner_index(hi)


def faces():
    """the 6 faces as (axis d, side s, corners, edges): the face's 4 corners have offset s along d"""
    out = []
    for d in range(3):
        for s in (0, 1):
            corners = [q for q in range(8) if corner_offset(q)[d] == s]
            edges = [e for e in range(12) if edge_axis_offset(e)[0] != d and edge_axis_offset(e)[1][d] == s]
            out.append((d, s, corners, edges))
    return out


def _mid(e):
    a, o = edge_axis_offset(e)
    return [o[x] + (0.5 if x == a else 0.0) for x in range(3)]


def _sub(u, v):
    return [u[i] - v[i] for i in range(3)]


def _det(u, v, w):
    return (u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0]))


def crossing(case, e):
    q0, q1 = edge_corners(e)
    return ((case >> q0) & 1) != ((case >> q1) & 1)


def face_segments(case, face):
    """the face rule: oriented segments (edge_from, edge_to) of one face"""
    d, s, corners, edges = face
    below = [q for q in corners if (case >> q) & 1]
    above = [q for q in corners if not (case >> q) & 1]
    cross = [e for e in edges if crossing(case, e)]
    if not cross:
        return []
    if len(cross) == 2:
        pairs = [(cross[0], cross[1])]
        mb = [sum(corner_offset(q)[x] for q in below) / len(below) for x in range(3)]
        ma = [sum(corner_offset(q)[x] for q in above) / len(above) for x in range(3)]
        sides = [_sub(ma, mb)]
    else:
        assert len(cross) == 4, (case, face)
        pairs, sides = [], []
        centre = [0.5 if x != d else float(s) for x in range(3)]
        for q in below:                       # cut each below corner off on its own
            pairs.append(tuple(e for e in cross if q in edge_corners(e)))
            sides.append(_sub(centre, list(corner_offset(q))))
    n = [0.0, 0.0, 0.0]
    n[d] = 1.0 if s else -1.0
    out = []
    for (p, q), u in zip(pairs, sides):
        det = _det(n, _sub(_mid(q), _mid(p)), u)
        assert det != 0.0, (case, face, p, q)
        out.append((p, q) if det > 0 else (q, p))
    return out


def case_triangles(case):
    """the triangles (edge triples) of one case, in table order"""
    nxt = {}
    for face in faces():
        for p, q in face_segments(case, face):
            assert p not in nxt, (case, p)   # one segment out of every crossing edge ...
            nxt[p] = q
    cross = [e for e in range(12) if crossing(case, e)]
    assert sorted(nxt) == cross and sorted(nxt.values()) == cross, case      # ... and one in
    tris, seen = [], set()
    for start in cross:
        if start in seen:
            continue
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        assert len(loop) >= 3, (case, loop)
        apex = next(k for k in range(len(loop)) if fan_ok(loop, k))
        loop = loop[apex:] + loop[:apex]
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


def share_face(p, q):
    return any(p in f[3] and q in f[3] for f in faces())


def fan_ok(loop, k):
    """no diagonal of the fan from loop[k] joins two edges of one face: such a diagonal lies IN the face (an ambiguous one, where
    the loop passes both segments), and the neighbour across it could draw the same one -- four triangles on one mesh edge"""
    m = len(loop)
    return all(not share_face(loop[k], loop[(k + i) % m]) for i in range(2, m - 1))


def tables():
    tris = [case_triangles(c) for c in range(256)]
    max_tris = max(len(t) for t in tris)
    # a loop through m edges gives m - 2 triangles; the rule's worst case is 5 (a 7-edge loop, or a hexagon plus a corner)
    assert max_tris == 5, max_tris
    assert len(tris[0]) == 0 and len(tris[255]) == 0
    return tris, max_tris


def render():
    tris, max_tris = tables()
    w = max_tris * 3
    lines = [
        "// GENERATED by tools/gen_mc_tables.py -- do not edit; re-run the generator (tests/test_mesh_tables.py checks the two agree).",
        "//",
        "// Marching-cubes case table of ls2fm_marching_cubes_* (marching_cubes.hip), derived from one rule:",
        "//   corner q at offset (q & 1, q >> 1 & 1, q >> 2 & 1) along (axis 0, axis 1, axis 2); case bit q = (value_q < level)",
        "//   (strict: a NaN is not below).  Edge e runs along axis a = e >> 2 from the corner with offsets (e & 1, e >> 1 & 1)",
        "//   along the two other axes in increasing order; it crosses iff exactly one end is below.",
        "//   Face rule: on each cube face the crossing edges are joined into segments -- 2 edges: one segment; 4 edges (ambiguous",
        "//   face): each below corner is cut off on its own.  The rule reads only the face's 4 corners, so cells sharing a face",
        "//   produce the same segments there, oriented oppositely: the mesh is crack-free by construction.  The segments close",
        "//   into loops, oriented so right-hand triangle normals point to the above side (increasing values), fan-triangulated",
        "//   from the first edge (in loop order from the smallest) whose fan puts no diagonal inside a face: every mesh edge off",
        "//   the volume's boundary then has exactly two triangles.",
        "//   This is deliberately simpler than scikit-image's Lewiner tables (asymptotic decider / MC33): the topology inside",
        "//   ambiguous cells may differ from theirs.",
        "#pragma once",
        "",
        "#include <stdint.h>",
        "",
        f"#define LS2FM_MC_MAX_TRIS {max_tris}",
        "",
        "// number of triangles of each case",
        "static __constant__ uint8_t kMcTriCount[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tris[r:r + 32]) + ",")
    lines += ["};", "", "// edges of each case's triangles (3 per triangle, -1 past the last)",
              f"static __constant__ int8_t kMcTriEdges[256][{w}] = {{"]
    for c, t in enumerate(tris):
        flat = [e for tri in t for e in tri] + [-1] * (w - 3 * len(t))
        lines.append("    {" + ", ".join(str(v) for v in flat) + f"}},  // {c}")
    lines += ["};", ""]
    return "\n".join(lines)


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    text = render()
    with open(out, "w", newline="\n") as f:
        f.write(text)
    print(f"wrote {out} (max {tables()[1]} triangles per case)")


if __name__ == "__main__":
    main(sys.argv)
