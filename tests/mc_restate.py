"""numpy float32 restatement of ls2fm_marching_cubes_* (csrc/marching_cubes.hip), the checker of the device mesh.

The case table is read from the committed csrc/mc_tables.h; the order and arithmetic are the header's (include/ls2fm.h):
vertices by (owner point's linear index, axis), t = (level - v0) / (v1 - v0), pos = (idx + t [on the edge's axis]) * spacing
+ origin, each operation rounded to float32; faces by (cell linear index, table order)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES_H = os.path.join(ROOT, "level-s2fm_official_amd", "csrc", "mc_tables.h")


def load_tables(path=TABLES_H):
    """(tri_count uint8 [256], tri_edges int8 [256, 3 * max_tris]) as committed"""
    text = open(path).read()
    max_tris = int(re.search(r"#define LS2FM_MC_MAX_TRIS (\d+)", text).group(1))

    def body(name):
        at = text.index(name)
        return text[text.index("{", at): text.index("};", at)]

    def ints(s):
        return [int(v) for v in re.findall(r"-?\d+", re.sub(r"//[^\n]*", "", s))]

    count = np.array(ints(body("kMcTriCount")), dtype=np.uint8)
    edges = np.array(ints(body("kMcTriEdges")), dtype=np.int8).reshape(256, 3 * max_tris)
    assert count.shape == (256,)
    return count, edges


def edge_axis_offset(e):
    """(axis, offset of the owning corner) of cell edge e (mc_tables.h's numbering)"""
    a = e >> 2
    b, c = [x for x in range(3) if x != a]
    o = [0, 0, 0]
    o[b] = e & 1
    o[c] = (e >> 1) & 1
    return a, tuple(o)


def _crossing(vol, level):
    """below [nx, ny, nz] (strict: a NaN is not below) and the crossing mask of every point's owned edges [nx, ny, nz, 3]"""
    below = vol < level
    cross = np.zeros(vol.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = below[:-1] != below[1:]
    cross[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    cross[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    return below, cross


def marching_cubes(vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), tables=None):
    """-> verts float32 [V, 3], faces int32 [F, 3]"""
    count, edges = tables if tables is not None else load_tables()
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    lv = np.float32(level)
    below, cross = _crossing(vol, lv)
    flat = cross.reshape(-1)
    vid = (np.cumsum(flat) - 1).astype(np.int64).reshape(cross.shape)
    # vertices, in (owner linear index, axis) order
    owner_axis = np.nonzero(flat)[0]
    owner, axis = owner_axis // 3, owner_axis % 3
    idx = np.stack(np.unravel_index(owner, vol.shape), axis=1)
    v0 = vol.reshape(-1)[owner]
    step = np.array([ny * nz, nz, 1], dtype=np.int64)
    v1 = vol.reshape(-1)[owner + step[axis]]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (lv - v0) / (v1 - v0)
    sp = np.asarray(spacing, dtype=np.float32)
    og = np.asarray(origin, dtype=np.float32)
    verts = np.empty((len(owner), 3), dtype=np.float32)
    for a in range(3):
        f = idx[:, a].astype(np.float32)
        f = np.where(axis == a, f + t, f).astype(np.float32)
        verts[:, a] = f * sp[a] + og[a]
    # faces, in (cell linear index, table order)
    b = below.astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for q in range(8):
        ox, oy, oz = q & 1, (q >> 1) & 1, (q >> 2) & 1
        case |= b[ox:nx - 1 + ox, oy:ny - 1 + oy, oz:nz - 1 + oz] << q
    cells = np.stack(np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij"), -1).reshape(-1, 3)
    case = case.reshape(-1)
    keep = count[case] > 0
    cells, case = cells[keep], case[keep]
    e = edges[case].astype(np.int64)                                   # [C, 3 * max_tris], -1 padded
    ids = np.full(e.shape, -1, dtype=np.int64)
    for ed in range(12):
        a, o = edge_axis_offset(ed)
        sel = e == ed
        rows = np.nonzero(sel)[0]
        c = cells[rows]
        ids[sel] = vid[c[:, 0] + o[0], c[:, 1] + o[1], c[:, 2] + o[2], a]
    faces = ids[e >= 0].reshape(-1, 3).astype(np.int32)
    return verts, faces


def directed_edges(faces):
    """int64 [3F, 2] directed edges (a, b) of the faces"""
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)


def euler_characteristic(verts, faces):
    d = directed_edges(faces)
    und = np.unique(np.sort(d, axis=1), axis=0)
    used = np.unique(np.asarray(faces).reshape(-1))
    return len(used) - len(und) + len(faces)


def vertex_owners(vol, level=0.0):
    """(owner lattice index int64 [V, 3], axis int64 [V]) of every vertex, in the output order"""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    _, cross = _crossing(vol, np.float32(level))
    owner_axis = np.nonzero(cross.reshape(-1))[0]
    return np.stack(np.unravel_index(owner_axis // 3, vol.shape), axis=1).astype(np.int64), owner_axis % 3


def boundary_planes(vol, level=0.0):
    """bool [V, 6]: vertex lies on the volume's boundary plane (axis d, low / high side)"""
    idx, axis = vertex_owners(vol, level)
    out = np.zeros((len(idx), 6), dtype=bool)
    for d in range(3):
        out[:, 2 * d] = (idx[:, d] == 0) & (axis != d)
        out[:, 2 * d + 1] = idx[:, d] == vol.shape[d] - 1
    return out
