"""The meshes the simplification tests share (tests/test_simplify_host.py on the restatement, tests/test_hip_simplify.py on the
kernels): marching-cubes meshes of analytic fields (tests/mc_restate.py) in voxel units, and hand-made meshes that meet the edges of
THE CLUSTERING RULE.  Every scene is a dict: verts float32 [V, 3], faces int32 [F, 3], cell, and colors float32 [V, C] or None."""
import functools

import numpy as np

import mc_restate

F32 = np.float32
THREADS = 256                    # the workgroup of csrc/mesh_simplify.hip's kernels
CELLS_PER_WORKGROUP = 4          # simplify_sums: one wave per output cell
OFF = np.array([0.37, -0.21, 0.13])


def _lattice(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def scene(verts, faces, cell, colors=None):
    return dict(verts=np.ascontiguousarray(verts, F32).reshape(-1, 3), faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3),
                cell=float(F32(cell)), colors=None if colors is None else np.ascontiguousarray(colors, F32))


@functools.lru_cache(maxsize=None)
def sphere_mesh(n, radius):
    """marching cubes of |x - c| - radius on an n^3 lattice of unit voxels, c off the lattice -> (verts, faces, c)"""
    c = (n - 1) / 2.0 + OFF
    x, y, z = _lattice((n, n, n))
    vol = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius
    v, f = mc_restate.marching_cubes(vol.astype(F32), 0.0)
    return v, f, c


@functools.lru_cache(maxsize=None)
def box_mesh(shape, half):
    """marching cubes of the max-norm box max_a(|x_a - c_a| - half_a), its faces off the lattice planes -> (verts, faces, c, half)"""
    c = (np.array(shape) - 1) / 2.0 + OFF
    h = np.array(half, dtype=np.float64)
    x = _lattice(shape)
    vol = np.maximum(np.maximum(np.abs(x[0] - c[0]) - h[0], np.abs(x[1] - c[1]) - h[1]), np.abs(x[2] - c[2]) - h[2])
    v, f = mc_restate.marching_cubes(vol.astype(F32), 0.0)
    return v, f, c, h


def box_distance(p, c, h):
    """distance of points p [n, 3] to the surface of the box |x - c| <= h"""
    q = np.abs(np.asarray(p, np.float64) - c) - h
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=1))
    inside = np.minimum(q.max(axis=1), 0.0)
    return np.abs(outside + inside)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def soup(seed=0, n_verts=300, n_faces=520, channels=3, cell=0.8):
    """random triangles over [-3, 3]^3: negative coordinates, vertices no face uses, a NaN and an inf vertex and faces on them, faces
    with a repeated index, an exact, a rotated and an opposite-oriented copy of earlier faces, vertices exactly on cell faces"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-3.0, 3.0, (n_verts, 3)).astype(F32)
    v[::17] = (np.round(v[::17] / cell) * F32(cell)).astype(F32)            # on the lattice planes: the floor decides
    v[5, 1] = np.nan
    v[11, 2] = np.inf
    v[12, 0] = -np.inf
    used = n_verts - 20                                                      # the last 20 vertices are in no face
    f = rng.integers(0, used, (n_faces, 3)).astype(np.int32)
    f[3] = (7, 7, 9)                                                         # repeated index
    f[4] = (8, 20, 8)
    f[10] = (5, 30, 31)                                                      # on the NaN vertex
    f[13] = (40, 11, 41)                                                     # on the inf vertex
    f[100] = f[50]                                                           # exact copy
    f[101] = f[51][[1, 2, 0]]                                                # rotated copy
    f[102] = f[52][[0, 2, 1]]                                                # opposite orientation: stays
    f[103] = f[52][[2, 1, 0]]                                                # the same opposite triangle, rotated: goes
    colors = None if not channels else rng.uniform(0.0, 1.0, (n_verts, channels)).astype(F32)
    return scene(v, f, cell, colors)


SEGMENT_LENGTHS = (1, 63, 64, 65, 300)


def segments(seed=1, lengths=SEGMENT_LENGTHS):
    """per length L one hub vertex alone in its cell and L faces (hub, a_i, b_i), the a_i in one neighbouring cell and the b_i in
    another: the hub cell's corner segment is L long, the two others' vertex and corner segments are L long"""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for j, n in enumerate(lengths):
        base = np.array([10.0 * j - 20.0, 0.0, 0.0])
        hub = len(verts)
        verts.append(base + 0.5 + rng.uniform(-0.3, 0.3, 3))
        for _ in range(n):
            a, b = len(verts), len(verts) + 1
            verts.append(base + [1.0, 0.0, 0.0] + rng.uniform(0.05, 0.95, 3))
            verts.append(base + [0.0, 1.0, 0.0] + rng.uniform(0.05, 0.95, 3))
            faces.append((hub, a, b))
    return scene(np.array(verts), np.array(faces), 1.0)


def sized(n_verts, n_faces, seed=2, channels=0):
    """a soup with exactly these counts (around a workgroup multiple)"""
    rng = np.random.default_rng(seed + 7 * n_verts + n_faces)
    v = rng.uniform(-2.0, 2.0, (n_verts, 3)).astype(F32)
    f = rng.integers(0, n_verts, (n_faces, 3)).astype(np.int32)
    colors = None if not channels else rng.uniform(0.0, 1.0, (n_verts, channels)).astype(F32)
    return scene(v, f, 0.7, colors)


def sheet(n=150):
    """a wavy n x n height field at unit spacing, cell 1: about one output cell per vertex -- n^2 of them, more than the first wave
    of workgroups of a launch that gives a workgroup CELLS_PER_WORKGROUP cells"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i + 0.5, j + 0.5, 0.5 + 0.3 * np.sin(0.31 * i) * np.cos(0.23 * j)], axis=-1).reshape(-1, 3)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + 1], axis=1), np.stack([a + 1, a + n, a + n + 1], axis=1)])
    return scene(v, f, 1.0)


def one_cell():
    """a mesh inside one cell: nothing survives"""
    rng = np.random.default_rng(5)
    return scene(rng.uniform(0.1, 0.9, (12, 3)), rng.integers(0, 12, (9, 3)), 1.0)


def extreme_cells(cell=0.8):
    """vertices in the lattice's last cell on all three axes (key 2^63 - 1, the largest a valid vertex can have), in its first
    (key 0) and beside them: one face among the top cells, one across the whole lattice"""
    c = float(F32(cell))
    top, low = (2.0 ** 20 - 0.5) * c, (-2.0 ** 20 + 0.5) * c
    v = np.array([[top, top, top], [top - c, top, top], [top, top - c, top], [low, low, low], [top, top, top - c]])
    return scene(v, [[0, 1, 2], [3, 0, 4], [0, 2, 1]], cell)


def gpu_scenes():
    """name -> scene: the smallest shapes at which the kernels can still go wrong"""
    v, f, _ = sphere_mesh(24, 8.3)
    bv, bf, _, _ = box_mesh((20, 18, 22), (5.3, 4.6, 6.2))
    rng = np.random.default_rng(9)
    out = {
        "sphere_2.5": scene(v, f, 2.5),
        "sphere_dyadic_2": scene(v, f, 2.0),                  # marching-cubes vertices sit exactly on cell faces
        "box": scene(bv, bf, 2.5, rng.uniform(0.0, 1.0, (len(bv), 4))),
        "soup_c3": soup(channels=3),
        "soup_c1": soup(seed=3, channels=1),
        "segments": segments(),
        "sheet": sheet(),
        "no_faces": scene(rng.uniform(-1, 1, (7, 3)), np.zeros((0, 3)), 0.5),
        "one_face": scene([[0.1, 0.1, 0.1], [1.2, 0.1, 0.1], [0.1, 1.3, 0.1]], [[0, 1, 2]], 1.0, [[0.25], [0.5], [1.0]]),
        "one_cell": one_cell(),
        "empty": scene(np.zeros((0, 3)), np.zeros((0, 3)), 1.0),
        "extreme_cells": extreme_cells(),
    }
    for nv in (THREADS - 1, THREADS, THREADS + 1):
        nf = 2 * THREADS + (nv - THREADS)
        out[f"sized_{nv}_{nf}"] = sized(nv, nf, channels=4 if nv == THREADS else 0)
    return out
