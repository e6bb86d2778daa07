"""CPU checks of mesh extraction: the generated marching-cubes case table (csrc/mc_tables.h, tools/gen_mc_tables.py), the numpy
restatement of the device kernels (tests/mc_restate.py) on random and structured volumes, the PLY writer, and the host-side
refusals of ls2fm.mesh / ls2fm_marching_cubes_*."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import mc_restate as R
from conftest import ROOT
from ls2fm import _lib, mesh


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "tools", "gen_mc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CORNER = [(q & 1, (q >> 1) & 1, (q >> 2) & 1) for q in range(8)]


def _edge_corners(e):
    a, o = R.edge_axis_offset(e)
    hi = list(o)
    hi[a] = 1
    return CORNER.index(o), CORNER.index(tuple(hi))


def _faces():
    """(axis, side, corners, edges) of the 6 cube faces"""
    return [(d, s, [q for q in range(8) if CORNER[q][d] == s],
             [e for e in range(12) if R.edge_axis_offset(e)[0] != d and R.edge_axis_offset(e)[1][d] == s])
            for d in range(3) for s in (0, 1)]


def _crossing(case, e):
    q0, q1 = _edge_corners(e)
    return ((case >> q0) & 1) != ((case >> q1) & 1)


def _face_rule(case, face):
    """the unoriented segments of the face rule: 2 crossing edges -> one segment; 4 -> each below corner cut off on its own"""
    _, _, corners, edges = face
    cross = [e for e in edges if _crossing(case, e)]
    if len(cross) == 2:
        return {frozenset(cross)}
    if len(cross) == 4:
        return {frozenset(e for e in cross if q in _edge_corners(e)) for q in corners if (case >> q) & 1}
    assert not cross
    return set()


def _triangles(count, edges, case):
    return [tuple(int(v) for v in edges[case, 3 * t:3 * t + 3]) for t in range(int(count[case]))]


def _boundary(tris):
    """directed edges of the triangle set whose reverse is not in it; asserts no directed edge repeats"""
    d = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(d)) == len(d)
    return {x for x in d if (x[1], x[0]) not in set(d)}, d


def test_generator_reproduces_the_committed_header(tmp_path):
    out = tmp_path / "mc_tables.h"
    _generator().main(["gen_mc_tables.py", str(out)])
    committed = open(R.TABLES_H, "rb").read()
    assert out.read_bytes() == committed


def test_case_table_properties():
    count, edges = R.load_tables()
    max_tris = edges.shape[1] // 3
    assert count.max() == max_tris and count[0] == 0 and count[255] == 0
    faces = _faces()
    for case in range(256):
        tris = _triangles(count, edges, case)
        assert (edges[case, 3 * len(tris):] == -1).all()
        used = {e for t in tris for e in t}
        assert used == {e for e in range(12) if _crossing(case, e)}, case          # only crossing edges, and all of them
        assert all(len(set(t)) == 3 for t in tris), case
        bnd, d = _boundary(tris)
        # the boundary is exactly the face rule's segments, each on its face
        on_face = {}
        for p, q in bnd:
            hits = [i for i, f in enumerate(faces) if p in f[3] and q in f[3]]
            assert len(hits) == 1, (case, p, q)
            on_face.setdefault(hits[0], set()).add(frozenset((p, q)))
        for i, f in enumerate(faces):
            assert on_face.get(i, set()) == _face_rule(case, f), (case, f[:2])
        # edges inside the cell appear once in each direction
        inner = [x for x in d if x not in bnd]
        assert all(inner.count((x[1], x[0])) == 1 for x in inner), case
        # and none lies inside a face (the neighbour could draw the same one)
        assert not any(p in f[3] and q in f[3] for p, q in inner for f in faces), case


def _mirror_edge(e, d):
    """the same lattice edge seen from the neighbour across the face normal to axis d (offset along d flipped)"""
    a, o = R.edge_axis_offset(e)
    o2 = list(o)
    o2[d] ^= 1
    for f in range(12):
        if R.edge_axis_offset(f) == (a, tuple(o2)):
            return f
    raise AssertionError


def test_shared_faces_cancel_between_neighbours():
    """cell A's high face along d is cell B's low face: for every A and every B agreeing on that face's corners, B's boundary
    segments there are A's, reversed"""
    count, edges = R.load_tables()
    faces = _faces()
    for a_case in range(256):
        a_bnd, _ = _boundary(_triangles(count, edges, a_case))
        for d in range(3):
            hi_face = faces[2 * d + 1]
            shared = 0
            for q in hi_face[2]:
                q_low = CORNER.index(tuple(c ^ (1 if x == d else 0) for x, c in enumerate(CORNER[q])))
                shared |= ((a_case >> q) & 1) << q_low
            a_seg = {(p, q) for p, q in a_bnd if p in hi_face[3] and q in hi_face[3]}
            for rest in range(16):
                b_case = shared
                for bit, q in enumerate(faces[2 * d + 1][2]):           # B's far corners: all 16 choices
                    b_case |= ((rest >> bit) & 1) << q
                b_bnd, _ = _boundary(_triangles(count, edges, b_case))
                lo = faces[2 * d][3]
                b_seg = {(p, q) for p, q in b_bnd if p in lo and q in lo}
                assert b_seg == {(_mirror_edge(q, d), _mirror_edge(p, d)) for p, q in a_seg}, (a_case, d, b_case)


def _sphere(shape, r, centre=None, spacing=1.0):
    axes = [np.arange(n, dtype=np.float64) * spacing for n in shape]
    c = [(n - 1) * spacing / 2 for n in shape] if centre is None else centre
    x, y, z = np.meshgrid(*axes, indexing="ij")
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)


def _torus(shape, R_, r):
    axes = [np.arange(n, dtype=np.float64) - (n - 1) / 2 for n in shape]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    return (np.sqrt((np.sqrt(x ** 2 + y ** 2) - R_) ** 2 + z ** 2) - r).astype(np.float32)


def _volumes():
    rng = np.random.default_rng(7)
    i, j, k = np.meshgrid(np.arange(7), np.arange(8), np.arange(9), indexing="ij")
    return {
        "noise_9x10x11": (rng.standard_normal((9, 10, 11)).astype(np.float32), 0.0),
        "checkerboard": (np.where((i + j + k) % 2 == 0, 1.0, -1.0).astype(np.float32), 0.0),
        "checker_2x2x2": (np.where((i + j) % 2 == 0, 1.0, -1.0)[:2, :2, :2].astype(np.float32), 0.0),
        "exact_level": (rng.integers(-1, 2, (8, 9, 10)).astype(np.float32), 0.0),
        "exact_level_0.5": (rng.integers(0, 3, (6, 7, 5)).astype(np.float32) * np.float32(0.5), 0.5),
        "sphere_level": (_sphere((12, 13, 14), 0.0), 4.2),
    }


def _check_watertight(vol, level, verts, faces):
    """every mesh edge not on the volume's boundary is used by exactly two faces, once in each direction"""
    d = R.directed_edges(faces)
    key = d[:, 0] * (len(verts) + 1) + d[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge repeats"
    rev = d[:, 1] * (len(verts) + 1) + d[:, 0]
    missing = ~np.isin(rev, key)
    on_plane = R.boundary_planes(vol, level)
    on_boundary = (on_plane[d[:, 0]] & on_plane[d[:, 1]]).any(axis=1)
    assert not (missing & ~on_boundary).any(), d[missing & ~on_boundary][:5]


@pytest.mark.parametrize("name", list(_volumes()))
def test_restatement_mesh_is_closed_and_oriented(name):
    vol, level = _volumes()[name]
    verts, faces = R.marching_cubes(vol, level)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and len(faces) > 0
    assert faces.min() >= 0 and faces.max() < len(verts)
    assert len(np.unique(faces)) == len(verts)                          # every vertex is used
    _check_watertight(vol, level, verts, faces)


def test_restatement_euler_characteristic_and_volume():
    vol = _sphere((32, 32, 32), 11.3)
    verts, faces = R.marching_cubes(vol)
    _check_watertight(vol, 0.0, verts, faces)
    assert R.euler_characteristic(verts, faces) == 2
    p = verts[faces.astype(np.int64)].astype(np.float64)
    signed = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6
    assert abs(signed / (4 / 3 * np.pi * 11.3 ** 3) - 1) < 0.02                 # outward normals: positive volume
    vol = _torus((32, 36, 20), 9.0, 3.5)
    verts, faces = R.marching_cubes(vol)
    _check_watertight(vol, 0.0, verts, faces)
    assert R.euler_characteristic(verts, faces) == 0


def test_restatement_vertices_follow_the_documented_arithmetic():
    vol = np.random.default_rng(3).standard_normal((5, 6, 7)).astype(np.float32)
    sp, og = (0.25, 0.5, 2.0), (-1.0, 0.125, 3.0)
    verts, _ = R.marching_cubes(vol, 0.1, sp, og)
    idx, axis = R.vertex_owners(vol, 0.1)
    for n in range(0, len(verts), 17):
        i = tuple(idx[n])
        j = list(i)
        j[axis[n]] += 1
        v0, v1 = vol[i], vol[tuple(j)]
        t = (np.float32(0.1) - v0) / (v1 - v0)
        for a in range(3):
            f = np.float32(i[a]) + (t if a == axis[n] else np.float32(0))
            assert verts[n, a] == np.float32(np.float32(f) * np.float32(sp[a])) + np.float32(og[a])


def test_all_above_and_all_below_give_empty_meshes():
    for v in (np.ones((4, 5, 6), np.float32), -np.ones((3, 3, 3), np.float32)):
        verts, faces = R.marching_cubes(v)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_write_ply_round_trip(tmp_path):
    vol = _sphere((10, 11, 12), 3.7)
    verts, faces = R.marching_cubes(vol, 0.0, (0.1, 0.2, 0.3), (-1.0, -2.0, -3.0))
    path = tmp_path / "mesh.ply"
    mesh.write_ply(str(path), torch.from_numpy(verts), torch.from_numpy(faces))
    data = path.read_bytes()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces))).encode()
    assert data.startswith(header) and len(data) == len(header) + 12 * len(verts) + 13 * len(faces)
    v2, f2 = mesh.read_ply(str(path))
    assert np.array_equal(v2, verts) and np.array_equal(f2, faces)
    mesh.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v3, f3 = mesh.read_ply(str(tmp_path / "empty.ply"))
    assert v3.shape == (0, 3) and f3.shape == (0, 3)
    try:
        import plyfile
    except ImportError:
        pytest.skip("plyfile is not installed: the file was checked against the writer's own layout only")
    ply = plyfile.PlyData.read(str(path))
    assert np.array_equal(np.stack([ply["vertex"][c] for c in "xyz"], 1), verts)
    assert np.array_equal(np.stack(ply["face"]["vertex_indices"]), faces)


def test_cpu_volume_is_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.marching_cubes(torch.zeros(4, 4, 4))


def test_workspace_size_refuses_what_int32_vertex_ids_cannot_index():
    lib = _lib.load()
    ws = lib.ls2fm_marching_cubes_workspace_bytes
    assert ws(512, 512, 512) >= 5 * 512 ** 3
    assert ws(2, 2, 2) > 0
    for dims in ((1024, 1024, 1024), (1, 8, 8), (8, 8, 1), (0, 4, 4), (-3, 4, 4), (1 << 40, 1 << 40, 1 << 40),
                 (1 << 31, 2, 2), (2, 1 << 20, 1 << 20), (1 << 29, 2, 2)):
        assert ws(*dims) == -1, dims
    assert ws(1 << 26, 2, 2) > 0 and ws((1 << 28) // 3, 2, 2) > 0                 # 3 n < 2^31 is the bound
    # refused before anything is enqueued (NULL buffers: nothing could be written)
    null = ctypes.c_void_p(0)
    assert lib.ls2fm_marching_cubes_count(null, 1, 4, 4, 0.0, null, null, null) == -1
    assert lib.ls2fm_marching_cubes_emit(null, 1024, 1024, 1024, 0.0, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), null, null,
                                         null, null) == -1
