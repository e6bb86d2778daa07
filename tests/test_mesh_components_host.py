"""CPU checks of the mesh-components ABI (include/ls2fm.h, ABI 13), of the vertex-adjacency rule on marching-cubes meshes, of
the ASCII PLY layout and of the surface-sampling restatement.  No device work: every library call here is refused before
anything is enqueued."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mc_restate as R
import mesh_restate as M
from conftest import ROOT
from ls2fm import _lib, mesh

NEW = ("ls2fm_mesh_components_workspace_bytes", "ls2fm_mesh_components", "ls2fm_mesh_largest_component_count",
       "ls2fm_mesh_largest_component_emit")
ERR_ARG, ERR_WS = -1, -4
FAKE = ctypes.c_void_p(0x1000)          # never dereferenced: every call below is refused first
NULL = ctypes.c_void_p(0)


def test_header_binding_and_library_agree_on_the_new_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    declared = set(re.findall(r"\b(ls2fm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert int(re.search(r"#define\s+LS2FM_ABI_VERSION\s+(\d+)", header).group(1)) == 13
    assert lib.ls2fm_abi_version() == _lib.ABI_VERSION == 13


def test_workspace_query():
    lib = _lib.load()
    assert lib.ls2fm_mesh_components_workspace_bytes(0, 0) >= 0
    small = lib.ls2fm_mesh_components_workspace_bytes(10, 8)
    big = lib.ls2fm_mesh_components_workspace_bytes(1 << 20, 1 << 21)
    assert 0 < small < big and big >= 20 * (1 << 20)
    for nv, nf in ((-1, 0), (0, -1), (1 << 31, 4), (4, 1 << 31), (0, 1)):
        assert lib.ls2fm_mesh_components_workspace_bytes(nv, nf) == ERR_ARG, (nv, nf)


def test_components_refusals_enqueue_nothing():
    lib = _lib.load()
    assert lib.ls2fm_mesh_components(NULL, 4, 2, FAKE, NULL) == ERR_ARG          # faces NULL
    assert lib.ls2fm_mesh_components(FAKE, 4, 2, NULL, NULL) == ERR_ARG          # labels NULL
    assert lib.ls2fm_mesh_components(FAKE, -1, 2, FAKE, NULL) == ERR_ARG
    assert lib.ls2fm_mesh_components(FAKE, 4, -2, FAKE, NULL) == ERR_ARG
    assert lib.ls2fm_mesh_components(FAKE, 1 << 31, 2, FAKE, NULL) == ERR_ARG
    assert lib.ls2fm_mesh_components(FAKE, 4, 1 << 31, FAKE, NULL) == ERR_ARG
    assert lib.ls2fm_mesh_components(FAKE, 0, 2, FAKE, NULL) == ERR_ARG          # faces without vertices
    assert lib.ls2fm_mesh_components(NULL, 0, 0, NULL, NULL) == 0                # nothing to do, nothing enqueued


def test_largest_component_refusals_enqueue_nothing():
    lib = _lib.load()
    ws = lib.ls2fm_mesh_components_workspace_bytes(4, 2)
    count, emit = lib.ls2fm_mesh_largest_component_count, lib.ls2fm_mesh_largest_component_emit
    for call, last in ((count, (FAKE, NULL)), (emit, (FAKE, FAKE))):
        args = lambda v=FAKE, nv=4, f=FAKE, nf=2, w=FAKE, wb=ws, o=last: (v, nv, f, nf, w, wb, *o, NULL)  # noqa: E731
        assert call(*args(v=NULL)) == ERR_ARG
        assert call(*args(f=NULL)) == ERR_ARG
        assert call(*args(nv=-1)) == ERR_ARG
        assert call(*args(nf=-1)) == ERR_ARG
        assert call(*args(nv=1 << 31)) == ERR_ARG
        assert call(*args(nf=1 << 31)) == ERR_ARG
        assert call(*args(w=NULL)) == ERR_WS
        assert call(*args(wb=ws - 1)) == ERR_WS
        assert call(*args(v=NULL, f=NULL, nf=0, w=NULL, wb=0, o=(NULL, NULL))) == 0      # F = 0: empty, nothing enqueued
    assert count(FAKE, 4, FAKE, 2, FAKE, ws, NULL, NULL, NULL) == ERR_ARG                # counts NULL
    assert emit(FAKE, 4, FAKE, 2, FAKE, ws, NULL, FAKE, NULL) == ERR_ARG                  # out_verts NULL
    assert emit(FAKE, 4, FAKE, 2, FAKE, ws, FAKE, NULL, NULL) == ERR_ARG                  # out_faces NULL


def test_python_wrappers_refuse_cpu_tensors():
    v = torch.zeros(3, 3)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        mesh.connected_components(f, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        mesh.largest_component(v, f)
    with pytest.raises(RuntimeError, match="GPU only"):
        mesh.sample_surface(v, f, 10)


def _sphere(shape, r, centre):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (np.sqrt(sum((x - c) ** 2 for x, c in zip(g, centre))) - r).astype(np.float32)


def _torus(shape, big, small):
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2 for n in shape], indexing="ij")
    return (np.sqrt((np.sqrt(x * x + y * y) - big) ** 2 + z * z) - small).astype(np.float32)


def _volumes():
    rng = np.random.default_rng(5)
    spheres = np.minimum(np.minimum(_sphere((40, 36, 44), 9.3, (12.2, 11.7, 13.1)), _sphere((40, 36, 44), 5.1, (29.4, 24.2, 30.6))),
                         _sphere((40, 36, 44), 2.6, (30.1, 8.3, 9.2)))
    return {
        "sphere": _sphere((33, 33, 33), 12.4, (16, 16, 16)),
        "three_spheres": spheres,
        "torus": _torus((40, 48, 56), 14.0, 5.5),
        "noise_24": rng.standard_normal((24, 24, 24)).astype(np.float32),
        "noise_31x17x23": rng.standard_normal((31, 17, 23)).astype(np.float32),
        "smooth_noise": (rng.standard_normal((30, 30, 30)).cumsum(0).cumsum(1) * 0.1).astype(np.float32),
    }


@pytest.mark.parametrize("name", list(_volumes()))
def test_vertex_adjacency_equals_edge_adjacency_on_marching_cubes_meshes(name):
    """the face rule draws the same segment on a cube face from both sides, so the faces around each lattice edge form one
    edge-connected fan: joining faces through shared vertices gives trimesh's edge-connected split"""
    verts, faces = R.marching_cubes(_volumes()[name])
    assert len(faces) > 0
    by_vertex = M.components(faces, len(verts))[faces[:, 0].astype(np.int64)]
    by_edge = M.face_components_by_edges(faces)
    # same partition of the faces: each vertex-component holds exactly one edge-component and vice versa
    pairs = np.unique(np.stack([by_vertex, by_edge], 1), axis=0)
    assert len(pairs) == len(np.unique(by_vertex)) == len(np.unique(by_edge))
    if name.startswith("noise"):
        assert len(np.unique(by_edge)) > 10                  # many components, many ambiguous cells


def test_restated_labels_are_the_smallest_vertex_index():
    faces = np.array([[5, 3, 7], [7, 9, 8], [1, 2, 4], [0, 6, 6]])
    labels = M.components(faces, 11)
    assert labels.tolist() == [0, 1, 1, 3, 1, 3, 0, 3, 3, 3, 10]


def test_ascii_ply_round_trip_and_binary_bytes_unchanged(tmp_path):
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((257, 3)) * 10.0 ** rng.integers(-20, 20, (257, 3))).astype(np.float32)
    v[:4] = [[0.0, -0.0, 1.0], [np.float32(1) / 3, 1e-38, 3.4e38], [np.nextafter(np.float32(1), np.float32(2)), -1.5, 2.0],
             [np.float32(0.1), np.float32(0.2), np.float32(0.3)]]
    f = rng.integers(0, 257, (300, 3)).astype(np.int32)
    p = str(tmp_path / "a.ply")
    mesh.write_ply(p, v, f, encoding="ascii")
    data = open(p, "rb").read()
    assert data.startswith(b"ply\nformat ascii 1.0\nelement vertex 257\nproperty float x\nproperty float y\nproperty float z\n"
                           b"element face 300\nproperty list uchar int vertex_indices\nend_header\n")
    body = data.split(b"end_header\n", 1)[1].decode().splitlines()
    assert len(body) == 557 and body[257] == "3 %d %d %d" % tuple(f[0])
    rv, rf = mesh.read_ply_ascii(p)
    assert np.array_equal(rv.view(np.uint32), v.view(np.uint32)) and np.array_equal(rf, f)
    # empty mesh
    mesh.write_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), encoding="ascii")
    ev, ef = mesh.read_ply_ascii(p)
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    # binary: the default and encoding="binary" write the same bytes, the layout extract_mesh has always written
    b1, b2 = str(tmp_path / "b1.ply"), str(tmp_path / "b2.ply")
    mesh.write_ply(b1, v, f)
    mesh.write_ply(b2, v, f, encoding="binary")
    rows = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    rows["n"], rows["idx"] = 3, f
    want = mesh.ply_header(len(v), len(f)) + v.astype("<f4").tobytes() + rows.tobytes()
    assert open(b1, "rb").read() == open(b2, "rb").read() == want
    with pytest.raises(ValueError):
        mesh.read_ply_ascii(b1)
    with pytest.raises(ValueError):
        mesh.write_ply(p, v, f, encoding="utf8")


def _two_triangles():
    v = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2.0, 3.0, 1.5]], dtype=np.float32)
    f = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    return v, f


def test_sampling_restatement_matches_trimesh_formula_by_hand():
    v, f = _two_triangles()
    a0 = 0.5 * np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0]).astype(np.float64))
    a1 = 0.5 * np.linalg.norm(np.cross((v[3] - v[1]).astype(np.float64), (v[2] - v[1]).astype(np.float64)))
    total = a0 + a1
    u0 = np.array([0.0, 0.1, a0 / total * 0.999, a0 / total * 1.001, 0.7, 0.999999])
    u1 = np.array([0.2, 0.9, 0.5, 0.3, 0.75, 0.0])
    u2 = np.array([0.3, 0.8, 0.5, 0.6, 0.5, 1.0])
    pts, face, cum = M.sample_surface(v, f, u0, u1, u2)
    assert np.allclose(cum, [a0, total], rtol=0, atol=1e-15)
    for i in range(len(u0)):
        want_face = 0 if u0[i] * total <= a0 else 1
        assert face[i] == want_face
        r1, r2 = u1[i], u2[i]
        if r1 + r2 > 1:
            r1, r2 = abs(r1 - 1), abs(r2 - 1)
        o, b, c = (v[f[want_face]].astype(np.float64))
        assert np.allclose(pts[i], o + r1 * (b - o) + r2 * (c - o), rtol=0, atol=1e-14)
    # the torch implementation (device-agnostic helper) on CPU tensors
    got, gface = mesh._sample_surface_from_uniforms(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(u0),
                                                    torch.from_numpy(u1), torch.from_numpy(u2))
    assert got.dtype == torch.float32 and np.array_equal(gface.numpy(), face)
    assert np.array_equal(got.numpy(), pts.astype(np.float32))
