"""numpy restatement of ls2fm_mesh_* (csrc/mesh_components.hip) and of ls2fm.mesh.sample_surface, the checkers of the device
results.  include/ls2fm.h states the rules: faces joined through shared vertex indices, the label of a vertex = the smallest
vertex index of its component; areas 0.5 |(b - a) x (c - a)| in float64; the largest component by area, ties to the one holding
the lowest-numbered face; extraction in original face and vertex order.  The sampling is trimesh.sample.sample_surface's
algorithm as published, with its uniforms passed in."""
import numpy as np


def _compress(parent):
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            return parent
        parent = nxt


def components(faces, n_verts):
    """labels int64 [n_verts]: union-find over vertex pairs (a, b), (a, c) of every face; roots hooked larger under smaller,
    so every root is its component's smallest index"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    parent = np.arange(n_verts, dtype=np.int64)
    e0 = np.concatenate([f[:, 0], f[:, 0]])
    e1 = np.concatenate([f[:, 1], f[:, 2]])
    while True:
        parent = _compress(parent)
        ra, rb = parent[e0], parent[e1]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        live = hi != lo
        if not live.any():
            return parent
        np.minimum.at(parent, hi[live], lo[live])


def face_components_by_edges(faces):
    """component id int64 [F] of every face, faces joined through shared undirected EDGES (trimesh's split rule): the id is the
    smallest face index of the component"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = len(f)
    und = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    owner = np.tile(np.arange(n, dtype=np.int64), 3)
    order = np.lexsort((owner, und[:, 1], und[:, 0]))
    und, owner = und[order], owner[order]
    same = (und[1:] == und[:-1]).all(axis=1)
    a, b = owner[:-1][same], owner[1:][same]
    parent = np.arange(n, dtype=np.int64)
    while True:
        parent = _compress(parent)
        ra, rb = parent[a], parent[b]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        live = hi != lo
        if not live.any():
            return parent
        np.minimum.at(parent, hi[live], lo[live])


def face_areas(verts, faces):
    """float64 [F]: 0.5 |(b - a) x (c - a)| from the float32 corners, trimesh's formula"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    u = v[f[:, 1]] - v[f[:, 0]]
    w = v[f[:, 2]] - v[f[:, 0]]
    c = np.cross(u, w)
    return np.sqrt((c ** 2).sum(axis=1)) / 2


def component_areas(verts, faces, labels):
    """float64 [V]: the area of the component labelled l at index l"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.bincount(labels[f[:, 0]], weights=face_areas(verts, f), minlength=len(labels))


def largest_label(verts, faces, labels, rel_tie=1e-9):
    """label of the largest component; components within rel_tie of the largest area count as tied, and the one holding the
    lowest-numbered face wins (np.argmax over components listed by lowest face)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    areas = component_areas(verts, f, labels)
    face_label = labels[f[:, 0]]
    best = areas.max()
    tied = areas >= best - rel_tie * best
    first = np.full(len(labels), len(f), dtype=np.int64)
    np.minimum.at(first, face_label, np.arange(len(f)))
    first[~tied] = len(f)
    return int(face_label[int(first.min())])


def extract(verts, faces, labels, label):
    """(verts float32 [V', 3], faces int32 [F', 3]) of the component `label`: faces in order, vertices in index order,
    renumbered (Trimesh.submesh)"""
    v = np.asarray(verts, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keep_f = labels[f[:, 0]] == label
    keep_v = labels == label
    new_id = np.cumsum(keep_v) - 1
    return v[keep_v], new_id[f[keep_f]].astype(np.int32)


def sample_surface(verts, faces, u0, u1, u2):
    """trimesh.sample.sample_surface(mesh, len(u0)) with its uniforms given (u0: face pick, u1 / u2: the point in the face),
    restated from trimesh's published source -> (points float64 [n, 3], face index int64 [n], cum float64 [F])"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    weight_cum = np.cumsum(face_areas(v, f))
    face_pick = np.asarray(u0, dtype=np.float64) * weight_cum[-1]
    face_index = np.searchsorted(weight_cum, face_pick)
    tri_origins = v[f[:, 0]]
    tri_vectors = v[f[:, 1:]].copy()
    tri_vectors -= np.tile(tri_origins, (1, 2)).reshape((-1, 2, 3))
    tri_origins = tri_origins[face_index]
    tri_vectors = tri_vectors[face_index]
    random_lengths = np.stack([u1, u2], axis=1).astype(np.float64).reshape(-1, 2, 1)
    random_transform = random_lengths.sum(axis=1).reshape(-1) > 1.0
    random_lengths[random_transform] -= 1.0
    random_lengths = np.abs(random_lengths)
    sample_vector = (tri_vectors * random_lengths).sum(axis=1)
    return sample_vector + tri_origins, face_index, weight_cum
