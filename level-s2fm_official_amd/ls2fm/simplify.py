"""Mesh simplification on the device: vertex clustering with quadric error metrics (Lindstrom 2000) behind ls2fm_mesh_simplify_*
(csrc/mesh_simplify.hip).  extract_mesh at 512^3 gives several hundred thousand faces; a viewer wants a tenth of that, and the usual
target-face-count export is a sequential edge collapse on the host.  Clustering is one order-free pass: every cell of an absolute
lattice of side `cell` keeps one vertex, placed where the summed quadrics of the faces touching the cell are smallest.

  simplify            one cell size -> SimplifiedMesh(vertices, faces, vertex_map, colors)
  count_faces         the faces that survive a cell size, from the keys kernels alone
  simplify_to_faces   the smallest cell of a fixed bisection whose surviving count is at most a target, then one simplify
  _simplify_torch     the same rule as plain torch ops with index_add_ in fp64, on any device: the timing baseline and a check

THE CLUSTERING RULE is stated in include/ls2fm.h and repeated in numpy by tests/simplify_restate.py; the result is a pure function
of the mesh, the cell and the options, identical bits on every call.  Stated deviations from an edge-collapse decimation: clustering
can create non-manifold edges and fold-overs; opposite-oriented duplicate faces both stay; nothing preserves boundaries or feature
edges beyond what the quadrics give; there are no texture coordinates; the lattice is anchored at 0, not at the mesh's box, so a
translated mesh simplifies differently.  There is no CPU path for the kernels: CPU tensors, a missing device or library raise.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .mesh import _check_mesh, _faces_i32

KEY_BITS = 21                                  # per axis, as ls2fm.metrics.voxel_downsample packs them
INVALID_KEY = -1                               # every cell's key is >= 0
N_SUMS = 13                                    # LS2FM_SIMPLIFY_SUMS: A (6), b (3), d d, sum p (3); the colour channels follow
DEFAULT_REG = 2.0 ** -2
_PLACEMENTS = {"quadric": 0, "mean": 1}
_STAGE_SUMS, _STAGE_SOLVE = 1, 2
BISECTION_STEPS = 20


class SimplifiedMesh(NamedTuple):
    """vertices float32 [V', 3], faces int32 [F', 3], vertex_map int32 [V] (the output index of each input vertex's cell, -1 for a
    vertex that is not finite or whose cell is not output), colors float32 [V', C] or None"""
    vertices: torch.Tensor
    faces: torch.Tensor
    vertex_map: torch.Tensor
    colors: Optional[torch.Tensor]


def _cell32(cell, what):
    c = np.float32(cell)
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"ls2fm.simplify.{what}: cell {cell} must be positive and finite in float32")
    return float(c)


def _options(placement, reg, what):
    if placement not in _PLACEMENTS:
        raise ValueError(f"ls2fm.simplify.{what}: placement must be 'quadric' or 'mean', got {placement!r}")
    reg = float(reg)
    if not (math.isfinite(reg) and reg >= 0):
        raise ValueError(f"ls2fm.simplify.{what}: reg {reg} must be finite and >= 0")
    return _PLACEMENTS[placement], reg


def _colors(colors, n_verts, what):
    if colors is None:
        return None
    if colors.dim() != 2 or colors.shape[0] != n_verts or not 1 <= colors.shape[1] <= 4:
        raise ValueError(f"ls2fm.simplify.{what}: colors must be [{n_verts}, 1 .. 4], got shape {tuple(colors.shape)}")
    return colors


def _bad(n_bad, what):
    return ValueError(f"ls2fm.simplify.{what}: {n_bad} vertices have a cell coordinate that does not fit in {KEY_BITS} bits "
                      f"(|v / cell| up to 2^{KEY_BITS - 1})")


def _first_oriented(tri, on):
    """bool [F]: face f is `on` and no earlier `on` face is the same oriented triangle (equal after rotating the smallest index to the
    front).  tri integer [F, 3] with distinct non-negative entries where `on`.  Two stable sorts of the rotated triples, no host read."""
    n = tri.shape[0]
    dev = tri.device
    t = tri.to(torch.int64)
    lead = t.argmin(dim=1)
    rot = torch.gather(t, 1, (lead[:, None] + torch.arange(3, device=dev)[None, :]) % 3)
    a = torch.where(on, rot[:, 0], torch.full_like(rot[:, 0], 1 << 31))
    bc = (rot[:, 1] << 31) | rot[:, 2]
    o1 = torch.sort(bc, stable=True).indices
    o2 = torch.sort(a[o1], stable=True).indices
    perm = o1[o2]
    sa, sbc = a[perm], bc[perm]
    first = torch.ones(n, dtype=torch.bool, device=dev)
    first[1:] = (sa[1:] != sa[:-1]) | (sbc[1:] != sbc[:-1])
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    keep[perm] = first
    return keep & on


def _prepare(verts, faces, what):
    """device-only, shapes, the face-index check (one host read) -> (verts float32, faces int32, library, workspace bytes)"""
    _check_mesh(verts, faces, what)
    lib = _lib.load()
    v = _lib.cf(verts)
    f = _faces_i32(faces, v.shape[0], f"ls2fm.simplify.{what}")
    ws_bytes = int(lib.ls2fm_mesh_simplify_workspace_bytes(v.shape[0], f.shape[0]))
    if ws_bytes < 0:
        raise ValueError(f"ls2fm.simplify.{what}: {v.shape[0]} vertices / {f.shape[0]} faces refused (V < 2^31 and 3 F < 2^31)")
    return v, f, lib, ws_bytes


def _keys(lib, v, f, cell, with_classes):
    """ls2fm_mesh_simplify_keys -> (vert_key int64 [V], face_class uint8 [F] or None, counts int64 [2] = surviving, bad)"""
    dev = v.device
    vert_key = torch.empty(v.shape[0], dtype=torch.int64, device=dev)
    face_class = torch.empty(f.shape[0], dtype=torch.uint8, device=dev) if with_classes else None
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    check(lib.ls2fm_mesh_simplify_keys(ptr(v), v.shape[0], ptr(f), f.shape[0], cell, ptr(vert_key), ptr(face_class), ptr(counts),
                                       stream_ptr()), "ls2fm_mesh_simplify_keys")
    return vert_key, face_class, counts


def _last(t):
    """the last entry of an inclusive prefix sum as int64 [1]; 0 for an empty one"""
    return t[-1:].to(torch.int64) if t.numel() else torch.zeros(1, dtype=torch.int64, device=t.device)


def _place(lib, st, stages):
    """ls2fm_mesh_simplify_place on the state of _simplify_device (tools/time_simplify.py times the sums stage alone with it)"""
    c = st["colors"]
    check(lib.ls2fm_mesh_simplify_place(ptr(st["verts"]), ptr(c), 0 if c is None else c.shape[1], st["verts"].shape[0], ptr(st["faces"]),
                                        st["faces"].shape[0], st["cell"], st["placement"], st["reg"], ptr(st["sorted_key"]),
                                        ptr(st["sorted_vert"]), ptr(st["sorted_corner_head"]), ptr(st["sorted_corner"]), st["n_out"],
                                        stages, ptr(st["sums"]), ptr(st["count"]), ptr(st["out_verts"]), ptr(st["out_colors"]),
                                        ptr(st["workspace"]), st["workspace"].numel(), stream_ptr()), "ls2fm_mesh_simplify_place")


def _simplify_device(v, f, lib, ws_bytes, cell, colors, placement, reg):
    """the calls of include/ls2fm.h with torch's sorts and prefix sums between them; ONE host read (the counts).
    -> (SimplifiedMesh, the state: every intermediate array by its header name)"""
    dev = v.device
    n_verts, n_faces = int(v.shape[0]), int(f.shape[0])
    with torch.cuda.device(dev):
        vert_key, face_class, counts = _keys(lib, v, f, cell, True)
        sorted_key, sorted_vert = torch.sort(vert_key, stable=True)
        ws = _lib.workspace(ws_bytes, "ls2fm_mesh_simplify_workspace_bytes", dev, min_bytes=256)
        corner_head = torch.empty(3 * n_faces, dtype=torch.int32, device=dev)
        head_used = torch.empty(n_verts, dtype=torch.int32, device=dev)
        check(lib.ls2fm_mesh_simplify_mark(ptr(sorted_key), ptr(sorted_vert), n_verts, ptr(f), n_faces, ptr(face_class), ptr(corner_head),
                                           ptr(head_used), ptr(ws), ws.numel(), stream_ptr()), "ls2fm_mesh_simplify_mark")
        head_rank = torch.cumsum(head_used, dim=0, dtype=torch.int32)
        sorted_corner_head, sorted_corner = torch.sort(corner_head, stable=True)
        vertex_map = torch.empty(n_verts, dtype=torch.int32, device=dev)
        face_index = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
        check(lib.ls2fm_mesh_simplify_index(ptr(head_used), ptr(head_rank), n_verts, ptr(f), n_faces, ptr(face_class), ptr(vertex_map),
                                            ptr(face_index), ptr(ws), ws.numel(), stream_ptr()), "ls2fm_mesh_simplify_index")
        keep = _first_oriented(face_index, face_class == 2)
        keep_rank = torch.cumsum(keep, dim=0, dtype=torch.int32)
        keep_u8 = keep.to(torch.uint8)
        n_out, n_surviving, n_bad, n_kept = (int(x) for x in torch.cat([_last(head_rank), counts, _last(keep_rank)]).cpu())
        if n_bad:
            raise _bad(n_bad, "simplify")
        n_ch = 0 if colors is None else int(colors.shape[1])
        st = dict(verts=v, faces=f, colors=colors, cell=cell, placement=placement, reg=reg, vert_key=vert_key, face_class=face_class,
                  sorted_key=sorted_key, sorted_vert=sorted_vert, sorted_corner_head=sorted_corner_head, sorted_corner=sorted_corner,
                  head_used=head_used, head_rank=head_rank, face_index=face_index, keep=keep, workspace=ws, n_out=n_out,
                  n_surviving=n_surviving, n_kept=n_kept,
                  sums=torch.empty(n_out, N_SUMS + n_ch, dtype=torch.float64, device=dev),
                  count=torch.empty(n_out, dtype=torch.int32, device=dev),
                  out_verts=torch.empty(n_out, 3, dtype=torch.float32, device=dev),
                  out_colors=None if colors is None else torch.empty(n_out, n_ch, dtype=torch.float32, device=dev))
        _place(lib, st, _STAGE_SUMS | _STAGE_SOLVE)
        out_faces = torch.empty(n_kept, 3, dtype=torch.int32, device=dev)
        check(lib.ls2fm_mesh_simplify_emit(ptr(face_index), ptr(keep_u8), ptr(keep_rank), n_faces, n_kept, ptr(out_faces), stream_ptr()),
              "ls2fm_mesh_simplify_emit")
    return SimplifiedMesh(st["out_verts"], out_faces, vertex_map, st["out_colors"]), st


def simplify(verts, faces, cell, colors=None, placement="quadric", reg=DEFAULT_REG) -> SimplifiedMesh:
    """The mesh clustered on the absolute lattice of side `cell` (world units; rounded to float32) by THE CLUSTERING RULE of
    include/ls2fm.h.  verts float32 [V, 3] and faces integer [F, 3] on the device; colors float32 [V, 1 .. 4] on the device are averaged
    per cell.  placement "quadric": each cell's vertex minimises the summed face quadrics, regularised towards the cell's mean vertex
    by reg * trace and falling back to that mean when the minimiser leaves the cell or the solve fails; "mean": the mean vertex.
    Vertices: the cells holding a corner of a surviving face, in ascending key order; faces: the surviving faces in input order
    without repeated oriented triangles.  A finite vertex whose cell coordinate does not fit in 21 bits raises ValueError (as
    ls2fm.metrics.voxel_downsample does); a vertex that is not finite takes its faces with it.  Two host reads: the face-index check and
    the counts."""
    cell = _cell32(cell, "simplify")
    code, reg = _options(placement, reg, "simplify")
    _lib.require_device_tensors("ls2fm.simplify", colors, phrase=" runs on the GPU only")
    v, f, lib, ws_bytes = _prepare(verts, faces, "simplify")
    c = _colors(colors, v.shape[0], "simplify")
    return _simplify_device(v, f, lib, ws_bytes, cell, None if c is None else _lib.cf(c), code, reg)[0]


def _count(lib, v, f, cell):
    with torch.cuda.device(v.device):
        return tuple(int(x) for x in _keys(lib, v, f, cell, False)[2].cpu())


def count_faces(verts, faces, cell) -> int:
    """the number of faces that survive clustering at `cell` -- their three vertices finite and in three different cells -- BEFORE
    duplicate removal: the keys kernels alone, no sort.  ValueError as simplify raises it."""
    cell = _cell32(cell, "count_faces")
    v, f, lib, _ = _prepare(verts, faces, "count_faces")
    n, n_bad = _count(lib, v, f, cell)
    if n_bad:
        raise _bad(n_bad, "count_faces")
    return n


def _diagonal(v):
    """the diagonal of the bounding box of the finite vertices, in float64 on the host (one read); 0.0 without a finite vertex"""
    if v.shape[0] == 0:
        return 0.0
    fin = torch.isfinite(v).all(dim=1, keepdim=True)
    lo = torch.where(fin, v, torch.full_like(v, float("inf"))).amin(dim=0)
    hi = torch.where(fin, v, torch.full_like(v, float("-inf"))).amax(dim=0)
    box = torch.stack([lo, hi]).to(torch.float64).cpu().numpy()
    return float(np.sqrt(((box[1] - box[0]) ** 2).sum())) if np.isfinite(box).all() else 0.0


def _bisect_cell(count, diagonal, target_faces):
    """the fixed bisection of simplify_to_faces on log(cell) between diagonal 2^-20 and diagonal; count(cell) -> (surviving, bad).
    -> the smallest cell tried whose count is <= target_faces (a cell with bad vertices counts as too small)"""
    def fits(cell):
        n, n_bad = count(cell)
        return n_bad == 0 and n <= target_faces

    best = float(np.float32(diagonal))
    if not fits(best):
        raise ValueError(f"ls2fm.simplify.simplify_to_faces: more than {target_faces} faces survive even a cell of the bounding box's "
                         f"diagonal {best}")
    lo, hi = math.log(diagonal) - BISECTION_STEPS * math.log(2.0), math.log(diagonal)
    for _ in range(BISECTION_STEPS):
        mid = 0.5 * (lo + hi)
        cell = float(np.float32(math.exp(mid)))
        if fits(cell):
            best, hi = min(best, cell), mid
        else:
            lo = mid
    return best


def simplify_to_faces(verts, faces, target_faces, **kw) -> SimplifiedMesh:
    """simplify at the smallest cell of a fixed bisection whose surviving-face count (count_faces) is at most target_faces: 20 steps
    on log(cell) between 2^-20 of the bounding box's diagonal and the diagonal, the count at the diagonal first, every cell rounded to
    float32.  Deterministic: the same cells are tried on every call.  The result can have FEWER faces than the count by the repeated
    oriented triangles simplify removes, and the count is not strictly monotone in `cell` (the lattice is absolute: a larger cell can
    split a cluster a smaller one kept together), so the cell found is the smallest TRIED that fits, not the smallest that exists.
    ValueError when even the diagonal leaves more than target_faces, or the mesh has no extent.  **kw as simplify's.  One host read
    per step on top of simplify's."""
    target_faces = int(target_faces)
    if target_faces < 0:
        raise ValueError(f"ls2fm.simplify.simplify_to_faces: target_faces {target_faces} must be >= 0")
    v, f, lib, _ = _prepare(verts, faces, "simplify_to_faces")
    diagonal = _diagonal(v)
    if not diagonal > 0:
        raise ValueError("ls2fm.simplify.simplify_to_faces: the finite vertices have no extent")
    cell = _bisect_cell(lambda c: _count(lib, v, f, c), diagonal, target_faces)
    return simplify(v, f, cell, **kw)


def apply(verts, faces, spec, what):
    """the `simplify=` keyword of extract_mesh and get_surface_high_res_mesh -> (verts, faces): a number is a cell size in world
    units (simplify), {"faces": n} a target face count (simplify_to_faces); nothing else is taken"""
    if isinstance(spec, dict):
        if set(spec) != {"faces"}:
            raise ValueError(f"{what}(simplify=...): None, a cell size or {{'faces': n}}; got {spec!r}")
        out = simplify_to_faces(verts, faces, spec["faces"])
    elif isinstance(spec, (int, float, np.floating, np.integer)) and not isinstance(spec, bool):
        out = simplify(verts, faces, float(spec))
    else:
        raise ValueError(f"{what}(simplify=...): None, a cell size or {{'faces': n}}; got {spec!r}")
    return out.vertices, out.faces


# ------------------------------------------------------------------------------------------------------------------ torch form
def _solve_torch(A, g, lam):
    """csrc/lm_math.h chol_solve at size 3, operation for operation, batched: A [n, 6] the upper triangle row-major, g [n, 3],
    lam [n]; solves (A + lam I) x = -g -> (x [n, 3], ok bool [n])"""
    one = torch.ones_like(lam)
    L00, L10, L20 = A[:, 0] + lam * one, A[:, 1] + 0.0, A[:, 2] + 0.0
    L11, L21, L22 = A[:, 3] + lam * one, A[:, 4] + 0.0, A[:, 5] + lam * one
    ok = L00 > 0
    l00 = torch.sqrt(torch.where(L00 > 0, L00, one))
    L10, L20 = L10 / l00, L20 / l00
    d = L11 - L10 * L10
    ok = ok & (d > 0)
    l11 = torch.sqrt(torch.where(d > 0, d, one))
    L21 = (L21 - L20 * L10) / l11
    d = (L22 - L20 * L20) - L21 * L21
    ok = ok & (d > 0)
    l22 = torch.sqrt(torch.where(d > 0, d, one))
    z0 = -g[:, 0] / l00
    z1 = (-g[:, 1] - L10 * z0) / l11
    z2 = ((-g[:, 2] - L20 * z0) - L21 * z1) / l22
    x2 = z2 / l22
    x1 = (z1 - L21 * x2) / l11
    x0 = ((z0 - L10 * x1) - L20 * x2) / l00
    x = torch.stack([x0, x1, x2], dim=1)
    return x, ok & torch.isfinite(x).all(dim=1)


def _place_torch(sums, count, centre, cell, mean_only, reg):
    """step 6 of the rule on per-cell sums [n, 13 + C], counts [n] and cell centres [n, 3] (fp64) -> (verts float32 [n, 3], colours)"""
    m = count.to(torch.float64)
    mean = sums[:, 10:13] / m[:, None]
    x = mean
    if not mean_only:
        t = (sums[:, 0] + sums[:, 3]) + sums[:, 5]
        lam = reg * t
        y, ok = _solve_torch(sums[:, :6], -(sums[:, 6:9] + lam[:, None] * mean), lam)
        ok = ok & (t != 0) & torch.isfinite(t) & (y.abs() <= cell / 2.0).all(dim=1)
        x = torch.where(ok[:, None], y, mean)
    return (centre + x).to(torch.float32), (sums[:, N_SUMS:] / m[:, None]).to(torch.float32)


def _simplify_torch(verts, faces, cell, colors=None, placement="quadric", reg=DEFAULT_REG, return_sums=False):
    """THE CLUSTERING RULE as plain torch ops on whatever device the mesh is on: keys by torch.unique, the per-cell sums by
    index_add_ in fp64 -- the same terms as the kernels', added in no stated order, so the sums agree with simplify's to within the
    summation bound and the rest exactly unless a sum's last bits decide a comparison.  The timing baseline of simplify and the CPU
    route of the host tests; nothing in the library falls back to it.  -> SimplifiedMesh, or (SimplifiedMesh, sums, count) with
    return_sums."""
    cell = _cell32(cell, "_simplify_torch")
    code, reg = _options(placement, reg, "_simplify_torch")
    dev = verts.device
    v32 = verts.to(torch.float32)
    f = faces.to(torch.int64)
    colors = _colors(colors, v32.shape[0], "_simplify_torch")
    n_ch = 0 if colors is None else int(colors.shape[1])
    vd = v32.to(torch.float64)
    half = float(1 << (KEY_BITS - 1))
    finite = torch.isfinite(v32).all(dim=1)
    k = torch.floor(vd / cell)
    valid = finite & ((k >= -half) & (k < half)).all(dim=1)
    n_bad = int((finite & ~valid).sum())
    if n_bad:
        raise _bad(n_bad, "_simplify_torch")
    kb = torch.where(valid[:, None], k, torch.zeros_like(k)).to(torch.int64) + (1 << (KEY_BITS - 1))
    key = torch.where(valid, (kb[:, 0] << (2 * KEY_BITS)) | (kb[:, 1] << KEY_BITS) | kb[:, 2], torch.full_like(kb[:, 0], INVALID_KEY))
    fk = key[f]
    face_valid = valid[f].all(dim=1) if f.numel() else torch.zeros(0, dtype=torch.bool, device=dev)
    surviving = face_valid & (fk[:, 0] != fk[:, 1]) & (fk[:, 1] != fk[:, 2]) & (fk[:, 0] != fk[:, 2])
    cells, inverse = torch.unique(key, return_inverse=True)
    used = torch.zeros(cells.shape[0], dtype=torch.bool, device=dev)
    used[inverse[f[surviving].reshape(-1)]] = True
    rank = torch.cumsum(used, dim=0) - 1
    out_key = cells[used]
    n_out = int(out_key.shape[0])
    vertex_map = torch.where(valid & used[inverse], rank[inverse], torch.full_like(inverse, -1))
    shifts = torch.tensor([2 * KEY_BITS, KEY_BITS, 0], device=dev)
    centre = ((((out_key[:, None] >> shifts[None, :]) & ((1 << KEY_BITS) - 1)) - (1 << (KEY_BITS - 1))).to(torch.float64) + 0.5) * cell
    sums = torch.zeros(n_out, N_SUMS + n_ch, dtype=torch.float64, device=dev)
    at = torch.nonzero(vertex_map >= 0)[:, 0]
    to = vertex_map[at]
    per_vertex = [vd[at] - centre[to]] + ([] if colors is None else [colors.to(torch.float32).to(torch.float64)[at]])
    sums[:, 10:] = torch.zeros(n_out, 3 + n_ch, dtype=torch.float64, device=dev).index_add_(0, to, torch.cat(per_vertex, dim=1))
    count = torch.zeros(n_out, dtype=torch.int64, device=dev).index_add_(0, to, torch.ones_like(to))
    quadric = torch.zeros(n_out, 10, dtype=torch.float64, device=dev)
    for c in range(3):
        first = face_valid & (vertex_map[f[:, c]] >= 0) if f.numel() else face_valid
        for e in range(c):
            first = first & (fk[:, c] != fk[:, e])
        fc = f[first]
        to = vertex_map[fc[:, c]]
        g = centre[to]
        pa, pb, pc = vd[fc[:, 0]] - g, vd[fc[:, 1]] - g, vd[fc[:, 2]] - g
        u, w = pb - pa, pc - pa
        n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        d = (n0 * pa[:, 0] + n1 * pa[:, 1]) + n2 * pa[:, 2]
        quadric.index_add_(0, to, torch.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, d * n0, d * n1, d * n2, d * d], dim=1))
    sums[:, :10] = quadric
    out_verts, out_colors = _place_torch(sums, count, centre, cell, code == _PLACEMENTS["mean"], reg)
    tri = vertex_map[f[surviving]]
    out_faces = tri[_first_oriented(tri, torch.ones(tri.shape[0], dtype=torch.bool, device=dev))].to(torch.int32)
    out = SimplifiedMesh(out_verts, out_faces, vertex_map.to(torch.int32), None if colors is None else out_colors)
    return (out, sums, count.to(torch.int32)) if return_sums else out
