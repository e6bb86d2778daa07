"""Mesh extraction on the device: marching cubes over a dense volume (ls2fm_marching_cubes_*), connected components and the
largest one by area (ls2fm_mesh_*), area-weighted surface sampling and a PLY writer / reader (binary and ASCII).

Replaces the third-party steps of the reference's extract_mesh (utils/util.py:392-425 -> convert_sigma_samples_to_ply,
util.py:345): skimage.measure.marching_cubes and plyfile; and of get_surface_high_res_mesh (utils/plots.py:140-222):
trimesh's split / area / submesh, trimesh.sample.sample_surface and trimesh.exchange.ply.export_ply.  The case table is
generated from one face rule (tools/gen_mc_tables.py; include/ls2fm.h documents the rule, the vertex arithmetic and the
output order).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


def marching_cubes(volume: torch.Tensor, level: float = 0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """the mesh of {volume = level}: verts float32 [V, 3] = (index + t) * spacing + origin along the volume's axes, faces int32
    [F, 3] with right-hand normals toward increasing values; both on the volume's device.  One host synchronisation (the counts)."""
    lib = _lib.load()
    if volume.dim() != 3:
        raise ValueError(f"marching_cubes: a 3-d volume is needed, got shape {tuple(volume.shape)}")
    _lib.require_device_tensors("ls2fm.mesh.marching_cubes", volume, phrase=" runs on the GPU only")
    vol = _lib.cf(volume)
    nx, ny, nz = (int(s) for s in vol.shape)
    dev = vol.device
    ws_bytes = int(lib.ls2fm_marching_cubes_workspace_bytes(nx, ny, nz))
    if ws_bytes < 0:
        raise ValueError(f"marching_cubes: volume {nx}x{ny}x{nz} refused (every side >= 2 and 3*nx*ny*nz < 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        check(lib.ls2fm_marching_cubes_count(ptr(vol), nx, ny, nz, float(level), ptr(ws), ptr(counts), stream_ptr()),
              "ls2fm_marching_cubes_count")
        n_verts, n_faces = (int(v) for v in counts.cpu())
        verts = torch.empty(n_verts, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
        if n_verts or n_faces:
            sp = (ctypes.c_float * 3)(*[float(v) for v in spacing])
            og = (ctypes.c_float * 3)(*[float(v) for v in origin])
            check(lib.ls2fm_marching_cubes_emit(ptr(vol), nx, ny, nz, float(level), sp, og, ptr(ws), ptr(verts), ptr(faces),
                                                stream_ptr()), "ls2fm_marching_cubes_emit")
    return verts, faces


class Mesh(NamedTuple):
    """a triangle mesh: vertices float32 [V, 3], faces int32 [F, 3]"""
    vertices: torch.Tensor
    faces: torch.Tensor


def select_faces(verts: torch.Tensor, faces: torch.Tensor, keep: torch.Tensor) -> Mesh:
    """the faces with keep (bool [F]) set, the vertices no kept face uses dropped and the faces re-indexed, both in their order,
    with torch ops: the compaction that ends ls2fm.raster.clean_mesh and ls2fm.fusion.extract"""
    kept = faces.long()[keep]
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    used[kept.reshape(-1)] = True
    renumber = torch.cumsum(used.to(torch.int64), dim=0) - 1
    return Mesh(verts[used], renumber[kept].to(torch.int32))


def finite_faces(verts: torch.Tensor, faces: torch.Tensor) -> Mesh:
    """the faces whose three vertices are finite, then select_faces' compaction: the tail of ls2fm.fusion.extract and
    ls2fm.cloud_mesh.extract, where marching cubes puts a NaN vertex on every edge into an undefined lattice point"""
    good = torch.isfinite(verts).all(dim=1)
    keep = good[faces.long()].all(dim=1) if faces.shape[0] else torch.zeros(0, dtype=torch.bool, device=verts.device)
    return select_faces(verts, faces, keep)


def _check_mesh(verts, faces, what):
    """device-only and [., 3] shapes"""
    _lib.require_device_tensors(f"ls2fm.mesh.{what}", faces, verts, phrase=" runs on the GPU only")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be [F, 3], got shape {tuple(faces.shape)}")
    if verts is not None and (verts.dim() != 2 or verts.shape[1] != 3):
        raise ValueError(f"{what}: verts must be [V, 3], got shape {tuple(verts.shape)}")


def _faces_i32(faces, n_verts, what):
    """faces as contiguous int32, every index checked in [0, n_verts) (one device reduction, one host read)"""
    f = faces if faces.dtype == torch.int32 and faces.is_contiguous() else faces.to(torch.int32).contiguous()
    if f.numel():
        lo, hi = (int(v) for v in torch.stack(torch.aminmax(faces.reshape(-1))).cpu())
        if lo < 0 or hi >= n_verts:
            raise ValueError(f"{what}: face indices span [{lo}, {hi}], outside [0, {n_verts})")
    return f


def connected_components(faces: torch.Tensor, n_verts: int) -> torch.Tensor:
    """labels int32 [n_verts] on the faces' device: the smallest vertex index of each vertex's component, faces joined through
    shared vertex indices (include/ls2fm.h); a vertex no face uses is its own component"""
    lib = _lib.load()
    _check_mesh(None, faces, "connected_components")
    n_verts = int(n_verts)
    f = _faces_i32(faces, n_verts, "connected_components")
    if lib.ls2fm_mesh_components_workspace_bytes(n_verts, f.shape[0]) < 0:
        raise ValueError(f"connected_components: {n_verts} vertices / {f.shape[0]} faces refused (both < 2^31)")
    with torch.cuda.device(f.device):
        labels = torch.empty(n_verts, dtype=torch.int32, device=f.device)
        check(lib.ls2fm_mesh_components(ptr(f), n_verts, f.shape[0], ptr(labels), stream_ptr()), "ls2fm_mesh_components")
    return labels


def _largest_count(verts, faces, want_areas):
    lib = _lib.load()
    v = _lib.cf(verts)
    n_verts = v.shape[0]
    f = _faces_i32(faces, n_verts, "largest_component")
    ws_bytes = int(lib.ls2fm_mesh_components_workspace_bytes(n_verts, f.shape[0]))
    if ws_bytes < 0:
        raise ValueError(f"largest_component: {n_verts} vertices / {f.shape[0]} faces refused (both < 2^31)")
    dev = v.device
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    areas = torch.zeros(n_verts, dtype=torch.float64, device=dev) if want_areas else None
    if f.shape[0]:
        check(lib.ls2fm_mesh_largest_component_count(ptr(v), n_verts, ptr(f), f.shape[0], ptr(ws), ws_bytes, ptr(counts),
                                                     ptr(areas), stream_ptr()), "ls2fm_mesh_largest_component_count")
    return v, f, ws, ws_bytes, counts, areas


def component_areas(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """float64 [V]: entry l = the area of the component labelled l (connected_components), 0 where l is no label.  Summed in
    64-bit fixed point: independent of the face order, identical bits on every call"""
    _check_mesh(verts, faces, "component_areas")
    with torch.cuda.device(faces.device):
        return _largest_count(verts, faces, True)[5]


def largest_component(verts: torch.Tensor, faces: torch.Tensor) -> Mesh:
    """the component of largest area (ties: the one holding the lowest-numbered face), as Trimesh.split + argmax(area) +
    submesh give it: its faces in their order, the vertices they use in index order, the faces renumbered.  One host read
    (the counts) after the index check's."""
    _check_mesh(verts, faces, "largest_component")
    with torch.cuda.device(faces.device):
        v, f, ws, ws_bytes, counts, _ = _largest_count(verts, faces, False)
        n_v, n_f = (int(c) for c in counts.cpu())
        out_v = torch.empty(n_v, 3, dtype=torch.float32, device=v.device)
        out_f = torch.empty(n_f, 3, dtype=torch.int32, device=v.device)
        if n_f:
            check(_lib.load().ls2fm_mesh_largest_component_emit(ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(ws), ws_bytes,
                                                                ptr(out_v), ptr(out_f), stream_ptr()),
                  "ls2fm_mesh_largest_component_emit")
    return Mesh(out_v, out_f)


def _face_areas64(verts, faces):
    """0.5 |(b - a) x (c - a)| in float64 (trimesh's area_faces on float64 vertices)"""
    tri = verts.to(torch.float64)[faces.long()]
    u, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cross = torch.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                         u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], dim=1)
    return (cross * cross).sum(dim=1).sqrt() / 2


def _sample_surface_from_uniforms(verts, faces, u0, u1, u2):
    """trimesh.sample.sample_surface with its uniforms given: u0 [n] picks the face by area, (u1, u2) [n] the point in it.
    -> (points float32 [n, 3], face index int64 [n])"""
    area = _face_areas64(verts, faces)
    cum = torch.cumsum(area, dim=0)
    face = torch.searchsorted(cum, u0.to(torch.float64) * cum[-1], side="left")
    face = face.clamp(max=faces.shape[0] - 1)             # u0 < 1 keeps pick < cum[-1]; guards the rounding of the product
    tri = verts.to(torch.float64)[faces.long()[face]]
    o, v1, v2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    r1, r2 = u1.to(torch.float64), u2.to(torch.float64)
    flip = r1 + r2 > 1.0
    r1 = torch.where(flip, (r1 - 1.0).abs(), r1)
    r2 = torch.where(flip, (r2 - 1.0).abs(), r2)
    pts = (v1 * r1[:, None] + v2 * r2[:, None]) + o       # trimesh: (vectors * lengths).sum(axis=1) + origins
    return pts.to(torch.float32), face


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, count: int, generator=None) -> torch.Tensor:
    """`count` points on the surface, faces picked with probability proportional to their area and points uniform in the
    face: trimesh.sample.sample_surface's algorithm in float64 on the device, cast to float32 (as plots.py:169 does).  The
    uniforms come from `generator` or torch's default generator of the device, so runs under torch.manual_seed repeat."""
    _check_mesh(verts, faces, "sample_surface")
    if faces.shape[0] == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    dev = verts.device
    u0 = torch.rand(count, dtype=torch.float64, device=dev, generator=generator)
    u12 = torch.rand(count, 2, dtype=torch.float64, device=dev, generator=generator)
    return _sample_surface_from_uniforms(verts, faces, u0, u12[:, 0], u12[:, 1])[0]


def _as_numpy(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1, 3))


_COLOR_NAMES = ("red", "green", "blue", "alpha")


def _n_color_channels(colors) -> int:
    """0 for None; else the channel count of a colour array [V, 3 | 4], or an int 3 | 4 itself"""
    if colors is None:
        return 0
    n = int(colors) if isinstance(colors, (int, np.integer)) else (int(colors.shape[1]) if getattr(colors, "ndim", 0) == 2 else -1)
    if n not in (3, 4):
        raise ValueError(f"ply colours must have 3 (red green blue) or 4 (+ alpha) channels, got {colors if n >= 0 else 'a wrong shape'}")
    return n


def _header(fmt: str, n_verts: int, n_faces: int, colors) -> bytes:
    color_lines = "".join(f"property uchar {name}\n" for name in _COLOR_NAMES[:_n_color_channels(colors)])
    return (f"ply\nformat {fmt} 1.0\n"
            f"element vertex {n_verts}\nproperty float x\nproperty float y\nproperty float z\n{color_lines}"
            f"element face {n_faces}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


def ply_header(n_verts: int, n_faces: int, colors=None) -> bytes:
    """the header plyfile writes for extract_mesh's two elements (binary, little endian); colors (an array [V, 3 | 4] or the
    channel count) adds `property uchar red green blue (alpha)` to the vertex element"""
    return _header("binary_little_endian", n_verts, n_faces, colors)


def ply_header_ascii(n_verts: int, n_faces: int, colors=None) -> bytes:
    """the header of write_ply(encoding="ascii"): the same elements as the binary layout"""
    return _header("ascii", n_verts, n_faces, colors)


_ASCII_BLOCK = 1 << 16          # rows formatted per string operation


def _ascii_rows(fh, rows, fmt):
    for at in range(0, len(rows), _ASCII_BLOCK):
        block = rows[at:at + _ASCII_BLOCK]
        fh.write(((fmt * len(block)) % tuple(block.ravel().tolist())).encode("ascii"))


def color_bytes(colors, n_verts: int) -> np.ndarray:
    """vertex colours [V, 3 | 4] (tensor or array) as the bytes write_ply stores: a uint8 array as it is, anything else
    round(clip(c, 0, 1) * 255) with halves to even (a NaN becomes 0)"""
    if isinstance(colors, torch.Tensor):
        colors = colors.detach().cpu().numpy()
    c = np.asarray(colors)
    if c.ndim != 2 or c.shape[1] not in (3, 4) or c.shape[0] != n_verts:
        raise ValueError(f"write_ply: colors must be [{n_verts}, 3] or [{n_verts}, 4], got shape {tuple(c.shape)}")
    if c.dtype == np.uint8:
        return np.ascontiguousarray(c)
    with np.errstate(invalid="ignore"):
        return np.rint(np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)


def _vertex_dtype(n_channels: int) -> np.dtype:
    """one packed row of the binary vertex element"""
    return np.dtype([("xyz", "<f4", (3,))] + ([("rgb", "u1", (n_channels,))] if n_channels else []))


_FACE_DTYPE = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])      # packed: 13 bytes per face


def write_ply(path, verts, faces, encoding: str = "binary", colors=None) -> None:
    """write verts [V, 3] / faces [F, 3] (tensors or arrays).
    encoding="binary": the layout extract_mesh's plyfile branch writes: binary_little_endian 1.0, `element vertex` of float
    x/y/z, `element face` of `property list uchar int vertex_indices`.
    encoding="ascii": the same elements as text (get_surface_high_res_mesh's export_ply(encoding='ascii')): one `x y z` line
    per vertex with 9 significant digits (a float32 round-trips), one `3 a b c` line per face.
    colors [V, 3] or [V, 4] in [0, 1] (color_bytes): `uchar red green blue` per vertex, a fourth channel `alpha`, what
    trimesh reads into mesh.visual.vertex_colors.  None: the bytes written without the argument."""
    if encoding not in ("binary", "ascii"):
        raise ValueError(f"write_ply: encoding must be 'binary' or 'ascii', got {encoding!r}")
    v = _as_numpy(verts, "<f4")
    f = _as_numpy(faces, "<i4")
    c = None if colors is None else color_bytes(colors, len(v))
    if encoding == "ascii":
        with open(path, "wb") as fh:
            fh.write(ply_header_ascii(len(v), len(f), c))
            if c is None:
                _ascii_rows(fh, v.astype(np.float64), "%.9g %.9g %.9g\n")
            else:
                rows = np.concatenate([v.astype(np.float64), c.astype(np.float64)], axis=1)
                _ascii_rows(fh, rows, "%.9g %.9g %.9g" + " %d" * c.shape[1] + "\n")
            _ascii_rows(fh, f, "3 %d %d %d\n")
        return
    rows = np.empty(len(f), dtype=_FACE_DTYPE)
    rows["n"] = 3
    rows["idx"] = f
    with open(path, "wb") as fh:
        fh.write(ply_header(len(v), len(f), c))
        if c is None:
            fh.write(v.tobytes())
        else:
            vrows = np.empty(len(v), dtype=_vertex_dtype(c.shape[1]))
            vrows["xyz"] = v
            vrows["rgb"] = c
            fh.write(vrows.tobytes())
        fh.write(rows.tobytes())


def _split_header(path, header_of, what):
    """(data, end of header, n_verts, n_faces, n colour channels) of a file whose header is header_of(V, F, colours)"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    n_verts = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    n_faces = int(next(ln for ln in lines if ln.startswith("element face")).split()[2])
    for n_channels in (0, 3, 4):
        if header_of(n_verts, n_faces, n_channels or None) == data[:end]:
            return data, end, n_verts, n_faces, n_channels
    raise ValueError(f"{path}: not the layout {what} writes")


def _read_binary(path):
    data, end, n_verts, n_faces, n_channels = _split_header(path, ply_header, "write_ply")
    vdt = _vertex_dtype(n_channels)
    vrows = np.frombuffer(data, dtype=vdt, count=n_verts, offset=end)
    rows = np.frombuffer(data, dtype=_FACE_DTYPE, count=n_faces, offset=end + vdt.itemsize * n_verts)
    if n_faces and not (rows["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    colors = vrows["rgb"].copy().reshape(n_verts, n_channels) if n_channels else None
    return vrows["xyz"].copy().reshape(n_verts, 3), rows["idx"].astype(np.int32).reshape(n_faces, 3), colors


def _read_ascii(path):
    data, end, n_verts, n_faces, n_channels = _split_header(path, ply_header_ascii, "write_ply(encoding='ascii')")
    body = data[end:].split(b"\n")
    if len(body) != n_verts + n_faces + 1 or body[-1] != b"":
        raise ValueError(f"{path}: {len(body) - 1} rows, expected {n_verts} + {n_faces}")
    width = 3 + n_channels
    v = np.array(b" ".join(body[:n_verts]).split(), dtype=np.float64)
    rows = np.array(b" ".join(body[n_verts:n_verts + n_faces]).split(), dtype=np.int64)
    if v.size != width * n_verts or rows.size != 4 * n_faces:
        raise ValueError(f"{path}: a row without three coordinates or a face that is not a triangle")
    v = v.reshape(n_verts, width)
    rows = rows.reshape(n_faces, 4)
    if n_faces and not (rows[:, 0] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    colors = v[:, 3:].astype(np.uint8) if n_channels else None
    return v[:, :3].astype(np.float32), rows[:, 1:].astype(np.int32), colors


def read_ply(path):
    """parse back a file of write_ply's layout (triangles only) -> (verts float32 [V, 3], faces int32 [F, 3]); vertex colours,
    if the file has them, are skipped (read_ply_colors returns them)"""
    return _read_binary(path)[:2]


def read_ply_ascii(path):
    """parse back a file of write_ply(encoding="ascii")'s layout (triangles only) -> (verts float32 [V, 3], faces int32 [F, 3])"""
    return _read_ascii(path)[:2]


def read_ply_colors(path):
    """a file of either layout of write_ply -> (verts float32 [V, 3], faces int32 [F, 3], colors uint8 [V, 3 | 4] or None)"""
    with open(path, "rb") as fh:
        ascii_file = fh.read(64).startswith(b"ply\nformat ascii")
    return _read_ascii(path) if ascii_file else _read_binary(path)


