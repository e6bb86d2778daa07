"""Mesh extraction on the device: marching cubes over a dense volume (ls2fm_marching_cubes_*) and a PLY writer.

Replaces the third-party steps of the reference's extract_mesh (utils/util.py:392-425 -> convert_sigma_samples_to_ply,
util.py:345): skimage.measure.marching_cubes and plyfile.  The case table is generated from one face rule
(tools/gen_mc_tables.py; include/ls2fm.h documents the rule, the vertex arithmetic and the output order).
"""
from __future__ import annotations

import ctypes

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
    if not volume.is_cuda:
        raise RuntimeError("ls2fm.mesh.marching_cubes runs on the GPU only (got a CPU tensor); there is no CPU fallback")
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


def _as_numpy(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1, 3))


def ply_header(n_verts: int, n_faces: int) -> bytes:
    """the header plyfile writes for extract_mesh's two elements (binary, little endian)"""
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {n_verts}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {n_faces}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


def write_ply(path, verts, faces) -> None:
    """write verts [V, 3] / faces [F, 3] (tensors or arrays) in the layout extract_mesh's plyfile branch writes:
    binary_little_endian 1.0, `element vertex` of float x/y/z, `element face` of `property list uchar int vertex_indices`"""
    v = _as_numpy(verts, "<f4")
    f = _as_numpy(faces, "<i4")
    rows = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))      # packed: 13 bytes per face
    rows["n"] = 3
    rows["idx"] = f
    with open(path, "wb") as fh:
        fh.write(ply_header(len(v), len(f)))
        fh.write(v.tobytes())
        fh.write(rows.tobytes())


def read_ply(path):
    """parse back a file of write_ply's layout (triangles only) -> (verts float32 [V, 3], faces int32 [F, 3])"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    n_verts = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    n_faces = int(next(ln for ln in lines if ln.startswith("element face")).split()[2])
    if ply_header(n_verts, n_faces) != data[:end]:
        raise ValueError(f"{path}: not the layout write_ply writes")
    v = np.frombuffer(data, dtype="<f4", count=3 * n_verts, offset=end).reshape(n_verts, 3)
    rows = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), count=n_faces, offset=end + 12 * n_verts)
    if n_faces and not (rows["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    return v.copy(), rows["idx"].astype(np.int32).reshape(n_faces, 3)
