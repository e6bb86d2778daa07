"""Posed views, stated once for ls2fm.raster, ls2fm.mesh_colors and ls2fm.fusion: the conversions of their shared arguments
(views, mesh_arrays, masks, near_plane; `who` is the qualified name of the public function the user called, which the messages name), the
iteration over chunks of views, and the rasteriser's projection as torch ops (project_torch) for the modules' *_torch forms."""
from __future__ import annotations

import functools

import torch

from . import _lib

device = functools.partial(_lib.require_device_tensors, "ls2fm.raster", phrase=": the rasteriser runs on MI355X only")


def views(pose, intr, who):
    """poses float32 [N, 3, 4] and intrinsics float32 [N, 4] = (fx, fy, cx, cy), both contiguous on the pose's device.  Only
    K[0,0], K[1,1], K[0,2] and K[1,2] are taken, with torch ops on the device: no host read.  A chunk is poses[s:e], k4[s:e]."""
    pose, intr = torch.as_tensor(pose), torch.as_tensor(intr)
    device(pose, intr)
    if pose.dim() not in (2, 3) or tuple(pose.shape[-2:]) != (3, 4):
        raise ValueError(f"{who}: pose must be [3, 4] or [V, 3, 4], got {tuple(pose.shape)}")
    poses = _lib.cf(pose.detach().reshape(-1, 3, 4))
    n = int(poses.shape[0])
    if intr.dim() not in (2, 3) or tuple(intr.shape[-2:]) != (3, 3):
        raise ValueError(f"{who}: intr must be [3, 3] or [V, 3, 3], got {tuple(intr.shape)}")
    K = intr.detach().reshape(-1, 3, 3).to(device=poses.device, dtype=torch.float32)
    if K.shape[0] not in (1, n):
        raise ValueError(f"{who}: {K.shape[0]} intrinsics for {n} poses")
    k4 = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], dim=1).expand(n, 4).contiguous()
    return poses, k4


def mesh_arrays(verts, faces, who):
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    device(verts, faces)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"{who}: verts must be [V, 3], got shape {tuple(verts.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: faces must be [F, 3], got shape {tuple(faces.shape)}")
    f = faces if faces.dtype == torch.int32 and faces.is_contiguous() else faces.to(torch.int32).contiguous()
    return _lib.cf(verts.detach()), f


def masks(m, n, who):
    m = torch.as_tensor(m)
    device(m)
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3 or m.shape[0] != n or m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: masks must be bool or uint8 [{n}, H, W], got {m.dtype} {tuple(m.shape)}")
    return m.contiguous().view(torch.uint8)


def near_plane(near, who):
    near = float(near)
    if not (0.0 < near < float("inf")):
        raise ValueError(f"{who}: near {near} must be positive and finite")
    return near


def chunks(n, bytes_per_pixel, H, W, budget, per_chunk=None):
    """the ranges (s, e) that cover n views in order: per_chunk views each, by default as many as keep bytes_per_pixel per
    pixel and view within `budget` bytes at H x W; at least one view per chunk"""
    per_chunk = max(1, int(budget) // (bytes_per_pixel * H * W) if per_chunk is None else int(per_chunk))
    return [(s, min(s + per_chunk, n)) for s in range(0, n, per_chunk)]


def project_torch(P, K, x, y, z, near, H, W):
    """The rasteriser's projection of the points x, y, z (float32 [n] each) into one view (P [3, 4], K [3, 3]) of H x W pixels as
    plain torch ops: the kernels' operations in their order, each a separate op, so each rounds once.  -> (c, u, v, usable, ok,
    px, py): the camera point c = [c_x, c_y, c_z], the projection, usable (c_z finite and >= near, |u| and |v| <= 65536), ok =
    usable and in the image (0 <= u < W, 0 <= v < H), the pixel as int64, zero where not ok.  The rule's other two statements:
    csrc/raster_project.h (the kernels) and tests/raster_restate.py::project (numpy)."""
    c = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
    u = K[0, 0] * (c[0] / c[2]) + K[0, 2]
    v = K[1, 1] * (c[1] / c[2]) + K[1, 2]
    usable = torch.isfinite(c[2]) & (c[2] >= near) & (u.abs() <= 65536.0) & (v.abs() <= 65536.0)
    ok = usable & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    px = torch.where(ok, u.floor(), torch.zeros_like(u)).long()
    py = torch.where(ok, v.floor(), torch.zeros_like(v)).long()
    return c, u, v, usable, ok, px, py
