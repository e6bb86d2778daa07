"""Texture atlases for meshes: where ls2fm.mesh_colors stops at one colour per vertex, this module gives every face its own patch
of an image, fills the image from the photographs or the radiance field, renders the textured mesh and writes OBJ + MTL + PNG.

  build_atlas      the parametrisation: per-face right-isosceles charts, two to a square cell, the cells Morton-packed by size
  atlas_texels     the map from texels to surface points and normals (ls2fm_texture_texels, csrc/mesh_texture.hip)
  photo_texture    the texels' points through THE VERTEX COLOUR RULE (ls2fm.mesh_colors.accumulate_views / finish_colors)
  field_texture    the radiance field head-on at the owned texels (ls2fm.mesh_colors.field_colors)
  texture_mesh     photographs where some view sees the texel, the field elsewhere
  render_textured  a rasterize(bary=True) result and the atlas -> images (ls2fm_texture_render); render_views rasterises itself
  write_obj / read_obj, write_png / read_png   the files, with the standard library only

THE ATLAS RULE and THE TEXTURE RENDER RULE are stated in include/ls2fm.h and restated in numpy in tests/texture_restate.py.  A face's
chart is found by arithmetic alone -- no search structure, no atomic, no ordering -- so texel points, and with them the texture,
are a pure function of the mesh, `texel`, `gutter` and the size.  Deviations from what texturing packages do, on purpose: no chart
merging (a seam between every pair of faces; colour stays continuous across it because both sides sample the same surface points
through the same rule), about 1 - L^2 / p^2 of the area spent on gutters, faces longer than the largest pitch undersampled, no
seam levelling or exposure compensation, no mip chain, 8-bit PNG.

CPU tensors take the same rules as torch ops (_texels_torch, render_textured_torch: the bits of the kernels); the rasteriser
has no CPU form, so a CPU call of photo_texture is handed the depth maps.
"""
from __future__ import annotations

import ctypes
import math
import os
import struct
import zlib
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, _posed, mesh_colors, raster
from ._lib import check, ptr, stream_ptr

MAX_SIZE = 32768
BISECT_STEPS = 20


class TextureAtlas(NamedTuple):
    """size S; gutter; texel (world units per texel); uv float32 [F, 3, 2], the corners in texel coordinates (half-integers), in the
    face's own vertex order; order int32 [F], order[slot] = face; rot int32 [F], the vertex on the chart's right angle; classes, a
    tuple of (k, faces) over every admissible pitch 2^k, descending; max_pitch"""
    size: int
    gutter: int
    texel: float
    uv: torch.Tensor
    order: torch.Tensor
    rot: torch.Tensor
    classes: tuple
    max_pitch: int


class Texels(NamedTuple):
    """face int32 [rows, S] (-1: unowned), point float32 [rows, S, 3], normal float32 [rows, S, 3] (not normalised); NaN where unowned"""
    face: torch.Tensor
    point: torch.Tensor
    normal: torch.Tensor


class Texture(NamedTuple):
    """texture float32 [S, S, C]; count int32 [S, S], the views that coloured each texel (0: it carries fill or the fallback)"""
    texture: torch.Tensor
    count: torch.Tensor


# ------------------------------------------------------------------------------------------------------------------ the atlas
def class_range(gutter, max_pitch=256):
    """the admissible classes k, ascending: 2 gutter + 4 <= 2^k <= max_pitch"""
    gutter, max_pitch = int(gutter), int(max_pitch)
    if not 0 <= gutter <= 64:
        raise ValueError(f"ls2fm.texture: gutter {gutter} outside 0 .. 64")
    if max_pitch < 4 or max_pitch > MAX_SIZE or max_pitch & (max_pitch - 1):
        raise ValueError(f"ls2fm.texture: max_pitch {max_pitch} must be a power of two in [4, {MAX_SIZE}]")
    k = 2
    while (1 << k) < 2 * gutter + 4:
        k += 1
    ks = list(range(k, max_pitch.bit_length()))
    if not ks or len(ks) > 8:
        raise ValueError(f"ls2fm.texture: gutter {gutter} and max_pitch {max_pitch} leave {len(ks)} pitches; 1 .. 8 are served")
    return ks


def class_thresholds(texel, gutter, ks):
    """T_k = ((2^k - 2 gutter - 3) texel)^2 in Python floats: the product, then its square"""
    out = []
    for k in ks:
        t = ((1 << k) - 2 * gutter - 3) * float(texel)
        out.append(t * t)
    return out


def _corners(verts, faces):
    """float32 [F, 3, 3]: every face's corners, NaN for a face with an index outside [0, V)"""
    n_v = int(verts.shape[0])
    idx = faces.long()
    in_range = ((idx >= 0) & (idx < n_v)).all(dim=1)
    if n_v == 0:
        return torch.full((idx.shape[0], 3, 3), float("nan"), dtype=torch.float32, device=verts.device)
    P = verts[torch.where(in_range[:, None], idx, torch.zeros_like(idx))]
    return torch.where(in_range[:, None, None], P, torch.full_like(P, float("nan")))


def _rotation_and_legs(verts, faces):
    """rot int32 [F], l2 float64 [F] (the larger squared leg at the chart's right angle), finite bool [F]: the rule's fp64 sums,
    products and comparisons as separate torch ops"""
    P = _corners(verts, faces)

    def edge(a, b):
        d = (P[:, b] - P[:, a]).to(torch.float64)
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    e0, e1, e2 = edge(1, 2), edge(2, 0), edge(0, 1)
    rot = torch.zeros(P.shape[0], dtype=torch.int32, device=P.device)
    up = e1 > e0
    rot = torch.where(up, torch.ones_like(rot), rot)
    best = torch.where(up, e1, e0)
    rot = torch.where(e2 > best, torch.full_like(rot, 2), rot)
    legs = torch.stack([torch.maximum(e1, e2), torch.maximum(e2, e0), torch.maximum(e0, e1)], dim=1)
    l2 = legs.gather(1, rot.long()[:, None])[:, 0]
    return rot, l2, torch.isfinite(P).all(dim=2).all(dim=1)


def _classes_of(l2, finite, texel, gutter, ks):
    cls = torch.full(l2.shape, ks[-1], dtype=torch.int32, device=l2.device)
    for k, thr in reversed(list(zip(ks, class_thresholds(texel, gutter, ks)))):
        cls = torch.where(l2 <= thr, torch.full_like(cls, k), cls)
    return torch.where(finite, cls, torch.full_like(cls, ks[0]))


def _histogram(cls, ks):
    """(k, faces) over every admissible k, descending: ONE host read"""
    counts = torch.bincount(cls.long() - ks[0], minlength=len(ks)).tolist() if cls.numel() else [0] * len(ks)
    return tuple((k, int(counts[k - ks[0]])) for k in reversed(ks))


def layout(classes):
    """per class: Morton offset of its first cell, its cells, its first slot; and the total area in texels"""
    starts, cells, slots = [], [], []
    at, slot = 0, 0
    for k, count in classes:
        starts.append(at)
        cells.append((count + 1) // 2)
        slots.append(slot)
        at += cells[-1] << (2 * k)
        slot += count
    return starts, cells, slots, at


def _interleave(x, y):
    m = torch.zeros_like(x)
    for b in range(16):
        m = m | (((x >> b) & 1) << (2 * b)) | (((y >> b) & 1) << (2 * b + 1))
    return m


def _deinterleave(m):
    x, y = torch.zeros_like(m), torch.zeros_like(m)
    for b in range(16):
        x = x | (((m >> (2 * b)) & 1) << b)
        y = y | (((m >> (2 * b + 1)) & 1) << b)
    return x, y


def _chart_corners(order, rot, classes, gutter):
    """uv float32 [F, 3, 2] from the packing alone, with torch ops on the packing's device: nothing read back"""
    dev = order.device
    uv = torch.zeros(order.shape[0], 3, 2, dtype=torch.float32, device=dev)
    starts, _, slots, _ = layout(classes)
    for (k, count), start, slot0 in zip(classes, starts, slots):
        if count == 0:
            continue
        p, L = 1 << k, (1 << k) - 2 * gutter - 3
        s = torch.arange(count, dtype=torch.int64, device=dev)
        x0, y0 = _deinterleave(start + ((s // 2) << (2 * k)))
        second = (s % 2) == 1
        f = order[slot0:slot0 + count].long()
        r = rot[f].long()
        for q, (ci, cj) in enumerate(((gutter, gutter), (gutter + L, gutter), (gutter, gutter + L))):
            x = x0 + torch.where(second, p - 1 - ci, ci)
            y = y0 + torch.where(second, p - 1 - cj, cj)
            uv[f, (r + q) % 3] = torch.stack([x.float() + 0.5, y.float() + 0.5], dim=1)
    return uv


@torch.no_grad()
def build_atlas(verts, faces, texel=None, size=None, gutter=1, max_pitch=256) -> TextureAtlas:
    """THE ATLAS RULE's parametrisation of a mesh (verts float32 [V, 3], faces int32 [F, 3]; device or CPU tensors) -> TextureAtlas.
      texel      world units per texel: a face's class is the smallest pitch whose chart holds its longer leg at this density
      size       the atlas is size x size, a power of two in [4, 32768]
      gutter     texels of gutter on the charts' straight sides (and the cell's diagonal keeps the bilinear taps apart)
      max_pitch  the largest pitch; a face longer than (max_pitch - 2 gutter - 3) texel is undersampled
    texel given, size None: the smallest size that holds the cells.  size given, texel None: the smallest texel of a fixed
    bisection that fits -- BISECT_STEPS steps on log(texel) between 2^-20 of the mesh's longest leg and that leg, where every face
    is of the smallest class.  Both given: ValueError unless it fits.
    Torch ops only: the fp32 differences, the fp64 squared lengths and their comparisons against thresholds formed on the host, a
    stable sort.  Host reads: one class histogram per evaluation -- 1 with texel given; with texel=None the longest leg, the
    histogram at that leg and one per step, 2 + BISECT_STEPS = 22 in all.  Face indices outside [0, V) are no error: such a face has
    NaN corners, takes the smallest class and NaN texels."""
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"ls2fm.texture.build_atlas: verts [V, 3] and faces [F, 3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if faces.device != verts.device:
        raise ValueError(f"ls2fm.texture.build_atlas: verts on {verts.device}, faces on {faces.device}")
    gutter, max_pitch = int(gutter), int(max_pitch)
    ks = class_range(gutter, max_pitch)
    v = _lib.cf(verts.detach())
    if size is not None:
        size = int(size)
        if size < 4 or size > MAX_SIZE or size & (size - 1):
            raise ValueError(f"ls2fm.texture.build_atlas: size {size} must be a power of two in [4, {MAX_SIZE}]")
    if texel is None and size is None:
        raise ValueError("ls2fm.texture.build_atlas: give texel, size or both")
    rot, l2, finite = _rotation_and_legs(v, faces)

    def evaluate(t):
        cls = _classes_of(l2, finite, t, gutter, ks)
        classes = _histogram(cls, ks)
        return cls, classes, layout(classes)[3]
    if texel is not None:
        texel = float(texel)
        if not (0.0 < texel < float("inf")):
            raise ValueError(f"ls2fm.texture.build_atlas: texel {texel} must be positive and finite")
        cls, classes, area = evaluate(texel)
        if size is None:
            size = 4
            while size * size < area:
                size *= 2
            if size > MAX_SIZE:
                raise ValueError(f"ls2fm.texture.build_atlas: texel {texel} needs {area} texels, more than {MAX_SIZE}^2")
        elif area > size * size:
            raise ValueError(f"ls2fm.texture.build_atlas: texel {texel} needs {area} texels, the atlas has {size}^2")
    else:
        usable = finite & torch.isfinite(l2)
        longest = math.sqrt(float(torch.where(usable, l2, torch.zeros_like(l2)).max())) if l2.numel() else 0.0
        if not longest > 0.0:
            longest = 1.0                                          # nothing to measure: any texel gives the smallest class
        hi, lo = longest, longest * 2.0 ** -20
        best = evaluate(hi)
        if best[2] > size * size:
            raise ValueError(f"ls2fm.texture.build_atlas: {int(faces.shape[0])} faces need {best[2]} texels at the smallest pitch, "
                             f"the atlas has {size}^2")
        for _ in range(BISECT_STEPS):
            mid = math.sqrt(lo * hi)
            got = evaluate(mid)
            if got[2] <= size * size:
                hi, best = mid, got
            else:
                lo = mid
        texel, (cls, classes, area) = hi, best
    # stable and descending: equal classes keep the faces' order
    order = torch.sort(ks[-1] - cls, stable=True).indices.to(torch.int32)
    return TextureAtlas(size, gutter, texel, _chart_corners(order, rot, classes, gutter), order, rot, classes, max_pitch)


def _texels_torch(atlas, verts, faces, rows=None, uv=None) -> Texels:
    """ls2fm_texture_texels as plain torch ops on whatever device the tensors are on, one op per rounded operation: the bits of
    the kernel.  The form CPU tensors take, the timing baseline and a check."""
    S, g = atlas.size, atlas.gutter
    r0, r1 = (0, S) if rows is None else (int(rows[0]), int(rows[1]))
    dev = verts.device
    v = _lib.cf(verts.detach())
    y, x = torch.meshgrid(torch.arange(r0, r1, dtype=torch.int64, device=dev), torch.arange(S, dtype=torch.int64, device=dev), indexing="ij")
    face = torch.full((r1 - r0, S), -1, dtype=torch.int32, device=dev)
    point = torch.full((r1 - r0, S, 3), float("nan"), dtype=torch.float32, device=dev)
    if faces.shape[0] == 0 or r1 == r0:
        return Texels(face, point, point.clone())
    m = _interleave(x, y)
    starts, cells, slots, _ = layout(atlas.classes)
    c = torch.zeros_like(m)
    for i, s in enumerate(starts):
        c = torch.where(m >= s, torch.full_like(c, i), c)
    tab = lambda vals: torch.tensor(vals, dtype=torch.int64, device=dev)[c]
    k = tab([t[0] for t in atlas.classes])
    p = torch.ones_like(k) << k
    cell = (m - tab(starts)) >> (2 * k)
    i, j = x & (p - 1), y & (p - 1)
    second = i + j > p - 1
    slot = tab(slots) + 2 * cell + second.long()
    owned = (cell < tab(cells)) & (slot < tab(slots) + tab([t[1] for t in atlas.classes]))
    f = atlas.order.long()[torch.where(owned, slot, torch.zeros_like(slot))]
    owned = owned & (f >= 0) & (f < faces.shape[0])
    f = torch.where(owned, f, torch.zeros_like(f))
    ii, jj = torch.where(second, p - 1 - i, i), torch.where(second, p - 1 - j, j)
    L = p - 2 * g - 3
    s = ((ii - g).float() / L.float())[..., None]
    t = ((jj - g).float() / L.float())[..., None]
    P = _corners(v, faces)[f]                                           # [rows, S, 3, 3]
    r = atlas.rot.long().clamp(0, 2)[f]
    pick = lambda q: P.gather(2, ((r + q) % 3)[..., None, None].expand(*r.shape, 1, 3))[..., 0, :]
    a, b, cc = pick(0), pick(1), pick(2)
    d1, d2 = b - a, cc - a
    X = (a + s * d1) + t * d2
    n = torch.stack([d1[..., 1] * d2[..., 2] - d1[..., 2] * d2[..., 1], d1[..., 2] * d2[..., 0] - d1[..., 0] * d2[..., 2],
                     d1[..., 0] * d2[..., 1] - d1[..., 1] * d2[..., 0]], dim=-1)
    nan = torch.full_like(X, float("nan"))
    if uv is not None:
        for q, (ci, cj) in enumerate(((g, g), (g + L, g), (g, g + L))):
            at = owned & (ii == ci) & (jj == cj)
            uv[f[at], ((r + q) % 3)[at]] = torch.stack([x[at].float() + 0.5, y[at].float() + 0.5], dim=1)
    return Texels(torch.where(owned, f.to(torch.int32), face), torch.where(owned[..., None], X, nan), torch.where(owned[..., None], n, nan))


def _class_arrays(atlas):
    n = len(atlas.classes)
    return n, (ctypes.c_int32 * n)(*[k for k, _ in atlas.classes]), (ctypes.c_int64 * n)(*[c for _, c in atlas.classes])


def _band(atlas, rows, who):
    r0, r1 = (0, atlas.size) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 <= r1 <= atlas.size:
        raise ValueError(f"{who}: rows {(r0, r1)} outside 0 <= begin <= end <= {atlas.size}")
    return r0, r1


@torch.no_grad()
def atlas_texels(atlas, verts, faces, rows=None, uv=None) -> Texels:
    """The surface point and normal of every texel of the rows [rows[0], rows[1]) of the atlas (None: all) -> Texels.  uv: a float32
    [F, 3, 2] tensor that takes the corners the band's corner texels hold (over all bands: atlas.uv), or None.  Device tensors:
    one ls2fm_texture_texels launch, nothing read back, so the call can be captured; bands leave the bits of one call.  CPU
    tensors: _texels_torch."""
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    r0, r1 = _band(atlas, rows, "ls2fm.texture.atlas_texels")
    if faces.dim() != 2 or faces.shape[1] != 3 or int(faces.shape[0]) != int(atlas.order.shape[0]):
        raise ValueError(f"ls2fm.texture.atlas_texels: faces {tuple(faces.shape)} for an atlas of {int(atlas.order.shape[0])} faces")
    if uv is not None and (tuple(uv.shape) != (int(faces.shape[0]), 3, 2) or uv.dtype != torch.float32 or not uv.is_contiguous()
                           or uv.device != verts.device):
        raise ValueError(f"ls2fm.texture.atlas_texels: uv must be contiguous float32 [{int(faces.shape[0])}, 3, 2] on {verts.device}")
    if not verts.is_cuda:
        return _texels_torch(atlas, verts, faces, (r0, r1), uv)
    lib = _lib.load()
    v, f = _posed.mesh_arrays(verts, faces, "ls2fm.texture.atlas_texels")
    dev, S = v.device, atlas.size
    order, rot = atlas.order.contiguous(), atlas.rot.contiguous()
    if order.device != dev or rot.device != dev or f.device != dev:
        raise ValueError(f"ls2fm.texture.atlas_texels: verts on {dev}, faces on {f.device}, the atlas on {order.device}")
    n, ks, counts = _class_arrays(atlas)
    with torch.cuda.device(dev):
        face = torch.empty(r1 - r0, S, dtype=torch.int32, device=dev)
        point = torch.empty(r1 - r0, S, 3, dtype=torch.float32, device=dev)
        normal = torch.empty(r1 - r0, S, 3, dtype=torch.float32, device=dev)
        check(lib.ls2fm_texture_texels(ptr(v), int(v.shape[0]), ptr(f), int(f.shape[0]), ptr(order), ptr(rot), n, ks, counts, atlas.gutter,
                                       S, r0, r1, ptr(face), ptr(point), ptr(normal), ptr(uv), stream_ptr()), "ls2fm_texture_texels")
    return Texels(face, point, normal)


# ------------------------------------------------------------------------------------------------------------------ filling
def _row_bands(S, bytes_per_texel, row_chunk, budget=2 ** 28):
    rows = max(1, int(budget) // (bytes_per_texel * S) if row_chunk is None else int(row_chunk))
    return [(s, min(s + rows, S)) for s in range(0, S, rows)]


@torch.no_grad()
def photo_texture(verts, faces, atlas, pose, intr, images, masks=None, weights="face", near=1e-3, depth_tol=1e-2, power=1,
                  fill=(0.5, 0.5, 0.5), fallback=None, view_chunk=None, row_chunk=None, depth=None) -> Texture:
    """The atlas's texture from photographs -> Texture(texture float32 [S, S, C], count int32 [S, S]): every texel's point as a
    "vertex" of THE VERTEX COLOUR RULE (ls2fm.mesh_colors), z-tested against the rasteriser's depth maps of the mesh.
      pose, intr, images, masks, near, depth_tol, power   as ls2fm.mesh_colors.photo_colors
      weights     "face": a view weighs cos^power of the angle between the chart's normal (b - a) x (c - a) and the direction to the
                  camera, and does not count where cos <= 0.  The normal follows the face's winding; ls2fm.mesh.marching_cubes
                  winds its faces so that it points from the inside (negative values) to the outside (tests/test_texture_host.py
                  checks this on the sphere scene), so cos > 0 is the side the cameras of an extracted surface are on.  None:
                  every view weighs 1, whatever side it is on.
      fill, fallback  the colour of a texel no view counts for: fallback [S, S, C], else fill.  Unowned texels have NaN points,
                  which the rule skips in every view: they take it too.
      view_chunk  views per chunk, as photo_colors; row_chunk: atlas rows per band (None: what keeps a band's points, normals and
                  state within 256 MiB).  The state is carried across the view chunks of a band and bands are independent, so
                  neither shows in the bits.
      depth       [N, H, W]: the rasteriser's depth maps, if the caller holds them; required for CPU tensors.  Otherwise they
                  are rasterised once when all of them fit 256 MiB, else per band and chunk of views.
    Device tensors: per band one ls2fm_texture_texels launch, per chunk one ls2fm_mesh_vertex_colors launch, then the finish; no
    host read."""
    if weights not in ("face", None):
        raise ValueError(f"ls2fm.texture.photo_texture: weights must be 'face' or None, got {weights!r}")
    depth_tol, power = mesh_colors._check_photo_args(depth_tol, power)
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    S = atlas.size
    images_t = torch.as_tensor(images)
    C = int(images_t.shape[-1])
    if fallback is not None:
        fallback = _lib.cf(torch.as_tensor(fallback).detach())
        if tuple(fallback.shape) != (S, S, C):
            raise ValueError(f"ls2fm.texture.photo_texture: fallback must be [{S}, {S}, {C}], got {tuple(fallback.shape)}")
    bands = _row_bands(S, 24 + 8 * (C + 1) + 4 + 4 * C, row_chunk)
    if not verts.is_cuda:
        if depth is None:
            raise RuntimeError("ls2fm.texture.photo_texture: CPU tensors need the depth maps (depth=...): the rasteriser runs on "
                               "MI355X only")
        tex, cnt = [], []
        for r0, r1 in bands:
            tx = _texels_torch(atlas, verts, faces, (r0, r1))
            got = mesh_colors.photo_colors_torch(tx.point.reshape(-1, 3), pose, intr, images_t, depth, masks,
                                                 tx.normal.reshape(-1, 3) if weights == "face" else None, near, depth_tol, power, fill,
                                                 None if fallback is None else fallback[r0:r1].reshape(-1, C))
            tex.append(got.colors.view(r1 - r0, S, C))
            cnt.append(got.count.view(r1 - r0, S))
        return Texture(torch.cat(tex), torch.cat(cnt))
    who = "ls2fm.texture.photo_texture"
    v, f = _posed.mesh_arrays(verts, faces, who)
    poses, k4 = _posed.views(pose, intr, who)
    n, dev = int(poses.shape[0]), v.device
    img = mesh_colors._images(images_t, n, "photo_texture")
    H, W = int(img.shape[1]), int(img.shape[2])
    m = None if masks is None else _posed.masks(masks, n, who)
    if m is not None and tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"{who}: masks of {tuple(m.shape[1:])} for images of {(H, W)}")
    near = _posed.near_plane(near, who)
    if depth is not None:
        depth = _lib.cf(torch.as_tensor(depth).detach())
        if tuple(depth.shape) != (n, H, W):
            raise ValueError(f"{who}: depth must be [{n}, {H}, {W}], got {tuple(depth.shape)}")
    for t in (poses, img, m, depth, fallback):
        if t is not None and t.device != dev:
            raise ValueError(f"{who}: verts on {dev}, another argument on {t.device}")
    with torch.cuda.device(dev):
        if depth is None and 4 * n * H * W <= 2 ** 28:
            depth = raster.rasterize_prepared(v, f, poses, k4, H, W, near).depth
        texture = torch.empty(S, S, C, dtype=torch.float32, device=dev)
        count = torch.empty(S, S, dtype=torch.int32, device=dev)
        for r0, r1 in bands:
            tx = atlas_texels(atlas, v, f, (r0, r1))
            pts = tx.point.view(-1, 3)
            nrm = tx.normal.view(-1, 3) if weights == "face" else None
            state = (torch.zeros(pts.shape[0], C + 1, dtype=torch.float64, device=dev), torch.zeros(pts.shape[0], dtype=torch.int32, device=dev))
            for s, e in _posed.chunks(n, 8, H, W, 2 ** 28, view_chunk):
                d = depth[s:e] if depth is not None else raster.rasterize_prepared(v, f, poses[s:e], k4[s:e], H, W, near).depth
                mesh_colors.accumulate_views(state, pts, (poses[s:e], k4[s:e]), img[s:e], d, None if m is None else m[s:e], nrm, near,
                                             depth_tol, power)
            fb = None if fallback is None else fallback[r0:r1].reshape(-1, C)
            texture[r0:r1] = mesh_colors.finish_colors(state, C, fill, fb).view(r1 - r0, S, C)
            count[r0:r1] = state[1].view(r1 - r0, S)
    return Texture(texture, count)


@torch.no_grad()
def field_texture(opt, sdf_field, rad_field, verts, faces, atlas, fill=(0.5, 0.5, 0.5), row_chunk=None) -> torch.Tensor:
    """The atlas's texture from the radiance field -> float32 [S, S, 3]: ls2fm.mesh_colors.field_colors head-on (v = -normalize(g))
    at the owned texels' points, `fill` at the unowned ones.  The owned texels of a band are gathered with a boolean mask (one
    host read per band), so the field is evaluated on them alone.  row_chunk: atlas rows per band (None: 256 MiB of points)."""
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    S = atlas.size
    out = torch.tensor(mesh_colors._fill(fill, 3), dtype=torch.float32, device=verts.device).expand(S, S, 3).contiguous()
    for r0, r1 in _row_bands(S, 28 + 24, row_chunk):
        tx = atlas_texels(atlas, verts, faces, (r0, r1))
        owned = tx.face >= 0
        pts = tx.point[owned]
        if pts.shape[0]:
            out[r0:r1][owned] = mesh_colors.field_colors(opt, sdf_field, rad_field, pts)
    return out


@torch.no_grad()
def texture_mesh(opt, sdf_field, rad_field, verts, faces, atlas, pose, intr, images, masks=None, near=1e-3, depth_tol=1e-2, power=1,
                 view_chunk=None, row_chunk=None, depth=None) -> Texture:
    """Photographs where some view sees the texel, the radiance field elsewhere -> Texture (texture [S, S, 3]), as
    ls2fm.mesh_colors.color_mesh does per vertex.  The views are weighted by the chart normals; count == 0 marks the texels that
    carry the field's colour (or, unowned, its fill)."""
    field = field_texture(opt, sdf_field, rad_field, verts, faces, atlas, row_chunk=row_chunk)
    return photo_texture(verts, faces, atlas, pose, intr, images, masks=masks, weights="face", near=near, depth_tol=depth_tol, power=power,
                         fallback=field, view_chunk=view_chunk, row_chunk=row_chunk, depth=depth)


# ------------------------------------------------------------------------------------------------------------------ rendering
def _render_args(atlas, texture, face_id, bary, who):
    texture, face_id, bary = torch.as_tensor(texture), torch.as_tensor(face_id), torch.as_tensor(bary)
    S = atlas.size
    if texture.dim() != 3 or tuple(texture.shape[:2]) != (S, S) or not 1 <= texture.shape[2] <= 4:
        raise ValueError(f"{who}: texture must be [{S}, {S}, C] with C from 1 to 4, got {tuple(texture.shape)}")
    if face_id.dim() == 2:
        face_id, bary = face_id[None], bary[None]
    if face_id.dim() != 3 or tuple(bary.shape) != tuple(face_id.shape) + (3,):
        raise ValueError(f"{who}: face_id [V, H, W] and bary [V, H, W, 3], got {tuple(face_id.shape)} and {tuple(bary.shape)}")
    return _lib.cf(texture.detach()), face_id.to(torch.int32).contiguous(), _lib.cf(bary.detach())


def render_textured_torch(atlas, texture, raster_out, background=(0.0, 0.0, 0.0)):
    """THE TEXTURE RENDER RULE as plain torch ops on whatever device the tensors are on, one op per rounded operation: the bits of
    ls2fm_texture_render.  The form CPU tensors take, the timing baseline and a check."""
    tex, face_id, bary = _render_args(atlas, texture, raster_out.face_id, raster_out.bary, "ls2fm.texture.render_textured_torch")
    S, C, dev = atlas.size, int(tex.shape[2]), tex.device
    uv = atlas.uv.to(dev)
    n_f = int(uv.shape[0])
    out = torch.tensor(mesh_colors._fill(background, C), dtype=torch.float32, device=dev).expand(*face_id.shape, C).contiguous()
    ok = (face_id >= 0) & (face_id < n_f)
    if n_f == 0 or not bool(ok.any()):
        return out
    c = uv[torch.where(ok, face_id, torch.zeros_like(face_id)).long()]                   # [V, H, W, 3, 2]
    w = bary
    xy = (w[..., 0, None] * c[..., 0, :] + w[..., 1, None] * c[..., 1, :]) + w[..., 2, None] * c[..., 2, :]

    def axis(u):
        s = u - 0.5
        u0 = s.floor()
        t = s - u0
        u0 = torch.where(torch.isnan(u0), torch.full_like(u0, -1.0), u0.clamp(-1.0, float(S))).long()
        return u0.clamp(0, S - 1), (u0 + 1).clamp(0, S - 1), t[..., None]
    x0, x1, tx = axis(xy[..., 0])
    y0, y1, ty = axis(xy[..., 1])
    flat = tex.view(S * S, C)
    b00, b10, b01, b11 = flat[y0 * S + x0], flat[y0 * S + x1], flat[y1 * S + x0], flat[y1 * S + x1]
    r0 = b00 + tx * (b10 - b00)
    r1 = b01 + tx * (b11 - b01)
    return torch.where(ok[..., None], r0 + ty * (r1 - r0), out)


@torch.no_grad()
def render_textured(atlas, texture, raster_out, background=(0.0, 0.0, 0.0)):
    """Images of the textured mesh from a rasterisation: raster_out is what ls2fm.raster.rasterize(..., bary=True) returned (face_id
    int32 [V, H, W], bary float32 [V, H, W, 3]); texture float32 [S, S, C], C from 1 to 4 -> float32 [V, H, W, C], the layout
    ls2fm.image_metrics.compare_images takes.  Pixels no face covers (and face ids outside the atlas) take `background` (a scalar
    or a sequence; a shorter one is extended with 1).  One ls2fm_texture_render launch, nothing read back.  CPU tensors:
    render_textured_torch."""
    if raster_out.bary is None:
        raise ValueError("ls2fm.texture.render_textured: the rasterisation carries no barycentrics: rasterize(..., bary=True)")
    tex, face_id, bary = _render_args(atlas, texture, raster_out.face_id, raster_out.bary, "ls2fm.texture.render_textured")
    if not tex.is_cuda:
        return render_textured_torch(atlas, texture, raster_out, background)
    lib = _lib.load()
    dev, C = tex.device, int(tex.shape[2])
    uv = atlas.uv.contiguous()
    if face_id.device != dev or bary.device != dev or uv.device != dev:
        raise ValueError(f"ls2fm.texture.render_textured: texture on {dev}, face_id on {face_id.device}, the atlas on {uv.device}")
    V, H, W = (int(s) for s in face_id.shape)
    bg = (ctypes.c_float * C)(*mesh_colors._fill(background, C))
    with torch.cuda.device(dev):
        out = torch.empty(V, H, W, C, dtype=torch.float32, device=dev)
        check(lib.ls2fm_texture_render(ptr(face_id), ptr(bary), V, H, W, ptr(uv), int(uv.shape[0]), ptr(tex), atlas.size, C, bg, ptr(out),
                                       stream_ptr()), "ls2fm_texture_render")
    return out


@torch.no_grad()
def render_views(verts, faces, atlas, texture, pose, intr, H, W, near=1e-3, background=(0.0, 0.0, 0.0), view_chunk=None):
    """Rasterise the mesh into the views (ls2fm.raster.rasterize with barycentrics) and render the texture -> float32 [V, H, W, C].
    view_chunk: views per chunk (None: what keeps a chunk's face ids and barycentrics within 256 MiB)."""
    v, f = _posed.mesh_arrays(verts, faces, "ls2fm.texture.render_views")
    poses, k4 = _posed.views(pose, intr, "ls2fm.texture.render_views")
    out = []
    for s, e in _posed.chunks(int(poses.shape[0]), 28, int(H), int(W), 2 ** 28, view_chunk):
        out.append(render_textured(atlas, texture, raster.rasterize_prepared(v, f, poses[s:e], k4[s:e], H, W, near, bary=True), background))
    return torch.cat(out) if out else torch.empty(0, int(H), int(W), int(torch.as_tensor(texture).shape[2]), device=v.device)


# ------------------------------------------------------------------------------------------------------------------ files
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
_PNG_TYPES = {1: 0, 2: 4, 3: 2, 4: 6}                       # channels -> PNG colour type: grey, grey + alpha, RGB, RGBA


def texture_bytes(texture) -> np.ndarray:
    """a texture [H, W, C] as the bytes write_png stores: a uint8 array as it is, anything else ls2fm.mesh.color_bytes' rounding,
    round(clip(c, 0, 1) * 255) with halves to even, a NaN becoming 0"""
    if isinstance(texture, torch.Tensor):
        texture = texture.detach().cpu().numpy()
    t = np.asarray(texture)
    if t.ndim == 2:
        t = t[..., None]
    if t.ndim != 3 or not 1 <= t.shape[2] <= 4:
        raise ValueError(f"ls2fm.texture.write_png: the image must be [H, W, C] with C from 1 to 4, got {tuple(t.shape)}")
    if t.dtype == np.uint8:
        return np.ascontiguousarray(t)
    with np.errstate(invalid="ignore"):
        return np.rint(np.clip(np.nan_to_num(t.astype(np.float64), nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, texture):
    """an 8-bit PNG of texture [H, W, C] (C = 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA), row 0 on top: standard library only (zlib,
    struct), filter type 0 on every row.  The bytes are a function of the image alone."""
    b = texture_bytes(texture)
    H, W, C = b.shape
    rows = np.concatenate([np.zeros((H, 1), np.uint8), b.reshape(H, W * C)], axis=1)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, _PNG_TYPES[C], 0, 0, 0))
                + _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 9)) + _png_chunk(b"IEND", b""))


def read_png(path) -> np.ndarray:
    """uint8 [H, W, C] of a PNG as write_png writes them: 8 bits, not interlaced, not paletted, filter type 0 on every row"""
    with open(path, "rb") as f:
        blob = f.read()
    if blob[:8] != _PNG_MAGIC:
        raise ValueError(f"ls2fm.texture.read_png: {path} is not a PNG")
    at, header, data = 8, None, b""
    while at < len(blob):
        n, = struct.unpack_from(">I", blob, at)
        tag, body = blob[at + 4:at + 8], blob[at + 8:at + 8 + n]
        crc, = struct.unpack_from(">I", blob, at + 8 + n)
        if zlib.crc32(tag + body) & 0xFFFFFFFF != crc:
            raise ValueError(f"ls2fm.texture.read_png: {path}: chunk {tag!r} fails its CRC")
        if tag == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            data += body
        at += 12 + n
    if header is None:
        raise ValueError(f"ls2fm.texture.read_png: {path} has no IHDR")
    W, H, bits, ctype, _, _, interlace = header
    channels = {v: k for k, v in _PNG_TYPES.items()}.get(ctype)
    if bits != 8 or channels is None or interlace:
        raise ValueError(f"ls2fm.texture.read_png: {path}: only 8-bit grey / RGB (with alpha), not interlaced, is read")
    rows = np.frombuffer(zlib.decompress(data), np.uint8).reshape(H, 1 + W * channels)
    if rows[:, 0].any():
        raise ValueError(f"ls2fm.texture.read_png: {path} uses row filters; only filter type 0 is read")
    return rows[:, 1:].reshape(H, W, channels).copy()


def _stem(path):
    path = os.fspath(path)
    return path[:-4] if path.lower().endswith(".obj") else path


def write_obj(path, verts, faces, atlas, texture):
    """<stem>.obj (v, vt, f v/vt; one vt per face corner: the charts share none), <stem>.mtl (one material, map_Kd) and <stem>.png
    (write_png of the texture).  vt = (x / S, 1 - y / S) of the corner's texel coordinates: S is a power of two and the corners are
    half-integers, so the decimals written are exact.  Vertices are written with 9 significant digits (float32 round-trips).
    -> the three paths"""
    stem = _stem(path)
    name = os.path.basename(stem)
    v = torch.as_tensor(verts).detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
    f = torch.as_tensor(faces).detach().cpu().numpy().astype(np.int64).reshape(-1, 3)
    uv = atlas.uv.detach().cpu().numpy().astype(np.float64)
    if uv.shape[0] != f.shape[0]:
        raise ValueError(f"ls2fm.texture.write_obj: {f.shape[0]} faces for an atlas of {uv.shape[0]}")
    S = float(atlas.size)
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(t) for t in p) for p in v]
    lines += [f"vt {float(x) / S!r} {1.0 - float(y) / S!r}" for x, y in uv.reshape(-1, 2)]
    lines += ["f " + " ".join(f"{int(a) + 1}/{3 * i + c + 1}" for c, a in enumerate(tri)) for i, tri in enumerate(f)]
    with open(stem + ".obj", "w", newline="\n") as out:
        out.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w", newline="\n") as out:
        out.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    write_png(stem + ".png", texture)
    return stem + ".obj", stem + ".mtl", stem + ".png"


def read_obj(path):
    """what write_obj wrote -> dict(verts float32 [V, 3], faces int32 [F, 3], uv float32 [F, 3, 2] (texel coordinates), size,
    texture uint8 [S, S, C])"""
    stem = _stem(path)
    v, vt, f, ft, mtl = [], [], [], [], None
    with open(stem + ".obj") as src:
        for line in src:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                v.append([float(t) for t in tok[1:4]])
            elif tok[0] == "vt":
                vt.append([float(t) for t in tok[1:3]])
            elif tok[0] == "f":
                pairs = [t.split("/") for t in tok[1:4]]
                f.append([int(p[0]) - 1 for p in pairs])
                ft.append([int(p[1]) - 1 for p in pairs])
            elif tok[0] == "mtllib":
                mtl = tok[1]
    png = None
    with open(os.path.join(os.path.dirname(stem), mtl)) as src:
        for line in src:
            tok = line.split()
            if tok and tok[0] == "map_Kd":
                png = tok[1]
    texture = read_png(os.path.join(os.path.dirname(stem), png))
    S = texture.shape[0]
    vt = np.asarray(vt, np.float64).reshape(-1, 2)
    corners = vt[np.asarray(ft, np.int64).reshape(-1, 3)] if len(ft) else np.zeros((0, 3, 2))
    uv = np.stack([corners[..., 0] * S, (1.0 - corners[..., 1]) * S], axis=-1).astype(np.float32)
    return dict(verts=np.asarray(v, np.float32).reshape(-1, 3), faces=np.asarray(f, np.int32).reshape(-1, 3), uv=uv, size=S, texture=texture)
