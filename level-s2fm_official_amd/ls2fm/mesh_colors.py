"""Vertex colours for extracted meshes, from the two colour sources that sit on the device next to the mesh.

  field_colors   the trained radiance field at the vertices (ls2fm_radiance_points, csrc/radiance_points.hip): per point what
                 Renderer.forward_composed forms per sample, seen along given directions or head-on (v = -normalize(g))
  photo_colors   the photographs: per vertex a weighted blend of the views that see it, visibility decided against the
                 rasteriser's depth maps of the same mesh (ls2fm_mesh_vertex_colors, csrc/mesh_colors.hip)
  color_mesh     photographs where some view sees the vertex, the field elsewhere; the field's normals weight the views

THE VERTEX COLOUR RULE is stated in include/ls2fm.h and restated in numpy in tests/mesh_colors_restate.py: the rasteriser's
camera point, projection and pixel; a mask byte; c_z <= d + depth_tol d against the mesh's own depth at that pixel; the weight
cos^power of the angle between the vertex normal and the direction to the camera; a bilinear sample; fp64 sums over the views in
index order, one lane per vertex and no atomics, so the colours are a pure function of the inputs.  Deviations from what texturing
packages do, on purpose: vertex colours only (no texture atlas), no seam levelling or exposure compensation between views, and
the z-test reads the vertex's own pixel only (no neighbourhood, no per-view depth bias beyond depth_tol).

CPU tensors take the same rules as torch ops (photo_colors_torch in fp64, the composed field evaluation); the rasteriser has
no CPU form, so a CPU call of photo_colors is handed the depth maps.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib, _posed, fused, raster
from ._lib import check, ptr, stream_ptr


class VertexColors(NamedTuple):
    """colors float32 [V, C]; weight float64 [V], the sum of the contributing views' weights; count int32 [V], their number"""
    colors: torch.Tensor
    weight: torch.Tensor
    count: torch.Tensor


# ------------------------------------------------------------------------------------------------ the field
def field_colors_composed(opt, sdf_field, rad_field, points, view_dirs=None, return_normals=False):
    """field_colors as the torch composition of Renderer.forward_composed's per-sample lines (models/Renderer.py:105-117), on
    whatever device the points are on: every configuration, CPU tensors included"""
    pts = torch.as_tensor(points).detach().float()
    with torch.no_grad():
        _, feats = sdf_field.infer_sdf(pts, mode="ret_all")
        g = sdf_field.gradient(pts.clone()).detach()
        v = -torch.nn.functional.normalize(g, dim=-1) if view_dirs is None else torch.as_tensor(view_dirs).detach().float().expand_as(pts)
        view = rad_field.infer_embed_v(ray_utils=v)
        geo = feats[..., 1:]
        if opt.Ablate_config.dual_field == True:  # noqa: E712
            geo = torch.cat([geo, rad_field.Geometry_feat(pts)[..., 1:]], dim=-1)
        rgb = rad_field.infer_app(torch.cat([pts, g, view, geo], dim=-1)).detach()
    return (rgb, g) if return_normals else rgb


def can_eval_field(opt, sdf_field, rad_field, points) -> bool:
    """True when ls2fm_radiance_points serves this call: device points and the configurations of the fused render"""
    return bool(points.is_cuda and fused.supported(opt, sdf_field, rad_field))


def field_points(opt, sdf_field, rad_field, points, view_dirs=None):
    """ls2fm_radiance_points on points float32 [n, 3] (, view_dirs [n, 3]) -> (rgb [n, 3], g [n, 3], sdf [n]).  Raises where
    can_eval_field is False.  Two launches, nothing read back: the call can be captured."""
    lib = _lib.load()
    if not can_eval_field(opt, sdf_field, rad_field, points):
        raise RuntimeError("ls2fm.mesh_colors.field_points: ls2fm_radiance_points does not serve this configuration "
                           "(CPU points, data.bg_sdf or layer sizes outside the fused ones); field_colors takes the composed form")
    p = _lib.cf(points.detach().reshape(-1, 3))
    n, dev = int(p.shape[0]), p.device
    d = None
    if view_dirs is not None:
        d = torch.as_tensor(view_dirs).detach()
        d = _lib.cf(d.to(dev).expand(n, 3) if d.dim() == 1 else d.reshape(-1, 3))
        if d.device != dev or d.shape[0] != n:
            raise ValueError(f"ls2fm.mesh_colors.field_points: {tuple(d.shape)} view_dirs on {d.device} for {n} points on {dev}")
    ts, dual = fused.param_tensors(sdf_field, rad_field)
    ts = [t.detach().contiguous() for t in ts]
    pstruct = fused._params_struct(ts, dual, float(sdf_field.beta_speed))
    fdesc = fused.field_desc(opt)
    g1 = sdf_field.embed_fn.embedder_obj.desc
    g2 = rad_field.embed_fn.embedder_obj.desc if dual else g1
    with torch.cuda.device(dev):
        rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
        g = torch.empty(n, 3, dtype=torch.float32, device=dev)
        sdf = torch.empty(n, dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.ls2fm_radiance_points_workspace_bytes(), "ls2fm_radiance_points_workspace_bytes", dev)
        check(lib.ls2fm_radiance_points(ctypes.byref(fdesc), ctypes.byref(g1), ctypes.byref(g2), ctypes.byref(pstruct), ptr(p), ptr(d), n,
                                        ptr(rgb), ptr(g), ptr(sdf), ptr(ws), stream_ptr()), "ls2fm_radiance_points")
    return rgb, g, sdf


def field_colors(opt, sdf_field, rad_field, points, view_dirs=None, return_normals=False):
    """The radiance field's colour at points [..., 3]: rgb float32 [..., 3] in [0, 1] (with return_normals also g [..., 3], the
    SDF's analytic gradient there, not normalised).  view_dirs [..., 3] (or one direction [3]) are the directions the points
    are seen along, as a camera ray's; None: v = -normalize(g), the surface seen head-on.
    Device points with the fused render's configuration run ls2fm_radiance_points; data.bg_sdf, other layer sizes and CPU
    tensors take field_colors_composed -- the same values to the parity of the fused render with the composed one."""
    points = torch.as_tensor(points)
    if not can_eval_field(opt, sdf_field, rad_field, points):
        return field_colors_composed(opt, sdf_field, rad_field, points, view_dirs, return_normals)
    shape = tuple(points.shape[:-1])
    rgb, g, _ = field_points(opt, sdf_field, rad_field, points, view_dirs)
    rgb, g = rgb.view(*shape, 3), g.view(*shape, 3)
    return (rgb, g) if return_normals else rgb


# ------------------------------------------------------------------------------------------------ the photographs
def _fill(fill, channels):
    """`channels` floats of a scalar or a sequence; a sequence that is shorter is extended with 1 (an opaque alpha)"""
    vals = [float(fill)] * channels if isinstance(fill, (int, float)) else [float(v) for v in fill]
    return (vals + [1.0] * channels)[:channels]


def _check_photo_args(depth_tol, power):
    depth_tol, power = float(depth_tol), int(power)
    if not (0.0 <= depth_tol < float("inf")):
        raise ValueError(f"ls2fm.mesh_colors.photo_colors: depth_tol {depth_tol} must be finite and not negative")
    if not 0 <= power <= 8:
        raise ValueError(f"ls2fm.mesh_colors.photo_colors: power {power} outside 0 .. 8")
    return depth_tol, power


def _images(images, n, name):
    images = torch.as_tensor(images)
    if images.dim() == 3:
        images = images[None]
    if images.dim() != 4 or images.shape[0] != n or not 1 <= images.shape[3] <= 4:
        raise ValueError(f"ls2fm.mesh_colors.{name}: images must be [{n}, H, W, C] with C from 1 to 4, got {tuple(images.shape)}")
    return _lib.cf(images.detach())


def accumulate_views(state, verts, pose4, images, depth, masks=None, normals=None, near=1e-3, depth_tol=1e-2, power=1):
    """ls2fm_mesh_vertex_colors over the views given: state = (sums float64 [V, C + 1], count int32 [V]) is extended in place.
    verts [V, 3], pose4 = (poses [N, 3, 4], intr [N, 4]), images [N, H, W, C], depth [N, H, W] float32 and masks uint8
    [N, H, W] or None, normals [V, 3] or None: contiguous on one device.  One launch, nothing read back."""
    lib = _lib.load()
    sums, count = state
    poses, k4 = pose4
    n, H, W, C = (int(s) for s in images.shape)
    check(lib.ls2fm_mesh_vertex_colors(ptr(verts), ptr(normals), int(verts.shape[0]), ptr(poses), ptr(k4), n, H, W, C, ptr(images),
                                       ptr(depth), ptr(masks), float(near), float(depth_tol), int(power), ptr(sums), ptr(count),
                                       stream_ptr()), "ls2fm_mesh_vertex_colors")


def finish_colors(state, channels, fill=(0.5, 0.5, 0.5), fallback=None):
    """ls2fm_mesh_vertex_colors_finish -> colors float32 [V, C]: sums / weight where count > 0, elsewhere fallback [V, C] or fill"""
    lib = _lib.load()
    sums, count = state
    n_v, dev = int(count.shape[0]), count.device
    fb = None
    if fallback is not None:
        fb = _lib.cf(torch.as_tensor(fallback).detach())
        if tuple(fb.shape) != (n_v, channels) or fb.device != dev:
            raise ValueError(f"ls2fm.mesh_colors: fallback must be [{n_v}, {channels}] on {dev}, got {tuple(fb.shape)} on {fb.device}")
    host_fill = (ctypes.c_float * channels)(*_fill(fill, channels))
    with torch.cuda.device(dev):
        colors = torch.empty(n_v, channels, dtype=torch.float32, device=dev)
        check(lib.ls2fm_mesh_vertex_colors_finish(ptr(sums), ptr(count), n_v, channels, ptr(fb), host_fill, ptr(colors), stream_ptr()),
              "ls2fm_mesh_vertex_colors_finish")
    return colors


def photo_colors_torch(verts, pose, intr, images, depth, masks=None, normals=None, near=1e-3, depth_tol=1e-2, power=1,
                       fill=(0.5, 0.5, 0.5), fallback=None, state=None):
    """THE VERTEX COLOUR RULE as plain torch ops on whatever device the tensors are on, vectorised over the vertices, the views
    in a loop: the fp32 steps as separate fp32 ops, the weights, samples and sums in fp64.  The form CPU tensors take, the
    timing baseline and a check of the kernel.  depth [N, H, W]: the rasteriser's depth of the same mesh and views.
    -> VertexColors; with state=(sums, count) those are extended and returned through it."""
    depth_tol, power = _check_photo_args(depth_tol, power)
    v = torch.as_tensor(verts).detach().float()
    dev = v.device
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).float()
    n = int(P.shape[0])
    K = torch.as_tensor(intr).detach().reshape(-1, 3, 3).float().expand(n, 3, 3)
    img = _images(images, n, "photo_colors_torch")
    H, W, C = int(img.shape[1]), int(img.shape[2]), int(img.shape[3])
    depth = torch.as_tensor(depth).detach().float().reshape(n, H, W)
    if masks is not None:
        masks = torch.as_tensor(masks)
        masks = (masks[None] if masks.dim() == 2 else masks).reshape(n, H, W)
    nrm = None if normals is None else torch.as_tensor(normals).detach().float().to(torch.float64)
    n_v = int(v.shape[0])
    sums, count = state if state is not None else (torch.zeros(n_v, C + 1, dtype=torch.float64, device=dev),
                                                   torch.zeros(n_v, dtype=torch.int32, device=dev))
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    tol = torch.tensor(depth_tol, dtype=torch.float32, device=dev)
    for i in range(n):
        c, u, w, _, ok, px, py = _posed.project_torch(P[i], K[i], x, y, z, near, H, W)
        at = py * W + px
        if masks is not None:
            ok = ok & (masks[i].reshape(-1)[at] != 0)
        d = depth[i].reshape(-1)[at]
        ok = ok & torch.isfinite(d) & (c[2] <= d + tol * d)
        wt = torch.ones(n_v, dtype=torch.float64, device=dev)
        if nrm is not None:
            R = P[i, :, :3].to(torch.float64)
            m = [(R[r, 0] * nrm[:, 0] + R[r, 1] * nrm[:, 1]) + R[r, 2] * nrm[:, 2] for r in range(3)]
            cd = [t.to(torch.float64) for t in c]
            dot = (m[0] * cd[0] + m[1] * cd[1]) + m[2] * cd[2]
            mm = ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]).sqrt()
            cc = ((cd[0] * cd[0] + cd[1] * cd[1]) + cd[2] * cd[2]).sqrt()
            cos = (-dot) / (mm * cc)
            ok = ok & (cos > 0) & torch.isfinite(cos)
            for _ in range(power):
                wt = wt * cos
        sx, sy = u.to(torch.float64) - 0.5, w.to(torch.float64) - 0.5
        sx = torch.where(ok, sx, torch.zeros_like(sx))
        sy = torch.where(ok, sy, torch.zeros_like(sy))
        fx0, fy0 = sx.floor(), sy.floor()
        tx, ty = sx - fx0, sy - fy0
        x0, x1 = fx0.long().clamp(0, W - 1), (fx0.long() + 1).clamp(0, W - 1)
        y0, y1 = fy0.long().clamp(0, H - 1), (fy0.long() + 1).clamp(0, H - 1)
        flat = img[i].reshape(H * W, C).to(torch.float64)
        a00, a10, a01, a11 = flat[y0 * W + x0], flat[y0 * W + x1], flat[y1 * W + x0], flat[y1 * W + x1]
        r0 = a00 + tx[:, None] * (a10 - a00)
        r1 = a01 + tx[:, None] * (a11 - a01)
        s = r0 + ty[:, None] * (r1 - r0)
        sums[:, :C] = torch.where(ok[:, None], sums[:, :C] + wt[:, None] * s, sums[:, :C])
        sums[:, C] = torch.where(ok, sums[:, C] + wt, sums[:, C])
        count += ok.to(torch.int32)
    seen = count > 0
    colors = (sums[:, :C] / sums[:, C:]).to(torch.float32)
    other = torch.tensor(_fill(fill, C), dtype=torch.float32, device=dev).expand(n_v, C) if fallback is None \
        else torch.as_tensor(fallback).detach().float().to(dev).reshape(n_v, C)
    return VertexColors(torch.where(seen[:, None], colors, other), sums[:, C].clone(), count)


@torch.no_grad()
def photo_colors(verts, faces, pose, intr, images, masks=None, normals=None, near=1e-3, depth_tol=1e-2, power=1,
                 fill=(0.5, 0.5, 0.5), fallback=None, view_chunk=None, depth=None):
    """Vertex colours of a mesh (verts float32 [V, 3], faces int32 [F, 3]) from photographs -> VertexColors(colors float32
    [V, C], weight float64 [V], count int32 [V]).
      pose, intr  [N, 3, 4] world-to-camera and [3, 3] or [N, 3, 3], as ls2fm.raster.rasterize
      images      float [N, H, W, C], C from 1 to 4, channel last (the layout of ls2fm.image.render_image's rgb)
      masks       bool or uint8 [N, H, W] or None: a view is not used for a vertex that lands on a zero byte
      normals     [V, 3] or None.  Given, a view weighs cos^power of the angle between the normal and the direction from the
                  vertex to the camera, and does not count where that cosine is <= 0.  None: every view weighs 1.
      depth_tol   the view counts where c_z <= d (1 + depth_tol), d the mesh's own rasterised depth at the vertex's pixel.
                  The relative depth change across one pixel on a surface inclined by theta to the image plane is about
                  tan(theta) / f_px, so 1e-2 at f_px ~ 1000 admits inclinations up to ~84 degrees: DESIGN 3.19.
      fill, fallback  the colour of a vertex no view counts for: fallback [V, C], else fill (a sequence shorter than C is
                  extended with 1)
      view_chunk  views rasterised per chunk (None: what keeps a chunk's depth and face maps within 256 MiB); the state is
                  carried across the chunks, so the chunking does not show in the result
      depth       [N, H, W]: the rasteriser's depth maps, if the caller holds them already; required for CPU tensors
    Device tensors: one ls2fm.raster.rasterize and one ls2fm_mesh_vertex_colors launch per chunk, then the finish launch; no
    host read.  CPU tensors: photo_colors_torch."""
    depth_tol, power = _check_photo_args(depth_tol, power)
    verts = torch.as_tensor(verts)
    if not verts.is_cuda:
        if depth is None:
            raise RuntimeError("ls2fm.mesh_colors.photo_colors: CPU tensors need the depth maps (depth=...): the rasteriser runs "
                               "on MI355X only")
        return photo_colors_torch(verts, pose, intr, images, depth, masks, normals, near, depth_tol, power, fill, fallback)
    v, f = _posed.mesh_arrays(verts, faces, "ls2fm.mesh_colors.photo_colors")
    poses, k4 = _posed.views(pose, intr, "ls2fm.mesh_colors.photo_colors")
    n, dev = int(poses.shape[0]), v.device
    img = _images(images, n, "photo_colors")
    H, W, C = int(img.shape[1]), int(img.shape[2]), int(img.shape[3])
    m = None if masks is None else _posed.masks(masks, n, "ls2fm.mesh_colors.photo_colors")
    if m is not None and tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"ls2fm.mesh_colors.photo_colors: masks of {tuple(m.shape[1:])} for images of {(H, W)}")
    near = _posed.near_plane(near, "ls2fm.mesh_colors.photo_colors")
    nrm = None
    if normals is not None:
        nrm = _lib.cf(torch.as_tensor(normals).detach())
        if tuple(nrm.shape) != tuple(v.shape):
            raise ValueError(f"ls2fm.mesh_colors.photo_colors: normals {tuple(nrm.shape)} for verts {tuple(v.shape)}")
    if depth is not None:
        depth = _lib.cf(torch.as_tensor(depth).detach())
        if tuple(depth.shape) != (n, H, W):
            raise ValueError(f"ls2fm.mesh_colors.photo_colors: depth must be [{n}, {H}, {W}], got {tuple(depth.shape)}")
    for t in (poses, img, m, nrm, depth):
        if t is not None and t.device != dev:
            raise ValueError(f"ls2fm.mesh_colors.photo_colors: verts on {dev}, another argument on {t.device}")
    with torch.cuda.device(dev):
        state = (torch.zeros(v.shape[0], C + 1, dtype=torch.float64, device=dev), torch.zeros(v.shape[0], dtype=torch.int32, device=dev))
        for s, e in _posed.chunks(n, 8, H, W, 2 ** 28, view_chunk):
            d = depth[s:e] if depth is not None else raster.rasterize_prepared(v, f, poses[s:e], k4[s:e], H, W, near).depth
            accumulate_views(state, v, (poses[s:e], k4[s:e]), img[s:e], d, None if m is None else m[s:e], nrm, near, depth_tol, power)
        colors = finish_colors(state, C, fill, fallback)
    return VertexColors(colors, state[0][:, C].clone(), state[1])


# ------------------------------------------------------------------------------------------------ both
def color_mesh(opt, sdf_field, rad_field, verts, faces, pose, intr, images, masks=None, near=1e-3, depth_tol=1e-2, power=1,
               view_chunk=None, depth=None):
    """Photographs where some view sees the vertex, the radiance field elsewhere -> VertexColors (colors [V, 3]).  The weights'
    normals are the field's analytic gradient g at the vertices (it points into free space, toward the cameras), so both come
    from one ls2fm_radiance_points call; count == 0 marks the vertices that carry the field's colour."""
    verts = torch.as_tensor(verts)
    rgb, g = field_colors(opt, sdf_field, rad_field, verts, return_normals=True)
    return photo_colors(verts, faces, pose, intr, images, masks=masks, normals=g, near=near, depth_tol=depth_tol, power=power,
                        fallback=rgb, view_chunk=view_chunk, depth=depth)


def resolve_colors(colors, verts, faces, sdf_field, rad_field, what):
    """the `colors` argument of extract_mesh / get_surface_high_res_mesh -> a colour array [V, 3 | 4] or None.  "field": the
    radiance field at the vertices (needs rad_field); a callable: colors(verts, faces)."""
    if colors is None:
        return None
    if callable(colors):
        return colors(verts, faces)
    if colors == "field":
        if rad_field is None or not isinstance(sdf_field, torch.nn.Module):
            raise ValueError(f"{what}(colors='field') needs the SDF field and rad_field=<the radiance field>")
        return field_colors(sdf_field.opt, sdf_field, rad_field, verts)
    raise ValueError(f"{what}: colors must be None, 'field' or a callable (verts, faces) -> colours, got {colors!r}")
