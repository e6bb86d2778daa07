"""A mesh rasteriser on the device: which faces of a mesh each camera sees, mesh depth maps, per-pixel face ids and barycentrics,
and the culling step that every published DTU Chamfer figure of an SDF method is taken after.

  rasterize    face_id / depth (/ barycentrics / per-face pixel counts) of a mesh in V views (ls2fm_rasterize, csrc/rasterize.hip)
  mask_votes   per vertex: in how many views it projects into the image, and in how many of those onto the mask
  clean_mesh   cull what projects outside the object masks, cull what no camera sees, keep the largest component

The rasterisation rule (include/ls2fm.h): fp32 camera points and projections of one rounding per operation, a snap to 8
sub-pixel bits, coverage in exact integers where exactly one of two faces takes a pixel centre on their shared edge, one fp64
depth expression per pixel, and the minimum of bits(depth) << 32 | face over the covering faces -- the nearest depth, among equal
depth bits the lowest face index.  The images are a pure function of the inputs: no visiting order, batching or path shows in
them, and tests/raster_restate.py holds them bit for bit.  A face with a vertex behind the near plane is not drawn in that view
(no clipping); back faces are drawn and occlude.  There is no CPU path: CPU tensors, a missing device or a missing library raise.

A caller chains  extract_mesh -> clean_mesh -> ls2fm.metrics.evaluate_mesh.
"""
from __future__ import annotations

import torch

from . import _lib, _posed
from ._lib import check, ptr, stream_ptr
from ._posed import device as _device, masks as _masks, mesh_arrays as _mesh, near_plane as _near, views as _views
from .options import Options


@torch.no_grad()
def rasterize(verts, faces, pose, intr, H, W, near=1e-3, bary=False, hits=False, max_workspace_bytes=2 ** 28):
    """Rasterise a mesh (verts float32 [n, 3], faces int32 [F, 3], on the device) into V views.  pose [3, 4] or [V, 3, 4]
    world-to-camera [R | t] as everywhere in ls2fm.image; intr [3, 3] or [V, 3, 3] (fx, fy, cx, cy are taken; skew is not
    modelled); pixel (px, py) has its centre at (px + 0.5, py + 0.5), as utils.camera.mesh_grid.
    -> Options(face_id int32 [V, H, W] (-1: empty), depth float32 [V, H, W] (+inf: empty), bary float32 [V, H, W, 3] or None
    (bary=True; perspective-correct weights of the face's three vertices, 0 where empty), face_hits int32 [F] or None (hits=True;
    the pixels each face won over all views)).  A face index outside [0, n) makes its face not drawn; it is no error.

    Depth convention: camera z, the third coordinate of R X + t.  utils.camera.camera_rays / get_center_and_ray form the ray of
    a pixel as the world direction of K^-1 [x, y, 1], un-normalised, so it has camera z = 1 whenever K's last row is [0, 0, 1]:
    the depth t of ls2fm.image.trace_image (point = centre + t ray) IS the camera z of the point it finds.  The two maps are
    directly comparable, pixel for pixel; neither is a Euclidean distance along the ray (that is t |ray|).

    The views are rasterised in chunks so that the 8-byte-per-pixel z-buffer stays within max_workspace_bytes (at least one view
    per chunk); views are independent, so the chunking does not show in the result.  Nothing is read back to the host, so a call
    can be captured into a graph."""
    v, f = _mesh(verts, faces, "ls2fm.raster.rasterize")
    poses, k4 = _views(pose, intr, "ls2fm.raster.rasterize")
    return rasterize_prepared(v, f, poses, k4, H, W, near, bary, hits, max_workspace_bytes)


@torch.no_grad()
def rasterize_prepared(v, f, poses, k4, H, W, near=1e-3, bary=False, hits=False, max_workspace_bytes=2 ** 28):
    """Internal to the package, not part of the API: rasterize on converted arguments (_posed.mesh_arrays, _posed.views or a
    chunk [s:e] of its pair), for the chunk loops of ls2fm.mesh_colors and ls2fm.fusion: the intrinsics are converted once."""
    lib = _lib.load()
    if poses.device != v.device or f.device != v.device:
        raise ValueError(f"ls2fm.raster.rasterize: verts on {v.device}, faces on {f.device}, poses on {poses.device}")
    H, W, near = int(H), int(W), _near(near, "ls2fm.raster.rasterize")
    if not (1 <= H <= 32768 and 1 <= W <= 32768):
        raise ValueError(f"ls2fm.raster.rasterize: image size {H} x {W} outside [1, 32768]")
    n, dev = int(poses.shape[0]), v.device
    n_f = int(f.shape[0])
    if n_f >= 1 << 31:
        raise ValueError(f"ls2fm.raster.rasterize: {n_f} faces, 2^31 or more")
    ranges = _posed.chunks(n, 8, H, W, max_workspace_bytes)
    with torch.cuda.device(dev):
        face_id = torch.empty(n, H, W, dtype=torch.int32, device=dev)
        depth = torch.empty(n, H, W, dtype=torch.float32, device=dev)
        bc = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev) if bary else None
        face_hits = torch.zeros(n_f, dtype=torch.int32, device=dev) if hits else None
        if n:
            ws = _lib.workspace(lib.ls2fm_rasterize_workspace_bytes(ranges[0][1], H, W), "ls2fm_rasterize_workspace_bytes", dev)
        for s, e in ranges:
            check(lib.ls2fm_rasterize(ptr(v), int(v.shape[0]), ptr(f), n_f, ptr(poses[s:e]), ptr(k4[s:e]), e - s, H, W, near,
                                      ptr(face_id[s:e]), ptr(depth[s:e]), ptr(bc[s:e]) if bary else ptr(None), ptr(face_hits),
                                      ptr(ws), stream_ptr()), "ls2fm_rasterize")
    return Options(face_id=face_id, depth=depth, bary=bc, face_hits=face_hits)


@torch.no_grad()
def mask_votes(verts, pose, intr, masks, near=1e-3):
    """(seen, inside) int32 [n] of the vertices verts float32 [n, 3]: seen counts the views where the vertex is usable (camera z
    finite and >= near, |u| and |v| <= 65536) and in the image (0 <= u < W and 0 <= v < H), inside those of them whose mask
    pixel (floor(u), floor(v)) is non-zero.  masks bool or uint8 [V, H, W]; pose and intr as rasterize.  One launch, no atomics."""
    lib = _lib.load()
    verts = torch.as_tensor(verts)
    _device(verts)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"ls2fm.raster.mask_votes: verts must be [n, 3], got shape {tuple(verts.shape)}")
    v = _lib.cf(verts.detach())
    poses, k4 = _views(pose, intr, "ls2fm.raster.mask_votes")
    n = int(poses.shape[0])
    m = _masks(masks, n, "ls2fm.raster.mask_votes")
    if poses.device != v.device or m.device != v.device:
        raise ValueError(f"ls2fm.raster.mask_votes: verts on {v.device}, poses on {poses.device}, masks on {m.device}")
    H, W, near = int(m.shape[1]), int(m.shape[2]), _near(near, "ls2fm.raster.mask_votes")
    with torch.cuda.device(v.device):
        seen = torch.empty(v.shape[0], dtype=torch.int32, device=v.device)
        inside = torch.empty(v.shape[0], dtype=torch.int32, device=v.device)
        check(lib.ls2fm_mesh_mask_votes(ptr(v), int(v.shape[0]), ptr(poses), ptr(k4), n, H, W, near, ptr(m), ptr(seen), ptr(inside),
                                        stream_ptr()), "ls2fm_mesh_mask_votes")
    return seen, inside


def mask_votes_torch(verts, pose, intr, masks, near=1e-3):
    """mask_votes as plain torch ops on whatever device the tensors are on: the same operations in the same order, each a
    separate op, so each rounds once.  The timing baseline and a check; nothing in the library falls back to it."""
    v = torch.as_tensor(verts).float()
    pose, intr, masks = torch.as_tensor(pose), torch.as_tensor(intr), torch.as_tensor(masks)
    P = pose.reshape(-1, 3, 4).float()
    K = intr.reshape(-1, 3, 3).float().expand(P.shape[0], 3, 3)
    masks = masks[None] if masks.dim() == 2 else masks
    H, W = int(masks.shape[1]), int(masks.shape[2])
    seen = torch.zeros(v.shape[0], dtype=torch.int32, device=v.device)
    inside = torch.zeros_like(seen)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    for i in range(P.shape[0]):
        _, _, _, _, ok, px, py = _posed.project_torch(P[i], K[i], x, y, z, near, H, W)
        seen += ok.to(torch.int32)
        inside += (ok & (masks[i].view(-1)[py * W + px] != 0)).to(torch.int32)
    return seen, inside


@torch.no_grad()
def clean_mesh(verts, faces, pose, intr, masks=None, H=None, W=None, dilate=0, max_outside=0, min_seen=1, visibility=True,
               min_pixels=1, keep_largest=False, near=1e-3):
    """The culling step in front of a DTU-style Chamfer evaluation -> (ls2fm.mesh.Mesh, kept_faces bool [F]).
      masks       bool or uint8 [V, H, W] object masks (None: no mask culling), first dilated by `dilate` pixels (a max_pool2d of
                  side 2 dilate + 1).  A vertex survives when seen >= min_seen and seen - inside <= max_outside (mask_votes): it is
                  in at least min_seen images and off the mask in at most max_outside of them.
      visibility  a face must also have won at least min_pixels pixels over all views in a rasterisation of the WHOLE mesh at
                  H x W (default: the masks' size): culled geometry still occludes, as in the usual scripts.  False: no
                  rasterisation runs.
    A face survives when its three vertices do (and it is visible).  Vertices no surviving face uses are dropped and the faces
    re-indexed, both in their order, with torch ops.  kept_faces is this selection; keep_largest then hands the result to
    ls2fm.mesh.largest_component.  Face indices are checked (one host read), the sizes of the result are another."""
    from . import mesh
    v, f = _mesh(verts, faces, "ls2fm.raster.clean_mesh")
    mesh._faces_i32(f, int(v.shape[0]), "ls2fm.raster.clean_mesh")
    dev = v.device
    with torch.cuda.device(dev):
        keep_v = torch.ones(v.shape[0], dtype=torch.bool, device=dev)
        if masks is not None:
            poses, _ = _views(pose, intr, "ls2fm.raster.clean_mesh")
            m = _masks(masks, int(poses.shape[0]), "ls2fm.raster.clean_mesh")
            if int(dilate) > 0:
                d = int(dilate)
                m = torch.nn.functional.max_pool2d(m[:, None].float(), kernel_size=2 * d + 1, stride=1, padding=d)[:, 0].to(torch.uint8)
            H = int(m.shape[1]) if H is None else int(H)
            W = int(m.shape[2]) if W is None else int(W)
            seen, inside = mask_votes(v, pose, intr, m, near=near)
            keep_v = (seen >= int(min_seen)) & (seen - inside <= int(max_outside))
        idx = f.long()
        keep_f = keep_v[idx].all(dim=1) if f.shape[0] else torch.zeros(0, dtype=torch.bool, device=dev)
        if visibility:
            if H is None or W is None:
                raise ValueError("ls2fm.raster.clean_mesh: visibility needs the image size (H, W) when no masks give it")
            keep_f = keep_f & (rasterize(v, f, pose, intr, H, W, near=near, hits=True).face_hits >= int(min_pixels))
        out = mesh.select_faces(v, f, keep_f)
        if keep_largest:
            out = mesh.largest_component(out.vertices, out.faces)
    return out, keep_f
