"""TSDF fusion on the device: from a set of posed depth maps back to a surface.

  TsdfVolume   a dense truncated-signed-distance volume and its weights, owned by the caller
  integrate    fuse depth maps [V, H, W] into a volume (ls2fm_tsdf_integrate, csrc/tsdf_fusion.hip): one launch, no host read
  extract      the mesh of the volume's zero level over the observed lattice points (ls2fm.mesh.marching_cubes)
  fuse_mesh    ls2fm.raster.rasterize -> integrate -> extract: the re-fusion step of the ScanNet protocol of the neural-surface
               papers (Manhattan-SDF, MonoSDF, NeuRIS).  The predicted mesh is rendered to depth at every test camera, the depth
               maps are fused and the re-fused mesh goes into ls2fm.metrics.evaluate_mesh: what no camera observes is removed,
               by the same rule on both sides.  ls2fm.raster.clean_mesh(visibility=True) is the DTU counterpart.
  fuse_field   the same from ls2fm.image.trace_image's depth of the SDF field, to set beside extract_mesh

The three producers of depth maps in the library -- raster.rasterize, image.trace_image and the sensor depth a ScanNet loader
reads -- share one convention: camera z, pixel for pixel (see raster.rasterize).  THE FUSION RULE is stated in include/ls2fm.h and
restated in numpy in tests/fusion_restate.py: a lattice point lands on the pixel on which the rasteriser would put a vertex there
(csrc/raster_project.h), takes that pixel's depth d, and with s = d - c_z >= -trunc extends its running average by
min(1, s / trunc) at the view's weight; every operation is one rounded fp32 operation, the views go in index order, one lane per
lattice point and no atomics.  So views split over several calls leave the bits of one call, and a rerun or a replay of a
captured graph repeats them.

Deviations from what fusion packages (Open3D, KinectFusion and their kin) do, on purpose: the distance is projective along camera
z, not along the ray; the depth is the nearest pixel's, not interpolated; the volume is dense (no hashing, no sparse bricks: 8
bytes per lattice point); and extract keeps the faces of a cell with an unobserved corner whose three vertices lie on observed
edges, where Open3D drops such cells whole.  Masks are the caller's business: one torch.where that writes +inf into the depth.
Colour is not part of the volume: ls2fm.mesh_colors.photo_colors colours any mesh from the photographs, the fused one included.

There is no CPU path: CPU tensors, a missing device or a missing library raise, as in ls2fm.raster.
"""
from __future__ import annotations

import ctypes
import functools
import math

import torch

from . import _lib, _posed, lattice, mesh, raster
from ._lib import check, ptr, stream_ptr

TRUNC_VOXELS = 3.0          # the default truncation distance, in voxels
_device = functools.partial(_lib.require_device_tensors, "ls2fm.fusion", phrase=": TSDF fusion runs on MI355X only")


class TsdfVolume:
    """A dense TSDF volume: tsdf and weight float32 [nx, ny, nz] on `device`, zero when fresh, on the lattice of ls2fm/lattice.py,
    so the extracted mesh is in the depth maps' world frame.  shape: three ints, each >= 2 for extract; origin: three floats;
    voxel and trunc positive and finite."""

    def __init__(self, shape, origin, voxel, trunc, device):
        shape = tuple(int(s) for s in shape)
        origin = tuple(float(v) for v in origin)
        voxel, trunc = float(voxel), float(trunc)
        if len(shape) != 3 or min(shape) < 0 or max(shape) > 2 ** 24:
            raise ValueError(f"ls2fm.fusion.TsdfVolume: shape {shape} must be three sides in [0, 2^24]")
        if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
            raise ValueError(f"ls2fm.fusion.TsdfVolume: origin {origin} must be three finite floats")
        if not (0.0 < voxel < math.inf and 0.0 < trunc < math.inf):
            raise ValueError(f"ls2fm.fusion.TsdfVolume: voxel {voxel} and trunc {trunc} must be positive and finite")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ls2fm.fusion: TSDF fusion runs on MI355X only (got a CPU device); there is no CPU fallback")
        self.shape, self.origin, self.voxel, self.trunc = shape, origin, voxel, trunc
        self.tsdf = torch.zeros(shape, dtype=torch.float32, device=device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=device)

    @property
    def device(self):
        return self.tsdf.device


def _depth_maps(depth, n, H, W):
    if depth.dim() == 3 and depth.shape[2] == 1 and H is not None and W is not None and depth.shape[1] == int(H) * int(W):
        depth = depth.reshape(depth.shape[0], int(H), int(W))               # [V, H W, 1], as ls2fm.image.trace_image returns it
    if depth.dim() == 2:
        depth = depth[None]
    if depth.dim() != 3 or depth.shape[0] != n or (H is not None and int(H) != depth.shape[1]) or (W is not None and int(W) != depth.shape[2]):
        raise ValueError(f"ls2fm.fusion.integrate: depth must be [{n}, H, W] (or [{n}, H W, 1] with H= and W=), got {tuple(depth.shape)}")
    return _lib.cf(depth.detach())


@torch.no_grad()
def integrate(volume: TsdfVolume, depth, pose, intr, near=1e-3, max_depth=math.inf, view_weight=None, max_weight=math.inf,
              H=None, W=None):
    """Fuse V depth maps into `volume` in place (THE FUSION RULE of include/ls2fm.h) -> volume.
      depth        float32 [V, H, W], camera z pixel for pixel; [V, H W, 1] as ls2fm.image.trace_image returns it is taken too,
                   with H= and W=.  A pixel that is not finite, not positive or above max_depth is not used: the rasteriser's
                   empty pixels (+inf), a tracer's misses, a sensor's zeros.  Masks: torch.where(mask, depth, inf) by the caller.
      pose, intr   [V, 3, 4] world-to-camera and [3, 3] or [V, 3, 3], as ls2fm.raster.rasterize
      view_weight  float [V] or None (every view weighs 1); a view whose weight is not > 0 is skipped
      max_weight   the weight saturates there: later views then move the average at 1 / max_weight at least
    One launch, no host read and no allocation beyond the argument conversions: the call can be captured.  The views of several
    calls, in order, leave the bits of one call over all of them."""
    depth, vw = torch.as_tensor(depth), None if view_weight is None else torch.as_tensor(view_weight)
    _device(depth, vw)
    poses, k4 = _posed.views(pose, intr, "ls2fm.fusion.integrate")
    n = int(poses.shape[0])
    d = _depth_maps(depth, n, H, W)
    if vw is not None:
        vw = _lib.cf(vw.detach().reshape(-1))
        if vw.shape[0] != n:
            raise ValueError(f"ls2fm.fusion.integrate: {vw.shape[0]} view weights for {n} views")
    return _integrate(volume, d, poses, k4, vw, near, max_depth, max_weight)


def _integrate(volume, d, poses, k4, vw, near, max_depth, max_weight):
    """integrate on converted arguments: d [n, H, W], poses [n, 3, 4], k4 [n, 4] and vw [n] or None, contiguous float32"""
    lib = _lib.load()
    n, dev = int(poses.shape[0]), volume.device
    for t in (poses, d, vw):
        if t is not None and t.device != dev:
            raise ValueError(f"ls2fm.fusion.integrate: the volume on {dev}, another argument on {t.device}")
    near = _posed.near_plane(near, "ls2fm.fusion.integrate")
    max_depth, max_weight = float(max_depth), float(max_weight)
    if not (max_depth > 0.0 and max_weight > 0.0):
        raise ValueError(f"ls2fm.fusion.integrate: max_depth {max_depth} and max_weight {max_weight} must be positive (inf is allowed)")
    if not (volume.tsdf.is_contiguous() and volume.weight.is_contiguous() and volume.tsdf.dtype == volume.weight.dtype == torch.float32
            and tuple(volume.tsdf.shape) == tuple(volume.weight.shape) == volume.shape):
        raise ValueError("ls2fm.fusion.integrate: the volume's tsdf and weight must be contiguous float32 of the volume's shape")
    origin = (ctypes.c_float * 3)(*volume.origin)
    with torch.cuda.device(dev):
        check(lib.ls2fm_tsdf_integrate(ptr(volume.tsdf), ptr(volume.weight), *volume.shape, origin, volume.voxel, volume.trunc, ptr(d),
                                       ptr(poses), ptr(k4), ptr(vw), n, int(d.shape[1]), int(d.shape[2]), near, max_depth, max_weight,
                                       stream_ptr()), "ls2fm_tsdf_integrate")
    return volume


@torch.no_grad()
def integrate_torch(volume: TsdfVolume, depth, pose, intr, near=1e-3, max_depth=math.inf, view_weight=None, max_weight=math.inf):
    """THE FUSION RULE as plain torch ops on the volume's device, vectorised over the lattice points, the views in a loop: the
    same operations in the same order, each a separate op, so each rounds once.  It reads and writes the whole volume once per
    view and per op.  The timing baseline (tools/time_fusion.py) and a check of the kernel; nothing in the library falls back
    to it.  view_weight: a sequence of floats or None.  -> volume"""
    dev = volume.device
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).float().to(dev)
    n = int(P.shape[0])
    K = torch.as_tensor(intr).detach().reshape(-1, 3, 3).float().to(dev).expand(n, 3, 3)
    depth = torch.as_tensor(depth).detach().float().to(dev)
    H, W = int(depth.shape[1]), int(depth.shape[2])
    x, y, z = lattice.points(volume.shape, volume.origin, volume.voxel, dev)
    T, Wt = volume.tsdf.view(-1), volume.weight.view(-1)
    # 0-dim device tensors: a division by a Python scalar would be a multiplication by its reciprocal
    scalar = lambda t: torch.tensor(float(t), dtype=torch.float32, device=dev)
    trunc, one, max_w = scalar(volume.trunc), scalar(1.0), scalar(max_weight)
    for i in range(n):
        w = 1.0 if view_weight is None else float(view_weight[i])
        if not w > 0.0:
            continue
        w = scalar(w)
        c, _, _, _, ok, px, py = _posed.project_torch(P[i], K[i], x, y, z, near, H, W)
        d = depth[i].reshape(-1)[py * W + px]
        ok = ok & torch.isfinite(d) & (d > 0) & (d <= max_depth)
        s = d - c[2]
        ok = ok & ~(s < -trunc)
        val = torch.fmin(one, s / trunc)
        Wn = Wt + w
        Tn = (Wt * T + w * val) / Wn
        T.copy_(torch.where(ok, Tn, T))
        Wt.copy_(torch.where(ok, torch.fmin(Wn, max_w), Wt))
    return volume


@torch.no_grad()
def extract(volume: TsdfVolume, min_weight=1.0) -> mesh.Mesh:
    """The mesh of the volume's zero level -> ls2fm.mesh.Mesh, in the depth maps' world frame, normals toward the cameras.
    A lattice point of weight < min_weight is unobserved and takes no part (lattice.zero_level): a cell with such a corner keeps the
    faces whose three vertices lie on observed edges (Open3D drops it whole).  Host reads: marching cubes' counts, the result's sizes."""
    return lattice.zero_level(volume.tsdf, volume.weight >= float(min_weight), volume.voxel, volume.origin)


def volume_for(bounds, voxel, trunc=None, device="cuda") -> TsdfVolume:
    """a fresh volume whose lattice covers bounds = ((x0, y0, z0), (x1, y1, z1)) as lattice.shape_for shapes it: origin at the low
    corner, per axis ceil((high - low) / voxel) + 1 points, at least 2.  trunc defaults to TRUNC_VOXELS = 3 voxels."""
    shape, origin = lattice.shape_for(bounds, voxel, "ls2fm.fusion: voxel {voxel} must be positive and finite, and the bounds {lo} .. {hi} finite")
    return TsdfVolume(shape, origin, voxel, TRUNC_VOXELS * float(voxel) if trunc is None else trunc, device)


@torch.no_grad()
def fuse_mesh(verts, faces, pose, intr, H, W, voxel, trunc=None, bounds=None, near=1e-3, max_depth=math.inf, min_weight=1.0,
              max_weight=math.inf, max_workspace_bytes=2 ** 28, return_volume=False):
    """Render a mesh to depth at every camera, fuse the depth maps and extract: ls2fm.raster.rasterize -> integrate -> extract.
    The re-fusion step of the ScanNet evaluation protocol; the result goes straight into ls2fm.metrics.evaluate_mesh.
      verts, faces, pose, intr, H, W, near   as ls2fm.raster.rasterize
      voxel        the lattice spacing;  trunc  the truncation distance, default 3 voxels (TRUNC_VOXELS)
      bounds       ((x0, y0, z0), (x1, y1, z1)) of the volume; default: the mesh's box grown by trunc, which costs one host
                   read (the box) -- give bounds to avoid it
    The views go in chunks whose z-buffer stays within max_workspace_bytes (at least one view per chunk), one rasterisation and
    one ls2fm_tsdf_integrate launch per chunk; the chunking does not show in the result.
    -> ls2fm.mesh.Mesh, with return_volume (Mesh, TsdfVolume)."""
    v, f = _posed.mesh_arrays(verts, faces, "ls2fm.fusion.fuse_mesh")
    poses, k4 = _posed.views(pose, intr, "ls2fm.fusion.fuse_mesh")
    H, W, voxel = int(H), int(W), float(voxel)
    trunc = TRUNC_VOXELS * voxel if trunc is None else float(trunc)
    if bounds is None:
        if not v.shape[0]:
            raise ValueError("ls2fm.fusion.fuse_mesh: an empty mesh has no box; give bounds")
        bounds = lattice.grown_box(v, trunc)
    volume = volume_for(bounds, voxel, trunc, v.device)
    for s, e in _posed.chunks(int(poses.shape[0]), 8, H, W, max_workspace_bytes):
        depth = raster.rasterize_prepared(v, f, poses[s:e], k4[s:e], H, W, near, max_workspace_bytes=max_workspace_bytes).depth
        _integrate(volume, depth, poses[s:e], k4[s:e], None, near, max_depth, max_weight)
    out = extract(volume, min_weight)
    return (out, volume) if return_volume else out


@torch.no_grad()
def fuse_field(sdf_field, pose, intr, H, W, voxel, bounds, trunc=None, near=1e-3, max_depth=math.inf, min_weight=1.0,
               max_weight=math.inf, max_workspace_bytes=2 ** 28, return_volume=False):
    """fuse_mesh's steps from the SDF field's own depth: ls2fm.image.trace_image -> integrate -> extract, a cross-check of the
    field against its depth maps to set beside extract_mesh.  A pixel whose ray did not `finish` (no surface found) is set to
    +inf and so not used.  pose [V, 3, 4], intr [3, 3] as trace_image takes them; bounds is required (a field has no box of its
    own here).  The views go in chunks whose traced maps (40 bytes per pixel) stay within max_workspace_bytes.
    -> ls2fm.mesh.Mesh, with return_volume (Mesh, TsdfVolume)."""
    from . import image
    poses = torch.as_tensor(pose).reshape(-1, 3, 4)
    _posed.device(poses)
    H, W = int(H), int(W)
    volume = volume_for(bounds, voxel, trunc, poses.device)
    for s, e in _posed.chunks(int(poses.shape[0]), 40, H, W, max_workspace_bytes):
        t = image.trace_image(sdf_field, poses[s:e], intr, H, W)
        depth = torch.where(t.finish, t.depth[..., 0], torch.full_like(t.depth[..., 0], math.inf)).view(e - s, H, W)
        integrate(volume, depth, poses[s:e], intr, near=near, max_depth=max_depth, max_weight=max_weight)
    out = extract(volume, min_weight)
    return (out, volume) if return_volume else out
