"""Meshing an oriented point cloud on the device: from a scan, a filtered MVS cloud or the mapper's points to a surface.

  ImplicitVolume        a dense lattice of signed distances to the cloud's local planes and of their weights (TsdfVolume's layout)
  implicit_from_cloud   the volume of a cloud with normals (ls2fm_cloud_implicit, csrc/cloud_implicit.hip): one launch
  extract               the mesh of the volume's zero level over the defined lattice points (ls2fm.mesh.marching_cubes)
  mesh_from_cloud       estimate_normals (when the cloud brings none) -> implicit_from_cloud -> extract; the result goes into
                        metrics.evaluate_mesh, raster.clean_mesh, mesh_colors.photo_colors and simplify.simplify as it stands
  cloud.depths_to_cloud gives the route its input from depth maps: mvs.filter_depths -> depths_to_cloud ->
                        cloud.statistical_outliers -> mesh_from_cloud is the classical dense route without a volume of depth maps

THE IMPLICIT RULE is stated in include/ls2fm.h and restated in numpy in tests/cloud_mesh_restate.py: a lattice point takes its k
nearest cloud points within the radius (the K-NEIGHBOUR RULE), weighs each by (1 - d2 / radius^2)^3 and averages the signed
distances to their tangent planes, in fp64 in list order.  The value is a pure function of the cloud, the normals, the lattice, k,
the radius and min_neighbors: no grid, brick, batch or rerun shows in it.  _implicit_torch is the same rule as plain torch ops on
whatever device the tensors are on: the timing baseline, and the route CPU tensors take.  A device tensor never takes it: a
missing library raises.

Deviations from what surface-reconstruction packages do, on purpose: a local moving-least-squares surface, not Poisson's global
solve -- holes stay holes and nothing is extrapolated beyond the radius; k <= 32, so where more than 32 points lie in the support
ball the list truncates and the value steps slightly; the lattice is dense (8 bytes per lattice point); structures thinner than
two voxels merge or vanish; no colour in the volume (mesh_colors.photo_colors colours the mesh); no gradients.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib, cloud, lattice, mesh
from ._lib import check, ptr, stream_ptr
from .point_grid import PointGrid, knn_k, points3, squared_cutoff

RADIUS_VOXELS = 3.0         # the default support radius, in voxels
# the launch plans of ls2fm_cloud_implicit_plan (include/ls2fm.h: LS2FM_CLOUD_IMPLICIT_BRICK0_* / _BRICK1_*) and the default one
BRICKS = ((2, 2, 64), (8, 8, 4))
DEFAULT_PLAN = dict(brick=1, empty_test=True)


class ImplicitVolume:
    """value and support float32 [nx, ny, nz] of THE IMPLICIT RULE on one device, on the lattice of ls2fm/lattice.py (TsdfVolume's
    layout), so the extracted mesh is in the cloud's frame.  value is NaN where the rule defines none; support is the sum of the
    weights (0 without a neighbour).  radius is the support radius the volume was made with."""

    def __init__(self, value, support, origin, voxel, radius):
        self.value, self.support = value, support
        self.shape = tuple(int(s) for s in value.shape)
        self.origin, self.voxel, self.radius = tuple(float(v) for v in origin), float(voxel), float(radius)

    @property
    def device(self):
        return self.value.device


def _lattice(bounds, voxel):
    shape, origin = lattice.shape_for(bounds, voxel, "ls2fm.cloud_mesh: the bounds {lo} .. {hi} must be two finite corners")
    if max(shape) > 2 ** 24 or math.prod(shape) >= 2 ** 31:
        raise ValueError(f"ls2fm.cloud_mesh: a lattice of {shape} points, a side above 2^24 or 2^31 points or more")
    return shape, origin


def _options(voxel, radius, k, min_neighbors):
    voxel = float(voxel)
    if not 0.0 < voxel < math.inf:
        raise ValueError(f"ls2fm.cloud_mesh: voxel {voxel} must be positive and finite")
    radius = RADIUS_VOXELS * voxel if radius is None else float(radius)
    max_d2 = squared_cutoff(radius)
    if not 0.0 < float(max_d2) < math.inf:
        raise ValueError(f"ls2fm.cloud_mesh: radius {radius} must have a positive finite fp32 square (the weight needs it)")
    k = knn_k(k)
    if isinstance(min_neighbors, bool) or int(min_neighbors) != min_neighbors or int(min_neighbors) < 1:
        raise ValueError(f"ls2fm.cloud_mesh: min_neighbors {min_neighbors} must be an integer >= 1")
    return voxel, radius, max_d2, k, int(min_neighbors)


@torch.no_grad()
def _implicit_torch(points, normals, shape, origin, voxel, radius, k=16, min_neighbors=3, grid=None, chunk=1 << 18):
    """THE IMPLICIT RULE as plain torch ops on the points' device -> (value, support) float32 [nx, ny, nz].  The lattice points go
    in chunks through PointGrid.knn (device tensors; `grid` is reused) or cloud._knn_torch (CPU tensors); the two sums are then
    accumulated over the list's columns in a Python loop, so that each add rounds once, both starting from their first term."""
    points, normals = points3(points, "points").float(), points3(normals, "normals").float()
    voxel, radius, max_d2, k, min_neighbors = _options(voxel, radius, k, min_neighbors)
    dev = points.device
    n_points = int(points.shape[0])
    total = math.prod(shape)
    value = torch.full((total,), math.nan, dtype=torch.float32, device=dev)
    support = torch.zeros(total, dtype=torch.float32, device=dev)
    if n_points == 0 or total == 0:
        return value.view(shape), support.view(shape)
    X = torch.stack(lattice.points(shape, origin, voxel, dev), dim=1)
    p64, n64 = points.to(torch.float64), normals.to(torch.float64)
    lim = torch.tensor(float(max_d2), dtype=torch.float64, device=dev)      # a tensor: a Python scalar would divide by its reciprocal
    if points.is_cuda and grid is None:
        grid = PointGrid(points)
    for s in range(0, total, chunk):
        q = X[s:s + chunk].contiguous()
        idx, d2, _ = grid.knn(q, k, radius) if points.is_cuda else cloud._knn_torch(q, points, k, radius)
        q64 = q.to(torch.float64)
        m = int(q.shape[0])
        den = torch.zeros(m, dtype=torch.float64, device=dev)
        num = torch.zeros(m, dtype=torch.float64, device=dev)
        n = torch.zeros(m, dtype=torch.int64, device=dev)
        for j in range(k):
            has = idx[:, j] >= 0
            i = torch.where(has, idx[:, j], torch.zeros_like(idx[:, j])).long()
            t = 1.0 - d2[:, j].to(torch.float64) / lim
            w = (t * t) * t
            P, N = p64[i], n64[i]
            sd = (N[:, 0] * (q64[:, 0] - P[:, 0]) + N[:, 1] * (q64[:, 1] - P[:, 1])) + N[:, 2] * (q64[:, 2] - P[:, 2])
            ws = w * sd
            first = n == 0
            den = torch.where(has, torch.where(first, w, den + w), den)
            num = torch.where(has, torch.where(first, ws, num + ws), num)
            n = n + has
        ok = (n >= min_neighbors) & (den > 0.0)
        value[s:s + chunk] = torch.where(ok, (num / den).float(), torch.full_like(den, math.nan, dtype=torch.float32))
        support[s:s + chunk] = den.float()
    return value.view(shape), support.view(shape)


def _implicit_device(points, normals, grid, shape, origin, voxel, k, max_d2, min_neighbors, plan=None):
    """one ls2fm_cloud_implicit launch on converted arguments -> (value, support); plan: dict(brick=0 | 1, empty_test=bool) runs
    ls2fm_cloud_implicit_plan (the tests and tools/time_cloud_mesh.py), None the library's default"""
    lib = _lib.load()
    dev = points.device
    og = (ctypes.c_float * 3)(*origin)
    with torch.cuda.device(dev):
        value = torch.empty(shape, dtype=torch.float32, device=dev)
        support = torch.empty(shape, dtype=torch.float32, device=dev)
        head = (ptr(points), ptr(normals), *grid.c_args(n_first=True), *shape, og, voxel, k, float(max_d2), min_neighbors)
        if plan is None:
            check(lib.ls2fm_cloud_implicit(*head, ptr(value), ptr(support), stream_ptr()), "ls2fm_cloud_implicit")
        else:
            check(lib.ls2fm_cloud_implicit_plan(*head, int(plan["brick"]), 1 if plan["empty_test"] else 0, ptr(value), ptr(support),
                                                stream_ptr()), "ls2fm_cloud_implicit_plan")
    return value, support


@torch.no_grad()
def implicit_from_cloud(points, normals, voxel, radius=None, k=16, min_neighbors=3, bounds=None, grid=None) -> ImplicitVolume:
    """The ImplicitVolume of the cloud `points` (float32 [N, 3]) with `normals` ([N, 3], any float type; rounded to float32).
      voxel          the lattice spacing;  radius  the support radius, default 3 voxels (RADIUS_VOXELS); a lattice point farther
                     than that from every point stays undefined (NaN)
      k              neighbours per lattice point, 1 .. 32;  min_neighbors  fewer neighbours inside the radius leave NaN
      bounds         ((x0, y0, z0), (x1, y1, z1)) of the lattice, shaped as lattice.shape_for shapes it; default: the cloud's box
                     grown by the radius, which costs one host read (the box) -- give bounds to avoid it
      grid           a point_grid.PointGrid over `points` to reuse; it is used when no point had to be dropped
    Points with a non-finite coordinate or normal are dropped first, with torch ops (the count of the rest is a host read, as is
    the box of a grid built here).  One launch on the device; CPU tensors go through _implicit_torch."""
    points, normals = points3(points, "points"), points3(normals, "normals")
    if points.shape[0] != normals.shape[0] or points.device != normals.device:
        raise ValueError(f"ls2fm.cloud_mesh.implicit_from_cloud: {points.shape[0]} points on {points.device}, "
                         f"{normals.shape[0]} normals on {normals.device}")
    voxel, radius, max_d2, k, min_neighbors = _options(voxel, radius, k, min_neighbors)
    points, normals = _lib.cf(points.detach()), _lib.cf(normals.detach())
    if grid is not None and (grid.n != points.shape[0] or grid.device != points.device):
        raise ValueError(f"ls2fm.cloud_mesh.implicit_from_cloud: the grid holds {grid.n} points on {grid.device}, the cloud "
                         f"{points.shape[0]} on {points.device}")
    keep = torch.isfinite(points).all(dim=1) & torch.isfinite(normals).all(dim=1)
    kept = points[keep]
    if kept.shape[0] != points.shape[0]:
        points, normals, grid = kept, normals[keep], None
    if bounds is None:
        if not points.shape[0]:
            raise ValueError("ls2fm.cloud_mesh.implicit_from_cloud: a cloud without a finite point has no box; give bounds")
        bounds = lattice.grown_box(points, radius)
    shape, origin = _lattice(bounds, voxel)
    if not points.is_cuda:
        value, support = _implicit_torch(points, normals, shape, origin, voxel, radius, k, min_neighbors)
    else:
        grid = PointGrid(points) if grid is None else grid
        value, support = _implicit_device(points, normals, grid, shape, origin, voxel, k, max_d2, min_neighbors)
    return ImplicitVolume(value, support, origin, voxel, radius)


@torch.no_grad()
def extract(volume: ImplicitVolume, min_support=0.0) -> mesh.Mesh:
    """The mesh of the volume's zero level -> ls2fm.mesh.Mesh in the cloud's frame, faces oriented along the normals (as
    fusion.extract's toward the cameras).  A lattice point of support < min_support takes no part (lattice.zero_level), like the
    undefined ones, whose value is NaN already.  Host reads: marching cubes' counts and the sizes of the result."""
    _lib.require_device_tensors("ls2fm.cloud_mesh.extract", volume.value, volume.support, phrase=": marching cubes runs on MI355X only")
    return lattice.zero_level(volume.value, volume.support >= float(min_support), volume.voxel, volume.origin)


@torch.no_grad()
def mesh_from_cloud(points, normals=None, voxel=None, toward=None, normals_k=16, min_support=0.0, return_volume=False, **implicit):
    """Mesh a cloud: implicit_from_cloud -> extract -> ls2fm.mesh.Mesh (with return_volume: (Mesh, ImplicitVolume)).
      normals     [N, 3], or None: cloud.estimate_normals(points, k=normals_k, toward=toward) over the finite points
      toward      what orients estimated normals: a position [3] (the scanner, a point outside or inside a closed object) or one
                  per point [N, 3] (each point's camera centre: depths_to_cloud's second result).  Required without normals: the
                  largest-component orientation of estimate_normals is not a global one, and a mesh made from it would be wrong
                  silently.  Ignored when normals are given.
      voxel       the lattice spacing (required);  **implicit: radius, k, min_neighbors, bounds, grid as implicit_from_cloud"""
    if voxel is None:
        raise ValueError("ls2fm.cloud_mesh.mesh_from_cloud: voxel, the lattice spacing, is required")
    points = points3(points, "points")
    if normals is None:
        if toward is None:
            raise ValueError("ls2fm.cloud_mesh.mesh_from_cloud: without normals, toward is required: estimated normals have no "
                             "global orientation of their own")
        points = _lib.cf(points.detach())
        toward = torch.as_tensor(toward, dtype=torch.float32).to(points.device)
        finite = torch.isfinite(points).all(dim=1)
        if toward.dim() == 2 and toward.shape[0] == points.shape[0] and toward.shape[0] != 1:
            toward = toward[finite]
        points = points[finite]
        grid = implicit.get("grid")
        if grid is not None and grid.n != points.shape[0]:
            implicit["grid"] = grid = None
        if points.is_cuda and grid is None and points.shape[0]:
            implicit["grid"] = grid = PointGrid(points)
        normals = cloud.estimate_normals(points, k=normals_k, toward=toward, grid=grid)
    volume = implicit_from_cloud(points, normals, voxel, **implicit)
    out = extract(volume, min_support)
    return (out, volume) if return_volume else out
