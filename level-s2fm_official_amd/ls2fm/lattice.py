"""The dense lattice under ls2fm.fusion's TsdfVolume and ls2fm.cloud_mesh's ImplicitVolume, stated once: lattice point i of an axis
sits at fl32(fl32((float32) i * voxel) + origin) -- marching cubes' vertex expression with spacing = (voxel,) * 3 -- so a mesh
extracted from a volume is in the frame of what filled it.  csrc/lattice.h is the device side; tests/fusion_restate.lattice is the
numpy restatement that `points` is held to by its bits."""
import math

import torch

from . import mesh


def shape_for(bounds, voxel, refusal):
    """(shape, origin) of the lattice over bounds = ((x0, y0, z0), (x1, y1, z1)): origin at the low corner, per axis
    ceil((high - low) / voxel) + 1 points, at least 2.  A voxel that is not positive and finite, or bounds that are not two finite
    corners, raise ValueError(refusal.format(voxel=, lo=, hi=)): the caller owns the message, and any further limit on the shape."""
    lo, hi = ([float(v) for v in b] for b in bounds)
    voxel = float(voxel)
    if not 0.0 < voxel < math.inf or len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in lo + hi):
        raise ValueError(refusal.format(voxel=voxel, lo=lo, hi=hi))
    return tuple(max(2, int(math.ceil((h - l) / voxel)) + 1) for l, h in zip(lo, hi)), tuple(lo)


def points(shape, origin, voxel, device):
    """(x, y, z), float32 [nx ny nz] each: the lattice expression as torch ops, axis 2 fastest"""
    axes = [torch.arange(s, device=device).float() * voxel + o for s, o in zip(shape, origin)]
    return tuple(t.reshape(-1) for t in torch.meshgrid(*axes, indexing="ij"))


def grown_box(x, margin):
    """the default bounds: the box of x [N, 3] (N >= 1; the caller refuses an empty one) grown by `margin`; one host read"""
    lo, hi = (t.tolist() for t in torch.stack([x.amin(dim=0), x.amax(dim=0)]).cpu())
    return [t - margin for t in lo], [t + margin for t in hi]


def zero_level(values, defined, voxel, origin) -> mesh.Mesh:
    """The mesh of the zero level of `values` [nx, ny, nz] over the lattice points where `defined` holds.  The others become NaN,
    which marching cubes' rule reads as "not below", so an edge from a below corner to one of them gets a NaN vertex; every face
    with a non-finite vertex coordinate is then dropped and the vertices no face uses, both in their order (mesh.finite_faces)."""
    with torch.cuda.device(values.device):
        vol = torch.where(defined, values, torch.full_like(values, math.nan))
        verts, faces = mesh.marching_cubes(vol, 0.0, spacing=(voxel,) * 3, origin=origin)
        return mesh.finite_faces(verts, faces)
