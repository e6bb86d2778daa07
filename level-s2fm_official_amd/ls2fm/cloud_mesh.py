"""Meshing an oriented point cloud on the device: from a scan, a filtered MVS cloud or the mapper's points to a surface.

  ImplicitVolume        a dense lattice of signed distances to the cloud's local planes and of their weights (TsdfVolume's layout)
  implicit_from_cloud   the volume of a cloud with normals (ls2fm_cloud_implicit, csrc/cloud_implicit.hip): one launch
  extract               the mesh of the volume's zero level over the defined lattice points (ls2fm.mesh.marching_cubes)
  PoissonVolume         the same lattice holding the indicator chi of a screened Poisson solve and the splatted density
  poisson_from_cloud    the PoissonVolume of a cloud with normals (ls2fm_poisson_solve, csrc/poisson.hip): a splat, a right-hand side
                        and a fixed number of geometric multigrid cycles on the dense lattice; poisson_residual says how far they got
  mesh_from_cloud       estimate_normals (when the cloud brings none) -> implicit_from_cloud or, with method="poisson",
                        poisson_from_cloud -> extract (-> trim); the result goes into metrics.evaluate_mesh, raster.clean_mesh,
                        mesh_colors.photo_colors and simplify.simplify as it stands
  cloud.depths_to_cloud gives the route its input from depth maps: mvs.filter_depths -> depths_to_cloud ->
                        cloud.statistical_outliers -> mesh_from_cloud is the classical dense route without a volume of depth maps

THE IMPLICIT RULE is stated in include/ls2fm.h and restated in numpy in tests/cloud_mesh_restate.py: a lattice point takes its k
nearest cloud points within the radius (the K-NEIGHBOUR RULE), weighs each by (1 - d2 / radius^2)^3 and averages the signed
distances to their tangent planes, in fp64 in list order.  The value is a pure function of the cloud, the normals, the lattice, k,
the radius and min_neighbors: no grid, brick, batch or rerun shows in it.  _implicit_torch is the same rule as plain torch ops on
whatever device the tensors are on: the timing baseline, and the route CPU tensors take.  A device tensor never takes it: a
missing library raises.

THE POISSON RULE is stated in include/ls2fm.h and restated in numpy in tests/poisson_restate.py: the normals are splatted
trilinearly with integer atomics, the right-hand side is the divergence of the edge targets, and chi solves the graph Laplacian
with a lumped screening term screen * W by W-cycles of red-black Gauss-Seidel; every lattice operation is one rounded fp32
operation, so the kernels, _poisson_torch and the restatement agree by bits.  The surface is the ZERO level of chi (positive
outside, like the implicit value): extract takes a PoissonVolume as it stands.  A global solve closes holes -- also those that
should stay open, which mesh_from_cloud's trim removes again.

Deviations from what surface-reconstruction packages do, on purpose.  The implicit route: a local moving-least-squares surface --
holes stay holes and nothing is extrapolated beyond the radius; k <= 32, so where more than 32 points lie in the support ball the
list truncates and the value steps slightly; the lattice is dense (8 bytes per lattice point); structures thinner than two voxels
merge or vanish.  The Poisson route: a trilinear (degree-1) splat and a lumped screening term, not degree-2 B-splines and point
interpolation; a dense lattice, 16 bytes per lattice point plus the workspace, no octree; no density-based scaling of the normals;
isotropic coarsening only, so a lattice much thinner along one axis stops coarsening early and converges slowly (poisson_residual
shows it); a fixed cycle count.  Both: no colour in the volume (mesh_colors.photo_colors colours the mesh); no gradients.
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
    """The mesh of the volume's zero level (an ImplicitVolume or a PoissonVolume) -> ls2fm.mesh.Mesh in the cloud's frame, faces
    oriented along the normals (as fusion.extract's toward the cameras).  A lattice point of support < min_support takes no part
    (lattice.zero_level), like the undefined ones, whose value is NaN already.  Host reads: marching cubes' counts and the sizes of
    the result."""
    _lib.require_device_tensors("ls2fm.cloud_mesh.extract", volume.value, volume.support, phrase=": marching cubes runs on MI355X only")
    return lattice.zero_level(volume.value, volume.support >= float(min_support), volume.voxel, volume.origin)


# ------------------------------------------------------------------------------------------------------ screened Poisson
POISSON_BRICK = (2, 2, 128)         # the sweep kernel's brick (include/ls2fm.h: LS2FM_POISSON_BRICK_X, _Y, _Z)
POISSON_TAIL_POINTS = 4096          # LS2FM_POISSON_TAIL_POINTS: from the first level this small downward one launch runs the sub-cycle
POISSON_COARSEST_SWEEPS, POISSON_EDGE_SWEEPS = 32, 2


class PoissonVolume:
    """value (chi) and support (the splatted density W) float32 [nx, ny, nz] of THE POISSON RULE on one device, on the lattice of
    ls2fm/lattice.py.  The surface is the zero level of value, positive on the side the normals point to; every lattice point is
    defined."""

    def __init__(self, value, support, origin, voxel, screen):
        self.value, self.support = value, support
        self.shape = tuple(int(s) for s in value.shape)
        self.origin, self.voxel, self.screen = tuple(float(v) for v in origin), float(voxel), float(screen)

    @property
    def device(self):
        return self.value.device


def poisson_levels(shape):
    """the shapes of the multigrid levels: a coarse side is (n + 1) // 2, and level l + 1 exists while level l has its smallest
    side >= 4 and its largest >= 5"""
    out = [tuple(int(s) for s in shape)]
    while min(out[-1]) >= 4 and max(out[-1]) >= 5:
        out.append(tuple((n + 1) // 2 for n in out[-1]))
    return out


def _poisson_options(screen, cycles, gamma):
    screen = float(screen)
    if not 0.0 < screen < math.inf or not 0.0 < float(torch.tensor(screen, dtype=torch.float32)) < math.inf:
        raise ValueError(f"ls2fm.cloud_mesh: screen {screen} must be positive and finite in fp32")
    if isinstance(cycles, bool) or int(cycles) != cycles or int(cycles) < 0:
        raise ValueError(f"ls2fm.cloud_mesh: cycles {cycles} must be an integer >= 0")
    if isinstance(gamma, bool) or gamma not in (1, 2):
        raise ValueError(f"ls2fm.cloud_mesh: gamma {gamma} must be 1 (V-cycle) or 2 (W-cycle)")
    return screen, int(cycles), int(gamma)


def _poisson_lattice(shape):
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 2 or max(shape) > 2 ** 24 or shape[0] * shape[1] >= 2 ** 31 or math.prod(shape) >= 2 ** 31:
        raise ValueError(f"ls2fm.cloud_mesh: a Poisson lattice of {shape} points: every side in 2 .. 2^24, fewer than 2^31 points")
    return shape


def _axis(axis, s):
    idx = [slice(None)] * 3
    idx[axis] = s
    return tuple(idx)


def _splat_torch(points, normals, shape, origin, voxel):
    """the splat and the finish of THE POISSON RULE -> (V float32 [3, nx, ny, nz], W float32 [nx, ny, nz]); the fixed-point sums
    go through index_add_ on int64"""
    dev = points.device
    total = math.prod(shape)
    acc = torch.zeros(4, total, dtype=torch.int64, device=dev)
    if points.shape[0]:
        n = torch.tensor(shape, dtype=torch.int64, device=dev)
        u = (points - torch.tensor(origin, dtype=torch.float32, device=dev)) / torch.tensor(voxel, dtype=torch.float32, device=dev)
        i = torch.floor(u)
        f = u - i
        ok = torch.isfinite(points).all(dim=1) & torch.isfinite(normals).all(dim=1) & (u >= 0).all(dim=1) & (u < (n - 1).float()).all(dim=1)
        i, f, N = i[ok].long(), f[ok], normals[ok].double()
        for dx in (0, 1):
            wx = f[:, 0] if dx else 1.0 - f[:, 0]
            for dy in (0, 1):
                wxy = wx * (f[:, 1] if dy else 1.0 - f[:, 1])
                for dz in (0, 1):
                    w = (wxy * (f[:, 2] if dz else 1.0 - f[:, 2])).double()
                    at = ((i[:, 0] + dx) * shape[1] + (i[:, 1] + dy)) * shape[2] + (i[:, 2] + dz)
                    for a in range(3):
                        acc[a].index_add_(0, at, torch.round(w * N[:, a] * 2.0 ** 32).long())
                    acc[3].index_add_(0, at, torch.round(w * 2.0 ** 32).long())
    out = (acc.double() * 2.0 ** -32).float().view(4, *shape)
    return out[:3], out[3].contiguous()


def _rhs_torch(V):
    shape = tuple(V.shape[1:])
    t = []
    for a in range(3):
        g = 0.5 * (V[a][_axis(a, slice(0, -1))] + V[a][_axis(a, slice(1, None))])
        pad = torch.zeros(tuple(s + (1 if x == a else 0) for x, s in enumerate(shape)), dtype=torch.float32, device=V.device)
        pad[_axis(a, slice(1, -1))] = g
        t.append(pad[_axis(a, slice(0, -1))] - pad[_axis(a, slice(1, None))])
    return (t[0] + t[1]) + t[2]


def _neighbour_sum_torch(chi):
    """(N, deg): the existing neighbours in the order -0, +0, -1, +1, -2, +2 from the first that exists, and their count"""
    N, deg = torch.zeros_like(chi), torch.zeros_like(chi)
    has = torch.zeros(chi.shape, dtype=torch.bool, device=chi.device)
    for a in range(3):
        for lo, hi in ((slice(1, None), slice(0, -1)), (slice(0, -1), slice(1, None))):
            nb, ex = torch.zeros_like(chi), torch.zeros_like(has)
            nb[_axis(a, lo)] = chi[_axis(a, hi)]
            ex[_axis(a, lo)] = True
            N = torch.where(ex, torch.where(has, N + nb, nb), N)
            has = has | ex
            deg = deg + ex.float()
    return N, deg


def _parity(shape, device):
    i0, i1, i2 = torch.meshgrid(*(torch.arange(s, device=device) for s in shape), indexing="ij")
    return (i0 + i1 + i2) & 1


def _f32(v, device):
    return torch.tensor(float(v), dtype=torch.float32, device=device)


def _sweep_colour_torch(chi, b, W, s, a, colour):
    N, deg = _neighbour_sum_torch(chi)
    s, a = _f32(s, chi.device), _f32(a, chi.device)
    return torch.where(_parity(chi.shape, chi.device) == colour, (b + s * N) / (s * deg + a * W), chi)


def _sweeps_torch(chi, b, W, s, a, count):
    for _ in range(count):
        chi = _sweep_colour_torch(_sweep_colour_torch(chi, b, W, s, a, 0), b, W, s, a, 1)
    return chi


def _residual_torch(chi, b, W, s, a):
    N, deg = _neighbour_sum_torch(chi)
    s, a = _f32(s, chi.device), _f32(a, chi.device)
    return b - (s * (deg * chi - N) + (a * W) * chi)


def _restrict_torch(r):
    """the transpose of the prolongation, halved per axis, the axes 0, 1, 2 in turn"""
    for axis in range(3):
        r = r.movedim(axis, 0)
        n = r.shape[0]
        nc, m = (n + 1) // 2, n // 2
        acc = 0.5 * r[0::2]
        acc[1:] = acc[1:] + 0.25 * r[1:2 * nc - 2:2]
        c = torch.full((m, 1, 1), 0.25, dtype=torch.float32, device=r.device)
        if n % 2 == 0:
            c[-1] = 0.5
        acc[:m] = acc[:m] + c * r[1::2]
        r = acc.movedim(0, axis)
    return r.contiguous()


def _prolong_torch(e, shape):
    for axis in range(3):
        e = e.movedim(axis, 0)
        n, nc = shape[axis], e.shape[0]
        out = torch.empty((n,) + tuple(e.shape[1:]), dtype=torch.float32, device=e.device)
        out[0::2] = e
        k = torch.arange(n // 2, device=e.device)
        out[1::2] = 0.5 * (e[k] + e[torch.clamp(k + 1, max=nc - 1)])
        e = out.movedim(0, axis)
    return e.contiguous()


def _cycle_torch(level, chi, b, Ws, a, gamma):
    s = 4.0 ** -level
    if level == len(Ws) - 1:
        return _sweeps_torch(chi, b, Ws[level], s, a, POISSON_COARSEST_SWEEPS)
    chi = _sweeps_torch(chi, b, Ws[level], s, a, POISSON_EDGE_SWEEPS)
    for _ in range(gamma):
        coarse_b = _restrict_torch(_residual_torch(chi, b, Ws[level], s, a))
        chi = chi + _prolong_torch(_cycle_torch(level + 1, torch.zeros_like(coarse_b), coarse_b, Ws, a, gamma), chi.shape)
    return _sweeps_torch(chi, b, Ws[level], s, a, POISSON_EDGE_SWEEPS)


@torch.no_grad()
def _poisson_torch(points, normals, shape, origin, voxel, screen=4.0, cycles=8, gamma=2):
    """THE POISSON RULE as plain torch ops on the points' device -> (value, density) float32 [nx, ny, nz]: the timing baseline, and
    the route CPU tensors take.  Every lattice operation is one torch op, so each rounds once."""
    points, normals = points3(points, "points").float(), points3(normals, "normals").float()
    screen, cycles, gamma = _poisson_options(screen, cycles, gamma)
    shape = _poisson_lattice(shape)
    V, W = _splat_torch(points, normals, shape, origin, voxel)
    b = _rhs_torch(V)
    Ws = [W]
    for _ in poisson_levels(shape)[1:]:
        Ws.append(_restrict_torch(Ws[-1]))
    chi = torch.zeros_like(b)
    for _ in range(cycles):
        chi = _cycle_torch(0, chi, b, Ws, screen, gamma)
    return chi.contiguous(), W


def _poisson_workspace(shape, device):
    size = int(_lib.load().ls2fm_poisson_workspace_bytes(*shape))
    if size < 0:
        raise ValueError(f"ls2fm.cloud_mesh: ls2fm_poisson_workspace_bytes refuses a lattice of {shape} points")
    return torch.empty(size, dtype=torch.uint8, device=device)


def _poisson_device(points, normals, shape, origin, voxel, screen, cycles, gamma, tail_points=None):
    """one ls2fm_poisson_solve on converted arguments -> (value, density); tail_points: 0 or POISSON_TAIL_POINTS runs
    ls2fm_poisson_solve_plan (the tests and tools/time_poisson.py), None the library's default"""
    lib = _lib.load()
    dev = points.device
    og = (ctypes.c_float * 3)(*origin)
    with torch.cuda.device(dev):
        value = torch.empty(shape, dtype=torch.float32, device=dev)
        density = torch.empty(shape, dtype=torch.float32, device=dev)
        ws = _poisson_workspace(shape, dev)
        head = (ptr(points), ptr(normals), int(points.shape[0]), *shape, og, voxel, screen, cycles, gamma)
        tail = (ptr(value), ptr(density), ptr(ws), ws.numel(), stream_ptr())
        if tail_points is None:
            check(lib.ls2fm_poisson_solve(*head, *tail), "ls2fm_poisson_solve")
        else:
            check(lib.ls2fm_poisson_solve_plan(*head, int(tail_points), *tail), "ls2fm_poisson_solve_plan")
    return value, density


def _poisson_splat_device(points, normals, shape, origin, voxel):
    """the splat, the finish and the right-hand side alone (ls2fm_poisson_splat) -> (V [3, nx, ny, nz], b, W)"""
    dev = points.device
    with torch.cuda.device(dev):
        V = torch.empty((3,) + tuple(shape), dtype=torch.float32, device=dev)
        b, W = torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev)
        ws = torch.empty(32 * math.prod(shape), dtype=torch.uint8, device=dev)
        check(_lib.load().ls2fm_poisson_splat(ptr(points), ptr(normals), int(points.shape[0]), *shape, (ctypes.c_float * 3)(*origin), voxel,
                                              ptr(V), ptr(b), ptr(W), ptr(ws), ws.numel(), stream_ptr()), "ls2fm_poisson_splat")
    return V, b, W


def _poisson_sweep_colour_device(chi, b, W, s, screen, colour):
    """one colour of one sweep in place (ls2fm_poisson_sweep_colour) -> chi"""
    with torch.cuda.device(chi.device):
        check(_lib.load().ls2fm_poisson_sweep_colour(ptr(chi), ptr(b), ptr(W), *chi.shape, s, screen, colour, stream_ptr()),
              "ls2fm_poisson_sweep_colour")
    return chi


def _poisson_restrict_device(chi, b=None, W=None, s=1.0, screen=1.0):
    """R of the residual of (chi, b, W) at scale s, or with b = W = None R chi itself (ls2fm_poisson_restrict) -> the coarse field"""
    with torch.cuda.device(chi.device):
        coarse = torch.empty(tuple((n + 1) // 2 for n in chi.shape), dtype=torch.float32, device=chi.device)
        check(_lib.load().ls2fm_poisson_restrict(ptr(chi), None if b is None else ptr(b), None if W is None else ptr(W), *chi.shape, s, screen,
                                                 ptr(coarse), stream_ptr()), "ls2fm_poisson_restrict")
    return coarse


def _poisson_prolong_device(chi, coarse):
    """chi += P coarse in place (ls2fm_poisson_prolong) -> chi"""
    with torch.cuda.device(chi.device):
        check(_lib.load().ls2fm_poisson_prolong(ptr(chi), *chi.shape, ptr(coarse), stream_ptr()), "ls2fm_poisson_prolong")
    return chi


def _oriented(points, normals, who):
    """the rows with a finite point and a finite non-zero normal, the normals normalised (float32): what the Poisson route takes"""
    points, normals = points3(points, "points"), points3(normals, "normals")
    if points.shape[0] != normals.shape[0] or points.device != normals.device:
        raise ValueError(f"ls2fm.cloud_mesh.{who}: {points.shape[0]} points on {points.device}, {normals.shape[0]} normals on "
                         f"{normals.device}")
    points, normals = _lib.cf(points.detach()), _lib.cf(normals.detach())
    length = torch.linalg.vector_norm(normals, dim=1)
    keep = torch.isfinite(points).all(dim=1) & torch.isfinite(normals).all(dim=1) & (length > 0) & torch.isfinite(length)
    return points[keep].contiguous(), (normals[keep] / length[keep, None]).contiguous()


@torch.no_grad()
def poisson_from_cloud(points, normals, voxel, screen=4.0, cycles=8, gamma=2, bounds=None) -> PoissonVolume:
    """The PoissonVolume of the cloud `points` (float32 [N, 3]) with `normals` ([N, 3], any float type; rounded to float32).
      voxel    the lattice spacing
      screen   the weight of the screening term screen * W chi^2, which pins the zero level to the points (4, the usual default)
      cycles   multigrid cycles, a fixed count (no stopping test, no host read): poisson_residual tells whether they were enough
      gamma    2 (W-cycle, the default: the restricted density is a rough coefficient) or 1 (V-cycle)
      bounds   ((x0, y0, z0), (x1, y1, z1)) of the lattice; default: the cloud's box grown by 10 % of its longest side plus 2
               voxels, which costs one host read (the box) -- give bounds to avoid it.  Points outside the lattice add nothing.
    Rows with a non-finite coordinate or normal or a zero normal are dropped and the normals normalised first, with torch ops (the
    count of the rest is a host read).  One ls2fm_poisson_solve on the device; CPU tensors go through _poisson_torch."""
    voxel = float(voxel)
    if not 0.0 < voxel < math.inf:
        raise ValueError(f"ls2fm.cloud_mesh: voxel {voxel} must be positive and finite")
    screen, cycles, gamma = _poisson_options(screen, cycles, gamma)
    points, normals = _oriented(points, normals, "poisson_from_cloud")
    if bounds is None:
        if not points.shape[0]:
            raise ValueError("ls2fm.cloud_mesh.poisson_from_cloud: a cloud without a finite oriented point has no box; give bounds")
        lo, hi = lattice.grown_box(points, 0.0)
        margin = 0.1 * max(h - l for l, h in zip(lo, hi)) + 2.0 * voxel
        bounds = [v - margin for v in lo], [v + margin for v in hi]
    shape, origin = _lattice(bounds, voxel)
    shape = _poisson_lattice(shape)
    if not points.is_cuda:
        value, density = _poisson_torch(points, normals, shape, origin, voxel, screen, cycles, gamma)
    else:
        value, density = _poisson_device(points, normals, shape, origin, voxel, screen, cycles, gamma)
    return PoissonVolume(value, density, origin, voxel, screen)


@torch.no_grad()
def poisson_residual(volume: PoissonVolume, points, normals) -> float:
    """max |r| / max |b| of the volume's chi in the level-0 equations of its cloud, as torch ops on the volume's device (0 when b
    vanishes): whether `cycles` was enough.  The right-hand side is formed again from the cloud; one host read."""
    points, normals = _oriented(points, normals, "poisson_residual")
    V, W = _splat_torch(points.to(volume.device), normals.to(volume.device), volume.shape, volume.origin, volume.voxel)
    b = _rhs_torch(V)
    top, r = (float(v) for v in torch.stack([b.abs().max(), _residual_torch(volume.value, b, W, 1.0, volume.screen).abs().max()]).cpu())
    return r / top if top > 0 else 0.0


def _trim(out, points, radius):
    """the faces of `out` whose three vertices lie within `radius` of the cloud (PointGrid.query), compacted"""
    if not out.faces.shape[0] or not points.shape[0]:
        return mesh.select_faces(out.vertices, out.faces, torch.zeros(out.faces.shape[0], dtype=torch.bool, device=out.faces.device))
    idx, _ = PointGrid(points).query(out.vertices, float(radius))
    return mesh.select_faces(out.vertices, out.faces, (idx >= 0)[out.faces.long()].all(dim=1))


@torch.no_grad()
def mesh_from_cloud(points, normals=None, voxel=None, toward=None, normals_k=16, min_support=0.0, return_volume=False, method="mls",
                    trim=None, **implicit):
    """Mesh a cloud: implicit_from_cloud or poisson_from_cloud -> extract -> ls2fm.mesh.Mesh (with return_volume: (Mesh, volume), an
    ImplicitVolume or a PoissonVolume by the method).
      method      "mls": the local surface of implicit_from_cloud (the default);  "poisson": poisson_from_cloud, whose zero level is
                  closed -- **implicit are then screen, cycles, gamma, bounds; a grid is used for the normals only, and any other
                  keyword (radius, k, min_neighbors) is refused
      trim        a distance, or None: faces with a vertex farther than that from every cloud point are dropped (PointGrid.query on
                  the vertices, then select_faces' compaction), which opens again what a global solve closed but should stay open
      normals     [N, 3], or None: cloud.estimate_normals(points, k=normals_k, toward=toward) over the finite points
      toward      what orients estimated normals: a position [3] (the scanner, a point outside or inside a closed object) or one
                  per point [N, 3] (each point's camera centre: depths_to_cloud's second result).  Required without normals: the
                  largest-component orientation of estimate_normals is not a global one, and a mesh made from it would be wrong
                  silently.  Ignored when normals are given.
      voxel       the lattice spacing (required);  **implicit: radius, k, min_neighbors, bounds, grid as implicit_from_cloud"""
    if voxel is None:
        raise ValueError("ls2fm.cloud_mesh.mesh_from_cloud: voxel, the lattice spacing, is required")
    if method not in ("mls", "poisson"):
        raise ValueError(f"ls2fm.cloud_mesh.mesh_from_cloud: method {method!r} is neither 'mls' nor 'poisson'")
    if trim is not None and not 0.0 <= float(trim) < math.inf:
        raise ValueError(f"ls2fm.cloud_mesh.mesh_from_cloud: trim {trim} must be a finite distance >= 0, or None")
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
    if method == "poisson":
        implicit.pop("grid", None)
        unknown = sorted(set(implicit) - {"screen", "cycles", "gamma", "bounds"})
        if unknown:
            raise ValueError(f"ls2fm.cloud_mesh.mesh_from_cloud: method 'poisson' takes screen, cycles, gamma and bounds (and ignores "
                             f"grid), not {', '.join(unknown)}")
        volume = poisson_from_cloud(points, normals, voxel, **implicit)
    else:
        volume = implicit_from_cloud(points, normals, voxel, **implicit)
    out = extract(volume, min_support)
    if trim is not None:
        cloud_points = _lib.cf(points3(points, "points").detach())
        out = _trim(out, cloud_points[torch.isfinite(cloud_points).all(dim=1)].contiguous(), trim)
    return (out, volume) if return_volume else out
