"""Point clouds on the device: what the mapper's points, surface samples, back-projected depths and ground-truth scans need before
they are scored, meshed or registered.

  knn                    the k nearest neighbours of every query (PointGrid.knn, ls2fm_point_grid_knn, csrc/point_grid.hip)
  estimate_normals       normals (and curvature) by PCA over the k nearest (ls2fm_cloud_normals, csrc/cloud_normals.hip): what
                         metrics.icp's point-to-plane residual and metrics.normal_consistency want from a cloud that brings none
  statistical_outliers   Open3D's rule: drop the points whose mean neighbour distance lies std_ratio deviations above the mean
  radius_outliers        drop the points with fewer than min_neighbors others inside a radius
  depths_to_cloud        back-project posed depth maps into a cloud and each point's camera centre (torch ops), the input of
                         estimate_normals(toward=...) and of ls2fm.cloud_mesh.mesh_from_cloud

include/ls2fm.h states the K-NEIGHBOUR RULE and the NORMAL RULE; both make the result a pure function of the inputs, and
tests/cloud_restate.py repeats them in numpy.  _knn_torch and _normals_torch are the same rules as plain torch ops on whatever
device the tensors are on: the timing baseline, and the route CPU tensors take (as in ls2fm.image_metrics).  A device tensor never
takes them: a missing library raises.  Not here: a consistent orientation by propagation over a neighbour graph (normals are
oriented per point, toward a given position or by their largest component), k above 32, radius counts above 32.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .point_grid import KNN_MAX_K, PointGrid, knn_k, points3, squared_cutoff

_JACOBI_SWEEPS = 30                        # pose_math.h's kJacobiSweeps


# ------------------------------------------------------------------------------------------------------------- torch forms
def _knn_torch(q, ref, k, max_dist=None, skip_own=False, chunk=None):
    """The K-NEIGHBOUR RULE as plain torch ops: all M x N distances of the distance rule, `chunk` queries at a time (default: 2^24
    distances per chunk), the entries that do not qualify set to +inf, then a two-key sort on (d2, index): a stable sort of d2 over
    columns that stand in index order.  -> (idx int32 [M, k], d2 float32 [M, k], count int32 [M])"""
    q, ref = points3(q, "q").float(), points3(ref, "ref").float()
    k = knn_k(k)
    dev = q.device
    ref = ref.to(dev)
    m, n = int(q.shape[0]), int(ref.shape[0])
    if skip_own and m != n:
        raise ValueError(f"ls2fm.cloud: skip_own needs the reference cloud as queries, got {m} queries for {n} points")
    max_d2 = float(squared_cutoff(max_dist))
    inf = float("inf")
    idx = torch.full((m, k), -1, dtype=torch.int32, device=dev)
    d2_out = torch.full((m, k), inf, dtype=torch.float32, device=dev)
    count = torch.zeros(m, dtype=torch.int32, device=dev)
    if m == 0 or n == 0:
        return idx, d2_out, count
    chunk = max(1, (1 << 24) // n) if chunk is None else max(1, int(chunk))
    rx, ry, rz = ref[:, 0][None, :], ref[:, 1][None, :], ref[:, 2][None, :]
    kk = min(k, n)
    for s in range(0, m, chunk):
        c = q[s:s + chunk]
        dx, dy, dz = c[:, 0:1] - rx, c[:, 1:2] - ry, c[:, 2:3] - rz
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = (d2 <= max_d2) & (d2 < inf)
        if skip_own:
            rows = torch.arange(c.shape[0], device=dev)
            ok[rows, rows + s] = False
        d2 = torch.where(ok, d2, torch.full_like(d2, inf))
        val, order = torch.sort(d2, dim=1, stable=True)
        val, order = val[:, :kk], order[:, :kk]
        has = val < inf
        idx[s:s + chunk, :kk] = torch.where(has, order, torch.full_like(order, -1)).to(torch.int32)
        d2_out[s:s + chunk, :kk] = val
        count[s:s + chunk] = has.sum(dim=1).to(torch.int32)
    return idx, d2_out, count


def _jacobi3_torch(a):
    """jacobi3_sym on a batch: a = six fp64 [M] tensors (xx xy xz yy yz zz) -> (the three diagonals, V[k][r] as [M] tensors).  A
    matrix that has met the threshold no longer changes, so masking it out of a sweep is its `break`."""
    a = list(a)
    one, zero = torch.ones_like(a[0]), torch.zeros_like(a[0])
    V = [[one.clone() if k == r else zero.clone() for r in range(3)] for k in range(3)]
    at = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    sid = lambda i, j: at[(min(i, j), max(i, j))]          # noqa: E731
    for _ in range(_JACOBI_SWEEPS):
        dia = (a[0] * a[0] + a[3] * a[3]) + a[5] * a[5]
        off = (a[1] * a[1] + a[2] * a[2]) + a[4] * a[4]
        active = off > 1e-30 * dia
        if not bool(active.any()):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            k = 3 - p - q
            apq = a[sid(p, q)]
            rot = active & (apq != 0.0)
            theta = (a[sid(q, q)] - a[sid(p, p)]) / (2.0 * apq)
            t = torch.where(theta >= 0.0, one, -one) / (theta.abs() + torch.sqrt(theta * theta + 1.0))
            c = 1.0 / torch.sqrt(t * t + 1.0)
            s = t * c
            akp, akq = a[sid(k, p)], a[sid(k, q)]
            new = {sid(k, p): c * akp - s * akq, sid(k, q): s * akp + c * akq, sid(p, p): a[sid(p, p)] - t * apq,
                   sid(q, q): a[sid(q, q)] + t * apq, sid(p, q): zero}
            for e, v in new.items():
                a[e] = torch.where(rot, v, a[e])
            for r in range(3):
                vp, vq = V[p][r], V[q][r]
                V[p][r] = torch.where(rot, c * vp - s * vq, vp)
                V[q][r] = torch.where(rot, s * vp + c * vq, vq)
    return (a[0], a[3], a[5]), V


def _normals_torch(points, idx, queries=None, toward=None):
    """The NORMAL RULE as plain torch ops in fp64: the mean and the covariance accumulated over the list's columns in a Python
    loop, so that each add rounds once, the Jacobi as masked batch operations.
    -> (normal fp64 [M, 3], curvature fp64 [M], cov fp64 [M, 6])"""
    points = points3(points, "points").float()
    idx = torch.as_tensor(idx).to(points.device)
    m, k = int(idx.shape[0]), int(idx.shape[1])
    n_points = int(points.shape[0])
    p64 = points.to(torch.float64) if n_points else points.new_zeros((1, 3), dtype=torch.float64)
    valid = (idx >= 0) & (idx < n_points)
    safe = torch.where(valid, idx, torch.zeros_like(idx)).long()
    n = torch.zeros(m, dtype=torch.int64, device=points.device)
    s = torch.zeros(m, 3, dtype=torch.float64, device=points.device)
    for j in range(k):
        v, p = valid[:, j], p64[safe[:, j]]
        s = torch.where(v[:, None], torch.where((n == 0)[:, None], p, s + p), s)
        n = n + v
    dn = n.to(torch.float64)
    mean = s / dn[:, None]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    acc = [torch.zeros(m, dtype=torch.float64, device=points.device) for _ in pairs]
    seen = torch.zeros(m, dtype=torch.bool, device=points.device)
    for j in range(k):
        v = valid[:, j]
        d = p64[safe[:, j]] - mean
        for e, (a, b) in enumerate(pairs):
            term = d[:, a] * d[:, b]
            acc[e] = torch.where(v, torch.where(seen, acc[e] + term, term), acc[e])
        seen = seen | v
    C = [x / dn for x in acc]
    cov = torch.stack(C, dim=1)
    trace = (C[0] + C[3]) + C[5]
    ev, V = _jacobi3_torch(C)
    best = torch.zeros(m, dtype=torch.int64, device=points.device)
    lam = ev[0]
    for i in (1, 2):
        lower = ev[i] < lam
        best, lam = torch.where(lower, torch.full_like(best, i), best), torch.where(lower, ev[i], lam)
    vec = [torch.where(best == 0, V[0][r], torch.where(best == 1, V[1][r], V[2][r])) for r in range(3)]
    length = torch.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2])
    vec = [x / length for x in vec]
    if toward is not None:
        t = _toward(toward, m, points.device).to(torch.float64) - points3(queries, "queries").float().to(torch.float64)
        flip = (vec[0] * t[:, 0] + vec[1] * t[:, 1]) + vec[2] * t[:, 2] < 0.0
    else:
        big = vec[0]
        for r in (1, 2):
            big = torch.where(vec[r].abs() > big.abs(), vec[r], big)
        flip = big < 0.0
    normal = torch.stack([torch.where(flip, -x, x) for x in vec], dim=1)
    curvature = lam / ((ev[0] + ev[1]) + ev[2])
    ok = (n >= 3) & (trace != 0.0) & (trace == trace)
    nan = torch.full_like(curvature, float("nan"))
    return torch.where(ok[:, None], normal, nan[:, None]), torch.where(ok, curvature, nan), cov


# ------------------------------------------------------------------------------------------------------------------ public
def _toward(toward, m, device):
    t = torch.as_tensor(toward, dtype=torch.float32).to(device)
    if t.dim() == 1:
        t = t[None, :]
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] not in (1, m):
        raise ValueError(f"ls2fm.cloud: toward must be [3], [1, 3] or [{m}, 3], got shape {tuple(t.shape)}")
    return _lib.cf(t)


def knn(q, ref, k, max_dist=None, exclude_self=False, cell_size=None):
    """(idx int32 [M, k], d2 float32 [M, k], count int32 [M]): the k nearest references of every query by the K-NEIGHBOUR RULE
    (1 <= k <= 32; -1 / +inf in the slots without a neighbour inside max_dist).  exclude_self: the queries ARE the references
    (`q is ref` is required) and a point is not its own neighbour; a duplicate at another index still is.  `ref` may be a
    point_grid.PointGrid, which is then reused (exclude_self: pass its cloud, grid.ref, as q).  Device tensors go through the grid,
    CPU tensors through _knn_torch."""
    grid = ref if isinstance(ref, PointGrid) else None
    if exclude_self and q is not (grid.ref if grid is not None else ref):
        raise ValueError("ls2fm.cloud.knn: exclude_self needs the references themselves as queries (q is ref)")
    q = points3(q, "q")
    k = knn_k(k)
    squared_cutoff(max_dist)
    if grid is None:
        ref = points3(ref, "ref")
        if ref.device != q.device:
            raise ValueError(f"ls2fm.cloud.knn: q on {q.device}, ref on {ref.device}")
        if not q.is_cuda:
            return _knn_torch(q, ref, k, max_dist, exclude_self)
        grid = PointGrid(ref, cell_size=cell_size)
    return grid.knn(q, k, max_dist, skip_own=exclude_self)


def normals_from_neighbors(points, idx, queries=None, toward=None, return_cov=False):
    """The NORMAL RULE on a neighbour list idx int32 [M, k] into points float32 [N, 3] -> (normal fp64 [M, 3], curvature fp64 [M])
    and, with return_cov, cov fp64 [M, 6] (xx xy xz yy yz zz).  toward ([3], [1, 3] or [M, 3]) orients the normals toward that
    position as seen from `queries` [M, 3] (needed with toward); without it the largest component is made positive.  One launch
    (ls2fm_cloud_normals), nothing read back; CPU tensors go through _normals_torch."""
    points = points3(points, "points")
    idx = torch.as_tensor(idx)
    if idx.dim() != 2 or idx.shape[1] < 1 or idx.dtype != torch.int32:
        raise ValueError(f"ls2fm.cloud: idx must be int32 [M, k >= 1], got {idx.dtype} {tuple(idx.shape)}")
    m, k = int(idx.shape[0]), int(idx.shape[1])
    if toward is not None:
        if queries is None:
            raise ValueError("ls2fm.cloud: toward needs the queries' positions")
        queries = points3(queries, "queries")
        if queries.shape[0] != m:
            raise ValueError(f"ls2fm.cloud: {queries.shape[0]} queries for {m} neighbour lists")
        toward = _toward(toward, m, points.device)
    if not points.is_cuda:
        normal, curvature, cov = _normals_torch(points, idx, queries, toward)
        return (normal, curvature, cov) if return_cov else (normal, curvature)
    _lib.require_device_tensors("ls2fm.cloud", idx, queries)
    dev = points.device
    points, idx = _lib.cf(points), idx.contiguous()
    queries = None if toward is None else _lib.cf(queries)
    with torch.cuda.device(dev):
        normal = torch.empty(m, 3, dtype=torch.float64, device=dev)
        curvature = torch.empty(m, dtype=torch.float64, device=dev)
        cov = torch.empty(m, 6, dtype=torch.float64, device=dev) if return_cov else None
        check(_lib.load().ls2fm_cloud_normals(ptr(points), int(points.shape[0]), ptr(idx), m, k, ptr(queries), ptr(toward),
                                              0 if toward is None else int(toward.shape[0]), ptr(normal), ptr(curvature), ptr(cov),
                                              stream_ptr()), "ls2fm_cloud_normals")
    return (normal, curvature, cov) if return_cov else (normal, curvature)


def estimate_normals(points, k=16, max_dist=None, toward=None, grid=None, return_curvature=False, dtype=torch.float32):
    """Normals of the cloud `points` (float32 [N, 3]) -> [N, 3] of `dtype` (float32: the rounding of the fp64 result), and with
    return_curvature the surface variation lambda_0 / (lambda_0 + lambda_1 + lambda_2) as well.  Each normal is the eigenvector of
    the smallest eigenvalue of the covariance of the point's k nearest neighbours inside max_dist, the point itself among them
    (k counts it, as Open3D's KNN search does); fewer than 3 neighbours or a neighbourhood without extent give NaN.  toward (a
    position [3] / [1, 3], e.g. the camera or scanner, or one per point [N, 3]) orients them; without it the largest component is
    positive, which is consistent across a smooth patch but not a global orientation.  grid: a point_grid.PointGrid over `points` to
    reuse.  Two launches on the device (knn, normals), nothing read back once the grid exists."""
    points = points3(points, "points")
    if grid is not None and grid.n != points.shape[0]:
        raise ValueError(f"ls2fm.cloud.estimate_normals: the grid holds {grid.n} points, the cloud {points.shape[0]}")
    if points.is_cuda:
        idx, _, _ = (grid if grid is not None else PointGrid(points)).knn(points, k, max_dist)
    else:
        idx, _, _ = _knn_torch(points, points, k, max_dist)
    normal, curvature = normals_from_neighbors(points, idx, points, toward)
    normal, curvature = normal.to(dtype), curvature.to(dtype)
    return (normal, curvature) if return_curvature else normal


def _self_neighbours(points, k, max_dist):
    """(d2 float32 [N, k], count int32 [N]) of every point's k nearest OTHER points.  On the device the cloud is first put into the
    order of its cells and the results put back: skip_own knows a query by its position, so the queries cannot be reordered
    under the grid, but the cloud can before the grid is built -- no result depends on it (the indices would; they are not used)."""
    if not points.is_cuda:
        _, d2, count = _knn_torch(points, points, k, max_dist, skip_own=True)
        return d2, count
    points = _lib.cf(points)
    n = int(points.shape[0])
    if n < 2:
        _, d2, count = PointGrid(points).knn(points, k, max_dist, skip_own=True)
        return d2, count
    perm = PointGrid(points).cell_order(points)
    moved = points[perm]
    _, d2, count = PointGrid(moved).knn(moved, k, max_dist, skip_own=True)
    return torch.empty_like(d2).index_copy_(0, perm, d2), torch.empty_like(count).index_copy_(0, perm, count)


def statistical_outliers(points, k=20, std_ratio=2.0):
    """(keep bool [N], mean_dist fp64 [N]) by Open3D's statistical rule: mean_dist is the fp64 mean of sqrt(double(d2)) over a
    point's k nearest OTHER points (fewer when the cloud is smaller; NaN without any, and such a point is dropped), mu and sigma
    the mean and the population deviation of the finite mean_dist, and a point is kept when mean_dist <= mu + std_ratio sigma."""
    points = points3(points, "points")
    if not (np.isfinite(std_ratio) and std_ratio >= 0):
        raise ValueError(f"ls2fm.cloud.statistical_outliers: std_ratio {std_ratio} must be finite and >= 0")
    d2, count = _self_neighbours(points, knn_k(k), None)
    dist = torch.sqrt(d2.to(torch.float64))
    dist = torch.where(d2 < float("inf"), dist, torch.zeros_like(dist))
    mean = dist.sum(dim=1) / count.to(torch.float64)                              # 0 / 0 = NaN: no neighbour
    finite = torch.isfinite(mean)
    nf = finite.sum().to(torch.float64)
    zero = torch.zeros_like(mean)
    mu = torch.where(finite, mean, zero).sum() / nf
    dev = torch.where(finite, mean - mu, zero)
    sigma = torch.sqrt((dev * dev).sum() / nf)
    return mean <= mu + float(std_ratio) * sigma, mean


def radius_outliers(points, radius, min_neighbors):
    """keep bool [N]: the points with at least min_neighbors OTHER points within `radius` (d2 <= float32(radius)^2), 1 <=
    min_neighbors <= 32.  One knn with k = min_neighbors: a point is kept when its list came back full, exact in integers."""
    points = points3(points, "points")
    if isinstance(min_neighbors, bool) or int(min_neighbors) != min_neighbors or not 1 <= int(min_neighbors) <= KNN_MAX_K:
        raise ValueError(f"ls2fm.cloud.radius_outliers: min_neighbors {min_neighbors} must be an integer in [1, {KNN_MAX_K}]")
    if radius is None:
        raise ValueError("ls2fm.cloud.radius_outliers: radius None is no radius")
    squared_cutoff(radius)
    _, count = _self_neighbours(points, int(min_neighbors), radius)
    return count == int(min_neighbors)


@torch.no_grad()
def depths_to_cloud(depth, pose, intr, stride=1, max_depth=float("inf")):
    """Back-project depth maps into one cloud -> (points float32 [M, 3], centers float32 [M, 3]).
      depth        float [V, H, W] or [H, W], camera z pixel for pixel (the convention of raster.rasterize, image.trace_image,
                   mvs and fusion.integrate).  A pixel that is not finite, not positive or above max_depth gives no point.
      pose, intr   [V, 3, 4] (or [3, 4]) world-to-camera [R | t] and [3, 3] or [V, 3, 3], as ls2fm/_posed.py takes them
      stride       every stride-th row and column
    Pixel (px, py) of depth d is the world point R^T (((px + 0.5 - cx) / fx d, (py + 0.5 - cy) / fy d, d) - t): the pixel's centre,
    which the rasteriser's projection puts back on (px + 0.5, py + 0.5) at c_z = d.  centers holds each point's camera centre
    -R^T t: the per-point `toward` of estimate_normals.  The points come view by view, row by row.  torch ops only, in fp64 and
    rounded once to float32, on the depth's device; the size of the result is a host read."""
    depth = torch.as_tensor(depth)
    if depth.dim() == 2:
        depth = depth[None]
    dev = depth.device
    P = torch.as_tensor(pose).detach().to(dev)
    if depth.dim() != 3 or P.dim() not in (2, 3) or tuple(P.shape[-2:]) != (3, 4):
        raise ValueError(f"ls2fm.cloud.depths_to_cloud: depth must be [V, H, W] and pose [V, 3, 4], got {tuple(depth.shape)} and {tuple(P.shape)}")
    P = P.reshape(-1, 3, 4).to(torch.float64)
    n, H, W = (int(s) for s in depth.shape)
    K = torch.as_tensor(intr).detach().to(dev)
    if K.dim() not in (2, 3) or tuple(K.shape[-2:]) != (3, 3) or K.reshape(-1, 3, 3).shape[0] not in (1, n) or P.shape[0] != n:
        raise ValueError(f"ls2fm.cloud.depths_to_cloud: {P.shape[0]} poses and intr {tuple(K.shape)} for {n} depth maps")
    K = K.reshape(-1, 3, 3).to(torch.float64).expand(n, 3, 3)
    if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
        raise ValueError(f"ls2fm.cloud.depths_to_cloud: stride {stride} must be an integer >= 1")
    max_depth = float(max_depth)
    if not max_depth > 0.0:
        raise ValueError(f"ls2fm.cloud.depths_to_cloud: max_depth {max_depth} must be positive (inf is allowed)")
    py, px = torch.arange(0, H, int(stride), device=dev), torch.arange(0, W, int(stride), device=dev)
    d = depth.detach()[:, py][:, :, px].to(torch.float64)                              # [V, h, w]
    ok = torch.isfinite(d) & (d > 0) & (d <= max_depth)
    u = (px.to(torch.float64) + 0.5)[None, None, :]
    v = (py.to(torch.float64) + 0.5)[None, :, None]
    fx, fy, cx, cy = (K[:, a, b][:, None, None] for a, b in ((0, 0), (1, 1), (0, 2), (1, 2)))
    cam = torch.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], dim=-1)               # [V, h, w, 3]
    R, t = P[:, :, :3], P[:, :, 3]
    world = torch.einsum("vji,vhwj->vhwi", R, cam - t[:, None, None, :])               # R^T (c - t)
    centre = -torch.einsum("vji,vj->vi", R, t)
    centers = centre[:, None, None, :].expand_as(world)
    return world[ok].float(), centers[ok].float()
