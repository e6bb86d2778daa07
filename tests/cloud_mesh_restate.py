"""numpy restatement of ls2fm.cloud_mesh, written for this project (no device, no torch): THE IMPLICIT RULE of include/ls2fm.h on
top of cloud_restate.knn (brute force), the two sums accumulated in float64 one list column at a time so that each add rounds
once, and the zero crossings of a volume on its lattice edges, which the property tests measure."""
import numpy as np

import cloud_restate as R
import metrics_restate as MR
from fusion_restate import lattice as lattice_points       # float32 [nx ny nz, 3], axis 2 fastest: the one restatement of the lattice

F32 = np.float32


def neighbours(points, shape, origin, voxel, radius, k=32):
    """cloud_restate.knn of every lattice point: (idx [M, k], d2 [M, k], count [M]); cloud_scenes.prefix cuts it to a smaller k"""
    return R.knn(lattice_points(shape, origin, voxel), points, k, radius)


def sums(points, normals, X, lists, radius):
    """(num fp64 [M], den fp64 [M], n int [M]) of the lists' entries in list order, both sums starting from their first term"""
    idx, d2, _ = lists
    p, nrm, X = np.asarray(points, F32).astype(np.float64), np.asarray(normals, F32).astype(np.float64), np.asarray(X, F32).astype(np.float64)
    lim = np.float64(MR.max_d2_of(radius))
    m = len(X)
    num, den, n = np.zeros(m), np.zeros(m), np.zeros(m, np.int64)
    if len(p) == 0:
        return num, den, n
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(idx.shape[1]):
            has = idx[:, j] >= 0
            i = np.where(has, idx[:, j], 0)
            t = 1.0 - np.where(has, d2[:, j], F32(0)).astype(np.float64) / lim
            w = (t * t) * t
            P, N = p[i], nrm[i]
            s = (N[:, 0] * (X[:, 0] - P[:, 0]) + N[:, 1] * (X[:, 1] - P[:, 1])) + N[:, 2] * (X[:, 2] - P[:, 2])
            ws = w * s
            first = n == 0
            den = np.where(has, np.where(first, w, den + w), den)
            num = np.where(has, np.where(first, ws, num + ws), num)
            n = n + has
    return num, den, n


def implicit(points, normals, shape, origin, voxel, radius, k, min_neighbors, lists=None):
    """(value float32 [nx, ny, nz], support float32 [nx, ny, nz]); lists: neighbours(...) at this k or its prefix, computed if None"""
    X = lattice_points(shape, origin, voxel)
    if lists is None:
        lists = R.knn(X, points, k, radius)
    num, den, n = sums(points, normals, X, lists, radius)
    ok = (n >= min_neighbors) & (den > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        value = np.where(ok, (num / den).astype(F32), F32(np.nan)).astype(F32)
    return value.reshape(shape), den.astype(F32).reshape(shape)


def same_bits(got, exp):
    """float32 arrays: NaN in the same places, every other entry the same bits"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.dtype != np.float32 or got.shape != exp.shape or not np.array_equal(np.isnan(got), np.isnan(exp)):
        return False
    ok = ~np.isnan(exp)
    return np.array_equal(got[ok].view(np.uint32), exp[ok].view(np.uint32))


def crossings(value, origin, voxel):
    """fp64 [C, 3]: where the value changes sign between two DEFINED lattice neighbours, by linear interpolation on the edge (a
    neighbour that is exactly zero is a crossing at that lattice point)"""
    v = np.asarray(value, np.float64)
    shape = v.shape
    X = lattice_points(shape, origin, voxel).astype(np.float64).reshape(*shape, 3)
    out = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        a, b = v[tuple(lo)], v[tuple(hi)]
        with np.errstate(invalid="ignore"):
            cross = ((a < 0) & (b >= 0)) | ((a >= 0) & (b < 0))
        t = a[cross] / (a[cross] - b[cross])
        Xa, Xb = X[tuple(lo)][cross], X[tuple(hi)][cross]
        out.append(Xa + t[:, None] * (Xb - Xa))
    return np.concatenate(out)
