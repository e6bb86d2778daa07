"""Deterministic clouds for the ls2fm.cloud tests (numpy only; at most about 2 000 points each), beside the grid scenes of
tests/metrics_scenes.py, which the k-NN and covariance tests run on as they are.  Every function is cached; callers do not write
into what they get.  tests/test_cloud_host.py asserts the properties the GPU tests lean on (eigen-gaps, threshold margins)."""
import functools

import numpy as np

import cloud_restate as R

F32 = np.float32
K_NORMALS = 16


def _frame(axis):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    u = np.cross(axis, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    return axis, u, np.cross(axis, u)


PLANE_AXIS = (0.3, -0.5, 0.8)
PLANE_SPACING = 0.025


@functools.lru_cache(maxsize=None)
def plane():
    """a 40 x 40 patch of a tilted plane: lattice points at PLANE_SPACING, moved by up to 0.3 of it inside the plane and by up to
    1 % of it along the axis -> dict(points float32 [1600, 3], axis fp64 [3])"""
    rng = np.random.default_rng(31)
    axis, u, v = _frame(PLANE_AXIS)
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    a = (i.reshape(-1) + rng.uniform(-0.3, 0.3, 1600)) * PLANE_SPACING
    b = (j.reshape(-1) + rng.uniform(-0.3, 0.3, 1600)) * PLANE_SPACING
    c = rng.uniform(-0.01, 0.01, 1600) * PLANE_SPACING
    p = np.array([0.2, 0.1, -0.3]) + a[:, None] * u + b[:, None] * v + c[:, None] * axis
    return dict(points=p.astype(F32), axis=axis)


SPHERE_CENTRE = (0.25, -0.5, 0.125)


@functools.lru_cache(maxsize=None)
def sphere():
    """2 000 points of a unit sphere about SPHERE_CENTRE, a Fibonacci spiral (so that no neighbourhood of 16 is much sparser than
    the rest) moved by up to 0.2 of the spacing along the surface -> dict(points float32 [2000, 3], centre fp64 [3])"""
    rng = np.random.default_rng(32)
    n = 2000
    t = np.arange(n) + 0.5
    z = 1.0 - 2.0 * t / n
    phi = t * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    p = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1) + rng.normal(size=(n, 3)) * 0.2 * np.sqrt(4 * np.pi / n) / np.sqrt(3)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return dict(points=(p + np.array(SPHERE_CENTRE)).astype(F32), centre=np.array(SPHERE_CENTRE))


@functools.lru_cache(maxsize=None)
def normals_expected(name):
    """dict of the restatement's two routes on the scene at K_NORMALS, the point itself among its neighbours: idx, jacobi =
    (normal, curvature, C, n), lapack = the same by eigh, gap = (lambda_1 - lambda_0) / trace per point (eigh's), angle = the
    angle between the two routes' normals per point"""
    p = {"plane": plane, "sphere": sphere}[name]()["points"]
    idx = R.knn(p, p, K_NORMALS)[0]
    jac, lap = R.normals(p, idx), R.normals(p, idx, lapack=True)
    ev = np.array([np.linalg.eigvalsh(R.full(c)) for c in jac[2]])
    return dict(idx=idx, jacobi=jac, lapack=lap, gap=(ev[:, 1] - ev[:, 0]) / ev.sum(axis=1), angle=R.angle(jac[0], lap[0]))


KS = (1, 2, 8, 9, 16, 17, 32)             # both sides of the list capacities 8 / 16 / 32


@functools.lru_cache(maxsize=None)
def expected_knn(name):
    """the restatement's (idx, d2, count) at k = 32 of the scene `name` of metrics_scenes, computed once; prefix(.., k) cuts it"""
    import metrics_scenes as MS
    sc = MS.scenes()[name]
    return R.knn(sc["q"], sc["ref"], 32, sc["max_dist"])


def prefix(full, k):
    """the rule's answer at a smaller k: the first k columns, the count capped"""
    idx, d2, count = full
    return idx[:, :k], d2[:, :k], np.minimum(count, k).astype(np.int32)


def same_knn(got, exp):
    """idx and count exactly, d2 by its bits"""
    return (got[0].dtype == np.int32 and got[0].shape == exp[0].shape and np.array_equal(got[0], exp[0])
            and np.array_equal(np.asarray(got[1], F32).view(np.uint32), np.asarray(exp[1], F32).view(np.uint32))
            and np.array_equal(got[2], exp[2]))


FLOOR = 16 * 2.0 ** -53


def check_normals(points, idx, normal, curvature, cov, queries=None, toward=None):
    """What every query of a scene is held to, the degenerate ones included.  `cov` equals the restatement's C bit for bit (NaN
    rows in the same places).  The NaN pattern of normal and curvature is the restatement's.  With bound = 4 x the worst residual
    |C v - (v^T C v) v| / |C|_F or length error ||v| - 1| that numpy.linalg.eigh leaves on the scene's matrices, floored at
    16 * 2^-53: the device's residual and length error stay below it, v^T C v is within bound |C|_F of eigh's smallest eigenvalue,
    and the curvature within 4 bound of eigh's lambda_0 / trace (lambda_0 is off by at most bound |C|_F <= bound trace, and
    the trace as the sum of three such eigenvalues by 3 bound trace, which the ratio <= 1 / 3 scales down to bound).
    -> (the restatement's Jacobi normals, bound)"""
    nj, cj, C, n = R.normals(points, idx, queries, toward)
    nl, cl, _, _ = R.normals(points, idx, queries, toward, lapack=True)
    normal, curvature, cov = np.asarray(normal, np.float64), np.asarray(curvature, np.float64), np.asarray(cov, np.float64)
    assert np.array_equal(np.isnan(cov), np.isnan(C)) and np.array_equal(np.isnan(C).any(axis=1), n == 0)
    ok = ~np.isnan(C)
    assert np.array_equal(cov[ok].view(np.uint64), C[ok].view(np.uint64)), f"{int((cov[ok] != C[ok]).sum())} covariance entries differ"
    assert np.array_equal(np.isnan(normal), np.isnan(nj)) and np.array_equal(np.isnan(curvature), np.isnan(cj))
    valid = ~np.isnan(nj[:, 0])
    if not valid.any():
        return nj, FLOOR
    res_l, unit_l, _ = R.eigen_residuals(C, nl)
    bound = max(4.0 * max(np.nanmax(res_l), np.nanmax(unit_l)), FLOOR)
    res, unit, ray = R.eigen_residuals(C, normal)
    assert res[valid].max() <= bound and unit[valid].max() <= bound, (res[valid].max(), unit[valid].max(), bound)
    lam0 = np.array([np.linalg.eigvalsh(R.full(c))[0] if v else np.nan for c, v in zip(C, valid)])
    fro = np.array([np.linalg.norm(R.full(c)) for c in C])
    assert (np.abs(ray - lam0)[valid] <= bound * fro[valid]).all(), np.nanmax(np.abs(ray - lam0) / fro)
    assert (np.abs(curvature - cl)[valid] <= 4.0 * bound).all(), np.nanmax(np.abs(curvature - cl))
    return nj, bound


STAT_K, STAT_RATIO, N_STRAGGLERS = 20, 2.0, 20


@functools.lru_cache(maxsize=None)
def stragglers():
    """a dense 30 x 30 patch (spacing 0.02, moved by up to 0.3 of it, thickness 0.2 of it) and N_STRAGGLERS points planted 0.3 to
    1.0 away from it, which come last -> float32 [920, 3]"""
    rng = np.random.default_rng(33)
    i, j = np.meshgrid(np.arange(30), np.arange(30), indexing="ij")
    patch = np.stack([(i.reshape(-1) + rng.uniform(-0.3, 0.3, 900)) * 0.02, (j.reshape(-1) + rng.uniform(-0.3, 0.3, 900)) * 0.02,
                      rng.uniform(-0.1, 0.1, 900) * 0.02], axis=1)
    far = np.stack([rng.uniform(-0.2, 0.8, N_STRAGGLERS), rng.uniform(-0.2, 0.8, N_STRAGGLERS),
                    rng.uniform(0.3, 1.0, N_STRAGGLERS) * rng.choice([-1.0, 1.0], N_STRAGGLERS)], axis=1)
    return np.concatenate([patch, far]).astype(F32)


@functools.lru_cache(maxsize=None)
def duplicates():
    """300 random points of the unit cube with every fifth one repeated at the end: 360 points, 60 exact pairs -- with skip_own a
    point's twin stays its neighbour at d2 = 0 -> float32 [360, 3]"""
    rng = np.random.default_rng(34)
    p = rng.uniform(0.0, 1.0, (300, 3)).astype(F32)
    return np.concatenate([p, p[::5]])


LONER_MAX_DIST = 0.25


@functools.lru_cache(maxsize=None)
def loner():
    """200 points in a cube of side 0.5, one point (index 7) 2 away from it, and a pair of points (the last two) 0.1 apart and 3
    away from the rest: within LONER_MAX_DIST and skip_own the first has no neighbour at all, each of the pair exactly one"""
    rng = np.random.default_rng(35)
    p = rng.uniform(0.0, 0.5, (200, 3))
    p[7] = [2.5, 0.25, 0.25]
    return np.concatenate([p, [[0.25, 3.5, 0.25], [0.25, 3.5, 0.35]]]).astype(F32)


@functools.lru_cache(maxsize=None)
def flat(kind):
    """exactly flat clouds of 400 points on dyadic coordinates (multiples of 1 / 64, so that every sum the rule takes is exact in
    its symmetry): "z" the plane z = 0.5 (normal (0, 0, 1) exactly); "diag_plus" the plane x + y = 0 (points (a, -a, b): the
    normal's x and y have the same magnitude and sign); "diag_minus" the plane x = y (opposite signs) -> float32 [400, 3]"""
    rng = np.random.default_rng(36)
    a, b = rng.integers(0, 64, 400) / 64.0, rng.integers(0, 64, 400) / 64.0
    if kind == "z":
        return np.stack([a, b, np.full(400, 0.5)], axis=1).astype(F32)
    if kind == "diag_plus":
        return np.stack([a, -a, b], axis=1).astype(F32)
    return np.stack([a, a, b], axis=1).astype(F32)


@functools.lru_cache(maxsize=None)
def cube():
    """600 points on the faces of the unit cube with the faces' outward normals (axis vectors: n . n = 1 exactly)
    -> (points float32 [600, 3], normals float32 [600, 3])"""
    rng = np.random.default_rng(37)
    p, nrm = rng.uniform(0.0, 1.0, (600, 3)), np.zeros((600, 3))
    for t in range(600):
        axis, side = t % 3, (t // 3) % 2
        p[t, axis] = float(side)
        nrm[t, axis] = 2.0 * side - 1.0
    return p.astype(F32), nrm.astype(F32)
