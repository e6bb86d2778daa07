"""Deterministic point-cloud scenes for the metrics tests (numpy only; N, M <= 4096), each built to break one way a grid query goes
wrong.  scenes() -> name -> dict(ref float32 [N, 3], q float32 [M, 3], cell_size (float, or None for the automatic one),
max_dist (float or None)).  expected(name) is the restatement's answer, computed once and shared; callers do not write into it.
tests/test_metrics_host.py asserts, per scene, the condition under which a wrong kernel fails it."""
import functools

import numpy as np

import metrics_restate as R

F32 = np.float32


def cells_of(p, ref, cell_size):
    """int64 [n, 3]: the grid's cell of every point, floor((p - origin) * (1 / h)) in fp32, origin the references' minimum; not
    clamped (a query outside the box shows as a cell outside the grid)"""
    o = np.asarray(ref, F32).min(axis=0)
    inv = F32(1) / F32(cell_size)
    return np.floor(((np.asarray(p, F32) - o).astype(F32) * inv).astype(F32)).astype(np.int64)


def _faces():
    """h = 0.25.  Per query cell and axis: a decoy 0.7 h - eps away inside the query's own cell and the true neighbour eps = h / 64
    away across the cell's upper face, ON the face (an exact multiple of h) or one fp32 ulp above it -- in the next cell, ring 1 --
    or one ulp below it, still in the query's cell.  The three axes' groups are stacked along z, 8 h apart."""
    h = 0.25
    ref, q = [np.zeros(3)], []
    for axis in range(3):
        for i in range(5):
            for j in range(5):
                for l in range(5):
                    base = np.array([i, j, l], np.float64) * h + np.array([0.0, 0.0, 8 * h * axis])
                    centre = base + h / 2
                    face = F32(base[axis] + h)
                    variant = (i + 2 * j + 3 * l) % 3
                    true = centre.copy()
                    true[axis] = [face, np.nextafter(face, F32(np.inf)), np.nextafter(face, F32(-np.inf))][variant]
                    decoy, query = centre.copy(), centre.copy()
                    decoy[axis] = base[axis] + 0.3 * h
                    query[axis] = base[axis] + h - h / 64
                    ref += [decoy, true]
                    q.append(query)
    return dict(ref=np.array(ref, F32), q=np.array(q, F32), cell_size=h, max_dist=None)


def _ties():
    """h = 0.5, references on the lattice corners (0 .. 6)^3 h, queries at the centres of the lattice cubes: 8 corners at exactly
    d2 = 3 (h / 2)^2 in 8 cells.  The lattice is stored in REVERSE cell order, so of the 8 tied corners the lowest index is the one
    in the highest cell, a ring after the query's own cell, whose corner holds the highest index.  20 exact duplicates of lattice
    points stand in front of the lattice (the duplicate holds the lower index) and 30 behind it (the original does)."""
    h = 0.5
    g = np.arange(7)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1] * h          # x fastest = cell order
    rev = lattice[::-1]
    ref = np.concatenate([lattice[100:120], rev, lattice[200:230]])
    c = np.arange(6) + 0.5
    q = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3) * h
    return dict(ref=ref.astype(F32), q=q.astype(F32), cell_size=h, max_dist=None)


def _outside():
    rng = np.random.default_rng(11)
    ref = rng.uniform(0.0, 1.0, (500, 3))
    q = [rng.uniform(0.0, 1.0, 3) for _ in range(40)]
    for axis in range(3):
        for off in (-50.0, -5.0, -0.001, 1.001, 6.0, 51.0):
            p = rng.uniform(0.0, 1.0, 3)
            p[axis] = off
            q.append(p)
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                q.append(0.5 + 20.0 * np.array([sx, sy, sz]))
                q.append(0.5 + np.array([sx * 0.51, sy * 3.0, sz * 40.0]))
    return dict(ref=ref.astype(F32), q=np.array(q, F32), cell_size=0.125, max_dist=None)


def _clusters():
    """two clusters of radius 0.01 a unit apart, queries within 0.02 of the point midway: ~10 empty rings at h = 0.05"""
    rng = np.random.default_rng(12)
    a, b = np.zeros(3), np.array([1.0, 0.5, 0.3])
    ref = np.concatenate([a + rng.uniform(-0.01, 0.01, (200, 3)), b + rng.uniform(-0.01, 0.01, (200, 3))])
    q = 0.5 * (a + b) + rng.uniform(-0.02, 0.02, (64, 3))
    return dict(ref=ref.astype(F32), q=q.astype(F32), cell_size=0.05, max_dist=None)


def _degenerate():
    rng = np.random.default_rng(13)
    q = rng.uniform(-0.5, 1.5, (50, 3)).astype(F32)
    plane = rng.uniform(0.0, 1.0, (300, 3))
    plane[:, 2] = 0.25
    line = np.zeros((300, 3)) + np.array([0.0, 0.5, -0.25])
    line[:, 0] = rng.uniform(0.0, 1.0, 300)
    out = {
        "n1": dict(ref=np.array([[0.3, -0.2, 0.9]], F32), q=q),
        "n257": dict(ref=rng.uniform(0.0, 1.0, (257, 3)).astype(F32), q=q),
        "identical": dict(ref=np.tile(np.array([[0.7, 0.1, 0.4]], F32), (100, 1)), q=q),
        "coplanar": dict(ref=plane.astype(F32), q=q),
        "collinear": dict(ref=line.astype(F32), q=q),
        "m1": dict(ref=rng.uniform(0.0, 1.0, (300, 3)).astype(F32), q=q[:1]),
    }
    return {f"degenerate_{k}": dict(v, cell_size=None, max_dist=None) for k, v in out.items()}


CUTOFF = 0.125          # float32(0.125)^2 = 0.015625 exactly


def _cutoff():
    """400 random references in the unit cube (nearest-neighbour distances on both sides of 0.125), and away from them: query 0
    with its only reference exactly 0.125 away along x (d2 == max_d2: it qualifies), query 1 with its only reference one ulp
    further (it does not)."""
    rng = np.random.default_rng(14)
    ref = rng.uniform(0.0, 1.0, (400, 3)).astype(F32)
    q = rng.uniform(0.0, 1.0, (200, 3)).astype(F32)
    q0, q1 = np.array([0.5, 0.5, 1.5], F32), np.array([0.5, 0.5, 2.0], F32)
    r0 = np.array([0.625, 0.5, 1.5], F32)
    r1 = np.array([np.nextafter(F32(0.625), F32(1)), 0.5, 2.0], F32)
    return dict(ref=np.concatenate([ref, [r0, r1]]).astype(F32), q=np.concatenate([[q0, q1], q]).astype(F32), cell_size=0.125,
                max_dist=CUTOFF)


def _nonfinite():
    rng = np.random.default_rng(15)
    ref = rng.uniform(0.0, 1.0, (300, 3)).astype(F32)
    q = rng.uniform(-0.2, 1.2, (96, 3)).astype(F32)
    bad = [(np.nan, 0.5, 0.5), (0.5, np.nan, 0.5), (0.5, 0.5, np.nan), (np.nan, np.nan, np.nan), (np.inf, 0.5, 0.5), (0.5, -np.inf, 0.5),
           (0.5, 0.5, np.inf), (-np.inf, -np.inf, -np.inf), (np.inf, np.nan, -np.inf), (np.inf, np.inf, np.inf)]
    rows = np.arange(len(bad)) * 9 + 1                     # spread through the finite ones, lane 1 of the first wave included
    q[rows] = np.array(bad, F32)
    return dict(ref=ref, q=q, cell_size=0.1, max_dist=None, bad_rows=rows)


def _sphere(rng, n, radius):
    v = rng.normal(size=(n, 3))
    return (radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


SURFACE_MAX_DIST, SURFACE_THRESHOLDS = 0.05, (0.022, 0.03)


def _surface():
    """the Chamfer scene: 4096 points on the unit sphere against 4096 on a sphere of radius 1.02.  With ~0.03 between neighbours
    of one cloud, distances fall on both sides of the thresholds and a few points have no neighbour inside max_dist = 0.05."""
    rng = np.random.default_rng(16)
    return dict(ref=_sphere(rng, 4096, 1.02), q=_sphere(rng, 4096, 1.0), cell_size=None, max_dist=None)


@functools.lru_cache(maxsize=None)
def scenes():
    out = dict(faces=_faces(), ties=_ties(), outside=_outside(), clusters=_clusters())
    out.update(_degenerate())
    out.update(cutoff=_cutoff(), nonfinite=_nonfinite(), surface=_surface())
    return out


NAMES = ("faces", "ties", "outside", "clusters", "degenerate_n1", "degenerate_n257", "degenerate_identical", "degenerate_coplanar",
         "degenerate_collinear", "degenerate_m1", "cutoff", "nonfinite", "surface")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(idx int32 [M], d2 float32 [M]) of the scene by tests/metrics_restate.py"""
    sc = scenes()[name]
    return R.nearest(sc["q"], sc["ref"], sc["max_dist"])


# ------------------------------------------------------------------------------------------------------------- camera scenes
def _rotation(rng, max_angle=np.pi):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.2, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _cameras(rng, n, noise_rot=0.0, noise_c=0.0):
    """n world-to-camera poses [n, 3, 4] scattered in a unit box, and a copy with every rotation turned by ~noise_rot rad and every
    centre moved by ~noise_c"""
    P, Q = np.zeros((n, 3, 4)), np.zeros((n, 3, 4))
    for v in range(n):
        Rv, C = _rotation(rng), rng.uniform(-1.0, 1.0, 3)
        P[v, :, :3], P[v, :, 3] = Rv, -Rv @ C
        Q[v, :, :3] = (_small(rng, noise_rot) if noise_rot else np.eye(3)) @ Rv
        Q[v, :, 3] = -Q[v, :, :3] @ (C + noise_c * rng.normal(size=3))
    return P, Q


def _small(rng, angle):
    w = rng.normal(size=3)
    w *= angle / np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(angle) / angle * K + (1 - np.cos(angle)) / angle ** 2 * K @ K


def transformed(P, s, A, a):
    """the poses of the same cameras after the world is mapped by X' = s A X + a: R' = R A^T, C' = s A C + a"""
    out = np.zeros_like(P)
    for v in range(len(P)):
        Rv = P[v, :, :3]
        C = -Rv.T @ P[v, :, 3]
        out[v, :, :3] = Rv @ A.T
        out[v, :, 3] = -out[v, :, :3] @ (s * A @ C + a)
    return out


@functools.lru_cache(maxsize=None)
def camera_cases():
    """name -> dict(est, gt [V, 3, 4], with_scale, and for the point alignment src, dst [V, 3]).  rigid / similarity: the
    ground truth is a rigid / similarity transform of noisy copies of the estimate's cameras, 8 to 50 of them; mirrored: dst is a
    REFLECTED, noisy copy of src, so the unconstrained optimum is a reflection and Umeyama's determinant case decides; fixed_scale:
    a similarity compared with with_scale=False."""
    rng = np.random.default_rng(21)
    out = {}
    for name, n, s, with_scale in (("rigid8", 8, 1.0, True), ("rigid50", 50, 1.0, True), ("similarity8", 8, 2.5, True),
                                   ("similarity23", 23, 0.37, True), ("similarity50", 50, 7.0, True), ("fixed_scale", 12, 1.7, False)):
        gt0, est = _cameras(rng, n, noise_rot=0.01, noise_c=0.01)
        gt = transformed(gt0, s, _rotation(rng), rng.uniform(-3.0, 3.0, 3))
        out[name] = dict(est=est, gt=gt, with_scale=with_scale)
    gt0, est = _cameras(rng, 20, noise_rot=0.01, noise_c=0.01)
    out["mirrored"] = dict(est=est, gt=gt0, with_scale=True)
    for name, c in out.items():
        c["src"], c["dst"] = R.centres(c["est"]), R.centres(c["gt"])
    mirror = np.diag([1.0, 1.0, -1.0])
    out["mirrored"]["dst"] = (out["mirrored"]["dst"] * np.array([1.0, 1.0, 0.05])) @ mirror + 0.3       # flat and reflected
    return out
