"""Deterministic oriented clouds for the screened Poisson tests (numpy only).  Every scene is a dict(points float32 [N, 3], normals
float32 [N, 3], shape, origin, voxel, distance): the lattice and, where the surface is known, distance(x fp64 [C, 3]) -> the distance
of x from the true surface.  Everything is cached; callers do not write into what they get."""
import functools

import numpy as np

import poisson_restate as PR
from cloud_mesh_scenes import _fibonacci

F32 = np.float32
VOXEL = 1.0 / 16.0                       # dyadic: i * VOXEL and the sums with a dyadic origin are exact
NAMES = ("sphere", "capped", "hemisphere", "plane", "crowded", "on_planes", "last_cell", "nan_rows", "two", "empty")
SCREEN, CYCLES, GAMMA = 4.0, 8, 2

# the centre has two half-integer and one integer lattice coordinate, so a lattice point's squared distance from it is an integer
# plus a half (in voxels^2) and never 65.75: no lattice point lies on the sphere
SPHERE_SHAPE = (32, 32, 35)
SPHERE_CENTRE = np.array([15.5, 15.5, 17.0]) * VOXEL
SPHERE_RADIUS = np.sqrt(65.75) * VOXEL                      # 8.1 voxels
CAP = 0.8                                                   # the capped sphere lacks the directions with z > CAP: a hole of radius 4.9 voxels
PLANE_HEIGHT = 0.40625                                      # 13 / 32


def sphere_cloud(n=4000):
    d = _fibonacci(n)
    return (SPHERE_CENTRE + SPHERE_RADIUS * d).astype(F32), d.astype(F32)


def sphere_distance(x):
    return np.abs(np.linalg.norm(x - SPHERE_CENTRE, axis=1) - SPHERE_RADIUS)


def _scene(points, normals, shape, origin, distance=None, voxel=VOXEL):
    return dict(points=np.ascontiguousarray(points, F32).reshape(-1, 3), normals=np.ascontiguousarray(normals, F32).reshape(-1, 3),
                shape=tuple(shape), origin=tuple(float(o) for o in origin), voxel=voxel, distance=distance)


def small(shape, n=700, seed=3, strays=40):
    """a sphere of 0.3 of the smallest side around the middle of any lattice, off the origin, with a few stray points outside it"""
    d = _fibonacci(n)
    origin = np.array([-0.25, 0.1875, 0.5])
    centre = origin + 0.5 * (np.array(shape) - 1) * VOXEL + np.array([0.013, -0.02, 0.007])
    p = centre + 0.3 * (min(shape) - 1) * VOXEL * d
    rng = np.random.default_rng(seed)
    stray = origin + rng.uniform(-2.0, np.array(shape) + 1.0, (strays, 3)) * VOXEL
    return _scene(np.concatenate([p, stray]), np.concatenate([d, rng.normal(size=(strays, 3))]), shape, origin, lambda x: np.abs(
        np.linalg.norm(x - centre, axis=1) - 0.3 * (min(shape) - 1) * VOXEL))


@functools.lru_cache(maxsize=None)
def scene(name):
    rng = np.random.default_rng({n: 90 + i for i, n in enumerate(NAMES)}[name])
    if name == "sphere":
        # a 4 000-point Fibonacci sphere of radius 8.1 voxels inside 32 x 32 x 35
        p, n = sphere_cloud()
        return _scene(p, n, SPHERE_SHAPE, (0.0, 0.0, 0.0), sphere_distance)
    if name == "capped":
        p, n = sphere_cloud()
        keep = n[:, 2] <= CAP
        return _scene(p[keep], n[keep], SPHERE_SHAPE, (0.0, 0.0, 0.0), sphere_distance)
    if name == "hemisphere":
        p, n = sphere_cloud()
        keep = n[:, 2] >= 0
        return _scene(p[keep], n[keep], SPHERE_SHAPE, (0.0, 0.0, 0.0), sphere_distance)
    if name == "plane":
        # the plane z = 13 / 32 with normal (0, 0, 1) through the whole box: points on multiples of 1 / 64
        xy = rng.integers(0, 92, (2500, 2)) / 64.0
        p = np.concatenate([xy, np.full((2500, 1), PLANE_HEIGHT)], axis=1)
        return _scene(p, np.tile([0.0, 0.0, 1.0], (2500, 1)), (24, 24, 16), (0.0, 0.0, 0.0), lambda x: np.abs(x[:, 2] - PLANE_HEIGHT))
    if name == "crowded":
        # a 600-point sphere of radius 5 voxels with every third point repeated, and 500 points inside one voxel
        d = _fibonacci(600)
        p = (np.array([0.2, -0.31, 0.43]) + 5.0 * VOXEL * d).astype(F32)
        heap = np.array([0.2, -0.31, 0.43]) + np.array([5.0, 0.1, 0.2]) * VOXEL + rng.uniform(0, 0.4, (500, 3)) * VOXEL
        return _scene(np.concatenate([p, p[::3], heap]), np.concatenate([d, d[::3], np.tile([1.0, 0.0, 0.0], (500, 1))]), (15, 17, 13),
                      (-0.25, -0.8125, 0.0625))
    if name == "on_planes":
        # points exactly on lattice planes: f = 0 on one, two or all three axes
        shape = (9, 8, 10)
        c = rng.uniform(0.5, np.array(shape) - 1.5, (300, 3))
        for t in range(300):
            for a in range(3):
                if (t >> a) & 1 or t % 8 == 0:
                    c[t, a] = np.floor(c[t, a])
        return _scene(-0.5 + c * 0.125, rng.normal(size=(300, 3)), shape, (-0.5, -0.5, -0.5), voxel=0.125)
    if name == "last_cell":
        # u = n - 1 (outside), one ulp below (inside), 0 and -0 (inside), just below 0 and far away (outside), per axis
        shape = (6, 5, 7)
        rows = []
        for a in range(3):
            top = F32((shape[a] - 1) * 0.25)
            for v in (top, np.nextafter(top, F32(0)), F32(0.0), F32(-0.0), np.nextafter(F32(0), F32(-1)), F32(-0.25), F32(9.0), F32(1e30)):
                row = [0.3, 0.55, 0.8]
                row[a] = v
                rows.append(row)
        rows += [[0.3, 0.55, 0.8], [1.2, 0.99, 1.49]]
        return _scene(rows, rng.normal(size=(len(rows), 3)), shape, (0.0, 0.0, 0.0), voxel=0.25)
    if name == "nan_rows":
        sc = small((10, 9, 11), 300)
        p, n = sc["points"].copy(), sc["normals"].copy()
        p[3, 0], p[40, 2], n[7, 1], n[100, 0], n[200, 2], p[250, 1] = np.nan, np.inf, np.nan, -np.inf, np.nan, -np.inf
        return _scene(p, n, sc["shape"], sc["origin"])
    if name == "two":
        return _scene([[0.21, 0.2, 0.26], [0.3, 0.24, 0.2]], [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], (8, 7, 9), (0.0, 0.0, 0.0))
    if name == "empty":
        return _scene(np.zeros((0, 3)), np.zeros((0, 3)), (4, 5, 6), (0.0, 0.0, 0.0))
    raise KeyError(name)


def lattice_of(sc):
    return sc["shape"], sc["origin"], sc["voxel"]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def system(name):
    """(V [3, ...], W, b) of the scene by the restatement"""
    sc = scene(name)
    V, W = PR.finish(PR.splat(sc["points"], sc["normals"], *lattice_of(sc)), sc["shape"])
    return _frozen(np.ascontiguousarray(V), np.ascontiguousarray(W), PR.rhs(V))


@functools.lru_cache(maxsize=None)
def expected(name, screen=SCREEN, cycles=CYCLES, gamma=GAMMA):
    """the restatement's (value, density) of the scene; computed once per set of options and not written into"""
    _, W, b = system(name)
    return _frozen(PR.solve_lattice(b, W, screen, cycles, gamma), W)


@functools.lru_cache(maxsize=None)
def expected_small(shape, screen, cycles, gamma):
    sc = small(shape)
    return _frozen(*PR.solve(sc["points"], sc["normals"], *lattice_of(sc), screen, cycles, gamma))
