"""Deterministic oriented clouds for the ls2fm.cloud_mesh tests (numpy only): a few thousand points with analytic normals on
lattices of at most 32^3, so that the brute-force restatement (tests/cloud_mesh_restate.py) stays within seconds.  Every scene is a
dict(points float32 [N, 3], normals float32 [N, 3], shape, origin, voxel, radius, distance): the lattice, the support radius (3
voxels) and, where the surface is known, distance(x fp64 [C, 3]) -> the distance of x from the true surface.  Everything is
cached; callers do not write into what they get.  tests/test_cloud_mesh_host.py asserts the properties the GPU tests lean on."""
import functools

import numpy as np

import cloud_mesh_restate as CR
import cloud_scenes as CS

F32 = np.float32
VOXEL = 1.0 / 16.0                       # dyadic: i * VOXEL and the sums with a dyadic origin are exact
K = 16
MIN_NEIGHBORS = 3
NAMES = ("sphere", "cube", "plane", "sheets", "hemisphere", "duplicates", "few", "empty")
SURFACES = ("sphere", "cube", "plane", "sheets", "hemisphere")          # the scenes with a known surface


def _fibonacci(n):
    t = np.arange(n) + 0.5
    z = 1.0 - 2.0 * t / n
    phi = t * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def _scene(points, normals, shape, origin, distance=None, voxel=VOXEL):
    return dict(points=np.asarray(points, F32).reshape(-1, 3), normals=np.asarray(normals, F32).reshape(-1, 3), shape=tuple(shape),
                origin=tuple(float(o) for o in origin), voxel=voxel, radius=3.0 * voxel, distance=distance)


# The centre is the middle of a lattice cell, so a lattice point's squared distance from it is (8 m + 3) / 4 voxels^2, and the
# squared radius 65.75 lies midway between two such values: no lattice point is nearer than SPHERE_MARGIN voxels to the surface.
# The rule's error on this cloud stays below that at every k (tests/test_cloud_mesh_host.py), so the sign at every lattice point,
# and with it the number of crossings, is the true sphere's whatever k is.
SPHERE_CENTRE = np.array([16.5, 16.5, 16.5]) * VOXEL
SPHERE_RADIUS = np.sqrt(65.75) * VOXEL
SPHERE_MARGIN = 0.06


def sphere_cloud(n):
    d = _fibonacci(n)
    return (SPHERE_CENTRE + SPHERE_RADIUS * d).astype(F32), d.astype(F32)


def _sphere_distance(x):
    return np.abs(np.linalg.norm(x - SPHERE_CENTRE, axis=1) - SPHERE_RADIUS)


CUBE_LO, CUBE_HI = 8.0 * VOXEL, 24.0 * VOXEL                 # the faces lie on lattice planes
PLANE_HEIGHT = 0.40625                  # 13 / 32
SHEET_MID = 0.5


@functools.lru_cache(maxsize=None)
def scene(name):
    rng = np.random.default_rng({n: 50 + i for i, n in enumerate(NAMES)}[name])
    if name == "sphere":
        # a 4 000-point Fibonacci sphere of radius 8.1 voxels inside 32^3
        p, n = sphere_cloud(4000)
        return _scene(p, n, (32, 32, 32), (0.0, 0.0, 0.0), _sphere_distance)
    if name == "cube":
        # 6 000 random points on the faces of a cube of side 16 voxels with the faces' outward normals
        p, n = rng.uniform(CUBE_LO, CUBE_HI, (6000, 3)), np.zeros((6000, 3))
        for t in range(6000):
            axis, side = t % 3, (t // 3) % 2
            p[t, axis] = CUBE_HI if side else CUBE_LO
            n[t, axis] = 2.0 * side - 1.0
        mid, half = 0.5 * (CUBE_LO + CUBE_HI), 0.5 * (CUBE_HI - CUBE_LO)

        def distance(x):
            q = np.abs(x - mid) - half
            outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
            return np.abs(outside + np.minimum(q.max(axis=1), 0.0))
        return _scene(p, n, (32, 32, 32), (0.0, 0.0, 0.0), distance)
    if name == "plane":
        # the plane z = 13 / 32 with normal (0, 0, 1): 2 500 points on multiples of 1 / 64 over the lattice's footprint and a
        # margin of the radius, a dyadic lattice -- every X.z - c is exact
        xy = rng.integers(-32, 129, (2500, 2)) / 64.0
        p = np.concatenate([xy, np.full((2500, 1), PLANE_HEIGHT)], axis=1)
        n = np.tile([0.0, 0.0, 1.0], (2500, 1))
        return _scene(p, n, (24, 24, 16), (0.0, 0.0, 0.0), lambda x: np.abs(x[:, 2] - PLANE_HEIGHT))
    if name == "sheets":
        # two sheets two voxels apart with opposite (outward) normals, points every half voxel: each keeps its own surface
        g = (np.arange(-8, 41) * 0.5 + 0.25) * VOXEL
        a, b = (t.reshape(-1) for t in np.meshgrid(g, g, indexing="ij"))
        up = np.stack([a, b, np.full_like(a, SHEET_MID + VOXEL)], axis=1)
        down = np.stack([a, b, np.full_like(a, SHEET_MID - VOXEL)], axis=1)
        n = np.concatenate([np.tile([0.0, 0.0, 1.0], (len(a), 1)), np.tile([0.0, 0.0, -1.0], (len(a), 1))])
        return _scene(np.concatenate([up, down]), n, (16, 16, 16), (0.0, 0.0, 0.0),
                      lambda x: np.minimum(np.abs(x[:, 2] - (SHEET_MID + VOXEL)), np.abs(x[:, 2] - (SHEET_MID - VOXEL))))
    if name == "hemisphere":
        # the upper half of the sphere scene, open at its rim.  The rule continues the surface below the rim along the rim's
        # tangent planes as far as the radius reaches and no farther; that continuation is held to the full sphere.
        p, n = sphere_cloud(4000)
        top = p[:, 2].astype(np.float64) >= SPHERE_CENTRE[2]
        return _scene(p[top], n[top], (32, 32, 32), (0.0, 0.0, 0.0), _sphere_distance)
    if name == "duplicates":
        # a 600-point sphere of radius 5 voxels with every third point repeated at the end, on an odd lattice off the origin
        d = _fibonacci(600)
        p = (np.array([0.2, -0.31, 0.43]) + 5.0 * VOXEL * d).astype(F32)
        return _scene(np.concatenate([p, p[::3]]), np.concatenate([d, d[::3]]), (15, 17, 13), (-0.25, -0.8125, 0.0625))
    if name == "few":
        # two points: fewer than MIN_NEIGHBORS anywhere, so every value is NaN while the support is not zero
        return _scene([[0.21, 0.2, 0.26], [0.3, 0.24, 0.2]], [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], (8, 7, 9), (0.0, 0.0, 0.0))
    if name == "empty":
        return _scene(np.zeros((0, 3)), np.zeros((0, 3)), (4, 5, 6), (0.0, 0.0, 0.0))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def lists(name):
    """cloud_restate.knn of every lattice point of the scene at k = 32 and its radius, computed once; cloud_scenes.prefix cuts it"""
    sc = scene(name)
    return CR.neighbours(sc["points"], sc["shape"], sc["origin"], sc["voxel"], sc["radius"], 32)


@functools.lru_cache(maxsize=None)
def expected(name, k=K, min_neighbors=MIN_NEIGHBORS):
    """the restatement's (value, support) of the scene; computed once per (scene, k, min_neighbors) and not written into"""
    sc = scene(name)
    out = CR.implicit(sc["points"], sc["normals"], sc["shape"], sc["origin"], sc["voxel"], sc["radius"], k, min_neighbors,
                      lists=CS.prefix(lists(name), k))
    for a in out:
        a.setflags(write=False)
    return out
