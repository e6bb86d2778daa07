"""Deterministic scenes for the tests of THE FUSION RULE (numpy only).  Each returns a dict; callers do not write into it.

edge_scene(H, W, S, C, nan_pose)   mvs_scenes.filter_scene's cameras and depth pattern -- the reprojection and the depth test at exact
                    equality, NaN, 0, -1 and inf depths, a -1 source column, a NaN pose -- with source rows that hold the view itself and
                    a view twice, normals drawn from NORMALS, and colours with NaNs: the shapes and edge cases of the bit-for-bit tests.
sphere_fused()      mvs_scenes.sphere_scene(hw=32, D=8) with its analytic depth filtered by the restated consistency rule
                    (min_consistent = 2), the sphere's analytic normals in each camera's frame and its texture as the colour: where
                    the rule is judged by its properties (tests/test_fuse_host.py)."""
import functools

import numpy as np

import mvs_restate as MR
import mvs_scenes as S

F32 = np.float32
NAN = np.nan
EDGE_ANGLE = 45.0           # degrees: cos2 = fl(cos(45 deg)^2) = 0.5 exactly
# against (0, 0, -1) and the cameras' identity rotations: (1, 0, -1) is the angle test at equality, a a = 1 = 0.5 (1 * 2); (1, 0, 0)
# gives a == 0, (0, 0, 1) a < 0, (2, 0, -1) an angle beyond; a zero and a NaN normal; lengths other than 1
NORMALS = [(0, 0, -1), (1, 0, -1), (0, 0, -1), (0, 0, -2), (0, 0, 0), (0, 0, -1), (NAN, 0, -1), (0, 0, 1), (1, 0, 0), (0, 0, -1),
           (0.5, 0, -0.5), (0, 0, -0.5), (2, 0, -1)]
# the kernels' tile is 32 x 8 (LS2FM_MVS_FUSE_TILE_W x _H; tests/test_fuse_host.py pins it): a whole tile and one past each of its edges
EDGE_SIZES = [(1, 1), (15, 17), (16, 16), (17, 33), (33, 31), (8, 32), (9, 33)]


@functools.lru_cache(maxsize=None)
def edge_scene(H, W, S_=5, C=3, nan_pose=False):
    """The source row of view v, from its other views o in rising order: S = 1: the next view; S = 2: (o_0, -1); S >= 3: (o_0, -1,
    v itself for an even v and o_2 for an odd one, o_last, o_0 again, ...) cut to S -- so a view has lower and higher partners, an
    entry equal to itself and a view listed twice."""
    base = S.filter_scene(H, W, 5, nan_pose)
    V = len(base["poses"])
    rows = []
    for v in range(V):
        o = [j for j in range(V) if j != v]
        rows.append(([(v + 1) % V] if S_ == 1 else [o[0], -1, v if v % 2 == 0 else o[2], o[-1], o[0]])[:S_])
    yy, xx = np.mgrid[0:H, 0:W]
    table = np.asarray(NORMALS, F32)
    normal = np.stack([table[(xx + 4 * yy + 3 * v) % len(table)] for v in range(V)])
    rng = np.random.default_rng(100 * H + W + C)
    colour = (rng.integers(0, 256, size=(V, H, W, C)) / 256.0).astype(F32)
    for v in range(V):
        for i in range(0, H, 2):
            colour[v, i, (2 * i + v) % W, (i + v) % C] = NAN
    return dict(depth=base["depth"], poses=base["poses"], intr=base["intr"], sources=np.asarray(rows), normal=normal, colour=colour,
                near=base["near"], max_reproj=base["max_reproj"], rel_depth=base["rel_depth"], max_normal_angle=EDGE_ANGLE, H=H, W=W)


def fuse_kw(sc):
    return dict(near=sc["near"], max_reproj=sc["max_reproj"], rel_depth=sc["rel_depth"], max_normal_angle=sc["max_normal_angle"])


@functools.lru_cache(maxsize=None)
def sphere_fused(hw=32):
    sc = S.sphere_scene(hw=hw, D=8)
    depth = sc["depth"].astype(F32)
    filtered, count = MR.filter_depths(depth, sc["poses"], sc["intr"], sc["sources"], near=sc["near"], max_reproj=sc["max_reproj"],
                                       rel_depth=sc["rel_depth"], min_consistent=2)
    K = sc["intr"].astype(np.float64)
    yy, xx = np.mgrid[0:hw, 0:hw].astype(np.float64)
    rays = np.stack([(xx + 0.5 - K[0, 2]) / K[0, 0], (yy + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(xx)], axis=-1)
    normal = np.full((5, hw, hw, 3), NAN, F32)
    world = np.full((5, hw, hw, 3), NAN)
    for v in range(5):
        P = sc["poses"][v].astype(np.float64)
        Rm, t = P[:, :3], P[:, 3]
        z = np.where(np.isfinite(sc["depth"][v]), sc["depth"][v], NAN).astype(np.float64)
        X = (rays * z[..., None] - t) @ Rm                             # R^T (c - t)
        world[v] = X
        radial = X / np.linalg.norm(X, axis=-1, keepdims=True)
        normal[v] = (radial @ Rm.T).astype(F32)                        # R n_w: the camera's frame
    return dict(depth=filtered, count=count, unfiltered=depth, world=world, poses=sc["poses"], intr=sc["intr"], sources=sc["sources"],
                normal=normal, colour=sc["images"][..., None].astype(F32), near=sc["near"], max_reproj=sc["max_reproj"],
                rel_depth=sc["rel_depth"], max_normal_angle=60.0, H=hw, W=hw, focal=2.0 * hw, footprint=2.0 / (2.0 * hw))
