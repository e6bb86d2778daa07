"""Deterministic scenes for the PatchMatch tests (numpy only).  Each returns a dict or arrays; callers do not write into them.

edge_state(sc)      a hand-made initial state (depth, normal) for a mvs_scenes.grid_scene: the true plane with fronto-parallel
                    normals, and in a pattern every edge THE PLANE SCORE and THE PATCHMATCH STEP name.
slanted_scene()     a plane tilted 30 degrees about y with mvs_scenes.sphere_texture, under five cameras arranged like
                    sphere_scene's, 48 x 48, with the true depth and camera-frame normal of every pixel in closed form."""
import functools

import numpy as np

import mvs_scenes as S
from raster_scenes import intrinsics, look_at

F32 = np.float32
TILE_H, TILE_W = 16, 32     # LS2FM_MVS_PM_TILE_H, LS2FM_MVS_PM_TILE_W of include/ls2fm.h (tests/test_patchmatch_host.py pins the copies)
EDGE_DEPTHS = [1.0, 1.0, 1.0, np.nan, 1.0, 0.0, 1.0, -1.0, 1.0, np.inf, 1.0, 1.0, 1.0]
N_NORMALS = 11


def edge_state(sc):
    """depth float32 [R, H, W] and normal float32 [R, H, W, 3] for a grid_scene.  The base is the plane z = 1 seen fronto-parallel
    (depth 1 for the cameras at z = 0, 1 / 4 for camera 5; normal (0, 0, -1)): neighbours then carry the very plane of the
    incumbent, so their candidates tie its score exactly.  Depths by the pattern EDGE_DEPTHS: NaN, 0, negative and +inf.  Normals
    by a pattern of N_NORMALS, all numbers dyadic: (1, 0, -xn_p) has g_p == 0 exactly, (0, 0, 1) faces away, one holds a NaN, and
    (1, 0, -(xn_p + 1 / 32)) has g_p = -1 / 32 at the pixel but g_q = +1 / 32 one column to the right: the sign changes inside
    every window."""
    refs, H, W = sc["refs"], sc["H"], sc["W"]
    K = sc["intr"]
    yy, xx = np.mgrid[0:H, 0:W]
    xn = ((xx.astype(F32) + F32(0.5)) - K[0, 2]) / K[0, 0]
    depth = np.empty((len(refs), H, W), F32)
    normal = np.zeros((len(refs), H, W, 3), F32)
    for r, rv in enumerate(refs):
        pick = np.asarray(EDGE_DEPTHS, F32)[(3 * xx + 5 * yy + 2 * r) % len(EDGE_DEPTHS)]
        depth[r] = pick * F32(0.25 if rv == 5 else 1.0)
        kind = (xx + 3 * yy + r) % N_NORMALS
        normal[r, ..., 2] = -1
        zero, away, bad, sign = kind == 3, kind == 5, kind == 7, kind == 9
        normal[r][zero] = np.stack([np.ones(zero.sum(), F32), np.zeros(zero.sum(), F32), -xn[zero]], axis=1)
        normal[r][away] = (0, 0, 1)
        normal[r][bad] = (0, np.nan, -1)
        normal[r][sign] = np.stack([np.ones(sign.sum(), F32), np.zeros(sign.sum(), F32), -(xn[sign] + F32(1 / 32))], axis=1)
    return depth, normal


SLANT_D, SLANT_DEG = 2.5, 30.0


@functools.lru_cache(maxsize=None)
def slanted_scene(hw=48, D=48):
    """The plane through the origin with the world normal (sin 30, 0, -cos 30): tilted 30 degrees about y against the central
    camera's image plane.  5 cameras at distance 2.5 from the origin, one on the -z axis and four turned 12 degrees about the x and
    y axes (sphere_scene's), f = 2 hw.  The image of a pixel is sphere_texture at the point its centre's ray hits; `depth` is that
    point's camera z and `normal` the plane's normal in the camera's frame, both float64 in closed form.  D planes uniform in depth
    over [2.0, 3.0]; every view takes the other four as sources."""
    a, tilt = np.deg2rad(12.0), np.deg2rad(SLANT_DEG)
    dirs = [(0, 0, -1), (np.sin(a), 0, -np.cos(a)), (-np.sin(a), 0, -np.cos(a)), (0, np.sin(a), -np.cos(a)), (0, -np.sin(a), -np.cos(a))]
    eyes = np.array(dirs, np.float64) * SLANT_D
    poses = np.stack([look_at(e, (0, 0, 0)) for e in eyes])
    K = intrinsics(2.0 * hw, hw / 2.0, hw / 2.0)
    K64 = K.astype(np.float64)
    nw = np.array([np.sin(tilt), 0.0, -np.cos(tilt)])
    yy, xx = np.mgrid[0:hw, 0:hw].astype(np.float64)
    rays = np.stack([(xx + 0.5 - K64[0, 2]) / K64[0, 0], (yy + 0.5 - K64[1, 2]) / K64[1, 1], np.ones_like(xx)], axis=-1)
    images, depth, normal = np.empty((5, hw, hw), F32), np.empty((5, hw, hw)), np.empty((5, hw, hw, 3))
    for i in range(5):
        Rm = poses[i].astype(np.float64)[:, :3]
        nc = Rm @ nw                                                   # the plane n_c . X_c = n_w . eye ... in camera i's frame
        depth[i] = -(nw @ eyes[i]) / (rays @ nc)                       # the ray z (xn, yn, 1) meets n_w . (R^T c + eye) = 0
        X = (rays * depth[i][..., None]) @ Rm + eyes[i]
        images[i] = S.sphere_texture(X)
        normal[i] = nc
    assert (depth > 0).all() and ((rays @ (poses[0].astype(np.float64)[:, :3] @ nw)) < 0).all()
    sources = np.array([[j for j in range(5) if j != i] for i in range(5)])
    depths = np.linspace(2.0, 3.0, D).astype(F32)
    return dict(images=images, poses=poses, intr=K, sources=sources, depths=np.broadcast_to(depths, (5, D)).copy(), depth=depth,
                normal=normal, half_width=2, near=1e-3, min_var=1e-4, min_sources=2, H=hw, W=hw)
