"""Deterministic scenes for the TSDF fusion tests (numpy only).

constant_scene()   one axis camera over a constant depth map, every number dyadic: the fused values are known in closed form.
sphere_scene(n, hw) a sphere of radius 0.5 under six axis cameras at distance 2.5 with analytic depth maps (+inf off the sphere),
                   a volume over [-0.8, 0.8]^3, trunc = 3 voxels: where THE FUSION RULE is judged by its properties
                   (tests/test_fusion_host.py).
edge_scene(shape, H, W, V)  the edge cases of the rule for the bit-for-bit GPU tests (see there).
Each returns a dict; callers do not write into it."""
import functools

import numpy as np

from raster_scenes import IDENTITY, intrinsics, look_at

F32 = np.float32
BRICK = (2, 2, 64)          # LS2FM_TSDF_BRICK_X / _Y / _Z of include/ls2fm.h (tests/test_fusion_host.py pins the copy)


@functools.lru_cache(maxsize=None)
def constant_scene():
    """The identity pose with fx = fy = 8, cx = cy = 4 over an 8 x 8 image of constant depth D = 2; the volume has 9 x 9 x 17
    points at voxel = 1 / 4 from origin (-1, -1, 1 / 4), trunc = 1 / 2: c_z = 1 / 4 + k / 4 for k = 0 .. 16, every product and
    quotient exact in fp32."""
    return dict(shape=(9, 9, 17), origin=(-1.0, -1.0, 0.25), voxel=0.25, trunc=0.5, D=2.0, near=0.125,
                depth=np.full((1, 8, 8), 2.0, F32), poses=IDENTITY[None].copy(), intr=intrinsics(8.0, 4.0, 4.0), H=8, W=8)


SPHERE_R, SPHERE_D, SPHERE_HALF = 0.5, 2.5, 0.8


def sphere_depth(eye, pose, K, H, W, radius=SPHERE_R):
    """the analytic camera-z depth map of a sphere at the origin, float32 [H, W], +inf off the sphere; pixel centres at + 0.5"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.stack([(xx + 0.5 - K[0, 2]) / K[0, 0], (yy + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(xx)], axis=-1)     # camera z = 1
    Rm = np.asarray(pose, np.float64)[:, :3]
    dw = dirs @ Rm                                                    # world direction R^T d, still camera z = 1 per unit
    eye = np.asarray(eye, np.float64)
    a = (dw * dw).sum(-1)
    b = 2.0 * (dw @ eye)
    c = eye @ eye - radius * radius
    disc = b * b - 4.0 * a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2.0 * a)
    return np.where(disc > 0, t, np.inf).astype(F32)


@functools.lru_cache(maxsize=None)
def sphere_scene(n=32, hw=128):
    """dict(shape, origin, voxel, trunc, poses [6, 3, 4], eyes, intr, H, W, depth float32 [6, H, W], near).  The focal length puts
    the volume's near face at 0.4 of the image's side about its middle, f = 0.4 hw (D - 0.8) / 0.8, so every lattice point is in
    every image; the sphere's silhouette is narrower still."""
    eyes = np.array([[SPHERE_D, 0, 0], [-SPHERE_D, 0, 0], [0, SPHERE_D, 0], [0, -SPHERE_D, 0], [0, 0, SPHERE_D], [0, 0, -SPHERE_D]], np.float64)
    poses = np.stack([look_at(e, (0, 0, 0), up=(0.0, 0.0, 1.0) if e[1] != 0 else (0.0, 1.0, 0.0)) for e in eyes])
    f = 0.4 * hw * (SPHERE_D - SPHERE_HALF) / SPHERE_HALF
    K = intrinsics(f, hw / 2, hw / 2)
    voxel = 2 * SPHERE_HALF / (n - 1)
    depth = np.stack([sphere_depth(eyes[i], poses[i], K.astype(np.float64), hw, hw) for i in range(6)])
    return dict(shape=(n, n, n), origin=(-SPHERE_HALF,) * 3, voxel=voxel, trunc=3 * voxel, poses=poses, eyes=eyes, intr=K, H=hw, W=hw,
                depth=depth, near=1e-3)


# ------------------------------------------------------------------------------------------------------------------ edge cases
EDGE_NEAR, EDGE_TRUNC, EDGE_VOXEL, EDGE_MAX_DEPTH, EDGE_MAX_WEIGHT = 0.5, 0.5, 0.25, 4.0, 1.5
EDGE_WEIGHTS = (1.0, 0.5, 1.0)          # against max_weight 3 / 2: views 0 and 1, or 1 and 2, reach it exactly; views 0 and 2 pass it
EDGE_KINDS = ["s_below_minus_trunc", "nan", "+inf", "-inf", "zero", "negative", "max_depth", "above_max_depth", "s_eq_minus_trunc",
              "s_eq_trunc", "s_beyond_trunc"]


def _up(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def _down(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


def _edge_depth(kind, cz):
    return {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "zero": 0.0, "negative": -1.0, "max_depth": EDGE_MAX_DEPTH,
            "above_max_depth": _up(EDGE_MAX_DEPTH), "s_eq_minus_trunc": cz - EDGE_TRUNC, 
            "s_below_minus_trunc": np.float64(cz) - EDGE_TRUNC - 2.0 ** -24 if cz < 1.5 else _down(cz - EDGE_TRUNC),
            "s_eq_trunc": cz + EDGE_TRUNC, "s_beyond_trunc": cz + 2 * EDGE_TRUNC}[kind]


@functools.lru_cache(maxsize=None)
def edge_scene(shape, H, W, V=3, nan_pose=False):
    """View 0 is the identity pose with fx = 2 W, fy = 2 H, cx = cy = 0: lattice point (ix, iy, iz) at voxel 1 / 4 from origin
    (0, 0, 1 / 4) has c_z = (iz + 1) / 4, u = W ix / (2 c_z) and v = H iy / (2 c_z).  So u is exactly 0 at ix = 0, and exactly the
    width (out) at ix = 1 on the plane iz = 1, whose c_z = 1 / 2 == near (usable; iz = 0 lies below near), and at ix = 2 on the
    plane c_z = 1; v likewise.  View 0's depth map is a dyadic pattern into which the kinds of EDGE_KINDS are written: the
    lattice points off the axis ix = iy = 0, in index order, each claim the pixel they land on, if it is still free, and put
    there the next kind's depth, formed exactly from their own c_z (s == -trunc is d = c_z - 1 / 2; s one ulp below -trunc is
    d = c_z - 1 / 2 - 2^-24, a float for c_z < 3 / 2, as the first claim's is, and the float below c_z - 1 / 2 further out;
    s == trunc and beyond give val exactly 1).  `claims` lists (kind, lattice index, pixel).
    View 1 sits inside the volume looking along +z, with lattice points behind it; view 2 looks from outside at an angle.
    Their depth maps are dyadic steps, some pixels +inf.  nan_pose puts a NaN into the third row of view 1's pose (every c_z is NaN).  The view weights 1, 1 / 2,
    1 against max_weight = 3 / 2: views 0 and 1 reach it exactly, views 0 and 2 pass it.
    -> dict(shape, origin, voxel, trunc, near, max_depth, max_weight, poses [V, 3, 4], intr [V, 3, 3], depth [V, H, W],
    view_weight [V], claims)"""
    import fusion_restate as FR
    import raster_restate as R
    origin = (0.0, 0.0, 0.25)
    ext = [max(n - 1, 1) * EDGE_VOXEL for n in shape]
    mid = (ext[0] / 2, ext[1] / 2, 0.25 + min(ext[2], 2.0) / 2)
    poses = np.stack([IDENTITY,
                      look_at((mid[0], mid[1], mid[2]), (mid[0] + 0.25, mid[1] + 0.125, mid[2] + 4.0)),
                      look_at((mid[0] + 0.5, mid[1] - 0.75, -1.0), mid)])
    if nan_pose:
        poses[1, 2, 1] = np.nan
    K0 = intrinsics(2.0 * W, 0.0, 0.0)
    K0[1, 1] = 2.0 * H
    Ks = np.stack([K0, intrinsics(0.75 * W, W / 2.0, H / 2.0), intrinsics(1.0 * W, W / 2.0, H / 2.0)])
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.empty((3, H, W), F32)
    depth[0] = 0.75 + 0.25 * ((xx + 2 * yy) % 12)
    for v in (1, 2):
        depth[v] = np.where((3 * xx + 5 * yy + v) % 7 == 0, np.inf, (0.5 if v == 1 else 1.5) + 0.125 * ((2 * xx + yy) % 16))
    claims, taken, kind = [], set(), 0
    if min(shape) > 0:
        X = FR.lattice(shape, origin, EDGE_VOXEL)
        cz, u, w, usable = R.project(X, poses[0], R.intr4(Ks[0], 1)[0], EDGE_NEAR)
        ok = usable & (u >= 0) & (u < F32(W)) & (w >= 0) & (w < F32(H))
        idx = np.stack(np.unravel_index(np.arange(len(X)), shape), axis=1)
        for j in np.nonzero(ok & (idx[:, 0] + idx[:, 1] > 0) & (cz > F32(EDGE_NEAR)) & (cz <= F32(3.0)))[0]:
            px, py = int(np.floor(u[j])), int(np.floor(w[j]))
            if (px, py) in taken:
                continue
            taken.add((px, py))
            name = EDGE_KINDS[kind % len(EDGE_KINDS)]
            depth[0, py, px] = _edge_depth(name, cz[j])
            claims.append((name, tuple(int(t) for t in idx[j]), (px, py)))
            kind += 1
    return dict(shape=shape, origin=origin, voxel=EDGE_VOXEL, trunc=EDGE_TRUNC, near=EDGE_NEAR, max_depth=EDGE_MAX_DEPTH,
                max_weight=EDGE_MAX_WEIGHT, poses=poses[:V], intr=Ks[:V], depth=depth[:V], view_weight=np.array(EDGE_WEIGHTS, F32)[:V],
                claims=claims)
