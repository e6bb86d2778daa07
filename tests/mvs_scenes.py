"""Deterministic scenes for the multi-view stereo tests (numpy only).  Each returns a dict; callers do not write into it.

exact_scene(last)   a textured plane at the dyadic depth 4 under five translated cameras, every number dyadic, whole-pixel
                    disparities: the sweep's answer is known in closed form.
sphere_scene()      a sphere with a procedural texture of world position, rendered analytically for 5 cameras of 64 x 64: where
                    THE SWEEP RULE and THE CONSISTENCY RULE are judged by their properties (tests/test_mvs_host.py).
grid_scene(...)     six axis-parallel cameras over a random dyadic texture on the plane z = 1: the shapes and the edge cases of the
                    bit-for-bit tests.
den_scene()         three planes whose scores are pred(1), 1, 1: the refinement's den is exactly 0.
filter_scene(...)   grid_scene's cameras with hand-made depth maps: the edge cases of the consistency filter."""
import functools

import numpy as np

import mvs_restate as MR
from fusion_scenes import sphere_depth
from raster_scenes import intrinsics, look_at

F32 = np.float32
TILE = 16                   # LS2FM_MVS_TILE of include/ls2fm.h (tests/test_mvs_host.py pins the copy)
FOCAL = 16.0


def _translated(C):
    """world-to-camera [I | -C]"""
    return np.concatenate([np.eye(3), -np.asarray(C, np.float64)[:, None]], axis=1).astype(F32)


def _texture(rng, h, w):
    """dyadic values k / 256 in [0, 1)"""
    return (rng.integers(0, 256, size=(h, w)) / 256.0).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ exact scene
@functools.lru_cache(maxsize=None)
def exact_scene(last=False):
    """24 x 32 images, f = 16, c = (16, 12); the plane z = 4 carries the texture T; camera i sits at (sx / 4, sy / 4, 0), so its image
    is T shifted by the whole pixels (sx, sy) = (0, 0), (2, 0), (-2, 0), (2, 1), (-2, 1) and a tap (qx, qy) of reference 0 lands in
    source i at x0 = qx - sx, y0 = qy - sy with tx = ty = 0.  A sample needs its right and lower neighbours inside, so the
    sources without a shift in y lose the last row of windows and those shifted by +2 in x the first columns: with w = 2 every
    pixel that has a window sees the true plane in at least one of the four.  depths holds 4 first (last=False) or last."""
    H, W, m = 24, 32, 8
    T = _texture(np.random.default_rng(11), H + 2 * m, W + 2 * m)
    shifts = [(0, 0), (2, 0), (-2, 0), (2, 1), (-2, 1)]
    images = np.stack([T[m + sy:m + sy + H, m + sx:m + sx + W] for sx, sy in shifts])
    poses = np.stack([_translated((sx / 4.0, sy / 4.0, 0.0)) for sx, sy in shifts])
    depths = np.array([2.0, 8.0, 3.0, 4.0] if last else [4.0, 2.0, 8.0, 3.0], F32)
    return dict(images=images, poses=poses, intr=intrinsics(FOCAL, W / 2.0, H / 2.0), refs=np.array([0]), sources=np.array([[1, 2, 3, 4]]),
                depths=depths[None], true_plane=3 if last else 0, half_width=2, near=0.5, min_var=1e-6, min_sources=1, H=H, W=W)


# ----------------------------------------------------------------------------------------------------------------- sphere scene
SPHERE_R, SPHERE_D = 0.5, 2.5


def sphere_texture(X):
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    return 0.5 + 0.15 * np.sin(37.0 * x + 1.3) + 0.15 * np.sin(41.0 * y + 0.7) + 0.15 * np.sin(43.0 * z + 2.1) + 0.1 * np.sin(23.0 * (x + y + z))


@functools.lru_cache(maxsize=None)
def sphere_scene(hw=64, D=48):
    """5 cameras at distance 2.5 from a sphere of radius 0.5 at the origin: one on the -z axis, four turned 12 degrees about the
    x and y axes; f = 2 hw, so the sphere's silhouette has a radius of about 0.4 hw pixels.  The image of a pixel is the texture at
    the point its centre's ray hits, NaN off the sphere (a masked photograph: a window that leaves the sphere is not valid).  D planes uniform in depth
    over [1.9, 2.6]; every view takes the other four as sources.  bounds and voxel: the volume of the end-to-end test."""
    a = np.deg2rad(12.0)
    dirs = [(0, 0, -1), (np.sin(a), 0, -np.cos(a)), (-np.sin(a), 0, -np.cos(a)), (0, np.sin(a), -np.cos(a)), (0, -np.sin(a), -np.cos(a))]
    eyes = np.array(dirs, np.float64) * SPHERE_D
    poses = np.stack([look_at(e, (0, 0, 0)) for e in eyes])
    K = intrinsics(2.0 * hw, hw / 2.0, hw / 2.0)
    K64 = K.astype(np.float64)
    depth = np.stack([sphere_depth(eyes[i], poses[i], K64, hw, hw, SPHERE_R) for i in range(5)])
    yy, xx = np.mgrid[0:hw, 0:hw].astype(np.float64)
    rays = np.stack([(xx + 0.5 - K64[0, 2]) / K64[0, 0], (yy + 0.5 - K64[1, 2]) / K64[1, 1], np.ones_like(xx)], axis=-1)
    images = np.empty((5, hw, hw), F32)
    for i in range(5):
        Rm = poses[i].astype(np.float64)[:, :3]
        z = np.where(np.isfinite(depth[i]), depth[i], 0.0).astype(np.float64)
        X = (rays * z[..., None]) @ Rm + eyes[i]                       # R^T c + eye
        images[i] = np.where(np.isfinite(depth[i]), sphere_texture(X), np.nan)
    sources = np.array([[j for j in range(5) if j != i] for i in range(5)])
    depths = np.linspace(1.9, 2.6, D).astype(F32)
    return dict(images=images, poses=poses, intr=K, sources=sources, depths=np.broadcast_to(depths, (5, D)).copy(), depth=depth,
                spacing=float(np.diff(depths.astype(np.float64)).max()), half_width=2, near=1e-3, min_var=1e-4, min_sources=2,
                max_reproj=1.0, rel_depth=0.01, min_consistent=2, H=hw, W=hw, bounds=((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6)), voxel=0.05)


# ------------------------------------------------------------------------------------------------------------------- grid scene
GRID_CAMERAS = [(0, 0, 0), (0.125, 0, 0), (-0.125, 0, 0), (0, 0.125, 0), (0, -0.125, 0), (0.0625, 0.03125, 0.75)]
GRID_NEAR = 0.5
# plane 0.5 is c_z == near for the cameras at z = 0 and lies behind camera 5; 0.25 is below near for every camera; 1 is the
# true plane, twice; 2 and 0.5 give whole-pixel disparities 1 and 4, the others fractions
GRID_DEPTHS = [0.5, 0.25, 1.0, 1.0, 2.0, 4.0, 0.75, 1.5, 3.0, 8.0, 0.625, 1.25, 0.875, 1.125, 6.0, 1.0625, 0.9375]


def block_var(blocks):
    """va of windows given as float32 [N, n] rows in tap order, by the rule's arithmetic"""
    blocks = np.asarray(blocks, F32)
    n = F32(blocks.shape[1])
    s = np.zeros(len(blocks), F32)
    for i in range(blocks.shape[1]):
        s = s + blocks[:, i]
    ma = s / n
    va = np.zeros(len(blocks), F32)
    for i in range(blocks.shape[1]):
        va = va + (blocks[:, i] - ma) * (blocks[:, i] - ma)
    assert va.dtype == F32
    return va


def ulp_pair(w):
    """two windows of (2 w + 1)^2 taps whose va are a float and the float below it: zero but for the centre tap, 1 / 16, and the
    first tap, j 2^-27, which moves va by less than an ulp per step: j is searched -> (block_at, block_below, va_at)"""
    n = (2 * w + 1) ** 2
    blocks = np.zeros((128, n), F32)
    blocks[:, n // 2] = 1 / 16.0
    blocks[:, 0] = np.arange(1, 129) * 2.0 ** -27
    va = block_var(blocks)
    below = np.nextafter(va, F32(-np.inf))
    for i in range(len(va)):
        j = np.nonzero(va == below[i])[0]
        if len(j):
            return blocks[i].reshape(2 * w + 1, -1), blocks[j[0]].reshape(2 * w + 1, -1), float(va[i])
    raise AssertionError("no pair of windows one ulp apart among the candidates")


@functools.lru_cache(maxsize=None)
def grid_scene(H, W, w=1, S=5, R=3, D=17, nan_pose=False, patches=False):
    """Six cameras with identity rotation at GRID_CAMERAS, f = 16, c = (W / 2, H / 2).  The plane z = 1 carries a random dyadic
    texture T; camera i at (a, b, 0) sees T shifted by (16 a, 16 b) = (2, 0), (-2, 0), (0, 2), (0, -2) whole pixels, so on the plane
    d a tap of reference 0 lands in source 1 at x0 = qx - 2 / d with tx = 0 for d = 1, 2, 1 / 2: x0 takes the values 0, -1, W - 2
    and W - 1 in sources 1 and 2, y0 likewise in sources 3 and 4.  Camera 5 stands further in, its image is another texture.
    The references are views 0, 1, 5 (the first R), their source rows hold a -1 in column 1 (S >= 2) or, for reference 1, as the
    only entry (S = 1); a view serves as reference and as source.  The depth rows are the first D of GRID_DEPTHS, rolled per
    reference so that the true plane comes first for reference 0 (D <= 2: depths start at 1) and last for reference 1.
    Pixels: a NaN in view 0, +inf in view 1, -inf in view 2.  nan_pose puts a NaN into view 2's pose.  patches (w = 1 or 2, an image
    of at least 17 x 33): two flat windows from ulp_pair are written into T, and min_var is the first one's va, so va == min_var at
    one pixel of reference 0 and one ulp below at another, and vb likewise in source 1; otherwise min_var = 1 / 64."""
    rng = np.random.default_rng(1000 * H + 10 * W + w)
    m = 4
    T = _texture(rng, H + 2 * m, W + 2 * m)
    min_var, claims = 1.0 / 64, {}
    if patches:
        at, below, min_var = ulp_pair(w)
        side = 2 * w + 1
        ya, xa, yb, xb = w + 1, 4 + w, w + 1 + side + 1, 4 + w + side + 2          # the centres, in view 0's pixels
        assert yb + w < H - 1 and xb + w < W - 1
        T[m + ya - w:m + ya + w + 1, m + xa - w:m + xa + w + 1] = at
        T[m + yb - w:m + yb + w + 1, m + xb - w:m + xb + w + 1] = below
        claims = dict(va_at=(ya, xa), va_below=(yb, xb))
    shift = lambda sx, sy: T[m + sy:m + sy + H, m + sx:m + sx + W].copy()
    images = np.stack([shift(0, 0), shift(2, 0), shift(-2, 0), shift(0, 2), shift(0, -2), _texture(rng, H, W)])
    images[0, H - 3, W // 2] = np.nan
    images[1, H - 2, 3] = np.inf
    images[2, 1, W - 3] = -np.inf
    poses = np.stack([_translated(C) for C in GRID_CAMERAS])
    if nan_pose:
        poses[2, 2, 3] = np.nan
    refs = np.array([0, 1, 5])[:R]
    rows = np.array([[1, -1, 2, 3, 4], [0, -1, 2, 3, 5], [0, -1, 1, 2, 3]])
    if S == 1:
        rows = np.array([[1], [-1], [0]])
    base = np.array(GRID_DEPTHS if D > 2 else [1.0, 2.0], F32)[:D]
    first = int(np.argmax(base == 1.0))
    depths = np.stack([np.roll(base, -first), np.roll(base, D - 1 - first), base])
    if D > 3:
        depths[1, 0] = 5.0                                             # the second 1 of GRID_DEPTHS, rolled to the front
    depths = depths[:R]
    return dict(images=images, poses=poses, intr=intrinsics(FOCAL, W / 2.0, H / 2.0), refs=refs, sources=rows[:R, :S], depths=depths,
                half_width=w, near=GRID_NEAR, min_var=min_var, min_sources=min(2, S), H=H, W=W, claims=claims)


# -------------------------------------------------------------------------------------------------------------------- den scene
@functools.lru_cache(maxsize=None)
def den_scene():
    """w = 1, one source at (1 / 8, 0, 0), planes (2, 1, 1): disparities 1, 2, 2.  The reference's rows are constant, g_i, but for
    column xc = 6, which holds g_i + e_i; the source is the reference shifted by 2.  At the pixel (xc - 2, 2) the reference window is
    (g_i, g_i, g_i) per row, the source window on the planes 1 is the same -- score 1 -- and on the plane 2 it is
    (g_i, g_i, g_i + e_i): a score just below 1.  e is searched until that score is the float below 1: then
    den = (pred(1) - 2) + 1 rounds to 0.  -> the scene, `pixel` = (y, x)"""
    H, W, xc = 5, 12, 6
    g = np.array([0.25, 0.5, 0.75, 0.375, 0.625], F32)
    K = intrinsics(FOCAL, W / 2.0, H / 2.0)
    poses = np.stack([_translated((0, 0, 0)), _translated((0.125, 0, 0))])
    want = np.nextafter(F32(1), F32(0))
    for j in range(1, 512):
        e = (np.array([1.0, -2.0, 1.5, 0.5, -1.0]) * j * 2.0 ** -17).astype(F32)
        wide = np.repeat(g[:, None], W + 2, axis=1)
        wide[:, xc] = g + e
        images = np.stack([wide[:, :W], wide[:, 2:W + 2]])
        sc = dict(images=images, poses=poses, intr=K, refs=np.array([0]), sources=np.array([[1]]),
                  depths=np.array([[2.0, 1.0, 1.0]], F32), half_width=1, near=0.5, min_var=1e-6, min_sources=1, H=H, W=W, pixel=(2, xc - 2))
        _, _, _, scores = MR.sweep(images, poses, K, sc["sources"], sc["depths"], refs=sc["refs"], half_width=1, near=0.5, min_var=1e-6,
                                   return_scores=True)
        s = scores[0][:, 2, xc - 2]
        if s[0] == want and s[1] == 1 and s[2] == 1:
            return sc
    raise AssertionError("no perturbation gives the float below 1")


# ----------------------------------------------------------------------------------------------------------------- filter scene
FILTER_VALUES = [1.0, 1.0, 1.0, 2.0, 1.25, np.nan, 0.0, -1.0, np.inf, 1.0, 1.0]


@functools.lru_cache(maxsize=None)
def filter_scene(H, W, S=5, nan_pose=False):
    """grid_scene's cameras; every depth map shows the plane z = 1 (1 for the cameras at z = 0, 1 / 4 for camera 5) but for a
    pattern of FILTER_VALUES: 2 at the source pixel puts the point one pixel off on the way back -- the reprojection test at
    equality with max_reproj = 1; 1.25 against 1 is the depth test at equality with rel_depth = 1 / 4; NaN, 0, -1 and inf are
    refused.  Every view has the S first of the other views as sources, with a -1 in column 1 (S >= 2)."""
    V = len(GRID_CAMERAS)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.empty((V, H, W), F32)
    for v in range(V):
        pick = np.asarray(FILTER_VALUES, F32)[(3 * xx + 5 * yy + 2 * v) % len(FILTER_VALUES)]
        depth[v] = pick * F32(0.25 if v == 5 else 1.0)
    poses = np.stack([_translated(C) for C in GRID_CAMERAS])
    if nan_pose:
        poses[2, 2, 3] = np.nan
    sources = np.array([[j for j in range(V) if j != i][:S] for i in range(V)])
    if S >= 2:
        sources[:, 1] = -1
    return dict(depth=depth, poses=poses, intr=intrinsics(FOCAL, W / 2.0, H / 2.0), sources=sources, near=GRID_NEAR, max_reproj=1.0,
                rel_depth=0.25, H=H, W=W)
