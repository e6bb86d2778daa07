"""Deterministic cameras and scenes for the undistortion tests (numpy only).  Each returns a dict or arrays; callers do not write
into them.

camera(name, Hs, Ws)   the test cameras float64 [12], scaled to a photograph of Hs x Ws: identity, barrel (with tangential terms),
                       pincushion (with k3), rational (k4 .. k6)
image_scene(...)       three views -- identity, barrel, rational -- of random photographs; the output cameras see a little more than
                       the photographs, so every call has invalid pixels
edge_scene()           8 x 8 photographs under cameras without distortion whose words are dyadic, so u and v are exact: u = 0, u = Ws,
                       one ulp to either side, the clamped taps, den = 0, a NaN and an infinite camera word, NaN and inf pixels
points_scene()         views of 0, 1, 63, 64, 65 and 257 points plus hand-placed ones
wave(...)              the sinusoid photograph of the bilinear-bound test
reimaged_sphere(hw)    the sphere scene's photographs seen through a barrel lens"""
import functools

import numpy as np

import undistort_restate as UR

F32, F64 = np.float32, np.float64
TILE_W, TILE_H = 32, 8      # LS2FM_UNDISTORT_TILE_W, LS2FM_UNDISTORT_TILE_H (tests/test_undistort_host.py pins the copies)

# (Hs, Ws) -> (H, W): inside one tile; a whole tile from one pixel past it on each axis and the reverse; the issue's example; two
# tiles across from one pixel past them
SIZES = [((6, 20), (7, 23)), ((9, 33), (8, 32)), ((8, 32), (9, 33)), ((33, 31), (15, 17)), ((17, 65), (16, 64))]

DISTORTIONS = {                       # k1, k2, p1, p2, k3, k4, k5, k6
    "identity": (0, 0, 0, 0, 0, 0, 0, 0),
    "barrel": (-0.25, 0.08, 1e-3, -5e-4, 0, 0, 0, 0),
    "pincushion": (0.1, 0.02, -7e-4, 3e-4, 0.01, 0, 0, 0),
    "rational": (0.2, 0.05, 1e-3, -5e-4, 0.01, 0.5, 0.02, 0.001),
}


def camera(name, Hs, Ws, f=None):
    """f defaults to the photograph's width: the half field of view is 0.5 across and Hs / (2 Ws) down"""
    f = float(Ws) if f is None else float(f)
    return np.array([f, f * 0.99, Ws / 2.0 + 0.3, Hs / 2.0 - 0.2, *DISTORTIONS[name]], F64)


@functools.lru_cache(maxsize=None)
def image_scene(Hs, Ws, H, W, C):
    rng = np.random.default_rng(Hs * 1000 + Ws * 10 + C)
    cam = np.stack([camera(n, Hs, Ws) for n in ("identity", "barrel", "rational")])
    out_intr = np.array([[0.8 * W, 0.8 * W, W / 2.0 + 0.25 * v, H / 2.0 - 0.125 * v] for v in range(3)], F64)
    return dict(images=rng.random((3, Hs, Ws, C), dtype=F32), cam=cam.astype(F32), out_intr=out_intr.astype(F32), H=H, W=W)


TINY = float(np.nextafter(F32(0), F32(1)))
BELOW_8 = float(np.nextafter(F32(8), F32(0)))
# per view (cx, cy) of a camera without distortion with fx = fy = 4 under out_intr = (4, 4, 2.5, 2.5): u = (px - 2) + cx exactly, so
# column 2 has u = cx and row 2 has v = cy
EDGE_CENTRES = [(0.0, 0.0), (TINY, TINY), (-TINY, 4.0), (8.0, 4.0), (BELOW_8, BELOW_8), (4.0, 8.0), (4.0, -TINY), (0.0, 4.0), (4.0, 4.0),
                (4.0, 4.0), (2.25, 2.75)]
EDGE_DEN0, EDGE_NAN, EDGE_INF, EDGE_PLAIN = 7, 8, 9, 10


@functools.lru_cache(maxsize=None)
def edge_scene(C=2):
    """view 7: k4 = -1, so den = 1 - r2 is exactly 0 where (xn, yn) = (1, 0), the pixel (6, 2); view 8: k2 = NaN; view 9: fx = inf"""
    rng = np.random.default_rng(5)
    V = len(EDGE_CENTRES)
    images = (rng.integers(0, 256, size=(V, 8, 8, C)) / 256.0).astype(F32)
    images[:, 3, 3, 0] = np.nan
    images[:, 2, 5, C - 1] = np.inf
    images[:, 0, 0, 0] = np.nan                 # under the clamped taps of u = 0, v = 0
    cam = np.zeros((V, 12), F32)
    cam[:, 0] = cam[:, 1] = 4.0
    cam[:, 2:4] = np.array(EDGE_CENTRES, F32)
    cam[EDGE_DEN0, 9] = -1.0
    cam[EDGE_NAN, 5] = np.nan
    cam[EDGE_INF, 0] = np.inf
    out_intr = np.tile(np.array([4.0, 4.0, 2.5, 2.5], F32), (V, 1))
    return dict(images=images, cam=cam, out_intr=out_intr, H=8, W=8)


POINT_COUNTS = [0, 1, 63, 64, 65, 257, 4, 3]
FOLD_VIEW, INF_VIEW = 6, 7


@functools.lru_cache(maxsize=None)
def points_scene():
    """photographs of 33 x 47.  Views 0 .. 5: the counts of the issue under the cameras identity, barrel, pincushion, rational, barrel,
    rational; view 2 holds its principal point first, view 3 a NaN point.  View 6 is RADIAL with k1 = -7, k2 = 4: at (x, y) = (1, 0)
    rad = -2 and d rad / d r2 = 1, so J = [0 0; 0 -2] and the start's det is exactly 0; its first point is that one.  View 7 has an
    infinite k1.  out_intr differs from the cameras' own pinholes."""
    rng = np.random.default_rng(9)
    names = ["identity", "barrel", "pincushion", "rational", "barrel", "rational"]
    cam = [camera(n, 33, 47, 40.0) for n in names]
    cam.append(np.array([8.0, 8.0, 4.0, 2.0, -7.0, 4.0, 0, 0, 0, 0, 0, 0], F64))
    cam.append(np.array([40.0, 40.0, 23.5, 16.5, np.inf, 0, 0, 0, 0, 0, 0, 0], F64))
    cam = np.stack(cam)
    start = np.concatenate([[0], np.cumsum(POINT_COUNTS)]).astype(np.int32)
    uv = rng.random((int(start[-1]), 2)) * [47.0, 33.0]
    uv[start[2]] = cam[2, 2:4]
    uv[start[3] + 5] = [np.nan, 7.0]
    uv[start[FOLD_VIEW]] = [8.0 * 1.0 + 4.0, 2.0]
    uv[start[FOLD_VIEW] + 1] = [4.5, 2.25]
    out_intr = np.stack([[c[0] * 1.25, c[1] * 0.75, c[2] + 1.5, c[3] - 0.25] for c in cam])
    return dict(uv=uv, view_start=start, cam=cam, out_intr=out_intr)


def grid_points(Hs, Ws):
    """every pixel centre of an Hs x Ws image, float64 [Hs Ws, 2], row-major"""
    ys, xs = np.mgrid[0:Hs, 0:Ws]
    return np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(F64)


def one_view(n):
    return np.array([0, n], np.int32)


def bilinear64(image, xy):
    """host fp64 bilinear sample of image [H, W] about the pixel centres with clamped taps at the positions xy [N, 2]; NaN stays"""
    H, W = image.shape
    x, y = xy[:, 0] - 0.5, xy[:, 1] - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    tx, ty = x - x0, y - y0
    xa, xb = np.clip(x0, 0, W - 1).astype(int), np.clip(x0 + 1, 0, W - 1).astype(int)
    ya, yb = np.clip(y0, 0, H - 1).astype(int), np.clip(y0 + 1, 0, H - 1).astype(int)
    img = image.astype(F64)
    r0 = img[ya, xa] + tx * (img[ya, xb] - img[ya, xa])
    r1 = img[yb, xa] + tx * (img[yb, xb] - img[yb, xa])
    return r0 + ty * (r1 - r0)


WAVELENGTH = 16.0


def wave(X, Y):
    """P of the issue, at output pixel coordinates"""
    return 0.5 + 0.5 * np.sin(2.0 * np.pi * X / WAVELENGTH) * np.sin(2.0 * np.pi * Y / WAVELENGTH)


@functools.lru_cache(maxsize=None)
def reimaged_sphere(hw=32):
    """mvs_scenes.sphere_scene(hw)'s photographs as a barrel lens of the same focal length and principal point would have taken them:
    every pixel centre of the photograph is undistorted by the restatement's inverse and the pinhole image is sampled there.
    -> (photographs float32 [5, hw, hw], cam float64 [12])"""
    import mvs_scenes
    sc = mvs_scenes.sphere_scene(hw=hw)
    K = sc["intr"].astype(F64)
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], -0.5, 0.1, 2e-3, -1e-3, 0, 0, 0, 0], F64)
    at, res = UR.camera_points(grid_points(hw, hw), one_view(hw * hw), cam[None], cam[None, :4], UR.UNDISTORT, 10)
    assert res.max() < 1e-18
    photos = np.stack([bilinear64(img, at).reshape(hw, hw) for img in sc["images"]]).astype(F32)
    return photos, cam
