"""Procedural test images for ls2fm.features (no image file is committed): band-limited noise plus a few dozen random blobs and
rectangles from a seeded numpy generator, float32 in [0, 1].
  A  47 x 61     odd sizes: tile edges, the halo, the odd down-sampling, the octave cut-off
  B  96 x 128
  C  a 240 x 320 pair: the second view is the first warped by a known similarity (15 degrees, scale 1.2), resampled bilinearly
  D  a constant image
  S16, S23, S31, S33  16 x 16 (the smallest legal size), 16 x 23, 31 x 18, 33 x 64: views of two and three octaves (33 x 64: three
     and four, the last exactly 8 high), to stand alone and beside longer views in one batch
  E  130 x 177 with two grids of Gaussian blobs sized for the deep octaves: sides 260 x 354, 130 x 177, 65 x 88, 32 x 44, odd
     where they are halved"""
import numpy as np

SIM_ANGLE = np.deg2rad(15.0)
SIM_SCALE = 1.2


def _smooth(a, passes):
    for _ in range(passes):
        a = (np.roll(a, 1, 0) + 2.0 * a + np.roll(a, -1, 0)) / 4.0
        a = (np.roll(a, 1, 1) + 2.0 * a + np.roll(a, -1, 1)) / 4.0
    return a


def scene(h, w, seed, shapes=40):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w))
    for passes, amp in ((2, 0.10), (8, 0.25), (32, 0.35)):
        n = _smooth(rng.standard_normal((h, w)), passes)
        img += amp * n / n.std()
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for _ in range(shapes):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        amp = rng.uniform(0.25, 0.6) * rng.choice([-1.0, 1.0])
        if rng.uniform() < 0.5:
            s = rng.uniform(1.5, 0.06 * min(h, w) + 2.0)
            img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
        else:
            hy, hx = rng.uniform(2.0, 0.1 * h + 3.0), rng.uniform(2.0, 0.1 * w + 3.0)
            img += amp * ((np.abs(yy - cy) < hy) & (np.abs(xx - cx) < hx))
    img = (img - img.min()) / (img.max() - img.min())
    return np.ascontiguousarray(img.astype(np.float32))


def similarity(h, w):
    """3x3 matrix mapping pixel coordinates (COLMAP convention, first pixel centre at 0.5) of the first view of C to the second:
    rotation by SIM_ANGLE and scale SIM_SCALE about the image centre"""
    c, s = SIM_SCALE * np.cos(SIM_ANGLE), SIM_SCALE * np.sin(SIM_ANGLE)
    cx, cy = w / 2.0, h / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0.0, 0.0, 1.0]])


def warp(img, M):
    """second view: out(p) = img(M^-1 p), bilinear, edge replication"""
    h, w = img.shape
    Mi = np.linalg.inv(M)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    px, py = xx + 0.5, yy + 0.5
    sx = Mi[0, 0] * px + Mi[0, 1] * py + Mi[0, 2] - 0.5
    sy = Mi[1, 0] * px + Mi[1, 1] * py + Mi[1, 2] - 0.5
    sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.minimum(np.floor(sx).astype(int), w - 2), np.minimum(np.floor(sy).astype(int), h - 2)
    fx, fy = sx - x0, sy - y0
    a = img.astype(np.float64)
    out = (a[y0, x0] * (1 - fx) + a[y0, x0 + 1] * fx) * (1 - fy) + (a[y0 + 1, x0] * (1 - fx) + a[y0 + 1, x0 + 1] * fx) * fy
    return np.ascontiguousarray(out.astype(np.float32))


SEED_A, SEED_B, SEED_C = 11, 12, 13


def scene_a():
    return scene(47, 61, SEED_A, shapes=24)


def scene_b():
    return scene(96, 128, SEED_B, shapes=40)


def scene_c():
    """-> (first view, second view, the similarity first -> second)"""
    first = scene(240, 320, SEED_C, shapes=60)
    M = similarity(240, 320)
    return first, warp(first, M), M


def scene_d():
    return np.full((40, 56), 0.37, dtype=np.float32)


# name -> (height, width, seed); SMALL_ROWS: rows of the float64 restatement at first_octave -1 and 0 (tests/test_sift_host.py
# recomputes them; the GPU tests use them as the floor below which a comparison would be vacuous)
SMALL = {"S16": (16, 16, 21), "S23": (16, 23, 22), "S31": (31, 18, 23), "S33": (33, 64, 24)}
SMALL_ROWS = {"S16": {-1: 4, 0: 1}, "S23": {-1: 10, 0: 2}, "S31": {-1: 9, 0: 3}, "S33": {-1: 44, 0: 14}}


def small(name):
    h, w, seed = SMALL[name]
    return scene(h, w, seed, shapes=12)


SEED_E = 32
# (rows, columns, smallest and largest sigma in pixels, smallest and largest amplitude) of a jittered grid of blobs of alternating
# sign: sigma 8 - 11 px answers in octave index 3 (4 input pixels per pixel at first_octave -1), 3.8 - 5.5 px in octave index 2
GRIDS_E = ((3, 4, 8.0, 11.0, 0.7, 1.1), (6, 8, 3.8, 5.5, 0.3, 0.6))
ROWS_E = (93, 89, 41, 12)              # rows of the float64 restatement per octave index


def scene_e():
    h, w = 130, 177
    rng = np.random.default_rng(SEED_E)
    img = scene(h, w, SEED_E, shapes=30).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for gy, gx, lo, hi, a_lo, a_hi in GRIDS_E:
        for iy in range(gy):
            for ix in range(gx):
                cy = (iy + 0.5 + rng.uniform(-0.2, 0.2)) * h / gy
                cx = (ix + 0.5 + rng.uniform(-0.2, 0.2)) * w / gx
                amp = rng.uniform(a_lo, a_hi) * (1.0 if (iy + ix) % 2 else -1.0)
                s = rng.uniform(lo, hi)
                img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
    img = (img - img.min()) / (img.max() - img.min())
    return np.ascontiguousarray(img.astype(np.float32))
