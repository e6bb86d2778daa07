"""Small scenes for the image-comparison tests (CPU and GPU), sized through the kernel's tile T: every size at which a tile of
window centres is exactly full, one past, or one short; C = 1, 3, 4; the Gaussian, the uniform, the 1-tap and the 33-tap window
(with the channel counts on either side of the kernel's all-channels-at-once threshold); masks whose edge lies on a tile boundary;
a batch with non-finite pixels in one view and one with an empty mask in one view.  Nothing exceeds 3 views of 80 x 100.

Not a test module: tests/test_image_metrics_host.py and tests/test_hip_image_metrics.py import it."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import image_metrics_restate as R


# the largest |restatement - scipy route| over the finite 11-tap scenes is 1.11e-12, on the ramp (whose variances cancel to
# 1e-6 of the moments; 9.1e-14 on the worst noisy scene): the bound is 4 x that
SCIPY_GAP = 1.11e-12
SCIPY_BOUND = 4 * SCIPY_GAP
# the tap-by-tap CPU path of compare_images performs the restatement's operations: measured gap 0 on every scene, so 4 x 0 --
# equality.  The conv2d form (_compare_torch) has its own summation order: measured gap on the CPU 8.63e-13 (the ramp again)
CONV_GAP = 8.63e-13
CONV_BOUND = 4 * CONV_GAP


@dataclass
class Scene:
    name: str
    a: np.ndarray                      # float32 [N, H, W, C]
    b: np.ndarray
    taps: np.ndarray                   # float64 [n]
    mask: Optional[np.ndarray] = None  # uint8 [N, H, W]
    data_range: float = 1.0
    k1: float = 0.01
    k2: float = 0.03

    @property
    def c1(self):
        return (self.k1 * self.data_range) ** 2

    @property
    def c2(self):
        return (self.k2 * self.data_range) ** 2

    @property
    def finite(self):
        return bool(np.isfinite(self.a).all() and np.isfinite(self.b).all())


def size_class(H, W, n, T):
    """the names of the size classes of the issue that an H x W image with an n-tap window falls into"""
    ch, cw = H - n + 1, W - n + 1
    out = set()
    if (ch, cw) == (1, 1):
        out.add("one centre")
    if (ch, cw) == (2, 2):
        out.add("n + 1")
    if (ch, cw) == (T, T):
        out.add("one tile")
    if (ch, cw) == (T + 1, T):
        out.add("one past in y")
    if (ch, cw) == (T, T + 1):
        out.add("one past in x")
    if (ch, cw) == (2 * T - 1, 2 * T - 1):
        out.add("one short of two tiles")
    return out


SIZE_CLASSES = {"one centre", "n + 1", "one tile", "one past in y", "one past in x", "one short of two tiles"}


def noisy(rng, N, H, W, C, noise=0.08):
    """a smooth random image and a noisy copy of it, both in [0, 1]"""
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = np.stack([0.5 + 0.3 * np.sin(3.0 * (c + 1) * xx + 2.0 * yy + v) * np.cos(2.0 * yy * (v + 1)) for v in range(N) for c in range(C)])
    a = base.reshape(N, C, H, W).transpose(0, 2, 3, 1) + 0.05 * rng.standard_normal((N, H, W, C))
    b = a + noise * rng.standard_normal((N, H, W, C))
    return np.clip(a, 0, 1).astype(np.float32), np.clip(b, 0, 1).astype(np.float32)


def ramp(H=40, W=52):
    """the smooth bright ramp: values 0.90 - 0.91, the second image offset by 0.001: fp32 moments lose 4e-4 of SSIM here"""
    a = (0.90 + 0.01 * np.linspace(0, 1, H * W).reshape(1, H, W, 1)).astype(np.float32)
    return a, (a.astype(np.float64) + 0.001).astype(np.float32)


def scenes(T=16):
    rng = np.random.default_rng(2026)
    gauss, uni, one, wide = R.gaussian_taps(11, 1.5), R.uniform_taps(7), np.ones(1), R.gaussian_taps(33, 5.0)
    n = 11
    out = []

    def add(name, a, b, taps, **kw):
        out.append(Scene(name, np.ascontiguousarray(a), np.ascontiguousarray(b), taps, **kw))

    # ---- the size classes, 11-tap Gaussian, C = 1, 3, 4
    add("one_centre_c3", *noisy(rng, 1, n, n, 3), gauss)
    add("n_plus_1_c1", *noisy(rng, 1, n + 1, n + 1, 1), gauss)
    add("one_tile_c3", *noisy(rng, 1, T + n - 1, T + n - 1, 3), gauss)
    a, b = noisy(rng, 1, T + n, T + n - 1, 3)
    add("past_tile_y_c3_random_mask", a, b, gauss, mask=(rng.random((1, T + n, T + n - 1)) < 0.6).astype(np.uint8))
    add("past_tile_x_c4", *noisy(rng, 1, T + n - 1, T + n, 4), gauss)
    s = 2 * T + n - 2
    a, b = noisy(rng, 1, s, s, 3)
    m = np.zeros((1, s, s), np.uint8)
    m[:, :, :T] = 1                                        # its edge is the boundary between tile columns 0 and 1
    m[:, 2 * T:, :] = 0                                    # and the third tile row (pixels only: no centres there) is off
    add("short_of_two_tiles_c3_mask_on_tile_edge", a, b, gauss, mask=m)
    # ---- content
    add("ramp_c1", *ramp(), gauss)
    a, _ = noisy(rng, 1, 30, 45, 3)
    add("identical_c3", a, a.copy(), gauss)
    add("constants_c3_uniform", np.full((1, 20, 22, 3), 0.25, np.float32), np.full((1, 20, 22, 3), 0.75, np.float32), uni)
    a, b = noisy(rng, 1, 40, 52, 3)
    add("noisy_c3_uniform_random_mask", a, b, uni, mask=(rng.random((1, 40, 52)) < 0.5).astype(np.uint8))
    add("one_tap_c3", *noisy(rng, 1, T + 1, 2 * T + 1, 3), one)
    a, b = noisy(rng, 1, 40, 52, 3)
    add("range_255_c3", np.rint(a * 255).astype(np.float32), np.rint(b * 255).astype(np.float32), gauss, data_range=255.0)
    # ---- 33 taps: C = 1 (all channels in LDS at once), C = 3 (one at a time); the threshold with four channels lies between 21 and 23 taps
    add("wide_c1", *noisy(rng, 1, 2 * T + 33 - 2, T + 33, 1), wide)
    add("wide_c3_one_tile", *noisy(rng, 1, 33, T + 33 - 1, 3), wide)
    add("taps_21_c4", *noisy(rng, 1, T + 21, 21 + 2, 4), R.gaussian_taps(21, 3.0))
    add("taps_23_c4", *noisy(rng, 1, T + 23, 23 + 2, 4), R.gaussian_taps(23, 3.0))
    # ---- batches
    a, b = noisy(rng, 3, 41, 50, 3)
    a[1, 7, 9, 1] = np.nan
    b[1, 30, 44, 2] = np.inf
    add("three_views_nonfinite_in_view_1", a, b, gauss)
    a, b = noisy(rng, 3, 48, 60, 3)
    m = (rng.random((3, 48, 60)) < 0.7).astype(np.uint8)
    m[1] = 0
    add("three_views_empty_mask_in_view_1", a, b, gauss, mask=m)
    return out


def reference(scene, T=16, ordered=True):
    return R.compare(scene.a, scene.b, scene.taps, scene.c1, scene.c2, mask=scene.mask, T=T, ordered=ordered)
