"""Image-quality metrics of rendered views against photographs, on the device: PSNR and SSIM, batched over views.

  compare_images   per-view squared error, PSNR and SSIM of two image batches (ls2fm_image_compare, csrc/image_metrics.hip)
  psnr, ssim       shorthands for one figure per view
  gaussian_window  the 11-tap, sigma 1.5 window of Wang et al. (the default);  uniform_window  scikit-image's 7-tap default

The rule (include/ls2fm.h): everything in fp64 from the fp32 pixels -- the squared error per pixel and channel, and SSIM over
the VALID region (no padding: a window never leaves the image): the five moments blurred separably, rows first, tap by tap
with one rounding per operation, then one expression and one division.  In fp32 the variance E[xx] - E[x]^2 cancels on the
smooth bright regions a DTU background is made of (4e-4 in SSIM on a 0.90 - 0.91 ramp); here the figure does not depend on who
wrote the convolution.  Two identical images give exactly 1.0 and psnr = +inf.  The window's taps are computed here with numpy
and handed to the library, which evaluates no exp itself.

The sums are taken in a stated order (tile by tile, lane by lane: include/ls2fm.h) without floating-point atomics, so a rerun,
a view taken alone and a graph replay give the same bits.  Nothing is read back to the host: every score is a device tensor and
a call can be captured into a graph.  tests/image_metrics_restate.py holds map and sums bit for bit.

CPU tensors take a second path: the same rule as plain torch ops in fp64, tap by tap (`_compare_taps`).  Its map follows the
same operations; its sums are torch.sum's, so they are NOT bit-identical to the device's (they agree within the rounding of an
fp64 sum).  `_compare_torch` is the form a user would write -- grouped conv2d in fp64 with the same taps -- kept as the timing
baseline (tools/time_image_metrics.py) and a check; nothing falls back to it.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

TILE = 16             # LS2FM_IMAGE_TILE of include/ls2fm.h: the tile of the summation order
MAX_TAPS = 33         # LS2FM_IMAGE_MAX_TAPS


def gaussian_window(size=11, sigma=1.5):
    """exp(-k^2 / 2 sigma^2) for k = -(size - 1) / 2 .. (size - 1) / 2, normalised by its sum: numpy fp64 [size]"""
    size = int(size)
    k = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    return g / g.sum()


def uniform_window(size=7):
    """1 / size, size times: numpy fp64 [size]"""
    return np.full(int(size), 1.0 / int(size), dtype=np.float64)


@dataclass
class ImageScores:
    """Per-view scores, each a tensor [N] on the inputs' device.  mse = sse / count, psnr = 10 log10(data_range^2 / mse),
    ssim = ssim_sum / ssim_count; a view without counted pixels has counts 0 and NaN scores."""
    sse: torch.Tensor                 # float64: sum of squared differences over the counted pixel-channels
    count: torch.Tensor               # int64: counted pixel-channels
    ssim_sum: torch.Tensor            # float64: sum of SSIM over the counted window centres, all channels
    ssim_count: torch.Tensor          # int64
    mse: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor
    data_range: float
    ssim_map: Optional[torch.Tensor] = None      # float64 [N, H - n + 1, W - n + 1, C] when full=True

    def mean(self):
        """the row of a results table: (mean PSNR, mean SSIM) over the views that have pixels, as 0-d device tensors"""
        has = (self.count > 0).to(torch.float64)
        has_s = (self.ssim_count > 0).to(torch.float64)
        zero = torch.zeros_like(self.psnr)
        return (torch.where(self.count > 0, self.psnr, zero).sum() / has.sum(),
                torch.where(self.ssim_count > 0, self.ssim, zero).sum() / has_s.sum())


def _scores(sse, count, ssim_sum, ssim_count, data_range, ssim_map):
    mse = sse / count.to(torch.float64)
    psnr = 10.0 * torch.log10(float(data_range) ** 2 / mse)
    return ImageScores(sse=sse, count=count, ssim_sum=ssim_sum, ssim_count=ssim_count, mse=mse, psnr=psnr,
                       ssim=ssim_sum / ssim_count.to(torch.float64), data_range=float(data_range), ssim_map=ssim_map)


def _batch(a, b, mask, H, W):
    """-> a, b float32 [N, H, W, C] contiguous, mask uint8 [N, H, W] or None, was_uint8"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape:
        raise ValueError(f"ls2fm.image_metrics: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    if a.device != b.device:
        raise ValueError(f"ls2fm.image_metrics: images on {a.device} and {b.device}")
    was_u8 = a.dtype == torch.uint8 and b.dtype == torch.uint8
    if (H is None) != (W is None):
        raise ValueError("ls2fm.image_metrics: give both H and W, or neither")
    if H is not None:
        if a.dim() != 3 or a.shape[1] != int(H) * int(W):
            raise ValueError(f"ls2fm.image_metrics: with H={H}, W={W} the images must be [N, {int(H) * int(W)}, C], got {tuple(a.shape)}")
        shape = (a.shape[0], int(H), int(W), a.shape[2])
    elif a.dim() == 4:
        shape = tuple(a.shape)
    elif a.dim() == 3 and a.shape[-1] <= 4:
        shape = (1,) + tuple(a.shape)                 # [H, W, C]
    elif a.dim() == 3:
        shape = tuple(a.shape) + (1,)                 # [N, H, W]
    else:
        raise ValueError(f"ls2fm.image_metrics: images must be [H, W, C], [N, H, W, C], [N, H, W] or [N, HW, C] with H=, W=; got {tuple(a.shape)}")
    if not 1 <= shape[3] <= 4:
        raise ValueError(f"ls2fm.image_metrics: {shape[3]} channels, outside 1 .. 4")
    a, b = _lib.cf(a.detach()).reshape(shape), _lib.cf(b.detach()).reshape(shape)
    if mask is not None:
        mask = torch.as_tensor(mask)
        if mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != shape[0] * shape[1] * shape[2]:
            raise ValueError(f"ls2fm.image_metrics: mask must be bool or uint8 with {shape[0]} x {shape[1]} x {shape[2]} entries, "
                             f"got {mask.dtype} {tuple(mask.shape)}")
        if mask.device != a.device:
            raise ValueError(f"ls2fm.image_metrics: images on {a.device}, mask on {mask.device}")
        mask = mask.contiguous().view(torch.uint8).reshape(shape[:3])
    return a, b, mask, was_u8


def _window(window, shape):
    taps = gaussian_window() if window is None else np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    n = int(taps.size)
    if taps.ndim != 1 or n < 1 or n > MAX_TAPS or n % 2 == 0:
        raise ValueError(f"ls2fm.image_metrics: the window must be an odd number of taps in 1 .. {MAX_TAPS}, got shape {taps.shape}")
    if shape[1] < n or shape[2] < n:
        raise ValueError(f"ls2fm.image_metrics: images of {shape[1]} x {shape[2]} are smaller than the window of {n} taps")
    return taps


def _constants(data_range, was_u8, k1, k2):
    data_range = (255.0 if was_u8 else 1.0) if data_range is None else float(data_range)
    c1, c2 = (float(k1) * data_range) ** 2, (float(k2) * data_range) ** 2
    if not (0.0 <= c1 < math.inf and 0.0 <= c2 < math.inf):
        raise ValueError(f"ls2fm.image_metrics: c1 = {c1}, c2 = {c2} must be non-negative and finite")
    return data_range, c1, c2


@torch.no_grad()
def compare_images(a, b, mask=None, data_range=None, window=None, k1=0.01, k2=0.03, full=False, H=None, W=None) -> ImageScores:
    """Compare two batches of images view by view -> ImageScores.
      a, b        [H, W, C], [N, H, W, C], [N, H, W] (one channel) or, with H= and W=, [N, HW, C] (render_image's rgb); 1 <= C <= 4;
                  float32, or uint8 converted with .float()
      mask        bool or uint8, [N, H, W] (or [H, W], or [N, HW]): the pixels that count; SSIM counts the windows whose CENTRE
                  pixel is on.  None: all
      data_range  the span of the values: 1.0 by default, 255 when both images are uint8
      window      numpy fp64 taps, odd, at most 33 (gaussian_window() by default), used along both axes
      k1, k2      c1 = (k1 data_range)^2, c2 = (k2 data_range)^2
      full        also return ssim_map [N, H - n + 1, W - n + 1, C]
    On the device: one call of ls2fm_image_compare, nothing read back.  On CPU tensors: the same rule as torch ops in fp64."""
    a, b, mask, was_u8 = _batch(a, b, mask, H, W)
    taps = _window(window, a.shape)
    data_range, c1, c2 = _constants(data_range, was_u8, k1, k2)
    if not a.is_cuda:
        return _compare_taps(a, b, mask, taps, c1, c2, data_range, full)
    lib = _lib.load()
    N, Hh, Ww, C = (int(s) for s in a.shape)
    n, dev = int(taps.size), a.device
    if Hh * Ww * C >= 1 << 31:
        raise ValueError(f"ls2fm.image_metrics: {Hh} x {Ww} x {C} is 2^31 pixel-channels per view or more")
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.ls2fm_image_compare_workspace_bytes(N, Hh, Ww, C, n), "ls2fm_image_compare_workspace_bytes", dev)
        sums = torch.empty(2, N, dtype=torch.float64, device=dev)
        counts = torch.empty(2, N, dtype=torch.int64, device=dev)
        smap = torch.empty(N, Hh - n + 1, Ww - n + 1, C, dtype=torch.float64, device=dev) if full else None
        check(lib.ls2fm_image_compare(ptr(a), ptr(b), ptr(mask), N, Hh, Ww, C, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n,
                                      c1, c2, ptr(sums[0]), ptr(counts[0]), ptr(sums[1]), ptr(counts[1]), ptr(smap), ptr(ws),
                                      ws.numel(), stream_ptr()), "ls2fm_image_compare")
        return _scores(sums[0], counts[0], sums[1], counts[1], data_range, smap)


def psnr(a, b, mask=None, data_range=None, H=None, W=None):
    """PSNR per view, float64 [N] on the images' device"""
    return compare_images(a, b, mask=mask, data_range=data_range, window=np.ones(1), H=H, W=W).psnr


def ssim(a, b, mask=None, data_range=None, window=None, k1=0.01, k2=0.03, H=None, W=None):
    """mean SSIM per view, float64 [N] on the images' device"""
    return compare_images(a, b, mask=mask, data_range=data_range, window=window, k1=k1, k2=k2, H=H, W=W).ssim


def _sums(se, sm, mask, n, data_range, full):
    """the four per-view numbers from the per-pixel squared errors and the SSIM map, with torch.sum"""
    N, Hh, Ww, C = se.shape
    r = (n - 1) // 2
    on = torch.ones(N, Hh, Ww, dtype=torch.bool, device=se.device) if mask is None else mask != 0
    ctr = on[:, r:Hh - n + 1 + r, r:Ww - n + 1 + r]
    zero = torch.zeros((), dtype=torch.float64, device=se.device)
    sse = torch.where(on[..., None], se, zero).reshape(N, -1).sum(dim=1)
    ssum = torch.where(ctr[..., None], sm, zero).reshape(N, -1).sum(dim=1)
    return _scores(sse, on.reshape(N, -1).sum(dim=1) * C, ssum, ctr.reshape(N, -1).sum(dim=1) * C, data_range, sm if full else None)


def _ssim_expr(mx, my, xx, yy, xy, c1, c2):
    vx, vy, cxy = xx - mx * mx, yy - my * my, xy - mx * my
    return ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def _compare_taps(a, b, mask, taps, c1, c2, data_range, full):
    """the rule as separate torch ops in fp64, tap by tap: acc = w[0] v[0]; acc = acc + w[k] v[k]"""
    x, y = a.double(), b.double()
    n = int(taps.size)

    def blur(v, dim):
        length = v.shape[dim] - n + 1
        acc = float(taps[0]) * v.narrow(dim, 0, length)
        for k in range(1, n):
            acc = acc + float(taps[k]) * v.narrow(dim, k, length)
        return acc

    m = [blur(blur(v, 2), 1) for v in (x, y, x * x, y * y, x * y)]
    d = x - y
    return _sums(d * d, _ssim_expr(*m, c1, c2), mask, n, data_range, full)


@torch.no_grad()
def _compare_torch(a, b, mask=None, data_range=None, window=None, k1=0.01, k2=0.03, full=False, H=None, W=None) -> ImageScores:
    """compare_images as a user would write it with torch ops, on whatever device the tensors are on: the five moments by one
    grouped conv2d per axis in fp64 with the same taps (rows first), then the same expression.  The convolution's own summation
    order and contraction apply, so the map agrees with the kernel's to rounding, not by its bits."""
    a, b, mask, was_u8 = _batch(a, b, mask, H, W)
    taps = _window(window, a.shape)
    data_range, c1, c2 = _constants(data_range, was_u8, k1, k2)
    N, Hh, Ww, C = a.shape
    n = int(taps.size)
    x, y = a.double().permute(0, 3, 1, 2), b.double().permute(0, 3, 1, 2)
    v = torch.cat([x, y, x * x, y * y, x * y], dim=1)                        # [N, 5 C, H, W]
    w = torch.from_numpy(taps).to(a.device)
    v = torch.nn.functional.conv2d(v, w.view(1, 1, 1, n).expand(5 * C, 1, 1, n), groups=5 * C)
    v = torch.nn.functional.conv2d(v, w.view(1, 1, n, 1).expand(5 * C, 1, n, 1), groups=5 * C)
    m = [t.permute(0, 2, 3, 1) for t in v.split(C, dim=1)]
    d = a.double() - b.double()
    return _sums(d * d, _ssim_expr(*m, c1, c2), mask, n, data_range, full)
