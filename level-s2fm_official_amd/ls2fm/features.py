"""SIFT feature extraction on the device: the `colmap feature_extractor` step of the reference's preparation/main.py:91, so that a
folder of images reaches LevelS2fM.load_matches' `n_views.npy` tables without COLMAP in the loop.

`extract` is VLFeat-style DoG SIFT with COLMAP's default options (first octave -1, 4 octaves of 3 levels, peak 0.02 / 3, edge 10,
at most 2 orientations and 8192 features, L1_ROOT uint8 descriptors in UBC order) for all views in one ls2fm_sift_extract call per
chunk (csrc/sift.hip).  `n_views_from_images` chains it with ls2fm.match.two_view_tables: main.py:91-247 minus the mapper.  Every
rule is stated in include/ls2fm.h; tests/sift_restate.py repeats it in numpy.  No bit parity with COLMAP or OpenCV is claimed.

There is no CPU path: a missing device or library raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

_NORMALIZATIONS = {"l1_root": 0, "l2": 1}
_REC709 = (0.2126, 0.7152, 0.0722)


@dataclass
class SiftOptions:
    """COLMAP's SiftExtractionOptions defaults (those the library restates)"""
    first_octave: int = -1
    num_octaves: int = 4
    octave_resolution: int = 3
    peak_threshold: float = 0.02 / 3
    edge_threshold: float = 10.0
    max_num_features: int = 8192
    max_num_orientations: int = 2
    upright: bool = False
    normalization: str = "l1_root"          # or "l2"
    max_workspace_bytes: int = 0            # 0: the library's default (2 GiB); the library splits a call into chunks below it
    chunk_views: int | None = None          # views per library call (None: all in one call)

    def c_struct(self, debug_levels=None, debug_keys=None):
        if self.normalization not in _NORMALIZATIONS:
            raise ValueError(f"ls2fm.features: normalization must be 'l1_root' or 'l2', got {self.normalization!r}")
        return _lib.SiftOpts(int(self.first_octave), int(self.num_octaves), int(self.octave_resolution), int(self.max_num_features),
                             int(self.max_num_orientations), 1 if self.upright else 0, _NORMALIZATIONS[self.normalization], 0,
                             float(self.peak_threshold), float(self.edge_threshold), int(self.max_workspace_bytes),
                             ctypes.c_void_p(debug_levels.data_ptr()) if debug_levels is not None else ctypes.c_void_p(0),
                             ctypes.c_void_p(debug_keys.data_ptr()) if debug_keys is not None else ctypes.c_void_p(0))


def _grey(image, dev):
    """float32 [H,W] on dev from float / uint8, grey [H,W] or RGB [H,W,3] (Rec.709 weights; that this is COLMAP's bitmap
    conversion is unconfirmed)"""
    t = torch.as_tensor(image)
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3):
        raise ValueError(f"ls2fm.features: an image is [H,W] or [H,W,3], got {tuple(t.shape)}")
    t = t.to(dev)
    if t.dtype == torch.uint8:
        # byte / 255 through a table divided on the host: the correctly rounded quotient whatever the device's division does
        t = (torch.arange(256, dtype=torch.float32) / 255.0).to(dev)[t.long()]
    elif t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.dim() == 3:
        t = (_REC709[0] * t[..., 0] + _REC709[1] * t[..., 1]) + _REC709[2] * t[..., 2]
    return t.contiguous()


def _call(greys, opt, dev, debug=False, with_keys=False):
    """one ls2fm_sift_extract call -> (keypoints [V * max,4], descriptors [V * max,128], counts [V] on the device, levels or None,
    packed keys [V * max,2] or None)"""
    lib = _lib.load()
    V = len(greys)
    heights = np.array([g.shape[0] for g in greys], dtype=np.int32)
    widths = np.array([g.shape[1] for g in greys], dtype=np.int32)
    sizes = heights.astype(np.int64) * widths
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    c_h, c_w, c_off = (a.ctypes.data_as(ctypes.c_void_p) for a in (heights, widths, offsets))
    with torch.cuda.device(dev):
        levels = None
        if debug:
            up = 2 if opt.first_octave == -1 else 1
            h, w, total = int(heights[0]) * up, int(widths[0]) * up, 0
            shapes = []
            for _ in range(opt.num_octaves):
                if min(h, w) < 8:
                    break
                shapes.append((h, w))
                total += 6 * h * w
                h, w = h // 2, w // 2
            levels = torch.empty(total, dtype=torch.float32, device=dev)
        keys = torch.zeros((V * opt.max_num_features, 2), dtype=torch.int32, device=dev) if with_keys else None
        c_opt = opt.c_struct(levels, keys)
        ws = _lib.workspace(lib.ls2fm_sift_workspace_bytes(c_h, c_w, V, ctypes.byref(c_opt)), "ls2fm_sift_workspace_bytes", dev, 256)
        pixels = torch.cat([g.reshape(-1) for g in greys])
        kp = torch.empty((V * opt.max_num_features, 4), dtype=torch.float32, device=dev)
        desc = torch.empty((V * opt.max_num_features, 128), dtype=torch.uint8, device=dev)
        counts = torch.empty(V, dtype=torch.int32, device=dev)
        check(lib.ls2fm_sift_extract(ptr(pixels), c_off, c_h, c_w, V, ctypes.byref(c_opt), ptr(kp), ptr(desc), ptr(counts), ptr(ws),
                                     stream_ptr()), "ls2fm_sift_extract")
        if debug:
            out, at = [], 0
            for h, w in shapes:
                out.append(levels[at:at + 6 * h * w].reshape(6, h, w))
                at += 6 * h * w
            levels = out
    return kp, desc, counts, levels, keys


def extract(images, options=None, return_keys=False):
    """SIFT keypoints and descriptors of every image.  images: list of [H,W] or [H,W,3] arrays / tensors, float in [0,1] or
    uint8, any sizes >= 16 x 16 (moved to the device once).  -> list of (keypoints float32 [n,4] = x, y, scale, orientation in
    COLMAP's pixel convention, descriptors uint8 [n,128]) device tensors, rows in the fixed order of include/ls2fm.h.  One library
    call per chunk of views and one synchronising read (the counts).  return_keys=True (debug): triples with int64 [n,5] = octave
    index, level, y cell, x cell, orientation index, the key the rows are ordered by."""
    images = list(images)
    if len(images) == 0:
        raise ValueError("ls2fm.features: no images")
    opt = options or SiftOptions()
    dev = _lib.find_device("ls2fm.features", images)
    greys = [_grey(i, dev) for i in images]
    step = len(greys) if not opt.chunk_views else max(int(opt.chunk_views), 1)
    parts = [_call(greys[a:a + step], opt, dev, with_keys=return_keys) for a in range(0, len(greys), step)]
    counts = torch.cat([p[2] for p in parts]).cpu().tolist()                 # the one synchronising read
    if min(counts) < 0:
        raise RuntimeError(f"ls2fm.features: view {counts.index(min(counts))} has more accepted extrema than the library holds per view "
                           "(include/ls2fm.h: counts = -1)")
    out, v = [], 0
    for kp, desc, _, _, keys in parts:
        for i in range(kp.shape[0] // opt.max_num_features):
            r0 = i * opt.max_num_features
            row = (kp[r0:r0 + counts[v]], desc[r0:r0 + counts[v]])
            if return_keys:
                k = keys[r0:r0 + counts[v]].to(torch.int64)
                p = k[:, 0] & 0xffffffff
                row += (torch.stack([p >> 30, (p >> 28) & 3, (p >> 14) & 0x3fff, p & 0x3fff, k[:, 1]], dim=1),)
            out.append(row)
            v += 1
    return out


def gaussian_levels(image, options=None):
    """debug entry: the Gaussian levels the extraction of ONE image builds -> list over octaves of float32 [6,h,w] device tensors"""
    opt = options or SiftOptions()
    dev = _lib.find_device("ls2fm.features", [image])
    return _call([_grey(image, dev)], opt, dev, debug=True)[3]


def n_views_from_images(images, intrinsic=None, options=None, **two_view_kwargs):
    """preparation/main.py:91-247 minus the mapper: extract, then ls2fm.match.two_view_tables (matcher, the < 50 filter, one
    batched two-view RANSAC, the n_views layout).  -> what two_view_tables returns: the list np.save would write as n_views.npy."""
    from . import match
    feats = extract(images, options)
    keypoints = [f[0][:, :2].cpu().numpy().astype(np.float64) for f in feats]
    return match.two_view_tables(keypoints, [f[1] for f in feats], intrinsic, **two_view_kwargs)
