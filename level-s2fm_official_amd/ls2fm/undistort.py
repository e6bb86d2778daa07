"""Lens-distortion camera models and image undistortion on the device: COLMAP's image_undistorter, the stage between the mapper and
the stereo.  Every other module knows the pinhole camera (fx, fy, cx, cy) alone; this one is the adapter in front of them.

A camera is 12 numbers (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6): OpenCV's rational model, COLMAP's FULL_OPENCV;
camera_from_colmap fills it from SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV and FULL_OPENCV, read_cameras_txt reads a
cameras.txt.  include/ls2fm.h states THE DISTORTION RULE and THE UNDISTORTION RULE; csrc/undistort.hip holds the two kernels,
tests/undistort_restate.py the numpy restatement, _undistort_images_torch and _camera_points_torch the rules as torch ops (the form
CPU tensors take, and the timing baseline).  All agree bit for bit.

    features.extract(photographs) -> undistort_keypoints -> match / mapper
    undistort_views(photographs, cam) -> (images, intr, valid) -> mvs.dense_reconstruct, mesh_colors.photo_colors, texture.photo_texture

Deviations from COLMAP, on purpose: no fisheye, FOV or thin-prism models (atan is not a correctly rounded operation and the rule
would lose its bits); no guard against a rational model that folds over; the scale and orientation of a key point are kept, only
its position moves; bilinear (and nearest) resampling only."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

CAMERA_PARAMS = 12          # LS2FM_CAMERA_PARAMS
CAMERA_MAX_ITERS = 32       # LS2FM_CAMERA_MAX_ITERS
CAMERA_DISTORT = 0          # LS2FM_CAMERA_DISTORT
CAMERA_UNDISTORT = 1        # LS2FM_CAMERA_UNDISTORT
CAMERA_POINTS_THREADS = 256  # LS2FM_CAMERA_POINTS_THREADS
UNDISTORT_BILINEAR = 0      # LS2FM_UNDISTORT_BILINEAR
UNDISTORT_NEAREST = 1       # LS2FM_UNDISTORT_NEAREST
UNDISTORT_TILE_W = 32       # LS2FM_UNDISTORT_TILE_W
UNDISTORT_TILE_H = 8        # LS2FM_UNDISTORT_TILE_H
MODES = {"bilinear": UNDISTORT_BILINEAR, "nearest": UNDISTORT_NEAREST}

# COLMAP's parameter order per model -> the word of the camera vector each parameter goes to; f fills fx and fy
_FX, _FY, _CX, _CY, _K1, _K2, _P1, _P2, _K3, _K4, _K5, _K6 = range(12)
_F = (_FX, _FY)
COLMAP_MODELS = {
    "SIMPLE_PINHOLE": (_F, _CX, _CY),
    "PINHOLE": (_FX, _FY, _CX, _CY),
    "SIMPLE_RADIAL": (_F, _CX, _CY, _K1),
    "RADIAL": (_F, _CX, _CY, _K1, _K2),
    "OPENCV": (_FX, _FY, _CX, _CY, _K1, _K2, _P1, _P2),
    "FULL_OPENCV": (_FX, _FY, _CX, _CY, _K1, _K2, _P1, _P2, _K3, _K4, _K5, _K6),
}
_UNSUPPORTED = ("OPENCV_FISHEYE", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE", "RAD_TAN_THIN_PRISM_FISHEYE")


# ------------------------------------------------------------------------------------------------------------------ cameras
def camera_from_colmap(model, params) -> torch.Tensor:
    """the camera vector float64 [12] of a COLMAP camera model name and its parameters in COLMAP's order"""
    name = str(model).upper()
    if name in _UNSUPPORTED:
        raise ValueError(f"ls2fm.undistort.camera_from_colmap: the model {name} is not supported: its rule needs atan, which is not a "
                         f"correctly rounded operation; supported: {', '.join(COLMAP_MODELS)}")
    if name not in COLMAP_MODELS:
        raise ValueError(f"ls2fm.undistort.camera_from_colmap: unknown camera model {model!r}; supported: {', '.join(COLMAP_MODELS)}")
    slots = COLMAP_MODELS[name]
    params = [float(p) for p in params]
    if len(params) != len(slots):
        raise ValueError(f"ls2fm.undistort.camera_from_colmap: {name} takes {len(slots)} parameters, got {len(params)}")
    cam = torch.zeros(CAMERA_PARAMS, dtype=torch.float64)
    for slot, p in zip(slots, params):
        for word in (slot if isinstance(slot, tuple) else (slot,)):
            cam[word] = p
    return cam


def read_cameras_txt(path) -> dict:
    """a cameras.txt in COLMAP's text layout, one camera per line `CAMERA_ID MODEL WIDTH HEIGHT PARAMS[]`, lines that begin with #
    and empty lines skipped -> {camera_id: dict(model=, width=, height=, cam=float64 [12])}"""
    out = {}
    with open(path) as f:
        for number, line in enumerate(f, 1):
            words = line.split()
            if not words or words[0].startswith("#"):
                continue
            if len(words) < 5:
                raise ValueError(f"{path}:{number}: expected CAMERA_ID MODEL WIDTH HEIGHT PARAMS[], got {line.strip()!r}")
            try:
                camera_id, width, height = int(words[0]), int(words[2]), int(words[3])
                cam = camera_from_colmap(words[1], words[4:])
            except ValueError as e:
                raise ValueError(f"{path}:{number}: {e}") from None
            if camera_id in out:
                raise ValueError(f"{path}:{number}: camera {camera_id} is listed twice")
            out[camera_id] = dict(model=words[1].upper(), width=width, height=height, cam=cam)
    return out


def _cameras(cam, n, dtype, dev, who):
    """cam [12] or [V, 12] -> [n, 12] of dtype on dev, contiguous (n None: as many as given)"""
    cam = torch.as_tensor(cam)
    if cam.dim() not in (1, 2) or cam.shape[-1] != CAMERA_PARAMS:
        raise ValueError(f"{who}: cam must be [12] or [V, 12], got {tuple(cam.shape)}")
    cam = cam.detach().reshape(-1, CAMERA_PARAMS).to(device=dev, dtype=dtype)
    if n is not None and cam.shape[0] not in (1, n):
        raise ValueError(f"{who}: {cam.shape[0]} cameras for {n} views")
    return cam.expand(cam.shape[0] if n is None else n, CAMERA_PARAMS).contiguous()


def _pinholes(out_intr, cam, who):
    """out_intr None (the cameras' own fx, fy, cx, cy), [4], [V, 4], [3, 3] or [V, 3, 3] -> [V, 4] like cam"""
    n = cam.shape[0]
    if out_intr is None:
        return cam[:, :4].contiguous()
    k = torch.as_tensor(out_intr).detach().to(device=cam.device, dtype=cam.dtype)
    if tuple(k.shape[-2:]) == (3, 3) and k.dim() in (2, 3):
        k = k.reshape(-1, 3, 3)
        k = torch.stack([k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2]], dim=1)
    elif k.shape[-1] == 4 and k.dim() in (1, 2):
        k = k.reshape(-1, 4)
    else:
        raise ValueError(f"{who}: out_intr must be [4], [V, 4], [3, 3] or [V, 3, 3], got {tuple(k.shape)}")
    if k.shape[0] not in (1, n):
        raise ValueError(f"{who}: {k.shape[0]} output cameras for {n} views")
    return k.expand(n, 4).contiguous()


def intrinsic_matrices(k4) -> torch.Tensor:
    """[V, 4] = (fx, fy, cx, cy) -> [V, 3, 3], what the other stages take as intr"""
    k4 = torch.as_tensor(k4)
    K = torch.zeros(k4.shape[0], 3, 3, dtype=k4.dtype, device=k4.device)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = k4[:, 0], k4[:, 1], k4[:, 2], k4[:, 3], 1.0
    return K


# ------------------------------------------------------------------------------------------------------------------ the rule as torch ops
def _distort_torch(c, x, y):
    """THE DISTORTION RULE: c the 12 words (each broadcasting against x), one torch op per rounded operation -> xd, yd, (r2, den, rad)"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = c
    r2 = (x * x) + (y * y)
    num = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    den = 1 + r2 * (k4 + r2 * (k5 + r2 * k6))
    rad = num / den
    xy = x * y
    xd = (x * rad) + (((2 * p1) * xy) + (p2 * (r2 + (2 * x) * x)))
    yd = (y * rad) + ((p1 * (r2 + (2 * y) * y)) + ((2 * p2) * xy))
    return xd, yd, (r2, den, rad)


def _jacobian_torch(c, shared, x, y):
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = c
    r2, den, rad = shared
    dnum = k1 + r2 * ((2 * k2) + r2 * (3 * k3))
    dden = k4 + r2 * ((2 * k5) + r2 * (3 * k6))
    g = (dnum - (rad * dden)) / den
    x2, y2 = 2 * x, 2 * y
    gx, gy = x2 * g, y2 * g
    p1_2, p2_2 = 2 * p1, 2 * p2
    a = ((rad + (x * gx)) + (p1_2 * y)) + (p2 * (6 * x))
    b = ((x * gy) + (p1_2 * x)) + (p2 * y2)
    cc = ((y * gx) + (p1 * x2)) + (p2_2 * y)
    d = ((rad + (y * gy)) + (p1 * (6 * y))) + (p2_2 * x)
    return a, b, cc, d


def _jacobian_k_torch(c, shared, x, y, xd, yd):
    """d(fx xd + cx, fy yd + cy)/d(the 12 words), THE CAMERA BLOCK of include/ls2fm.h -> (row u [12 tensors], row v [12 tensors])"""
    fx, fy = c[0], c[1]
    r2, den, rad = shared
    zero, one = torch.zeros_like(x), torch.ones_like(x)
    fxx, fyy, xy2 = fx * x, fy * y, 2 * (x * y)
    q1 = r2 / den
    q2 = q1 * r2
    q3 = q2 * r2
    n1, n2, n3 = 0 - (rad * q1), 0 - (rad * q2), 0 - (rad * q3)
    ju = [xd, zero, one, zero, fxx * q1, fxx * q2, fx * xy2, fx * (r2 + (2 * x) * x), fxx * q3, fxx * n1, fxx * n2, fxx * n3]
    jv = [zero, yd, zero, one, fyy * q1, fyy * q2, fy * (r2 + (2 * y) * y), fy * xy2, fyy * q3, fyy * n1, fyy * n2, fyy * n3]
    return ju, jv


def _views_of_rows(view_start, n):
    """per row its view (the last v with view_start[v] <= row) and whether the row belongs to any"""
    vs = view_start.long()
    rows = torch.arange(n, device=vs.device)
    view = (torch.searchsorted(vs[:-1].contiguous(), rows, right=True) - 1).clamp(0, vs.shape[0] - 2)
    return view, (vs[view] <= rows) & (rows < vs[view + 1])


def _camera_points_torch(uv, view_start, cam, out_intr, direction, iters):
    """ls2fm_camera_points as torch ops on whatever device the tensors are on: uv float64 [N, 2], view_start [V + 1], cam [V, 12],
    out_intr [V, 4] -> (uv_out [N, 2], residual [N]); rows outside the views are NaN"""
    n = uv.shape[0]
    view, owned = _views_of_rows(view_start, n)
    c, k = cam[view].unbind(1), out_intr[view].unbind(1)
    u, v = uv[:, 0], uv[:, 1]
    if direction == CAMERA_DISTORT:
        x, y = (u - k[2]) / k[0], (v - k[3]) / k[1]
        xd, yd, _ = _distort_torch(c, x, y)
        ou, ov = (c[0] * xd) + c[2], (c[1] * yd) + c[3]
        res = torch.zeros_like(ou)
    else:
        xd, yd = (u - c[2]) / c[0], (v - c[3]) / c[1]
        x, y = xd, yd
        live = torch.ones_like(owned)
        for _ in range(iters):
            fx_, fy_, shared = _distort_torch(c, x, y)
            ja, jb, jc, jd = _jacobian_torch(c, shared, x, y)
            ex, ey = fx_ - xd, fy_ - yd
            det = (ja * jd) - (jb * jc)
            live = live & (det != 0) & torch.isfinite(det)
            x = torch.where(live, x - (((jd * ex) - (jb * ey)) / det), x)
            y = torch.where(live, y - (((ja * ey) - (jc * ex)) / det), y)
        fx_, fy_, _ = _distort_torch(c, x, y)
        px, py = c[0] * (fx_ - xd), c[1] * (fy_ - yd)
        res = (px * px) + (py * py)
        ou, ov = (k[0] * x) + k[2], (k[1] * y) + k[3]
    nan = torch.full_like(ou, math.nan)
    return torch.stack([torch.where(owned, ou, nan), torch.where(owned, ov, nan)], dim=1), torch.where(owned, res, nan)


def _undistort_images_torch(images, cam, out_intr, H, W, mode, fill):
    """ls2fm_undistort_images as torch ops on whatever device the tensors are on: images float32 [V, Hs, Ws, C], cam [V, 12],
    out_intr [V, 4], fill a sequence of C floats -> (out float32 [V, H, W, C], valid uint8 [V, H, W])"""
    V, Hs, Ws, C = images.shape
    dev = images.device
    c = [w[:, None, None] for w in cam.unbind(1)]
    k = [w[:, None, None] for w in out_intr.unbind(1)]
    xn = ((torch.arange(W, dtype=torch.float32, device=dev)[None, None, :] + 0.5) - k[2]) / k[0]
    yn = ((torch.arange(H, dtype=torch.float32, device=dev)[None, :, None] + 0.5) - k[3]) / k[1]
    xd, yd, _ = _distort_torch(c, xn, yn)
    u, v = (c[0] * xd) + c[2], (c[1] * yd) + c[3]
    ok = (u >= 0) & (u < float(Ws)) & (v >= 0) & (v < float(Hs))
    half = torch.full_like(u, 0.5)
    us, vs = torch.where(ok, u, half), torch.where(ok, v, half)
    flat = images.reshape(V * Hs * Ws, C)
    base = (torch.arange(V, device=dev) * (Hs * Ws))[:, None, None]

    def taps(s, size):
        x = s - 0.5
        x0 = x.floor()
        i = x0.long()
        return i.clamp(0, size - 1), (i + 1).clamp(0, size - 1), (x - x0)[..., None]
    if mode == UNDISTORT_BILINEAR:
        x0, x1, tx = taps(us, Ws)
        y0, y1, ty = taps(vs, Hs)
        a00, a10 = flat[base + y0 * Ws + x0], flat[base + y0 * Ws + x1]
        a01, a11 = flat[base + y1 * Ws + x0], flat[base + y1 * Ws + x1]
        r0 = a00 + tx * (a10 - a00)
        r1 = a01 + tx * (a11 - a01)
        s = r0 + ty * (r1 - r0)
    else:
        s = flat[base + vs.floor().long() * Ws + us.floor().long()]
    bg = torch.tensor(list(fill), dtype=torch.float32, device=dev).expand(V, H, W, C)
    return torch.where(ok[..., None], s, bg).contiguous(), ok.to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ key points
def _points(uv, cam, view_start, out_intr, direction, iters, who):
    uv = torch.as_tensor(uv)
    if uv.dim() != 2 or uv.shape[1] != 2:
        raise ValueError(f"{who}: uv must be [N, 2], got {tuple(uv.shape)}")
    iters = int(iters)
    if not 0 <= iters <= CAMERA_MAX_ITERS:
        raise ValueError(f"{who}: iters {iters} must be in [0, {CAMERA_MAX_ITERS}]")
    dev, n = uv.device, int(uv.shape[0])
    if n >= 2 ** 31:
        raise ValueError(f"{who}: {n} points; at most 2^31 - 1")
    uv = uv.detach().to(torch.float64).contiguous()
    cams = _cameras(cam, None, torch.float64, dev, who)
    k4 = _pinholes(out_intr, cams, who)
    V = int(cams.shape[0])
    if view_start is None:
        if V != 1:
            raise ValueError(f"{who}: {V} cameras need view_start [V + 1]")
        vs = torch.tensor([0, n], dtype=torch.int32, device=dev)
    else:
        vs = torch.as_tensor(view_start).detach().to(device=dev, dtype=torch.int32).contiguous()
        if vs.dim() != 1 or vs.shape[0] != V + 1:
            raise ValueError(f"{who}: view_start must be [{V + 1}] for {V} cameras, got {tuple(vs.shape)}")
    if not uv.is_cuda:
        return _camera_points_torch(uv, vs, cams, k4, direction, iters)
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.full((n, 2), math.nan, dtype=torch.float64, device=dev)
        res = torch.full((n,), math.nan, dtype=torch.float64, device=dev)
        check(lib.ls2fm_camera_points(ptr(uv), n, ptr(vs), V, ptr(cams), ptr(k4), direction, iters, ptr(out), ptr(res), stream_ptr()),
              "ls2fm_camera_points")
    return out, res


@torch.no_grad()
def undistort_points(uv, cam, view_start=None, out_intr=None, iters=10):
    """Positions in the photographs as taken -> positions under the pinhole cameras out_intr (None: each camera's own fx, fy, cx,
    cy), by `iters` Newton steps of THE DISTORTION RULE's inverse.  uv [N, 2] sorted by view, view_start int [V + 1] (None: one
    view), cam [12] or [V, 12], out_intr [4], [V, 4], [3, 3] or [V, 3, 3] -> (uv float64 [N, 2], residual float64 [N]): the squared
    distance, in photograph pixels, between the point and the image of its answer; drop what did not converge by it.  Rows outside
    every view are NaN.  One launch, nothing read back; CPU tensors take the torch form."""
    return _points(uv, cam, view_start, out_intr, CAMERA_UNDISTORT, iters, "ls2fm.undistort.undistort_points")


@torch.no_grad()
def distort_points(uv, cam, view_start=None, out_intr=None):
    """Positions under the pinhole cameras out_intr -> positions in the photographs: THE DISTORTION RULE -> (uv float64 [N, 2],
    residual float64 [N] = 0).  Arguments as undistort_points."""
    return _points(uv, cam, view_start, out_intr, CAMERA_DISTORT, 0, "ls2fm.undistort.distort_points")


@torch.no_grad()
def undistort_keypoints(keypoints, counts, cam, out_intr=None, iters=10):
    """features.extract's table: keypoints float32 [V * max, 4] = x, y, scale, orientation, counts int [V] -> a table of the same
    shape whose columns 0 and 1 are the undistorted positions of the rows v max .. v max + counts[v] - 1.  Scale and orientation
    are kept (a deviation: the local warp of the lens is not applied to them), and so is every row past counts[v].  Nothing is
    read back."""
    who = "ls2fm.undistort.undistort_keypoints"
    kp, counts = torch.as_tensor(keypoints), torch.as_tensor(counts)
    V = int(counts.shape[0]) if counts.dim() == 1 else -1
    if kp.dim() != 2 or kp.shape[1] != 4 or V < 1 or kp.shape[0] % V:
        raise ValueError(f"{who}: keypoints [V * max, 4] and counts [V], got {tuple(kp.shape)} and {tuple(counts.shape)}")
    cap = int(kp.shape[0]) // V
    starts = torch.arange(V + 1, dtype=torch.int32, device=kp.device) * cap
    uv, _ = _points(kp[:, :2], _cameras(cam, V, torch.float64, kp.device, who), starts, out_intr, CAMERA_UNDISTORT, iters, who)
    live = torch.arange(cap, device=kp.device)[None, :] < counts.to(kp.device).long()[:, None]
    out = kp.clone()
    out[:, :2] = torch.where(live.reshape(-1, 1), uv.to(kp.dtype), kp[:, :2])
    return out


# ------------------------------------------------------------------------------------------------------------------ the output camera
def undistorted_intrinsics(cam, H, W, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """The pinhole camera and size of the undistorted image of one camera [12] whose photographs are H x W -> (intr float64 [4] =
    fx, fy, cx', cy', H', W').  blank_pixels = 0 keeps the largest rectangle about the principal point in which every pixel sees
    the photograph, 1 the smallest that keeps every pixel of the photograph, values between blend the two scales.  Modelled on
    COLMAP's option of the same name; no parity with it is claimed.  Host fp64 on the 2 (H + W) border pixels' centres, which
    are undistorted into the camera's own pinhole; the focal lengths are kept."""
    who = "ls2fm.undistort.undistorted_intrinsics"
    cam = _cameras(cam, 1, torch.float64, "cpu", who)[0]
    H, W, blank = int(H), int(W), float(blank_pixels)
    if H < 1 or W < 1 or not 0.0 <= blank <= 1.0 or not 0.0 < float(min_scale) <= float(max_scale):
        raise ValueError(f"{who}: H {H}, W {W} >= 1, blank_pixels {blank} in [0, 1], 0 < min_scale <= max_scale")
    ys, xs = torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5
    border = torch.cat([torch.stack([torch.full_like(ys, 0.5), ys], 1), torch.stack([torch.full_like(ys, W - 0.5), ys], 1),
                        torch.stack([xs, torch.full_like(xs, 0.5)], 1), torch.stack([xs, torch.full_like(xs, H - 0.5)], 1)])
    p, _ = undistort_points(border, cam)
    left, right, top, bottom = p[:H, 0], p[H:2 * H, 0], p[2 * H:2 * H + W, 1], p[2 * H + W:, 1]

    def axis(c, size, low, high):
        l_min, l_max, h_min, h_max = float(low.min()), float(low.max()), float(high.min()), float(high.max())
        s_min = min(c / (c - l_min), (size - 0.5 - c) / (h_max - c))
        s_max = max(c / (c - l_max), (size - 0.5 - c) / (h_min - c))
        s = 1.0 / (s_min * blank + s_max * (1.0 - blank))
        s = min(max(s, float(min_scale)), float(max_scale))
        n = max(1, int(s * size))
        return n, c * n / size
    fx, fy, cx, cy = (float(w) for w in cam[:4])
    Wn, cxn = axis(cx, W, left, right)
    Hn, cyn = axis(cy, H, top, bottom)
    return torch.tensor([fx, fy, cxn, cyn], dtype=torch.float64), Hn, Wn


# ------------------------------------------------------------------------------------------------------------------ images
def _fill(fill, C):
    """a scalar or a sequence of C floats -> C floats"""
    values = [float(fill)] * C if not hasattr(fill, "__len__") else [float(f) for f in fill]
    if len(values) != C:
        raise ValueError(f"ls2fm.undistort.undistort_images: fill has {len(values)} values for {C} channels")
    return values


@torch.no_grad()
def undistort_images(images, cam, out_intr, H, W, mode="bilinear", fill=math.nan):
    """THE UNDISTORTION RULE of include/ls2fm.h: the photographs images float32 [V, Hs, Ws, C] (or [V, Hs, Ws]), 1 <= C <= 4, taken
    by the cameras cam [12] or [V, 12], resampled under the pinhole cameras out_intr ([4], [V, 4], [3, 3] or [V, 3, 3]) at H x W ->
    (images float32 [V, H, W, C] (or [V, H, W]), valid uint8 [V, H, W]).  A pixel that does not see the photograph takes `fill` (a
    scalar or C values; NaN is what the sweep and PatchMatch treat as invalid) and valid = 0.  mode "nearest" copies the pixel
    (floor u, floor v): for depth maps and masks.  One launch, nothing read back; views in several calls leave the bits of one.
    CPU tensors take the torch form."""
    who = "ls2fm.undistort.undistort_images"
    images = torch.as_tensor(images)
    grey = images.dim() == 3
    if grey:
        images = images[..., None]
    if images.dim() != 4 or not 1 <= images.shape[3] <= 4:
        raise ValueError(f"{who}: images must be [V, Hs, Ws, C] with C from 1 to 4 or [V, Hs, Ws], got {tuple(images.shape)}")
    if mode not in MODES:
        raise ValueError(f"{who}: mode {mode!r} must be one of {', '.join(MODES)}")
    images = _lib.cf(images.detach())
    V, Hs, Ws, C = (int(s) for s in images.shape)
    H, W = int(H), int(W)
    for name, s in (("Hs", Hs), ("Ws", Ws), ("H", H), ("W", W)):
        if not 1 <= s <= 32768:
            raise ValueError(f"{who}: {name} = {s} must be in [1, 32768]")
    if V * max(Hs * Ws, H * W) >= 2 ** 40:
        raise ValueError(f"{who}: {V} views of {Hs} x {Ws} -> {H} x {W}: 2^40 pixels or more")
    dev = images.device
    cams = _cameras(cam, V, torch.float32, dev, who)
    k4 = _pinholes(out_intr, cams, who)
    values = _fill(fill, C)
    if not images.is_cuda:
        out, valid = _undistort_images_torch(images, cams, k4, H, W, MODES[mode], values)
    else:
        lib = _lib.load()
        with torch.cuda.device(dev):
            out = torch.empty((V, H, W, C), dtype=torch.float32, device=dev)
            valid = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
            check(lib.ls2fm_undistort_images(ptr(images), V, Hs, Ws, C, ptr(cams), ptr(k4), H, W, MODES[mode], (ctypes.c_float * C)(*values),
                                             ptr(out), ptr(valid), stream_ptr()), "ls2fm_undistort_images")
    return (out[..., 0] if grey else out), valid


@torch.no_grad()
def undistort_views(images, cam, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, mode="bilinear", fill=math.nan):
    """The photographs of one size [V, Hs, Ws, C] (or [V, Hs, Ws]) with their cameras cam [12] or [V, 12] -> (images [V, H', W', C],
    intr float32 [V, 3, 3], valid uint8 [V, H', W']): undistorted_intrinsics per camera (the cameras come to the host: 12 numbers
    each), then one undistort_images call at one output size.  With several cameras the size is the per-axis minimum of (H', W')
    over the views and each view keeps its own cx', cy'.  intr is what mvs.dense_reconstruct, mesh_colors.photo_colors and
    texture.photo_texture take."""
    who = "ls2fm.undistort.undistort_views"
    images = torch.as_tensor(images)
    if images.dim() not in (3, 4):
        raise ValueError(f"{who}: images must be [V, Hs, Ws, C] or [V, Hs, Ws], got {tuple(images.shape)}")
    V, Hs, Ws = (int(s) for s in images.shape[:3])
    cams = torch.as_tensor(cam).detach().to(device="cpu", dtype=torch.float64).reshape(-1, CAMERA_PARAMS)
    if cams.shape[0] not in (1, V):
        raise ValueError(f"{who}: {cams.shape[0]} cameras for {V} views")
    each = [undistorted_intrinsics(c, Hs, Ws, blank_pixels, min_scale, max_scale) for c in cams]
    H, W = min(e[1] for e in each), min(e[2] for e in each)
    k4 = torch.stack([e[0] for e in each]).to(torch.float32).expand(V, 4).contiguous()
    out, valid = undistort_images(images, cams, k4.to(images.device), H, W, mode=mode, fill=fill)
    return out, intrinsic_matrices(k4.to(images.device)), valid
