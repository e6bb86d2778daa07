"""THE DISTORTION RULE and THE UNDISTORTION RULE of include/ls2fm.h restated in numpy, one numpy operation per rounded operation of
the rule, in the rule's precision: fp32 for images (ls2fm_undistort_images), fp64 for key points (ls2fm_camera_points).  The kernels
of csrc/undistort.hip and the torch forms of ls2fm.undistort are held to these bits; the rules themselves are judged on this file
(tests/test_undistort_host.py)."""
import numpy as np

F32, F64 = np.float32, np.float64
PARAMS = 12                 # LS2FM_CAMERA_PARAMS
MAX_ITERS = 32              # LS2FM_CAMERA_MAX_ITERS
DISTORT, UNDISTORT = 0, 1   # LS2FM_CAMERA_DISTORT, LS2FM_CAMERA_UNDISTORT
BILINEAR, NEAREST = 0, 1    # LS2FM_UNDISTORT_BILINEAR, LS2FM_UNDISTORT_NEAREST


def _words(cam):
    """the 12 words of cameras [..., 12] as arrays [...]"""
    return [cam[..., i] for i in range(PARAMS)]


def distort(cam, x, y):
    """(x, y) -> (xd, yd) and what the Jacobian shares (r2, den, rad); cam [..., 12] broadcasts against x; all of one dtype"""
    T = x.dtype.type
    assert cam.dtype == x.dtype == y.dtype
    one, two = T(1), T(2)
    _, _, _, _, k1, k2, p1, p2, k3, k4, k5, k6 = _words(cam)
    with np.errstate(all="ignore"):
        r2 = (x * x) + (y * y)
        num = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        den = one + r2 * (k4 + r2 * (k5 + r2 * k6))
        rad = num / den
        xy = x * y
        xd = (x * rad) + (((two * p1) * xy) + (p2 * (r2 + (two * x) * x)))
        yd = (y * rad) + ((p1 * (r2 + (two * y) * y)) + ((two * p2) * xy))
    return xd, yd, (r2, den, rad)


def to_image(cam, xd, yd):
    with np.errstate(all="ignore"):
        return (cam[..., 0] * xd) + cam[..., 2], (cam[..., 1] * yd) + cam[..., 3]


def jacobian(cam, shared, x, y):
    """J = d(xd, yd)/d(x, y) = [a b; c d]"""
    T = x.dtype.type
    two, three, six = T(2), T(3), T(6)
    r2, den, rad = shared
    _, _, _, _, k1, k2, p1, p2, k3, k4, k5, k6 = _words(cam)
    with np.errstate(all="ignore"):
        dnum = k1 + r2 * ((two * k2) + r2 * (three * k3))
        dden = k4 + r2 * ((two * k5) + r2 * (three * k6))
        g = (dnum - (rad * dden)) / den
        x2, y2 = two * x, two * y
        gx, gy = x2 * g, y2 * g
        p1_2, p2_2 = two * p1, two * p2
        a = ((rad + (x * gx)) + (p1_2 * y)) + (p2 * (six * x))
        b = ((x * gy) + (p1_2 * x)) + (p2 * y2)
        c = ((y * gx) + (p1 * x2)) + (p2_2 * y)
        d = ((rad + (y * gy)) + (p1 * (six * y))) + (p2_2 * x)
    return a, b, c, d


def views_of_rows(view_start, n):
    """per row its view (the last v with view_start[v] <= row) and whether the row belongs to any"""
    vs = np.asarray(view_start, np.int64)
    rows = np.arange(n, dtype=np.int64)
    view = np.clip(np.searchsorted(vs[:-1], rows, side="right") - 1, 0, len(vs) - 2)
    return view, (vs[view] <= rows) & (rows < vs[view + 1])


def camera_points(uv, view_start, cam, out_intr, direction, iters=10):
    """ls2fm_camera_points: uv float64 [N, 2], view_start [V + 1], cam [V, 12], out_intr [V, 4] -> (uv_out [N, 2], residual [N]);
    rows outside the views keep NaN here (the kernel does not write them)"""
    uv, cam, k = np.asarray(uv, F64), np.asarray(cam, F64), np.asarray(out_intr, F64)
    assert uv.ndim == 2 and uv.shape[1] == 2 and cam.shape[1:] == (PARAMS,) and k.shape == (cam.shape[0], 4) and 0 <= iters <= MAX_ITERS
    n = uv.shape[0]
    view, owned = views_of_rows(view_start, n)
    c, k = cam[view], k[view]
    u, v = uv[:, 0], uv[:, 1]
    with np.errstate(all="ignore"):
        if direction == DISTORT:
            x, y = (u - k[:, 2]) / k[:, 0], (v - k[:, 3]) / k[:, 1]
            xd, yd, _ = distort(c, x, y)
            ou, ov = to_image(c, xd, yd)
            res = np.zeros(n)
        else:
            assert direction == UNDISTORT
            xd, yd = (u - c[:, 2]) / c[:, 0], (v - c[:, 3]) / c[:, 1]
            x, y = xd.copy(), yd.copy()
            live = np.ones(n, bool)
            for _ in range(iters):
                fx_, fy_, shared = distort(c, x, y)
                ja, jb, jc, jd = jacobian(c, shared, x, y)
                ex, ey = fx_ - xd, fy_ - yd
                det = (ja * jd) - (jb * jc)
                live = live & (det != 0.0) & np.isfinite(det)
                x = np.where(live, x - (((jd * ex) - (jb * ey)) / det), x)
                y = np.where(live, y - (((ja * ey) - (jc * ex)) / det), y)
            fx_, fy_, _ = distort(c, x, y)
            px, py = c[:, 0] * (fx_ - xd), c[:, 1] * (fy_ - yd)
            res = (px * px) + (py * py)
            ou, ov = (k[:, 0] * x) + k[:, 2], (k[:, 1] * y) + k[:, 3]
    out = np.stack([ou, ov], axis=1)
    out[~owned] = np.nan
    return out, np.where(owned, res, np.nan)


def source_coordinates(cam, out_intr, H, W):
    """steps 1 and 2 of THE UNDISTORTION RULE: (u, v) float32 [V, H, W] of every output pixel"""
    cam, k = np.asarray(cam, F32), np.asarray(out_intr, F32)
    assert cam.shape[1:] == (PARAMS,) and k.shape == (cam.shape[0], 4)
    half = F32(0.5)
    c = cam[:, None, None, :]
    with np.errstate(all="ignore"):
        xn = ((np.arange(W, dtype=F32)[None, None, :] + half) - k[:, 2, None, None]) / k[:, 0, None, None]
        yn = ((np.arange(H, dtype=F32)[None, :, None] + half) - k[:, 3, None, None]) / k[:, 1, None, None]
        xn, yn = np.broadcast_arrays(xn, yn)
        xd, yd, _ = distort(c, np.ascontiguousarray(xn), np.ascontiguousarray(yn))
        return to_image(c, xd, yd)


def _taps(u, size):
    half = F32(0.5)
    x = u - half
    x0 = np.floor(x)
    t = x - x0
    i = x0.astype(np.int64)
    return np.clip(i, 0, size - 1), np.clip(i + 1, 0, size - 1), t


def undistort_images(images, cam, out_intr, H, W, mode=BILINEAR, fill=np.nan):
    """ls2fm_undistort_images: images float32 [V, Hs, Ws, C] -> (out float32 [V, H, W, C], valid uint8 [V, H, W])"""
    images = np.asarray(images, F32)
    V, Hs, Ws, C = images.shape
    fill = np.broadcast_to(np.asarray(fill, F32), (C,))
    u, v = source_coordinates(cam, out_intr, H, W)
    with np.errstate(all="ignore"):
        ok = (u >= F32(0)) & (u < F32(Ws)) & (v >= F32(0)) & (v < F32(Hs))
        us, vs = np.where(ok, u, F32(0.5)), np.where(ok, v, F32(0.5))
        view = np.arange(V)[:, None, None]
        if mode == BILINEAR:
            x0, x1, tx = _taps(us, Ws)
            y0, y1, ty = _taps(vs, Hs)
            tx, ty = tx[..., None], ty[..., None]
            a00, a10, a01, a11 = images[view, y0, x0], images[view, y0, x1], images[view, y1, x0], images[view, y1, x1]
            r0 = a00 + tx * (a10 - a00)
            r1 = a01 + tx * (a11 - a01)
            s = r0 + ty * (r1 - r0)
        else:
            assert mode == NEAREST
            s = images[view, np.floor(vs).astype(np.int64), np.floor(us).astype(np.int64)]
    out = np.where(ok[..., None], s, fill[None, None, None, :]).astype(F32)
    return out, ok.astype(np.uint8)
