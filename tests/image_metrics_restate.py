"""The image-comparison rule of include/ls2fm.h (ls2fm_image_compare), restated in numpy tap by tap with whole-array operations.
numpy's element-wise fp64 operations round once each and never contract, so every value below is bit for bit what the kernel
computes.  The sums come in two forms: the stated tile-and-lane order (`ordered=True`) and np.sum.

Not a test module: tests/test_image_metrics_host.py and tests/test_hip_image_metrics.py import it."""
import numpy as np

WAVE = 64


def gaussian_taps(size=11, sigma=1.5):
    k = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return g / g.sum()


def uniform_taps(size=7):
    return np.full(size, 1.0 / size, dtype=np.float64)


def blur_valid(v, w, axis):
    """acc = w[0] v[0]; acc = acc + w[k] v[k], k = 1 .. n - 1, along `axis`, over the valid positions"""
    n, length = len(w), v.shape[axis] - len(w) + 1

    def tap(k):
        sl = [slice(None)] * v.ndim
        sl[axis] = slice(k, k + length)
        return v[tuple(sl)]

    w = np.asarray(w, dtype=v.dtype)
    acc = w[0] * tap(0)
    for k in range(1, n):
        acc = acc + w[k] * tap(k)
    return acc


def ssim_map(a, b, taps, c1, c2, dtype=np.float64):
    """a, b [N, H, W, C] -> [N, H - n + 1, W - n + 1, C]; dtype float32 runs the same rule in fp32 (what the rule is NOT)"""
    x, y = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    c1, c2, two = dtype(c1), dtype(c2), dtype(2.0)
    with np.errstate(all="ignore"):
        mx, my, xx, yy, xy = (blur_valid(blur_valid(v, taps, 2), taps, 1) for v in (x, y, x * x, y * y, x * y))
        vx, vy, cxy = xx - mx * mx, yy - my * my, xy - mx * my
        return ((two * mx * my + c1) * (two * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def squared_error(a, b):
    d = np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)
    with np.errstate(all="ignore"):
        return d * d


def _tile_sums(terms, on, T):
    """terms [N, h, w, C] with `on` bool [N, h, w] (h, w <= the tile grid's extent: the caller pads) -> [N] in the stated
    order: lane T ly + lx adds its channels from 0.0, uncounted terms are +0.0; xor butterfly 32 .. 1 inside each wave of 64
    lanes, the waves in index order; then the tiles in row-major order from 0.0."""
    N, h, w, C = terms.shape
    assert h % T == 0 and w % T == 0
    t = np.where(on[..., None], terms, 0.0)
    with np.errstate(all="ignore"):
        lane = np.zeros((N, h, w))
        for c in range(C):
            lane = lane + t[..., c]
        # [N, ty, ly, tx, lx] -> [N, ty, tx, ly * T + lx]
        v = lane.reshape(N, h // T, T, w // T, T).transpose(0, 1, 3, 2, 4).reshape(N, h // T, w // T, (T * T) // WAVE, WAVE)
        idx = np.arange(WAVE)
        o = WAVE // 2
        while o:
            v = v + v[..., idx ^ o]
            o //= 2
        waves = v[..., 0]
        tile = waves[..., 0]
        for k in range(1, waves.shape[-1]):
            tile = tile + waves[..., k]
        tile = tile.reshape(N, -1)
        acc = np.zeros(N)
        for k in range(tile.shape[1]):
            acc = acc + tile[:, k]
    return acc


def _pad(v, h, w):
    out = np.zeros((v.shape[0], h, w) + v.shape[3:], dtype=v.dtype)
    out[:, :v.shape[1], :v.shape[2]] = v
    return out


def compare(a, b, taps, c1, c2, mask=None, T=16, ordered=True):
    """-> dict(sse, count, ssim_sum, ssim_count [N]; ssim_map; sse_abs, ssim_abs [N]: the sums of |term|, for the bounds)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    N, H, W, C = a.shape
    n = len(taps)
    r = (n - 1) // 2
    on = np.ones((N, H, W), dtype=bool) if mask is None else np.asarray(mask) != 0
    ctr = on[:, r:H - n + 1 + r, r:W - n + 1 + r]
    se, sm = squared_error(a, b), ssim_map(a, b, taps, c1, c2)
    with np.errstate(all="ignore"):
        se_t, sm_t = np.where(on[..., None], se, 0.0), np.where(ctr[..., None], sm, 0.0)
        if ordered:
            hp, wp = -(-H // T) * T, -(-W // T) * T
            sse = _tile_sums(_pad(se, hp, wp), _pad(on, hp, wp), T)
            ssum = _tile_sums(_pad(sm, hp, wp), _pad(ctr, hp, wp), T)
        else:
            sse, ssum = se_t.reshape(N, -1).sum(axis=1), sm_t.reshape(N, -1).sum(axis=1)
        return dict(sse=sse, count=on.reshape(N, -1).sum(axis=1).astype(np.int64) * C, ssim_sum=ssum,
                    ssim_count=ctr.reshape(N, -1).sum(axis=1).astype(np.int64) * C, ssim_map=sm,
                    sse_abs=np.abs(se_t).reshape(N, -1).sum(axis=1), ssim_abs=np.abs(sm_t).reshape(N, -1).sum(axis=1))


def sum_bound(count, abs_sum):
    """|fl(sum) - sum| <= (count + 16) 2^-53 sum |term| for any order of `count` additions (the bound the ICP tests use)"""
    return (np.asarray(count, dtype=np.float64) + 16.0) * 2.0 ** -53 * np.asarray(abs_sum)
