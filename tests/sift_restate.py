"""Numpy restatement of ls2fm.features (include/ls2fm.h, "SIFT feature extraction"): VLFeat-style DoG SIFT with COLMAP's default
options, written from the published algorithm for this project.  It is the checker of csrc/sift.hip, NOT COLMAP or OpenCV, and
claims no bit parity with either.  Every function takes `dtype` (np.float32 or np.float64): the float32 run follows the device's
order of operations where the header fixes one (the blur, the quadratic fit), the float64 run is the reference, and the gap
between the two is the yardstick of the GPU tests.

Coordinates: inside an octave o a pixel is (x, y) with integer centres; one octave pixel is 2^o input pixels and octave pixel 0
sits on input pixel 0.  Output keypoints add COLMAP's half pixel: x_out = x * 2^o + 0.5.
"""
import numpy as np

S = 3                          # octave_resolution
N_LEVELS = S + 3               # Gaussian levels s = -1 .. S + 1 at index l = s + 1
SIGMA0 = 1.6 * 2.0 ** (1.0 / S)
SIGMA_N = 0.5                  # nominal blur of the input
MIN_SIDE = 8                   # an octave smaller than this on a side is not built
TWO_PI = 2.0 * np.pi
# descriptor bin order: VLFeat's index 8 (4 by + bx) + t  ->  UBC's 8 (4 by + bx) + (8 - t) % 8   (COLMAP stores UBC)
UBC_FROM_VLFEAT = np.array([8 * c + (8 - t) % 8 for c in range(16) for t in range(8)], dtype=np.int64)

DEFAULTS = dict(first_octave=-1, num_octaves=4, peak_threshold=0.02 / S, edge_threshold=10.0, max_num_features=8192,
                max_num_orientations=2, upright=False, normalization="l1_root")


def to_grey(image):
    """float32 [H,W] in [0,1] from float / uint8, grey or RGB (Rec.709 weights)"""
    a = np.asarray(image)
    if a.dtype == np.uint8:
        a = a.astype(np.float32) / np.float32(255.0)
    a = a.astype(np.float32)
    if a.ndim == 3:
        a = (np.float32(0.2126) * a[..., 0] + np.float32(0.7152) * a[..., 1]) + np.float32(0.0722) * a[..., 2]
    return np.ascontiguousarray(a)


def gaussian_taps(sigma):
    """normalised taps of radius ceil(4 sigma), computed in float64 (the device receives them rounded to float32)"""
    r = int(np.ceil(4.0 * sigma))
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 * (k / sigma) ** 2)
    return g / g.sum()


def blur(img, sigma, dtype):
    """rows (along x) then columns, edge replication; taps summed from -r to r, one multiply and one add each"""
    w = gaussian_taps(sigma).astype(dtype)
    r = (len(w) - 1) // 2
    H, W = img.shape
    p = np.pad(img, ((0, 0), (r, r)), mode="edge")
    acc = np.zeros((H, W), dtype=dtype)
    for k in range(2 * r + 1):
        acc = acc + w[k] * p[:, k:k + W]
    p = np.pad(acc, ((r, r), (0, 0)), mode="edge")
    out = np.zeros((H, W), dtype=dtype)
    for k in range(2 * r + 1):
        out = out + w[k] * p[k:k + H, :]
    return out


def upsample2(img, dtype):
    """2x by linear interpolation between neighbours, the last row and column repeated"""
    H, W = img.shape
    half = dtype(0.5)
    right = np.concatenate([img[:, 1:], img[:, -1:]], axis=1)
    wide = np.empty((H, 2 * W), dtype=dtype)
    wide[:, 0::2] = img
    wide[:, 1::2] = half * (img + right)
    below = np.concatenate([wide[1:], wide[-1:]], axis=0)
    out = np.empty((2 * H, 2 * W), dtype=dtype)
    out[0::2] = wide
    out[1::2] = half * (wide + below)
    return out


def level_sigmas():
    """blur of level l = s + 1 in octave pixels"""
    return [SIGMA0 * 2.0 ** ((l - 1) / S) for l in range(N_LEVELS)]


def step_sigmas(first_octave):
    """the blur applied to reach each level: [first level of the first octave from the base] + [level l from l - 1]"""
    sg = level_sigmas()
    base = SIGMA_N * 2.0 ** (-first_octave)
    return [np.sqrt(sg[0] ** 2 - base ** 2)] + [np.sqrt(sg[l] ** 2 - sg[l - 1] ** 2) for l in range(1, N_LEVELS)]


def scale_space(image, first_octave=-1, num_octaves=4, dtype=np.float64):
    """-> list over octaves of Gaussian levels [6,h,w]; octave k has o = first_octave + k"""
    img = to_grey(image).astype(dtype)
    base = upsample2(img, dtype) if first_octave == -1 else img
    steps = step_sigmas(first_octave)
    octaves = []
    for k in range(num_octaves):
        if k == 0:
            cur = blur(base, steps[0], dtype)
        else:
            cur = octaves[-1][S][0::2, 0::2][:octaves[-1].shape[1] // 2, :octaves[-1].shape[2] // 2]     # level s = S - 1: twice the first level's blur
        if min(cur.shape) < MIN_SIDE:
            break
        levels = [cur]
        for l in range(1, N_LEVELS):
            levels.append(blur(levels[-1], steps[l], dtype))
        octaves.append(np.stack(levels))
    return octaves


def _fit(D, d, y, x, dtype):
    """the 3-D quadratic fit at DoG index d (arrays of candidates) -> offsets b [3,n] (x, y, s), value, Dxx, Dyy, Dxy"""
    half, quarter = dtype(0.5), dtype(0.25)
    at = lambda dx, dy, ds: D[d + ds, y + dy, x + dx]       # noqa: E731
    v0 = at(0, 0, 0)
    Dx = half * (at(1, 0, 0) - at(-1, 0, 0))
    Dy = half * (at(0, 1, 0) - at(0, -1, 0))
    Ds = half * (at(0, 0, 1) - at(0, 0, -1))
    two = v0 + v0
    Dxx = (at(1, 0, 0) + at(-1, 0, 0)) - two
    Dyy = (at(0, 1, 0) + at(0, -1, 0)) - two
    Dss = (at(0, 0, 1) + at(0, 0, -1)) - two
    Dxy = quarter * ((at(1, 1, 0) + at(-1, -1, 0)) - (at(-1, 1, 0) + at(1, -1, 0)))
    Dxs = quarter * ((at(1, 0, 1) + at(-1, 0, -1)) - (at(-1, 0, 1) + at(1, 0, -1)))
    Dys = quarter * ((at(0, 1, 1) + at(0, -1, -1)) - (at(0, -1, 1) + at(0, 1, -1)))
    c00 = Dyy * Dss - Dys * Dys
    c01 = Dxs * Dys - Dxy * Dss
    c02 = Dxy * Dys - Dxs * Dyy
    c11 = Dxx * Dss - Dxs * Dxs
    c12 = Dxy * Dxs - Dxx * Dys
    c22 = Dxx * Dyy - Dxy * Dxy
    det = (Dxx * c00 + Dxy * c01) + Dxs * c02
    ok = det != 0
    safe = np.where(ok, det, dtype(1.0))
    zero = dtype(0.0)
    b0 = np.where(ok, -(((c00 * Dx + c01 * Dy) + c02 * Ds) / safe), zero)
    b1 = np.where(ok, -(((c01 * Dx + c11 * Dy) + c12 * Ds) / safe), zero)
    b2 = np.where(ok, -(((c02 * Dx + c12 * Dy) + c22 * Ds) / safe), zero)
    val = v0 + half * ((Dx * b0 + Dy * b1) + Ds * b2)
    return b0, b1, b2, val, Dxx, Dyy, Dxy


def detect(levels, peak_threshold, edge_threshold, dtype):
    """accepted keypoints of one octave -> dict of arrays: level (0..S-1), ycell, xcell (the extremum's cell), x, y, s (refined,
    octave units), in rising (level, ycell, xcell)"""
    D = levels[1:] - levels[:-1]                                   # DoG index d <-> s = d - 1
    nd, h, w = D.shape
    c = D[1:-1, 1:-1, 1:-1]
    is_max = np.ones(c.shape, dtype=bool)
    is_min = np.ones(c.shape, dtype=bool)
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if ds == 0 and dy == 0 and dx == 0:
                    continue
                n = D[1 + ds:nd - 1 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                is_max &= c > n
                is_min &= c < n
    cand = (is_max | is_min) & (np.abs(c) > dtype(0.8 * peak_threshold))
    d0, y0, x0 = np.nonzero(cand)                                  # rising (d, y, x)
    d0, y0, x0 = d0 + 1, y0 + 1, x0 + 1
    n = len(d0)
    x, y = x0.copy(), y0.copy()
    live = np.ones(n, dtype=bool)
    out = [np.zeros(n, dtype=dtype) for _ in range(7)]
    for rnd in range(5):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        res = _fit(D, d0[idx], y[idx], x[idx], dtype)
        for o, r in zip(out, res):
            o[idx] = r
        b0, b1 = res[0], res[1]
        dx = ((b0 > dtype(0.6)) & (x[idx] < w - 2)).astype(np.int64) - ((b0 < dtype(-0.6)) & (x[idx] > 1)).astype(np.int64)
        dy = ((b1 > dtype(0.6)) & (y[idx] < h - 2)).astype(np.int64) - ((b1 < dtype(-0.6)) & (y[idx] > 1)).astype(np.int64)
        move = ((dx != 0) | (dy != 0)) & (rnd < 4)                 # the fifth fit is used where it stands
        x[idx] += np.where(move, dx, 0)
        y[idx] += np.where(move, dy, 0)
        live[idx] = move
    b0, b1, b2, val, Dxx, Dyy, Dxy = out
    xn = x.astype(dtype) + b0
    yn = y.astype(dtype) + b1
    sn = (d0 - 1).astype(dtype) + b2
    r = dtype(edge_threshold)
    tr = Dxx + Dyy
    det2 = Dxx * Dyy - Dxy * Dxy
    lim = dtype(1.5)
    si = np.floor(sn + dtype(0.5))
    good = (np.abs(b0) < lim) & (np.abs(b1) < lim) & (np.abs(b2) < lim) & (np.abs(val) > dtype(peak_threshold)) \
        & (det2 > 0) & ((tr * tr) * r < ((r + dtype(1.0)) * (r + dtype(1.0))) * det2) \
        & (xn >= 0) & (xn <= dtype(w - 1)) & (yn >= 0) & (yn <= dtype(h - 1)) & (si >= 0) & (si <= S - 1)
    g = np.nonzero(good)[0]
    return dict(level=d0[g] - 1, ycell=y0[g], xcell=x0[g], x=xn[g], y=yn[g], s=sn[g], si=si[g].astype(np.int64))


def _gradient_window(L, xi, yi, W, dtype):
    """samples of the (2W+1)^2 window around (xi, yi) clipped to the interior 1 .. w-2 / 1 .. h-2 -> xs, ys, modulus, angle"""
    h, w = L.shape
    ys = np.arange(max(-W, 1 - yi), min(W, h - 2 - yi) + 1)
    xs = np.arange(max(-W, 1 - xi), min(W, w - 2 - xi) + 1)
    if ys.size == 0 or xs.size == 0:
        z = np.zeros(0, dtype=dtype)
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), z, z
    yy, xx = np.meshgrid(yi + ys, xi + xs, indexing="ij")
    yy, xx = yy.ravel(), xx.ravel()
    gx = dtype(0.5) * (L[yy, xx + 1] - L[yy, xx - 1])
    gy = dtype(0.5) * (L[yy + 1, xx] - L[yy - 1, xx])
    mod = np.sqrt(gx * gx + gy * gy)
    ang = np.arctan2(gy, gx)
    ang = np.where(ang < 0, ang + dtype(TWO_PI), ang)
    return xx, yy, mod, ang


def orientations(L, x, y, sigma_oct, max_num, dtype):
    """angles of one keypoint at its nearest level L (octave units) -> list of at most max_num angles in bin order"""
    sw = dtype(1.5) * sigma_oct
    W = max(int(np.floor(dtype(3.0) * sw)), 1)
    xi, yi = int(np.floor(x + dtype(0.5))), int(np.floor(y + dtype(0.5)))
    xx, yy, mod, ang = _gradient_window(L, xi, yi, W, dtype)
    dx = xx.astype(dtype) - x
    dy = yy.astype(dtype) - y
    r2 = dx * dx + dy * dy
    keep = r2 < dtype(W * W) + dtype(0.6)
    wgt = np.exp(-(r2 / (dtype(2.0) * sw * sw))) * mod
    fbin = ang * dtype(36.0 / TWO_PI)
    b = np.floor(fbin - dtype(0.5))
    rb = (fbin - b) - dtype(0.5)
    bi = b.astype(np.int64)
    lo = (wgt * (dtype(1.0) - rb)).astype(dtype)[keep]
    hi = (wgt * rb).astype(dtype)[keep]
    # the bins are summed exactly (the device: 2^-40 fixed point, so in any order), then rounded once
    hist = np.bincount((bi[keep] + 36) % 36, weights=lo, minlength=36) + np.bincount((bi[keep] + 1) % 36, weights=hi, minlength=36)
    hist = hist.astype(dtype)
    third = dtype(1.0 / 3.0)
    for _ in range(6):
        hist = ((np.roll(hist, 1) + hist) + np.roll(hist, -1)) * third
    top = hist.max()
    out = []
    for i in range(36):
        h0, hm, hp = hist[i], hist[(i + 35) % 36], hist[(i + 1) % 36]
        if h0 > dtype(0.8) * top and h0 > hm and h0 > hp:
            di = dtype(-0.5) * (hp - hm) / ((hp + hm) - (h0 + h0))
            out.append(dtype(TWO_PI / 36.0) * ((dtype(i) + di) + dtype(0.5)))
            if len(out) == max_num:
                break
    return out


def descriptor_float(L, x, y, sigma_oct, angle, dtype):
    """the 128 floats in VLFeat's order (t + 8 bx + 32 by) after L2-normalise, clamp at 0.2, L2-normalise"""
    sbp = dtype(3.0) * sigma_oct
    W = int(np.floor(dtype(np.sqrt(2.0) * 2.5) * sbp + dtype(0.5)))
    xi, yi = int(np.floor(x + dtype(0.5))), int(np.floor(y + dtype(0.5)))
    xx, yy, mod, ang = _gradient_window(L, xi, yi, W, dtype)
    ct, st = np.cos(angle), np.sin(angle)
    dx = xx.astype(dtype) - x
    dy = yy.astype(dtype) - y
    th = ang - angle
    th = np.where(th < 0, th + dtype(TWO_PI), th)
    th = np.where(th >= dtype(TWO_PI), th - dtype(TWO_PI), th)
    nx = (ct * dx + st * dy) / sbp
    ny = (ct * dy - st * dx) / sbp
    nt = th * dtype(8.0 / TWO_PI)
    win = np.exp(-((nx * nx + ny * ny) / dtype(8.0))) * mod          # window of 2 bins: 2 * 2^2 = 8
    bx, by, bt = np.floor(nx - dtype(0.5)), np.floor(ny - dtype(0.5)), np.floor(nt)
    rx, ry, rt = (nx - bx) - dtype(0.5), (ny - by) - dtype(0.5), nt - bt
    bxi, byi, bti = bx.astype(np.int64), by.astype(np.int64), bt.astype(np.int64)
    acc = np.zeros(128, dtype=np.float64)
    one = dtype(1.0)
    for ex in (0, 1):
        wx = rx if ex else one - rx
        for ey in (0, 1):
            wy = ry if ey else one - ry
            for et in (0, 1):
                wt = rt if et else one - rt
                cx, cy = bxi + ex, byi + ey
                ok = (cx >= -2) & (cx < 2) & (cy >= -2) & (cy < 2)
                v = (((win * wx) * wy) * wt).astype(dtype)
                acc += np.bincount(((bti[ok] + et) % 8) + 8 * (cx[ok] + 2) + 32 * (cy[ok] + 2), weights=v[ok], minlength=128)
    d = acc.astype(dtype)
    n = np.sqrt((d * d).sum(dtype=dtype))
    d = d / np.maximum(n, dtype(1e-30))
    d = np.minimum(d, dtype(0.2))
    n = np.sqrt((d * d).sum(dtype=dtype))
    return d / np.maximum(n, dtype(1e-30))


def quantise(d, normalization, dtype):
    """COLMAP's L1_ROOT (or L2), 512 v rounded half up, capped at 255, in UBC order"""
    if normalization == "l1_root":
        v = np.sqrt(d / np.maximum(d.sum(dtype=dtype), dtype(1e-30)))
    elif normalization == "l2":
        v = d / np.maximum(np.sqrt((d * d).sum(dtype=dtype)), dtype(1e-30))
    else:
        raise ValueError(normalization)
    q = np.minimum(np.floor(dtype(512.0) * v + dtype(0.5)), dtype(255.0)).astype(np.uint8)
    out = np.zeros(128, dtype=np.uint8)
    out[UBC_FROM_VLFEAT] = q
    return out


def extract(image, dtype=np.float64, **options):
    """-> dict(keypoints float [n,4] (x, y, scale, orientation), descriptors uint8 [n,128], keys int64 [n,5] (octave index,
    level, ycell, xcell, orientation index), levels (the Gaussian levels per octave))"""
    o = dict(DEFAULTS)
    o.update(options)
    octs = scale_space(image, o["first_octave"], o["num_octaves"], dtype)
    rows, keys, descs = [], [], []
    for k, levels in enumerate(octs):
        step = dtype(2.0 ** (o["first_octave"] + k))
        det = detect(levels, o["peak_threshold"], o["edge_threshold"], dtype)
        for i in range(len(det["x"])):
            x, y, s = det["x"][i], det["y"][i], det["s"][i]
            sigma_oct = dtype(SIGMA0) * np.exp2(s / dtype(S))
            L = levels[det["si"][i] + 1]
            angles = [dtype(0.0)] if o["upright"] else orientations(L, x, y, sigma_oct, o["max_num_orientations"], dtype)
            for a, ang in enumerate(angles):
                rows.append([x * step + dtype(0.5), y * step + dtype(0.5), sigma_oct * step, ang])
                keys.append([k, det["level"][i], det["ycell"][i], det["xcell"][i], a])
                descs.append(quantise(descriptor_float(L, x, y, sigma_oct, ang, dtype), o["normalization"], dtype))
    kp = np.array(rows, dtype=dtype).reshape(-1, 4)
    keys = np.array(keys, dtype=np.int64).reshape(-1, 5)
    descs = np.array(descs, dtype=np.uint8).reshape(-1, 128)
    return cap_rows(dict(keypoints=kp, descriptors=descs, keys=keys, levels=octs), o["max_num_features"])


def cap_rows(result, cap):
    """the cap, the last step of `extract`: above `cap` rows the largest scales are kept, ties by the output order, order preserved"""
    kp = result["keypoints"]
    if len(kp) <= cap:
        return result
    order = np.lexsort((np.arange(len(kp)), -kp[:, 2]))
    keep = np.sort(order[:cap])
    return dict(keypoints=kp[keep], descriptors=result["descriptors"][keep], keys=result["keys"][keep], levels=result["levels"])


def pair_rows(keys_a, keys_b):
    """rows of a and b with the same key -> (index into a, index into b)"""
    index = {tuple(k): i for i, k in enumerate(keys_b.tolist())}
    ia = [i for i, k in enumerate(keys_a.tolist()) if tuple(k) in index]
    ib = [index[tuple(keys_a[i].tolist())] for i in ia]
    return np.array(ia, dtype=np.int64), np.array(ib, dtype=np.int64)


def gaps(a, b):
    """two extractions of one image -> dict of the worst differences (the yardstick's entries) and the unpaired share"""
    ia, ib = pair_rows(a["keys"], b["keys"])
    ka, kb = a["keypoints"][ia].astype(np.float64), b["keypoints"][ib].astype(np.float64)
    dth = np.abs(ka[:, 3] - kb[:, 3])
    dth = np.minimum(dth, TWO_PI - dth)
    n = max(len(a["keys"]), len(b["keys"]), 1)
    return dict(
        level=[[float(np.abs(la.astype(np.float64) - lb.astype(np.float64)).max()) for la, lb in zip(oa, ob)] for oa, ob in zip(a["levels"], b["levels"])],
        x=float(np.abs(ka[:, 0] - kb[:, 0]).max(initial=0.0)), y=float(np.abs(ka[:, 1] - kb[:, 1]).max(initial=0.0)),
        scale=float(np.abs(ka[:, 2] - kb[:, 2]).max(initial=0.0)), orientation=float(dth.max(initial=0.0)),
        descriptor=int(np.abs(a["descriptors"][ia].astype(np.int64) - b["descriptors"][ib].astype(np.int64)).max(initial=0)),
        unpaired=max(len(a["keys"]) - len(ia), len(b["keys"]) - len(ib)) / n, paired=len(ia), n_a=len(a["keys"]), n_b=len(b["keys"]))


def quarter_turn(keypoints, width):
    """keypoints of an image [H, width] -> where np.rot90(image) (a quarter turn counter-clockwise, out[i, j] = image[j, width - 1 - i])
    carries them.  The pixel of row r and column c goes to row width - 1 - c and column r; with x = c + 0.5 and y = r + 0.5 that is
    (x, y) -> (y, width - x).  A direction (dx, dy) goes to (dy, -dx), and so does the gradient (d out / dx' = d image / dy,
    d out / dy' = -d image / dx): an angle t measured from +x towards +y becomes t - pi / 2.  Scales stay."""
    k = np.asarray(keypoints, dtype=np.float64)
    return np.stack([k[:, 1], width - k[:, 0], k[:, 2], np.mod(k[:, 3] - 0.5 * np.pi, TWO_PI)], axis=1)


def quarter_turn_check(kp, desc, kp_turned, desc_turned, width):
    """rows of an image against the rows of np.rot90(image): every row is mapped through the turn and paired with the nearest
    turned row in (position, scale), mutually; a pair counts when it lies within half a pixel, a sixth of an octave in scale and
    0.1 rad (peaks of one histogram are at least two bins, 0.35 rad, apart: a row whose histogram has two peaks above 0.8 keeps
    the first in BIN order, which a turn by nine bins changes, and such rows do not pair).
    -> dict(share = pairs / max(rows), paired (indices), x, y, scale, orientation, descriptor: the worst differences over the pairs)"""
    m, t = quarter_turn(kp, width), np.asarray(kp_turned, dtype=np.float64)
    n = max(len(m), len(t), 1)
    if len(m) == 0 or len(t) == 0:
        return dict(share=0.0, paired=np.zeros(0, dtype=np.int64), x=0.0, y=0.0, scale=0.0, orientation=0.0, descriptor=0)
    d = np.hypot(m[:, None, 0] - t[None, :, 0], m[:, None, 1] - t[None, :, 1]) + np.abs(m[:, None, 2] - t[None, :, 2])
    j = d.argmin(axis=1)
    mutual = d.argmin(axis=0)[j] == np.arange(len(m))
    dth = np.abs(m[:, 3] - t[j, 3])
    dth = np.minimum(dth, TWO_PI - dth)
    ok = mutual & (np.hypot(m[:, 0] - t[j, 0], m[:, 1] - t[j, 1]) < 0.5) & (np.abs(np.log2(m[:, 2] / t[j, 2])) < 1.0 / 6.0) & (dth < 0.1)
    i = np.nonzero(ok)[0]
    j = j[i]
    return dict(share=len(i) / n, paired=i, x=float(np.abs(m[i, 0] - t[j, 0]).max(initial=0.0)), y=float(np.abs(m[i, 1] - t[j, 1]).max(initial=0.0)),
                scale=float(np.abs(m[i, 2] - t[j, 2]).max(initial=0.0)), orientation=float(dth[i].max(initial=0.0)),
                descriptor=int(np.abs(np.asarray(desc)[i].astype(np.int64) - np.asarray(desc_turned)[j].astype(np.int64)).max(initial=0)))
