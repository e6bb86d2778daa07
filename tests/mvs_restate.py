"""THE SWEEP RULE and THE CONSISTENCY RULE of include/ls2fm.h (ls2fm_mvs_sweep, ls2fm_mvs_filter) restated in plain numpy for this
project: float32 arrays over the pixels of one reference view, the references, planes, sources and window taps in loops, so that
every fp32 operation rounds once, in the order the header gives.  The camera point, projection and usable rule are
raster_restate's.  Test infrastructure only."""
import numpy as np

import raster_restate as R

F32 = np.float32
NAN = F32(np.nan)


def compose(pa, pb):
    """P_a o P_b^-1 of float64 [..., 3, 4] arrays, elementwise in the order ls2fm.mvs.relative_poses states"""
    Ra, ta, Rb, tb = pa[..., :3], pa[..., 3], pb[..., :3], pb[..., 3]
    p = Ra[..., :, None, :] * Rb[..., None, :, :]
    Rm = (p[..., 0] + p[..., 1]) + p[..., 2]
    q = Rm * tb[..., None, :]
    t = ta - ((q[..., 0] + q[..., 1]) + q[..., 2])
    return np.concatenate([Rm, t[..., None]], axis=-1)


def relative_poses(poses, refs, sources, back=False):
    """float32 [R, S, 3, 4]: P_s o P_r^-1 (back: P_r o P_s^-1) in float64, rounded once"""
    P = np.asarray(poses, F32).reshape(-1, 3, 4).astype(np.float64)
    V = len(P)
    refs = np.asarray(refs, np.int64).reshape(-1)
    sources = np.asarray(sources, np.int64).reshape(len(refs), -1)
    Pr, Ps = P[np.clip(refs, 0, V - 1)][:, None], P[np.clip(sources, 0, V - 1)]
    with np.errstate(all="ignore"):
        return (compose(Pr, Ps) if back else compose(Ps, Pr)).astype(F32)


def taps(Z, w):
    """the (2 w + 1)^2 shifted copies of Z [H, W], dy outer and dx inner; a tap outside the image reads NaN"""
    H, W = Z.shape
    pad = np.full((H + 2 * w, W + 2 * w), NAN, F32)
    pad[w:w + H, w:w + W] = Z
    return [pad[i:i + H, j:j + W] for i in range(2 * w + 1) for j in range(2 * w + 1)]


def window(Z, w, picked=None):
    """per pixel of Z [H, W]: the window's taps (every one, or those at the places `picked` of taps), whether all are finite
    (False where the pixel has no window), their sum in tap order"""
    t = taps(Z, w)
    if picked is not None:
        t = [t[i] for i in picked]
    total, finite = np.zeros(Z.shape, F32), np.ones(Z.shape, bool)
    for a in t:
        total = total + a
        finite &= np.isfinite(a)
    assert total.dtype == F32
    return t, finite, total


def window_stats(Z, w, picked=None):
    """step 1 per pixel of the reference Z: the taps a, whether all are finite, ma and va over them"""
    a, finite, sa = window(Z, w, picked)
    ma = sa / F32(len(a))
    va = np.zeros(Z.shape, F32)
    for t in a:
        va = va + (t - ma) * (t - ma)
    assert va.dtype == F32
    return a, finite, ma, va


def lift(k4, H, W):
    """xn float32 [1, W], yn float32 [H, 1] of the pixel centres"""
    fx, fy, cx, cy = (F32(t) for t in k4)
    xn = ((np.arange(W).astype(F32) + F32(0.5)) - cx) / fx
    yn = ((np.arange(H).astype(F32) + F32(0.5)) - cy) / fy
    assert xn.dtype == F32
    return xn[None, :], yn[:, None]


def sample(src, P, k4, X, Y, Z, near, stats=None):
    """steps 2 and 3 for the camera points (X, Y, Z) of the reference, float32 [N] each: b float32 [N], NaN where not valid"""
    H, W = src.shape
    if H < 2 or W < 2:
        return np.full(len(X), NAN, F32)
    cz, u, v, usable = R.project(np.stack([X, Y, Z], axis=1), P, k4, near)
    x, y = u - F32(0.5), v - F32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    tx, ty = x - x0, y - y0
    inside = (x0 >= 0) & (x0 <= F32(W - 2)) & (y0 >= 0) & (y0 <= F32(H - 2))
    ok = usable & inside
    ix, iy = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
    b00, b10, b01, b11 = src[iy, ix], src[iy, ix + 1], src[iy + 1, ix], src[iy + 1, ix + 1]
    r0 = b00 + tx * (b10 - b00)
    r1 = b01 + tx * (b11 - b01)
    b = r0 + ty * (r1 - r0)
    assert b.dtype == F32 and tx.dtype == F32
    if stats is not None:
        note = lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(np.count_nonzero(m)))
        yin, xin = usable & (y0 >= 0) & (y0 <= F32(H - 2)), usable & (x0 >= 0) & (x0 <= F32(W - 2))
        note("x0 == 0", yin & (x0 == 0))
        note("x0 == -1", yin & (x0 == -1))
        note("x0 + 1 == W - 1", yin & (x0 == F32(W - 2)))
        note("x0 + 1 == W", yin & (x0 == F32(W - 1)))
        note("y0 == 0", xin & (y0 == 0))
        note("y0 == -1", xin & (y0 == -1))
        note("y0 + 1 == H - 1", xin & (y0 == F32(H - 2)))
        note("y0 + 1 == H", xin & (y0 == F32(H - 1)))
        note("c_z == near", inside & (cz == F32(near)))
        note("plane behind the source", cz < 0)
        note("c_z is NaN", np.isnan(cz))
        note("source sample not finite", ok & ~np.isfinite(b))
    return np.where(ok & np.isfinite(b), b, NAN)


def warp_sample(src, P, k4, xn, yn, d, near, stats=None):
    """steps 2 and 3 for every pixel of the reference as a tap on the fronto-parallel plane d: b float32 [H, W]"""
    H, W = src.shape
    X = np.broadcast_to(xn * d, (H, W)).reshape(-1)
    Y = np.broadcast_to(yn * d, (H, W)).reshape(-1)
    return sample(src, P, k4, X, Y, np.full(H * W, d, F32), near, stats).reshape(H, W)


def sweep(images, poses, intr, sources, depths, refs=None, half_width=3, near=1e-3, min_var=1e-6, min_sources=1, stats=None,
          return_scores=False):
    """-> depth float32 [R, H, W], score float32 [R, H, W], plane int32 [R, H, W]; with return_scores also every plane's score
    float32 [R, D, H, W].  stats: a dict that collects, by name, how often each edge of the rule was met"""
    img = np.asarray(images, F32)
    V, H, W = img.shape
    refs = np.arange(V) if refs is None else np.asarray(refs, np.int64).reshape(-1)
    sources = np.asarray(sources, np.int64).reshape(len(refs), -1)
    depths = np.asarray(depths, F32)
    depths = np.broadcast_to(depths, (len(refs), depths.shape[-1]))
    Rn, D, w = len(refs), depths.shape[1], int(half_width)
    k4 = R.intr4(intr, V)
    rel = relative_poses(poses, refs, sources)
    n, mv = F32((2 * w + 1) ** 2), F32(min_var)
    out_d, out_s = np.full((Rn, H, W), NAN, F32), np.full((Rn, H, W), NAN, F32)
    out_k = np.full((Rn, H, W), -1, np.int32)
    all_scores = np.full((Rn, D, H, W), NAN, F32)
    note = (lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(np.count_nonzero(m)))) if stats is not None else None
    yy, xx = np.mgrid[0:H, 0:W]
    has_window = (xx >= w) & (xx <= W - 1 - w) & (yy >= w) & (yy <= H - 1 - w)
    with np.errstate(all="ignore"):
        for r in range(Rn):
            rv = int(refs[r])
            if not 0 <= rv < V:
                continue
            # 1. reference window
            a, a_finite, ma, va = window_stats(img[rv], w)
            assert not (a_finite & ~has_window).any()
            pixel_ok = has_window & a_finite & ~(va < mv)
            if note:
                note("reference tap not finite", has_window & ~a_finite)
                note("va == min_var", has_window & a_finite & (va == mv))
                note("va one ulp below min_var", has_window & a_finite & (va == np.nextafter(mv, F32(-np.inf))))
            xn, yn = lift(k4[rv], H, W)
            scores = all_scores[r]
            for k in range(D):
                d = depths[r, k]
                total, count = np.zeros((H, W), F32), np.zeros((H, W), np.int64)
                for s in range(sources.shape[1]):
                    sv = int(sources[r, s])
                    if not 0 <= sv < V:
                        if note:
                            note("source skipped", 1)
                        continue
                    if note:
                        note("a view is reference and source", np.isin(sv, refs))
                    # 2. warp, 3. sample
                    b = warp_sample(img[sv], rel[r, s], k4[sv], xn, yn, d, near, stats)
                    # 4. NCC
                    bt, b_finite, sb = window(b, w)
                    mb = sb / n
                    vb, cov = np.zeros((H, W), F32), np.zeros((H, W), F32)
                    for ai, bi in zip(a, bt):
                        vb = vb + (bi - mb) * (bi - mb)
                        cov = cov + (ai - ma) * (bi - mb)
                    valid = pixel_ok & b_finite & ~(vb < mv)
                    ncc = cov / np.sqrt(va * vb)
                    assert ncc.dtype == F32 and cov.dtype == F32
                    if note:
                        note("vb == min_var", pixel_ok & b_finite & (vb == mv))
                        note("vb one ulp below min_var", pixel_ok & b_finite & (vb == np.nextafter(mv, F32(-np.inf))))
                        note("source window not valid", pixel_ok & ~b_finite)
                    total = np.where(valid, total + ncc, total)
                    count += valid
                # 5. aggregate
                scores[k] = np.where(count >= int(min_sources), total / count.astype(F32), NAN)
                if note:
                    note("count == min_sources - 1", pixel_ok & (count == int(min_sources) - 1))
            # 6. select: the largest score, the lowest k among equals, never a NaN
            best, best_k = np.full((H, W), NAN, F32), np.full((H, W), -1, np.int64)
            for k in range(D):
                better = ~np.isnan(scores[k]) & ((best_k < 0) | (scores[k] > best))
                if note:
                    note("tie goes to the lower plane", ~np.isnan(scores[k]) & (best_k >= 0) & (scores[k] == best))
                best, best_k = np.where(better, scores[k], best), np.where(better, k, best_k)
            # 7. refine
            found = best_k >= 0
            kk = np.clip(best_k, 0, D - 1)
            pick = lambda j: np.take_along_axis(scores, np.clip(j, 0, D - 1)[None], axis=0)[0]
            inner = found & (best_k > 0) & (best_k < D - 1)
            sm, sp = np.where(inner, pick(kk - 1), NAN), np.where(inner, pick(kk + 1), NAN)
            dr = depths[r]
            d0, dn, dp = dr[kk], dr[np.clip(kk + 1, 0, D - 1)], dr[np.clip(kk - 1, 0, D - 1)]
            den = (sm - F32(2) * best) + sp
            off = (F32(0.5) * (sm - sp)) / den
            step = np.where(off >= 0, dn - d0, d0 - dp)
            do = inner & ~np.isnan(sm) & ~np.isnan(sp) & (den < 0)
            depth = np.where(do, d0 + off * step, d0)
            assert depth.dtype == F32 and off.dtype == F32
            if note:
                note("best plane at k = 0", found & (best_k == 0))
                note("best plane at k = D - 1", found & (best_k == D - 1))
                note("invalid neighbour", inner & (np.isnan(sm) | np.isnan(sp)))
                note("den == 0", inner & (den == 0))
                note("refined", do)
                note("pixel without a plane", pixel_ok & ~found)
            out_d[r], out_s[r], out_k[r] = np.where(found, depth, NAN), best, best_k
    return (out_d, out_s, out_k, all_scores) if return_scores else (out_d, out_s, out_k)


def filter_depths(depth, poses, intr, sources, near=1e-3, max_reproj=1.0, rel_depth=0.01, min_consistent=2, stats=None):
    """-> filtered float32 [V, H, W], count uint8 [V, H, W]"""
    depth = np.asarray(depth, F32)
    V, H, W = depth.shape
    sources = np.asarray(sources, np.int64).reshape(V, -1)
    k4 = R.intr4(intr, V)
    refs = np.arange(V)
    rel, back = relative_poses(poses, refs, sources), relative_poses(poses, refs, sources, back=True)
    mr, rd = F32(max_reproj), F32(rel_depth)
    reproj2 = mr * mr
    count = np.zeros((V, H * W), np.int64)
    note = (lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(np.count_nonzero(m)))) if stats is not None else None
    uc = np.broadcast_to(np.arange(W).astype(F32)[None, :] + F32(0.5), (H, W)).reshape(-1)
    vc = np.broadcast_to(np.arange(H).astype(F32)[:, None] + F32(0.5), (H, W)).reshape(-1)
    with np.errstate(all="ignore"):
        for r in range(V):
            d = depth[r].reshape(-1)
            has = np.isfinite(d) & (d > 0)
            fx, fy, cx, cy = k4[r]
            X, Y = ((uc - cx) / fx) * d, ((vc - cy) / fy) * d
            dz = rd * d
            for s in range(sources.shape[1]):
                sv = int(sources[r, s])
                if not 0 <= sv < V:
                    continue
                cz, u, v, usable = R.project(np.stack([X, Y, d], axis=1), rel[r, s], k4[sv], near)
                ok = usable & (u >= 0) & (u < F32(W)) & (v >= 0) & (v < F32(H))
                sx, sy = np.where(ok, np.floor(u), 0).astype(np.int64), np.where(ok, np.floor(v), 0).astype(np.int64)
                ds = depth[sv][sy, sx]
                if note:
                    seen = has & ok
                    note("pixel leaves the source image", has & usable & ~ok)
                    note("d_s nan", seen & np.isnan(ds))
                    note("d_s zero", seen & (ds == 0))
                    note("d_s negative", seen & (ds < 0))
                    note("d_s inf", seen & np.isinf(ds))
                ok = has & ok & np.isfinite(ds) & (ds > 0)
                sfx, sfy, scx, scy = k4[sv]
                Xs = (((sx.astype(F32) + F32(0.5)) - scx) / sfx) * ds
                Ys = (((sy.astype(F32) + F32(0.5)) - scy) / sfy) * ds
                z2, u2, v2, usable2 = R.project(np.stack([Xs, Ys, ds], axis=1), back[r, s], k4[r], near)
                du, dv = u2 - uc, v2 - vc
                e = du * du + dv * dv
                dd = np.abs(z2 - d)
                assert e.dtype == F32 and dd.dtype == F32 and dz.dtype == F32
                good = ok & usable2 & (e <= reproj2) & (dd <= dz)
                if note:
                    note("reprojection at equality", ok & usable2 & (e == reproj2) & (dd <= dz))
                    note("reprojection beyond", ok & usable2 & (e > reproj2))
                    note("depth at equality", ok & usable2 & (e <= reproj2) & (dd == dz))
                    note("depth beyond", ok & usable2 & (dd > dz))
                    note("consistent", good)
                count[r] += good
    flat = depth.reshape(V, -1)
    out = np.where(count >= int(min_consistent), flat, NAN).astype(F32)
    return out.reshape(V, H, W), count.astype(np.uint8).reshape(V, H, W)
