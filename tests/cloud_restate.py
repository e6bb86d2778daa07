"""numpy restatement of ls2fm.cloud, written for this project (no device, no torch): the K-NEIGHBOUR RULE by brute force
(metrics_restate.d2_matrix plus np.lexsort((index, d2))), the NORMAL RULE (mean and covariance by a loop over the list, a cyclic
Jacobi that repeats the stated rule, numpy.linalg.eigh as the second route), the two outlier filters and normal consistency."""
import math

import numpy as np

import metrics_restate as MR

F32 = np.float32
JACOBI_SWEEPS = 30


def knn(q, ref, k, max_dist=None, skip_own=False, chunk=256):
    """(idx int32 [M, k], d2 float32 [M, k], count int32 [M]): the qualifying references ordered by (d2, index), the first k"""
    q, ref = np.asarray(q, F32).reshape(-1, 3), np.asarray(ref, F32).reshape(-1, 3)
    m, n = len(q), len(ref)
    idx, out, count = np.full((m, k), -1, np.int32), np.full((m, k), np.inf, F32), np.zeros(m, np.int32)
    if n == 0:
        return idx, out, count
    lim = MR.max_d2_of(max_dist)
    index = np.arange(n)
    for s in range(0, m, chunk):
        d2 = MR.d2_matrix(q[s:s + chunk], ref)
        with np.errstate(invalid="ignore"):
            ok = (d2 <= lim) & (d2 < np.inf)
        for t in range(len(d2)):
            if skip_own:
                ok[t, s + t] = False
            cand = index[ok[t]]
            order = cand[np.lexsort((cand, d2[t, cand]))][:k]
            idx[s + t, :len(order)] = order
            out[s + t, :len(order)] = d2[t, order]
            count[s + t] = len(order)
    return idx, out, count


def covariance(points, idx):
    """(n int [M], mean fp64 [M, 3], C fp64 [M, 6] as xx xy xz yy yz zz): fp64 of the fp32 points, the sums in list order starting
    from the first term, one rounding per operation (python floats); NaN rows for n = 0"""
    p = np.asarray(points, F32).astype(np.float64)
    idx = np.asarray(idx)
    m = len(idx)
    n, mean, C = np.zeros(m, np.int64), np.full((m, 3), np.nan), np.full((m, 6), np.nan)
    for t in range(m):
        rows = [p[i] for i in idx[t] if 0 <= i < len(p)]
        n[t] = len(rows)
        if not rows:
            continue
        s = rows[0].copy()
        for r in rows[1:]:
            s = s + r
        mu = s / float(len(rows))
        acc = None
        for r in rows:
            d = r - mu
            term = np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]])
            acc = term if acc is None else acc + term
        mean[t], C[t] = mu, acc / float(len(rows))
    return n, mean, C


def full(c):
    xx, xy, xz, yy, yz, zz = c
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def jacobi3(c):
    """cyclic Jacobi of the symmetric 3 x 3 given as its six entries (tracks_restate.jacobi4's rules at size 3)
    -> (eigenvalues [3], V[k] = vector k)"""
    a = full(np.asarray(c, np.float64))
    V = np.eye(3)
    for _ in range(JACOBI_SWEEPS):
        dia = (a[0, 0] * a[0, 0] + a[1, 1] * a[1, 1]) + a[2, 2] * a[2, 2]
        off = (a[0, 1] * a[0, 1] + a[0, 2] * a[0, 2]) + a[1, 2] * a[1, 2]
        if not (off > 1e-30 * dia):
            break
        for p in range(2):
            for q in range(p + 1, 3):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c_ = 1.0 / math.sqrt(t * t + 1.0)
                s_ = t * c_
                k = 3 - p - q
                akp, akq = a[k, p], a[k, q]
                a[k, p] = a[p, k] = c_ * akp - s_ * akq
                a[k, q] = a[q, k] = s_ * akp + c_ * akq
                a[p, p] -= t * apq
                a[q, q] += t * apq
                a[p, q] = a[q, p] = 0.0
                vp, vq = V[p].copy(), V[q].copy()
                V[p] = c_ * vp - s_ * vq
                V[q] = s_ * vp + c_ * vq
    return np.diag(a).copy(), V


def orient(v, query=None, toward=None):
    if toward is not None:
        t = np.asarray(toward, F32).astype(np.float64) - np.asarray(query, F32).astype(np.float64)
        flip = (v[0] * t[0] + v[1] * t[1]) + v[2] * t[2] < 0.0
    else:
        big = v[0]
        for r in (1, 2):
            if abs(v[r]) > abs(big):
                big = v[r]
        flip = big < 0.0
    return -v if flip else v


def normals(points, idx, queries=None, toward=None, lapack=False):
    """(normal fp64 [M, 3], curvature fp64 [M], C fp64 [M, 6], n [M]) by the NORMAL RULE; lapack: numpy.linalg.eigh in the Jacobi's
    place (the second route: eigenvalues ascending, so the first vector)"""
    n, _, C = covariance(points, idx)
    m = len(n)
    normal, curvature = np.full((m, 3), np.nan), np.full(m, np.nan)
    tw = None if toward is None else np.broadcast_to(np.asarray(toward, F32).reshape(-1, 3), (m, 3))
    for t in range(m):
        if n[t] < 3:
            continue
        trace = (C[t, 0] + C[t, 3]) + C[t, 5]
        if trace == 0.0 or trace != trace:
            continue
        if lapack:
            ev, vec = np.linalg.eigh(full(C[t]))
            v, lam = vec[:, 0], ev[0]
        else:
            ev, V = jacobi3(C[t])
            best = 0
            for i in (1, 2):
                if ev[i] < ev[best]:
                    best = i
            v, lam = V[best], ev[best]
        v = v / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        normal[t] = orient(v, None if tw is None else queries[t], None if tw is None else tw[t])
        curvature[t] = lam / ((ev[0] + ev[1]) + ev[2])
    return normal, curvature, C, n


def eigen_residuals(C, v):
    """per matrix: (|C v - (v^T C v) v| / |C|_F, ||v| - 1|, v^T C v) for C [M, 6], v [M, 3]; NaN rows where v is NaN"""
    m = len(C)
    res, unit, ray = np.full(m, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    for t in range(m):
        if not np.isfinite(v[t]).all():
            continue
        A = full(C[t])
        Av = A @ v[t]
        ray[t] = v[t] @ Av
        res[t] = np.linalg.norm(Av - ray[t] * v[t]) / np.linalg.norm(A)
        unit[t] = abs(np.linalg.norm(v[t]) - 1.0)
    return res, unit, ray


def angle(a, b):
    """the unsigned angle between the lines of a and b (rad), from the cross product and the dot product together"""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(axis=-1)))


def mean_distances(points, k):
    """fp64 [N]: the mean of sqrt(double(d2)) over each point's k nearest other points, NaN without any; and the terms' sums"""
    _, d2, count = knn(points, points, k, skip_own=True)
    dist = np.where(d2 < np.inf, np.sqrt(d2.astype(np.float64)), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dist.sum(axis=1) / count, dist.sum(axis=1)


def statistical_outliers(points, k, std_ratio):
    mean, _ = mean_distances(points, k)
    ok = np.isfinite(mean)
    mu = mean[ok].mean()
    sigma = math.sqrt(((mean[ok] - mu) ** 2).mean())
    threshold = mu + std_ratio * sigma
    with np.errstate(invalid="ignore"):
        return mean <= threshold, mean, threshold


def radius_outliers(points, radius, min_neighbors):
    return knn(points, points, min_neighbors, radius, skip_own=True)[2] == min_neighbors


def normal_consistency(pred, pn, gt, gn, max_dist):
    def side(q, qn, ref, refn):
        idx, _ = MR.nearest(q, ref, max_dist)
        has = idx >= 0
        a, b = np.asarray(qn, np.float64)[has], np.asarray(refn, np.float64)[idx[has]]
        dot = np.abs((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
        return int(has.sum()), float(dot.sum() / has.sum()) if has.any() else float("nan")
    na, acc = side(pred, pn, gt, gn)
    nc, com = side(gt, gn, pred, pn)
    return dict(accuracy=acc, completeness=com, overall=0.5 * (acc + com), n_accuracy=na, n_completeness=nc)
