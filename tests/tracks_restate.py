"""numpy fp64 restatement of ls2fm.tracks (include/ls2fm.h, "Feature tracks and multi-view triangulation"): the labels of the match
graph, the track table, and the robust N-view triangulation of every track -- hypotheses over the pairs of the first 64
observations, exact integer scoring, the 64-bit selection key, the local optimisation and the acceptance.  Written for this project
from the rules in the header, not from the kernels.

`lapack=True` swaps BOTH Jacobi routines for numpy.linalg (svd for the two-view DLT, eigh for the normal matrix): a second fp64 route
to the same answers, which is what the GPU tests' tolerance is measured against.

`triangulate_tracks(..., margins=True)` also returns how close any decision of the run came to its threshold (pixel error against
max_error_px, angles against min_tri_angle, depths against DBL_EPSILON): the tests assert that their scenes keep clear of them, so
that integer outputs can be compared exactly."""
import math

import numpy as np

HYP_OBS = 64
MAX_OBS = 4096
LO_ITERS = 10
SUB = 8                     # the lanes an LO sum is dealt to
JACOBI_SWEEPS = 30
DBL_EPS = float(np.finfo(np.float64).eps)
EDGE_RANGE, EDGE_IMAGE = 1, 2


# ------------------------------------------------------------------------------------------------------------------ labels
def edge_status(image_start, edges):
    image_start = np.asarray(image_start, np.int64)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    n = int(image_start[-1])
    out_of_range = ((e < 0) | (e >= n)).any(axis=1)
    status = EDGE_RANGE if out_of_range.any() else 0
    ok = e[~out_of_range]
    img = np.searchsorted(image_start[1:], ok, side="right")
    if len(ok) and (img[:, 0] == img[:, 1]).any():
        status |= EDGE_IMAGE
    return status


def track_labels(image_start, edges):
    """labels [n_nodes]: the smallest node id of each node's component (union-find with the smaller root on top; bad edges join
    nothing)"""
    image_start = np.asarray(image_start, np.int64)
    n = int(image_start[-1])
    parent = list(range(n))
    view = np.searchsorted(image_start[1:], np.arange(n), side="right").tolist()

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist():
        if not (0 <= a < n and 0 <= b < n):
            continue
        if view[a] == view[b]:
            continue
        ra, rb = root(a), root(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([root(i) for i in range(n)], np.int32)


def build_tracks(image_start, labels):
    """-> dict(track_start [T + 1], obs_node, obs_view, n_conflicts): components of >= 2 nodes with at most one node per image, in
    label order, their nodes in rising id; a component with two nodes in one image is dropped whole and counted"""
    image_start = np.asarray(image_start, np.int64)
    labels = np.asarray(labels, np.int64)
    view = np.searchsorted(image_start[1:], np.arange(len(labels)), side="right")
    starts, nodes, views, conflicts = [0], [], [], 0
    for lab in np.unique(labels):
        members = np.nonzero(labels == lab)[0]
        if len(members) < 2:
            continue
        if len(set(view[members].tolist())) < len(members):
            conflicts += 1
            continue
        nodes += members.tolist()
        views += view[members].tolist()
        starts.append(len(nodes))
    return dict(track_start=np.array(starts, np.int32), obs_node=np.array(nodes, np.int32), obs_view=np.array(views, np.int32),
                n_conflicts=conflicts)


def edges_from_n_views(n_views):
    """the masked rows of every pair v < j of the n_views tables -> (image_start int32 [V + 1], edges int32 [E, 2])"""
    counts = [len(t["kypts"]) for t in n_views]
    image_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    edges = []
    for v, t in enumerate(n_views):
        others = [j for j in range(len(n_views)) if j != v]
        for slot, j in enumerate(others):
            if j < v:
                continue
            idx = np.asarray(t["indxes"][slot]).reshape(-1, 2) if len(t["indxes"][slot]) else np.zeros((0, 2), np.int64)
            m = np.asarray(t["mask"][slot]).astype(bool).reshape(-1)
            idx = idx.astype(np.int64)[m]
            edges.append(np.stack([image_start[v] + idx[:, 0], image_start[j] + idx[:, 1]], axis=1))
    edges = np.concatenate(edges) if edges else np.zeros((0, 2), np.int64)
    return image_start, edges.astype(np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------ Jacobi
def dlt_jacobi(A):
    """right singular vector of the smallest singular value of every 4 x 4 of A [B,4,4] (rows = equations) by one-sided Jacobi on
    the columns: the device's pair order, threshold and stopping rule; unit norm, w >= 0 -> [B,4]"""
    a = np.ascontiguousarray(np.swapaxes(np.array(A, np.float64), 1, 2))        # a[b, c] = column c
    B = a.shape[0]
    V = np.tile(np.eye(4), (B, 1, 1))                                            # V[b, c] = column c of V
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            any_rot = False
            for p in range(3):
                for q in range(p + 1, 4):
                    ap, aq = a[:, p].copy(), a[:, q].copy()
                    al = ((ap[:, 0] * ap[:, 0] + ap[:, 1] * ap[:, 1]) + ap[:, 2] * ap[:, 2]) + ap[:, 3] * ap[:, 3]
                    be = ((aq[:, 0] * aq[:, 0] + aq[:, 1] * aq[:, 1]) + aq[:, 2] * aq[:, 2]) + aq[:, 3] * aq[:, 3]
                    ga = ((ap[:, 0] * aq[:, 0] + ap[:, 1] * aq[:, 1]) + ap[:, 2] * aq[:, 2]) + ap[:, 3] * aq[:, 3]
                    rot = np.abs(ga) > 1e-15 * np.sqrt(al * be)
                    if not rot.any():
                        continue
                    any_rot = True
                    zeta = (be - al) / (2.0 * ga)
                    t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    c, s, r = c[:, None], s[:, None], rot[:, None]
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    a[:, p] = np.where(r, c * ap - s * aq, ap)
                    a[:, q] = np.where(r, s * ap + c * aq, aq)
                    V[:, p] = np.where(r, c * vp - s * vq, vp)
                    V[:, q] = np.where(r, s * vp + c * vq, vq)
            if not any_rot:
                break
        nrm = ((a[:, :, 0] * a[:, :, 0] + a[:, :, 1] * a[:, :, 1]) + a[:, :, 2] * a[:, :, 2]) + a[:, :, 3] * a[:, :, 3]
        bi = np.zeros(B, np.int64)
        best = nrm[:, 0].copy()
        for c in range(1, 4):
            lower = nrm[:, c] < best
            bi = np.where(lower, c, bi)
            best = np.where(lower, nrm[:, c], best)
        X = V[np.arange(B), bi]
        n = np.sqrt(((X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]) + X[:, 2] * X[:, 2]) + X[:, 3] * X[:, 3])
        return X * (np.where(X[:, 3] < 0.0, -1.0, 1.0) / n)[:, None]


def dlt_lapack(A):
    X = np.linalg.svd(np.asarray(A, np.float64))[2][:, -1]
    X = X / np.linalg.norm(X, axis=1, keepdims=True)
    return X * np.where(X[:, 3] < 0.0, -1.0, 1.0)[:, None]


def jacobi4(a):
    """cyclic Jacobi of the symmetric 4 x 4 a (relpose_restate.jacobi9's rules at size 4) -> (eigenvalues, V[k] = vector k)"""
    a = np.array(a, np.float64)
    V = np.eye(4)
    for _ in range(JACOBI_SWEEPS):
        dia = 0.0
        off = 0.0
        for i in range(4):
            dia += a[i, i] * a[i, i]
            for j in range(i + 1, 4):
                off += a[i, j] * a[i, j]
        if not (off > 1e-30 * dia):
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    if k in (p, q):
                        continue
                    akp, akq = a[k, p], a[k, q]
                    a[k, p] = a[p, k] = c * akp - s * akq
                    a[k, q] = a[q, k] = s * akp + c * akq
                a[p, p] -= t * apq
                a[q, q] += t * apq
                a[p, q] = a[q, p] = 0.0
                vp, vq = V[p].copy(), V[q].copy()
                V[p] = c * vp - s * vq
                V[q] = s * vp + c * vq
    return np.diag(a).copy(), V


def smallest_eigenvector(N, lapack):
    if lapack:
        return np.linalg.eigh(N)[1][:, 0]
    ev, V = jacobi4(N)
    best = 0
    for k in range(1, 4):
        if ev[k] < ev[best]:
            best = k
    return V[best]


# ---------------------------------------------------------------------------------------------------------------- geometry
def centres(poses):
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    return -np.stack([(P[:, 0, k] * P[:, 0, 3] + P[:, 1, k] * P[:, 1, 3]) + P[:, 2, k] * P[:, 2, 3] for k in range(3)], axis=1)


def observe(P, K, uv, X):
    """P [n,3,4], K [n,4], uv [n,2] of n observations against points X [...,3] -> (e2, depth) [..., n]"""
    X0, X1, X2 = X[..., 0:1], X[..., 1:2], X[..., 2:3]
    with np.errstate(all="ignore"):
        xc = ((P[:, 0, 0] * X0 + P[:, 0, 1] * X1) + P[:, 0, 2] * X2) + P[:, 0, 3]
        yc = ((P[:, 1, 0] * X0 + P[:, 1, 1] * X1) + P[:, 1, 2] * X2) + P[:, 1, 3]
        zc = ((P[:, 2, 0] * X0 + P[:, 2, 1] * X1) + P[:, 2, 2] * X2) + P[:, 2, 3]
        du = (K[:, 0] * (xc / zc) + K[:, 2]) - uv[:, 0]
        dv = (K[:, 1] * (yc / zc) + K[:, 3]) - uv[:, 1]
        return du * du + dv * dv, zc


def tri_angle(Ca, Cb, X):
    """min(a, pi - a) of the angle at X between the centres Ca and Cb (all [..., 3])"""
    a, b = X - Ca, X - Cb
    with np.errstate(all="ignore"):
        na = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
        nb = np.sqrt((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2])
        c = ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) / (na * nb)
        c = np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))
        ang = np.arccos(c)
        return np.where(ang < math.pi - ang, ang, math.pi - ang)


def pair_list(m):
    return [(i, j) for i in range(m) for j in range(i + 1, m)]


class _Margins:
    def __init__(self, thr, min_angle):
        self.thr, self.min_angle = thr, min_angle
        self.error_px = self.angle = self.depth = math.inf

    def errors(self, e2, z):
        if e2.size:
            with np.errstate(all="ignore"):
                d = np.abs(np.sqrt(e2) - self.thr)
            front = z > DBL_EPS
            if front.any():
                self.error_px = min(self.error_px, float(np.nanmin(d[front])))
            self.depth = min(self.depth, float(np.nanmin(np.abs(z - DBL_EPS))))

    def angles(self, a):
        a = np.asarray(a, np.float64)
        if a.size and np.isfinite(a).any():
            self.angle = min(self.angle, float(np.nanmin(np.abs(a - self.min_angle))))


def _lane_sum(terms):
    """terms[k] of the track's observation k (None: not added) -> the 8-lane sum: lane k % 8 adds its own in rising order from zero,
    then the butterfly 4, 2, 1"""
    zero = None
    for t in terms:
        if t is not None:
            zero = np.zeros_like(np.asarray(t[0] if isinstance(t, list) else t, np.float64))
            break
    if zero is None:
        return None
    lanes = [zero.copy() for _ in range(SUB)]
    for k, t in enumerate(terms):
        if t is not None:
            for part in (t if isinstance(t, list) else [t]):
                lanes[k % SUB] = lanes[k % SUB] + part
    o = SUB // 2
    while o:
        lanes = [lanes[l] + lanes[l ^ o] for l in range(SUB)]
        o //= 2
    return lanes[0]


LO_EXITS = ("below two", "not finite", "fewer", "unchanged", "limit")


def triangulate_track(P, K, C, uv, thr2, min_angle, lapack=False, mg=None, trace=None):
    """one track: P [n,3,4], K [n,4], C [n,3] (centres), uv [n,2] of its observations -> dict of its outputs.  trace: a dict that, for a
    track that reaches the local optimisation, receives iterations (the refits computed) and exit (one of LO_EXITS: how the loop
    was left); it changes no result"""
    n = len(uv)
    out = dict(X=np.zeros(3), inliers=np.zeros(n, np.uint8), num_inliers=0, success=False, tri_angle=0.0, mean_error_px=0.0,
               best_pair=-1)
    if n < 2 or n > MAX_OBS:
        return out
    m = min(n, HYP_OBS)
    pairs = np.array(pair_list(m), np.int64)
    i, j = pairs[:, 0], pairs[:, 1]
    xy = np.stack([(uv[:, 0] - K[:, 2]) / K[:, 0], (uv[:, 1] - K[:, 3]) / K[:, 1]], axis=1)
    A = np.stack([xy[i, 0:1] * P[i, 2] - P[i, 0], xy[i, 1:2] * P[i, 2] - P[i, 1],
                  xy[j, 0:1] * P[j, 2] - P[j, 0], xy[j, 1:2] * P[j, 2] - P[j, 1]], axis=1)
    h = dlt_lapack(A) if lapack else dlt_jacobi(A)
    with np.errstate(all="ignore"):
        X = h[:, :3] / h[:, 3:4]
    finite = np.isfinite(X).all(axis=1)
    Xs = np.where(finite[:, None], X, 0.0)
    zi = ((P[i, 2, 0] * Xs[:, 0] + P[i, 2, 1] * Xs[:, 1]) + P[i, 2, 2] * Xs[:, 2]) + P[i, 2, 3]
    zj = ((P[j, 2, 0] * Xs[:, 0] + P[j, 2, 1] * Xs[:, 1]) + P[j, 2, 2] * Xs[:, 2]) + P[j, 2, 3]
    ang = tri_angle(C[i], C[j], Xs)
    front = finite & (zi > DBL_EPS) & (zj > DBL_EPS)
    valid = front & (ang >= min_angle)
    if mg is not None:
        mg.angles(ang[front])
        if finite.any():
            mg.depth = min(mg.depth, float(np.abs(np.r_[zi[finite], zj[finite]] - DBL_EPS).min()))
    if not valid.any():
        return out
    e2, z = observe(P, K, uv, Xs[valid][:, None, :].reshape(-1, 3))
    if mg is not None:
        mg.errors(e2, z)
    counts = ((z > DBL_EPS) & (e2 <= thr2)).sum(axis=1)
    qs = np.nonzero(valid)[0]
    keys = [(int(c) << 32) | (0xFFFFFFFF - int(q)) for c, q in zip(counts, qs) if c > 0]
    if not keys:
        return out
    key = max(keys)
    q = 0xFFFFFFFF - (key & 0xFFFFFFFF)
    cur = key >> 32
    Xc = Xs[q].copy()

    def mask_of(Y):
        e2, z = observe(P, K, uv, Y.reshape(1, 3))
        if mg is not None:
            mg.errors(e2, z)
        return ((z > DBL_EPS) & (e2 <= thr2))[0], e2[0]

    inl, e2c = mask_of(Xc)
    assert int(inl.sum()) == cur
    iterations, left_by = 0, "limit"
    for _ in range(LO_ITERS):
        if cur < 2:
            left_by = "below two"
            break
        terms = []
        for k in range(n):
            if not inl[k]:
                terms.append(None)
                continue
            rows = []
            for r in range(2):
                d = xy[k, r] * P[k, 2] - P[k, r]
                d = d * (1.0 / math.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]))
                rows.append(np.outer(d, d))
            terms.append(rows)
        N = _lane_sum(terms)
        v = smallest_eigenvector(N, lapack)
        iterations += 1
        with np.errstate(all="ignore"):
            Xn = v[:3] / v[3]
        if not np.isfinite(Xn).all():
            left_by = "not finite"
            break
        inl_n, e2n = mask_of(Xn)
        cnt = int(inl_n.sum())
        if cnt < cur:
            left_by = "fewer"
            break
        changed = bool((inl_n != inl).any())
        Xc, cur, inl, e2c = Xn, cnt, inl_n, e2n
        if not changed:
            left_by = "unchanged"
            break
    if trace is not None:
        trace.update(iterations=iterations, exit=left_by)
    first = np.nonzero(inl)[0][:HYP_OBS]
    best_angle = 0.0
    if len(first) >= 2:
        pp = np.array(pair_list(len(first)), np.int64)
        a = tri_angle(C[first[pp[:, 0]]], C[first[pp[:, 1]]], Xc)
        if mg is not None:
            mg.angles(a.max())
        a = a[~np.isnan(a)]
        best_angle = float(a.max()) if len(a) else 0.0
    ok = cur >= 2 and best_angle >= min_angle
    err = _lane_sum([math.sqrt(e2c[k]) if inl[k] else None for k in range(n)])
    out.update(X=Xc if ok else np.zeros(3), inliers=inl.astype(np.uint8), num_inliers=int(cur), success=bool(ok), tri_angle=best_angle,
               mean_error_px=float(err) / cur if cur > 0 else 0.0, best_pair=int(q))
    return out


def triangulate_tracks(poses, intrinsics, track_start, obs_view, obs_uv, max_error_px=4.0, min_tri_angle_deg=1.5, lapack=False,
                       margins=False, trace=None):
    """every track -> dict(X [T,3], inliers uint8 [n_obs], num_inliers, success, tri_angle, mean_error_px, best_pair) and, with
    margins=True, dict(error_px, angle, depth): the closest any decision came to its threshold.  trace: a list that receives one
    dict per track (triangulate_track's; empty for a track that never reached the local optimisation)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    intr = np.asarray(intrinsics, np.float64).reshape(-1, 4)
    if len(intr) == 1:
        intr = np.repeat(intr, len(poses), axis=0)
    ts = np.asarray(track_start, np.int64)
    view = np.asarray(obs_view, np.int64)
    uv = np.asarray(obs_uv, np.float64).reshape(-1, 2)
    C = centres(poses)
    thr2 = float(max_error_px) * float(max_error_px)
    min_angle = float(min_tri_angle_deg) * (math.pi / 180.0)
    mg = _Margins(float(max_error_px), min_angle) if margins else None
    T = len(ts) - 1
    res = dict(X=np.zeros((T, 3)), inliers=np.zeros(len(uv), np.uint8), num_inliers=np.zeros(T, np.int32), success=np.zeros(T, bool),
               tri_angle=np.zeros(T), mean_error_px=np.zeros(T), best_pair=np.full(T, -1, np.int32))
    for t in range(T):
        s, e = int(ts[t]), int(ts[t + 1])
        v = view[s:e]
        tr = {} if trace is not None else None
        o = triangulate_track(poses[v], intr[v], C[v], uv[s:e], thr2, min_angle, lapack, mg, tr)
        if trace is not None:
            trace.append(tr)
        res["inliers"][s:e] = o.pop("inliers")
        for k, val in o.items():
            res[k][t] = val
    if margins:
        return res, dict(error_px=mg.error_px, angle=mg.angle, depth=mg.depth)
    return res
