"""numpy restatement of ls2fm.metrics, written for this project (no device, no torch): the brute-force nearest neighbour by the
distance rule of include/ls2fm.h, voxel thinning, the Chamfer dict, and Umeyama's alignment by two routes (SVD; Horn's
quaternion through eigh) with the pose errors on top."""
import numpy as np

F32 = np.float32


def max_d2_of(max_dist):
    if max_dist is None:
        return F32(np.inf)
    with np.errstate(over="ignore"):
        return F32(F32(max_dist) * F32(max_dist))


def d2_matrix(q, ref):
    """fp32 [M, N]: dx = q.x - r.x, dy, dz likewise, d2 = (dx dx + dy dy) + dz dz; numpy rounds every array operation once"""
    q, ref = np.asarray(q, F32), np.asarray(ref, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, 0:1] - ref[None, :, 0]
        dy = q[:, 1:2] - ref[None, :, 1]
        dz = q[:, 2:3] - ref[None, :, 2]
        return ((dx * dx + dy * dy) + dz * dz).astype(F32)


def nearest(q, ref, max_dist=None, chunk=512):
    """(idx int32 [M], d2 float32 [M]): the qualifying reference (d2 <= max_d2 and d2 < +inf) of smallest d2, the lowest index
    among equals (np.argmin takes the first minimum); -1 / +inf without one"""
    q, ref = np.asarray(q, F32).reshape(-1, 3), np.asarray(ref, F32).reshape(-1, 3)
    m, n = len(q), len(ref)
    idx, out = np.full(m, -1, np.int32), np.full(m, np.inf, F32)
    if n == 0:
        return idx, out
    lim = max_d2_of(max_dist)
    for s in range(0, m, chunk):
        d2 = d2_matrix(q[s:s + chunk], ref)
        with np.errstate(invalid="ignore"):
            ok = (d2 <= lim) & (d2 < np.inf)
        d2 = np.where(ok, d2, F32(np.inf))
        a = np.argmin(d2, axis=1)
        best = d2[np.arange(len(a)), a]
        idx[s:s + chunk] = np.where(best < np.inf, a, -1)
        out[s:s + chunk] = best
    return idx, out


def voxel_downsample(points, voxel):
    """ascending int64 indices: the lowest-index point of every voxel floor(double(p) / voxel) (np.unique over the coordinate
    rows returns the first occurrence of each)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros(0, np.int64)
    v = np.floor(p / float(voxel)).astype(np.int64)
    _, first = np.unique(v, axis=0, return_index=True)
    return np.sort(first).astype(np.int64)


def _side(q, ref, max_dist, thresholds):
    idx, d2 = nearest(q, ref, max_dist)
    has = idx >= 0
    n = int(has.sum())
    dist = np.sqrt(d2[has].astype(np.float64))
    mean = float(dist.sum() / n) if n else float("nan")
    rates = tuple((float((has & (d2 <= F32(F32(t) * F32(t)))).sum()) / len(q)) if len(q) else float("nan") for t in thresholds)
    return n, mean, rates


def chamfer(pred, gt, max_dist, thresholds=()):
    na, acc, prec = _side(pred, gt, max_dist, thresholds)
    nc, com, rec = _side(gt, pred, max_dist, thresholds)
    f = tuple((2 * p * r / (p + r)) if p + r > 0 else (0.0 if p + r == 0 else float("nan")) for p, r in zip(prec, rec))
    return dict(accuracy=acc, completeness=com, overall=0.5 * (acc + com), n_accuracy=na, n_completeness=nc,
                thresholds=tuple(float(t) for t in thresholds), precision=prec, recall=rec, fscore=f)


# ------------------------------------------------------------------------------------------------------------ alignment
def _moments(src, dst):
    a, b = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    mu_a, mu_b = a.mean(axis=0), b.mean(axis=0)
    xa, xb = a - mu_a, b - mu_b
    return mu_a, mu_b, xa, xb


def umeyama_svd(src, dst, with_scale=True):
    """Umeyama 1991: cov = mean xb xa^T = U D V^T, R = U S V^T with S = diag(1, 1, sign det U det V), s = tr(D S) / var(src)"""
    mu_a, mu_b, xa, xb = _moments(src, dst)
    cov = xb.T @ xa / len(xa)
    U, D, Vt = np.linalg.svd(cov)
    S = np.array([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ np.diag(S) @ Vt
    s = float((D * S).sum() / (xa * xa).sum(axis=1).mean()) if with_scale else 1.0
    return s, R, mu_b - s * R @ mu_a


def umeyama_horn(src, dst, with_scale=True):
    """Horn 1987: the rotation is the unit quaternion of the largest eigenvalue of the symmetric 4 x 4 matrix of the cross
    covariance (always a proper rotation: no determinant case), the scale sum xb . R xa / sum |xa|^2"""
    mu_a, mu_b, xa, xb = _moments(src, dst)
    M = xa.T @ xb                                       # M[i, j] = sum a_i b_j
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = M
    N = np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                  [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                  [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
                  [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz]])
    w, v = np.linalg.eigh(N)
    q0, q1, q2, q3 = v[:, -1]
    R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                  [2 * (q2 * q1 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                  [2 * (q3 * q1 - q0 * q2), 2 * (q3 * q2 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
    s = float((xb * (xa @ R.T)).sum() / (xa * xa).sum()) if with_scale else 1.0
    return s, R, mu_b - s * R @ mu_a


def centres(poses):
    P = np.asarray(poses, np.float64)
    R, t = P[:, :3, :3], P[:, :3, 3]
    return -np.einsum("vji,vj->vi", R, t)


def pose_errors(poses_est, poses_gt, align=True, with_scale=True, registered=None, route=umeyama_svd):
    """dict(rot_err_deg [V], centre_err [V] (NaN for views left out), ate_rmse, scale): centres aligned by `route`, the estimated
    orientations rotated along"""
    Pe, Pg = np.asarray(poses_est, np.float64), np.asarray(poses_gt, np.float64)
    V = len(Pe)
    reg = np.ones(V, bool) if registered is None else np.asarray(registered, bool)
    sel = np.nonzero(reg)[0]
    Ce, Cg = centres(Pe[sel]), centres(Pg[sel])
    s, A, a = route(Ce, Cg, with_scale) if align else (1.0, np.eye(3), np.zeros(3))
    centre = np.linalg.norm(s * Ce @ A.T + a - Cg, axis=1)
    D = np.einsum("vij,kj,vlk->vil", Pe[sel][:, :3, :3], A, Pg[sel][:, :3, :3])       # R_est A^T R_gt^T
    # the angle from the rotation's axis part and trace together: arccos of the trace alone loses half the digits near 0
    axis = 0.5 * np.linalg.norm(np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1), axis=1)
    rot = np.degrees(np.arctan2(axis, (np.trace(D, axis1=1, axis2=2) - 1) / 2))
    full_r, full_c = np.full(V, np.nan), np.full(V, np.nan)
    full_r[sel], full_c[sel] = rot, centre
    return dict(rot_err_deg=full_r, centre_err=full_c, ate_rmse=float(np.sqrt((centre ** 2).mean())), scale=float(s))
