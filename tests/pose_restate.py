"""numpy float64 restatement of ls2fm_p3p / ls2fm_absolute_pose / ls2fm_pose_refine (csrc/absolute_pose.hip), the checker of the
device results.  include/ls2fm.h states the rules this file repeats step by step: the SplitMix64 sample stream, Lambda Twist P3P
(Persson & Nordberg, ECCV 2018) with the same choices (largest real root of the cubic, lines in the order +/-, roots in the
order q / C, A / q), scoring, selection by (count, then lowest trial * 4 + solution), the round stopping rule, Gauss-Newton local
optimisation and Levenberg-Marquardt with a Cauchy loss.  Scalar Python where the device runs one thread per sample; vectorised
over the correspondences where the device spreads them over threads (same operation order per element)."""
import math

import numpy as np

M64 = (1 << 64) - 1
ROUND = 1024                  # trials per view per round (LS2FM_POSE_ROUND)
LO_ITERS = 10
GN_TOL = 1e-10                # LM: gradient tolerance (max |g_j|)
STEP_TOL = 1e-12              # LM: step tolerance (max |delta_j| <= STEP_TOL (1 + max |t_j|))


# ------------------------------------------------------------------------------------------------------------ sample stream
def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def trial_key(seed, t):
    return splitmix64((seed & M64) ^ splitmix64(t))


def draw(seed, t, k, n):
    """k-th draw of trial t over n correspondences: the high 32 bits of splitmix64(key + k), scaled to [0, n)"""
    return ((splitmix64((trial_key(seed, t) + k) & M64) >> 32) * n) >> 32


def sample(seed, t, n):
    """the 3 distinct indices of trial t, or None (64 draws without three distinct values)"""
    got = []
    for k in range(64):
        i = draw(seed, t, k, n)
        if i not in got:
            got.append(i)
            if len(got) == 3:
                return got
    return None


# ------------------------------------------------------------------------------------------------------------------- P3P
def _det3(c0, c1, c2):
    """determinant of the matrix with columns c0, c1, c2"""
    return (c0[0] * (c1[1] * c2[2] - c1[2] * c2[1]) - c1[0] * (c0[1] * c2[2] - c0[2] * c2[1])
            + c2[0] * (c0[1] * c1[2] - c0[2] * c1[1]))


def _cubic_root(b, c, d):
    """a real root of x^3 + b x^2 + c x + d: the only one, or the largest of three; two Newton steps"""
    p = c - b * b / 3.0
    q = 2.0 * b * b * b / 27.0 - b * c / 3.0 + d
    disc = q * q / 4.0 + p * p * p / 27.0
    if disc > 0.0:
        s = math.sqrt(disc)
        u = -q / 2.0 + (s if q <= 0.0 else -s)
        cu = math.copysign(abs(u) ** (1.0 / 3.0), u)
        x = (cu - p / (3.0 * cu) if cu != 0.0 else 0.0) - b / 3.0
    else:
        m = math.sqrt(max(-p / 3.0, 0.0))
        arg = (3.0 * q / (2.0 * p) * math.sqrt(-3.0 / p)) if p < 0.0 else 0.0
        arg = min(max(arg, -1.0), 1.0)
        x = 2.0 * m * math.cos(math.acos(arg) / 3.0) - b / 3.0
    for _ in range(2):
        f = ((x + b) * x + c) * x + d
        df = (3.0 * x + 2.0 * b) * x + c
        if df != 0.0:
            x = x - f / df
    return x


def _null_vec(D, s):
    """unit vector of the null space of the symmetric D - s I (largest cross product of two rows)"""
    r0 = np.array([D[0][0] - s, D[0][1], D[0][2]])
    r1 = np.array([D[1][0], D[1][1] - s, D[1][2]])
    r2 = np.array([D[2][0], D[2][1], D[2][2] - s])
    c01, c02, c12 = np.cross(r0, r1), np.cross(r0, r2), np.cross(r1, r2)
    n01, n02, n12 = c01 @ c01, c02 @ c02, c12 @ c12
    best, nb = (c01, n01) if n01 >= n02 else (c02, n02)
    best, nb = (best, nb) if nb >= n12 else (c12, n12)
    return best / math.sqrt(nb) if nb > 0.0 else None


def _quad(O, u, v):
    return float(u @ O @ v)


def p3p(y, x):
    """Lambda Twist.  y [3,3] unit bearings, x [3,3] world points -> list of 4 entries (slot order), each None or a
    world-to-camera [3,4] pose"""
    y = np.asarray(y, np.float64)
    x = np.asarray(x, np.float64)
    out = [None] * 4
    d01, d02, d12 = x[0] - x[1], x[0] - x[2], x[1] - x[2]
    a01, a02, a12 = d01 @ d01, d02 @ d02, d12 @ d12
    cr = np.cross(d01, d02)
    if not (cr @ cr > 1e-20 * a01 * a02) or not (a01 > 0.0 and a02 > 0.0 and a12 > 0.0):
        return out
    b01, b02, b12 = y[0] @ y[1], y[0] @ y[2], y[1] @ y[2]
    M01 = np.array([[1.0, -b01, 0.0], [-b01, 1.0, 0.0], [0.0, 0.0, 0.0]])
    M02 = np.array([[1.0, 0.0, -b02], [0.0, 0.0, 0.0], [-b02, 0.0, 1.0]])
    M12 = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, -b12], [0.0, -b12, 1.0]])
    D1 = a12 * M01 - a01 * M12
    D2 = a12 * M02 - a02 * M12
    # det(D1 + g D2) = c3 g^3 + c2 g^2 + c1 g + c0
    c0 = _det3(D1[:, 0], D1[:, 1], D1[:, 2])
    c3 = _det3(D2[:, 0], D2[:, 1], D2[:, 2])
    c1 = _det3(D2[:, 0], D1[:, 1], D1[:, 2]) + _det3(D1[:, 0], D2[:, 1], D1[:, 2]) + _det3(D1[:, 0], D1[:, 1], D2[:, 2])
    c2 = _det3(D1[:, 0], D2[:, 1], D2[:, 2]) + _det3(D2[:, 0], D1[:, 1], D2[:, 2]) + _det3(D2[:, 0], D2[:, 1], D1[:, 2])
    if abs(c3) >= abs(c0):
        if c3 == 0.0:
            return out
        g = _cubic_root(c2 / c3, c1 / c3, c0 / c3)
        D0, O = D1 + g * D2, D2
    else:
        g = _cubic_root(c1 / c0, c2 / c0, c3 / c0)
        D0, O = g * D1 + D2, D1
    tr = D0[0, 0] + D0[1, 1] + D0[2, 2]
    m2 = (D0[0, 0] * D0[1, 1] - D0[0, 1] * D0[0, 1]) + (D0[0, 0] * D0[2, 2] - D0[0, 2] * D0[0, 2]) \
        + (D0[1, 1] * D0[2, 2] - D0[1, 2] * D0[1, 2])
    if not (m2 < 0.0):
        return out
    sq = math.sqrt(max(tr * tr - 4.0 * m2, 0.0))
    if tr >= 0.0:
        s1 = 0.5 * (tr + sq)
        s2 = m2 / s1
    else:
        s2 = 0.5 * (tr - sq)
        s1 = m2 / s2
    e1, e2 = _null_vec(D0, s1), _null_vec(D0, s2)
    if e1 is None or e2 is None:
        return out
    r = math.sqrt(-s2 / s1)
    A_ = (a01, a02, a12)
    B_ = (b01, b02, b12)
    IJ = ((0, 1), (0, 2), (1, 2))
    ks = 0 if (a01 >= a02 and a01 >= a12) else (1 if a02 >= a12 else 2)      # the scale equation: the longest side
    for li, sgn in enumerate((1.0, -1.0)):
        w = e1 - (sgn * r) * e2
        k = 0 if (abs(w[0]) >= abs(w[1]) and abs(w[0]) >= abs(w[2])) else (1 if abs(w[1]) >= abs(w[2]) else 2)
        i, j = (k + 1) % 3, (k + 2) % 3
        p = np.zeros(3)
        qv = np.zeros(3)
        p[i] = 1.0
        p[k] = -w[i] / w[k]
        qv[j] = 1.0
        qv[k] = -w[j] / w[k]
        A, B, C = _quad(O, p, p), _quad(O, p, qv), _quad(O, qv, qv)
        disc = B * B - A * C
        if not (disc >= 0.0):
            continue
        qq = -(B + math.copysign(math.sqrt(disc), B))
        taus = (qq / C if C != 0.0 else math.nan, A / qq if qq != 0.0 else math.nan)
        for ri, tau in enumerate(taus):
            if not math.isfinite(tau):
                continue
            dvec = p + tau * qv
            ia, ib = IJ[ks]
            qs = dvec[ia] * dvec[ia] + dvec[ib] * dvec[ib] - 2.0 * B_[ks] * dvec[ia] * dvec[ib]
            if not (qs > 0.0):
                continue
            sc = math.sqrt(A_[ks] / qs)
            if dvec[0] + dvec[1] + dvec[2] < 0.0:
                sc = -sc
            lam = sc * dvec
            lam = _refine_lambda(lam, A_, B_)
            pose = _pose_from_depths(lam, y, x)
            if pose is not None:
                out[2 * li + ri] = pose
    return out


def _refine_lambda(lam, A_, B_):
    """five Gauss-Newton steps on the three distance equations, each kept only when it lowers the squared residual"""
    l0, l1, l2 = float(lam[0]), float(lam[1]), float(lam[2])

    def res(l0, l1, l2):
        return (l0 * l0 + l1 * l1 - 2.0 * B_[0] * l0 * l1 - A_[0], l0 * l0 + l2 * l2 - 2.0 * B_[1] * l0 * l2 - A_[1],
                l1 * l1 + l2 * l2 - 2.0 * B_[2] * l1 * l2 - A_[2])

    r = res(l0, l1, l2)
    e = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    for _ in range(5):
        J = ((2.0 * (l0 - B_[0] * l1), 2.0 * (l1 - B_[0] * l0), 0.0),
             (2.0 * (l0 - B_[1] * l2), 0.0, 2.0 * (l2 - B_[1] * l0)),
             (0.0, 2.0 * (l1 - B_[2] * l2), 2.0 * (l2 - B_[2] * l1)))
        det = _det3((J[0][0], J[1][0], J[2][0]), (J[0][1], J[1][1], J[2][1]), (J[0][2], J[1][2], J[2][2]))
        if det == 0.0 or not math.isfinite(det):
            break
        # Cramer: delta_c = det(J with column c replaced by r) / det
        cols = [(J[0][0], J[1][0], J[2][0]), (J[0][1], J[1][1], J[2][1]), (J[0][2], J[1][2], J[2][2])]
        dl = []
        for c in range(3):
            cc = list(cols)
            cc[c] = r
            dl.append(_det3(cc[0], cc[1], cc[2]) / det)
        n0, n1, n2 = l0 - dl[0], l1 - dl[1], l2 - dl[2]
        rn = res(n0, n1, n2)
        en = rn[0] * rn[0] + rn[1] * rn[1] + rn[2] * rn[2]
        if not (en < e):
            break
        l0, l1, l2, r, e = n0, n1, n2, rn, en
    return np.array([l0, l1, l2])


def _frame(a, b):
    """orthonormal frame (columns) of the triangle edges a, b: e1 = a / |a|, e2 = the part of b orthogonal to e1, e3 = e1 x e2"""
    na = a @ a
    if not (na > 0.0):
        return None
    e1 = a / math.sqrt(na)
    b2 = b - (e1 @ b) * e1
    nb = b2 @ b2
    if not (nb > 0.0):
        return None
    e2 = b2 / math.sqrt(nb)
    return np.stack([e1, e2, np.cross(e1, e2)], axis=1)


def _pose_from_depths(lam, y, x):
    if not (lam[0] > 0.0 and lam[1] > 0.0 and lam[2] > 0.0):
        return None
    c = lam[:, None] * y
    Fc = _frame(c[0] - c[1], c[0] - c[2])
    Fw = _frame(x[0] - x[1], x[0] - x[2])
    if Fc is None or Fw is None:
        return None
    R = Fc @ Fw.T
    t = (c[0] + c[1] + c[2]) / 3.0 - R @ ((x[0] + x[1] + x[2]) / 3.0)
    P = np.concatenate([R, t[:, None]], axis=1)
    if not np.isfinite(P).all():
        return None
    z = x @ R[2] + t[2]
    if not (z > 0.0).all():
        return None
    return P


def bearings(uv, intr):
    """unit bearings of pixels uv [n,2] through intr (fx, fy, cx, cy)"""
    fx, fy, cx, cy = intr
    uv = np.asarray(uv, np.float64)
    b = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], axis=1)
    return b / np.sqrt((b * b).sum(axis=1, keepdims=True))


def well_conditioned(y, x, min_angle_deg=5.0, min_bearing_deg=2.0):
    """every triangle angle >= min_angle_deg and every pair of bearings >= min_bearing_deg apart"""
    for k in range(3):
        u, v = x[(k + 1) % 3] - x[k], x[(k + 2) % 3] - x[k]
        if np.degrees(np.arccos(np.clip(u @ v / np.linalg.norm(u) / np.linalg.norm(v), -1, 1))) < min_angle_deg:
            return False
        if np.degrees(np.arccos(np.clip(y[k] @ y[(k + 1) % 3], -1, 1))) < min_bearing_deg:
            return False
    return True


# --------------------------------------------------------------------------------------------------------------- scoring
def project_err2(P, xyz, uv, intr):
    """(camera z, squared pixel error) of every correspondence under P, in the device's operation order"""
    fx, fy, cx, cy = intr
    X = ((P[0, 0] * xyz[:, 0] + P[0, 1] * xyz[:, 1]) + P[0, 2] * xyz[:, 2]) + P[0, 3]
    Y = ((P[1, 0] * xyz[:, 0] + P[1, 1] * xyz[:, 1]) + P[1, 2] * xyz[:, 2]) + P[1, 3]
    Z = ((P[2, 0] * xyz[:, 0] + P[2, 1] * xyz[:, 1]) + P[2, 2] * xyz[:, 2]) + P[2, 3]
    iz = 1.0 / Z
    du = (fx * (X * iz) + cx) - uv[:, 0]
    dv = (fy * (Y * iz) + cy) - uv[:, 1]
    return Z, du * du + dv * dv


def inliers(P, xyz, uv, intr, max_error_px):
    Z, e2 = project_err2(P, xyz, uv, intr)
    return (Z > 0.0) & (e2 < max_error_px * max_error_px)


# ------------------------------------------------------------------------------------------------------------- stopping
def num_trials(eps, confidence, min_trials, max_trials):
    """clamp(ceil(log(1 - confidence) / log(1 - eps^3)), min_trials, max_trials); eps <= 0 -> max, eps >= 1 -> min"""
    if eps <= 0.0:
        return max_trials
    if eps >= 1.0:
        return min_trials
    den = math.log(1.0 - eps * eps * eps)
    if den >= 0.0:
        return max_trials
    n = math.ceil(math.log(1.0 - confidence) / den)
    return int(max(min_trials, min(max_trials, n)))


def max_trials_eff(confidence, min_inlier_ratio, max_num_trials):
    """the trial cap: max_num_trials, lowered to the count the stopping rule gives at min_inlier_ratio (COLMAP's RANSAC)"""
    return num_trials(min_inlier_ratio, confidence, 0, max_num_trials)


# ------------------------------------------------------------------------------------------------- least squares (GN / LM)
def _rodrigues(w):
    th2 = w @ w
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th2 < 1e-30:
        return np.eye(3) + K
    th = math.sqrt(th2)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / th2) * (K @ K)


def update(P, delta):
    """R <- exp([w]x) R, t <- exp([w]x) t + dt: the camera-space points move by the increment (delta = (w, dt))"""
    E = _rodrigues(np.asarray(delta[:3]))
    return np.concatenate([E @ P[:, :3], (E @ P[:, 3] + delta[3:])[:, None]], axis=1)


def normal_eqs(P, xyz, uv, intr, loss_scale=None):
    """H = sum w J^T J, g = sum w J^T r, F = 0.5 sum rho(s) over the given correspondences; w = rho'(s) (1 without a loss)"""
    fx, fy, cx, cy = intr
    X = ((P[0, 0] * xyz[:, 0] + P[0, 1] * xyz[:, 1]) + P[0, 2] * xyz[:, 2]) + P[0, 3]
    Y = ((P[1, 0] * xyz[:, 0] + P[1, 1] * xyz[:, 1]) + P[1, 2] * xyz[:, 2]) + P[1, 3]
    Z = ((P[2, 0] * xyz[:, 0] + P[2, 1] * xyz[:, 1]) + P[2, 2] * xyz[:, 2]) + P[2, 3]
    iz = 1.0 / Z
    du = (fx * (X * iz) + cx) - uv[:, 0]
    dv = (fy * (Y * iz) + cy) - uv[:, 1]
    s = du * du + dv * dv
    if loss_scale is None:
        w = np.ones_like(s)
        F = 0.5 * s.sum()
    else:
        c2 = loss_scale * loss_scale
        w = 1.0 / (1.0 + s / c2)
        F = 0.5 * (c2 * np.log1p(s / c2)).sum()
    # d(u, v) / d p  (p = camera point) times d p / d(w, dt) = [-[p]x | I]
    ju = np.stack([fx * iz, np.zeros_like(iz), -fx * X * iz * iz], axis=1)
    jv = np.stack([np.zeros_like(iz), fy * iz, -fy * Y * iz * iz], axis=1)
    p = np.stack([X, Y, Z], axis=1)

    def rows(jp):
        jw = np.cross(p, jp)          # jp^T (-[p]x) = (p x jp)^T
        return np.concatenate([jw, jp], axis=1)

    Ju, Jv = rows(ju), rows(jv)
    H = (Ju * w[:, None]).T @ Ju + (Jv * w[:, None]).T @ Jv
    g = (Ju * (w * du)[:, None]).sum(0) + (Jv * (w * dv)[:, None]).sum(0)
    return H, g, F


def _chol_solve(A, b):
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    z = np.linalg.solve(L, b)
    return np.linalg.solve(L.T, z)


def local_optimise(P, xyz, uv, intr, max_error_px):
    """-> (pose, inlier mask): up to LO_ITERS Gauss-Newton steps on the inliers' squared pixel error, each followed by a recount;
    a step is kept when its count is >= the old one; stop when it is not, or when the inlier set does not change"""
    m = inliers(P, xyz, uv, intr, max_error_px)
    for _ in range(LO_ITERS):
        if m.sum() < 3:
            break
        H, g, _ = normal_eqs(P, xyz[m], uv[m], intr)
        d = _chol_solve(H, -g)
        if d is None or not np.isfinite(d).all():
            break
        C = update(P, d)
        mc = inliers(C, xyz, uv, intr, max_error_px)
        if mc.sum() < m.sum():
            break
        same = np.array_equal(mc, m)
        P, m = C, mc
        if same:
            break
    return P, m


def refine(P, xyz, uv, intr, mask, loss_scale=1.0, max_iters=100):
    """Levenberg-Marquardt on the fixed mask with the Cauchy loss rho(s) = c^2 log(1 + s / c^2) (IRLS weights rho'(s)), damping
    lambda diag(H) (diag floored at 1e-12 of its largest entry), lambda from 1e-4, x 0.1 on a kept step, x 10 on a rejected one"""
    xyz, uv = xyz[mask], uv[mask]
    if len(xyz) < 3:
        return P
    lam = 1e-4
    for _ in range(max_iters):
        H, g, F = normal_eqs(P, xyz, uv, intr, loss_scale)
        if np.abs(g).max() <= GN_TOL:
            break
        dg = np.diag(H)
        dg = np.maximum(dg, 1e-12 * dg.max())
        d = _chol_solve(H + lam * np.diag(dg), -g)
        if d is None or not np.isfinite(d).all():
            lam *= 10.0
            if lam > 1e32:
                break
            continue
        C = update(P, d)
        _, _, Fc = normal_eqs(C, xyz, uv, intr, loss_scale)
        if Fc < F:
            P = C
            lam = max(lam * 0.1, 1e-16)
            if np.abs(d).max() <= STEP_TOL * (1.0 + np.abs(P[:, 3]).max()):
                break
        else:
            lam *= 10.0
            if lam > 1e32:
                break
    return P


# ------------------------------------------------------------------------------------------------------------ estimation
def absolute_pose(uv, xyz, intr, max_error_px=12.0, confidence=0.9999, min_inlier_ratio=0.01, min_num_trials=1000,
                  max_num_trials=100000, seed=0, refine_pose=True):
    """one view -> dict(pose [3,4], inliers bool [n], num_inliers, trials, best_trial, success)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(uv)
    fail = dict(pose=np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), inliers=np.zeros(n, bool), num_inliers=0, trials=0,
                best_trial=-1, success=False)
    if n < 3:
        return fail
    cap = max_trials_eff(confidence, min_inlier_ratio, max_num_trials)
    min_num_trials = min(min_num_trials, cap)               # the cap wins over min_num_trials
    bear = bearings(uv, intr)
    best_key, best_pose = 0, None
    trials = 0
    target = num_trials(0.0, confidence, min_num_trials, cap)
    while trials < target:
        for t in range(trials, trials + ROUND):
            idx = sample(seed, t, n)
            if idx is None:
                continue
            sols = p3p(bear[idx], xyz[idx])
            for s, P in enumerate(sols):
                if P is None:
                    continue
                cnt = int(inliers(P, xyz, uv, intr, max_error_px).sum())
                key = (cnt << 32) | (0xFFFFFFFF - (t * 4 + s)) if cnt > 0 else 0
                if key > best_key:
                    best_key, best_pose = key, P
        trials += ROUND
        eps = (best_key >> 32) / n
        target = num_trials(eps, confidence, min_num_trials, cap)
    if best_pose is None:
        fail.update(trials=trials)
        return fail
    best_trial = (0xFFFFFFFF - (best_key & 0xFFFFFFFF)) // 4
    P, m = local_optimise(best_pose, xyz, uv, intr, max_error_px)
    cnt = int(m.sum())
    if refine_pose and cnt >= 4:
        P = refine(P, xyz, uv, intr, m)
    return dict(pose=P, inliers=m, num_inliers=cnt, trials=trials, best_trial=int(best_trial), success=cnt >= 4,
                sampled_pose=best_pose)
