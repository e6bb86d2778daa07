"""numpy / Python float64 restatement of ls2fm_seven_point / ls2fm_four_point_homography / ls2fm_fundamental_matrix /
ls2fm_homography (csrc/two_view.hip) and of ls2fm.pose.two_view_geometry's verdict, the checker of the device results.
include/ls2fm.h states the rules this file repeats: Hartley conditioning, the null space by Gauss-Jordan, the cubic of the
seven-point pencil with its closed-form roots and bracketed Newton polish, the four-point DLT, the two scores, the SplitMix64
sample stream and the round stopping rule (tests/relpose_restate.py, with eps^7 / eps^4), selection by (count, then lowest
trial * S + slot), local optimisation through the normal matrix's Jacobi eigenvector, and COLMAP's configuration rules.

The pencil's cubic is formed here by numpy polynomial arithmetic on the cofactor expansion, and the rank-2 step uses numpy's SVD:
the device's multilinear expansion and one-sided Jacobi are checked, not repeated."""
import math

import numpy as np

import relpose_restate as RR
from pose_restate import draw

ROUND = RR.ROUND
LO_ITERS = 10
NEWTON_ITERS = 5
DBL_EPS = np.finfo(np.float64).eps
DEGENERATE, CALIBRATED, UNCALIBRATED, PLANAR_OR_PANORAMIC = 1, 2, 3, 6

canonical = RR.canonical           # unit norm, the largest |entry| positive (the first of equals)


# ------------------------------------------------------------------------------------------------------------ conditioning
def hartley(x):
    """[n,2] -> (T [3,3], normalised [n,2]) or None"""
    x = np.asarray(x, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        c = x.sum(axis=0) / len(x)
        d = x - c
        rms = math.sqrt((d * d).sum() / len(x)) if np.isfinite((d * d).sum()) else float("nan")
    if not (rms > 0.0) or not math.isfinite(rms):
        return None
    s = math.sqrt(2.0) / rms
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]]), d * s


def nullspace(A):
    """Gauss-Jordan with partial pivoting on the R x 9 rows A -> the [9 - R, 9] basis of the free columns, or None (rank != R)"""
    A = [[float(v) for v in r] for r in A]
    R = len(A)
    amax = max(abs(v) for r in A for v in r)
    if not (amax > 0.0) or not math.isfinite(amax):
        return None
    rank, piv, free = 0, [], []
    for c in range(9):
        p, best = -1, 0.0
        for r in range(rank, R):
            if p < 0 or abs(A[r][c]) > best:
                p, best = r, abs(A[r][c])
        if rank == R or not (best > 1e-12 * amax):
            free.append(c)
            continue
        A[rank], A[p] = A[p], A[rank]
        inv = 1.0 / A[rank][c]
        A[rank] = [v * inv for v in A[rank]]
        for r in range(R):
            if r != rank:
                f = A[r][c]
                A[r] = [A[r][k] - f * A[rank][k] for k in range(9)]
        piv.append(c)
        rank += 1
    if rank != R or len(free) != 9 - R:
        return None
    basis = []
    for f in free:
        v = [1.0 if k == f else 0.0 for k in range(9)]
        for i, c in enumerate(piv):
            v[c] = -A[i][f]
        basis.append(v)
    return np.array(basis)


# ------------------------------------------------------------------------------------------------------------------ cubic
def _polish(c, x, lo, hi):
    for _ in range(NEWTON_ITERS):
        f = ((c[3] * x + c[2]) * x + c[1]) * x + c[0]
        df = (3.0 * c[3] * x + 2.0 * c[2]) * x + c[1]
        if df == 0.0:
            break
        xn = x - f / df
        if not (lo <= xn <= hi) or xn == x:
            break
        x = xn
    return x


def cubic_roots(c):
    """real roots, ascending, of c[0] + c[1] x + c[2] x^2 + c[3] x^3: closed form, then the bracketed Newton polish"""
    c = [float(v) for v in c]
    if not all(math.isfinite(v) for v in c):
        return []
    m = max(abs(v) for v in c)
    if not (m > 0.0):
        return []
    c = [v / m for v in c]
    inf = math.inf
    if abs(c[3]) < 1e-14:
        c[3] = 0.0
        if abs(c[2]) < 1e-14:
            if c[1] == 0.0:
                return []
            r = -c[0] / c[1]
            return [r] if math.isfinite(r) else []
        disc = c[1] * c[1] - 4.0 * c[2] * c[0]
        if not (disc >= 0.0):
            return []
        q = -0.5 * (c[1] + (1.0 if c[1] >= 0.0 else -1.0) * math.sqrt(disc))
        x0 = q / c[2]
        x1 = c[0] / q if q != 0.0 else x0
        x0, x1 = min(x0, x1), max(x0, x1)
        vertex = -c[1] / (2.0 * c[2])
        out = sorted([_polish(c, x0, -inf, vertex), _polish(c, x1, vertex, inf)])
        return out if all(math.isfinite(v) for v in out) else []
    a, b, d = c[2] / c[3], c[1] / c[3], c[0] / c[3]
    Q = (a * a - 3.0 * b) / 9.0
    R = ((2.0 * a * a - 9.0 * b) * a + 27.0 * d) / 54.0
    R2, Q3, mid = R * R, Q * Q * Q, -a / 3.0
    if R2 < Q3:
        sq = math.sqrt(Q)
        th = math.acos(min(1.0, max(-1.0, R / math.sqrt(Q3))))
        out = sorted([_polish(c, -2.0 * sq * math.cos(th / 3.0) + mid, -inf, mid - sq),
                      _polish(c, -2.0 * sq * math.cos((th - 2.0 * math.pi) / 3.0) + mid, mid - sq, mid + sq),
                      _polish(c, -2.0 * sq * math.cos((th + 2.0 * math.pi) / 3.0) + mid, mid + sq, inf)])
        return out if all(math.isfinite(v) for v in out) else []
    A = -(1.0 if R >= 0.0 else -1.0) * np.cbrt(abs(R) + math.sqrt(R2 - Q3))
    B = Q / A if A != 0.0 else 0.0
    x = (A + B) + mid
    lo, hi = -inf, inf
    if Q > 0.0:
        sq = math.sqrt(Q)
        if x < mid:
            hi = mid - sq
        else:
            lo = mid + sq
    x = _polish(c, float(x), lo, hi)
    return [x] if math.isfinite(x) else []


# --------------------------------------------------------------------------------------------------------- minimal solvers
def seven_point(p1, p2):
    """pixels p1, p2 [7,2] -> list of unit F [3,3] with x2h^T F x1h = 0 (ascending root order)"""
    n1, n2 = hartley(p1), hartley(p2)
    if n1 is None or n2 is None:
        return []
    (T1, a), (T2, b) = n1, n2
    h1, h2 = np.c_[a, np.ones(7)], np.c_[b, np.ones(7)]
    basis = nullspace((h2[:, :, None] * h1[:, None, :]).reshape(7, 9))
    if basis is None:
        return []
    b0, b1 = basis                                   # modified Gram-Schmidt, as the five-point basis
    n0 = float(b0 @ b0)
    if not (n0 > 0.0) or not math.isfinite(n0):
        return []
    b0 = b0 * (1.0 / math.sqrt(n0))
    b1 = b1 - float(b0 @ b1) * b0
    n1 = float(b1 @ b1)
    if not (n1 > 0.0) or not math.isfinite(n1):
        return []
    b1 = b1 * (1.0 / math.sqrt(n1))
    F1, F2 = b0.reshape(3, 3), b1.reshape(3, 3)
    # det(F2 + l (F1 - F2)) by polynomial arithmetic on the first row's cofactors
    P = np.polynomial.polynomial
    D = F1 - F2
    e = [[np.array([F2[i, j], D[i, j]]) for j in range(3)] for i in range(3)]

    def minor(j0, j1):
        return P.polysub(P.polymul(e[1][j0], e[2][j1]), P.polymul(e[1][j1], e[2][j0]))

    det = P.polyadd(P.polysub(P.polymul(e[0][0], minor(1, 2)), P.polymul(e[0][1], minor(0, 2))), P.polymul(e[0][2], minor(0, 1)))
    det = np.concatenate([det, np.zeros(4 - len(det))])
    out = []
    for lam in cubic_roots(det):
        F = canonical(T2.T @ (lam * F1 + (1.0 - lam) * F2) @ T1)
        if F is not None:
            out.append(F.reshape(3, 3))
    return out


def dlt_rows(a, b):
    """normalised points a -> b [n,2]: the [2n, 9] homography rows"""
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    z, o = np.zeros(len(a)), np.ones(len(a))
    ra = np.stack([-x, -y, -o, z, z, z, u * x, u * y, u], axis=1)
    rb = np.stack([z, z, z, -x, -y, -o, v * x, v * y, v], axis=1)
    return np.stack([ra, rb], axis=1).reshape(-1, 9)


def four_point(p1, p2):
    """pixels p1, p2 [4,2] -> list (0 or 1) of unit H [3,3] with x2h ~ H x1h"""
    n1, n2 = hartley(p1), hartley(p2)
    if n1 is None or n2 is None:
        return []
    (T1, a), (T2, b) = n1, n2
    basis = nullspace(dlt_rows(a, b))
    if basis is None:
        return []
    H = canonical(np.linalg.inv(T2) @ basis[0].reshape(3, 3) @ T1)
    return [] if H is None else [H.reshape(3, 3)]


# ---------------------------------------------------------------------------------------------------------------- scoring
def f_inliers_of(F, uv0, uv1, max_error_px=4.0):
    return RR.sampson2(F, np.asarray(uv0, np.float64).reshape(-1, 2), np.asarray(uv1, np.float64).reshape(-1, 2)) <= max_error_px ** 2


def h_inliers_of(H, uv0, uv1, max_error_px=4.0):
    H = np.asarray(H, np.float64).reshape(9)
    a, b = np.asarray(uv0, np.float64).reshape(-1, 2), np.asarray(uv1, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        w = (H[6] * a[:, 0] + H[7] * a[:, 1]) + H[8]
        dx = ((H[0] * a[:, 0] + H[1] * a[:, 1]) + H[2]) / w - b[:, 0]
        dy = ((H[3] * a[:, 0] + H[4] * a[:, 1]) + H[5]) / w - b[:, 1]
        return (np.abs(w) > DBL_EPS) & np.isfinite(w) & (dx * dx + dy * dy <= max_error_px ** 2)


# ------------------------------------------------------------------------------------------------------------------- LO
def _smallest_eigenvector(Q):
    ev, V = RR.jacobi9(Q.T @ Q)
    return V[min(range(9), key=lambda k: (ev[k], k))]


def f_from_inliers(uv0, uv1):
    n1, n2 = hartley(uv0), hartley(uv1)
    if n1 is None or n2 is None:
        return None
    (T1, a), (T2, b) = n1, n2
    h1, h2 = np.c_[a, np.ones(len(a))], np.c_[b, np.ones(len(b))]
    F = _smallest_eigenvector((h2[:, :, None] * h1[:, None, :]).reshape(-1, 9)).reshape(3, 3)
    U, s, Vt = np.linalg.svd(F)
    F = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    F = canonical(T2.T @ F @ T1)
    return None if F is None else F.reshape(3, 3)


def h_from_inliers(uv0, uv1):
    n1, n2 = hartley(uv0), hartley(uv1)
    if n1 is None or n2 is None:
        return None
    (T1, a), (T2, b) = n1, n2
    H = canonical(np.linalg.inv(T2) @ _smallest_eigenvector(dlt_rows(a, b)).reshape(3, 3) @ T1)
    return None if H is None else H.reshape(3, 3)


# ---------------------------------------------------------------------------------------------------------------- RANSAC
def num_trials(k, eps, confidence, min_t, max_t):
    """relpose_restate.num_trials with eps^k, multiplied left to right"""
    if eps <= 0.0:
        return max_t
    if eps >= 1.0:
        return min_t
    pk = eps
    for _ in range(1, k):
        pk = pk * eps
    den = math.log(1.0 - pk)
    if den >= 0.0:
        return max_t
    n = math.ceil(math.log(1.0 - confidence) / den)
    if n >= max_t:
        return max(min_t, max_t)
    return max(int(n), min_t)


def sample(seed, t, n, k):
    got = []
    for j in range(64):
        i = draw(seed, t, j, n)
        if i not in got:
            got.append(i)
            if len(got) == k:
                return got
    return None


def _ransac(uv0, uv1, k, n_slots, solver, inliers_of, refit, min_ok, max_error_px, confidence, min_inlier_ratio, min_num_trials,
            max_num_trials, seed):
    uv0, uv1 = np.asarray(uv0, np.float64).reshape(-1, 2), np.asarray(uv1, np.float64).reshape(-1, 2)
    n = len(uv0)
    cap = num_trials(k, min_inlier_ratio, confidence, 0, max_num_trials)
    min_t = min(min_num_trials, cap)
    best_key, best_M, trials = 0, None, 0
    if n >= k:
        while True:
            for tl in range(ROUND):
                t = trials + tl
                s = sample(seed, t, n, k)
                if s is None:
                    continue
                for slot, M in enumerate(solver(uv0[s], uv1[s])):
                    c = int(inliers_of(M, uv0, uv1, max_error_px).sum())
                    key = (c << 32) | (0xFFFFFFFF - (t * n_slots + slot)) if c > 0 else 0
                    if key > best_key:
                        best_key, best_M = key, M
            trials += ROUND
            if trials >= num_trials(k, (best_key >> 32) / n, confidence, min_t, cap) or trials >= cap:
                break
    fail = dict(model=np.zeros((3, 3)), inliers=np.zeros(n, bool), num_inliers=0, trials=trials, success=False,
                best_trial=(0xFFFFFFFF - (best_key & 0xFFFFFFFF)) // n_slots if best_key else -1)
    if best_key == 0:
        return fail
    M = best_M
    inl = inliers_of(M, uv0, uv1, max_error_px)
    cur = int(inl.sum())
    for _ in range(LO_ITERS):
        if cur < min_ok:
            break
        C = refit(uv0[inl], uv1[inl])
        if C is None:
            break
        new = inliers_of(C, uv0, uv1, max_error_px)
        if int(new.sum()) < cur:
            break
        changed = bool((new != inl).any())
        M, inl, cur = C, new, int(new.sum())
        if not changed:
            break
    if cur < min_ok:
        return fail
    return dict(model=M, inliers=inl, num_inliers=cur, trials=trials, best_trial=fail["best_trial"], success=True)


def fundamental_matrix(uv0, uv1, max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.25, min_num_trials=100,
                       max_num_trials=10000, seed=0):
    """one pair -> dict(model, inliers, num_inliers, trials, best_trial, success)"""
    return _ransac(uv0, uv1, 7, 3, seven_point, f_inliers_of, f_from_inliers, 8, max_error_px, confidence, min_inlier_ratio,
                   min_num_trials, max_num_trials, seed)


def homography(uv0, uv1, max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.25, min_num_trials=100, max_num_trials=10000,
               seed=0):
    return _ransac(uv0, uv1, 4, 1, four_point, h_inliers_of, h_from_inliers, 4, max_error_px, confidence, min_inlier_ratio,
                   min_num_trials, max_num_trials, seed)


# ---------------------------------------------------------------------------------------------------------------- verdict
def config_of(nE, okE, nF, okF, nH, min_num_inliers=15, min_E_F_inlier_ratio=0.95, max_H_inlier_ratio=0.8):
    """one pair's counts (nE / okE None: no calibration) -> (config, which inlier set: "E", "F", "H" or None)"""
    if nE is not None and okE and nE >= min_num_inliers and (nE / nF if nF else (math.inf if nE else math.nan)) > min_E_F_inlier_ratio:
        config, best, who = CALIBRATED, nE, "E"
    elif okF and nF >= min_num_inliers:
        config, best, who = UNCALIBRATED, nF, "F"
    else:
        return DEGENERATE, None
    if nH / best > max_H_inlier_ratio:
        config = PLANAR_OR_PANORAMIC
        if nH > best:
            who = "H"
    return config, who
