"""numpy / Python float64 restatement of ls2fm_five_point / ls2fm_relative_pose / ls2fm_triangulate (csrc/relative_pose.hip), the
checker of the device results.  include/ls2fm.h states the rules this file repeats: the null space by Gauss-Jordan, Nister's
cubic constraints, the elimination, the degree-10 polynomial, Sturm bisection with Newton polish, E per root, the squared Sampson
error, the SplitMix64 sample stream (tests/pose_restate.py), selection by (count, then lowest trial * 10 + slot), the round
stopping rule with eps^5, local optimisation through the normal matrix's Jacobi eigenvectors, and COLMAP's pose recovery.

The 10 x 20 constraint matrix is built here by GENERIC polynomial arithmetic (dicts of monomial exponents), not from the device's
index tables, and pose recovery uses numpy's SVD for E and for the DLT: the device's one-sided Jacobi is checked, not repeated.
Scalar Python where the device runs one thread per problem (small problems run faster as Python floats than as numpy arrays),
numpy over the correspondences."""
import math

import numpy as np

from pose_restate import draw, splitmix64, trial_key  # noqa: F401  (the same sample stream)

ROUND = 1024
MAX_SOL = 10
LO_ITERS = 10
STURM_TRIM = 1e-14            # LS2FM_STURM_TRIM
BISECT_TOL = 1e-10            # LS2FM_BISECT_TOL
BISECT_ITERS = 100
NEWTON_ITERS = 5
JACOBI_SWEEPS = 30
DBL_EPS = np.finfo(np.float64).eps

# COLMAP's monomial order of the 10 x 20 matrix: exponents of (x, y, z)
MONOMIALS = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
             (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
_VARS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


# ------------------------------------------------------------------------------------------------------------ sample stream
def sample(seed, t, n):
    """the first five distinct draws of trial t among k = 0..63, or None"""
    got = []
    for k in range(64):
        i = draw(seed, t, k, n)
        if i not in got:
            got.append(i)
            if len(got) == 5:
                return got
    return None


def num_trials(eps, confidence, min_t, max_t):
    if eps <= 0.0:
        return max_t
    if eps >= 1.0:
        return min_t
    den = math.log(1.0 - eps * eps * eps * eps * eps)
    if den >= 0.0:
        return max_t
    n = math.ceil(math.log(1.0 - confidence) / den)
    if n >= max_t:
        return max(min_t, max_t)
    return max(int(n), min_t)


def max_trials_eff(confidence, min_inlier_ratio, max_num_trials):
    return num_trials(min_inlier_ratio, confidence, 0, max_num_trials)


# ------------------------------------------------------------------------------------------------------------ polynomials
def padd(a, b, s=1.0):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0.0) + s * v
    return out


def pmul(a, b):
    out = {}
    for ka, va in a.items():
        for kb, vb in b.items():
            k = (ka[0] + kb[0], ka[1] + kb[1], ka[2] + kb[2])
            out[k] = out.get(k, 0.0) + va * vb
    return out


def pscale(a, s):
    return {k: s * v for k, v in a.items()}


def constraint_matrix(basis):
    """basis [4, 9] (X, Y, Z, W) -> the 10 x 20 matrix of 2 E E^T E - tr(E E^T) E (rows 0..8) and det E (row 9)"""
    E = [[{_VARS[v]: float(basis[v][3 * i + j]) for v in range(4)} for j in range(3)] for i in range(3)]
    EEt = [[{} for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                EEt[i][j] = padd(EEt[i][j], pmul(E[i][k], E[j][k]))
    tr = padd(padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    rows = []
    for i in range(3):
        for j in range(3):
            acc = {}
            for k in range(3):
                acc = padd(acc, pscale(pmul(EEt[i][k], E[k][j]), 2.0))
            rows.append(padd(acc, pmul(tr, E[i][j]), -1.0))
    det = {}
    for (a, b, c), s in (((0, 1, 2), 1), ((0, 2, 1), -1), ((1, 0, 2), -1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((2, 1, 0), -1)):
        det = padd(det, pmul(pmul(E[0][a], E[1][b]), E[2][c]), float(s))
    rows.append(det)
    return np.array([[r.get(m, 0.0) for m in MONOMIALS] for r in rows])


def nullspace5(x1, x2):
    """Gauss-Jordan with partial pivoting on the 5 x 9 rows kron((x2, 1), (x1, 1)), then modified Gram-Schmidt -> [4, 9] or None"""
    A = [[float(b[i] * a[j]) for i in range(3) for j in range(3)]
         for a, b in zip(np.c_[np.asarray(x1, float), np.ones(5)], np.c_[np.asarray(x2, float), np.ones(5)])]
    amax = max(abs(v) for r in A for v in r)
    if not (amax > 0.0) or not math.isfinite(amax):
        return None
    rank, piv, free = 0, [], []
    for c in range(9):
        p, best = -1, 0.0
        for r in range(rank, 5):
            if p < 0 or abs(A[r][c]) > best:
                p, best = r, abs(A[r][c])
        if rank == 5 or not (best > 1e-12 * amax):
            free.append(c)
            continue
        A[rank], A[p] = A[p], A[rank]
        inv = 1.0 / A[rank][c]
        A[rank] = [v * inv for v in A[rank]]
        for r in range(5):
            if r != rank:
                f = A[r][c]
                A[r] = [A[r][k] - f * A[rank][k] for k in range(9)]
        piv.append(c)
        rank += 1
    if rank != 5 or len(free) != 4:
        return None
    basis = []
    for f in free:
        v = [1.0 if k == f else 0.0 for k in range(9)]
        for i, c in enumerate(piv):
            v[c] = -A[i][f]
        basis.append(v)
    for j in range(4):
        for i in range(j):
            d = sum(basis[i][k] * basis[j][k] for k in range(9))
            basis[j] = [basis[j][k] - d * basis[i][k] for k in range(9)]
        n = sum(v * v for v in basis[j])
        if not (n > 0.0) or not math.isfinite(n):
            return None
        basis[j] = [v / math.sqrt(n) for v in basis[j]]
    return np.array(basis)


def _horner(c, x):
    r = c[-1]
    for v in reversed(c[:-1]):
        r = r * x + v
    return r


def _normalise(c):
    m = max(abs(v) for v in c)
    return [v / m for v in c] if m > 0.0 else list(c)


def sturm_roots(poly):
    """real roots (ascending) of the ascending-coefficient polynomial: Sturm sequence, bisection, Newton polish"""
    c = [float(v) for v in poly]
    d = len(c) - 1
    while d >= 0 and c[d] == 0.0:
        d -= 1
    if d < 1 or not all(math.isfinite(v) for v in c[:d + 1]):
        return []
    p0 = _normalise(c[:d + 1])
    seq = [p0, _normalise([(i + 1) * p0[i + 1] for i in range(d)])]
    while len(seq) < 11 and len(seq[-1]) - 1 > 0:
        u, v = list(seq[-2]), seq[-1]
        du, dv = len(u) - 1, len(v) - 1
        for k in range(du - dv, -1, -1):
            q = u[dv + k] / v[dv]
            for j in range(dv):
                u[j + k] -= q * v[j]
            u[dv + k] = 0.0
        dr = dv - 1
        while dr >= 0 and not (abs(u[dr]) > STURM_TRIM):
            dr -= 1
        if dr < 0:
            break
        seq.append(_normalise([-u[i] for i in range(dr + 1)]))

    def changes(x):
        n, last = 0, 0.0
        for p in seq:
            v = _horner(p, x)
            if v != 0.0:
                if last != 0.0 and (v > 0.0) != (last > 0.0):
                    n += 1
                last = v
        return n

    bound = 1.0 + max(abs(p0[i] / p0[d]) for i in range(d))
    if not math.isfinite(bound):
        return []
    v_lo = changes(-bound)
    total = v_lo - changes(bound)
    roots, lo = [], -bound
    for k in range(1, total + 1):
        if len(roots) >= MAX_SOL:
            break
        hi = bound
        for _ in range(BISECT_ITERS):
            mid = 0.5 * (lo + hi)
            if not (hi - lo > BISECT_TOL * max(1.0, abs(lo), abs(hi))) or mid == lo or mid == hi:
                break
            if v_lo - changes(mid) >= k:
                hi = mid
            else:
                lo = mid
        x = 0.5 * (lo + hi)
        for _ in range(NEWTON_ITERS):
            f, df = p0[d], 0.0
            for i in range(d - 1, -1, -1):
                df = df * x + f
                f = f * x + p0[i]
            if df == 0.0:
                break
            xn = x - f / df
            if not (lo <= xn <= hi) or xn == x:
                break
            x = xn
        roots.append(x)
    return roots


def canonical(e):
    e = np.asarray(e, float).reshape(9)
    n = float(e @ e)
    if not (n > 0.0) or not math.isfinite(n):
        return None
    e = e / math.sqrt(n)
    k = int(np.argmax(np.abs(e)))          # the first of equals
    return e if e[k] >= 0 else -e


def solve_from_basis(basis):
    """the five-point steps from the constraints on -> list of unit E [3,3] (ascending root order)"""
    A = constraint_matrix(basis)
    amax = np.abs(A).max()
    if not (amax > 0.0) or not np.isfinite(amax):
        return []
    A = [list(r) for r in A]
    for c in range(10):
        p = max(range(c, 10), key=lambda r: (abs(A[r][c]), -r))
        if not (abs(A[p][c]) > 1e-14 * amax):
            return []
        A[c], A[p] = A[p], A[c]
        inv = 1.0 / A[c][c]
        A[c] = [v * inv for v in A[c]]
        for r in range(10):
            if r != c:
                f = A[r][c]
                A[r] = [A[r][k] - f * A[c][k] for k in range(20)]
    AA = np.array(A)[:, 10:]
    # B(z) [x y 1]^T = 0, ascending powers of z: <e> - z <f> for (e, f) = (x^2 z, x^2), (y^2 z, y^2), (xyz, xy)
    P = np.polynomial.polynomial
    B = []
    for i in range(3):
        e, f = AA[2 * i + 4], AA[2 * i + 5]
        cols = []
        for lo, hi in ((0, 3), (3, 6), (6, 10)):
            ce, cf = e[lo:hi][::-1], f[lo:hi][::-1]          # ascending powers
            cols.append(P.polysub(ce, P.polymulx(cf)))
        B.append(cols)
    det = P.polyadd(P.polyadd(P.polymul(B[0][0], P.polysub(P.polymul(B[1][1], B[2][2]), P.polymul(B[1][2], B[2][1]))),
                              -P.polymul(B[0][1], P.polysub(P.polymul(B[1][0], B[2][2]), P.polymul(B[1][2], B[2][0])))),
                    P.polymul(B[0][2], P.polysub(P.polymul(B[1][0], B[2][1]), P.polymul(B[1][1], B[2][0]))))
    det = np.concatenate([det, np.zeros(11 - len(det))])
    out = []
    for z in sturm_roots(det):
        Bz = np.array([[P.polyval(z, B[i][c]) for c in range(3)] for i in range(3)])
        crs = [np.cross(Bz[0], Bz[1]), np.cross(Bz[0], Bz[2]), np.cross(Bz[1], Bz[2])]
        ns = [float(v @ v) for v in crs]
        k = 0 if ns[0] >= ns[1] else 1
        k = k if ns[k] >= ns[2] else 2
        X, nb = crs[k], ns[k]
        if not (nb > 0.0) or not math.isfinite(nb) or not (abs(X[2]) >= 1e-10 * math.sqrt(nb)):
            continue
        x, y = X[0] / X[2], X[1] / X[2]
        e = canonical(x * basis[0] + y * basis[1] + z * basis[2] + basis[3])
        if e is not None:
            out.append(e.reshape(3, 3))
    return out


def five_point(x1, x2):
    """x1, x2 [5,2] normalised points -> list of unit E [3,3]"""
    basis = nullspace5(x1, x2)
    return [] if basis is None else solve_from_basis(basis)


# ---------------------------------------------------------------------------------------------------------------- scoring
def normalised(uv, K):
    fx, fy, cx, cy = (float(v) for v in K)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    return np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy], axis=1)


def sampson2(E, x1, x2):
    E = np.asarray(E, np.float64).reshape(9)
    a0 = (E[0] * x1[:, 0] + E[1] * x1[:, 1]) + E[2]
    a1 = (E[3] * x1[:, 0] + E[4] * x1[:, 1]) + E[5]
    a2 = (E[6] * x1[:, 0] + E[7] * x1[:, 1]) + E[8]
    b0 = (E[0] * x2[:, 0] + E[3] * x2[:, 1]) + E[6]
    b1 = (E[1] * x2[:, 0] + E[4] * x2[:, 1]) + E[7]
    num = (x2[:, 0] * a0 + x2[:, 1] * a1) + a2
    den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1
    with np.errstate(divide="ignore", invalid="ignore"):
        return num * num / den


def threshold2(K0, K1, max_error_px):
    f0, f1 = 0.5 * (K0[0] + K0[1]), 0.5 * (K1[0] + K1[1])
    e = 0.5 * (max_error_px / f0 + max_error_px / f1)
    return e * e


def inliers_of(E, x1, x2, thr2):
    return sampson2(E, x1, x2) <= thr2


# ------------------------------------------------------------------------------------------------------------ Jacobi, LO
def jacobi9(a):
    """cyclic Jacobi of the symmetric 9 x 9 a, the device's rotation order and stopping rule -> (eigenvalues, V[k] = vector k)"""
    a = np.array(a, np.float64)
    V = np.eye(9)
    for _ in range(JACOBI_SWEEPS):
        off = sum(a[i, j] ** 2 for i in range(9) for j in range(i + 1, 9))
        dia = sum(a[i, i] ** 2 for i in range(9))
        if not (off > 1e-30 * dia):
            break
        for p in range(8):
            for q in range(p + 1, 9):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(9):
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


def local_basis(x1, x2):
    """the normal matrix of the rows kron((x2, 1), (x1, 1)), its four smallest-eigenvalue vectors as X, Y, Z, W"""
    h1, h2 = np.c_[x1, np.ones(len(x1))], np.c_[x2, np.ones(len(x2))]
    Q = (h2[:, :, None] * h1[:, None, :]).reshape(-1, 9)
    ev, V = jacobi9(Q.T @ Q)
    order = sorted(range(9), key=lambda k: (ev[k], k))
    return np.array([V[order[3]], V[order[2]], V[order[1]], V[order[0]]])


# ------------------------------------------------------------------------------------------------------------------ pose
def triangulate(P0, P1, p0, p1):
    """DLT of cv2.triangulatePoints by numpy's SVD -> unit homogeneous [n,4] with w >= 0"""
    P0, P1 = np.asarray(P0, float), np.asarray(P1, float)
    out = []
    for (u0, v0), (u1, v1) in zip(np.asarray(p0, float).reshape(-1, 2), np.asarray(p1, float).reshape(-1, 2)):
        A = np.stack([u0 * P0[2] - P0[0], v0 * P0[2] - P0[1], u1 * P1[2] - P1[0], v1 * P1[2] - P1[1]])
        X = np.linalg.svd(A)[2][-1]
        X = X / np.linalg.norm(X)
        out.append(-X if X[3] < 0 else X)
    return np.array(out).reshape(-1, 4)


def pose_candidates(E):
    U, _, Vt = np.linalg.svd(np.asarray(E, float).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2] / np.linalg.norm(U[:, 2])
    return [np.c_[R1, t], np.c_[R2, t], np.c_[R1, -t], np.c_[R2, -t]]


def count_in_front(P, x1, x2):
    if len(x1) == 0:
        return 0
    X = triangulate(np.eye(3, 4), P, x1, x2)
    ok = X[:, 3] > 0
    Xe = X[:, :3] / np.where(ok, X[:, 3], 1.0)[:, None]
    max_depth = 1000.0 * np.linalg.norm(P[:, :3].T @ P[:, 3])
    d1 = Xe[:, 2]
    d2 = (Xe @ P[2, :3] + P[2, 3]) * np.linalg.norm(P[:, 2])
    return int((ok & (d1 > DBL_EPS) & (d1 < max_depth) & (d2 > DBL_EPS) & (d2 < max_depth)).sum())


def recover_pose(E, x1, x2):
    """COLMAP's PoseFromEssentialMatrix: the candidate with the most points in front (ties: the later) -> (pose [3,4], count)"""
    best, bestf = None, -1
    for P in pose_candidates(E):
        f = count_in_front(P, x1, x2)
        if f >= bestf:
            best, bestf = P, f
    return best, bestf


# ---------------------------------------------------------------------------------------------------------------- RANSAC
def relative_pose(uv0, uv1, K0, K1, max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.01, min_num_trials=1000,
                  max_num_trials=100000, seed=0):
    """one pair -> dict(E, pose, inliers, num_inliers, trials, best_trial, success)"""
    x1, x2 = normalised(uv0, K0), normalised(uv1, K1)
    n = len(x1)
    thr2 = threshold2(K0, K1, max_error_px)
    cap = max_trials_eff(confidence, min_inlier_ratio, max_num_trials)
    min_t = min(min_num_trials, cap)
    best_key, best_E, trials = 0, None, 0
    if n >= 5:
        while True:
            for tl in range(ROUND):
                t = trials + tl
                s = sample(seed, t, n)
                if s is None:
                    continue
                for slot, E in enumerate(five_point(x1[s], x2[s])):
                    c = int(inliers_of(E, x1, x2, thr2).sum())
                    key = (c << 32) | (0xFFFFFFFF - (t * MAX_SOL + slot)) if c > 0 else 0
                    if key > best_key:
                        best_key, best_E = key, E
            trials += ROUND
            if trials >= num_trials((best_key >> 32) / n, confidence, min_t, cap) or trials >= cap:
                break
    if best_key == 0:
        return dict(E=np.zeros((3, 3)), pose=np.eye(3, 4), inliers=np.zeros(n, bool), num_inliers=0, trials=trials, best_trial=-1,
                    success=False)
    E = best_E
    inl = inliers_of(E, x1, x2, thr2)
    cur = int(inl.sum())
    for _ in range(LO_ITERS):
        if cur < 5:
            break
        cands = solve_from_basis(local_basis(x1[inl], x2[inl]))
        counts = [int(inliers_of(C, x1, x2, thr2).sum()) for C in cands]
        if not cands:
            break
        b = int(np.argmax(counts))             # the first of the largest
        if counts[b] < cur:
            break
        new = inliers_of(cands[b], x1, x2, thr2)
        changed = bool((new != inl).any())
        E, inl, cur = cands[b], new, counts[b]
        if not changed:
            break
    pose, front = recover_pose(E, x1[inl], x2[inl])
    ok = cur >= 5 and front > 0
    return dict(E=E, pose=pose if ok else np.eye(3, 4), inliers=inl, num_inliers=cur, trials=trials,
                best_trial=(0xFFFFFFFF - (best_key & 0xFFFFFFFF)) // MAX_SOL, success=ok)
