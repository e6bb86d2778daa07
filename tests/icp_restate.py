"""numpy restatement of ls2fm.metrics.icp, written for this project (no device, no torch): the rule of include/ls2fm.h's ICP section.

  transform      p' = s ((R_i0 x + R_i1 y) + R_i2 z) + t_i in fp64 in the stated association, then one rounding to fp32
  pairs          metrics_restate.nearest (the distance rule) on the distinct p' -- a pair is a pure function of the query, so equal
                 queries share one search
  terms          the 36 per-pair terms in fp64 in the stated association, and their absolute values
  solve_chol     the stated Cholesky order (lm_math::chol_solve);  solve_numpy  numpy.linalg.solve: the two routes
  update         Rodrigues' formula, k = 1 + expm1(lambda), s <- k s, R <- E R, t <- k (E t) + upsilon
  step / run     one iteration / the loop with the status rules
A transform is a tuple (s float, R float64 [3, 3], t float64 [3])."""
import math

import numpy as np

import metrics_restate as MR

F32 = np.float32
RUNNING, CONVERGED, DEGENERATE = 0, 1, 2


def identity():
    return 1.0, np.eye(3), np.zeros(3)


def transform(src, T):
    """(p' float64 [n, 3] before the rounding, p' float32 [n, 3])"""
    s, R, t = T
    p = np.asarray(src, F32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        cols = [np.float64(s) * ((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)]
        p64 = np.stack(cols, axis=1)
        return p64, p64.astype(F32)


def pairs(pf, dst, max_dist):
    """(idx int32 [n], d2 float32 [n]) of the fp32 points pf against dst by the distance rule; -1 / +inf without a pair (a NaN or
    infinite p' has none)"""
    pf = np.ascontiguousarray(pf, F32).reshape(-1, 3)
    if len(pf) == 0:
        return np.zeros(0, np.int32), np.zeros(0, F32)
    u = pf.view(np.uint32)
    order = np.lexsort((u[:, 2], u[:, 1], u[:, 0]))
    first = np.ones(len(u), bool)
    first[1:] = (u[order][1:] != u[order][:-1]).any(axis=1)
    inverse = np.empty(len(u), np.int64)
    inverse[order] = np.cumsum(first) - 1
    idx, d2 = MR.nearest(pf[order][first], dst, max_dist)
    return idx[inverse], d2[inverse]


def jacobians(p, q, normals=None):
    """J float64 [n, rows, 7] and r float64 [n, rows] of the pairs (p', q), both fp32 widened; rows = 3 point to point, 1 point to
    plane (normals float32 [n, 3] of the matched references)"""
    p, q = np.asarray(p, F32).astype(np.float64), np.asarray(q, F32).astype(np.float64)
    n = len(p)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    d = p - q
    zero, one = np.zeros(n), np.ones(n)
    if normals is None:
        J = np.stack([np.stack([zero, pz, -py, one, zero, zero, px], axis=1),
                      np.stack([-pz, zero, px, zero, one, zero, py], axis=1),
                      np.stack([py, -px, zero, zero, zero, one, pz], axis=1)], axis=1)
        return J, d
    nn = np.asarray(normals, F32).astype(np.float64)
    nx, ny, nz = nn[:, 0], nn[:, 1], nn[:, 2]
    J = np.stack([py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz, (nx * px + ny * py) + nz * pz], axis=1)[:, None, :]
    r = ((nx * d[:, 0] + ny * d[:, 1]) + nz * d[:, 2])[:, None]
    return J, r


def terms(p, q, normals=None):
    """float64 [n, 36]: per pair the 28 entries of the upper triangle of J^T J row-major, the 7 of J^T r, |r|^2; over three rows a
    term is (row 0 + row 1) + row 2, every operation one rounded fp64 operation"""
    J, r = jacobians(p, q, normals)
    rows = J.shape[1]

    def dot(a, b):
        t = a[:, 0] * b[:, 0]
        if rows == 3:
            t = (t + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        return t

    with np.errstate(all="ignore"):
        out = [dot(J[:, :, a], J[:, :, b]) for a in range(7) for b in range(a, 7)]
        out += [dot(J[:, :, a], r) for a in range(7)]
        out.append(dot(r, r))
    return np.stack(out, axis=1) if len(J) else np.zeros((0, 36))


def system(sums, with_scale):
    """(H [m, m] symmetric, g [m]) of the 36 sums; m = 7 with scale, else the leading 6"""
    m = 7 if with_scale else 6
    H = np.zeros((7, 7))
    q = 0
    for a in range(7):
        for b in range(a, 7):
            H[a, b] = H[b, a] = sums[q]
            q += 1
    return H[:m, :m].copy(), np.asarray(sums[28:28 + m], np.float64).copy()


def solve_chol(sums, with_scale):
    """delta [m] by the stated order (lm_math::chol_solve with lam = 0), or None for a pivot <= 0 or a delta that is not finite"""
    H, g = system(sums, with_scale)
    m = len(g)
    L = [[0.0] * m for _ in range(m)]
    for r in range(m):
        for c in range(r, m):
            L[c][r] = float(H[r, c]) + 0.0
    ok = True
    for j in range(m):
        d = L[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k]
        ok = ok and d > 0.0
        ljj = math.sqrt(d if d > 0.0 else 1.0)
        L[j][j] = ljj
        for i in range(j + 1, m):
            s = L[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s / ljj
    z = [0.0] * m
    for i in range(m):
        s = -float(g[i])
        for k in range(i):
            s -= L[i][k] * z[k]
        z[i] = s / L[i][i]
    x = [0.0] * m
    for i in range(m - 1, -1, -1):
        s = z[i]
        for k in range(i + 1, m):
            s -= L[k][i] * x[k]
        x[i] = s / L[i][i]
    x = np.array(x)
    return x if ok and np.isfinite(x).all() else None


def solve_numpy(sums, with_scale):
    """delta [m] by numpy.linalg (LAPACK's pivoted LU), None where the matrix is not positive definite or delta is not finite"""
    H, g = system(sums, with_scale)
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return None
    try:
        np.linalg.cholesky(H)
        x = np.linalg.solve(H, -g)
    except np.linalg.LinAlgError:
        return None
    return x if np.isfinite(x).all() else None


def rodrigues(w):
    w0, w1, w2 = (float(v) for v in w)
    th2 = (w0 * w0 + w1 * w1) + w2 * w2
    A, Bc = 1.0, 0.0
    if th2 >= 1e-30:
        th = math.sqrt(th2)
        A = math.sin(th) / th
        Bc = (1.0 - math.cos(th)) / th2
    K = [[0.0, -w2, w1], [w2, 0.0, -w0], [-w1, w0, 0.0]]
    E = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j]
            E[i, j] = ((1.0 if i == j else 0.0) + A * K[i][j]) + Bc * kk
    return E


def update(T, delta, with_scale):
    """the transform after the left perturbation delta = (omega, upsilon[, lambda])"""
    s, R, t = T
    E = rodrigues(delta[:3])
    k = 1.0 + math.expm1(float(delta[6])) if with_scale else 1.0
    Rn, tn = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            Rn[i, j] = (E[i, 0] * R[0, j] + E[i, 1] * R[1, j]) + E[i, 2] * R[2, j]
        tn[i] = k * ((E[i, 0] * t[0] + E[i, 1] * t[1]) + E[i, 2] * t[2]) + float(delta[3 + i])
    return k * float(s), Rn, tn


LANES, MAX_GROUPS = 512, 512          # the stated launch shape: min(ceil(n_src / 512), 512) workgroups of 512 lanes


def ordered_sum(tm, has):
    """The 36 sums in the STATED order of include/ls2fm.h, from the terms tm [n_pairs, 36] of the source points with has [n_src]:
    point i belongs to lane i mod (groups x 512) and a lane adds its points in index order (a point without a pair adds nothing);
    the 64 lanes of a wave are added by the xor butterfly 32, 16, ..., 1, the 8 waves of a workgroup in index order, the workgroups'
    rows in row order.  Every addition is one rounded fp64 operation."""
    n = len(has)
    groups = max(1, min(-(-n // LANES), MAX_GROUPS))
    lanes = groups * LANES
    passes = max(1, -(-n // lanes))
    full = np.zeros((passes * lanes, tm.shape[1]))
    full[np.nonzero(has)[0]] = tm
    full = full.reshape(passes, lanes, -1)
    with np.errstate(all="ignore"):
        acc = np.zeros((lanes, tm.shape[1]))
        for p in range(passes):
            acc = acc + full[p]
        v = acc.reshape(groups, LANES // 64, 64, -1)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ o, :]
        waves = v[:, :, 0, :]
        rows = waves[:, 0, :]
        for w in range(1, LANES // 64):
            rows = rows + waves[:, w, :]
        out = np.zeros(tm.shape[1])
        for r in range(groups):
            out = out + rows[r]
    return out


def accumulate(src, dst, normals, T, max_dist):
    """dict(pair_idx, pair_d2, n_pairs, sums [36]: the stated order (ordered_sum), plain_sums [36]: the same terms added by numpy in
    its own order, abs_sums [36]: the sums of the terms' absolute values) at the transform T"""
    _, pf = transform(src, T)
    idx, d2 = pairs(pf, dst, max_dist)
    has = idx >= 0
    q = np.asarray(dst, F32).reshape(-1, 3)[idx[has]]
    tm = terms(pf[has], q, None if normals is None else np.asarray(normals, F32)[idx[has]])
    return dict(pair_idx=idx, pair_d2=d2, n_pairs=int(has.sum()), sums=ordered_sum(tm, has), plain_sums=tm.sum(axis=0),
                abs_sums=np.abs(tm).sum(axis=0))


def step(src, dst, normals, T, max_dist, with_scale, tol_rot, tol_trans):
    """one iteration from T: accumulate's dict plus, per solve route ("chol": the stated order, "numpy": numpy.linalg), delta (None
    if degenerate), T_new (T itself if degenerate) and status as dicts over the route; kappa: the 2-norm condition number of H"""
    out = accumulate(src, dst, normals, T, max_dist)
    out.update(solve_step(out["sums"], out["n_pairs"], T, with_scale, tol_rot, tol_trans))
    return out


def solve_step(sums, n_pairs, T, with_scale, tol_rot, tol_trans):
    """the solve and the update of one iteration from the 36 sums and the pair count, by both routes: dict(delta, T_new, status: dicts
    over "chol" / "numpy"; kappa)"""
    m = 7 if with_scale else 6
    out = dict(sums=np.asarray(sums, np.float64), n_pairs=int(n_pairs), delta={}, T_new={}, status={}, kappa=float("inf"))
    for name, route in (("chol", solve_chol), ("numpy", solve_numpy)):
        delta = route(out["sums"], with_scale) if out["n_pairs"] >= m else None
        out["delta"][name] = delta
        if delta is None:
            out["T_new"][name], out["status"][name] = T, DEGENERATE
            continue
        lam = abs(delta[6]) if with_scale else 0.0
        rot, trans = max(np.abs(delta[:3]).max(), lam), np.abs(delta[3:6]).max()
        out["T_new"][name] = update(T, delta, with_scale)
        out["status"][name] = CONVERGED if rot <= tol_rot and trans <= tol_trans else RUNNING
    if out["delta"]["chol"] is not None:
        out["kappa"] = float(np.linalg.cond(system(out["sums"], with_scale)[0]))
    return out


def run(src, dst, normals, T, max_dist, with_scale, iters, tol_rot, tol_trans, route="chol"):
    """the loop, following one solve route: dict(T (final), status, iterations, steps: the list of step dicts, steps[k] taken from
    T_k).  A degenerate step is not counted and leaves T; a converged one is applied and counted."""
    steps, status, done = [], RUNNING, 0
    for _ in range(iters):
        st = step(src, dst, normals, T, max_dist, with_scale, tol_rot, tol_trans)
        steps.append(st)
        status = st["status"][route]
        if status == DEGENERATE:
            break
        T, done = st["T_new"][route], done + 1
        if status == CONVERGED:
            break
    return dict(T=T, status=status, iterations=done, steps=steps)


def apply(T, points):
    s, R, t = T
    return s * (np.asarray(points, np.float64) @ np.asarray(R).T) + np.asarray(t)


def flat(T):
    """float64 [13]: s, R row-major, t"""
    return np.concatenate([[float(T[0])], np.asarray(T[1], np.float64).reshape(-1), np.asarray(T[2], np.float64).reshape(-1)])
