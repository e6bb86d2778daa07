"""Seeded synthetic 640 x 480 two-view scenes for the two-view geometry tests (numpy only): a general 3-D scene, a planar scene,
a pure rotation, and minimal problems with their true F / H.  One pinhole camera (f 600, centre 320 / 240) for both views, as in
the relative-pose tests."""
import numpy as np

import twoview_restate as TV

F_PX, CX, CY = 600.0, 320.0, 240.0
INTR = (F_PX, F_PX, CX, CY)
K = np.array([[F_PX, 0.0, CX], [0.0, F_PX, CY], [0.0, 0.0, 1.0]])
K_INV = np.linalg.inv(K)
FAR2 = 400.0 * 16.0                # an outlier's squared error: at least 20 x the 4 px threshold


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def rotation(rng, deg):
    w = rng.normal(size=3)
    w /= np.linalg.norm(w)
    a = np.radians(deg)
    W = skew(w)
    return np.eye(3) + np.sin(a) * W + (1.0 - np.cos(a)) * (W @ W)


def project(X):
    return (X / X[:, 2:]) @ K.T[:, :2]


def true_f(R, t):
    return TV.canonical(K_INV.T @ skew(t) @ R @ K_INV).reshape(3, 3)


def _motion(rng):
    t = rng.normal(size=3)
    return rotation(rng, rng.uniform(5, 20)), t / np.linalg.norm(t)


def _points(rng, n, R, t, depth):
    """n points in front of both cameras; depth(x, y) gives z"""
    X = np.zeros((0, 3))
    while len(X) < n:
        xy = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n)], axis=1)
        C = np.c_[xy, depth(rng, xy)]
        X = np.concatenate([X, C[(C @ R.T + t)[:, 2] > 1.0]])
    return X[:n]


def _add_outliers(rng, uv0, uv1, outlier_ratio, err2):
    """replace a share of uv1 by random pixels whose TRUE squared error err2(uv0_i, pixel) is >= FAR2 (redrawn up to 1000 times,
    the farthest draw kept and labelled by its true error) -> inlier truth"""
    n = len(uv0)
    truth = np.ones(n, bool)
    for i in rng.choice(n, int(round(outlier_ratio * n)), replace=False):
        best, bs = None, -1.0
        for _ in range(1000):
            cand = rng.uniform((0, 0), (640, 480))
            s = float(err2(uv0[i], cand))
            if s > bs:
                best, bs = cand, s
            if s >= FAR2:
                break
        uv1[i] = best
        truth[i] = not (bs > 16.0)
    return truth


def general_scene(rng, n, outlier_ratio=0.0, sigma=0.0):
    """camera 2 = [R | t] (|t| = 1, rotation 5-20 degrees), points 4-10 units deep -> (uv0, uv1, true unit F, truth, [R | t])"""
    R, t = _motion(rng)
    X = _points(rng, n, R, t, lambda g, xy: g.uniform(4, 10, len(xy)))
    uv0, uv1 = project(X), project(X @ R.T + t)
    if sigma:
        uv0, uv1 = uv0 + rng.normal(size=uv0.shape) * sigma, uv1 + rng.normal(size=uv1.shape) * sigma
    F = true_f(R, t)
    truth = _add_outliers(rng, uv0, uv1, outlier_ratio, lambda a, b: TV.RR.sampson2(F, a[None], b[None])[0])
    return uv0, uv1, F, truth, np.c_[R, t]


def _transfer2(H):
    def err2(a, b):
        q = H @ np.array([a[0], a[1], 1.0])
        return ((q[:2] / q[2] - b) ** 2).sum()
    return err2


def planar_scene(rng, n, outlier_ratio=0.0, sigma=0.0):
    """the same motion over points of the plane z = 6 + 0.3 x + 0.2 y -> (uv0, uv1, true unit H, truth)"""
    R, t = _motion(rng)
    X = _points(rng, n, R, t, lambda g, xy: 6.0 + 0.3 * xy[:, 0] + 0.2 * xy[:, 1])
    nrm, d = np.array([-0.3, -0.2, 1.0]), 6.0                      # nrm . X = d
    H = TV.canonical(K @ (R + np.outer(t, nrm) / d) @ K_INV).reshape(3, 3)
    uv0, uv1 = project(X), project(X @ R.T + t)
    if sigma:
        uv0, uv1 = uv0 + rng.normal(size=uv0.shape) * sigma, uv1 + rng.normal(size=uv1.shape) * sigma
    truth = _add_outliers(rng, uv0, uv1, outlier_ratio, _transfer2(H))
    return uv0, uv1, H, truth


def rotation_scene(rng, n, sigma=0.0):
    """pure rotation (no baseline) over a general 3-D scene -> (uv0, uv1)"""
    R = rotation(rng, rng.uniform(5, 15))
    X = _points(rng, n, R, np.zeros(3), lambda g, xy: g.uniform(4, 10, len(xy)))
    uv0, uv1 = project(X), project(X @ R.T)
    if sigma:
        uv0, uv1 = uv0 + rng.normal(size=uv0.shape) * sigma, uv1 + rng.normal(size=uv1.shape) * sigma
    return uv0, uv1


def seven_point_problems(rng, m):
    """m noise-free two-camera problems (rotation up to 60 degrees) -> (uv0 [m,7,2], uv1 [m,7,2], true unit F [m,3,3])"""
    a, b, Fs = [], [], []
    while len(a) < m:
        R, t = rotation(rng, rng.uniform(0, 60)), rng.normal(size=3)
        t /= np.linalg.norm(t)
        X1 = np.concatenate([rng.uniform(-1, 1, (7, 2)), rng.uniform(2, 6, (7, 1))], axis=1)
        X2 = X1 @ R.T + t
        if (X2[:, 2] > 0.5).all():
            a.append(project(X1))
            b.append(project(X2))
            Fs.append(true_f(R, t))
    return np.array(a), np.array(b), np.array(Fs)


def four_point_problems(rng, m):
    """m noise-free problems: random pixels through a random near-identity homography -> (uv0 [m,4,2], uv1, true unit H)"""
    a, b, Hs = [], [], []
    while len(a) < m:
        H = K @ (np.eye(3) + rng.normal(size=(3, 3)) * 0.1) @ K_INV
        p = rng.uniform((0, 0), (640, 480), (4, 2))
        q = np.c_[p, np.ones(4)] @ H.T
        if (q[:, 2] > 0.2).all():
            a.append(p)
            b.append(q[:, :2] / q[:, 2:])
            Hs.append(TV.canonical(H).reshape(3, 3))
    return np.array(a), np.array(b), np.array(Hs)


def degenerate_seven(rng):
    """coincident correspondences, all zeros, NaN -> (uv0 [3,7,2], uv1)"""
    a, b, _ = seven_point_problems(rng, 3)
    a[0, 1], b[0, 1] = a[0, 0], b[0, 0]
    a[1], b[1] = 0.0, 0.0
    a[2] = np.nan
    return a, b


def degenerate_four(rng):
    """coincident correspondences, three collinear points (in both images: they go through the true H), all zeros, NaN"""
    a, b, Hs = four_point_problems(rng, 4)
    a[0, 1], b[0, 1] = a[0, 0], b[0, 0]
    a[1, 2] = 0.25 * a[1, 0] + 0.75 * a[1, 1]
    q = Hs[1] @ np.array([a[1, 2, 0], a[1, 2, 1], 1.0])
    b[1, 2] = q[:2] / q[2]
    a[2], b[2] = 0.0, 0.0
    a[3] = np.nan
    return a, b
