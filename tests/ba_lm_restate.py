"""float64 restatement of the Levenberg-Marquardt bundle adjustment (ls2fm.stage.LMBALoop / csrc/bundle_adjust_lm.hip; the rules are in
include/ls2fm.h), written in numpy for this project, by TWO routes on the same linearization:

    (a) "schur"  eliminate the points, the reduced camera system by numpy.linalg.cholesky, back-substitution
    (b) "full"   the damped normal equations over ALL parameters (6 V + 3 P), numpy.linalg.solve

The gap between the two routes on the same state is the yardstick of the tests (`within_gap`): two correctly rounded evaluations can
each sit one gap from the truth, doubled for headroom (MARGIN, as ba_restate.MARGIN), with a floor of 16 fp64 spacings of the
quantity's largest magnitude.  Also the scenes both test files share."""
import numpy as np

LOSSES = ("trivial", "soft_l1", "cauchy")
MARGIN = 4.0
FLOOR_SPACINGS = 16.0
REASONS = {0: "running", 1: "gradient", 2: "step", 3: "lambda"}


# ------------------------------------------------------------------------------------------------------------ the model
def residuals(poses, X, op, ov, uv, k4, loss, c):
    """-> x_c [n,3], r [n,2], rho [n], w [n]"""
    fx, fy, cx, cy = k4
    R, t = poses[ov][:, :, :3], poses[ov][:, :, 3]
    xc = np.einsum("nij,nj->ni", R, X[op]) + t
    with np.errstate(all="ignore"):
        r = np.stack([fx * xc[:, 0] / xc[:, 2] + cx - uv[:, 0], fy * xc[:, 1] / xc[:, 2] + cy - uv[:, 1]], axis=1)
        s = (r * r).sum(1)
        c2 = c * c
        if loss == "trivial":
            rho, w = s, np.ones_like(s)
        elif loss == "soft_l1":
            q = np.sqrt(1.0 + s / c2)
            rho, w = 2.0 * c2 * (q - 1.0), 1.0 / q
        elif loss == "cauchy":
            rho, w = c2 * np.log1p(s / c2), 1.0 / (1.0 + s / c2)
        else:
            raise ValueError(loss)
    return xc, r, rho, w


def cost_of(poses, X, op, ov, uv, k4, loss, c):
    return 0.5 * float(residuals(poses, X, op, ov, uv, k4, loss, c)[2].sum())


def point_constant(op, P, min_point_views=2):
    return np.bincount(op, minlength=P) < min_point_views


def jacobians(poses, xc, op, ov, k4, view_const, point_const):
    """J_c [n,2,6] for the perturbation d x_c = -[x_c]x omega + dt, J_p = J_proj R [n,2,3]"""
    fx, fy = k4[0], k4[1]
    n = xc.shape[0]
    x, y, z = xc[:, 0], xc[:, 1], xc[:, 2]
    with np.errstate(all="ignore"):
        Jproj = np.zeros((n, 2, 3))
        Jproj[:, 0, 0], Jproj[:, 0, 2] = fx / z, -fx * x / (z * z)
        Jproj[:, 1, 1], Jproj[:, 1, 2] = fy / z, -fy * y / (z * z)
        skew = np.zeros((n, 3, 3))
        skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 0], skew[:, 1, 2], skew[:, 2, 0], skew[:, 2, 1] = -z, y, z, -x, -y, x
        Jc = np.concatenate([-np.einsum("nij,njk->nik", Jproj, skew), Jproj], axis=2)
        Jp = np.einsum("nij,njk->nik", Jproj, poses[ov][:, :, :3])
    Jc[view_const[ov]] = 0.0
    Jp[point_const[op]] = 0.0
    return Jc, Jp


def damp(B, lam):
    d = np.diagonal(B, axis1=-2, axis2=-1)
    add = lam * np.maximum(d, 1e-12 * d.max(axis=-1, keepdims=True))
    out = B.copy()
    k = np.arange(B.shape[-1])
    out[..., k, k] += add
    return out


def linearize(poses, X, op, ov, uv, k4, loss, c, view_const, point_const):
    V, P = poses.shape[0], X.shape[0]
    xc, r, rho, w = residuals(poses, X, op, ov, uv, k4, loss, c)
    Jc, Jp = jacobians(poses, xc, op, ov, k4, view_const, point_const)
    U, gc, Vp, gp = np.zeros((V, 6, 6)), np.zeros((V, 6)), np.zeros((P, 3, 3)), np.zeros((P, 3))
    with np.errstate(all="ignore"):
        np.add.at(U, ov, w[:, None, None] * np.einsum("nki,nkj->nij", Jc, Jc))
        np.add.at(gc, ov, w[:, None] * np.einsum("nki,nk->ni", Jc, r))
        np.add.at(Vp, op, w[:, None, None] * np.einsum("nki,nkj->nij", Jp, Jp))
        np.add.at(gp, op, w[:, None] * np.einsum("nki,nk->ni", Jp, r))
        W = w[:, None, None] * np.einsum("nki,nkj->nij", Jc, Jp)
    gmax = max(float(np.abs(gc).max()), float(np.abs(gp[~point_const]).max()) if (~point_const).any() else 0.0)
    seen = np.unique(op)
    pmax = max(float(np.abs(poses[:, :, 3]).max()), float(np.abs(X[seen]).max()))
    return dict(U=U, gc=gc, Vp=Vp, gp=gp, W=W, Jc=Jc, Jp=Jp, r=r, w=w, rho=rho, cost=0.5 * float(rho.sum()), gmax=gmax, pmax=pmax)


def _finite(*arrays):
    return all(np.isfinite(a).all() for a in arrays)


def step_schur(lin, lam, op, ov, view_const, point_const):
    """route (a) -> (delta_c [V,6], delta_p [P,3]) or None after a non-positive (or non-finite) pivot"""
    V, P = lin["U"].shape[0], lin["Vp"].shape[0]
    free = ~point_const
    Vs = damp(lin["Vp"], lam)
    Vinv = np.zeros((P, 3, 3))
    if not _finite(Vs, lin["U"], lin["W"]):
        return None
    try:
        for p in np.nonzero(free)[0]:
            L = np.linalg.cholesky(Vs[p])
            Li = np.linalg.inv(L)
            Vinv[p] = Li.T @ Li
    except np.linalg.LinAlgError:
        return None
    Us = damp(lin["U"], lam)
    S = np.zeros((6 * V, 6 * V))
    b = np.zeros(6 * V)
    for v in range(V):
        if view_const[v]:
            S[6 * v:6 * v + 6, 6 * v:6 * v + 6] = np.eye(6)
        else:
            S[6 * v:6 * v + 6, 6 * v:6 * v + 6] = Us[v]
            b[6 * v:6 * v + 6] = -lin["gc"][v]
    Wd = np.zeros((6 * V, P, 3))                                  # W as a dense [6 V, 3 P]: test-scale scenes only
    for o in range(len(op)):
        Wd[6 * ov[o]:6 * ov[o] + 6, op[o]] = lin["W"][o]
    Y = np.einsum("apk,pkl->apl", Wd, Vinv)
    S -= np.einsum("apk,bpk->ab", Y, Wd)
    b += np.einsum("apk,pk->a", Y, lin["gp"])
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    dc = np.linalg.solve(L.T, np.linalg.solve(L, b))
    s = lin["gp"] + np.einsum("apk,a->pk", Wd, dc)
    dp = -np.einsum("pkl,pl->pk", Vinv, s)
    return dc.reshape(V, 6), dp


def full_system(lin, op, ov, view_const, point_const):
    """route (b)'s own linearization: H = (sqrt(w) J)^T (sqrt(w) J) and g = (sqrt(w) J)^T sqrt(w) r over all 6 V + 3 P parameters
    as matrix products of the whole Jacobian (another order of every sum than route (a)'s blocks) -> (H, g, const) or None"""
    V, P, n = lin["U"].shape[0], lin["Vp"].shape[0], len(op)
    N = 6 * V + 3 * P
    J = np.zeros((2 * n, N))
    with np.errstate(all="ignore"):
        sw = np.sqrt(lin["w"])
        for o in range(n):
            J[2 * o:2 * o + 2, 6 * ov[o]:6 * ov[o] + 6] = sw[o] * lin["Jc"][o]
            J[2 * o:2 * o + 2, 6 * V + 3 * op[o]:6 * V + 3 * op[o] + 3] = sw[o] * lin["Jp"][o]
        rw = (sw[:, None] * lin["r"]).reshape(-1)
    if not _finite(J, rw):
        return None
    const = np.concatenate([np.repeat(view_const, 6), np.repeat(point_const, 3)])
    return J.T @ J, J.T @ rw, const


def full_gradient(lin, op, ov, view_const, point_const):
    sys_ = full_system(lin, op, ov, view_const, point_const)
    return None if sys_ is None else sys_[1]


def step_full(lin, lam, op, ov, view_const, point_const):
    """route (b): the damped normal equations over all parameters, numpy.linalg.solve"""
    V, P = lin["U"].shape[0], lin["Vp"].shape[0]
    N = 6 * V + 3 * P
    sys_ = full_system(lin, op, ov, view_const, point_const)
    if sys_ is None:
        return None
    H, g, const = sys_
    # damping per block: the largest diagonal entry of the parameter's own 6 x 6 or 3 x 3
    d = np.diagonal(H).copy()
    blk = np.concatenate([np.repeat(d[:6 * V].reshape(V, 6).max(1), 6), np.repeat(d[6 * V:].reshape(P, 3).max(1), 3)])
    H[np.arange(N), np.arange(N)] += lam * np.maximum(d, 1e-12 * blk)
    H[const, :] = 0.0
    H[:, const] = 0.0
    H[const, const] = 1.0
    g[const] = 0.0
    if not _finite(H):
        return None
    try:
        np.linalg.cholesky(H)                                       # positive definite <=> every V_p* and S are
    except np.linalg.LinAlgError:
        return None
    d = np.linalg.solve(H, -g)
    return d[:6 * V].reshape(V, 6), d[6 * V:].reshape(P, 3)


STEPS = dict(schur=step_schur, full=step_full)


def pose_update(P, d):
    """R <- exp([w]x) R, t <- exp([w]x) t + dt (csrc/lm_math.h)"""
    w = d[:3]
    th2 = float(w @ w)
    A, B = 1.0, 0.0
    if th2 >= 1e-30:
        th = np.sqrt(th2)
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    C = (np.eye(3) + A * K + B * (K @ K)) @ P
    C[:, 3] += d[3:]
    return C


def candidate(poses, X, dc, dp, view_const):
    cand = poses.copy()
    for v in range(poses.shape[0]):
        if not view_const[v]:
            cand[v] = pose_update(poses[v], dc[v])
    return cand, X + dp


# ------------------------------------------------------------------------------------------------------------ the loop
def new_state():
    return dict(lam=0.0, done=False, iters=0, cost=0.0, reason=0)


def iterate(route, poses, X, state, op, ov, uv, k4, view_const, loss="trivial", c=1.0, initial_lambda=1e-4, grad_tol=1e-10,
            step_tol=1e-10, min_point_views=2):
    """ONE iteration -> (row [6], poses, X, detail).  state is updated in place.  detail: dc, dp, lin (None after the stop)"""
    point_const = point_constant(op, X.shape[0], min_point_views)
    view_const = np.asarray(view_const, bool)
    if not state["lam"] > 0.0:
        state["lam"] = initial_lambda
    lam = state["lam"]
    if state["done"]:
        return np.array([state["cost"], state["cost"], lam, -1.0, 0.0, 0.0]), poses, X, None
    lin = linearize(poses, X, op, ov, uv, k4, loss, c, view_const, point_const)
    cost, gmax = lin["cost"], lin["gmax"]
    if route == "full":                       # route (b) sums the cost and forms the gradient on its own
        cost = 0.5 * float(np.sum(lin["rho"][::-1]))
        g = full_gradient(lin, op, ov, view_const, point_const)
        gmax = float(np.abs(g).max()) if g is not None else gmax
    else:
        g = np.concatenate([lin["gc"].reshape(-1), lin["gp"].reshape(-1)])
    cand_cost, dmax, acc, detail = float("nan"), 0.0, 0.0, dict(lin=lin, dc=None, dp=None, g=g)
    if gmax <= grad_tol:
        state["done"], state["reason"] = True, 1
        cand_cost = cost
    else:
        step = STEPS[route](lin, lam, op, ov, view_const, point_const)
        if step is None:
            state["lam"] = lam * 10.0
        else:
            dc, dp = step
            detail.update(dc=dc, dp=dp)
            cp, cx = candidate(poses, X, dc, dp, view_const)
            rho_c = residuals(cp, cx, op, ov, uv, k4, loss, c)[2]
            cand_cost = 0.5 * float(np.sum(rho_c[::-1] if route == "full" else rho_c))
            dmax = float(np.fmax(np.abs(dc).max(), np.abs(dp).max()))
            if cand_cost < cost:
                acc = 1.0
                poses, X = cp, cx
                state["lam"] = max(lam * 0.1, 1e-16)
                if dmax <= step_tol * (1.0 + lin["pmax"]):
                    state["done"], state["reason"] = True, 2
            else:
                state["lam"] = lam * 10.0
    if not state["done"] and state["lam"] > 1e32:
        state["done"], state["reason"] = True, 3
    state["iters"] += 1
    state["cost"] = cand_cost if acc else cost
    return np.array([cost, cand_cost, lam, acc, gmax, dmax]), poses, X, detail


def run(route, poses, X, op, ov, uv, k4, view_const, n_iters, **kw):
    """-> dict(log [n_iters, 6], poses, X, state; per row the gradient and the step as vectors, None where there is none)"""
    poses, X = np.array(poses, np.float64), np.array(X, np.float64)
    state, rows, grads, steps = new_state(), [], [], []
    for _ in range(n_iters):
        row, poses, X, d = iterate(route, poses, X, state, op, ov, uv, k4, view_const, **kw)
        rows.append(row)
        grads.append(None if d is None else d["g"])
        steps.append(None if d is None or d["dc"] is None else np.concatenate([d["dc"].reshape(-1), d["dp"].reshape(-1)]))
    return dict(log=np.stack(rows), poses=poses, X=X, state=state, grads=grads, steps=steps)


def vector_gap(a, b, key):
    """the routes' gap of the gradient / the step THEMSELVES, the largest over the rows and the elements: the yardstick of the
    log's max |g| / max |delta| columns.  Those are norms of the vectors, so they can differ by as much as the vectors do
    (| max|x| - max|y| | <= max|x - y|), while the gap of the two norms alone is small whenever the routes' largest elements
    happen to agree."""
    gaps = [float(np.abs(x - y).max()) for x, y in zip(a[key], b[key]) if x is not None and y is not None]
    return max(gaps) if gaps else 0.0


# ------------------------------------------------------------------------------------------------------------- the bar
def within_gap(name, key, mine, ref_a, ref_b, margin=MARGIN, gap=None):
    """|mine - route (a)| <= max(margin * |route (b) - route (a)|, FLOOR_SPACINGS fp64 spacings of the quantity's largest magnitude),
    maxima over the quantity's elements (NaN must meet NaN).  Prints the figures, returns the failure or None."""
    mine, ref_a, ref_b = (np.asarray(a, dtype=np.float64) for a in (mine, ref_a, ref_b))
    if not (np.isnan(mine) == np.isnan(ref_a)).all():
        return (key, "NaN pattern differs")
    ok = ~np.isnan(ref_a)
    if not ok.any():
        return None
    d = float(np.abs(mine - ref_a)[ok].max())
    gap = max(float(np.abs(ref_b - ref_a)[ok].max()), gap or 0.0)
    mag = float(np.abs(ref_a[ok]).max())
    floor = FLOOR_SPACINGS * float(np.spacing(mag))
    bar = max(margin * gap, floor)
    print(f"[{name}] {key:10s} mine-(a) {d:.3e}  (b)-(a) {gap:.3e}  {FLOOR_SPACINGS:g} spacings {floor:.2e}  bar {bar:.3e}  (largest magnitude {mag:.3e})")
    return None if d <= bar else (key, d, gap, floor)


def routes_agree(name, a, b, step_scale_tol=1e-9):
    """the scene conditions of the tests: the two routes' logs agree EXACTLY in accepted flags, lambdas and stop state, and their
    gap is at most step_scale_tol of the largest magnitude of each column"""
    la, lb = a["log"], b["log"]
    assert np.array_equal(la[:, 3], lb[:, 3]), f"{name}: accept / reject decisions differ between the routes"
    assert np.array_equal(la[:, 2], lb[:, 2]), f"{name}: lambdas differ between the routes"
    assert np.array_equal(np.isnan(la), np.isnan(lb)), f"{name}: NaN pattern of the logs"
    assert (a["state"]["done"], a["state"]["reason"], a["state"]["iters"]) == (b["state"]["done"], b["state"]["reason"], b["state"]["iters"]), name
    for col, key in ((0, "cost"), (1, "candidate"), (4, "max |g|"), (5, "max |delta|")):
        ok = ~np.isnan(la[:, col])
        gap, mag = float(np.abs(la[ok, col] - lb[ok, col]).max()), float(np.abs(la[ok, col]).max())
        print(f"[{name}] routes: {key:12s} gap {gap:.3e}  largest {mag:.3e}")
        assert gap <= step_scale_tol * max(mag, 1e-300), f"{name}: the routes' gap of {key} is {gap:.3e} at magnitude {mag:.3e}"


# ----------------------------------------------------------------------------------------------------------- the scenes
K4 = np.array([520.0, 515.0, 320.0, 240.0])


def look_at_poses(V, rng, radius=6.0):
    """V cameras on an arc looking at the origin, world to camera [V,3,4]"""
    out = np.zeros((V, 3, 4))
    for v in range(V):
        ang = (v - 0.5 * (V - 1)) * min(0.25, 2.0 / max(V, 1)) + rng.uniform(-0.02, 0.02)
        c = np.array([radius * np.sin(ang), rng.uniform(-0.3, 0.3), -radius * np.cos(ang)])
        z = -c / np.linalg.norm(c)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        out[v, :, :3], out[v, :, 3] = R, -R @ c
    return out


def project(poses, X, op, ov, k4):
    xc = np.einsum("nij,nj->ni", poses[ov][:, :, :3], X[op]) + poses[ov][:, :, 3]
    return np.stack([k4[0] * xc[:, 0] / xc[:, 2] + k4[2], k4[1] * xc[:, 1] / xc[:, 2] + k4[3]], axis=1)


def perturb(poses, X, rng, rot, trans, pts):
    out = poses.copy()
    for v in range(poses.shape[0]):
        out[v] = pose_update(poses[v], np.concatenate([rng.normal(0.0, rot, 3), rng.normal(0.0, trans, 3)]))
    return out, X + rng.normal(0.0, pts, X.shape)


def scene(counts, P, seed, noise=0.5, rot=0.01, trans=0.02, pts=0.02, unseen=0, shared_by_all=True, constant=(0, 1), k4=K4, disjoint=None,
          exact_constants=False):
    """counts[v] observations in view v over P points (the last `unseen` observed by none; point 0 by every view when shared_by_all);
    the observations of a view in random order; disjoint = (i, j): views i and j share no point.  Key points: the true projection
    + N(0, noise px); start: the true state perturbed (exact_constants: the points with one observation, which do not move, start
    at their true place).  -> dict(poses, X, op, ov, uv, view_start, view_const, k4, truth)"""
    rng = np.random.default_rng(seed)
    V = len(counts)
    Xt = rng.uniform(-1.0, 1.0, size=(P, 3))
    Pt = look_at_poses(V, rng)
    seen = P - unseen
    ids = []
    for v, cnt in enumerate(counts):
        pool = np.arange(1 if shared_by_all else 0, seen)
        if disjoint is not None and v in disjoint:
            half = (seen - 1) // 2
            pool = pool[:half] if v == disjoint[0] else pool[half:]
        k = cnt - 1 if shared_by_all else cnt
        i = rng.choice(pool, size=k, replace=False)
        if shared_by_all and not (disjoint is not None and v == disjoint[1]):
            i = np.concatenate([[0], i])
        elif shared_by_all:
            i = np.concatenate([i, rng.choice(np.setdiff1d(pool, i), size=1)])
        ids.append(i[rng.permutation(len(i))].astype(np.int64))
    op = np.concatenate(ids)
    ov = np.concatenate([np.full(len(i), v) for v, i in enumerate(ids)])
    uv = project(Pt, Xt, op, ov, k4) + rng.normal(0.0, noise, (len(op), 2))
    poses, X = perturb(Pt, Xt, rng, rot, trans, pts)
    if exact_constants:
        fixed = point_constant(op, P)
        X[fixed] = Xt[fixed]
    vc = np.zeros(V, bool)
    for v in constant:
        if v < V:
            vc[v] = True
            poses[v] = Pt[v]
    vs = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int32)
    return dict(poses=poses, X=X, op=op, ov=ov, uv=uv, view_start=vs, view_const=vc, k4=np.asarray(k4, np.float64), truth=(Pt, Xt), ids=ids)


def scene_edges(seed=7):
    """7 views with 1 / 255 / 256 / 257 observations among them (around the kernels' 256 threads), point 0 seen by every view but one,
    40 points seen by none, views 2 and 5 sharing no point.  Views 0 and 1 are constant: view 1's single observation could not hold
    six parameters, and the routes' gap would measure that instead of the arithmetic"""
    return scene((60, 1, 255, 256, 257, 120, 90), 700, seed, unseen=40, constant=(0, 1), disjoint=(2, 5))


def scene_single(seed=3):
    """V = 1: a 6 x 6 reduced system; every point has one observation, so all points are constant"""
    return scene((80,), 100, seed, constant=(), shared_by_all=False)


def scene_pair(seed=5):
    """V = 2 sharing exactly ONE point (point 0); neither view constant"""
    s = scene((40, 40), 200, seed, constant=(), disjoint=(0, 1))
    ids = s["ids"]
    assert len(np.intersect1d(ids[0], ids[1])) == 0
    s["op"] = s["op"].copy()
    s["op"][0] = 0 if 0 not in ids[0] else s["op"][0]
    s["op"][int(s["view_start"][1])] = 0
    Pt, Xt = s["truth"]
    rng = np.random.default_rng(seed + 1)
    s["uv"] = project(Pt, Xt, s["op"], s["ov"], s["k4"]) + rng.normal(0.0, 0.5, s["uv"].shape)
    assert len(np.intersect1d(s["op"][:40], s["op"][40:])) == 1
    return s


def scene_cap(seed=11, V=128):
    """the cap: 128 views x 40 observations over 600 points"""
    return scene((40,) * V, 600, seed, constant=(0, 1))


def scene_small(seed=21, **kw):
    """5 views x 60 observations over 150 points: the loops, the losses, the permutation"""
    kw.setdefault("constant", (0, 1))
    return scene((60,) * 5, 150, seed, **kw)


def scene_pivot(seed=38):
    """initial_lambda = 1e-12: a far start (the first undamped steps overshoot and are REJECTED on their cost) and one extra view
    whose reduced block loses its damping exactly when lambda reaches its floor of 1e-16: the view is the identity, sees ONE point,
    (0, 0, 1), at exactly the principal point, with fx = fy = 512, so every entry of its U is 0 or +-2^18, its gradient is exactly 0
    (it never moves) and the point is constant (one observation).  2^18 (1 + lambda) rounds to 2^18 for lambda < 2^-53, and the
    fourth pivot of the block is then 2^18 - 512 * 512 = 0 in every evaluation order: a non-positive pivot, whichever route."""
    k4 = np.array([512.0, 512.0, 320.0, 240.0])
    s = scene((60,) * 4, 120, seed, rot=0.1, trans=0.3, pts=0.5, constant=(0, 1), k4=k4)
    V, P = s["poses"].shape[0], s["X"].shape[0]
    s["poses"] = np.concatenate([s["poses"], np.eye(3, 4)[None]])
    s["X"] = np.concatenate([s["X"], np.array([[0.0, 0.0, 1.0]])])
    s["op"] = np.concatenate([s["op"], [P]])
    s["ov"] = np.concatenate([s["ov"], [V]])
    s["uv"] = np.concatenate([s["uv"], [[320.0, 240.0]]])
    s["view_start"] = np.concatenate([s["view_start"], [len(s["op"])]]).astype(np.int32)
    s["view_const"] = np.concatenate([s["view_const"], [False]])
    return s


def lists_of(s):
    """per view: key points [n_v, 2] and point ids [n_v] (what ls2fm.stage.TrackedViews takes)"""
    vs = s["view_start"]
    return [s["uv"][vs[v]:vs[v + 1]] for v in range(len(vs) - 1)], [s["op"][vs[v]:vs[v + 1]] for v in range(len(vs) - 1)]


# ------------------------------------------------------------------------------------- what both test files run, stated once
LOOP_KW = dict(step_tol=1e-5)             # the loops stop on the step rule before a cost comparison is decided by rounding
PIVOT_KW = dict(initial_lambda=1e-12, grad_tol=0.0, step_tol=0.0)
PIVOT_ITERS = 9
SCENES = dict(edges=scene_edges, single=scene_single, pair=scene_pair, small=scene_small)
_CACHE = {}


def reference(name, n_iters, **kw):
    """(scene, route (a), route (b)) of a named scene, computed once per process and shared (the results are not modified)"""
    key = (name, n_iters, tuple(sorted(kw.items())))
    if key not in _CACHE:
        s = (SCENES.get(name) or globals()["scene_" + name])()
        args = (s["poses"], s["X"], s["op"], s["ov"], s["uv"], s["k4"], s["view_const"], n_iters)
        _CACHE[key] = (s, run("schur", *args, **kw), run("full", *args, **kw))
    return _CACHE[key]


def variant_reference(kind, n_iters=3):
    """scene_small with every view constant ("points only") or every point constant ("poses only": min_point_views above every
    count) -> (scene, loop keywords, route (a), route (b)), computed once"""
    key = ("variant", kind, n_iters)
    if key not in _CACHE:
        s = scene_small()
        args = (s["poses"], s["X"], s["op"], s["ov"], s["uv"], s["k4"])
        if kind == "points only":
            vc, rkw, kw = np.ones(5, bool), {}, dict(constant_views=range(5))
        else:
            vc, rkw, kw = s["view_const"], dict(min_point_views=6), dict(min_point_views=6)
        _CACHE[key] = (s, kw, run("schur", *args, vc, n_iters, **rkw), run("full", *args, vc, n_iters, **rkw))
    return _CACHE[key]


def views_of(s, device="cpu"):
    """the scene as the object LMBALoop reads (poses [V,3,4], K [3,3], per-view key points and point ids, points), fp64"""
    import types
    import torch
    kps, ids = lists_of(s)
    k = s["k4"]
    K = torch.tensor([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return types.SimpleNamespace(poses=torch.tensor(s["poses"], device=device), intrinsic=K.to(device), host_intrinsic=K,
                                 keypoints=[torch.tensor(a, device=device) for a in kps],
                                 track_ids=[torch.tensor(a, device=device) for a in ids], xyzs=torch.tensor(s["X"], device=device))


def build_loop(s, device="cpu", **kw):
    from ls2fm import stage
    kw.setdefault("constant_views", [int(v) for v in np.nonzero(s["view_const"])[0]])
    return stage.LMBALoop(views_of(s, device), **kw)


def check_against_routes(name, logs, loop, a, b):
    """every log column, the poses and the points of a loop against route (a) within the bar; flags and lambdas exactly"""
    f = lambda t: t.detach().double().cpu().numpy()
    assert np.array_equal(f(logs["accepted"]), a["log"][:, 3]), (name, f(logs["accepted"]), a["log"][:, 3])
    assert np.array_equal(f(logs["lambda"]), a["log"][:, 2]), (name, f(logs["lambda"]), a["log"][:, 2])
    bad = [within_gap(name, key, f(logs[col]), a["log"][:, q], b["log"][:, q], gap=gap)
           for q, col, key, gap in ((0, "cost", "cost", None), (1, "cost_candidate", "candidate", None),
                                    (4, "grad_max", "max |g|", vector_gap(a, b, "grads")), (5, "step_max", "max |delta|", vector_gap(a, b, "steps")))]
    bad += [within_gap(name, "poses", f(loop.poses), a["poses"], b["poses"]), within_gap(name, "points", f(loop.xyzs_all), a["X"], b["X"])]
    bad = [x for x in bad if x]
    assert not bad, f"{name}: beyond {MARGIN:g} x the routes' gap (floor {FLOOR_SPACINGS:g} spacings): {bad}"
    reason, iters = loop.stopped()
    want = REASONS[a["state"]["reason"]]
    assert (reason if reason != "max_iter" else "running") == want and iters == a["state"]["iters"], (name, reason, iters, a["state"])
