"""float64 restatement of the classical bundle adjustment (ls2fm.stage.TradBALoop / csrc/bundle_adjust.hip; the loop of
pipelines/BA_Trad.py:86-130 of the reference), the checker of the device and host results.  Every step is written out: the
11-term series of the se(3) exponential, the projection with the first camera's intrinsic, the robust + plain mean, the weight
select, Adam's update (torch.optim.Adam's defaults) per group and ExponentialLR's chained multiplication.  Only the gradient
is left to autograd (torch, float64).  tests/test_bundle_adjust_host.py pins this file to the reference's own fp64 trajectory.

Also the fixture readers the two test files share."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("local", "global", "single", "heavy")            # 20 recorded iterations (single: 10); "long": 1000, log and final state
TERMS = 11


def load_case(name):
    g = dict(np.load(os.path.join(GOLDEN, f"stage_ba_trad_{name}.npz")))
    g["meta"] = json.loads(bytes(g.pop("meta_json")).decode())
    return g


def tracked_lists(g):
    """per view of the scene: the key points that have a 3-D point and the point each observes (Camera.idx2d_to_3d != -1)"""
    ks, kp, ids = g["kypts_start"], [], []
    for v in range(len(ks) - 1):
        k, i = g["kypts"][ks[v]:ks[v + 1]], g["idx2d_to_3d"][ks[v]:ks[v + 1]]
        kp.append(k[i != -1])
        ids.append(i[i != -1])
    return kp, ids


def cam_pick_of(g):
    given = g["cam_pick_given"]
    return None if given[0] < 0 else [int(c) for c in given]


def observation_list(g):
    """util.get_idx3d_camset over cam_pick -> (obs_point [n], obs_view [n], obs_uv [n,2])"""
    kp, ids = tracked_lists(g)
    pick = cam_pick_of(g) or list(range(len(kp)))
    return (np.concatenate([ids[c] for c in pick]), np.concatenate([np.full(len(ids[c]), j) for j, c in enumerate(pick)]),
            np.concatenate([kp[c] for c in pick]), pick)


def series(theta, first):
    """sum_i (-1)^i theta^(2i) / d_i, left to right; d_0 = first, d_i = d_(i-1) (2i + first - 1 ... ) as utils/camera.py:100-147:
    A: 1 / (2i + 1)!, B: 1 / (2i + 2)!, C: 1 / (2i + 3)!"""
    total, denom = 0.0, 1.0
    for k in range(1, first + 1):
        denom *= k
    for i in range(TERMS):
        if i > 0:
            denom *= (2 * i + first - 1) * (2 * i + first)
        total = total + (-1) ** i * theta ** (2 * i) / denom
    return total


def se3_to_SE3(wu):
    w, u = wu[..., :3], wu[..., 3:]
    zero = torch.zeros_like(w[..., 0])
    wx = torch.stack([torch.stack([zero, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], zero, -w[..., 0]], -1),
                      torch.stack([-w[..., 1], w[..., 0], zero], -1)], -2)
    theta = w.norm(dim=-1)[..., None, None]
    eye = torch.eye(3, dtype=wu.dtype)
    A, B, C = series(theta, 1), series(theta, 2), series(theta, 3)
    R = eye + A * wx + B * wx @ wx
    V = eye + B * wx + C * wx @ wx
    return torch.cat([R, V @ u[..., None]], dim=-1)


def run(se3, xyzs, obs_point, obs_view, obs_uv, intrinsic, n_iters, max_iter, lr_pose_r=5e-3, lr_pose_t=1e-2, lr_xyzs=1e-2, lr_sdf=1e-4,
        lr_sdf_end=5e-5, betas=(0.9, 0.999), eps=1e-8):
    """-> dict: reproj / weight / err_mean [n_iters], se3 / xyzs (stepped), se3_written / xyzs_written (entering the last
    iteration; xyzs_written per observation as the reference's `xyzs_forward`)"""
    f64 = torch.float64
    params = [torch.tensor(se3[:, :3], dtype=f64), torch.tensor(se3[:, 3:], dtype=f64), torch.tensor(xyzs, dtype=f64)]
    uv_obs, K = torch.tensor(obs_uv, dtype=f64), torch.tensor(intrinsic, dtype=f64)
    op, ov = torch.tensor(obs_point, dtype=torch.long), torch.tensor(obs_view, dtype=torch.long)
    lrs = [lr_pose_r, lr_pose_t, lr_xyzs]
    gamma = (lr_sdf_end / lr_sdf) ** (1.0 / max_iter)
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    out = dict(reproj=[], weight=[], err_mean=[])
    for it in range(n_iters):
        r, t, x = [p.clone().requires_grad_(True) for p in params]
        wu = torch.cat([r, t], dim=1)
        pose = se3_to_SE3(wu[ov])                                            # [n,3,4]
        xf = x[op]
        xc = (pose[:, :, :3] @ xf[:, :, None])[..., 0] + pose[:, :, 3]
        u = xc @ K.T
        uv = (u / (u[:, 2:] + 1e-6))[:, :2]
        err = (uv - uv_obs).norm(dim=-1)
        reproj = 0.5 * (2 * torch.log(1 + err ** 2 / 4)).mean() + 0.5 * err.mean()
        weight = 10.0 if float(reproj.detach()) > 10 else 1.0
        out["reproj"].append(float(reproj.detach())); out["weight"].append(weight); out["err_mean"].append(float(err.detach().mean()))
        out["se3_written"], out["xyzs_written"] = wu.detach().numpy().copy(), xf.detach().numpy().copy()
        grads = torch.autograd.grad(weight * reproj, [r, t, x])
        step = it + 1
        bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
        for q in range(3):
            g = grads[q]
            m[q] = m[q] + (1 - betas[0]) * (g - m[q])
            v[q] = v[q] * betas[1] + (1 - betas[1]) * g * g
            params[q] = params[q] - (lrs[q] / bc1) * (m[q] / (v[q].sqrt() / bc2 ** 0.5 + eps))
            lrs[q] = lrs[q] * gamma
    out = {k: np.asarray(val) for k, val in out.items()}
    out["se3"] = torch.cat(params[:2], dim=1).numpy()
    out["xyzs"] = params[2].numpy()
    return out


def one_iteration(se3, xyzs, obs_point, obs_view, obs_uv, intrinsic, dtype=torch.float64, zero_err_obs=()):
    """The loss of ONE iteration and its gradient, written on its own (not through `run`): the reference's formula in `dtype`
    (float64: the checker; float32: the same formula rounded on the CPU, the yardstick of the bars).
    zero_err_obs: observations whose key point is replaced by this evaluation's own projection, so that err == 0 exactly in
    every precision (norm backward at 0: zero) -- the device test places the key point on the kernel's fp32 projection.
    -> dict: reproj, err_mean, weight (floats), d_se3 [V,6], d_points [P,3] (float64 numpy, of the UNWEIGHTED reproj), u_z [n]"""
    wu = torch.tensor(np.asarray(se3), dtype=dtype).requires_grad_(True)
    x = torch.tensor(np.asarray(xyzs), dtype=dtype).requires_grad_(True)
    K, key = torch.tensor(np.asarray(intrinsic), dtype=dtype), torch.tensor(np.asarray(obs_uv), dtype=dtype)
    op, ov = torch.tensor(np.asarray(obs_point), dtype=torch.long), torch.tensor(np.asarray(obs_view), dtype=torch.long)
    pose = se3_to_SE3(wu)[ov]                                                # [n,3,4]
    xc = (pose[:, :, :3] @ x[op][:, :, None])[..., 0] + pose[:, :, 3]
    u = xc @ K.T
    uv = (u / (u[:, 2:] + 1e-6))[:, :2]
    if len(zero_err_obs):
        key = key.clone()
        key[list(zero_err_obs)] = uv.detach()[list(zero_err_obs)]
    err = (uv - key).norm(dim=-1)
    reproj = 0.5 * (2 * torch.log(1 + err ** 2 / 4)).mean() + 0.5 * err.mean()
    d_se3, d_points = torch.autograd.grad(reproj, [wu, x])
    return dict(reproj=float(reproj.detach()), err_mean=float(err.detach().mean()), weight=10.0 if float(reproj.detach()) > 10 else 1.0,
                d_se3=d_se3.double().numpy(), d_points=d_points.double().numpy(), u_z=u.detach()[:, 2].double().numpy())


# ------------------------------------------------------------------------------------- a scene of the kernels' rarely hit branches
SCENE_COUNTS = (300, 1, 255, 256, 257, 5000, 120)       # observations per view: around the residual kernel's 256 threads
SCENE_POINTS, SCENE_UNSEEN = 6000, 200                  # the last SCENE_UNSEEN points are observed by no view
SCENE_K = np.array([[520.0, 0.0, 320.0], [0.0, 515.0, 240.0], [0.0, 0.0, 1.0]], dtype=np.float32)


def _fma32(a, b, c):
    """fmaf on float32 values: the product of two float32 is exact in float64; the sum is then rounded to float64 and to float32
    (a double rounding differs from one only on a 2^-29 tie pattern; the device test notices: it asserts the zero gradient)"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def project_identity_f32(x, K):
    """csrc/reproject_point.h's arithmetic, operation by operation in float32, for the IDENTITY pose (x_c = x exactly):
    u_a = fmaf(k_a2, z, fmaf(k_a1, y, k_a0 * x)) ; inv = 1 / (u_z + 1e-6f) ; uv = u_xy * inv"""
    f = np.float32
    x, K = np.asarray(x, dtype=f), np.asarray(K, dtype=f)
    u = [_fma32(K[a, 2], x[2], _fma32(K[a, 1], x[1], f(K[a, 0] * x[0]))) for a in range(3)]
    inv = f(1.0) / f(u[2] + f(1e-6))
    return np.array([f(u[0] * inv), f(u[1] * inv)], dtype=f)


def synthetic_scene(seed=2024):
    """7 views over 6000 points, float32 values.  On purpose: view 0 has se3 = 0 exactly (theta = 0), view 1 |w| = 1e-4 and ONE
    observation, view 6 |w| = 3.0 (about the optical axis, so every depth stays near 6); 255 / 256 / 257 / 5000 observations
    in views 2..5; point 0 is observed by every view, point 1 by view 0 only and its key point IS the kernel's fp32 projection
    (err == 0 bit for bit), most points by exactly one view, the last 200 by none; the observations of a view are in random
    order.  Key points: the float64 projection + N(0, 2 px).  -> dict(se3, xyzs, intrinsic, keypoints, track_ids, zero_err_obs)"""
    rng = np.random.default_rng(seed)
    V, P = len(SCENE_COUNTS), SCENE_POINTS
    xyzs = (rng.uniform(-1.0, 1.0, size=(P, 3)) + np.array([0.0, 0.0, 6.0])).astype(np.float32)
    se3 = np.zeros((V, 6), dtype=np.float64)
    for v in range(1, V):
        w = rng.normal(size=3)
        se3[v, :3] = w / np.linalg.norm(w) * rng.uniform(0.05, 0.6)
        se3[v, 3:] = rng.uniform(-0.3, 0.3, size=3)
    w = rng.normal(size=3)
    se3[1, :3] = w / np.linalg.norm(w) * 1e-4
    w = np.array([0.02, -0.015, 1.0])
    se3[6, :3] = w / np.linalg.norm(w) * 3.0
    se3 = se3.astype(np.float32)
    seen = P - SCENE_UNSEEN
    ids = []
    for v, c in enumerate(SCENE_COUNTS):
        others = rng.choice(np.arange(2, seen), size=c - 1, replace=False)
        i = np.concatenate([[0], others])
        if v == 0:
            i[1] = 1
        ids.append(i[rng.permutation(c)].astype(np.int64))
    assert ids[1].tolist() == [0]
    op = np.concatenate(ids)
    ov = np.concatenate([np.full(len(i), v) for v, i in enumerate(ids)])
    with torch.no_grad():
        pose = se3_to_SE3(torch.tensor(se3, dtype=torch.float64))[torch.tensor(ov)]
        xc = (pose[:, :, :3] @ torch.tensor(xyzs, dtype=torch.float64)[torch.tensor(op)][:, :, None])[..., 0] + pose[:, :, 3]
        u = xc @ torch.tensor(SCENE_K, dtype=torch.float64).T
        uv = (u[:, :2] / u[:, 2:]).numpy()
    assert u[:, 2].min() > 3.0, "a point too close to a camera"
    uv = (uv + rng.normal(0.0, 2.0, size=uv.shape)).astype(np.float32)
    k0 = int(np.nonzero(ids[0] == 1)[0][0])                          # view 0 starts the list: its local index is the global one
    uv[k0] = project_identity_f32(xyzs[1], SCENE_K)
    starts = np.concatenate([[0], np.cumsum(SCENE_COUNTS)])
    kps = [uv[starts[v]:starts[v + 1]] for v in range(V)]
    return dict(se3=se3, xyzs=xyzs, intrinsic=SCENE_K.copy(), keypoints=kps, track_ids=ids, zero_err_obs=[k0], obs_point=op, obs_view=ov,
                obs_uv=uv)


# ---------------------------------------------------------------------------------------------------- the bars of both test files
MARGIN = 4.0          # two independently rounded fp32 runs can each sit one fp32-vs-fp64 gap from the truth; doubled for headroom


def within_f32_gap(name, key, mine, ref64, ref32, margin=MARGIN):
    """one quantity of a single evaluation: |mine - fp64| <= max(margin * |fp32 on the CPU - fp64|, one fp32 spacing of the
    quantity's largest magnitude), maxima over the quantity's elements.  Prints the figures, returns the failure or None."""
    mine, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (mine, ref64, ref32))
    d, gap = float(np.abs(mine - ref64).max()), float(np.abs(ref32 - ref64).max())
    quantum = float(np.spacing(np.float32(np.abs(ref64).max())))
    bar = max(margin * gap, quantum)
    print(f"[{name}] {key:10s} device-fp64 {d:.3e}  fp32-fp64 {gap:.3e}  spacing {quantum:.2e}  bar {bar:.3e}  (largest magnitude {np.abs(ref64).max():.3e})")
    return None if d <= bar else (key, d, gap, quantum)


def build_loop(g, device, shuffle_seed=None, **kw):
    """ls2fm.stage.TradBALoop over a fixture's scene (TrackedViews holds every view; cam_pick selects as the reference's
    cam_pick_ids).  shuffle_seed: permute every view's observations (the list stays sorted by view)"""
    import torch
    from ls2fm import stage
    kp, ids = tracked_lists(g)
    if shuffle_seed is not None:
        rng = np.random.default_rng(shuffle_seed)
        perms = [rng.permutation(len(i)) for i in ids]
        kp, ids = [k[p] for k, p in zip(kp, perms)], [i[p] for i, p in zip(ids, perms)]
    V = len(kp)
    views = stage.TrackedViews(torch.tensor(g["se3"], device=device), torch.tensor(g["intrinsic"], device=device),
                               torch.zeros(V, 1, 3, device=device), [torch.tensor(k, device=device) for k in kp],
                               [torch.tensor(i, device=device) for i in ids], torch.tensor(g["xyzs"], device=device), 1, 1)
    kw.setdefault("max_iter", g["meta"]["max_iter_opt"])
    return stage.TradBALoop(views, cam_pick=cam_pick_of(g), lr_xyzs=g["meta"]["lr_xyzs"], lr_pose_r=g["meta"]["optim"]["lr_pose_r"],
                            lr_pose_t=g["meta"]["optim"]["lr_pose_t"], lr_sdf=g["meta"]["optim"]["lr_sdf"],
                            lr_sdf_end=g["meta"]["optim"]["lr_sdf_end"], **kw)


def distances(g, logs, loop, tag="f32"):
    """per quantity: (distance of the loop's result to the fixture's `tag` trajectory, the fixture's fp32-vs-fp64 gap, one fp32
    spacing of the quantity) -- the log terms relative, the states absolute, as the generator measures the gap"""
    f = lambda t: t.detach().double().cpu().numpy()
    se3_w, xyzs_w, err_w = loop.written_back()
    ref_se3 = np.concatenate([g[f"{tag}/r_final"], g[f"{tag}/t_final"]], axis=1)
    rel = lambda mine, ref, key: (float(np.abs(np.asarray(mine) / ref - 1).max()), float(g[f"gap/{key}"]), 2.0 ** -23)
    ab = lambda mine, ref, key: (float(np.abs(mine - ref).max()), float(g[f"gap/{key}"]), float(np.spacing(np.float32(np.abs(ref).max()))))
    return {
        "reproj": rel(f(logs["reproj_error"]), g[f"{tag}/reproj"], "reproj"),
        "err_mean": rel(f(logs["err_mean"]), g[f"{tag}/err_mean"], "err_mean"),
        # the returned value IS the last iteration's mean(err): ONE sample of the quantity whose gap `err_mean` takes over every
        # recorded iteration, so its yardstick is the larger of the two (`single`: its own one-sample gap is 1.9e-7 where the
        # per-iteration one is 1.2e-6; the host torch path sits 5.7 of the former, 0.9 of the latter, from the reference)
        "err_returned": rel(float(err_w), float(g[f"{tag}/err_returned"]), "err_returned")[:1]
                        + (max(float(g["gap/err_returned"]), float(g["gap/err_mean"])), 2.0 ** -23),
        "se3_final": ab(f(loop.poses_se3()), ref_se3, "se3_final"),
        "xyzs_final": ab(f(loop.xyzs_all), g[f"{tag}/xyzs_final"], "xyzs_final"),
        "se3_written": ab(f(se3_w), g[f"{tag}/se3_written"], "se3_written"),
        "xyzs_written": ab(f(xyzs_w)[g["obs_point"]], g[f"{tag}/xyzs_written"], "xyzs_written"),
    }


def assert_within_gap(name, dist, margin=MARGIN):
    """prints every figure (distance, gap, ratio), then asserts  distance <= margin * gap + one fp32 spacing  for each quantity.
    The spacing term is the format's own resolution, not headroom: the results are fp32 numbers, and two fp32 numbers whose real
    values agree to any precision can still be one spacing apart, while the gap of ONE recorded pair of runs can by luck be far
    below a spacing (`single`: 5.9e-8 on translations near 5, whose spacing is 4.8e-7 -- there the host torch path sits exactly one
    spacing from the reference's fp32 run, 8.0 gaps).  Everywhere the gap exceeds a spacing the bar is the issue's 4 x gap."""
    bad = []
    for k, (d, gap, quantum) in dist.items():
        print(f"[ba_trad {name}] {k:13s} distance {d:.3e}  gap {gap:.3e}  ratio {d / gap:6.2f}  (bar {margin:g} gaps + one fp32 spacing {quantum:.2e})")
        if not d <= margin * gap + quantum:
            bad.append((k, d, gap, d / gap))
    assert not bad, f"{name}: beyond {margin:g} x the fixture's fp32-vs-fp64 gap (+ one fp32 spacing): {bad}"
