"""GPU: ls2fm_p3p / ls2fm_absolute_pose / ls2fm_pose_refine (csrc/absolute_pose.hip) against ground truth on seeded synthetic
scenes and against the numpy restatement (tests/pose_restate.py); batch against single-view calls; the pycolmap shim driven
as Registration.PnP drives pycolmap."""
import numpy as np
import pytest
import torch

import pose_restate as PR
from ls2fm import pose
from ls2fm.utils import pycolmap_compat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INTR = (600.0, 600.0, 320.0, 240.0)


def rot_err_deg(A, B):
    c = (np.trace(np.asarray(A)[:3, :3].T @ np.asarray(B)[:3, :3]) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def scene(rng, n, outlier_ratio=0.0, sigma=0.0, intr=INTR):
    """a known w2c pose, n points 3-8 units in front of the camera, SIMPLE_PINHOLE projection (+ N(0, sigma) px noise), a
    fraction replaced by pixels >= 20 px from their true projection -> (uv, xyz, P [3,4], inlier truth)"""
    q = rng.normal(size=4)
    R = pose.qvec_to_rotmat(q / np.linalg.norm(q))
    t = rng.normal(size=3) * 0.5
    fx, fy, cx, cy = intr
    z = rng.uniform(3, 8, n)
    pc = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], axis=1)
    xyz = (pc - t) @ R
    uv = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], axis=1)
    if sigma:
        uv = uv + rng.normal(size=uv.shape) * sigma
    truth = np.ones(n, bool)
    k = int(round(outlier_ratio * n))
    if k:
        idx = rng.choice(n, k, replace=False)
        ang = rng.uniform(0, 2 * np.pi, k)
        rad = rng.uniform(20, 200, k)
        uv[idx] += np.stack([np.cos(ang), np.sin(ang)], axis=1) * rad[:, None]
        truth[idx] = False
    return uv, xyz, np.concatenate([R, t[:, None]], axis=1), truth


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def random_triples(rng, m):
    """m well-conditioned minimal problems (PR.well_conditioned; the others are redrawn)"""
    ys, xs, Ps = [], [], []
    while len(ys) < m:
        q = rng.normal(size=4)
        R = pose.qvec_to_rotmat(q / np.linalg.norm(q))
        t = rng.normal(size=3)
        pc = np.concatenate([rng.uniform(-1, 1, (3, 2)), rng.uniform(2, 6, (3, 1))], axis=1)
        y, x = pc / np.linalg.norm(pc, axis=1, keepdims=True), (pc - t) @ R
        if PR.well_conditioned(y, x):
            ys.append(y)
            xs.append(x)
            Ps.append(np.concatenate([R, t[:, None]], axis=1))
    return np.array(ys), np.array(xs), np.array(Ps)


def test_p3p_recovers_truth_and_matches_the_restatement():
    rng = np.random.default_rng(10)
    y, x, P = random_triples(rng, 10000)
    poses, n = pose.p3p(dev(y), dev(x))
    poses, n = poses.cpu().numpy(), n.cpu().numpy()
    assert np.isfinite(poses).all() and (n >= 1).all() and (n <= 4).all()
    worst = 0.0
    for i in range(len(y)):
        e = [max(np.abs(poses[i, s, :, :3] - P[i, :, :3]).max(), np.abs(poses[i, s, :, 3] - P[i, :, 3]).max() / np.linalg.norm(P[i, :, 3]))
             for s in range(n[i])]
        worst = max(worst, min(e))
    assert worst <= 1e-9, worst
    for i in range(1000):                                  # the restatement's solution sets, slot order, compacted
        ref = [s for s in PR.p3p(y[i], x[i]) if s is not None]
        assert len(ref) == n[i], i
        for s, Q in enumerate(ref):
            assert np.abs(poses[i, s] - Q).max() <= 1e-8, (i, s)


def test_p3p_degenerate_triples_give_no_solution():
    y = np.tile(np.eye(3)[None], (4, 1, 1))
    x = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2.0]], [[0, 0, 0], [0, 0, 0], [1, 2, 3.0]], np.zeros((3, 3)),
                  [[1, 2, 3], [1, 2, 3], [1, 2, 3.0]]])
    poses, n = pose.p3p(dev(y), dev(x))
    assert n.cpu().tolist() == [0, 0, 0, 0]
    assert torch.isfinite(poses).all() and (poses == 0).all()


def test_noise_free_exact_and_equal_to_the_restatement():
    rng = np.random.default_rng(11)
    uv, xyz, P, truth = scene(rng, 1000, outlier_ratio=0.6)
    r = pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), max_error_px=3.0)
    assert bool(r["success"][0])
    assert np.abs(r["poses"][0].cpu().numpy() - P).max() <= 1e-9
    assert np.array_equal(r["inliers"].cpu().numpy(), truth)
    ref = PR.absolute_pose(uv, xyz, INTR, max_error_px=3.0)
    assert int(r["best_trial"][0]) == ref["best_trial"]
    assert int(r["trials"][0]) == ref["trials"] == 1024
    assert int(r["num_inliers"][0]) == ref["num_inliers"] == int(truth.sum())
    assert np.abs(r["poses"][0].cpu().numpy() - ref["pose"]).max() <= 1e-9


def test_multi_round_view_equal_to_the_restatement():
    # 88 % outliers: the stopping rule asks for ~5300 trials, six rounds; with this seed the first all-inlier sample is trial
    # 3674, so the winner is selected in round 4 (t0 = 3072) and kept through rounds 5 and 6
    rng = np.random.default_rng(18)
    uv, xyz, P, truth = scene(rng, 1000, outlier_ratio=0.88)
    r = pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), max_error_px=3.0, seed=17)
    ref = PR.absolute_pose(uv, xyz, INTR, max_error_px=3.0, seed=17)
    assert int(r["trials"][0]) == ref["trials"] == 6144
    assert int(r["best_trial"][0]) == ref["best_trial"] == 3674
    assert int(r["num_inliers"][0]) == ref["num_inliers"] == int(truth.sum())
    assert np.array_equal(r["inliers"].cpu().numpy(), truth)
    assert np.abs(r["poses"][0].cpu().numpy() - P).max() <= 1e-9
    assert np.abs(r["poses"][0].cpu().numpy() - ref["pose"]).max() <= 1e-9
    # min_num_trials above the cap (min_inlier_ratio 0.5: cap 69): the cap wins on both sides, one round
    kw = dict(max_error_px=3.0, seed=17, min_inlier_ratio=0.5, min_num_trials=50000)
    r = pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), **kw)
    ref = PR.absolute_pose(uv, xyz, INTR, **kw)
    assert int(r["trials"][0]) == ref["trials"] == 1024
    assert int(r["best_trial"][0]) == ref["best_trial"]


def test_noisy_scene():
    rng = np.random.default_rng(12)
    uv, xyz, P, truth = scene(rng, 2000, outlier_ratio=0.3, sigma=0.5)
    r = pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), max_error_px=3.0)
    assert bool(r["success"][0])
    Q = r["poses"][0].cpu().numpy()
    assert rot_err_deg(Q, P) < 0.05
    Z, e2 = PR.project_err2(Q, xyz, uv, INTR)
    assert np.array_equal(r["inliers"].cpu().numpy(), (Z > 0) & (np.sqrt(e2) < 3.0))
    assert (r["inliers"].cpu().numpy() <= truth).all()


MULTI_ROUND = (5, 30)


def _batch_views(rng):
    sizes = [int(s) for s in rng.integers(50, 1500, 40)]
    sizes[3], sizes[17], sizes[5], sizes[30] = 0, 3, 1000, 1000
    intr = np.array([[500.0 + 10 * v, 500.0 + 10 * v, 320.0, 240.0] for v in range(40)])
    views = []
    for v, n in enumerate(sizes):
        ratio = rng.uniform(0.0, 0.6)
        if v in MULTI_ROUND:         # 88 % outliers: these views run several rounds beside views done after one
            ratio = 0.88
        uv, xyz, _, _ = scene(rng, n, outlier_ratio=ratio, sigma=0.3 * (v % 2), intr=tuple(intr[v]))
        if v == 25:                  # all outliers: five random key points against five random 3-D points
            uv, xyz = rng.uniform((0, 0), (640, 480), (5, 2)), rng.uniform(-2, 2, (5, 3)) + (0, 0, 6)
        views.append((uv, xyz))
    return views, intr


def test_batch_equals_single_views():
    rng = np.random.default_rng(13)
    views, intr = _batch_views(rng)
    kw = dict(max_error_px=4.0, max_num_trials=20000)
    r = pose.absolute_pose([dev(u) for u, _ in views], [dev(x) for _, x in views], dev(intr), **kw)
    vs = r["view_start"].cpu().numpy()
    inl = r["inliers"].cpu().numpy()
    for v, (u, x) in enumerate(views):
        s = pose.absolute_pose(dev(u.reshape(-1, 2)), dev(x.reshape(-1, 3)), dev(intr[v]), **kw)
        assert torch.equal(s["poses"][0], r["poses"][v]), v
        assert np.array_equal(s["inliers"].cpu().numpy(), inl[vs[v]:vs[v + 1]]), v
        for key in ("num_inliers", "trials", "best_trial", "success"):
            assert s[key][0].item() == r[key][v].item(), (v, key)
    succ = r["success"].cpu().numpy()
    assert not succ[3] and not succ[17] and not succ[25]
    assert not PR.absolute_pose(views[25][0], views[25][1], intr[25], **kw)["success"]
    assert int(r["trials"][3]) == 0 and int(r["num_inliers"][3]) == 0             # N = 0: nothing to sample
    assert int(r["trials"][17]) == 1024 and int(r["num_inliers"][17]) <= 3        # N = 3: sampled, fails the >= 4 rule
    assert succ.sum() == 37
    tr = r["trials"].cpu().numpy()
    assert all(tr[v] > 1024 for v in MULTI_ROUND), tr
    assert (tr == 1024).sum() >= 30                 # the others stopped after the first round


def test_determinism():
    rng = np.random.default_rng(14)
    views, intr = _batch_views(rng)
    a = pose.absolute_pose([dev(u) for u, _ in views[:10]], [dev(x) for _, x in views[:10]], dev(intr[:10]), max_error_px=4.0)
    b = pose.absolute_pose([dev(u) for u, _ in views[:10]], [dev(x) for _, x in views[:10]], dev(intr[:10]), max_error_px=4.0)
    for key in ("poses", "inliers", "num_inliers", "trials", "best_trial", "success"):
        assert torch.equal(a[key], b[key]), key
    tr = a["trials"].cpu().numpy()
    assert tr[MULTI_ROUND[0]] > 1024 and (tr == 1024).any()      # a multi-round view among views done after one round


def test_view_start_must_cover_the_correspondences():
    rng = np.random.default_rng(19)
    uv, xyz, _, _ = scene(rng, 100)
    for vs in ([0, 50, 105], [1, 50, 100], [0, 60, 50, 100]):
        with pytest.raises(ValueError, match="view_start"):
            pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), view_start=torch.tensor(vs, device=DEV))
        with pytest.raises(ValueError, match="view_start"):
            pose.refine_pose(dev(uv), dev(xyz), dev(np.array(INTR)), dev(np.zeros((len(vs) - 1, 3, 4))), dev(np.ones(100, bool)),
                             view_start=torch.tensor(vs, device=DEV))


def test_refinement_matches_the_restatement_and_composes():
    rng = np.random.default_rng(15)
    uv, xyz, P, truth = scene(rng, 1500, outlier_ratio=0.2, sigma=0.5)
    # a pose ~2 degrees and 5 % of the depth away, on the true mask
    w = rng.normal(size=3)
    start = PR.update(P, np.concatenate([w / np.linalg.norm(w) * np.radians(2.0), np.array([0.0, 0.0, 0.05 * 5.5])]))
    got = pose.refine_pose(dev(uv), dev(xyz), dev(np.array(INTR)), dev(start), dev(truth))[0].cpu().numpy()
    ref = PR.refine(start, xyz, uv, INTR, truth)
    assert np.abs(got - ref).max() <= 1e-8
    assert rot_err_deg(got, P) < 0.05
    kw = dict(max_error_px=3.0, seed=5)
    a = pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), refine=True, **kw)
    b = pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), refine=False, **kw)
    c = pose.refine_pose(dev(uv), dev(xyz), dev(np.array(INTR)), b["poses"], b["inliers"])
    assert torch.equal(a["poses"], c) and torch.equal(a["inliers"], b["inliers"])


def test_shim_as_registration_drives_pycolmap():
    rng = np.random.default_rng(16)
    uv, xyz, P, truth = scene(rng, 800, outlier_ratio=0.4, sigma=0.5)
    id_2d, id_3d = np.arange(800) + 1000, np.arange(800) + 5000
    mask = np.ones(800, bool)
    mask[::50] = False                                       # the caller's SDF filter
    p2d, p3d = uv[mask], xyz[mask]
    f, cx, cy = torch.tensor(600.0), 320.0, 240.0           # Camera.f is a tensor in the reference
    camera_colmap = pycolmap_compat.Camera(model='SIMPLE_PINHOLE', width=640, height=480, params=[f, cx, cy], )
    answer = pycolmap_compat.absolute_pose_estimation(p2d, p3d, camera_colmap, max_error_px=3.0)
    assert answer["success"] is True
    assert set(answer) >= {"success", "qvec", "tvec", "num_inliers", "inliers"}
    assert answer["inliers"].dtype == bool and answer["inliers"].shape == (len(p2d),)
    sel_2d = id_2d[mask][answer['inliers']]
    assert len(sel_2d) == answer["num_inliers"] and np.isin(sel_2d - 1000, np.nonzero(truth)[0]).all()
    answer = pycolmap_compat.pose_refinement(answer['tvec'], answer['qvec'], p2d, p3d, answer['inliers'], camera_colmap)
    assert answer["success"]
    rot = pycolmap_compat.qvec_to_rotmat(answer["qvec"])
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12
    SE3 = np.concatenate([rot, answer['tvec'].reshape(3, 1)], axis=-1)
    assert rot_err_deg(SE3, P) < 0.1 and np.abs(SE3[:, 3] - P[:, 3]).max() < 0.05
    # the pose the shim returns is the device's
    r = pose.absolute_pose(dev(p2d), dev(p3d), dev(np.array(INTR)), max_error_px=3.0)
    Q = r["poses"][0].cpu().numpy()
    ans = pycolmap_compat.absolute_pose_estimation(p2d, p3d, camera_colmap, max_error_px=3.0)
    assert np.abs(pycolmap_compat.qvec_to_rotmat(ans["qvec"]) - Q[:, :3]).max() < 1e-12
    assert np.array_equal(ans["tvec"], Q[:, 3])


def test_one_view_of_a_million_correspondences():
    rng = np.random.default_rng(17)
    n = 1 << 20
    uv, xyz, P, truth = scene(rng, n, outlier_ratio=0.2, sigma=0.3)
    from ls2fm import _lib
    ws = _lib.load().ls2fm_absolute_pose_workspace_bytes(1, n)
    assert 0 < ws < 1 << 20
    r = pose.absolute_pose(dev(uv), dev(xyz), dev(np.array(INTR)), max_error_px=3.0)
    torch.cuda.synchronize()
    assert bool(r["success"][0]) and int(r["trials"][0]) == 1024
    assert rot_err_deg(r["poses"][0].cpu().numpy(), P) < 0.01
    assert int(r["num_inliers"][0]) >= int(0.99 * truth.sum())
