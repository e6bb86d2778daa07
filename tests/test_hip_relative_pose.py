"""GPU: ls2fm_five_point / ls2fm_relative_pose / ls2fm_triangulate (csrc/relative_pose.hip) against ground truth on seeded
synthetic scenes and against the numpy restatement (tests/relpose_restate.py); batch against single-pair calls; the pycolmap and
cv2 shims driven as Initializer and the _Trad drivers drive the originals."""
import numpy as np
import pytest
import torch

import relpose_restate as RR
from ls2fm import pose
from ls2fm.utils import cv2_compat, pycolmap_compat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, CX, CY = 600.0, 320.0, 240.0
INTR = (F, F, CX, CY)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def small_rotation(rng, deg):
    w = rng.normal(size=3)
    w *= np.radians(deg) / np.linalg.norm(w)
    q = np.concatenate([[np.cos(np.linalg.norm(w) / 2)], np.sin(np.linalg.norm(w) / 2) * w / np.linalg.norm(w)])
    return pose.qvec_to_rotmat(q)


def rot_err_deg(A, B):
    c = (np.trace(np.asarray(A)[:3, :3].T @ np.asarray(B)[:3, :3]) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def dir_err_deg(a, b):
    a, b = np.asarray(a) / np.linalg.norm(a), np.asarray(b) / np.linalg.norm(b)
    return float(np.degrees(np.arccos(np.clip(a @ b, -1, 1))))


def scene(rng, n, outlier_ratio=0.0, sigma=0.0, intr0=INTR, intr1=INTR):
    """camera 1 at the identity, camera 2 = [R | t] (|t| = 1, rotation 5-20 degrees), n points 4-10 units in front of both;
    outliers: random pixels in camera 2 whose TRUE Sampson distance is at least 20x the 4 px threshold (redrawn otherwise, up to
    1000 draws; the farthest draw is kept, and it is labelled by its true distance)
    -> (uv0, uv1, P [3,4], inlier truth)"""
    R = small_rotation(rng, rng.uniform(5, 20))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 10, n)], axis=1)
    X2 = X @ R.T + t
    keep = X2[:, 2] > 1.0
    while not keep.all():
        k = int((~keep).sum())
        X[~keep] = np.stack([rng.uniform(-2, 2, k), rng.uniform(-1.5, 1.5, k), rng.uniform(4, 10, k)], axis=1)
        X2 = X @ R.T + t
        keep = X2[:, 2] > 1.0
    fx0, fy0, cx0, cy0 = intr0
    fx1, fy1, cx1, cy1 = intr1
    uv0 = np.stack([fx0 * X[:, 0] / X[:, 2] + cx0, fy0 * X[:, 1] / X[:, 2] + cy0], axis=1)
    uv1 = np.stack([fx1 * X2[:, 0] / X2[:, 2] + cx1, fy1 * X2[:, 1] / X2[:, 2] + cy1], axis=1)
    if sigma:
        uv0 = uv0 + rng.normal(size=uv0.shape) * sigma
        uv1 = uv1 + rng.normal(size=uv1.shape) * sigma
    truth = np.ones(n, bool)
    k = int(round(outlier_ratio * n))
    if k:
        E = skew(t) @ R
        thr2 = RR.threshold2(intr0, intr1, 4.0)
        idx = rng.choice(n, k, replace=False)
        for i in idx:
            best, bs = None, -1.0
            for _ in range(1000):          # the Sampson distance is bounded: some geometries allow no far pixel
                cand = rng.uniform((0, 0), (640, 480))
                s = RR.sampson2(E, RR.normalised(uv0[i], intr0), RR.normalised(cand, intr1))[0]
                if s > bs:
                    best, bs = cand, s
                if s >= 400 * thr2:
                    break
            uv1[i] = best
            truth[i] = not (bs > thr2)
    return uv0, uv1, np.c_[R, t], truth


def minimal_problems(rng, m):
    x1s, x2s, Es = [], [], []
    while len(x1s) < m:
        R, t = small_rotation(rng, rng.uniform(0, 60)), rng.normal(size=3)
        t /= np.linalg.norm(t)
        X1 = np.concatenate([rng.uniform(-1, 1, (5, 2)), rng.uniform(2, 6, (5, 1))], axis=1)
        X2 = X1 @ R.T + t
        if (X2[:, 2] > 0.5).all():
            E = skew(t) @ R
            x1s.append(X1[:, :2] / X1[:, 2:])
            x2s.append(X2[:, :2] / X2[:, 2:])
            Es.append(E / np.linalg.norm(E))
    return np.array(x1s), np.array(x2s), np.array(Es)


def test_five_point_recovers_truth_and_matches_the_restatement():
    rng = np.random.default_rng(20)
    x1, x2, Et = minimal_problems(rng, 10000)
    E, n = pose.five_point(dev(x1), dev(x2))
    E, n = E.cpu().numpy(), n.cpu().numpy()
    assert np.isfinite(E).all() and (n >= 1).all() and (n <= 10).all() and (n % 2 == 0).all()
    err = np.array([min(min(np.abs(E[i, s] - Et[i]).max(), np.abs(E[i, s] + Et[i]).max()) for s in range(n[i]))
                    for i in range(len(x1))])
    # the elimination loses digits on a small fraction of problems: 1e-9 for 99 %, 1e-5 for 99.9 %
    assert (err <= 1e-9).mean() >= 0.99 and (err <= 1e-5).mean() >= 0.999 and err.max() < 1e-2, np.sort(err)[-10:]
    for i in range(len(x1)):
        assert (E[i, n[i]:] == 0).all()
    same, close = 0, 0
    for i in range(300):
        ref = RR.five_point(x1[i], x2[i])
        if len(ref) == n[i]:
            same += 1
            close += all(np.abs(E[i, s] - ref[s]).max() <= 1e-8 for s in range(n[i]))
    assert same >= 297 and close >= 294, (same, close)


def test_five_point_degenerate_samples():
    rng = np.random.default_rng(21)
    x1, x2, _ = minimal_problems(rng, 3)
    x1[0, 1], x2[0, 1] = x1[0, 0], x2[0, 0]                        # coincident correspondences
    x1[1], x2[1] = 0.0, 0.0                                        # all zeros
    x1[2, :, 1], x2[2, :, 1] = 0.0, 0.0                            # on one line through the principal point: rank deficient
    x1 = np.concatenate([x1, np.full((1, 5, 2), np.nan)])
    x2 = np.concatenate([x2, np.zeros((1, 5, 2))])
    E, n = pose.five_point(dev(x1), dev(x2))
    assert n.cpu().tolist() == [0, 0, 0, 0]
    assert (E == 0).all()


def _check_against_restatement(uv0, uv1, truth, P, kw):
    r = pose.relative_pose(dev(uv0), dev(uv1), dev(np.array(INTR)), dev(np.array(INTR)), **kw)
    ref = RR.relative_pose(uv0, uv1, INTR, INTR, **kw)
    assert bool(r["success"][0]) and ref["success"]
    assert int(r["trials"][0]) == ref["trials"]
    assert int(r["best_trial"][0]) == ref["best_trial"]
    assert int(r["num_inliers"][0]) == ref["num_inliers"] == int(truth.sum())
    assert np.array_equal(r["inliers"].cpu().numpy(), truth)
    Q = r["poses"][0].cpu().numpy()
    assert np.abs(Q - ref["pose"]).max() <= 1e-9
    assert np.abs(Q - P).max() <= 1e-9
    assert np.abs(r["E"][0].cpu().numpy() - ref["E"]).max() <= 1e-9
    return r


def test_noise_free_exact_and_equal_to_the_restatement():
    rng = np.random.default_rng(22)
    uv0, uv1, P, truth = scene(rng, 300, outlier_ratio=0.3)
    r = _check_against_restatement(uv0, uv1, truth, P, dict(max_error_px=4.0))
    assert int(r["trials"][0]) == 1024


def test_multi_round_pair_equal_to_the_restatement():
    # 70 % outliers: eps^5 = 0.0024 asks for ~2840 trials, three rounds
    rng = np.random.default_rng(23)
    uv0, uv1, P, truth = scene(rng, 200, outlier_ratio=0.7)
    r = _check_against_restatement(uv0, uv1, truth, P, dict(max_error_px=4.0, seed=3))
    assert int(r["trials"][0]) == 3072


@pytest.mark.parametrize("ratio", [0.3, 0.7])
def test_noisy_scene(ratio):
    rng = np.random.default_rng(24 + int(ratio * 10))
    uv0, uv1, P, truth = scene(rng, 2000, outlier_ratio=ratio, sigma=0.5)
    r = pose.relative_pose(dev(uv0), dev(uv1), dev(np.array(INTR)), dev(np.array(INTR)))
    assert bool(r["success"][0])
    Q = r["poses"][0].cpu().numpy()
    # at 0.7 the local optimisation's estimate may count fewer inliers than the sampled E and is then not kept
    assert rot_err_deg(Q, P) < (0.1 if ratio < 0.5 else 1.5)
    assert dir_err_deg(Q[:, 3], P[:, 3]) < (1.0 if ratio < 0.5 else 6.0)
    inl = r["inliers"].cpu().numpy()
    assert (inl <= truth).all() and inl.sum() >= 0.95 * truth.sum()
    x1, x2 = RR.normalised(uv0, INTR), RR.normalised(uv1, INTR)
    assert np.array_equal(inl, RR.inliers_of(r["E"][0].cpu().numpy(), x1, x2, RR.threshold2(INTR, INTR, 4.0)))


MULTI_ROUND = (5, 30)


def _batch_pairs(rng):
    sizes = [int(s) for s in rng.integers(30, 600, 40)]
    sizes[3], sizes[17] = 0, 4
    intr0 = np.array([[500.0 + 10 * p, 500.0 + 10 * p, 320.0, 240.0] for p in range(40)])
    intr1 = np.array([[520.0 + 5 * p, 530.0 + 5 * p, 330.0, 250.0] for p in range(40)])
    pairs = []
    for p, n in enumerate(sizes):
        ratio = 0.75 if p in MULTI_ROUND else rng.uniform(0.0, 0.5)
        uv0, uv1, _, _ = scene(rng, n, outlier_ratio=ratio, sigma=0.3 * (p % 2), intr0=tuple(intr0[p]), intr1=tuple(intr1[p]))
        if p == 25:                 # all outliers: random pixels against random pixels
            uv0, uv1 = rng.uniform((0, 0), (640, 480), (6, 2)), rng.uniform((0, 0), (640, 480), (6, 2))
        pairs.append((uv0, uv1))
    return pairs, intr0, intr1


def test_batch_equals_single_pairs():
    rng = np.random.default_rng(25)
    pairs, k0, k1 = _batch_pairs(rng)
    r = pose.relative_pose([dev(a) for a, _ in pairs], [dev(b) for _, b in pairs], dev(k0), dev(k1))
    ps = r["pair_start"].cpu().numpy()
    inl = r["inliers"].cpu().numpy()
    for p, (a, b) in enumerate(pairs):
        s = pose.relative_pose(dev(a.reshape(-1, 2)), dev(b.reshape(-1, 2)), dev(k0[p]), dev(k1[p]))
        assert torch.equal(s["poses"][0], r["poses"][p]), p
        assert torch.equal(s["E"][0], r["E"][p]), p
        assert np.array_equal(s["inliers"].cpu().numpy(), inl[ps[p]:ps[p + 1]]), p
        for key in ("num_inliers", "trials", "best_trial", "success"):
            assert s[key][0].item() == r[key][p].item(), (p, key)
    succ = r["success"].cpu().numpy()
    assert not succ[3] and not succ[17]
    assert int(r["trials"][3]) == 0 and int(r["trials"][17]) == 0           # fewer than 5: nothing to sample
    assert torch.equal(r["poses"][3], torch.eye(3, 4, dtype=torch.float64, device=DEV))
    tr = r["trials"].cpu().numpy()
    assert all(tr[p] > 1024 for p in MULTI_ROUND), tr
    assert (tr == 1024).sum() >= 30
    assert succ.sum() >= 37


def test_batch_with_multi_tile_pairs():
    # a tile boundary (1025), an empty pair sharing the next pair's tile offset, and a three-tile pair (2049) in one scoring grid
    rng = np.random.default_rng(29)
    sizes = [1025, 0, 2049, 300]
    k0 = np.array([[500.0 + 10 * p, 500.0 + 10 * p, 320.0, 240.0] for p in range(4)])
    k1 = np.array([[520.0 + 5 * p, 530.0 + 5 * p, 330.0, 250.0] for p in range(4)])
    pairs = [scene(rng, n, outlier_ratio=0.3, sigma=0.3 * (p % 2), intr0=tuple(k0[p]), intr1=tuple(k1[p]))[:2]
             for p, n in enumerate(sizes)]
    r = pose.relative_pose([dev(a) for a, _ in pairs], [dev(b) for _, b in pairs], dev(k0), dev(k1))
    ps = r["pair_start"].cpu().numpy()
    assert ps.tolist() == [0, 1025, 1025, 3074, 3374]
    inl = r["inliers"].cpu().numpy()
    for p, (a, b) in enumerate(pairs):
        s = pose.relative_pose(dev(a.reshape(-1, 2)), dev(b.reshape(-1, 2)), dev(k0[p]), dev(k1[p]))
        assert torch.equal(s["E"][0], r["E"][p]), p
        assert torch.equal(s["poses"][0], r["poses"][p]), p
        assert np.array_equal(s["inliers"].cpu().numpy(), inl[ps[p]:ps[p + 1]]), p
        for key in ("num_inliers", "trials", "best_trial", "success"):
            assert s[key][0].item() == r[key][p].item(), (p, key)
        if sizes[p]:
            x1, x2 = RR.normalised(a, tuple(k0[p])), RR.normalised(b, tuple(k1[p]))
            mask = RR.inliers_of(r["E"][p].cpu().numpy(), x1, x2, RR.threshold2(tuple(k0[p]), tuple(k1[p]), 4.0))
            assert np.array_equal(inl[ps[p]:ps[p + 1]], mask), p
    assert int(r["trials"][1]) == 0 and not bool(r["success"][1])
    assert torch.equal(r["poses"][1], torch.eye(3, 4, dtype=torch.float64, device=DEV))


def test_determinism():
    rng = np.random.default_rng(26)
    pairs, k0, k1 = _batch_pairs(rng)
    a = pose.relative_pose([dev(u) for u, _ in pairs[:10]], [dev(v) for _, v in pairs[:10]], dev(k0[:10]), dev(k1[:10]))
    b = pose.relative_pose([dev(u) for u, _ in pairs[:10]], [dev(v) for _, v in pairs[:10]], dev(k0[:10]), dev(k1[:10]))
    for key in ("E", "poses", "inliers", "num_inliers", "trials", "best_trial", "success"):
        assert torch.equal(a[key], b[key]), key


def test_triangulate_against_numpy_dlt():
    rng = np.random.default_rng(27)
    Ps0, Ps1, u0s, u1s = [], [], [], []
    for p in range(3):
        K = np.array([[F, 0, CX], [0, F, CY], [0, 0, 1.0]])
        uv0, uv1, P, _ = scene(rng, 100 + 50 * p, sigma=0.5)
        Ps0.append(K @ np.eye(3, 4))
        Ps1.append(K @ P)
        u0s.append(uv0)
        u1s.append(uv1)
    X = pose.triangulate(dev(np.array(Ps0)), dev(np.array(Ps1)), [dev(u) for u in u0s], [dev(u) for u in u1s]).cpu().numpy()
    ref = np.concatenate([RR.triangulate(Ps0[p], Ps1[p], u0s[p], u1s[p]) for p in range(3)])
    assert np.abs(np.linalg.norm(X, axis=1) - 1).max() < 1e-12 and (X[:, 3] >= 0).all()
    assert np.abs(X - ref).max() <= 1e-9
    # cv2's layout through the shim
    H = cv2_compat.triangulatePoints(Ps0[0], Ps1[0], u0s[0].T, u1s[0].T)
    assert H.shape == (4, len(u0s[0])) and np.abs(H.T - ref[:len(u0s[0])]).max() <= 1e-9


def test_shim_as_initializer_drives_pycolmap():
    rng = np.random.default_rng(28)
    uv0, uv1, P, truth = scene(rng, 800, outlier_ratio=0.4, sigma=0.5)
    kypts0, kypts1 = uv0.astype(np.float32), uv1.astype(np.float32)          # the driver's .cpu().numpy() of float tensors
    intr = np.array([[F, 0, CX], [0, F, CY], [0, 0, 1]], dtype=np.float32)
    f, cx, cy = intr[0, 0], intr[0, 2], intr[1, 2]
    camera_colmap = pycolmap_compat.Camera(model='SIMPLE_PINHOLE', width=640, height=480, params=[f, cx, cy], )
    answer = pycolmap_compat.essential_matrix_estimation(kypts0, kypts1, camera_colmap, camera_colmap)
    assert answer["success"] is True
    assert set(answer) >= {"success", "E", "qvec", "tvec", "num_inliers", "inliers"}
    assert answer["inliers"].dtype == bool and answer["inliers"].shape == (800,) and answer["inliers"].sum() == answer["num_inliers"]
    two_view_rot = torch.from_numpy(pycolmap_compat.qvec_to_rotmat(answer["qvec"]))
    two_view_t = torch.from_numpy(answer["tvec"]).view(3, 1) * 1
    rel_pose = torch.cat([two_view_rot, two_view_t], dim=-1).float()
    assert rot_err_deg(rel_pose.numpy(), P) < 0.5 and dir_err_deg(answer["tvec"], P[:, 3]) < 3.0
    # camera.pose.compose_pair(w2c_pose, rel_pose): rel_pose applied after w2c_pose (X2 = R X1 + t)
    w2c = np.c_[small_rotation(rng, 30), rng.normal(size=3)]
    R_b, t_b = rel_pose.numpy()[:, :3].astype(np.float64), rel_pose.numpy()[:, 3].astype(np.float64)
    composed = np.c_[R_b @ w2c[:, :3], R_b @ w2c[:, 3] + t_b]
    assert rot_err_deg(composed, np.c_[P[:, :3] @ w2c[:, :3], P[:, :3] @ w2c[:, 3] + P[:, 3]]) < 0.5
    assert np.abs(answer["E"] - RR.canonical(skew(P[:, 3]) @ P[:, :3]).reshape(3, 3)).max() < 0.05


def test_shim_zero_input_fails_cleanly():
    c = pycolmap_compat.Camera(model="SIMPLE_PINHOLE", width=640, height=480, params=[500.0, 320.0, 240.0])
    assert pycolmap_compat.essential_matrix_estimation(np.zeros((8, 2)), np.zeros((8, 2)), c, c) == {"success": False}
    assert pycolmap_compat.essential_matrix_estimation(np.zeros((0, 2)), np.zeros((0, 2)), c, c) == {"success": False}
    torch.cuda.synchronize()
