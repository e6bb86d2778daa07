"""CPU: the numpy restatement of the two-view geometry (tests/twoview_restate.py) against ground truth, the verdict rules of
ls2fm.pose.two_view_config on hand-made counts, and the argument checks of the new Python entries.  No device is needed."""
import numpy as np
import pytest
import torch

import twoview_restate as TV
import twoview_scenes as S
from ls2fm import match, pose
from ls2fm.utils import pycolmap_compat


def test_restated_seven_point_contains_the_true_f():
    rng = np.random.default_rng(40)
    a, b, Ft = S.seven_point_problems(rng, 500)
    err, counts = [], []
    for i in range(500):
        sol = TV.seven_point(a[i], b[i])
        counts.append(len(sol))
        err.append(min([np.abs(F - Ft[i]).max() for F in sol] + [9.0]))
    err = np.array(err)
    # reached on this seed: 100 % within 1e-9, the worst 2.4e-11 (with the Gauss-Jordan basis NOT orthonormalised the same
    # problems reach 98.8 % and 1.2e-7: the reason the rule has the Gram-Schmidt step); 433 problems have 3 solutions, 67 have 1
    assert (err <= 1e-9).mean() >= 0.99 and err.max() < 1e-2, np.sort(err)[-10:]
    assert set(counts) <= {1, 3}


def test_restated_four_point_recovers_the_true_h():
    rng = np.random.default_rng(41)
    a, b, Ht = S.four_point_problems(rng, 200)
    for i in range(200):
        sol = TV.four_point(a[i], b[i])
        assert len(sol) == 1 and np.abs(sol[0] - Ht[i]).max() <= 1e-9, i


def test_restated_degenerate_samples_give_no_solution():
    a, b = S.degenerate_seven(np.random.default_rng(42))
    assert [len(TV.seven_point(x, y)) for x, y in zip(a, b)] == [0, 0, 0]
    a, b = S.degenerate_four(np.random.default_rng(43))
    assert [len(TV.four_point(x, y)) for x, y in zip(a, b)] == [0, 0, 0, 0]


def test_restated_cubic_roots():
    assert np.allclose(TV.cubic_roots([-6.0, 11.0, -6.0, 1.0]), [1.0, 2.0, 3.0], atol=1e-14)
    assert np.allclose(TV.cubic_roots([-1.0, 1.0, -1.0, 1.0]), [1.0], atol=1e-14)             # (x - 1)(x^2 + 1)
    assert np.allclose(TV.cubic_roots([2.0, -3.0, 1.0, 1e-15]), [1.0, 2.0], atol=1e-14)       # the leading term is dropped
    assert np.allclose(TV.cubic_roots([-4.0, 2.0, 0.0, 0.0]), [2.0], atol=1e-14)
    assert TV.cubic_roots([1.0, 0.0, 1.0, 0.0]) == [] and TV.cubic_roots([0.0] * 4) == [] and TV.cubic_roots([np.nan, 1, 1, 1]) == []


# (nE, okE, nF, okF, nH) -> (config, the chosen inlier set); defaults 15 / 0.95 / 0.8
VERDICTS = [
    ((100, True, 100, True, 10), (pose.CALIBRATED, 0)),
    ((96, True, 100, True, 10), (pose.CALIBRATED, 0)),
    ((95, True, 100, True, 10), (pose.UNCALIBRATED, 1)),           # nE / nF = 0.95 is not > 0.95
    ((100, False, 100, True, 10), (pose.UNCALIBRATED, 1)),         # E failed
    ((14, True, 14, True, 0), (pose.DEGENERATE, -1)),              # below min_num_inliers
    ((15, True, 15, True, 0), (pose.CALIBRATED, 0)),
    ((14, True, 15, True, 0), (pose.UNCALIBRATED, 1)),
    ((20, True, 0, False, 0), (pose.CALIBRATED, 0)),               # nE / 0 = +inf
    ((0, False, 0, False, 0), (pose.DEGENERATE, -1)),              # 0 / 0 is NaN: no comparison holds
    ((100, True, 100, True, 80), (pose.CALIBRATED, 0)),            # nH / n_best = 0.8 is not > 0.8
    ((100, True, 100, True, 81), (pose.PLANAR_OR_PANORAMIC, 0)),
    ((100, True, 100, True, 100), (pose.PLANAR_OR_PANORAMIC, 0)),  # nH == n_best keeps E's set
    ((100, True, 100, True, 101), (pose.PLANAR_OR_PANORAMIC, 2)),
    ((50, True, 100, True, 90), (pose.PLANAR_OR_PANORAMIC, 1)),    # uncalibrated, n_best = nF
    ((50, True, 100, True, 120), (pose.PLANAR_OR_PANORAMIC, 2)),
    ((10, True, 12, True, 200), (pose.DEGENERATE, -1)),            # a degenerate pair stays degenerate whatever H counts
    ((None, None, 100, True, 10), (pose.UNCALIBRATED, 1)),
    ((None, None, 100, True, 95), (pose.PLANAR_OR_PANORAMIC, 1)),
    ((None, None, 100, False, 0), (pose.DEGENERATE, -1)),
]


def test_verdict_rules_on_hand_made_counts():
    assert (pose.DEGENERATE, pose.CALIBRATED, pose.UNCALIBRATED, pose.PLANAR_OR_PANORAMIC) == (1, 2, 3, 6)
    who = {0: "E", 1: "F", 2: "H", -1: None}
    for with_e in (True, False):
        rows = [(c, w) for c, w in VERDICTS if (c[0] is not None) == with_e]
        nE, okE, nF, okF, nH = (list(col) for col in zip(*[c for c, _ in rows]))
        cfg, choice = pose.two_view_config(torch.tensor(nE, dtype=torch.int32) if with_e else None,
                                           torch.tensor(okE) if with_e else None, torch.tensor(nF, dtype=torch.int32),
                                           torch.tensor(okF), torch.tensor(nH, dtype=torch.int32))
        assert cfg.dtype == torch.int32
        for k, (c, want) in enumerate(rows):
            assert (int(cfg[k]), int(choice[k])) == want, (c, int(cfg[k]), int(choice[k]))
            assert TV.config_of(*c) == (want[0], who[want[1]]), c
    # the three thresholds are arguments
    cfg, _ = pose.two_view_config(torch.tensor([30]), torch.tensor([True]), torch.tensor([40]), torch.tensor([True]), torch.tensor([20]),
                                  min_num_inliers=35, min_E_F_inlier_ratio=0.7, max_H_inlier_ratio=0.4)
    assert int(cfg[0]) == pose.PLANAR_OR_PANORAMIC                   # E too few -> F (40 >= 35); 20 / 40 > 0.4


def test_argument_checks():
    a = torch.zeros(7, 2, dtype=torch.float64)
    for fn in (pose.seven_point, pose.four_point_homography, pose.fundamental_matrix, pose.homography):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(a, a)
    with pytest.raises(RuntimeError, match="MI355X only"):
        pose.two_view_geometry(a, a)
    with pytest.raises(ValueError, match="both or neither"):
        pose.two_view_geometry(a, a, intr0=(600.0, 600.0, 320.0, 240.0))
    with pytest.raises(TypeError, match="unexpected options"):
        pose.two_view_geometry(a, a, refine=True)
    for fn in (pycolmap_compat.fundamental_matrix_estimation, pycolmap_compat.homography_matrix_estimation):
        with pytest.raises(ValueError, match=r"must be \[n, 2\]"):
            fn(np.zeros((8, 3)), np.zeros((8, 2)))
        with pytest.raises(ValueError, match="8 points2D1 against 9 points2D2"):
            fn(np.zeros((8, 2)), np.zeros((9, 2)))


def test_two_view_tables_without_intrinsics_needs_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    kp = [np.zeros((60, 2)) for _ in range(3)]
    desc = [np.zeros((60, 128), np.uint8) for _ in range(3)]
    with pytest.raises(RuntimeError, match="no device found"):
        match.two_view_tables(kp, desc, intrinsic=None)
    with pytest.raises(RuntimeError, match="no device found"):
        match.two_view_tables(kp, desc, return_configs=True)
    for fn in (pycolmap_compat.fundamental_matrix_estimation, pycolmap_compat.homography_matrix_estimation):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(np.zeros((8, 2)), np.zeros((8, 2)))
