"""GPU: every output bit of ls2fm.pose.absolute_pose, fundamental_matrix, homography and the four minimal solvers against what the
library of the commit before csrc/two_view.h produced on an MI355X (tests/golden/ransac_parent.npz, recorded by
tests/golden/make_golden_ransac_parent.py).  The build is -ffp-contract=off and every reduction is fixed-order, so there is no
tolerance: only a moved operation changes a bit.  relative_pose has its own fixture (test_hip_two_view.py)."""
import json
import os

import numpy as np
import pytest
import torch

from ls2fm import pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("inliers", "num_inliers", "trials", "best_trial", "success")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ransac_parent.json")) as f:
        note = json.load(f)
    return np.load(os.path.join(GOLDEN, "ransac_parent.npz")), note


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("refine", [False, True])
def test_absolute_pose_bits_unchanged(golden, refine):
    g, note = golden
    r = pose.absolute_pose(dev(g["abs_uv"]), dev(g["abs_xyz"]), dev(np.array(note["intrinsics"])), dev(g["abs_view_start"]),
                           refine=refine, **note["absolute_pose_options"])
    for key in ("poses",) + KEYS:
        same(r[key], g[f"abs_refine{int(refine)}_{key}"], key)
    # the fixture itself: 1100 (two scoring tiles), 300 at 88 % outliers (more than one round), 3 (a pose, no success) and 2 correspondences
    assert np.diff(g["abs_view_start"]).tolist() == [1100, 300, 3, 2]
    tr, ok, num = (g[f"abs_refine{int(refine)}_{k}"] for k in ("trials", "success", "num_inliers"))
    assert tr[1] > 1024 and tr[2] >= 1024 and tr[3] == 0 and ok.tolist() == [True, True, False, False]      # success needs 4 inliers
    assert (num[:2] >= [700, 33]).all() and num[2:].tolist() == [3, 0]
    assert np.array_equal(g[f"abs_refine{int(refine)}_poses"][3], np.eye(3, 4))
    if refine:
        assert not np.array_equal(g["abs_refine1_poses"][:2], g["abs_refine0_poses"][:2])


@pytest.mark.parametrize("which, fn, sizes, least", [("F", pose.fundamental_matrix, [1100, 400, 7, 6], [700, 130]),
                                                       ("H", pose.homography, [1100, 400, 12, 3], [700, 90])])
def test_two_view_bits_unchanged(golden, which, fn, sizes, least):
    g, note = golden
    r = fn(dev(g[f"{which}_uv0"]), dev(g[f"{which}_uv1"]), dev(g[f"{which}_pair_start"]), **note["two_view_options"])
    for key in (which,) + KEYS:
        same(r[key], g[f"{which}_{key}"], key)
    # the fixture itself: one pair of more than a scoring tile, one of more than one round, one that ran and failed, one never run
    assert np.diff(g[f"{which}_pair_start"]).tolist() == sizes
    tr, ok, num, ps = (g[f"{which}_{k}"] for k in ("trials", "success", "num_inliers", "pair_start"))
    assert tr[1] > 1024 and tr[2] >= 1024 and tr[3] == 0 and ok.tolist() == [True, True, False, False]
    assert (num[:2] >= least).all() and (num[2:] == 0).all()
    assert not g[f"{which}_{which}"][2:].any() and not g[f"{which}_inliers"][ps[2]:].any()


@pytest.mark.parametrize("name, fn", [("p3p", pose.p3p), ("five_point", pose.five_point), ("seven_point", pose.seven_point),
                                      ("four_point", pose.four_point_homography)])
def test_minimal_solver_bits_unchanged(golden, name, fn):
    g, _ = golden
    out, n = fn(dev(g[f"{name}_a"]), dev(g[f"{name}_b"]))
    same(out, g[f"{name}_out"], name)
    same(n, g[f"{name}_n"], name)
    # the fixture itself: 64 solvable problems, then degenerate ones without a solution
    assert len(g[f"{name}_n"]) >= 67 and (g[f"{name}_n"][:64] >= 1).all() and (g[f"{name}_n"][64:] == 0).all()
    assert g[f"{name}_out"][:64].any() and not g[f"{name}_out"][64:].any()
