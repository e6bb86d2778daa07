#!/usr/bin/env python
"""Record tests/golden/ransac_parent.npz / .json: the inputs and every output of ls2fm.pose.absolute_pose (refine off and on),
fundamental_matrix, homography and the four minimal solvers on an MI355X, for tests/test_hip_ransac_bits.py.  Run it with the
library whose bits are to be kept (LS2FM_LIB names another build than the tree's); the scenes are the tests' own generators.
relative_pose has its own fixture (relative_pose_parent.*).
    python tests/golden/make_golden_ransac_parent.py [--out tests/golden]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd"), os.path.join(ROOT, "tests")]

import test_hip_absolute_pose as TA  # noqa: E402
import test_hip_relative_pose as TR  # noqa: E402
import twoview_scenes as S  # noqa: E402
from ls2fm import _lib, pose  # noqa: E402

DEV = "cuda:0"
ABS_OPTS = dict(max_error_px=4.0, seed=17)
TV_OPTS = dict(seed=9)
KEYS = ("inliers", "num_inliers", "trials", "best_trial", "success")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cat(parts):
    return np.concatenate([np.asarray(p, dtype=np.float64).reshape(len(p), -1) for p in parts])


def starts(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)


def absolute_views(rng):
    """1100 correspondences (two scoring tiles); 88 % outliers (more than one round); exactly 3 (a pose, no success); 2 (below the sample)"""
    return [TA.scene(rng, 1100, 0.3, 0.5)[:2], TA.scene(rng, 300, 0.88, 0.5)[:2], TA.scene(rng, 3)[:2], TA.scene(rng, 2)[:2]]


def f_pairs(rng):
    """1100; 65 % outliers (more than one round); 7 random pixels against 7 (no fundamental matrix has 8 inliers); 6 (below the sample)"""
    noise = (rng.uniform((0, 0), (640, 480), (7, 2)), rng.uniform((0, 0), (640, 480), (7, 2)))
    return [S.general_scene(rng, 1100, 0.3, 0.5)[:2], S.general_scene(rng, 400, 0.65, 0.5)[:2], noise, S.general_scene(rng, 6)[:2]]


def h_pairs(rng):
    """1100; 75 % outliers (more than one round); 12 pixels of one line against random pixels (every sample is collinear: no
    homography, so no pair of this kind reaches 4 inliers); 3 (below the sample)"""
    s = rng.uniform(0, 1, (12, 1))
    line = np.array([[50.0, 60.0]]) + s * np.array([[500.0, 350.0]])
    noise = (line, rng.uniform((0, 0), (640, 480), (12, 2)))
    return [S.planar_scene(rng, 1100, 0.3, 0.5)[:2], S.planar_scene(rng, 400, 0.75, 0.5)[:2], noise, S.planar_scene(rng, 3)[:2]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    rng = np.random.default_rng(80)
    out = {}

    views = absolute_views(rng)
    uv, xyz, vs = cat([v[0] for v in views]), cat([v[1] for v in views]), starts([v[0] for v in views])
    out.update(abs_uv=uv, abs_xyz=xyz, abs_view_start=vs)
    K = dev(np.array(TA.INTR))
    for refine in (False, True):
        r = pose.absolute_pose(dev(uv), dev(xyz), K, dev(vs), refine=refine, **ABS_OPTS)
        for key in ("poses",) + KEYS:
            out[f"abs_refine{int(refine)}_{key}"] = r[key].cpu().numpy()
    tr, ok = out["abs_refine0_trials"], out["abs_refine0_success"]
    assert tr[1] > 1024 and ok[:2].all() and not ok[2:].any() and tr[2] >= 1024 and tr[3] == 0, (tr, ok)     # success needs 4 inliers

    for which, fn, pairs in (("F", pose.fundamental_matrix, f_pairs(rng)), ("H", pose.homography, h_pairs(rng))):
        uv0, uv1, ps = cat([p[0] for p in pairs]), cat([p[1] for p in pairs]), starts([p[0] for p in pairs])
        out.update({f"{which}_uv0": uv0, f"{which}_uv1": uv1, f"{which}_pair_start": ps})
        r = fn(dev(uv0), dev(uv1), dev(ps), **TV_OPTS)
        for key in (which,) + KEYS:
            out[f"{which}_{key}"] = r[key].cpu().numpy()
        tr, ok, num = out[f"{which}_trials"], out[f"{which}_success"], out[f"{which}_num_inliers"]
        assert tr[1] > 1024 and ok[:2].all() and not ok[2:].any() and tr[2] >= 1024 and tr[3] == 0 and (num[2:] == 0).all(), (tr, ok, num)

    y, x, _ = TA.random_triples(rng, 64)
    yd = np.tile(np.eye(3)[None], (4, 1, 1))
    xd = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2.0]], [[0, 0, 0], [0, 0, 0], [1, 2, 3.0]], np.zeros((3, 3)),
                   [[1, 2, 3], [1, 2, 3], [1, 2, 3.0]]])                  # test_p3p_degenerate_triples_give_no_solution's
    x1, x2, _ = TR.minimal_problems(rng, 64)
    d1, d2, _ = TR.minimal_problems(rng, 3)                               # test_five_point_degenerate_samples'
    d1[0, 1], d2[0, 1] = d1[0, 0], d2[0, 0]
    d1[1], d2[1] = 0.0, 0.0
    d1[2, :, 1], d2[2, :, 1] = 0.0, 0.0
    d1, d2 = np.concatenate([d1, np.full((1, 5, 2), np.nan)]), np.concatenate([d2, np.zeros((1, 5, 2))])
    a7, b7, _ = S.seven_point_problems(rng, 64)
    da7, db7 = S.degenerate_seven(rng)
    a4, b4, _ = S.four_point_problems(rng, 64)
    da4, db4 = S.degenerate_four(rng)
    for name, fn, a, b in (("p3p", pose.p3p, np.concatenate([y, yd]), np.concatenate([x, xd])),
                           ("five_point", pose.five_point, np.concatenate([x1, d1]), np.concatenate([x2, d2])),
                           ("seven_point", pose.seven_point, np.concatenate([a7, da7]), np.concatenate([b7, db7])),
                           ("four_point", pose.four_point_homography, np.concatenate([a4, da4]), np.concatenate([b4, db4]))):
        sol, n = fn(dev(a), dev(b))
        out.update({f"{name}_a": a, f"{name}_b": b, f"{name}_out": sol.cpu().numpy(), f"{name}_n": n.cpu().numpy()})
        k = len(a) - 64
        assert (out[f"{name}_n"][:64] >= 1).all() and (out[f"{name}_n"][64:] == 0).all() and k >= 3, (name, out[f"{name}_n"])

    note = dict(what="inputs and outputs of ls2fm.pose.absolute_pose (refine False / True), fundamental_matrix, homography, p3p, "
                     "five_point, seven_point and four_point_homography, recorded on an MI355X from the library built at the commit "
                     "before csrc/two_view.h existed",
                made_by="tests/golden/make_golden_ransac_parent.py, numpy default_rng(80)",
                intrinsics=list(TA.INTR), absolute_pose_options=ABS_OPTS, two_view_options=TV_OPTS,
                views=absolute_views.__doc__, F_pairs=" ".join(f_pairs.__doc__.split()), H_pairs=" ".join(h_pairs.__doc__.split()),
                minimal="64 random problems each, then the degenerate ones of the test_*_degenerate_* tests",
                device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH),
                abs_trials=out["abs_refine0_trials"].tolist(), abs_num_inliers=out["abs_refine0_num_inliers"].tolist(),
                F_trials=out["F_trials"].tolist(), F_num_inliers=out["F_num_inliers"].tolist(), F_best_trial=out["F_best_trial"].tolist(),
                H_trials=out["H_trials"].tolist(), H_num_inliers=out["H_num_inliers"].tolist(), H_best_trial=out["H_best_trial"].tolist())
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "ransac_parent.npz"), **out)
    with open(os.path.join(args.out, "ransac_parent.json"), "w") as f:
        json.dump(note, f, indent=1)
    print(json.dumps(note, indent=1))


if __name__ == "__main__":
    main()
