"""CPU: the absolute-pose restatement (tests/pose_restate.py) against ground truth and hand-computed values, the C ABI's
refusals (returned before any device work), and the pycolmap shim's argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import pose_restate as PR
from ls2fm import _lib, pose
from ls2fm.utils import pycolmap_compat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ls2fm_p3p", "ls2fm_absolute_pose_workspace_bytes", "ls2fm_absolute_pose", "ls2fm_pose_refine")


def random_rotation(rng):
    q = rng.normal(size=4)
    return pose.qvec_to_rotmat(q / np.linalg.norm(q))


def random_triple(rng):
    """a well-conditioned minimal problem: points 2-6 units in front of a random camera -> (bearings, world points, R, t)"""
    while True:
        R, t = random_rotation(rng), rng.normal(size=3)
        pc = np.concatenate([rng.uniform(-1, 1, (3, 2)), rng.uniform(2, 6, (3, 1))], axis=1)
        xw = (pc - t) @ R                          # R^T (pc - t)
        y = pc / np.linalg.norm(pc, axis=1, keepdims=True)
        if PR.well_conditioned(y, xw):
            return y, xw, R, t


def test_restated_p3p_recovers_the_pose():
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(300):
        y, x, R, t = random_triple(rng)
        errs = [max(np.abs(P[:, :3] - R).max(), np.abs(P[:, 3] - t).max() / np.linalg.norm(t)) for P in PR.p3p(y, x) if P is not None]
        assert errs, "no solution"
        worst = max(worst, min(errs))
    assert worst <= 1e-9, worst


def test_restated_p3p_degenerate_triples():
    y = np.eye(3)
    for x in (np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2.0]]), np.array([[0, 0, 0], [0, 0, 0], [1, 2, 3.0]]), np.zeros((3, 3))):
        assert PR.p3p(y, x) == [None] * 4


def test_sample_stream_fixed_vectors():
    # SplitMix64's published test vector (state 1234567: first output)
    assert PR.splitmix64(1234567) == 6457827717110365317
    # the header's definition, written out once more by hand for seed 0, trial 0
    z = (0 + 0x9E3779B97F4A7C15) % 2**64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2**64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2**64
    assert PR.splitmix64(0) == z ^ (z >> 31)
    assert PR.trial_key(0, 0) == PR.splitmix64(0 ^ PR.splitmix64(0))
    # recorded draws: the sample of trials 0..3 over 1000 correspondences, seed 0 and seed 7
    assert [PR.sample(0, t, 1000) for t in range(4)] == FIXED_SAMPLES_SEED0
    assert [PR.sample(7, t, 1000) for t in range(4)] == FIXED_SAMPLES_SEED7
    # always three distinct in-range indices, the key excludes the view
    for t in range(200):
        s = PR.sample(3, t, 5)
        assert s is not None and len(set(s)) == 3 and all(0 <= i < 5 for i in s)
    assert PR.sample(0, 0, 2) is None


FIXED_SAMPLES_SEED0 = [[138, 258, 574], [693, 423, 83], [98, 1, 602], [329, 691, 496]]
FIXED_SAMPLES_SEED7 = [[306, 40, 86], [967, 946, 846], [664, 96, 193], [751, 193, 305]]


@pytest.mark.parametrize("eps, want", [
    (0.5, math.ceil(math.log(1e-4) / math.log(1 - 0.125))),          # 69 -> clamped to min
    (0.2, math.ceil(math.log(1e-4) / math.log(1 - 0.008))),          # 1147
    (0.1, math.ceil(math.log(1e-4) / math.log(1 - 0.001))),          # 9206
    (0.01, 100000),                                                    # 9.2 M -> max
    (0.0, 100000), (1.0, 1000)])
def test_stopping_rule(eps, want):
    assert PR.num_trials(eps, 0.9999, 1000, 100000) == max(1000, min(100000, want))


def test_stopping_rule_hand_values():
    assert PR.num_trials(0.2, 0.9999, 0, 10**9) == 1147
    assert PR.num_trials(0.1, 0.9999, 0, 10**9) == 9206
    assert PR.num_trials(0.5, 0.99, 0, 10**9) == 35           # log(0.01) / log(0.875) = 34.49
    assert PR.max_trials_eff(0.9999, 0.01, 100000) == 100000
    assert PR.max_trials_eff(0.9999, 0.1, 100000) == 9206


def test_qvec_rotmat_round_trip():
    rng = np.random.default_rng(1)
    for _ in range(200):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        q = q if q[0] >= 0 else -q
        R = pose.qvec_to_rotmat(q)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert np.abs(pose.rotmat_to_qvec(R) - q).max() < 1e-12
    assert np.allclose(pose.qvec_to_rotmat([1, 0, 0, 0]), np.eye(3))


def test_restated_ransac_noise_free():
    rng = np.random.default_rng(2)
    R, t = random_rotation(rng), np.array([0.1, -0.2, 4.0])
    n = 200
    pc = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(3, 6, (n, 1))], axis=1)
    xyz = (pc - t) @ R
    intr = (500.0, 500.0, 320.0, 240.0)
    uv = np.stack([500 * pc[:, 0] / pc[:, 2] + 320, 500 * pc[:, 1] / pc[:, 2] + 240], axis=1)
    out = rng.random(n) < 0.3
    uv[out] += rng.uniform(30, 60, (int(out.sum()), 2)) * rng.choice([-1, 1], (int(out.sum()), 2))
    r = PR.absolute_pose(uv, xyz, intr, max_error_px=3.0, min_num_trials=100, max_num_trials=5000)
    assert r["success"] and np.array_equal(r["inliers"], ~out)
    assert np.abs(r["pose"] - np.concatenate([R, t[:, None]], axis=1)).max() < 1e-9
    assert r["trials"] == 1024


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    lib = _lib.load()
    for name in SYMS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    decl = re.search(r"int ls2fm_absolute_pose\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib._SIGNATURES["ls2fm_absolute_pose"][1]) == 14
    decl = re.search(r"int ls2fm_pose_refine\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib._SIGNATURES["ls2fm_pose_refine"][1]) == 11
    assert ctypes.sizeof(_lib.PoseRansacOpts) == 56


def test_workspace_bytes():
    lib = _lib.load()
    one = lib.ls2fm_absolute_pose_workspace_bytes(1, 1 << 20)
    assert 0 < one < 1 << 20
    assert lib.ls2fm_absolute_pose_workspace_bytes(1, 0) == one              # the correspondences need none
    assert lib.ls2fm_absolute_pose_workspace_bytes(40, 80000) >= 40 * 1024 * 48 * 8
    assert lib.ls2fm_absolute_pose_workspace_bytes(0, 10) == -1
    assert lib.ls2fm_absolute_pose_workspace_bytes(1, -1) == -1


def _opts(**kw):
    o = dict(max_error_px=12.0, confidence=0.9999, min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000, seed=0,
             refine=1)
    o.update(kw)
    return _lib.PoseRansacOpts(o["max_error_px"], o["confidence"], o["min_inlier_ratio"], o["min_num_trials"], o["max_num_trials"],
                               o["seed"], o["refine"])


@pytest.mark.parametrize("case", ["views", "view_start", "intr", "poses", "err0", "errneg", "conf0", "conf1", "ratio", "trials",
                                  "minmax", "refine", "opts"])
def test_absolute_pose_refusals(case):
    lib = _lib.load()
    fake, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)      # never dereferenced: every refusal comes first
    V = 0 if case == "views" else 1
    o = {"err0": _opts(max_error_px=0.0), "errneg": _opts(max_error_px=-1.0), "conf0": _opts(confidence=0.0),
         "conf1": _opts(confidence=1.0), "ratio": _opts(min_inlier_ratio=1.0), "trials": _opts(max_num_trials=0),
         "minmax": _opts(min_num_trials=10, max_num_trials=5), "refine": _opts(refine=2)}.get(case, _opts())
    assert lib.ls2fm_absolute_pose(fake, fake, nul if case == "view_start" else fake, V, nul if case == "intr" else fake,
                                   None if case == "opts" else ctypes.byref(o), nul if case == "poses" else fake, fake, fake, fake,
                                   fake, fake, fake, nul) == -1


def test_refine_and_p3p_refusals():
    lib = _lib.load()
    fake, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
    assert lib.ls2fm_pose_refine(fake, fake, fake, 0, fake, fake, fake, 1.0, 100, fake, nul) == -1
    assert lib.ls2fm_pose_refine(fake, fake, fake, 1, fake, fake, fake, 0.0, 100, fake, nul) == -1
    assert lib.ls2fm_pose_refine(fake, fake, fake, 1, fake, fake, fake, 1.0, -1, fake, nul) == -1
    assert lib.ls2fm_pose_refine(fake, fake, fake, 1, fake, nul, fake, 1.0, 100, fake, nul) == -1
    assert lib.ls2fm_p3p(fake, fake, -1, fake, fake, nul) == -1
    assert lib.ls2fm_p3p(nul, fake, 5, fake, fake, nul) == -1
    assert lib.ls2fm_p3p(nul, nul, 0, nul, nul, nul) == 0                  # nothing to do


# --------------------------------------------------------------------------------------------------------------- the shim
def test_shim_camera_models():
    c = pycolmap_compat.Camera(model="SIMPLE_PINHOLE", width=640, height=480, params=[500.0, 320.0, 240.0])
    assert np.array_equal(c.intrinsics, [500.0, 500.0, 320.0, 240.0])
    c = pycolmap_compat.Camera(model="PINHOLE", width=640, height=480, params=[500.0, 510.0, 320.0, 240.0])
    assert np.array_equal(c.intrinsics, [500.0, 510.0, 320.0, 240.0])
    with pytest.raises(NotImplementedError):
        pycolmap_compat.Camera(model="OPENCV", width=640, height=480, params=[1.0] * 8)
    with pytest.raises(ValueError):
        pycolmap_compat.Camera(model="SIMPLE_PINHOLE", width=640, height=480, params=[500.0, 320.0])
    with pytest.raises(NotImplementedError):
        pycolmap_compat.essential_matrix_estimation(np.zeros((8, 2)), np.zeros((8, 2)), c, c)


def test_shim_shape_checks_and_no_device(monkeypatch):
    cam = pycolmap_compat.Camera(model="SIMPLE_PINHOLE", width=640, height=480, params=[500.0, 320.0, 240.0])
    with pytest.raises(ValueError):
        pycolmap_compat.absolute_pose_estimation(np.zeros((10, 3)), np.zeros((10, 3)), cam)
    with pytest.raises(ValueError):
        pycolmap_compat.absolute_pose_estimation(np.zeros((10, 2)), np.zeros((9, 3)), cam)
    with pytest.raises(ValueError):
        pycolmap_compat.pose_refinement(np.zeros(3), [1, 0, 0, 0], np.zeros((10, 2)), np.zeros((10, 4)), np.ones(10, bool), cam)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pycolmap_compat.absolute_pose_estimation(np.zeros((10, 2)), np.zeros((10, 3)), cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pycolmap_compat.pose_refinement(np.zeros(3), [1, 0, 0, 0], np.zeros((10, 2)), np.zeros((10, 3)), np.ones(10, bool), cam)


def test_device_api_refuses_cpu_tensors():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.absolute_pose(torch.zeros(10, 2), torch.zeros(10, 3), torch.tensor([500.0, 500.0, 320.0, 240.0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.p3p(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3))
