"""CPU: the relative-pose restatement (tests/relpose_restate.py) against ground truth and np.roots, the C ABI's refusals
(returned before any device work), the pycolmap shim's SIMPLE_PINHOLE-only rule and the cv2 shim's checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import relpose_restate as RR
from ls2fm import _lib, pose
from ls2fm.utils import cv2_compat, pycolmap_compat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ls2fm_five_point", "ls2fm_relative_pose_workspace_bytes", "ls2fm_relative_pose", "ls2fm_triangulate")


def random_rotation(rng):
    q = rng.normal(size=4)
    return pose.qvec_to_rotmat(q / np.linalg.norm(q))


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def minimal_problem(rng):
    """five points 2-6 units in front of camera 1, in front of camera 2 -> (x1, x2 [5,2] normalised, unit E)"""
    while True:
        R, t = random_rotation(rng), rng.normal(size=3)
        t /= np.linalg.norm(t)
        X1 = np.concatenate([rng.uniform(-1, 1, (5, 2)), rng.uniform(2, 6, (5, 1))], axis=1)
        X2 = X1 @ R.T + t
        if (X2[:, 2] > 0.5).all():
            E = skew(t) @ R
            return X1[:, :2] / X1[:, 2:], X2[:, :2] / X2[:, 2:], E / np.linalg.norm(E)


def e_err(sols, E):
    return min((min(np.abs(S - E).max(), np.abs(S + E).max()) for S in sols), default=np.inf)


def test_restated_five_point_recovers_the_truth():
    rng = np.random.default_rng(0)
    errs = []
    for _ in range(200):
        x1, x2, E = minimal_problem(rng)
        sols = RR.five_point(x1, x2)
        assert len(sols) % 2 == 0 and len(sols) <= 10
        for S in sols:
            assert abs(np.linalg.norm(S) - 1) < 1e-12 and abs(np.linalg.det(S)) < 1e-8
        errs.append(e_err(sols, E))
    errs = np.array(errs)
    assert (errs <= 1e-9).mean() >= 0.98 and errs.max() <= 1e-6, (np.sort(errs)[-5:])


def test_restated_constraints_vanish_on_the_truth():
    # the generic polynomial arithmetic: every row of the 10 x 20 matrix evaluates to 0 at the true (x, y, z)
    rng = np.random.default_rng(1)
    for _ in range(20):
        x1, x2, E = minimal_problem(rng)
        basis = RR.nullspace5(x1, x2)
        c = np.linalg.lstsq(basis.T, E.reshape(9), rcond=None)[0]
        x, y, z = c[:3] / c[3]
        mono = np.array([x ** a * y ** b * z ** g for a, b, g in RR.MONOMIALS])
        A = RR.constraint_matrix(basis)
        assert np.abs(A @ mono).max() <= 1e-9 * np.abs(A).max() * np.abs(mono).max()


def test_sturm_roots_equal_np_roots():
    rng = np.random.default_rng(2)
    for _ in range(300):
        k = int(rng.integers(0, 6))
        real = np.sort(rng.uniform(-5, 5, k))
        cplx = rng.normal(size=((10 - k) // 2, 2))
        roots = list(real) + [complex(a, b + 0.5 * np.sign(b)) for a, b in cplx] + [complex(a, -(b + 0.5 * np.sign(b))) for a, b in cplx]
        c = np.real(np.poly(roots))[::-1] * rng.uniform(0.5, 2)            # ascending coefficients
        got = RR.sturm_roots(c)
        ref = np.sort(np.real([r for r in np.roots(c[::-1]) if abs(r.imag) < 1e-7]))
        assert len(got) == len(ref), (got, ref)
        assert np.allclose(got, ref, rtol=0, atol=1e-9 * max(1.0, np.abs(ref).max(initial=0))), (got, ref)


def test_restated_degenerate_samples():
    rng = np.random.default_rng(3)
    x1, x2, _ = minimal_problem(rng)
    x1[1], x2[1] = x1[0], x2[0]                                   # coincident correspondences
    assert RR.five_point(x1, x2) == []
    assert RR.five_point(np.zeros((5, 2)), np.zeros((5, 2))) == []
    assert RR.sturm_roots(np.zeros(11)) == []


def test_sample_stream_five_distinct():
    for t in range(200):
        s = RR.sample(3, t, 6)
        assert s is not None and len(set(s)) == 5 and all(0 <= i < 6 for i in s)
    assert RR.sample(0, 0, 4) is None
    assert RR.sample(0, 0, 1000)[:3] == [138, 258, 574]           # the absolute pose's stream (its first three draws)


def test_stopping_rule_uses_eps5():
    assert RR.num_trials(0.5, 0.999, 0, 10 ** 9) == int(np.ceil(np.log(0.001) / np.log(1 - 0.5 ** 5)))    # 218
    assert RR.num_trials(0.3, 0.999, 1000, 100000) == 2840
    assert RR.max_trials_eff(0.999, 0.01, 100000) == 100000


def test_restated_triangulation_and_pose_candidates():
    rng = np.random.default_rng(4)
    q = np.concatenate([[1.0], rng.normal(size=3) * 0.1])
    R, t = pose.qvec_to_rotmat(q / np.linalg.norm(q)), np.array([1.0, 0.2, -0.1])
    X = np.concatenate([rng.uniform(-1, 1, (20, 2)), rng.uniform(3, 6, (20, 1))], axis=1)
    X2 = X @ R.T + t
    assert (X2[:, 2] > 1).all()
    x1, x2 = X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]
    P = np.c_[R, t]
    H = RR.triangulate(np.eye(3, 4), P, x1, x2)
    assert np.abs(H[:, :3] / H[:, 3:] - X).max() < 1e-9
    E = skew(t / np.linalg.norm(t)) @ R
    pose_, front = RR.recover_pose(E, x1, x2)
    assert front == 20 and np.abs(pose_ - np.c_[R, t / np.linalg.norm(t)]).max() < 1e-9


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    lib = _lib.load()
    for name in SYMS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name, n in (("ls2fm_relative_pose", 16), ("ls2fm_triangulate", 9), ("ls2fm_five_point", 6)):
        decl = re.search(r"int " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]) == n, name


def test_workspace_bytes():
    lib = _lib.load()
    one = lib.ls2fm_relative_pose_workspace_bytes(1, 1 << 20)
    assert 1024 * 90 * 8 < one < 1 << 20
    assert lib.ls2fm_relative_pose_workspace_bytes(1, 0) == one
    assert lib.ls2fm_relative_pose_workspace_bytes(0, 10) == -1
    assert lib.ls2fm_relative_pose_workspace_bytes(1, -1) == -1


def _opts(**kw):
    o = dict(max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000, seed=0, refine=0)
    o.update(kw)
    return _lib.PoseRansacOpts(o["max_error_px"], o["confidence"], o["min_inlier_ratio"], o["min_num_trials"], o["max_num_trials"],
                               o["seed"], o["refine"])


@pytest.mark.parametrize("case", ["pairs", "pair_start", "intr0", "intr1", "E", "poses", "err0", "conf1", "ratio", "trials", "minmax",
                                  "refine", "opts"])
def test_relative_pose_refusals(case):
    lib = _lib.load()
    fake, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)      # never dereferenced: every refusal comes first
    P = 0 if case == "pairs" else 1
    o = {"err0": _opts(max_error_px=0.0), "conf1": _opts(confidence=1.0), "ratio": _opts(min_inlier_ratio=1.0),
         "trials": _opts(max_num_trials=0), "minmax": _opts(min_num_trials=10, max_num_trials=5), "refine": _opts(refine=1)}.get(case, _opts())
    f = lambda name: nul if case == name else fake                # noqa: E731
    assert lib.ls2fm_relative_pose(fake, fake, f("pair_start"), P, f("intr0"), f("intr1"), None if case == "opts" else ctypes.byref(o),
                                   f("E"), f("poses"), fake, fake, fake, fake, fake, fake, nul) == -1


def test_five_point_and_triangulate_refusals():
    lib = _lib.load()
    fake, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
    assert lib.ls2fm_five_point(fake, fake, -1, fake, fake, nul) == -1
    assert lib.ls2fm_five_point(nul, fake, 5, fake, fake, nul) == -1
    assert lib.ls2fm_five_point(nul, nul, 0, nul, nul, nul) == 0
    assert lib.ls2fm_triangulate(fake, fake, fake, fake, fake, 0, 10, fake, nul) == -1
    assert lib.ls2fm_triangulate(nul, fake, fake, fake, fake, 1, 10, fake, nul) == -1
    assert lib.ls2fm_triangulate(fake, fake, fake, fake, fake, 1, -1, fake, nul) == -1
    assert lib.ls2fm_triangulate(fake, fake, fake, fake, nul, 1, 10, fake, nul) == -1
    assert lib.ls2fm_triangulate(fake, fake, nul, fake, fake, 1, 10, fake, nul) == -1
    assert lib.ls2fm_triangulate(fake, fake, nul, nul, fake, 1, 0, nul, nul) == 0


# --------------------------------------------------------------------------------------------------------------- the shims
def test_essential_shim_takes_simple_pinhole_only(monkeypatch):
    simple = pycolmap_compat.Camera(model="SIMPLE_PINHOLE", width=640, height=480, params=[500.0, 320.0, 240.0])
    pin = pycolmap_compat.Camera(model="PINHOLE", width=640, height=480, params=[500.0, 510.0, 320.0, 240.0])
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for a, b in ((pin, pin), (simple, pin), (pin, simple)):
        with pytest.raises(NotImplementedError, match="SIMPLE_PINHOLE"):
            pycolmap_compat.essential_matrix_estimation(np.zeros((8, 2)), np.zeros((8, 2)), a, b)
        with pytest.raises(NotImplementedError):                 # before any shape check
            pycolmap_compat.essential_matrix_estimation(np.zeros((8, 3)), np.zeros((7, 2)), a, b)
    with pytest.raises(ValueError):
        pycolmap_compat.essential_matrix_estimation(np.zeros((8, 3)), np.zeros((8, 2)), simple, simple)
    with pytest.raises(ValueError):
        pycolmap_compat.essential_matrix_estimation(np.zeros((8, 2)), np.zeros((7, 2)), simple, simple)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pycolmap_compat.essential_matrix_estimation(np.zeros((8, 2)), np.zeros((8, 2)), simple, simple)


def test_cv2_shim_checks(monkeypatch):
    P = np.eye(3, 4)
    with pytest.raises(ValueError):
        cv2_compat.triangulatePoints(np.eye(3), P, np.zeros((2, 5)), np.zeros((2, 5)))
    with pytest.raises(ValueError):
        cv2_compat.triangulatePoints(P, P, np.zeros((5, 2)), np.zeros((5, 2)))
    with pytest.raises(ValueError):
        cv2_compat.triangulatePoints(P, P, np.zeros((2, 5)), np.zeros((2, 4)))
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv2_compat.triangulatePoints(P, P, np.zeros((2, 5)), np.zeros((2, 5)))


def test_device_api_refuses_cpu_tensors():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.relative_pose(torch.zeros(10, 2), torch.zeros(10, 2), torch.tensor([500.0, 500.0, 320.0, 240.0]),
                           torch.tensor([500.0, 500.0, 320.0, 240.0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.five_point(torch.zeros(1, 5, 2), torch.zeros(1, 5, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.triangulate(torch.eye(3, 4), torch.eye(3, 4), torch.zeros(3, 2), torch.zeros(3, 2))
