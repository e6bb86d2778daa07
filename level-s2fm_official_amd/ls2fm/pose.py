"""Absolute and relative pose on the device: what Registration.PnP (pipelines/Registration.py:94-109 of the reference) and
Initializer (pipelines/Initialization.py:86-95) ask of pycolmap, and the _Trad drivers of cv2.triangulatePoints.

`absolute_pose` runs LO-RANSAC (Lambda Twist P3P, Gauss-Newton local optimisation, Cauchy-loss Levenberg-Marquardt refinement)
for one or MANY views in one call of ls2fm_absolute_pose (csrc/absolute_pose.hip) -- the next-best-view search of
LevelS2fM.train (pipelines/LevelS2fM.py:247-281) forms every candidate view's pnp score from one call instead of one host round
trip per view.  `refine_pose` is pose_refinement alone (ls2fm_pose_refine), `p3p` the minimal solver alone.  `relative_pose`
runs LO-RANSAC over Nister's five-point algorithm and recovers [R | t] for one or many view pairs (ls2fm_relative_pose,
csrc/relative_pose.hip); `five_point` is the minimal solver alone and `triangulate` the batched two-view DLT.
`fundamental_matrix` and `homography` are the uncalibrated LO-RANSACs in pixels (csrc/two_view.hip; `seven_point` and
`four_point_homography` their minimal solvers) and `two_view_geometry` COLMAP's verdict over their inlier counts.  Every rule is
stated in include/ls2fm.h; tests/pose_restate.py, tests/relpose_restate.py and tests/twoview_restate.py repeat them in numpy.

Poses are world-to-camera [3,4] = [R | t], fp64; intrinsics per view (fx, fy, cx, cy).  The defaults are pycolmap 0.3.0's
absolute_pose_estimation defaults as we read them.  There is no CPU path: CPU tensors, a missing device or a missing library raise.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


_device = functools.partial(_lib.require_device_tensors, "ls2fm.pose")


def _f64(t, shape_tail, what):
    t = torch.as_tensor(t)
    _device(t)
    if t.dim() < 1 or tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"ls2fm.pose: {what} must have shape [n, {', '.join(map(str, shape_tail))}], got {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def _intrinsics(intr, n_views, dev):
    """[V,4] / [4] (fx, fy, cx, cy) or [V,3,3] / [3,3] K -> [V,4] fp64 on the device"""
    k = torch.as_tensor(intr, dtype=torch.float64, device=dev)
    if k.shape[-2:] == (3, 3):
        k = k.reshape(-1, 3, 3)
        k = torch.stack([k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2]], dim=1)
    k = k.reshape(-1, 4)
    if k.shape[0] == 1 and n_views > 1:
        k = k.expand(n_views, 4)
    if k.shape[0] != n_views:
        raise ValueError(f"ls2fm.pose: {k.shape[0]} intrinsics for {n_views} views")
    return k.contiguous()


def _ragged(uv, xyz, view_start):
    """(uv [n,2], xyz [n,3], view_start int32 [V+1]) on the device from tensors or lists of per-view tensors"""
    return _ragged_common(uv, xyz, view_start, (3,), "uv", "xyz", "view_start")


def _ransac(symbol, a, b, starts, extra_in, model_out, max_error_px, confidence, min_inlier_ratio, min_num_trials, max_num_trials, seed,
            refine=False):
    """One LO-RANSAC entry of the library: ls2fm_<symbol>(a, b, starts, G, *extra_in, opts, *model_out, inliers, num_inliers, trials,
    best_trial, success, workspace, stream) with its workspace -> the dict entries every estimator returns"""
    G, n, dev = starts.numel() - 1, a.shape[0], a.device
    lib = _lib.load()
    opts = _lib.PoseRansacOpts(float(max_error_px), float(confidence), float(min_inlier_ratio), int(min_num_trials),
                               int(max_num_trials), int(seed) & ((1 << 64) - 1), 1 if refine else 0)
    ws = _lib.workspace(getattr(lib, symbol + "_workspace_bytes")(G, n), symbol + "_workspace_bytes", dev)
    inl = torch.empty(n, dtype=torch.uint8, device=dev)
    num, trials, best, succ = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(4))
    check(getattr(lib, symbol)(ptr(a), ptr(b), ptr(starts), G, *map(ptr, extra_in), ctypes.byref(opts), *map(ptr, model_out), ptr(inl),
                               ptr(num), ptr(trials), ptr(best), ptr(succ), ptr(ws), stream_ptr()), symbol)
    return dict(inliers=inl.view(torch.bool), num_inliers=num, trials=trials, best_trial=best, success=succ.bool())


def p3p(bearings, points):
    """Lambda Twist P3P of m minimal problems: bearings [m,3,3] (unit rows), points [m,3,3] (device) -> (poses [m,4,3,4] fp64,
    kept ones first, zero beyond; n_solutions int32 [m])"""
    b = torch.as_tensor(bearings)
    x = torch.as_tensor(points)
    _device(b, x)
    b = b.to(torch.float64).reshape(-1, 3, 3).contiguous()
    x = x.to(torch.float64).reshape(-1, 3, 3).contiguous()
    if b.shape != x.shape:
        raise ValueError(f"ls2fm.pose.p3p: bearings {tuple(b.shape)} against points {tuple(x.shape)}")
    m = b.shape[0]
    poses = torch.empty(m, 4, 3, 4, dtype=torch.float64, device=b.device)
    n = torch.empty(m, dtype=torch.int32, device=b.device)
    check(_lib.load().ls2fm_p3p(ptr(b), ptr(x), m, ptr(poses), ptr(n), stream_ptr()), "ls2fm_p3p")
    return poses, n


def absolute_pose(uv, xyz, intrinsics, view_start=None, max_error_px=12.0, confidence=0.9999, min_inlier_ratio=0.01,
                  min_num_trials=1000, max_num_trials=100000, seed=0, refine=True):
    """LO-RANSAC absolute pose of V views in one call.  uv [n,2] pixels, xyz [n,3] world points (device; float64 is used
    throughout), sorted by view with view_start [V+1] (None: one view), or lists of per-view tensors; intrinsics [V,4] / [4]
    (fx, fy, cx, cy) or K [V,3,3] / [3,3].  -> dict(poses [V,3,4] fp64 world-to-camera, inliers bool [n], num_inliers,
    trials, best_trial, success (int32 / bool [V]))"""
    uv, xyz, vs = _ragged(uv, xyz, view_start)
    V = vs.numel() - 1
    dev = uv.device
    intr = _intrinsics(intrinsics, V, dev)
    poses = torch.empty(V, 3, 4, dtype=torch.float64, device=dev)
    r = _ransac("ls2fm_absolute_pose", uv, xyz, vs, (intr,), (poses,), max_error_px, confidence, min_inlier_ratio, min_num_trials,
                max_num_trials, seed, refine)
    return dict(poses=poses, **r, view_start=vs)


def refine_pose(uv, xyz, intrinsics, poses, mask, view_start=None, loss_scale_px=1.0, max_iters=100):
    """pose_refinement on a fixed mask: Levenberg-Marquardt with the Cauchy loss c^2 log(1 + s / c^2), c = loss_scale_px.
    poses [V,3,4] (or [3,4]) world-to-camera, mask bool [n] -> refined poses [V,3,4] fp64"""
    uv, xyz, vs = _ragged(uv, xyz, view_start)
    V = vs.numel() - 1
    dev = uv.device
    intr = _intrinsics(intrinsics, V, dev)
    p = torch.as_tensor(poses, device=dev).to(torch.float64).reshape(-1, 3, 4).contiguous()
    if p.shape[0] != V:
        raise ValueError(f"ls2fm.pose.refine_pose: {p.shape[0]} poses for {V} views")
    m = torch.as_tensor(mask, device=dev).reshape(-1)
    if m.numel() != uv.shape[0]:
        raise ValueError(f"ls2fm.pose.refine_pose: mask of {m.numel()} for {uv.shape[0]} correspondences")
    m = m.to(torch.uint8).contiguous()
    out = torch.empty_like(p)
    check(_lib.load().ls2fm_pose_refine(ptr(uv), ptr(xyz), ptr(vs), V, ptr(intr), ptr(m), ptr(p), float(loss_scale_px),
                                        int(max_iters), ptr(out), stream_ptr()), "ls2fm_pose_refine")
    return out


# ---------------------------------------------------------------------------------------------------- COLMAP's quaternions
def qvec_to_rotmat(qvec):
    """COLMAP's (w, x, y, z) quaternion -> 3 x 3 rotation (numpy float64)"""
    w, x, y, z = np.asarray(qvec, dtype=np.float64).reshape(4)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def rotmat_to_qvec(R):
    """3 x 3 rotation -> unit (w, x, y, z) with w >= 0 (COLMAP's convention), Shepperd's method"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = np.array([(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s])
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s])
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


# ----------------------------------------------------------------------------------------------------------- relative pose
def _ragged_pairs(uv0, uv1, pair_start):
    """(uv0 [n,2], uv1 [n,2], pair_start int32 [P+1]) on the device from tensors or lists of per-pair tensors"""
    return _ragged_common(uv0, uv1, pair_start, (2,), "uv0", "uv1", "pair_start")


def _ragged_common(a, b, starts, tail_b, name_a, name_b, name_s):
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(b) != len(a) or len(a) == 0:
            raise ValueError(f"ls2fm.pose: {name_a} and {name_b} lists must have the same non-zero length")
        if starts is not None:
            raise ValueError(f"ls2fm.pose: {name_s} is implied by lists of per-view / per-pair tensors")
        dev = torch.as_tensor(a[0]).device
        As = [torch.as_tensor(u).reshape(-1, 2) for u in a]
        Bs = [torch.as_tensor(x).reshape(-1, *tail_b) for x in b]
        for u, x in zip(As, Bs):
            if u.shape[0] != x.shape[0]:
                raise ValueError(f"ls2fm.pose: {u.shape[0]} {name_a} rows against {x.shape[0]} {name_b} rows")
        counts = [u.shape[0] for u in As]
        st = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)
        return (_f64(torch.cat(As).to(dev), (2,), name_a), _f64(torch.cat(Bs).to(dev), tail_b, name_b), st)
    a = _f64(a, (2,), name_a)
    b = _f64(b, tail_b, name_b)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"ls2fm.pose: {a.shape[0]} {name_a} rows against {b.shape[0]} {name_b} rows")
    if starts is None:
        starts = torch.tensor([0, a.shape[0]], dtype=torch.int32, device=a.device)
    starts = torch.as_tensor(starts, device=a.device).to(torch.int32).contiguous()
    if starts.dim() != 1 or starts.numel() < 2:
        raise ValueError(f"ls2fm.pose: {name_s} must be 1-D, one entry more than there are views / pairs")
    if not torch.cuda.is_current_stream_capturing():
        # the kernels index the correspondences (and masks) through the start array: it must cover exactly [0, n), in order
        h = starts.cpu()
        if int(h[0]) != 0 or int(h[-1]) != a.shape[0] or bool((h[1:] < h[:-1]).any()):
            raise ValueError(f"ls2fm.pose: {name_s} must rise from 0 to the {a.shape[0]} correspondences, "
                             f"got {h[0].item()} .. {h[-1].item()}")
    return a, b, starts


def five_point(x1, x2):
    """Nister's five-point solver of m minimal problems: normalised points x1, x2 [m,5,2] (device) -> (E [m,10,3,3] fp64, unit
    Frobenius norm, kept ones first and zero beyond; n_solutions int32 [m])"""
    return _minimal(x1, x2, 5, 10, "ls2fm_five_point", "five_point", "x1", "x2")


def relative_pose(uv0, uv1, intr0, intr1, pair_start=None, max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.01,
                  min_num_trials=1000, max_num_trials=100000, seed=0):
    """LO-RANSAC relative pose of P view pairs in one call (ls2fm_relative_pose).  uv0 / uv1 [n,2] pixels of the two views,
    sorted by pair with pair_start [P+1] (None: one pair), or lists of per-pair tensors; intr0 / intr1 [P,4] / [4]
    (fx, fy, cx, cy) or K [P,3,3] / [3,3] of each pair's first and second camera.  -> dict(E [P,3,3], poses [P,3,4] fp64 with
    X2 = R X1 + t and |t| = 1, inliers bool [n], num_inliers, trials, best_trial, success, pair_start)"""
    uv0, uv1, ps = _ragged_pairs(uv0, uv1, pair_start)
    P = ps.numel() - 1
    dev = uv0.device
    k0 = _intrinsics(intr0, P, dev)
    k1 = _intrinsics(intr1, P, dev)
    E = torch.empty(P, 3, 3, dtype=torch.float64, device=dev)
    poses = torch.empty(P, 3, 4, dtype=torch.float64, device=dev)
    r = _ransac("ls2fm_relative_pose", uv0, uv1, ps, (k0, k1), (E, poses), max_error_px, confidence, min_inlier_ratio, min_num_trials,
                max_num_trials, seed)
    return dict(E=E, poses=poses, **r, pair_start=ps)


def triangulate(P0, P1, uv0, uv1, pair_start=None):
    """two-view DLT (cv2.triangulatePoints' system, one-sided Jacobi): projection matrices P0 / P1 [P,3,4] (or [3,4]), pixel pairs
    uv0 / uv1 [n,2] sorted by pair (pair_start [P+1]; None: one pair) -> homogeneous points [n,4] fp64, unit norm, w >= 0"""
    uv0, uv1, ps = _ragged_pairs(uv0, uv1, pair_start)
    P = ps.numel() - 1
    dev = uv0.device
    a = torch.as_tensor(P0)
    b = torch.as_tensor(P1)
    _device(a, b)
    a = a.to(device=dev, dtype=torch.float64).reshape(-1, 3, 4).contiguous()
    b = b.to(device=dev, dtype=torch.float64).reshape(-1, 3, 4).contiguous()
    if a.shape[0] != P or b.shape[0] != P:
        raise ValueError(f"ls2fm.pose.triangulate: {a.shape[0]} / {b.shape[0]} projection matrices for {P} pairs")
    X = torch.empty(uv0.shape[0], 4, dtype=torch.float64, device=dev)
    check(_lib.load().ls2fm_triangulate(ptr(a), ptr(b), ptr(uv0), ptr(uv1), ptr(ps), P, uv0.shape[0], ptr(X), stream_ptr()),
          "ls2fm_triangulate")
    return X


# ------------------------------------------------------------------------------------------------- uncalibrated two-view geometry
# COLMAP's TwoViewGeometry::ConfigurationType values
DEGENERATE, CALIBRATED, UNCALIBRATED, PLANAR_OR_PANORAMIC = 1, 2, 3, 6


def _minimal(x1, x2, k, n_sol, symbol, name, name_a="uv0", name_b="uv1"):
    a = torch.as_tensor(x1)
    b = torch.as_tensor(x2)
    _device(a, b)
    a = a.to(torch.float64).reshape(-1, k, 2).contiguous()
    b = b.to(torch.float64).reshape(-1, k, 2).contiguous()
    if a.shape != b.shape:
        raise ValueError(f"ls2fm.pose.{name}: {name_a} {tuple(a.shape)} against {name_b} {tuple(b.shape)}")
    m = a.shape[0]
    out = torch.empty(m, n_sol, 3, 3, dtype=torch.float64, device=a.device)
    n = torch.empty(m, dtype=torch.int32, device=a.device)
    check(getattr(_lib.load(), symbol)(ptr(a), ptr(b), m, ptr(out), ptr(n), stream_ptr()), symbol)
    return out, n


def seven_point(uv0, uv1):
    """seven-point fundamental matrices of m minimal problems: pixels uv0, uv1 [m,7,2] (device) -> (F [m,3,3,3] fp64 with
    x2h^T F x1h = 0, unit Frobenius norm, kept ones first and zero beyond; n_solutions int32 [m])"""
    return _minimal(uv0, uv1, 7, 3, "ls2fm_seven_point", "seven_point")


def four_point_homography(uv0, uv1):
    """four-point DLT homographies of m minimal problems: pixels uv0, uv1 [m,4,2] (device) -> (H [m,3,3] fp64 with x2h ~ H x1h,
    unit Frobenius norm, zero where there is none; n_solutions int32 [m], 0 or 1)"""
    H, n = _minimal(uv0, uv1, 4, 1, "ls2fm_four_point_homography", "four_point_homography")
    return H[:, 0], n


def _two_view_ransac(symbol, key, uv0, uv1, ps, **opts):
    M = torch.empty(ps.numel() - 1, 3, 3, dtype=torch.float64, device=uv0.device)
    return {key: M, **_ransac(symbol, uv0, uv1, ps, (), (M,), **opts), "pair_start": ps}


def fundamental_matrix(uv0, uv1, pair_start=None, max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.25, min_num_trials=100,
                       max_num_trials=10000, seed=0):
    """LO-RANSAC fundamental matrix of P view pairs in one call (ls2fm_fundamental_matrix): seven-point hypotheses scored by the
    squared Sampson error in pixels, no intrinsics.  uv0 / uv1 and pair_start as `relative_pose`; the defaults are COLMAP's
    two-view geometry RANSAC options.  -> dict(F [P,3,3] fp64 with x2h^T F x1h = 0 (zero for a failing pair), inliers bool [n],
    num_inliers, trials, best_trial, success (num_inliers >= 8), pair_start)"""
    uv0, uv1, ps = _ragged_pairs(uv0, uv1, pair_start)
    return _two_view_ransac("ls2fm_fundamental_matrix", "F", uv0, uv1, ps, max_error_px=max_error_px, confidence=confidence,
                            min_inlier_ratio=min_inlier_ratio, min_num_trials=min_num_trials, max_num_trials=max_num_trials, seed=seed)


def homography(uv0, uv1, pair_start=None, max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.25, min_num_trials=100,
               max_num_trials=10000, seed=0):
    """LO-RANSAC homography of P view pairs in one call (ls2fm_homography): four-point DLT hypotheses scored by the squared
    forward transfer error |pi(H x1h) - x2|^2 in pixels.  Arguments as `fundamental_matrix`.  -> dict(H [P,3,3] fp64 with
    x2h ~ H x1h (zero for a failing pair), inliers, num_inliers, trials, best_trial, success (num_inliers >= 4), pair_start)"""
    uv0, uv1, ps = _ragged_pairs(uv0, uv1, pair_start)
    return _two_view_ransac("ls2fm_homography", "H", uv0, uv1, ps, max_error_px=max_error_px, confidence=confidence,
                            min_inlier_ratio=min_inlier_ratio, min_num_trials=min_num_trials, max_num_trials=max_num_trials, seed=seed)


def two_view_config(nE, okE, nF, okF, nH, min_num_inliers=15, min_E_F_inlier_ratio=0.95, max_H_inlier_ratio=0.8):
    """The verdict of `two_view_geometry` from the per-pair inlier counts and success flags (integer / bool tensors on any
    device; nE / okE None: no calibration) -> (config int32, choice int64: 0 = E's, 1 = F's, 2 = H's inlier set, -1 = none).
    Torch ops only: nothing is read back."""
    nF = torch.as_tensor(nF).to(torch.int64)
    nH = torch.as_tensor(nH, device=nF.device).to(torch.int64)
    okF = torch.as_tensor(okF, device=nF.device).bool()
    uncal = okF & (nF >= min_num_inliers)
    if nE is None:
        cal = torch.zeros_like(uncal)
        nE = torch.zeros_like(nF)
    else:
        nE = torch.as_tensor(nE, device=nF.device).to(torch.int64)
        okE = torch.as_tensor(okE, device=nF.device).bool()
        # nE / nF > ratio with nF = 0 is +inf or NaN in COLMAP's doubles: true only for nE > 0
        ratio = nE.double() / nF.double()
        cal = okE & (ratio > min_E_F_inlier_ratio) & (nE >= min_num_inliers)
    n_best = torch.where(cal, nE, nF)
    live = cal | uncal
    planar = live & (nH.double() / n_best.double() > max_H_inlier_ratio)
    config = torch.full_like(nF, DEGENERATE)
    config = torch.where(uncal, torch.full_like(nF, UNCALIBRATED), config)
    config = torch.where(cal, torch.full_like(nF, CALIBRATED), config)
    config = torch.where(planar, torch.full_like(nF, PLANAR_OR_PANORAMIC), config)
    choice = torch.where(cal, torch.zeros_like(nF), torch.ones_like(nF))
    choice = torch.where(planar & (nH > n_best), torch.full_like(nF, 2), choice)
    choice = torch.where(live, choice, torch.full_like(nF, -1))
    return config.to(torch.int32), choice


def two_view_geometry(uv0, uv1, intr0=None, intr1=None, pair_start=None, min_num_inliers=15, min_E_F_inlier_ratio=0.95,
                      max_H_inlier_ratio=0.8, **ransac):
    """COLMAP's two-view geometry verdict of P view pairs: ONE `fundamental_matrix` call, ONE `homography` call and, when
    intr0 / intr1 are given, ONE `relative_pose` call over all pairs, then a few integer comparisons per pair on the device
    (`two_view_config`; no host read).  uv0 / uv1 / pair_start / intrinsics as `relative_pose`; **ransac (max_error_px,
    confidence, min_inlier_ratio, min_num_trials, max_num_trials, seed) goes to all three estimators, default COLMAP's two-view
    options (max_error_px 4, confidence 0.999, min_inlier_ratio 0.25, trials 100 - 10 000).

    The rules are COLMAP's EstimateCalibrated / EstimateUncalibrated, with nE, nF, nH the inlier counts:
      CALIBRATED           E succeeded, nE / nF > min_E_F_inlier_ratio and nE >= min_num_inliers (n_best = nE, E's inliers);
      UNCALIBRATED         otherwise, F succeeded and nF >= min_num_inliers (n_best = nF, F's inliers);
      DEGENERATE           otherwise (all-false inliers);
      PLANAR_OR_PANORAMIC  a non-degenerate pair with nH / n_best > max_H_inlier_ratio; it takes H's inliers when nH > n_best.
    -> dict(config int32 [P] (the module constants DEGENERATE = 1, CALIBRATED = 2, UNCALIBRATED = 3, PLANAR_OR_PANORAMIC = 6,
    COLMAP's values), F, H, E [P,3,3] (E None without intrinsics), inliers bool [n] of the chosen model, num_inliers int32 [P],
    pair_start)"""
    if (intr0 is None) != (intr1 is None):
        raise ValueError("ls2fm.pose.two_view_geometry: intr0 and intr1 go together (both or neither)")
    unknown = set(ransac) - {"max_error_px", "confidence", "min_inlier_ratio", "min_num_trials", "max_num_trials", "seed"}
    if unknown:
        raise TypeError(f"ls2fm.pose.two_view_geometry: unexpected options {sorted(unknown)}")
    uv0, uv1, ps = _ragged_pairs(uv0, uv1, pair_start)
    opt = dict(max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.25, min_num_trials=100, max_num_trials=10000, seed=0)
    opt.update(ransac)
    f = fundamental_matrix(uv0, uv1, ps, **opt)
    h = homography(uv0, uv1, ps, **opt)
    e = relative_pose(uv0, uv1, intr0, intr1, ps, **opt) if intr0 is not None else None
    config, choice = two_view_config(e["num_inliers"] if e else None, e["success"] if e else None, f["num_inliers"], f["success"],
                                     h["num_inliers"], min_num_inliers, min_E_F_inlier_ratio, max_H_inlier_ratio)
    P = ps.numel() - 1
    # the pair of each correspondence, then its chosen model's mask
    pair_of = torch.repeat_interleave(torch.arange(P, device=uv0.device), (ps[1:] - ps[:-1]).to(torch.int64), output_size=uv0.shape[0])
    pick = choice[pair_of]
    inl = (pick == 1) & f["inliers"] | (pick == 2) & h["inliers"]
    if e:
        inl = inl | (pick == 0) & e["inliers"]
    return dict(config=config, F=f["F"], H=h["H"], E=e["E"] if e else None, inliers=inl,
                num_inliers=torch.zeros(P, dtype=torch.int32, device=uv0.device).index_add_(0, pair_of, inl.to(torch.int32)), pair_start=ps)
