"""Absolute pose on the device: what Registration.PnP asks of pycolmap (pipelines/Registration.py:94-109 of the reference).

`absolute_pose` runs LO-RANSAC (Lambda Twist P3P, Gauss-Newton local optimisation, Cauchy-loss Levenberg-Marquardt refinement)
for one or MANY views in one call of ls2fm_absolute_pose (csrc/absolute_pose.hip) -- the next-best-view search of
LevelS2fM.train (pipelines/LevelS2fM.py:247-281) forms every candidate view's pnp score from one call instead of one host round
trip per view.  `refine_pose` is pose_refinement alone (ls2fm_pose_refine), `p3p` the minimal solver alone.  Every rule is stated
in include/ls2fm.h; tests/pose_restate.py repeats them in numpy.

Poses are world-to-camera [3,4] = [R | t], fp64; intrinsics per view (fx, fy, cx, cy).  The defaults are pycolmap 0.3.0's
absolute_pose_estimation defaults as we read them.  There is no CPU path: CPU tensors, a missing device or a missing library raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


def _device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ls2fm.pose: runs on MI355X only (got a CPU tensor); there is no CPU fallback")


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
    if isinstance(uv, (list, tuple)):
        if not isinstance(xyz, (list, tuple)) or len(xyz) != len(uv) or len(uv) == 0:
            raise ValueError("ls2fm.pose: uv and xyz lists must have the same non-zero length")
        if view_start is not None:
            raise ValueError("ls2fm.pose: view_start is implied by lists of per-view tensors")
        dev = torch.as_tensor(uv[0]).device
        us = [torch.as_tensor(u).reshape(-1, 2) for u in uv]
        xs = [torch.as_tensor(x).reshape(-1, 3) for x in xyz]
        for u, x in zip(us, xs):
            if u.shape[0] != x.shape[0]:
                raise ValueError(f"ls2fm.pose: {u.shape[0]} key points against {x.shape[0]} 3-D points")
        counts = [u.shape[0] for u in us]
        vs = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)
        return (_f64(torch.cat(us).to(dev), (2,), "uv"), _f64(torch.cat(xs).to(dev), (3,), "xyz"), vs)
    uv = _f64(uv, (2,), "uv")
    xyz = _f64(xyz, (3,), "xyz")
    if uv.shape[0] != xyz.shape[0]:
        raise ValueError(f"ls2fm.pose: {uv.shape[0]} key points against {xyz.shape[0]} 3-D points")
    if view_start is None:
        view_start = torch.tensor([0, uv.shape[0]], dtype=torch.int32, device=uv.device)
    view_start = torch.as_tensor(view_start, device=uv.device).to(torch.int32).contiguous()
    if view_start.dim() != 1 or view_start.numel() < 2:
        raise ValueError("ls2fm.pose: view_start must be [V + 1]")
    if not torch.cuda.is_current_stream_capturing():
        # the kernels index uv / xyz / the mask through view_start: it must cover exactly [0, n), in order
        h = view_start.cpu()
        if int(h[0]) != 0 or int(h[-1]) != uv.shape[0] or bool((h[1:] < h[:-1]).any()):
            raise ValueError(f"ls2fm.pose: view_start must rise from 0 to the {uv.shape[0]} correspondences, "
                             f"got {h[0].item()} .. {h[-1].item()}")
    return uv, xyz, view_start


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
    lib = _lib.load()
    opts = _lib.PoseRansacOpts(float(max_error_px), float(confidence), float(min_inlier_ratio), int(min_num_trials),
                               int(max_num_trials), int(seed) & ((1 << 64) - 1), 1 if refine else 0)
    ws_bytes = lib.ls2fm_absolute_pose_workspace_bytes(V, uv.shape[0])
    if ws_bytes < 0:
        check(int(ws_bytes), "ls2fm_absolute_pose_workspace_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    poses = torch.empty(V, 3, 4, dtype=torch.float64, device=dev)
    inl = torch.empty(uv.shape[0], dtype=torch.uint8, device=dev)
    num, trials, best, succ = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(4))
    check(lib.ls2fm_absolute_pose(ptr(uv), ptr(xyz), ptr(vs), V, ptr(intr), ctypes.byref(opts), ptr(poses), ptr(inl), ptr(num),
                                  ptr(trials), ptr(best), ptr(succ), ptr(ws), stream_ptr()), "ls2fm_absolute_pose")
    return dict(poses=poses, inliers=inl.view(torch.bool), num_inliers=num, trials=trials, best_trial=best,
                success=succ.bool(), view_start=vs)


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
