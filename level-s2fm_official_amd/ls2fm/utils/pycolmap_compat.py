"""The subset of pycolmap the reference's registration uses, on the device (ls2fm.pose), numpy in and out.

pipelines/Registration.py and Registration_Trad.py run after one edit:
    import pycolmap   ->   from ls2fm.utils import pycolmap_compat as pycolmap

Camera (SIMPLE_PINHOLE, PINHOLE), absolute_pose_estimation, pose_refinement and qvec_to_rotmat follow pycolmap 0.3.0's names,
arguments, defaults and result keys as we read them (pycolmap is not available to confirm them).  absolute_pose_estimation
refines the pose on its inliers before it returns, as we read 0.3.0 to do.  There is no CPU fallback: without a GPU every
estimation call raises RuntimeError.

essential_matrix_estimation (Initializer's two-view initialisation, pipelines/Initialization.py:86-95 and
Initialization_Trad.py:81-85) runs ls2fm.pose.relative_pose.  It takes SIMPLE_PINHOLE cameras only -- the only model any
reference driver builds for this call -- and raises NotImplementedError for any other model, before any device or shape check;
ls2fm.pose.relative_pose itself takes general (fx, fy, cx, cy).  Its defaults (max_error_px 4, min_inlier_ratio 0.01, trials
1000 - 100 000, confidence 0.999) are our reading of pycolmap 0.3.0, unconfirmed as the rest.

fundamental_matrix_estimation and homography_matrix_estimation (no camera: pixels in) run ls2fm.pose.fundamental_matrix and
ls2fm.pose.homography with the same RANSAC defaults; F has x2h^T F x1h = 0 and H has x2h ~ H x1h for points2D1 -> points2D2.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import pose as _pose

_MODELS = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4}


class Camera:
    """pycolmap.Camera(model=, width=, height=, params=) for the two pinhole models"""

    def __init__(self, model="SIMPLE_PINHOLE", width=0, height=0, params=()):
        model = str(model)
        if model not in _MODELS:
            raise NotImplementedError(f"pycolmap_compat.Camera: model {model!r} (only SIMPLE_PINHOLE and PINHOLE are supported)")
        params = np.array([float(v) for v in np.asarray(params, dtype=object).reshape(-1)], dtype=np.float64)  # tensors too
        if params.size != _MODELS[model]:
            raise ValueError(f"pycolmap_compat.Camera: {model} takes {_MODELS[model]} parameters, got {params.size}")
        self.model_name = model
        self.width, self.height = int(width), int(height)
        self.params = params

    @property
    def intrinsics(self):
        """(fx, fy, cx, cy)"""
        p = self.params
        if self.model_name == "SIMPLE_PINHOLE":
            return np.array([p[0], p[0], p[1], p[2]])
        return p.copy()

    def __repr__(self):
        return f"Camera(model={self.model_name}, width={self.width}, height={self.height}, params={self.params.tolist()})"


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("pycolmap_compat: the pose estimation runs on the GPU (ls2fm.pose) and there is no CPU fallback; "
                           "no device is available")
    return torch.device("cuda", torch.cuda.current_device())


def _inputs(points2D, points3D, camera):
    if not isinstance(camera, Camera):
        raise TypeError("pycolmap_compat: camera must be a pycolmap_compat.Camera")
    p2 = np.asarray(points2D, dtype=np.float64)
    p3 = np.asarray(points3D, dtype=np.float64)
    if p2.ndim != 2 or p2.shape[1] != 2:
        raise ValueError(f"pycolmap_compat: points2D must be [n, 2], got {p2.shape}")
    if p3.ndim != 2 or p3.shape[1] != 3:
        raise ValueError(f"pycolmap_compat: points3D must be [n, 3], got {p3.shape}")
    if p2.shape[0] != p3.shape[0]:
        raise ValueError(f"pycolmap_compat: {p2.shape[0]} points2D against {p3.shape[0]} points3D")
    dev = _device()
    return (torch.from_numpy(np.ascontiguousarray(p2)).to(dev), torch.from_numpy(np.ascontiguousarray(p3)).to(dev),
            torch.from_numpy(camera.intrinsics).to(dev))


def absolute_pose_estimation(points2D, points3D, camera, max_error_px=12.0, min_inlier_ratio=0.01, min_num_trials=1000,
                             max_num_trials=100000, confidence=0.9999, seed=0):
    """-> {success, qvec, tvec, num_inliers, inliers (numpy bool [n])}; {success: False} on failure"""
    uv, xyz, intr = _inputs(points2D, points3D, camera)
    r = _pose.absolute_pose(uv, xyz, intr, max_error_px=max_error_px, confidence=confidence, min_inlier_ratio=min_inlier_ratio,
                            min_num_trials=min_num_trials, max_num_trials=max_num_trials, seed=seed, refine=True)
    if not bool(r["success"][0]):
        return {"success": False}
    P = r["poses"][0].cpu().numpy()
    return {"success": True, "qvec": _pose.rotmat_to_qvec(P[:, :3]), "tvec": P[:, 3].copy(),
            "num_inliers": int(r["num_inliers"][0]), "inliers": r["inliers"].cpu().numpy()}


def pose_refinement(tvec, qvec, points2D, points3D, inlier_mask, camera):
    """-> {success, qvec, tvec}: Cauchy-loss Levenberg-Marquardt on the inliers (loss scale 1 px, 100 iterations)"""
    uv, xyz, intr = _inputs(points2D, points3D, camera)
    mask = np.asarray(inlier_mask, dtype=bool).reshape(-1)
    if mask.size != uv.shape[0]:
        raise ValueError(f"pycolmap_compat.pose_refinement: inlier_mask of {mask.size} for {uv.shape[0]} points")
    P = np.concatenate([qvec_to_rotmat(qvec), np.asarray(tvec, dtype=np.float64).reshape(3, 1)], axis=1)
    out = _pose.refine_pose(uv, xyz, intr, torch.from_numpy(P).to(uv.device), torch.from_numpy(mask).to(uv.device))
    R = out[0].cpu().numpy()
    return {"success": bool(mask.sum() >= 3), "qvec": _pose.rotmat_to_qvec(R[:, :3]), "tvec": R[:, 3].copy()}


def qvec_to_rotmat(qvec):
    return _pose.qvec_to_rotmat(qvec)


def rotmat_to_qvec(R):
    return _pose.rotmat_to_qvec(R)


def essential_matrix_estimation(points2D1, points2D2, camera1, camera2, max_error_px=4.0, min_inlier_ratio=0.01,
                                min_num_trials=1000, max_num_trials=100000, confidence=0.999, seed=0):
    """-> {success, E, qvec, tvec, num_inliers, inliers (numpy bool [n])}; {success: False} on failure.  qvec / tvec map camera 1
    to camera 2 (X2 = R X1 + t, |t| = 1)"""
    for cam in (camera1, camera2):
        if not isinstance(cam, Camera):
            raise TypeError("pycolmap_compat: camera must be a pycolmap_compat.Camera")
        if cam.model_name != "SIMPLE_PINHOLE":
            raise NotImplementedError(f"pycolmap_compat.essential_matrix_estimation: camera model {cam.model_name!r} "
                                      "(only SIMPLE_PINHOLE is supported)")
    p0 = np.asarray(points2D1, dtype=np.float64)
    p1 = np.asarray(points2D2, dtype=np.float64)
    for name, p in (("points2D1", p0), ("points2D2", p1)):
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"pycolmap_compat: {name} must be [n, 2], got {p.shape}")
    if p0.shape[0] != p1.shape[0]:
        raise ValueError(f"pycolmap_compat: {p0.shape[0]} points2D1 against {p1.shape[0]} points2D2")
    dev = _device()
    r = _pose.relative_pose(torch.from_numpy(np.ascontiguousarray(p0)).to(dev), torch.from_numpy(np.ascontiguousarray(p1)).to(dev),
                            torch.from_numpy(camera1.intrinsics).to(dev), torch.from_numpy(camera2.intrinsics).to(dev),
                            max_error_px=max_error_px, confidence=confidence, min_inlier_ratio=min_inlier_ratio,
                            min_num_trials=min_num_trials, max_num_trials=max_num_trials, seed=seed)
    if not bool(r["success"][0]):
        return {"success": False}
    P = r["poses"][0].cpu().numpy()
    return {"success": True, "E": r["E"][0].cpu().numpy(), "qvec": _pose.rotmat_to_qvec(P[:, :3]), "tvec": P[:, 3].copy(),
            "num_inliers": int(r["num_inliers"][0]), "inliers": r["inliers"].cpu().numpy()}


def _pixel_pairs(points2D1, points2D2):
    p0 = np.asarray(points2D1, dtype=np.float64)
    p1 = np.asarray(points2D2, dtype=np.float64)
    for name, p in (("points2D1", p0), ("points2D2", p1)):
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"pycolmap_compat: {name} must be [n, 2], got {p.shape}")
    if p0.shape[0] != p1.shape[0]:
        raise ValueError(f"pycolmap_compat: {p0.shape[0]} points2D1 against {p1.shape[0]} points2D2")
    dev = _device()
    return torch.from_numpy(np.ascontiguousarray(p0)).to(dev), torch.from_numpy(np.ascontiguousarray(p1)).to(dev)


def _two_view_answer(r, key):
    if not bool(r["success"][0]):
        return {"success": False}
    return {"success": True, key: r[key][0].cpu().numpy(), "num_inliers": int(r["num_inliers"][0]),
            "inliers": r["inliers"].cpu().numpy()}


def fundamental_matrix_estimation(points2D1, points2D2, max_error_px=4.0, min_inlier_ratio=0.01, min_num_trials=1000,
                                  max_num_trials=100000, confidence=0.999, seed=0):
    """-> {success, F, num_inliers, inliers (numpy bool [n])}; {success: False} on failure"""
    a, b = _pixel_pairs(points2D1, points2D2)
    return _two_view_answer(_pose.fundamental_matrix(a, b, max_error_px=max_error_px, confidence=confidence,
                                                     min_inlier_ratio=min_inlier_ratio, min_num_trials=min_num_trials,
                                                     max_num_trials=max_num_trials, seed=seed), "F")


def homography_matrix_estimation(points2D1, points2D2, max_error_px=4.0, min_inlier_ratio=0.01, min_num_trials=1000,
                                 max_num_trials=100000, confidence=0.999, seed=0):
    """-> {success, H, num_inliers, inliers (numpy bool [n])}; {success: False} on failure"""
    a, b = _pixel_pairs(points2D1, points2D2)
    return _two_view_answer(_pose.homography(a, b, max_error_px=max_error_px, confidence=confidence,
                                             min_inlier_ratio=min_inlier_ratio, min_num_trials=min_num_trials,
                                             max_num_trials=max_num_trials, seed=seed), "H")
