"""The one cv2 function the reference's _Trad drivers use for geometry, on the device (ls2fm.pose.triangulate), numpy in and out.

pipelines/Initialization_Trad.py:97 and Registration_Trad.py:258 run after one edit:
    cv2.triangulatePoints(...)   ->   from ls2fm.utils import cv2_compat as cv2  (or cv2_compat.triangulatePoints)

triangulatePoints builds cv2's 4 x 4 DLT system per point and returns its right singular vector of the smallest singular value,
unit norm with w >= 0 (cv2's result up to its arbitrary sign), as float64.  Image I/O and everything else of cv2 are not
provided.  There is no CPU fallback: without a GPU the call raises RuntimeError.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import pose as _pose


def triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2):  # noqa: N802,N803  (cv2's names)
    """projMatr1 / projMatr2 [3,4], projPoints1 / projPoints2 [2,n] pixels -> homogeneous points [4,n] (float64)"""
    P0 = np.asarray(projMatr1, dtype=np.float64)
    P1 = np.asarray(projMatr2, dtype=np.float64)
    if P0.shape != (3, 4) or P1.shape != (3, 4):
        raise ValueError(f"cv2_compat.triangulatePoints: projection matrices must be [3, 4], got {P0.shape} and {P1.shape}")
    p0 = np.asarray(projPoints1, dtype=np.float64)
    p1 = np.asarray(projPoints2, dtype=np.float64)
    if p0.ndim != 2 or p0.shape[0] != 2 or p1.shape != p0.shape:
        raise ValueError(f"cv2_compat.triangulatePoints: points must be [2, n] each, got {p0.shape} and {p1.shape}")
    if not torch.cuda.is_available():
        raise RuntimeError("cv2_compat: triangulatePoints runs on the GPU (ls2fm.pose) and there is no CPU fallback; "
                           "no device is available")
    dev = torch.device("cuda", torch.cuda.current_device())
    if p0.shape[1] == 0:
        return np.zeros((4, 0))
    X = _pose.triangulate(torch.from_numpy(P0).to(dev), torch.from_numpy(P1).to(dev),
                          torch.from_numpy(np.ascontiguousarray(p0.T)).to(dev), torch.from_numpy(np.ascontiguousarray(p1.T)).to(dev))
    return X.cpu().numpy().T.copy()
