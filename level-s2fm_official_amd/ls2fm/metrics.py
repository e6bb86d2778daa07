"""Reconstruction metrics on the device: how good a result is against ground truth.  The paper reports camera error after a
similarity alignment (rotation in degrees, ATE) and the DTU Chamfer distance of the mesh (accuracy, completeness, their mean); the
reference ships neither, and the usual CPU KD-tree evaluation of two DTU-sized clouds takes minutes per scan.

  PointGrid / nearest_neighbors   exact nearest neighbours over a uniform grid: ls2fm/point_grid.py, re-exported here
  normal_consistency              mean |n . n'| over the nearest-neighbour pairs, both directions
  voxel_downsample                one point per voxel, the lowest index
  chamfer / evaluate_mesh         accuracy, completeness, overall, precision / recall / F-score
  align_sim3 / pose_errors        Umeyama's similarity alignment, rotation and centre errors, ATE
  icp / IcpResult                 registration of a cloud to ground truth over the grid (ls2fm_icp_run, csrc/icp.hip); evaluate_mesh
                                  takes it (init=, icp=) for a mesh in another gauge than the ground truth

ls2fm/point_grid.py states the distance rule.  There is no CPU path for the grid: CPU tensors, a missing device or a missing library raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .point_grid import (AUTO_CELL_RULE, KNN_MAX_K, PointGrid, auto_cell_size, cell_dims, knn_k, nearest_neighbors,  # noqa: F401
                         nearest_neighbors_bruteforce, points3, require_device, squared_cutoff)
_points, _max_d2, _knn_k, _dims = points3, squared_cutoff, knn_k, cell_dims          # the names they had while they lived here


_VOXEL_BITS = 21


def voxel_downsample(points, voxel):
    """int64 indices, ascending, of the points kept when every voxel of side `voxel` keeps its lowest-index point.  Voxel
    coordinates are floor(double(p) / voxel), each stored in 21 bits (so inside [-2^20, 2^20): ValueError beyond, and for a NaN or
    infinite point) of one int64 key; torch ops on the points' device, one host read for that check.
    A stated deviation: the usual DTU evaluation script thins a cloud by a sequential greedy radius rule (a point is dropped when
    a kept point lies within the radius), which depends on the visiting order and keeps points up to sqrt(3) times sparser or denser
    than this; one point per voxel is order-free up to the choice of the lowest index and runs as one sort."""
    p = points3(points, "points")
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError(f"ls2fm.metrics.voxel_downsample: voxel {voxel} must be positive and finite")
    if p.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=p.device)
    v = torch.floor(p.to(torch.float64) / float(voxel))
    half = float(1 << (_VOXEL_BITS - 1))
    if not bool((torch.isfinite(v) & (v >= -half) & (v < half)).all()):
        raise ValueError(f"ls2fm.metrics.voxel_downsample: a voxel coordinate does not fit in {_VOXEL_BITS} bits "
                         f"(|p / voxel| up to 2^{_VOXEL_BITS - 1}), or a point is not finite")
    c = v.to(torch.int64) + (1 << (_VOXEL_BITS - 1))
    key = (c[:, 0] << (2 * _VOXEL_BITS)) | (c[:, 1] << _VOXEL_BITS) | c[:, 2]
    key, order = torch.sort(key, stable=True)                     # stable: the first of a run of equal keys is its lowest index
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    return torch.sort(order[first]).values


def _masked(x, mask, name):
    x = points3(x, name)
    if mask is None:
        return x
    mask = torch.as_tensor(mask, device=x.device)
    if mask.dtype != torch.bool or mask.shape != (x.shape[0],):
        raise ValueError(f"ls2fm.metrics: {name}_mask must be bool [{x.shape[0]}], got {mask.dtype} {tuple(mask.shape)}")
    return x[mask]


def _one_side(q, ref, max_dist, thresholds, brute_force):
    """fp64 [2 + len(thresholds)] on the device: the number of queries with a neighbour, the mean of their distances, and per
    threshold the fraction of ALL queries whose neighbour passes it"""
    if brute_force:
        idx, d2 = nearest_neighbors_bruteforce(q, ref, max_dist)
    else:
        idx, d2 = nearest_neighbors(q, ref, max_dist)
    has = idx >= 0
    n = has.sum().to(torch.float64)
    dist = torch.sqrt(d2.to(torch.float64))
    mean = torch.where(has, dist, torch.zeros_like(dist)).sum() / n                    # 0 / 0 = NaN for an empty side
    m = torch.tensor(float(q.shape[0]), dtype=torch.float64, device=q.device)
    rates = [(has & (d2 <= float(np.float32(t) * np.float32(t)))).sum().to(torch.float64) / m for t in thresholds]
    return torch.stack([n, mean] + rates)


def chamfer(pred, gt, max_dist, thresholds=(), pred_mask=None, gt_mask=None, brute_force=False):
    """The DTU-style Chamfer figures of a predicted cloud against ground truth (both float32 [., 3], on the device unless
    brute_force): a dict of
      accuracy        mean distance from the points of `pred` to their nearest point of `gt`, over those with one inside max_dist
      completeness    the same from `gt` to `pred`;  overall: the mean of the two
      n_accuracy, n_completeness   how many points had such a neighbour (ints)
      thresholds, precision, recall, fscore   per threshold tau (tuples in the order given): the fraction of pred (of gt) whose
                      neighbour has d2 <= float32(tau)^2, and 2 p r / (p + r) (0 when both are 0)
    Distances are sqrt(double(d2)) of the fp32 d2 of the distance rule, the means are fp64 sums on the device, and the dict costs
    one host read.  pred_mask / gt_mask (bool) select the points that take part: visibility volumes and ground-plane filters
    are the dataset's and stay with the caller.  An empty side gives NaN for its mean (and its rates) and 0 for its count.
    brute_force=True takes nearest_neighbors_bruteforce instead of the grid (any device; for checks and small clouds)."""
    pred, gt = _masked(pred, pred_mask, "pred"), _masked(gt, gt_mask, "gt")
    thresholds = tuple(float(t) for t in thresholds)
    if not brute_force:
        require_device(pred, gt)
    if pred.device != gt.device:
        raise ValueError(f"ls2fm.metrics.chamfer: pred on {pred.device}, gt on {gt.device}")
    acc = _one_side(pred, gt, max_dist, thresholds, brute_force)
    com = _one_side(gt, pred, max_dist, thresholds, brute_force)
    a, c = torch.stack([acc, com]).cpu().tolist()                                     # the one host read
    return _chamfer_dict(a, c, thresholds)


def _chamfer_dict(a, c, thresholds):
    prec, rec = tuple(a[2:]), tuple(c[2:])
    f = tuple((2.0 * p * r / (p + r)) if p + r > 0 else (0.0 if p + r == 0 else float("nan")) for p, r in zip(prec, rec))
    return dict(accuracy=a[1], completeness=c[1], overall=0.5 * (a[1] + c[1]), n_accuracy=int(a[0]), n_completeness=int(c[0]),
                thresholds=thresholds, precision=prec, recall=rec, fscore=f)


def _consistency_side(q, qn, ref, refn, max_dist):
    """fp64 [2] on the device: the number of queries with a reference inside max_dist and the mean of |n_q . n_ref| over them"""
    idx, _ = nearest_neighbors(q, ref, max_dist)
    has = idx >= 0
    a, b = qn.to(torch.float64), refn.to(torch.float64)[idx.clamp(min=0).long()]
    dot = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).abs()
    n = has.sum().to(torch.float64)
    return torch.stack([n, torch.where(has, dot, torch.zeros_like(dot)).sum() / n])


def normal_consistency(pred_points, pred_normals, gt_points, gt_normals, max_dist):
    """The normal consistency the neural-surface papers report beside Chamfer (MonoSDF, NeuRIS), in both directions: a dict of
      accuracy        the fp64 mean of |n_pred . n_gt| over the points of `pred` paired with their nearest point of `gt` inside max_dist
      completeness    the same from `gt` to `pred`;  overall: the mean of the two
      n_accuracy, n_completeness   the numbers of pairs (ints)
    (and, empty, the threshold entries of `chamfer`'s dict).  The pairs are PointGrid.query's; the absolute value is there because
    estimated normals (ls2fm.cloud.estimate_normals) are unoriented.  Normals are taken as given, not normalised.  A side without
    a pair gives NaN.  Torch ops on two queries, one host read."""
    pred, gt = points3(pred_points, "pred_points"), points3(gt_points, "gt_points")
    pn, gn = points3(pred_normals, "pred_normals"), points3(gt_normals, "gt_normals")
    require_device(pred, gt, pn, gn)
    if pn.shape[0] != pred.shape[0] or gn.shape[0] != gt.shape[0]:
        raise ValueError(f"ls2fm.metrics.normal_consistency: {pn.shape[0]} normals for {pred.shape[0]} points, {gn.shape[0]} for {gt.shape[0]}")
    if len({t.device for t in (pred, gt, pn, gn)}) != 1:
        raise ValueError("ls2fm.metrics.normal_consistency: the four tensors are not on one device")
    a = _consistency_side(pred, pn, gt, gn, max_dist) if gt.shape[0] else pred.new_tensor([0.0, float("nan")], dtype=torch.float64)
    c = _consistency_side(gt, gn, pred, pn, max_dist) if pred.shape[0] else pred.new_tensor([0.0, float("nan")], dtype=torch.float64)
    a, c = torch.stack([a, c]).cpu().tolist()                                         # the one host read
    return _chamfer_dict(a, c, ())


def evaluate_mesh(verts, faces, gt_points, max_dist, density, thresholds=(), generator=None, brute_force=False, return_points=False,
                  init=None, icp=None):
    """The Chamfer figures of a mesh against a ground-truth cloud: ceil(area / density^2) points of ls2fm.mesh.sample_surface
    (uniforms from `generator`), both clouds thinned by voxel_downsample at `density`, then `chamfer`.
    -> the dict of chamfer plus n_pred and n_gt, the sizes of the two clouds compared (and, with return_points, pred_points and
    gt_points themselves).  One host read for the area, one per thinning, one for the dict.  A dataset's masks need the sampled
    points: such a caller runs these steps itself and passes the masks to `chamfer`.
    init, icp: for a mesh in another gauge than the ground truth (a reconstruction from estimated poses).  With both None nothing
    changes.  Otherwise the vertices are first moved by init = (s, R, t) as align_sim3 returns it (None: the identity), x -> s R x +
    t in fp64, rounded to fp32; the thinned sample is registered to the thinned ground truth by `icp` (the function below) with the
    options of the dict `icp` (None: its defaults; max_dist defaults to this call's max_dist, brute_force to this call's), and
    `chamfer` runs on the registered sample.  The dict gains s, R, t -- the whole transform from the mesh's frame, ICP after init,
    fp64 device tensors -- and icp_rmse, icp_n_pairs, icp_iterations, icp_status (one more host read)."""
    from . import mesh
    verts, gt = points3(verts, "verts"), points3(gt_points, "gt_points")
    require_device(verts, faces, gt)
    if not (np.isfinite(density) and density > 0):
        raise ValueError(f"ls2fm.metrics.evaluate_mesh: density {density} must be positive and finite")
    register = init is not None or icp is not None
    if register:
        s0, R0, t0 = _sim3(init, verts.device)
        verts = (s0 * (verts.to(torch.float64) @ R0.t()) + t0).float()
    area = float(mesh._face_areas64(verts, faces).sum())
    count = int(math.ceil(area / (float(density) * float(density))))
    if count >= 1 << 31:
        raise ValueError(f"ls2fm.metrics.evaluate_mesh: {count} samples (area {area} at density {density}), 2^31 or more")
    pts = mesh.sample_surface(verts, faces, count, generator=generator) if count else verts.new_zeros((0, 3), dtype=torch.float32)
    pts = pts[voxel_downsample(pts, density)]
    gt = gt.float()
    gt = gt[voxel_downsample(gt, density)]
    if register:
        options = dict(max_dist=max_dist, brute_force=brute_force)
        options.update(icp or {})
        reg = _icp(pts, gt, **options)
        pts = reg.apply(pts).float()
    out = chamfer(pts, gt, max_dist, thresholds=thresholds, brute_force=brute_force)
    out.update(n_pred=int(pts.shape[0]), n_gt=int(gt.shape[0]))
    if register:
        out.update(s=reg.s * s0, R=reg.R @ R0, t=reg.s * (reg.R @ t0) + reg.t, icp_rmse=reg.rmse, icp_n_pairs=reg.n_pairs,
                   icp_iterations=reg.iterations, icp_status=reg.status)
    if return_points:
        out.update(pred_points=pts, gt_points=gt)
    return out


# ------------------------------------------------------------------------------------------------------------- camera poses
def align_sim3(src, dst, with_scale=True):
    """Umeyama's closed form: the similarity (s, R, t) that minimises sum |dst_i - (s R src_i + t)|^2 over [n, 3] point sets, in
    fp64.  The means, the 3 x 3 covariance and the variance are torch ops on the inputs' device; the 3 x 3 SVD runs on the host
    (no dependence on a device solver); a reflection is corrected through the sign of det(U) det(V).  with_scale=False fixes s = 1.
    -> (s float, R fp64 [3, 3], t fp64 [3]; tensors on src's device)."""
    src, dst = points3(src, "src"), points3(dst, "dst")
    if src.shape != dst.shape or src.shape[0] < 1:
        raise ValueError(f"ls2fm.metrics.align_sim3: {tuple(src.shape)} against {tuple(dst.shape)}")
    dev = src.device
    a, b = src.to(torch.float64), dst.to(device=dev, dtype=torch.float64)
    n = a.shape[0]
    mu_a, mu_b = a.sum(dim=0) / n, b.sum(dim=0) / n
    xa, xb = a - mu_a, b - mu_b
    cov = (xb.t() @ xa) / n
    var_a = (xa * xa).sum() / n
    host = torch.cat([cov.reshape(-1), var_a.reshape(1), mu_a, mu_b]).cpu().numpy()      # the one host read
    cov_h, var_h, mu_ah, mu_bh = host[:9].reshape(3, 3), host[9], host[10:13], host[13:16]
    U, D, Vt = np.linalg.svd(cov_h)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = (U * S) @ Vt
    s = float((D * S).sum() / var_h) if with_scale and var_h > 0 else 1.0
    t = mu_bh - s * (R @ mu_ah)
    return s, torch.as_tensor(R, dtype=torch.float64, device=dev), torch.as_tensor(t, dtype=torch.float64, device=dev)


def _rt(poses, name):
    p = torch.as_tensor(poses)
    if p.dim() != 3 or tuple(p.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"ls2fm.metrics.pose_errors: {name} must be [V, 3, 4] or [V, 4, 4], got {tuple(p.shape)}")
    p = p.to(torch.float64)
    return p[:, :3, :3], p[:, :3, 3]


def pose_errors(poses_est, poses_gt, align=True, with_scale=True, registered=None):
    """Camera errors of estimated poses against ground truth, both [R | t] world-to-camera ([V, 3, 4] or [V, 4, 4]; the mapper's
    convention), in fp64.  The camera centres C = -R^T t of the estimate are aligned to the ground truth's by align_sim3 (align=
    False compares them as they are), X_gt = s A X_est + a, and the estimated orientations are taken along: R_est A^T.
    registered: bool [V] (read on the host) or None; views that are not registered are left out and counted.  -> dict of
      rot_err_deg [V], centre_err [V]   per view (fp64 host tensors; NaN for a view left out): the angle of R_est A^T R_gt^T, taken as
                      atan2(|axis part|, (trace - 1) / 2) so that it is accurate near 0, and |s A C_est + a - C_gt|
      ate_rmse        sqrt(mean centre_err^2), the absolute trajectory error
      rot_err_mean_deg, rot_err_max_deg, centre_err_mean, centre_err_max, scale, n_views (compared), n_unregistered
    An alignment needs three views; fewer raise.  One host read for the alignment's SVD, one for the dict."""
    Re, te = _rt(poses_est, "poses_est")
    Rg, tg = _rt(poses_gt, "poses_gt")
    dev = Re.device
    Rg, tg = Rg.to(dev), tg.to(dev)
    V = Re.shape[0]
    if Rg.shape[0] != V:
        raise ValueError(f"ls2fm.metrics.pose_errors: {V} estimated poses against {Rg.shape[0]}")
    reg = torch.ones(V, dtype=torch.bool) if registered is None else torch.as_tensor(registered).cpu()      # the mapper keeps it on the host
    if reg.dtype != torch.bool or reg.shape != (V,):
        raise ValueError(f"ls2fm.metrics.pose_errors: registered must be bool [{V}]")
    sel_host = torch.nonzero(reg).reshape(-1)
    sel = sel_host.to(dev)
    n = int(sel.numel())
    if n < (3 if align else 1):
        raise ValueError(f"ls2fm.metrics.pose_errors: {n} registered views; {'an alignment needs three' if align else 'none to compare'}")
    Re, te, Rg, tg = Re[sel], te[sel], Rg[sel], tg[sel]
    Ce = -(Re.transpose(1, 2) @ te[:, :, None])[:, :, 0]
    Cg = -(Rg.transpose(1, 2) @ tg[:, :, None])[:, :, 0]
    if align:
        s, A, a = align_sim3(Ce, Cg, with_scale=with_scale)
    else:
        s, A, a = 1.0, torch.eye(3, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
    centre = ((s * (Ce @ A.t()) + a) - Cg).norm(dim=1)
    D = (Re @ A.t()) @ Rg.transpose(1, 2)
    axis = torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], dim=1).norm(dim=1) / 2
    rot = torch.rad2deg(torch.atan2(axis, ((D[:, 0, 0] + D[:, 1, 1]) + D[:, 2, 2] - 1) / 2))
    nan = torch.full((V,), float("nan"), dtype=torch.float64, device=dev)
    out = torch.stack([nan.index_copy(0, sel, rot), nan.index_copy(0, sel, centre)]).cpu()          # the dict's host read
    r, c = out[0][sel_host], out[1][sel_host]
    return dict(rot_err_deg=out[0], centre_err=out[1], ate_rmse=float((c * c).mean().sqrt()),
                rot_err_mean_deg=float(r.mean()), rot_err_max_deg=float(r.max()), centre_err_mean=float(c.mean()),
                centre_err_max=float(c.max()), scale=float(s), n_views=n, n_unregistered=V - n)


# ------------------------------------------------------------------------------------------------------------------- ICP
ICP_RUNNING, ICP_CONVERGED, ICP_DEGENERATE = 0, 1, 2
ICP_MAX_ITERS = 65536                     # LS2FM_ICP_MAX_ITERS
ICP_TOL_ROT = 1e-9                        # the default tol_rot (radians; |lambda| too)
ICP_TOL_TRANS_REL = 1e-9                  # the default tol_trans, as a fraction of the diagonal of the fixed cloud's box
_S_COST, _S_PAIRS, _S_ITERS, _S_STATUS, _S_SIZE = 13, 14, 15, 16, 24


def _sim3(init, device):
    """(s fp64 0-dim, R fp64 [3, 3], t fp64 [3]) on `device` of an (s, R, t) as align_sim3 returns it; None: the identity"""
    if init is None:
        init = (1.0, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    s, R, t = init
    s = torch.as_tensor(s, dtype=torch.float64).to(device).reshape(())
    R = torch.as_tensor(R).to(device=device, dtype=torch.float64)
    t = torch.as_tensor(t).to(device=device, dtype=torch.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"ls2fm.metrics.icp: init must be (s, R [3, 3], t [3]), got R {tuple(R.shape)}, t {tuple(t.shape)}")
    return s, R, t


class IcpResult:
    """What `icp` returns.  s (0-dim), R [3, 3], t [3]: fp64 tensors on the clouds' device, views of `state` (fp64 [24], the layout
    of include/ls2fm.h; pass it back as icp(..., state=) to continue bit for bit).  rmse = sqrt(cost / n_pairs) and n_pairs come from
    a closing evaluation at the returned transform (the cost is the sum of squared residuals: distances point to point, distances
    along the normal point to plane; NaN without a pair); iterations and status (ICP_RUNNING: the iterations ran out,
    ICP_CONVERGED, ICP_DEGENERATE) from the state.  With read=False these four are None and `evaluation`, the fp64 [24] state of
    the closing evaluation (cost at 13, pair count at 14), holds them on the device.  pair_idx int32 [M] / pair_d2 float32 [M] (with
    return_pairs): each source point's reference at the returned transform, -1 / +inf without one."""

    def __init__(self, state, evaluation, pair_idx=None, pair_d2=None):
        self.state, self.evaluation, self.pair_idx, self.pair_d2 = state, evaluation, pair_idx, pair_d2
        self.s, self.R, self.t = state[0], state[1:10].view(3, 3), state[10:13]
        self.rmse = self.n_pairs = self.iterations = self.status = None

    def read(self):
        """the one host read: fills rmse, n_pairs, iterations, status"""
        cost, pairs, iterations, status = torch.cat([self.evaluation[_S_COST:_S_PAIRS + 1], self.state[_S_ITERS:_S_STATUS + 1]]).cpu().tolist()
        self.n_pairs, self.iterations, self.status = int(pairs), int(iterations), int(status)
        self.rmse = math.sqrt(cost / pairs) if pairs else float("nan")
        return self

    def apply(self, points):
        """s R p + t of points [n, 3] in fp64 (on the state's device)"""
        p = points3(points, "points").to(device=self.state.device, dtype=torch.float64)
        return self.s * (p @ self.R.t()) + self.t


def _icp_state(init, state, device):
    if state is not None:
        state = torch.as_tensor(state)
        if state.dtype != torch.float64 or state.shape != (_S_SIZE,):
            raise ValueError(f"ls2fm.metrics.icp: state must be float64 [{_S_SIZE}], got {state.dtype} {tuple(state.shape)}")
        return state.to(device).clone()
    s, R, t = _sim3(init, device)
    out = torch.zeros(_S_SIZE, dtype=torch.float64, device=device)
    out[0] = s
    out[1:10] = R.reshape(-1)
    out[10:13] = t
    return out


def _chol_solve(H, g):
    """H x = -g by the Cholesky order of the device's solve (lm_math::chol_solve), so that the torch form calls the same systems
    degenerate: None for a pivot <= 0 (a NaN included) or an x that is not finite"""
    m = len(g)
    L = [[0.0] * m for _ in range(m)]
    for j in range(m):
        d = float(H[j, j]) - sum(L[j][k] * L[j][k] for k in range(j))
        if not d > 0.0:
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, m):
            L[i][j] = (float(H[j, i]) - sum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    z, x = [0.0] * m, [0.0] * m
    for i in range(m):
        z[i] = (-float(g[i]) - sum(L[i][k] * z[k] for k in range(i))) / L[i][i]
    for i in range(m - 1, -1, -1):
        x[i] = (z[i] - sum(L[k][i] * x[k] for k in range(i + 1, m))) / L[i][i]
    x = np.array(x)
    return x if np.isfinite(x).all() else None


def _icp_torch_step(src64, ref, normals, state, neighbours, with_scale, tol_rot, tol_trans, solve):
    """one iteration of the rule as plain torch ops: the transform in the stated association, `neighbours` for the pairs, the
    normal equations as masked fp64 reductions; with `solve` the 7 x 7 system goes to the host, is solved there (_chol_solve) and
    the state updated.  -> (idx, d2)"""
    s, R, t = state[0], state[1:10].view(3, 3), state[10:13]
    x, y, z = src64[:, 0], src64[:, 1], src64[:, 2]
    p = torch.stack([s * ((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], dim=1).float()
    idx, d2 = neighbours(p)
    has = idx >= 0
    j = idx.clamp(min=0).long()
    w = has.to(torch.float64)
    p64 = torch.where(has[:, None], p.to(torch.float64), torch.zeros((), dtype=torch.float64, device=p.device))
    if ref.shape[0] == 0:                                          # no reference: nothing to gather, no pair
        ref, normals = ref.new_zeros((1, 3)), None if normals is None else normals.new_zeros((1, 3))
    d = (p64 - ref[j].to(torch.float64)) * w[:, None]
    px, py, pz = p64[:, 0], p64[:, 1], p64[:, 2]
    zero = torch.zeros_like(px)
    if normals is None:
        J = torch.stack([torch.stack([zero, pz, -py, w, zero, zero, px], dim=1), torch.stack([-pz, zero, px, zero, w, zero, py], dim=1),
                         torch.stack([py, -px, zero, zero, zero, w, pz], dim=1)], dim=1)
        r = d
    else:
        n = normals[j].to(torch.float64) * w[:, None]
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        J = torch.stack([py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz, (nx * px + ny * py) + nz * pz], dim=1)[:, None, :]
        r = ((nx * d[:, 0] + ny * d[:, 1]) + nz * d[:, 2])[:, None]
    # the Gram matrix of [J | r], 4096 rows at a time as one batched product (a single product over millions of rows runs as one
    # long dot product per entry): H, g and the cost are its blocks
    A = torch.cat([J.reshape(-1, 7), r.reshape(-1, 1)], dim=1)
    A = torch.nn.functional.pad(A, (0, 0, 0, -A.shape[0] % 4096)).view((A.shape[0] + 4095) // 4096, 4096, 8)
    G = torch.bmm(A.transpose(1, 2), A).sum(dim=0)
    H, g = G[:7, :7], G[:7, 7]
    state[_S_COST] = G[7, 7]
    state[_S_PAIRS] = w.sum()
    if not solve:
        return idx, d2
    host = torch.cat([H.reshape(-1), g, state[:_S_SIZE]]).cpu().numpy()                # the iteration's host read
    Hh, gh, st = host[:49].reshape(7, 7), host[49:56], host[56:].copy()
    m = 7 if with_scale else 6
    delta = None
    if st[_S_PAIRS] >= m:
        delta = _chol_solve(Hh[:m, :m], gh[:m])
    if delta is None:
        st[_S_STATUS] = ICP_DEGENERATE
    else:
        wv = delta[:3]
        th2 = float(wv @ wv)
        K = np.array([[0.0, -wv[2], wv[1]], [wv[2], 0.0, -wv[0]], [-wv[1], wv[0], 0.0]])
        th = math.sqrt(th2)
        E = np.eye(3) + K if th2 < 1e-30 else np.eye(3) + math.sin(th) / th * K + (1.0 - math.cos(th)) / th2 * (K @ K)
        lam = float(delta[6]) if with_scale else 0.0
        k = 1.0 + math.expm1(lam)
        st[0] = k * st[0]
        st[10:13] = k * (E @ st[10:13]) + delta[3:6]
        st[1:10] = (E @ st[1:10].reshape(3, 3)).reshape(-1)
        st[_S_ITERS] += 1
        if max(np.abs(wv).max(), abs(lam)) <= tol_rot and np.abs(delta[3:6]).max() <= tol_trans:
            st[_S_STATUS] = ICP_CONVERGED
    state.copy_(torch.as_tensor(st).to(state.device))
    return idx, d2


def _icp_torch(src, ref, normals, state, neighbours, with_scale, iters, tol_rot, tol_trans):
    """the loop of _icp_torch_step with the status rules (the status lives on the host here: one read per iteration)"""
    src64 = src.to(torch.float64)
    for _ in range(iters):
        if int(state[_S_STATUS]) != ICP_RUNNING:
            break
        _icp_torch_step(src64, ref, normals, state, neighbours, with_scale, tol_rot, tol_trans, True)


def icp(src, dst, init=None, dst_normals=None, max_dist=None, with_scale=False, iters=50, tol_rot=ICP_TOL_ROT, tol_trans=None,
        return_pairs=False, brute_force=False, state=None, read=True):
    """Registers the moving cloud `src` (float32 [M, 3]) to the fixed cloud `dst` (float32 [N, 3], or a PointGrid built over it: the
    grid is then reused across calls and cut-off stages) by ICP -> IcpResult.  Each iteration pairs every moved source point
    p' = s R p + t (fp64, rounded once to fp32) with its nearest point of dst by the distance rule, within max_dist (None: no
    cut-off), and takes one Gauss-Newton step on the similarity (with_scale) or rigid transform for the point-to-point residual,
    or, with dst_normals (float32 [N, 3], normals of the FIXED cloud), the point-to-plane residual; a cloud that brings none (a
    scan, the mapper's points, a back-projected depth map) gets them from ls2fm.cloud.estimate_normals(dst), whose sign does not
    matter here.  include/ls2fm.h states the rule
    (csrc/icp.hip: two launches per iteration, no host read, no floating-point atomic: a run is a pure function of its inputs);
    tests/icp_restate.py repeats it in numpy.
    init: the start, an (s, R, t) as align_sim3 returns it (None: the identity); state: an earlier result's state to continue from
    instead.  The loop stops at `iters` iterations (at most ICP_MAX_ITERS), when a step has max(|omega|, |lambda|) <= tol_rot and
    max |upsilon| <= tol_trans (status ICP_CONVERGED), or at a system that cannot be solved -- fewer pairs than unknowns, a pivot
    <= 0 -- (ICP_DEGENERATE, the transform as it was).  The defaults are an interface choice, not a measurement: tol_rot = 1e-9
    (ICP_TOL_ROT) and tol_trans = 1e-9 (ICP_TOL_TRANS_REL) times the diagonal of the fixed cloud's bounding box.
    The only host read is the final one for rmse, n_pairs, iterations and status; read=False skips it, and the call can then be
    captured into a graph (with dst a PointGrid: building one reads the box).  Deviations from the usual formulations: Gauss-Newton
    on the linearisation for both residuals, where point to point has a closed form (one accumulate and one solve serve both, and
    the camera alignment starts it close); normals on the fixed cloud only; no robust loss beyond the cut-off; a source point's
    correspondence is its nearest reference only.
    brute_force=True runs the same rule as plain torch ops on any device over nearest_neighbors_bruteforce, with the solve on the
    host: the timing baseline and the CPU route of the host tests; nothing in the library falls back to it."""
    src = points3(src, "src")
    grid = dst if isinstance(dst, PointGrid) else None
    ref = grid.ref if grid is not None else points3(dst, "dst")
    if not brute_force:
        require_device(src, ref, dst_normals)
    dev = src.device
    if ref.device != dev:
        raise ValueError(f"ls2fm.metrics.icp: src on {dev}, dst on {ref.device}")
    iters = int(iters)
    if not 0 <= iters <= ICP_MAX_ITERS:
        raise ValueError(f"ls2fm.metrics.icp: iters {iters} must be in [0, {ICP_MAX_ITERS}]")
    max_d2 = squared_cutoff(max_dist)
    n = int(ref.shape[0])
    normals = None
    if dst_normals is not None:
        normals = points3(dst_normals, "dst_normals")
        if normals.shape[0] != n or normals.device != dev:
            raise ValueError(f"ls2fm.metrics.icp: dst_normals {tuple(normals.shape)} on {normals.device} for {n} points on {dev}")
        normals = _lib.cf(normals)
    if tol_trans is None:
        if grid is not None:
            diagonal = float(np.linalg.norm(grid.box_max.astype(np.float64) - grid.origin.astype(np.float64)))
        elif brute_force:
            diagonal = float((ref.double().amax(dim=0) - ref.double().amin(dim=0)).norm()) if n else 0.0
        else:
            grid = PointGrid(ref)
            diagonal = float(np.linalg.norm(grid.box_max.astype(np.float64) - grid.origin.astype(np.float64)))
        tol_trans = ICP_TOL_TRANS_REL * diagonal
    tol_rot, tol_trans = float(tol_rot), float(tol_trans)
    if not (tol_rot >= 0 and tol_trans >= 0):
        raise ValueError(f"ls2fm.metrics.icp: tol_rot {tol_rot} and tol_trans {tol_trans} must be >= 0")
    src = _lib.cf(src)
    m = int(src.shape[0])
    if m >= 1 << 31:
        raise ValueError(f"ls2fm.metrics.icp: {m} source points, 2^31 or more")
    state = _icp_state(init, state, dev)
    if brute_force:
        ref = ref.float()
        neighbours = lambda p: nearest_neighbors_bruteforce(p, ref, max_dist)      # noqa: E731
        _icp_torch(src, ref, normals, state, neighbours, with_scale, iters, tol_rot, tol_trans)
        evaluation = state.clone()
        evaluation[_S_STATUS] = ICP_RUNNING
        idx, d2 = _icp_torch_step(src.to(torch.float64), ref, normals, evaluation, neighbours, with_scale, tol_rot, tol_trans, False)
        out = IcpResult(state, evaluation, *((idx, d2) if return_pairs else ()))
        return out.read() if read else out
    if grid is None:
        grid = PointGrid(ref)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.ls2fm_icp_workspace_bytes(m), "ls2fm_icp_workspace_bytes", dev)
        idx = torch.empty(m, dtype=torch.int32, device=dev) if return_pairs else None
        d2 = torch.empty(m, dtype=torch.float32, device=dev) if return_pairs else None

        def run(st, n_iters, pair_idx, pair_d2):
            check(lib.ls2fm_icp_run(ptr(src), m, *grid.c_args(), ptr(normals), float(max_d2), 1 if with_scale else 0, n_iters, tol_rot, tol_trans,
                                    ptr(st), None, ptr(pair_idx), ptr(pair_d2), ptr(ws), stream_ptr()), "ls2fm_icp_run")

        if iters:
            run(state, iters, None, None)
        # the closing evaluation: a copy of the state set to RUNNING, so that it runs whatever the status has become
        evaluation = state.clone()
        evaluation[_S_STATUS:_S_STATUS + 1].zero_()                 # ICP_RUNNING; a fill, not a host copy: capturable
        run(evaluation, 0, idx, d2)
    out = IcpResult(state, evaluation, idx, d2)
    return out.read() if read else out


_icp = icp          # evaluate_mesh has a parameter of this name
