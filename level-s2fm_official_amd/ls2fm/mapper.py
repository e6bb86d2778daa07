"""An incremental mapper on the device: the step that composes ls2fm.match / ls2fm.pose / ls2fm.tracks / ls2fm.stage.TradBALoop into a
reconstruction -- the view order `colmap mapper` is run for in the reference's preparation (preparation/main.py:106-175 ->
pose_graph.npy, read at pipelines/LevelS2fM.py:99-109) and the fully classical driver (Ablate_config.tri_trad + ba_trad with
nbv_mode != "colmap", pipelines/LevelS2fM.py:243-346: one PnP per candidate view, Registration_Trad.PnP, pairwise triangulation,
local and global BA_Trad).

`view_scores` (ls2fm_view_scores) is COLMAP's visibility-pyramid score of every view in one call and `update_observations`
(ls2fm_update_observations) holds the observation and point state to the current poses and points -- completing tracks into new
views, dropping observations that no longer reproject and points whose triangulation angle collapsed (csrc/mapper.hip; the rules
are in include/ls2fm.h, tests/mapper_restate.py repeats them in numpy).  `reconstruct` is the loop: the initial pair from ONE
relative_pose call over the best-matched pairs, then per step one view_scores call, ONE absolute_pose call over the best
candidates, refine_pose, update_observations, triangulate_tracks over a device-built sub-table of the tracks without a point, a
local and (every global_ba_every registrations) a global TradBALoop, update_observations.  It is deterministic: every ranking breaks
ties by the lower index and every device call repeats its bits.

Host reads per step: THREE small ones (tests/test_hip_mapper.py counts them).  (1) The [2, V] scores and counts that rank the
candidates; they also size the candidates' 2D-3D pairs, which absolute_pose takes as host-sized lists.  (2) The [2, K] verdict of
the absolute-pose call, the decision itself; a further group of candidates, tried only when a whole group fails, costs one more.
(3) One [2, V] vector of per-view counts before the bundle adjustments, because ls2fm_bundle_adjust_run takes its observation
count from the host.  Nothing else comes back: refine_pose and absolute_pose get per-view lists, so their start arrays are built
from host sizes; the bundle-adjustment loops take the intrinsic's host copy from the mapper instead of reading the device tensor
back; the log's figures stay on the device until the loop ends.

The initial pair must also not be one a homography explains: with H inliers above options.init_max_h_inlier_ratio (0.8, COLMAP's
max_H_inlier_ratio) of the relative pose's, the pair is planar or panoramic in COLMAP's verdict -- views without parallax are
explained by the five-point model as a plane under a rotation and a translation, with every match an inlier and a large median
angle, and only the homography tells.  COLMAP would still try such a pair with the pose of the homography; this mapper passes on.

Bundle adjustment: options.ba_solver = "adam" (the default) runs TradBALoop, the reference's loop; "lm" runs LMBALoop, Levenberg-
Marquardt with a Schur complement (ls2fm_bundle_adjust_lm_run): the first registered view constant when it is picked, soft_l1 for the
local adjustment and the plain squared error for the global one (COLMAP's choices), options.lm_iters iterations at most, the fp64
poses and points written back as they are.  At most 128 views can be adjusted at once with "lm".

Deviations from COLMAP's mapper: with "adam", Adam bundle adjustment instead of Ceres' Levenberg-Marquardt; with "lm", IRLS weights
without Ceres' second-order correction of the loss, a dense reduced camera system instead of a sparse or iterative Schur solver,
damping per block by its own diagonal; either way the error is in pixels and there is no refinement of the
intrinsics (one shared pinhole camera, as the reference and TradBALoop assume); no merging of points; completion and filtering by
pixel error (one threshold, options.tri_max_error_px) instead of angular error; tracks follow the conflict-dropping rule of
ls2fm.tracks (a component with two key points in one image is dropped whole), so no track is split while triangulating; a view
that fails its absolute pose is retried only while other candidates remain in the same step.

There is no CPU path for the device calls: CPU tensors, a missing device or a missing library raise.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from . import _lib, tracks as _tracks
from ._lib import check, ptr, stream_ptr

VIEW_SCORE_MAX = 17895696       # LS2FM_VIEW_SCORE_MAX: every cell of every level occupied
_STATUS = {1: f"track_start does not rise inside [0, n_obs] or a track has more than {_tracks.MAX_OBS} observations",
           2: "an obs_view outside [0, n_views)", 4: "a counting observation with a non-finite pixel"}


_device = functools.partial(_lib.require_device_tensors, "ls2fm.mapper")


def _table(tracks, obs_uv, what):
    ts, view = torch.as_tensor(tracks["track_start"]), torch.as_tensor(tracks["obs_view"])
    uv = torch.as_tensor(obs_uv)
    _device(ts, view, uv)
    dev = ts.device
    ts = ts.to(torch.int32).contiguous()
    view = view.to(device=dev, dtype=torch.int32).contiguous()
    uv = uv.to(device=dev, dtype=torch.float64).reshape(-1, 2).contiguous()
    T, n_obs = ts.numel() - 1, view.numel()
    if T < 0 or uv.shape[0] != n_obs:
        raise ValueError(f"ls2fm.mapper.{what}: {uv.shape[0]} pixel rows for {n_obs} observations of {T} tracks")
    return ts, view, uv, T, n_obs, dev


def _flags(x, n, dev, name, what):
    x = torch.as_tensor(x)
    _device(x)
    if x.numel() != n:
        raise ValueError(f"ls2fm.mapper.{what}: {x.numel()} {name} flags for {n}")
    return (x.reshape(-1) != 0).to(device=dev, dtype=torch.uint8).contiguous()


def view_scores(tracks, obs_uv, obs_keep, track_valid, registered, image_size, validate=True):
    """COLMAP's visibility-pyramid score of every view (ls2fm_view_scores; the rules are in include/ls2fm.h).  tracks: the dict of
    ls2fm.tracks.build_tracks (track_start, obs_view); obs_uv [n_obs, 2] pixels; obs_keep [n_obs], track_valid [T], registered [V]
    flags on the device; image_size (W, H) for all views or [V, 2].
    -> (score int64 [V], num_visible int32 [V] (= ls2fm.tracks.visible_points), status int32 [1]).
    The call reads nothing back and can be captured; validate=True (ignored while a stream is capturing) reads the status word
    afterwards and raises ValueError for a malformed table or a non-finite pixel."""
    ts, view, uv, T, n_obs, dev = _table(tracks, obs_uv, "view_scores")
    reg = torch.as_tensor(registered)
    _device(reg)
    V = reg.numel()
    reg = _flags(reg, V, dev, "registered", "view_scores")
    keep = _flags(obs_keep, n_obs, dev, "obs_keep", "view_scores")
    valid = _flags(track_valid, T, dev, "track_valid", "view_scores")
    if torch.is_tensor(image_size):
        _device(image_size)
        size = image_size.to(device=dev, dtype=torch.float64).reshape(-1, 2)
    else:
        h = np.asarray(image_size, np.float64).reshape(-1, 2)
        if not (np.isfinite(h).all() and (h > 0).all()):
            raise ValueError(f"ls2fm.mapper.view_scores: image sizes must be positive and finite, got {image_size}")
        size = torch.as_tensor(h, device=dev)
    if size.shape[0] == 1 and V > 1:
        size = size.expand(V, 2)
    if V < 1 or size.shape[0] != V:
        raise ValueError(f"ls2fm.mapper.view_scores: {size.shape[0]} image sizes for {V} views")
    size = size.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.ls2fm_view_scores_workspace_bytes(T, V, n_obs), "ls2fm_view_scores_workspace_bytes", dev)
        score = torch.empty(V, dtype=torch.int64, device=dev)
        num = torch.empty(V, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.ls2fm_view_scores(ptr(ts), T, ptr(view), ptr(uv), n_obs, ptr(keep), ptr(valid), ptr(reg), ptr(size), V, ptr(score),
                                    ptr(num), ptr(status), ptr(ws), stream_ptr()), "ls2fm_view_scores")
        if validate and not torch.cuda.is_current_stream_capturing():
            _lib.raise_status(status, "ls2fm.mapper.view_scores", _STATUS)
    return score, num, status


def update_observations(tracks, obs_uv, poses, intrinsics, registered, X, track_valid, max_error_px=4.0, min_tri_angle_deg=1.5,
                        validate=True):
    """The observation and point state at the current poses and points (ls2fm_update_observations; rules in include/ls2fm.h): an
    observation is kept iff its track was valid, its view is registered, the point lies in front of it and reprojects within
    max_error_px; a track stays valid iff it keeps >= 2 observations whose largest triangulation angle is >= min_tri_angle_deg.
    poses [V, 3, 4] world-to-camera (those of views that are not registered are not read), intrinsics as ls2fm.pose takes them,
    X [T, 3], track_valid [T], registered [V].
    -> dict(obs_keep bool [n_obs], track_valid bool [T], num_kept int32 [T], tri_angle fp64 [T] radians, status int32 [1]).
    Reads nothing back and can be captured; validate as in view_scores."""
    from .pose import _intrinsics
    if not (np.isfinite(max_error_px) and max_error_px > 0):
        raise ValueError(f"ls2fm.mapper.update_observations: max_error_px {max_error_px} must be positive and finite")
    if not 0.0 <= min_tri_angle_deg <= 90.0:
        raise ValueError(f"ls2fm.mapper.update_observations: min_tri_angle_deg {min_tri_angle_deg} outside [0, 90]")
    ts, view, uv, T, n_obs, dev = _table(tracks, obs_uv, "update_observations")
    p = torch.as_tensor(poses)
    x = torch.as_tensor(X)
    _device(p, x)
    if p.dim() != 3 or tuple(p.shape[1:]) != (3, 4):
        raise ValueError(f"ls2fm.mapper.update_observations: poses must be [V, 3, 4], got {tuple(p.shape)}")
    p = p.to(device=dev, dtype=torch.float64).contiguous()
    V = p.shape[0]
    x = x.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    if x.shape[0] != T:
        raise ValueError(f"ls2fm.mapper.update_observations: {x.shape[0]} points for {T} tracks")
    intr = _intrinsics(intrinsics, V, dev)
    reg = _flags(registered, V, dev, "registered", "update_observations")
    valid_in = _flags(track_valid, T, dev, "track_valid", "update_observations")
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.ls2fm_update_observations_workspace_bytes(T, V, n_obs), "ls2fm_update_observations_workspace_bytes", dev)
        keep = torch.empty(n_obs, dtype=torch.uint8, device=dev)
        valid = torch.empty(T, dtype=torch.uint8, device=dev)
        num = torch.empty(T, dtype=torch.int32, device=dev)
        ang = torch.empty(T, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.ls2fm_update_observations(ptr(p), ptr(intr), ptr(reg), V, ptr(ts), T, ptr(view), ptr(uv), n_obs, ptr(x), ptr(valid_in),
                                            float(max_error_px), float(min_tri_angle_deg), ptr(keep), ptr(valid), ptr(num), ptr(ang),
                                            ptr(status), ptr(ws), stream_ptr()), "ls2fm_update_observations")
        if validate and not torch.cuda.is_current_stream_capturing():
            _lib.raise_status(status, "ls2fm.mapper.update_observations", _STATUS)
    return dict(obs_keep=keep.view(torch.bool), track_valid=valid.view(torch.bool), num_kept=num, tri_angle=ang, status=status)


# ------------------------------------------------------------------------------------------------------------------ options
@dataclasses.dataclass
class MapperOptions:
    """The options of `reconstruct`; the names follow COLMAP's IncrementalMapperOptions where one exists.  lr_* are TradBALoop's
    rates (its ExponentialLR runs from lr_sdf to lr_sdf_end over each loop's iterations).  ba_solver: "adam" (TradBALoop with
    local_ba_iters / global_ba_iters and the rates) or "lm" (LMBALoop with lm_iters and the lm_* choices; at most 128 views)."""
    init_min_num_inliers: int = 100
    init_min_tri_angle_deg: float = 16.0
    init_candidates: int = 16
    init_max_h_inlier_ratio: float = 0.8
    abs_pose_max_error_px: float = 12.0
    abs_pose_min_num_inliers: int = 30
    abs_pose_min_inlier_ratio: float = 0.25
    next_view_candidates: int = 4
    tri_max_error_px: float = 4.0
    tri_min_angle_deg: float = 1.5
    local_ba_views: int = 6
    local_ba_iters: int = 1000
    global_ba_iters: int = 1000
    global_ba_every: int = 1
    seed: int = 0
    lr_pose_r: float = 5e-3
    lr_pose_t: float = 1e-2
    lr_xyzs: float = 1e-2
    lr_sdf: float = 1e-4
    lr_sdf_end: float = 5e-5
    ba_solver: str = "adam"
    lm_iters: int = 50
    lm_local_loss: str = "soft_l1"
    lm_local_loss_scale: float = 1.0
    lm_global_loss: str = "trivial"
    lm_global_loss_scale: float = 1.0
    lm_constant_first_view: bool = True

    def __post_init__(self):
        def refuse(name, why):
            raise ValueError(f"ls2fm.mapper.MapperOptions: {name} = {getattr(self, name)!r} {why}")

        for name in ("init_min_num_inliers", "init_candidates", "abs_pose_min_num_inliers", "next_view_candidates", "global_ba_every"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                refuse(name, "must be an integer >= 1")
        if self.abs_pose_min_num_inliers < 3:
            refuse("abs_pose_min_num_inliers", "must be >= 3 (the P3P sample)")
        if isinstance(self.local_ba_views, bool) or not isinstance(self.local_ba_views, (int, np.integer)) or self.local_ba_views < 2:
            refuse("local_ba_views", "must be an integer >= 2 (the new view and at least one other)")
        for name in ("local_ba_iters", "global_ba_iters", "seed"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                refuse(name, "must be an integer >= 0")
        for name in ("init_min_tri_angle_deg", "tri_min_angle_deg"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and 0.0 <= v <= 90.0):
                refuse(name, "must lie in [0, 90] degrees")
        for name in ("abs_pose_max_error_px", "tri_max_error_px", "lr_pose_r", "lr_pose_t", "lr_xyzs", "lr_sdf", "lr_sdf_end"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0.0):
                refuse(name, "must be positive and finite")
        for name in ("abs_pose_min_inlier_ratio", "init_max_h_inlier_ratio"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and 0.0 <= v <= 1.0):
                refuse(name, "must lie in [0, 1]")
        if self.ba_solver not in ("adam", "lm"):
            refuse("ba_solver", 'must be "adam" or "lm"')
        if isinstance(self.lm_iters, bool) or not isinstance(self.lm_iters, (int, np.integer)) or self.lm_iters < 0:
            refuse("lm_iters", "must be an integer >= 0")
        for name in ("lm_local_loss", "lm_global_loss"):
            if getattr(self, name) not in ("trivial", "soft_l1", "cauchy"):
                refuse(name, 'must be "trivial", "soft_l1" or "cauchy"')
        for name in ("lm_local_loss_scale", "lm_global_loss_scale"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0.0):
                refuse(name, "must be positive and finite")
        if not isinstance(self.lm_constant_first_view, bool):
            refuse("lm_constant_first_view", "must be a bool")

    def ba_rates(self):
        return dict(lr_pose_r=self.lr_pose_r, lr_pose_t=self.lr_pose_t, lr_xyzs=self.lr_xyzs, lr_sdf=self.lr_sdf, lr_sdf_end=self.lr_sdf_end)


# ------------------------------------------------------------------------------------------------------- rankings (host, pure)
def _pair_entry(n_views, a, b):
    """(rows [m, 2] of (key point of a, key point of b), mask bool [m]) of pair a < b, from view a's entry"""
    t = n_views[a]
    idx = np.asarray(t["indxes"][b - 1])
    if idx.size == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, bool)
    return idx.reshape(-1, 2).astype(np.int64), np.asarray(t["mask"][b - 1]).reshape(-1).astype(bool)


def rank_init_pairs(n_views, min_matches, limit):
    """The candidates for the initial pair: pairs (a, b), a < b, by their number of kept matches (the mask of the tables of
    ls2fm.match.two_view_tables), most first, ties by the lower (a, b); only pairs with >= min_matches, at most `limit`.
    -> list of (a, b, count).  Pure host function."""
    out = []
    for a in range(len(n_views)):
        for b in range(a + 1, len(n_views)):
            c = int(_pair_entry(n_views, a, b)[1].sum())
            if c >= min_matches:
                out.append((a, b, c))
    out.sort(key=lambda r: (-r[2], r[0], r[1]))
    return out[:int(limit)]


def rank_candidates(score, num_visible, registered, min_visible):
    """The next-view candidates: the views that are not registered and see >= min_visible points, by score, highest first, ties
    by the lower index -> list of view indices.  Pure host function."""
    score = np.asarray(score).reshape(-1)
    num = np.asarray(num_visible).reshape(-1)
    reg = np.asarray(registered).reshape(-1).astype(bool)
    ids = [v for v in range(len(score)) if not reg[v] and num[v] >= min_visible]
    ids.sort(key=lambda v: (-int(score[v]), v))
    return ids


# ------------------------------------------------------------------------------------------------------------ the result
class _BAViews:
    """what TradBALoop reads of a TrackedViews, over ALL views and ALL tracks (no renumbering: the loop adjusts its cam_pick and
    leaves the points no picked view observes unchanged)"""

    def __init__(self, poses_se3, intrinsic, host_intrinsic, keypoints, track_ids, xyzs):
        self.poses, self.intrinsic, self.keypoints, self.track_ids, self.xyzs = poses_se3, intrinsic, keypoints, track_ids, xyzs
        self.host_intrinsic = host_intrinsic                    # the same K as a CPU tensor


_LOOP = None


def _loop_class():
    """TradBALoop whose host copy of the intrinsic comes from the mapper's host values: TradBALoop moves the intrinsic to the device
    and reads it back for the C call's argument, one blocking read per loop; the mapper has the values on the host already"""
    global _LOOP
    if _LOOP is None:
        from .stage import TradBALoop

        class _MapperBALoop(TradBALoop):
            def _init_device(self):
                on_device = self.intrinsic
                self.intrinsic = self.views.host_intrinsic
                try:
                    super()._init_device()
                finally:
                    self.intrinsic = on_device

        _LOOP = _MapperBALoop
    return _LOOP


class Reconstruction:
    """What `reconstruct` returns.  order: the view indices in registration order, the initial pair first; registered bool [V]
    (host); poses fp64 [V, 3, 4] world-to-camera (identity for a view that is not registered); X fp64 [T, 3], track_valid bool [T],
    obs_keep bool [n_obs] over `tracks` (the dict of ls2fm.tracks.build_tracks) with obs_uv fp64 [n_obs, 2]; init: the initial
    pair's figures; log: one dict per registration (view, score, num_pairs, pnp_inliers, new_points, valid_points, ba_error)."""

    def __init__(self, order, registered, poses, X, track_valid, obs_keep, tracks, obs_uv, intrinsic, H, W, init, log):
        self.order, self.registered, self.poses, self.X = list(order), registered, poses, X
        self.track_valid, self.obs_keep, self.tracks, self.obs_uv = track_valid, obs_keep, tracks, obs_uv
        self.intrinsic, self.H, self.W, self.init, self.log = intrinsic, int(H), int(W), init, log

    def pose_graph(self):
        """the int array preparation/main.py saves as pose_graph.npy: the view indices in registration order"""
        return np.asarray(self.order, dtype=np.int64)

    def to_tracked_views(self, images=None):
        """ls2fm.stage.TrackedViews of the registered views, renumbered 0 .. in rising view index (`views` of the result lists
        them), with the valid points renumbered in track order: the input of TradBALoop or the neural loops"""
        from .stage import TrackedViews
        views = [v for v in range(len(self.registered)) if self.registered[v]]
        ts = self.tracks["track_start"].long()
        n_obs = self.tracks["obs_view"].numel()
        track_of = torch.bucketize(torch.arange(n_obs, device=ts.device), ts[1:], right=True)
        keep = self.obs_keep & self.track_valid[track_of]
        new_id = torch.cumsum(self.track_valid.long(), 0) - 1
        view = self.tracks["obs_view"].long()
        kps, ids = [], []
        for v in views:
            sel = keep & (view == v)
            kps.append(self.obs_uv[sel].float())
            ids.append(new_id[track_of[sel]])
        if any(k.shape[0] == 0 for k in kps):
            raise ValueError("ls2fm.mapper.Reconstruction.to_tracked_views: a registered view keeps no observation")
        dev = self.X.device
        if images is None:
            images = torch.zeros(len(views), 0, 3, device=dev)
        out = TrackedViews(self.poses[views], torch.as_tensor(self.intrinsic).to(dev).float(), images, kps, ids,
                           self.X[self.track_valid].float(), self.H, self.W)
        out.views = views
        return out

    def pose_errors(self, gt_poses, align=True, with_scale=True):
        """ls2fm.metrics.pose_errors of the registered views' poses against ground truth [V, 3, 4] or [V, 4, 4]"""
        from .metrics import pose_errors
        return pose_errors(self.poses, gt_poses, align=align, with_scale=with_scale,
                           registered=torch.as_tensor(np.asarray(self.registered, dtype=bool)))


# ---------------------------------------------------------------------------------------------------------------- the loop
def _intrinsic4(intrinsic):
    k = np.asarray(intrinsic.detach().cpu() if torch.is_tensor(intrinsic) else intrinsic, np.float64)
    if k.shape == (3, 3):
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape != (4,):
        raise ValueError(f"ls2fm.mapper.reconstruct: intrinsic must be K [3, 3] or (fx, fy, cx, cy), got shape {k.shape}")
    return k


def _angle(a, b):
    """min(t, pi - t) of the angle between the rows of a and b"""
    c = (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))
    t = torch.acos(c.clamp(-1.0, 1.0))
    return torch.minimum(t, math.pi - t)


class _Mapper:
    def __init__(self, n_views, intrinsic, H, W, opt, device):
        self.opt, self.n_views, self.H, self.W = opt, n_views, int(H), int(W)
        self.k4 = _intrinsic4(intrinsic)
        dev = self.dev = torch.device(device)
        self.K = torch.tensor([[self.k4[0], 0.0, self.k4[2]], [0.0, self.k4[1], self.k4[3]], [0.0, 0.0, 1.0]], dtype=torch.float64, device=dev)
        self.intr = torch.as_tensor(self.k4, device=dev)
        self.K_host = torch.tensor([[self.k4[0], 0.0, self.k4[2]], [0.0, self.k4[1], self.k4[3]], [0.0, 0.0, 1.0]], dtype=torch.float32)
        self.K_host64 = torch.tensor([[self.k4[0], 0.0, self.k4[2]], [0.0, self.k4[1], self.k4[3]], [0.0, 0.0, 1.0]], dtype=torch.float64)
        V = self.V = len(n_views)
        image_start, edges = _tracks.edges_from_n_views(n_views)
        self.kp = [torch.as_tensor(np.asarray(t["kypts"], np.float64).reshape(len(t["kypts"]), -1)[:, :2], device=dev) for t in n_views]
        self.tracks = tr = _tracks.build_tracks(image_start, torch.as_tensor(edges, device=dev))
        self.uv = _tracks._observations(tr, self.kp)
        self.T, self.n_obs = tr["track_start"].numel() - 1, tr["obs_view"].numel()
        self.view = tr["obs_view"].long()
        self.arange = torch.arange(self.n_obs, device=dev)
        self.track_of = torch.bucketize(self.arange, tr["track_start"].long()[1:], right=True)
        self.poses = torch.eye(3, 4, dtype=torch.float64, device=dev).repeat(V, 1, 1)
        self.reg_host = np.zeros(V, bool)
        self.reg = torch.zeros(V, dtype=torch.bool, device=dev)
        self.X = torch.zeros(self.T, 3, dtype=torch.float64, device=dev)
        self.track_valid = torch.zeros(self.T, dtype=torch.bool, device=dev)
        self.obs_keep = torch.zeros(self.n_obs, dtype=torch.bool, device=dev)
        self.size = torch.tensor([[float(self.W), float(self.H)]], dtype=torch.float64, device=dev).expand(V, 2).contiguous()
        self.order, self.log, self._pending = [], [], []

    # ---- the initial pair
    def initialise(self):
        opt = self.opt
        cands = rank_init_pairs(self.n_views, opt.init_min_num_inliers, opt.init_candidates)
        if not cands:
            raise RuntimeError(f"ls2fm.mapper.reconstruct: no initial pair: no view pair has {opt.init_min_num_inliers} kept matches")
        uv0, uv1 = [], []
        for a, b, _ in cands:
            rows, mask = _pair_entry(self.n_views, a, b)
            rows = torch.as_tensor(rows[mask], device=self.dev)
            uv0.append(self.kp[a][rows[:, 0]])
            uv1.append(self.kp[b][rows[:, 1]])
        from . import pose as _pose
        rel = _pose.relative_pose(uv0, uv1, self.intr, self.intr, seed=opt.seed)
        # the same pairs through ONE homography call: a pair a homography explains (COLMAP's PLANAR_OR_PANORAMIC verdict) is not taken
        hom = _pose.homography(uv0, uv1, seed=opt.seed)
        P = len(cands)
        P0 = (self.K @ torch.eye(3, 4, dtype=torch.float64, device=self.dev)).expand(P, 3, 4).contiguous()
        P1 = self.K @ rel["poses"]
        Xh = _pose.triangulate(P0, P1, uv0, uv1)
        counts = [u.shape[0] for u in uv0]
        pair_of = torch.repeat_interleave(torch.arange(P, device=self.dev), torch.tensor(counts, device=self.dev), output_size=sum(counts))
        Xe = Xh[:, :3] / Xh[:, 3:4]
        R, t = rel["poses"][:, :, :3], rel["poses"][:, :, 3]
        C1 = -(R.transpose(1, 2) @ t[:, :, None])[:, :, 0]
        ang = _angle(Xe, Xe - C1[pair_of])
        ang = torch.where(rel["inliers"] & torch.isfinite(ang), ang, torch.full_like(ang, float("nan")))
        # the median per pair in one call: the pairs' angles padded with NaN to [P, longest]
        first = rel["pair_start"].long()[:-1]
        padded = torch.full((P, max(counts)), float("nan"), dtype=torch.float64, device=self.dev)
        padded[pair_of, torch.arange(sum(counts), device=self.dev) - first[pair_of]] = ang
        med = torch.nanmedian(padded, dim=1).values
        verdict = torch.stack([rel["success"].double(), rel["num_inliers"].double(), med, hom["num_inliers"].double()]).cpu().numpy()      # the decision's read
        planar = verdict[3] > opt.init_max_h_inlier_ratio * verdict[1]
        for angle_deg in (opt.init_min_tri_angle_deg, 0.5 * opt.init_min_tri_angle_deg):
            for i, (a, b, c) in enumerate(cands):
                if verdict[0, i] and verdict[1, i] >= opt.init_min_num_inliers and not planar[i] and verdict[2, i] >= math.radians(angle_deg):
                    self.poses[b] = rel["poses"][i]
                    self.init = dict(pair=(a, b), matches=c, inliers=int(verdict[1, i]), median_angle_deg=math.degrees(verdict[2, i]), h_inliers=int(verdict[3, i]),
                                     min_tri_angle_deg=angle_deg, candidates=[(p, q) for p, q, _ in cands])
                    self._register(a)
                    self._register(b)
                    return
        medians = verdict[2][(verdict[0] > 0) & np.isfinite(verdict[2])]
        best = float(medians.max()) if medians.size else float("nan")
        raise RuntimeError(f"ls2fm.mapper.reconstruct: no initial pair: none of the {P} best-matched pairs has {opt.init_min_num_inliers} "
                           f"relative-pose inliers, a homography's inliers at most {opt.init_max_h_inlier_ratio:g} of them ({int(planar.sum())} pairs "
                           f"are planar or panoramic) and a median triangulation angle of {0.5 * opt.init_min_tri_angle_deg:g} degrees "
                           f"(the largest median was {math.degrees(best):.3g})")

    def _register(self, v):
        self.order.append(int(v))
        self.reg_host[v] = True
        self.reg[v] = True

    # ---- the state calls
    def update(self):
        r = update_observations(self.tracks, self.uv, self.poses, self.intr, self.reg, self.X, self.track_valid,
                                self.opt.tri_max_error_px, self.opt.tri_min_angle_deg, validate=False)
        self.obs_keep, self.track_valid = r["obs_keep"], r["track_valid"]

    def triangulate_new(self):
        """triangulate_tracks over the sub-table of the tracks without a point that have >= 2 observations in registered views, built
        on the device at fixed shapes (the chosen observations sorted to the front; a track without any is an empty track)
        -> the number of new points (0-d tensor)"""
        n_obs, T = self.n_obs, self.T
        cand = self.reg[self.view] & ~self.track_valid[self.track_of]
        cnt = torch.zeros(T, dtype=torch.int64, device=self.dev).index_add_(0, self.track_of, cand.long())
        sel = cand & (cnt >= 2)[self.track_of]
        perm = torch.argsort((~sel).long() * n_obs + self.arange)
        start = torch.zeros(T + 1, dtype=torch.int64, device=self.dev)
        start[1:] = torch.cumsum(torch.where(cnt >= 2, cnt, torch.zeros_like(cnt)), 0)
        sub = dict(track_start=start.to(torch.int32), obs_view=self.view[perm].to(torch.int32))
        tri = _tracks.triangulate_tracks(sub, None, self.poses, self.intr, self.opt.tri_max_error_px, self.opt.tri_min_angle_deg,
                                         obs_uv=self.uv[perm], validate=False)
        new = tri["success"] & ~self.track_valid
        self.X = torch.where(new[:, None], tri["X"], self.X)
        self.track_valid = self.track_valid | new
        inl = torch.zeros(n_obs, dtype=torch.bool, device=self.dev)
        inl[perm] = tri["inliers"] & sel[perm]
        self.obs_keep = self.obs_keep | (inl & new[self.track_of])
        return new.sum()

    def _ba_views(self, counts):
        """the kept observations as per-view lists (counts: their host counts per view, from the step's bookkeeping read)"""
        keep = self.obs_keep & self.track_valid[self.track_of]
        perm = torch.argsort(torch.where(keep, self.view, torch.full_like(self.view, self.V)) * self.n_obs + self.arange)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        ids = [self.track_of[perm[off[v]:off[v + 1]]] for v in range(self.V)]
        if self.opt.ba_solver == "lm":                              # fp64 as it is: no se(3) / fp32 round trip
            return _BAViews(self.poses, self.K, self.K_host64, [self.uv[perm[off[v]:off[v + 1]]] for v in range(self.V)], ids, self.X)
        kps = [self.uv[perm[off[v]:off[v + 1]]].float() for v in range(self.V)]
        from .utils import camera as _cam
        se3 = _cam.lie.SE3_to_se3(self.poses).float()
        return _BAViews(se3, self.K.float(), self.K_host, kps, ids, self.X.float())

    def bundle_adjust_lm(self, views, pick, local):
        """LMBALoop over the views `pick`; writes its fp64 poses and points back -> the mean pixel error at the end (0-d tensor)"""
        from .stage import LMBALoop
        opt = self.opt
        loss, scale = (opt.lm_local_loss, opt.lm_local_loss_scale) if local else (opt.lm_global_loss, opt.lm_global_loss_scale)
        loop = LMBALoop(views, cam_pick=pick, constant_views=self.order[:1] if opt.lm_constant_first_view else (), max_iter=opt.lm_iters,
                        loss=loss, loss_scale=scale)
        loop.run()
        self.poses[torch.as_tensor(pick, device=self.dev)] = loop.poses
        moved = torch.zeros(self.T, dtype=torch.bool, device=self.dev)
        moved[loop.obs_point] = True
        self.X = torch.where(moved[:, None], loop.xyzs_all, self.X)
        return loop.mean_error()

    def bundle_adjust(self, views, pick, iters):
        """TradBALoop over the views `pick`; writes back what BA_Trad writes back -> that iteration's mean error (0-d tensor)"""
        from .utils import camera as _cam
        if len(pick) == 1 and iters < 2:                         # a single picked view halves the iterations (BA_Trad.py:39-41)
            return torch.full((), float("nan"), dtype=torch.float64, device=self.dev)
        loop = _loop_class()(views, cam_pick=pick, max_iter=iters, **self.opt.ba_rates())
        loop.run()
        se3, xyz, err = loop.written_back()
        self.poses[torch.as_tensor(pick, device=self.dev)] = _cam.lie.se3_to_SE3(se3.double())
        moved = torch.zeros(self.T, dtype=torch.bool, device=self.dev)
        moved[loop.obs_point] = True
        self.X = torch.where(moved[:, None], xyz.double(), self.X)
        return err.double()

    def adjust(self, new_view, do_global):
        """the step's bookkeeping read, then the local and the global bundle adjustment -> mean error of the last one run"""
        opt = self.opt
        keep = self.obs_keep & self.track_valid[self.track_of]
        per_view = torch.zeros(self.V, dtype=torch.int64, device=self.dev).index_add_(0, self.view, keep.long())
        if new_view is None:
            shared = torch.zeros_like(per_view)
        else:
            has_new = torch.zeros(self.T, dtype=torch.int64, device=self.dev).index_add_(0, self.track_of, (keep & (self.view == new_view)).long()) > 0
            shared = torch.zeros(self.V, dtype=torch.int64, device=self.dev).index_add_(0, self.view, (keep & has_new[self.track_of]).long())
        h = torch.stack([per_view, shared]).cpu().numpy()                        # the bookkeeping read
        views = None
        err = torch.full((), float("nan"), dtype=torch.float64, device=self.dev)
        if opt.ba_solver == "lm":
            return self._adjust_lm(new_view, do_global, h, err)
        if new_view is not None and opt.local_ba_iters > 0 and h[0, new_view] > 0:
            others = [v for v in range(self.V) if v != new_view and self.reg_host[v] and h[1, v] > 0]
            others.sort(key=lambda v: (-int(h[1, v]), v))
            pick = [int(new_view)] + others[:opt.local_ba_views - 1]
            if not (do_global and opt.global_ba_iters > 0 and len(pick) == int(self.reg_host.sum())):      # the global one covers it
                views = self._ba_views(h[0])
                err = self.bundle_adjust(views, pick, opt.local_ba_iters)
        if do_global and opt.global_ba_iters > 0:
            pick = [v for v in range(self.V) if self.reg_host[v] and h[0, v] > 0]
            if pick:
                views = self._ba_views(h[0])                                      # the local loop moved poses and points
                err = self.bundle_adjust(views, pick, opt.global_ba_iters)
        return err

    def _adjust_lm(self, new_view, do_global, h, err):
        """`adjust` with LMBALoop: the same picks; both adjustments run options.lm_iters iterations at most"""
        opt = self.opt
        if opt.lm_iters < 1:
            return err
        n_reg = int(self.reg_host.sum())
        if new_view is not None and h[0, new_view] > 0:
            others = [v for v in range(self.V) if v != new_view and self.reg_host[v] and h[1, v] > 0]
            others.sort(key=lambda v: (-int(h[1, v]), v))
            pick = [int(new_view)] + others[:opt.local_ba_views - 1]
            if not (do_global and len(pick) == n_reg):                            # the global one covers it
                err = self.bundle_adjust_lm(self._ba_views(h[0]), pick, True)
        if do_global:
            pick = [v for v in range(self.V) if self.reg_host[v] and h[0, v] > 0]
            if pick:
                err = self.bundle_adjust_lm(self._ba_views(h[0]), pick, False)      # the local loop moved poses and points
        return err

    # ---- one registration
    def step(self, number):
        """-> False when no candidate is left or none could be registered"""
        from . import pose as _pose
        opt = self.opt
        score, num, _ = view_scores(self.tracks, self.uv, self.obs_keep, self.track_valid, self.reg, self.size, validate=False)
        h = torch.stack([score, num.long()]).cpu().numpy()                       # the ranking's read
        ranked = rank_candidates(h[0], h[1], self.reg_host, opt.abs_pose_min_num_inliers)
        if not ranked:
            return False
        # the counting observations sorted by view: view v owns h[1, v] of them (the rule of ls2fm_view_scores, as index operations)
        kept_reg = self.obs_keep & self.track_valid[self.track_of] & self.reg[self.view]
        seen = torch.zeros(self.T, dtype=torch.int64, device=self.dev).index_add_(0, self.track_of, kept_reg.long()) > 0
        counting = seen[self.track_of] & ~self.reg[self.view]
        perm = torch.argsort(torch.where(counting, self.view, torch.full_like(self.view, self.V)) * self.n_obs + self.arange)
        off = np.concatenate([[0], np.cumsum(h[1])]).astype(np.int64)
        for g in range(0, len(ranked), opt.next_view_candidates):
            group = ranked[g:g + opt.next_view_candidates]
            rows = [perm[off[v]:off[v + 1]] for v in group]
            uvs = [self.uv[r] for r in rows]
            xyz = [self.X[self.track_of[r]] for r in rows]
            res = _pose.absolute_pose(uvs, xyz, self.intr, max_error_px=opt.abs_pose_max_error_px,
                                      min_inlier_ratio=opt.abs_pose_min_inlier_ratio, seed=opt.seed + number, refine=False)
            verdict = torch.stack([res["success"].long(), res["num_inliers"].long()]).cpu().numpy()       # the decision's read
            for i, v in enumerate(group):
                n_pairs, n_inl = int(h[1, v]), int(verdict[1, i])
                if verdict[0, i] and n_inl >= opt.abs_pose_min_num_inliers and n_inl >= opt.abs_pose_min_inlier_ratio * n_pairs:
                    s = int(sum(h[1, u] for u in group[:i]))
                    mask = res["inliers"][s:s + n_pairs]
                    # one-element lists: the start array is then built from host sizes, nothing is read back
                    self.poses[v] = _pose.refine_pose([uvs[i]], [xyz[i]], self.intr, res["poses"][i:i + 1], mask)[0]
                    self._register(v)
                    self.update()
                    n_new = self.triangulate_new()
                    err = self.adjust(v, len(self.order) % opt.global_ba_every == 0)
                    self.update()
                    self.log.append(dict(view=int(v), score=int(h[0, v]), num_pairs=n_pairs, pnp_inliers=n_inl))
                    self._pending.append(torch.stack([n_new.double(), self.track_valid.sum().double(), err]))
                    return True
        return False

    def finish(self):
        if self._pending:
            rows = torch.stack(self._pending).cpu().numpy()                      # the log's figures, once
            for entry, (n_new, n_valid, err) in zip(self.log, rows):
                entry.update(new_points=int(n_new), valid_points=int(n_valid), ba_error=float(err))
        return Reconstruction(self.order, self.reg_host.copy(), self.poses, self.X, self.track_valid, self.obs_keep, self.tracks, self.uv,
                              self.K, self.H, self.W, self.init, self.log)


def reconstruct(n_views, intrinsic, H, W, options=None, device="cuda"):
    """Incremental structure from motion over the tables of ls2fm.match.two_view_tables / `n_views.npy` (per view a dict of kypts,
    indxes, mask) with one shared pinhole camera (K [3, 3] or (fx, fy, cx, cy)) and the image size H, W -> `Reconstruction`.
    Views that cannot be registered (no kept matches, another component) end with registered == False; that is not an error.
    RuntimeError when no initial pair passes options.init_min_num_inliers / init_min_tri_angle_deg (halved once)."""
    opt = MapperOptions() if options is None else options
    if not isinstance(opt, MapperOptions):
        raise TypeError("ls2fm.mapper.reconstruct: options must be a MapperOptions")
    if len(n_views) < 2:
        raise ValueError(f"ls2fm.mapper.reconstruct: {len(n_views)} views; two are needed")
    _lib.find_device("ls2fm.mapper")             # called for its refusal: without a device the mapper raises here
    m = _Mapper(n_views, intrinsic, H, W, opt, device)
    with torch.cuda.device(m.dev):
        m.initialise()
        m.update()                           # nothing is valid yet: clears the state
        n_new = m.triangulate_new()
        m.init["new_points"] = n_new
        m.adjust(None, True)
        m.update()
        number = 0
        while len(m.order) < m.V:
            number += 1
            if not m.step(number):
                break
        m.init["new_points"] = int(m.init["new_points"])
        return m.finish()


def refine_camera(rec, camera=None, refine=("f", "k1", "k2"), max_iter=50, loss="cauchy", loss_scale=2.0):
    """Estimate the shared camera's words from a finished `Reconstruction`: ONE global ls2fm.stage.LMBALoop over the registered
    views with THE CAMERA BLOCK of include/ls2fm.h, the first registered view constant -> (camera fp64 [12] on rec's device,
    Reconstruction).  camera: the starting 12 words of ls2fm.undistort (None: the pinhole rec.intrinsic with zero distortion);
    refine: the words that move, as LMBALoop takes them.  The photographs' own key points are
    distort_points(rec.obs_uv, camera, out_intr=rec.intrinsic); the returned reconstruction carries the new poses and points, those
    key points undistorted under the refined camera's pinhole, and that pinhole (K fp64 [3, 3], host) as its intrinsic.
    `reconstruct` itself still registers under fixed intrinsics: re-running it under a moving camera is not done here."""
    from . import undistort as _und
    from .stage import LMBALoop
    dev = rec.X.device
    k4 = torch.as_tensor(_intrinsic4(rec.intrinsic), dtype=torch.float64)
    if camera is None:
        camera = torch.cat([k4, torch.zeros(_und.CAMERA_PARAMS - 4, dtype=torch.float64)])
    camera = torch.as_tensor(camera).detach().to(device=dev, dtype=torch.float64)
    raw = _und.distort_points(rec.obs_uv.to(dev), camera, out_intr=k4)[0]
    views = [v for v in range(len(rec.registered)) if rec.registered[v]]
    if not views:
        raise ValueError("ls2fm.mapper.refine_camera: no registered view")
    ts = rec.tracks["track_start"].long()
    n_obs = rec.tracks["obs_view"].numel()
    track_of = torch.bucketize(torch.arange(n_obs, device=ts.device), ts[1:], right=True)
    keep = rec.obs_keep & rec.track_valid[track_of]
    new_id = torch.cumsum(rec.track_valid.long(), 0) - 1
    view = rec.tracks["obs_view"].long()
    sels = [keep & (view == v) for v in views]
    ba = _BAViews(rec.poses[views].double(), None, None, [raw[s] for s in sels], [new_id[track_of[s]] for s in sels],
                  rec.X[rec.track_valid].double())
    loop = LMBALoop(ba, constant_views=(views.index(rec.order[0]),) if rec.order else (0,), max_iter=max_iter, loss=loss,
                    loss_scale=loss_scale, camera=camera, refine=refine)
    loop.run()
    poses, X = rec.poses.clone(), rec.X.clone()
    poses[views] = loop.poses.to(poses.dtype)
    X[rec.track_valid] = loop.xyzs_all.to(X.dtype)
    out_cam = loop.camera.detach().clone()
    K = _und.intrinsic_matrices(out_cam[None, :4].cpu())[0]
    obs_uv = _und.undistort_points(raw, out_cam)[0].to(rec.obs_uv.dtype)
    return out_cam, Reconstruction(rec.order, rec.registered, poses, X, rec.track_valid, rec.obs_keep, rec.tracks, obs_uv, K, rec.H, rec.W,
                                   rec.init, rec.log)
