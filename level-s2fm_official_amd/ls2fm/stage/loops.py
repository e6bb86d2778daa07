"""The stage LOOPS: `Refine.run` (pipelines/rendering_refine.py:72-97) and `BA.run_ba` (pipelines/BA.py:110-188) as loops over
`RenderStage`, and beside them `Initializer.run`, `Registration.geo_init_nf` and `BA_Trad.BA`:
every iteration is the reference's -- ray pick, multi-view tracing consistency of one random camera's key points, render +
tracing + masks + losses, (BA: the point side and the re-projection through the pose parameters), one backward, one Adam
update over every parameter group, one ExponentialLR step -- with nothing read back to the host inside an iteration: the
reference's `.item()` (the adaptive re-projection weight, BA.py:164), `mask_surf.sum() == 0` and `mask_finish.sum() > 0`
branches are device-side selects here, the logs come back as device tensors.  Scene containers are plain tensors: the
reference's Camera / Point3D bookkeeping (COLMAP ids, feature tracks) stays with the caller.
"""
from __future__ import annotations

import ctypes
import math
import random

import numpy as np
import torch

from .. import _lib
from .. import dist as _dist
from .. import fused as _fused
from ..optim import FusedAdam
from ..undistort import _distort_torch, _jacobian_k_torch, _jacobian_torch
from ..utils import camera as _cam
from .step import RenderStage, _EarlyTrace, _capture_step, _point_side, _weight_factor, _weight_lookup
from .terms import _BATerms, _MatchTerm, _TracingTerm, _weighted_pair, host_intrinsic, reprojection_term


class TrackedViews:
    """What the loops need of a CameraSet + Point3DSet: world-to-camera poses [V,3,4] (or se(3) parameters [V,6]), one
    intrinsic matrix [3,3], the images as [V, H*W, 3], per view its key points [n_v, 2] (pixels) and the index of the tracked 3-D
    point each of them observes [n_v] (Camera.idx2d_to_3d entries != -1), the points [M,3]."""

    def __init__(self, poses, intrinsic, images, keypoints, track_ids, xyzs, H, W):
        self.poses, self.intrinsic, self.images = poses, intrinsic, images
        self.keypoints, self.track_ids, self.xyzs = list(keypoints), [t.long() for t in track_ids], xyzs
        self.H, self.W = int(H), int(W)
        self.grid = _cam.mesh_grid(H=H, W=W, device=images.device)
        n_max = max(k.shape[0] for k in self.keypoints)
        dev = images.device
        # key points padded to one shape (a captured step has fixed shapes): padding repeats the view's first key point -- a
        # duplicate ray finishes its sphere tracing exactly when the original does, so the global trip count is unchanged
        self.kp_pad = torch.stack([torch.cat([k, k[:1].expand(n_max - k.shape[0], 2)]) for k in self.keypoints]).to(dev)
        self.id_pad = torch.stack([torch.cat([t, t[:1].expand(n_max - t.shape[0])]) for t in self.track_ids]).to(dev)
        self.kp_live = torch.stack([torch.arange(n_max, device=dev) < k.shape[0] for k in self.keypoints]).float()
        # K^-1 on the host for the fused ray construction (ls2fm_camera_rays): read back here, once, outside any captured step
        self.kinv_host = _cam.host_inverse_intrinsic(intrinsic) if images.is_cuda else None

    @staticmethod
    def observations(views, device, pick=None):
        """the observation list of util.get_idx3d_camset (utils/util.py:450-464) of `views` -- a TrackedViews, or any object with its
        `track_ids` and `keypoints` (TradBALoop reads no more of the lists; the class itself pads key points and takes no empty
        view): per view of `pick` (None: every view, in order), every key point with a 3-D point, sorted by view -> obs_view [n] long (the position IN the pick), obs_point [n] long, obs_uv
        [n,2], view_start [len(pick) + 1] int32 (view j owns rows view_start[j] : view_start[j + 1]), all on `device`"""
        pick = range(len(views.track_ids)) if pick is None else pick
        ids = [views.track_ids[c] for c in pick]
        obs_view = torch.cat([torch.full((t.shape[0],), j, dtype=torch.long) for j, t in enumerate(ids)])
        view_start = torch.tensor([0] + [t.shape[0] for t in ids], dtype=torch.int64).cumsum(0).to(torch.int32)
        return (obs_view.to(device), torch.cat(ids).long().to(device), torch.cat([views.keypoints[c] for c in pick]).to(device),
                view_start.to(device))


def keypoint_rays(pose, intrinsic, kypts):
    """centers / rays of a view's key points as `Camera.get_pts3D` forms them (pipelines/Camera.py:129-133): pose [3,4],
    kypts [n,2] -> [1,n,3] each"""
    in_cam = _cam.img2cam(_cam.to_hom(kypts), intrinsic.unsqueeze(0))            # [1,n,3]
    center = _cam.cam2world(torch.zeros_like(in_cam), pose.unsqueeze(0))
    return center, _cam.cam2world(in_cam, pose.unsqueeze(0)) - center


def _to_pixels(uv):
    """homogeneous image coordinates [..,3] -> pixels [..,2] with the reference's guarded divide (Camera.py:173)"""
    return (uv / (uv[..., 2:] + 1e-6))[..., :2]


class TracingConsistency:
    """The multi-view tracing-consistency block of `CameraSet.render` (pipelines/Camera.py:466-476) as a step's extra loss:
    the key points of ONE view are sphere-traced onto the surface; tracing_loss = mean ||xyz - surface point||, and the SDF at
    the end of the tracks becomes `ret.sdfs` (sdf_surf = mean |sdfs|).  The view's rays live in buffers that `select()` rewrites
    in place, so a captured step sees the new view at replay."""

    def __init__(self, sdf_field, views, w_tracing, w_surf, static_trips=True):
        self.sdf, self.views, self.static = sdf_field, views, static_trips
        self.w_tracing, self.w_surf = _weight_factor(w_tracing), _weight_factor(w_surf)
        n = views.kp_pad.shape[1]
        dev = views.kp_pad.device
        self.center, self.ray = torch.zeros(1, n, 3, device=dev), torch.zeros(1, n, 3, device=dev)
        self.target, self.live = torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev)
        self.use_sdfs = True                   # False: `ret.sdfs` was set by the caller before the render (BA.py:122, Camera.py:474)
        self._early = _EarlyTrace(sdf_field, slot=1)

    def prepare(self):
        """launch the tracing now (RenderStage(extra_prepare=...)): it runs beside the render's forward"""
        if self.static:
            self._early.launch(self.center, self.ray)

    @torch.no_grad()
    def select(self, view, poses, fixed=None):
        """view: a Python int, or a DEVICE long tensor [1] (then nothing here touches the host: the selection can sit inside a
        captured step and follow the tensor's value at every replay).  fixed: a `_FixedPoseRays` of these poses."""
        if torch.is_tensor(view):
            pick = lambda t: t.index_select(0, view)[0]

            def into(src, index, out):
                # `out=` neither casts nor broadcasts, and a shape mismatch makes torch RESIZE the out tensor -- new storage, while
                # a captured graph and the early tracing hold the old address (round-4 advisor): refuse instead
                want = (index.numel(),) + tuple(src.shape[1:])
                if src.dtype != out.dtype or tuple(out.shape) != want:
                    raise RuntimeError(f"ls2fm.stage.TracingConsistency.select: source {tuple(src.shape)} {src.dtype} does not "
                                       f"fit the persistent buffer {tuple(out.shape)} {out.dtype}")
                torch.index_select(src, 0, index, out=out)
            if fixed is not None:
                into(fixed.kp_center, view, self.center)
                into(fixed.kp_ray, view, self.ray)
            elif self.views.kinv_host is not None and poses.shape[-1] == 4:
                # one launch: the selected view's pose and key points -> its rays, written into the buffers the tracing reads
                _cam.camera_rays(self.views.kinv_host, poses=poses, xy=self.views.kp_pad, view_sel=view, out=(self.center, self.ray))
            else:
                c, r = keypoint_rays(pick(poses), self.views.intrinsic, pick(self.views.kp_pad))
                self.center.copy_(c); self.ray.copy_(r)
            # index_select straight INTO the persistent buffers: a `.copy_()` of a fresh result is a device-to-device memcpy node in
            # a captured iteration -- 20 - 80 us each on this stack, against 4 us for the gather kernel writing in place
            into(self.views.xyzs, pick(self.views.id_pad), self.target)
            into(self.views.kp_live, view, self.live.view(1, -1))
            return
        c, r = keypoint_rays(poses[view], self.views.intrinsic, self.views.kp_pad[view])
        self.center.copy_(c); self.ray.copy_(r)
        self.target.copy_(self.views.xyzs[self.views.id_pad[view]])
        self.live.copy_(self.views.kp_live[view])

    def __call__(self, ret, raw=False):
        """raw=True (fused CUDA path without sdf_surf only): the UNWEIGHTED tracing loss -- the caller multiplies by `w_tracing`"""
        d, sdf_last = self._early.take_or_trace(self.center, self.ray, self.static)[:2]
        if d.is_cuda and d.dtype == torch.float32:
            # one node each way (ls2fm_tracing_term_fwd / _bwd): in a captured iteration every torch kernel of the lines below and
            # of their autograd mirror is a graph node of >= 4.6 us, whatever its size
            terms = _TracingTerm.apply(self.center, self.ray, d, self.target, self.live, sdf_last if self.use_sdfs else None)
            ret["tracing_loss"] = terms[0]
            if raw and not self.use_sdfs:          # the caller weights it inside a fused node of its own (BALoop)
                return ret["tracing_loss"]
            if self.use_sdfs:
                ret["sdf_surf"] = terms[1]
                return _weighted_pair(ret["tracing_loss"], ret["sdf_surf"], self.w_tracing, self.w_surf)
            return self.w_tracing * ret["tracing_loss"]
        # (few, fat torch ops: in a captured iteration every elementwise kernel here and in its backward is ~8 us of launch gap)
        surface = torch.addcmul(self.center[0], self.ray[0], d.reshape(-1, 1))
        weight = self.live / self.live.sum()                                    # no graph: 1 / count on the live key points
        ret["tracing_loss"] = torch.dot(torch.linalg.vector_norm(self.target - surface, dim=-1), weight)
        loss = self.w_tracing * ret["tracing_loss"]
        if self.use_sdfs:
            ret["sdf_surf"] = torch.dot(sdf_last.reshape(-1).abs(), weight)
            loss = loss + self.w_surf * ret["sdf_surf"]
        return loss


class _HostPicks:
    """The per-iteration ray pick of the loops -- the first k entries of a random permutation of the H W pixels, as the reference's
    `torch.randperm(H * W, device=...)[:k]` (pipelines/Camera.py:263, 431, 468) -- drawn on the HOST (numpy `Generator.choice`
    without replacement: the same distribution; seeded from `torch.initial_seed()`) and handed to the device with ONE asynchronous
    copy, together with the iteration's view index, from a ring of pinned buffers.  The device-side randperm is a radix sort of
    H W keys: 12 launches / 56 us in front of every captured iteration, for 15 us of host time that overlaps the previous
    iteration.  `dev[:k]` are the pixel indices, `dev[k:]` the tail values (the view); `device_picks=True` on a loop keeps the
    device-side draw."""
    RING = 8
    _instances = 0          # every loop instance draws from a stream of its own (round-5 advisor: they all replayed ONE sequence)

    def __init__(self, n_total, k, device, tail=1, shared=False):
        """shared=True (a loop under torch.distributed: every rank must evaluate the replicated terms on the SAME pixels and view):
        the generator is seeded with rank 0's seed -- one 8-byte broadcast at construction, no collective per iteration -- and
        the view index comes from the same generator (`view(V)`) instead of the process-global, per-rank `random` module."""
        self.n, self.k, self.tail = int(n_total), int(k), int(tail)
        seed = (int(torch.initial_seed()) + 0x9E3779B97F4A7C15 * _HostPicks._instances) & 0x7FFFFFFFFFFFFFFF
        _HostPicks._instances += 1
        self.shared = bool(shared) and _dist.is_distributed()
        if self.shared:
            import torch.distributed as tdist
            t = torch.tensor([seed], dtype=torch.long, device=device if tdist.get_backend() == "nccl" else "cpu")
            tdist.broadcast(t, 0)
            seed = int(t.item())
        self.rng = np.random.default_rng(seed)
        self.dev = torch.zeros(self.k + self.tail, dtype=torch.long, device=device)
        cuda = self.dev.is_cuda
        self.host = [torch.zeros(self.k + self.tail, dtype=torch.long).pin_memory() if cuda else torch.zeros(self.k + self.tail, dtype=torch.long)
                     for _ in range(self.RING if cuda else 1)]
        self.events = [None] * len(self.host)
        self.slot = 0

    def view(self, n_views):
        """the iteration's random view (the reference: `random.randint(0, V - 1)`): from this generator when the picks are shared
        between ranks, else from the `random` module as the reference draws it"""
        return int(self.rng.integers(0, n_views)) if self.shared else random.randint(0, n_views - 1)

    def shared_pixels(self, rays_idx):
        """a device-side pixel draw under a shared pick: rank 0's"""
        if self.shared:
            import torch.distributed as tdist
            tdist.broadcast(rays_idx, 0)
        return rays_idx

    def draw(self, *tail_values):
        h, ev = self.host[self.slot], self.events[self.slot]
        if ev is not None:
            ev.synchronize()                     # (the copy that last read this pinned buffer: RING iterations ago)
        h[:self.k] = torch.from_numpy(self.rng.choice(self.n, self.k, replace=False))
        for q, v in enumerate(tail_values):
            h[self.k + q] = int(v)
        self.dev.copy_(h, non_blocking=True)
        if self.dev.is_cuda:
            self.events[self.slot] = torch.cuda.Event()
            self.events[self.slot].record()
        self.slot = (self.slot + 1) % len(self.host)

    def pick(self, n_views=None, rays_idx=None, view=None, device_picks=False):
        """one iteration's pick, left in `dev`.  Nothing given: the host draw -- the view (when there is a tail slot for it) BEFORE
        the pixels, one asynchronous copy.  Else the caller's pixels, or (`device_picks`) the reference's device-side
        `torch.randperm(H * W, device=...)[:k]` (rank 0's under a shared pick), and the caller's view or a drawn one, written
        in place"""
        if rays_idx is None and view is None and not device_picks:
            self.draw(*([self.view(n_views)] if self.tail else []))
            return
        if rays_idx is None:
            rays_idx = self.shared_pixels(torch.randperm(self.n, device=self.dev.device)[:self.k])
        self.dev[:self.k].copy_(rays_idx)
        if self.tail:
            self.dev[self.k:].fill_(self.view(n_views) if view is None else int(view))


def _pick_rays(views, poses, rays_idx, se3=None, poses_out=None):
    """CameraSet.render's ray pick for given poses (Camera.py:457-463): the same pixels in every view.  se3 [V,6]: the poses are
    the exponentials of these parameters, formed in the same launch (and left in poses_out)"""
    if views.kinv_host is not None and not (poses if se3 is None else se3).requires_grad:
        centers, rays = _cam.camera_rays(views.kinv_host, poses=None if se3 is not None else poses, se3=se3, pix=rays_idx, width=views.W,
                                         poses_out=poses_out)
    else:
        if se3 is not None:
            poses = _cam.lie.se3_to_SE3(se3)
            if poses_out is not None:
                poses_out.copy_(poses)
        centers, rays = _cam.get_center_and_ray(None, poses, intr=views.intrinsic.unsqueeze(0), rays_idx=rays_idx, xy_grid=views.grid)
    return centers, rays, views.images[:, rays_idx, :]


class _FixedPoseRays:
    """Loops whose poses do not move (Refine, Init): the rays of EVERY pixel and of every (padded) key point are formed once;
    an iteration then only gathers its pick -- three index kernels instead of the ~40 launch-bound ones of the pinhole / pose
    algebra (which cost a captured iteration 0.3 ms).  Same arithmetic as `_pick_rays` / `keypoint_rays`: a ray does not depend on
    which other pixels are picked with it."""

    def __init__(self, views, poses):
        with torch.no_grad():
            self.centers, self.rays = _cam.get_center_and_ray(None, poses, intr=views.intrinsic.unsqueeze(0), rays_idx=None, xy_grid=views.grid)
            kc, kr = zip(*[keypoint_rays(poses[v], views.intrinsic, views.kp_pad[v]) for v in range(poses.shape[0])])
            self.kp_center, self.kp_ray = torch.cat(kc, dim=0), torch.cat(kr, dim=0)              # [V, n_max, 3]
        self.views = views

    def pick(self, rays_idx):
        return self.centers[:, rays_idx, :], self.rays[:, rays_idx, :], self.views.images[:, rays_idx, :]


class _LoggedLoop:
    """a loop whose `step(...)` returns one iteration's terms as device tensors and whose `_keys` names the ones to log"""

    def _run_logged(self, n_iters, step_args=None):
        """n_iters calls of `step(*step_args[it])` (None: `step()`) -> the logged terms, each stacked to [n_iters]"""
        logs = {k: [] for k in self._keys}
        for it in range(n_iters):
            ret = self.step(*(step_args[it] if step_args is not None else ()))
            for k in self._keys:
                logs[k].append(ret[k].detach().reshape(()).clone())
        return {("all" if k == "loss_all" else k): torch.stack(v) for k, v in logs.items()}


class RefineLoop(_LoggedLoop):
    """`Refine` (pipelines/rendering_refine.py:15-126): fields only, fixed poses, eikonal over every normal, tracing consistency
    and sdf_surf on one random view's key points.

        loop = RefineLoop(opt, renderer, sdf, rad, views, weights=opt.loss_weight.refine, lr_sdf=1e-3, lr_sdf_end=5e-4,
                          lr_color=1e-3, max_iter=500, rand_rays=8192)
        logs = loop.run()                      # {"all": [max_iter], "PSNR": ..., ...} device tensors

    picks: optional per-iteration (rays_idx, view) pairs (parity tests replay the reference's draws); default: the pixel indices and
    the view drawn on the host and copied in one asynchronous transfer (`_HostPicks`; `device_picks=True`: the reference's
    device-side `torch.randperm(H * W)` head) -- no device synchronisation either way."""

    def __init__(self, opt, renderer, sdf_field, rad_field, views, weights, lr_sdf, lr_sdf_end, lr_color, max_iter, rand_rays,
                 capture=False, static_trips=None, distributed=False, device_picks=False):
        """distributed=True (a process group is up; every rank holds the same views, weights and per-iteration picks): the render
        rays are sharded by view, the gradients all-reduced (RenderStage(shard_views=True, reducer="auto"))"""
        get = _weight_lookup(weights)
        self.views, self.max_iter, self.rand_rays = views, int(max_iter), int(rand_rays)
        static = _fused.available(sdf_field, views.images) if static_trips is None else static_trips
        self.extra = TracingConsistency(sdf_field, views, get("tracing_loss"), get("sdf_surf"), static_trips=static)
        self.stage = RenderStage(opt, renderer, sdf_field, rad_field, weights=weights, lr=lr_sdf, lr_end=lr_sdf_end, max_iter=max_iter,
                                 lr_color=lr_color, capture=capture, extra_loss=self.extra, eikonal_over="all", extra_prepare=self.extra.prepare,
                                 input_fn=self._inputs, share_gradients=bool(static), shard_views=bool(distributed),
                                 reducer="auto" if distributed else None)
        self.poses = views.poses if views.poses.shape[-1] == 4 else _cam.lie.se3_to_SE3(views.poses)
        self._keys = ("loss_all", "PSNR", "rgb_loss", "DC_loss", "eikonal_loss", "sdf_surf", "tracing_loss")
        # an iteration's picks as device tensors, updated in place: the ray pick and the key-point rays are formed INSIDE the step
        dev = self.poses.device
        k = self.rand_rays // self.poses.shape[0]
        self._picks = _HostPicks(views.H * views.W, k, dev, tail=1, shared=distributed)   # pixel indices + the view, one buffer, one copy per iteration
        self._idx, self._view = self._picks.dev[:k], self._picks.dev[k:]
        self.device_picks = bool(device_picks)
        self._fixed = _FixedPoseRays(views, self.poses)

    def _inputs(self):
        self.extra.select(self._view, self.poses, fixed=self._fixed)
        return self._fixed.pick(self._idx)

    def step(self, rays_idx=None, view=None):
        self._picks.pick(self.poses.shape[0], rays_idx, view, self.device_picks)
        return self.stage.step()

    def run(self, n_iters=None, picks=None):
        return self._run_logged(self.max_iter if n_iters is None else int(n_iters), picks)


class InitLoop(_LoggedLoop):
    """`Initializer.run` (pipelines/Initialization.py:139-226) for the two initial views with given poses (the essential-matrix
    pose initialisation of `Initializer.__init__` stays caller side: `ls2fm.pose.relative_pose`, or the one-line swap to
    `ls2fm.utils.pycolmap_compat.essential_matrix_estimation`, gives it on the device): per iteration the matched key points of each
    view are sphere-traced onto the surface and projected into the OTHER view (`Camera.proj_cam_i`, Camera.py:168-178) --
    reproj_error = mean ||uv_proj - key point||, sdf_surf = mean |SDF at the end of the tracks|, both over the 2 n tracks; the
    gradient reaches the SDF field through the traced depth -- then the render with the cameras' poses, eikonal over EVERY
    normal, rgb, depth consistency; one backward; Adam over the two fields (the poses are not in this optimizer,
    Initialization.py:124-125); ExponentialLR.  `triangulate()` is the block after the loop (Initialization.py:182-213).

    views: a two-view `TrackedViews` whose key points are the inlier matches, row j of view 0 <-> row j of view 1 (what
    `kypts[mch_msks[..., 0]][inlier_msks]` and `cam_i.kypts[mch_msks[..., 1]][inlier_msks]` select); track_ids / xyzs unused."""

    def __init__(self, opt, renderer, sdf_field, rad_field, views, weights, lr_sdf, lr_sdf_end, lr_color, max_iter, rand_rays,
                 capture=False, static_trips=None, sdf_filter=True, device_picks=False):
        get = _weight_lookup(weights)
        if len(views.keypoints) != 2 or views.keypoints[0].shape != views.keypoints[1].shape:
            raise ValueError("ls2fm.stage.InitLoop: two views with the same number of matched key points")
        self.sdf, self.views, self.max_iter, self.rand_rays = sdf_field, views, int(max_iter), int(rand_rays)
        self.sdf_filter = bool(sdf_filter)
        self.poses = (views.poses if views.poses.shape[-1] == 4 else _cam.lie.se3_to_SE3(views.poses)).detach()
        self.static = _fused.available(sdf_field, views.images) if static_trips is None else static_trips
        self.w_reproj, self.w_surf = _weight_factor(get("reproj_error")), _weight_factor(get("sdf_surf"))
        with torch.no_grad():              # the poses do not move during the loop: the key points' rays are formed once
            self._kp_rays = [keypoint_rays(self.poses[v], views.intrinsic, views.keypoints[v]) for v in range(2)]
        self.stage = RenderStage(opt, renderer, sdf_field, rad_field, weights=weights, lr=lr_sdf, lr_end=lr_sdf_end, max_iter=max_iter,
                                 lr_color=lr_color, capture=capture, extra_loss=self._extra, eikonal_over="all", extra_prepare=self._prepare,
                                 input_fn=lambda: self._fixed.pick(self._idx), share_gradients=bool(self.static))
        self._picks = _HostPicks(views.H * views.W, self.rand_rays // 2, self.poses.device, tail=0)
        self._idx = self._picks.dev
        self.device_picks = bool(device_picks)
        self._fixed = _FixedPoseRays(views, self.poses)
        self._keys = ("loss_all", "PSNR", "rgb_loss", "DC_loss", "eikonal_loss", "sdf_surf", "reproj_error")
        self._surface = self._finish = None
        self._early = [_EarlyTrace(sdf_field, slot=1), _EarlyTrace(sdf_field, slot=2)]
        self._match = None
        if self.poses.is_cuda and self.poses.dtype == torch.float32:
            # the fixed operands of the fused match node: segment v = the key points of view v, seen through the OTHER view
            with torch.no_grad():
                n = views.keypoints[0].shape[0]
                cen = torch.cat([self._kp_rays[v][0].reshape(-1, 3) for v in range(2)]).float().contiguous()
                ray = torch.cat([self._kp_rays[v][1].reshape(-1, 3) for v in range(2)]).float().contiguous()
                uv = torch.cat([views.keypoints[1 - v].reshape(-1, 2) for v in range(2)]).float().contiguous()
                pose_o = torch.stack([self.poses[1 - v] for v in range(2)]).float().contiguous()
            self._match = (cen, ray, uv, pose_o, host_intrinsic(views.intrinsic), n)
            self._surface_buf = torch.zeros(2, n, 3, device=self.poses.device)

    def _prepare(self):
        if self.static:
            for v in range(2):
                self._early[v].launch(*self._kp_rays[v])

    def _extra(self, ret):
        """the explicit-match terms (Initialization.py:154-160, 252-255), already weighted"""
        if self._match is not None:
            # one node each way for the whole block below (ls2fm_match_term_fwd / _bwd): ~70 graph nodes of a captured iteration
            ds, sls, fins = [], [], []
            for v in range(2):
                d, sdf_last, _, fin = self._early[v].take_or_trace(*self._kp_rays[v], self.static)
                ds.append(d); sls.append(sdf_last); fins.append(fin.reshape(-1).bool())
            terms = _MatchTerm.apply(self._match, self._surface_buf.view(-1, 3), *ds, *sls)
            ret["reproj_error"], ret["sdf_surf"] = terms[0], terms[1]
            self._surface, self._finish = self._surface_buf, torch.stack(fins)
            return _weighted_pair(ret["reproj_error"], ret["sdf_surf"], self.w_reproj, self.w_surf)
        errs, sdfs, surface, finish = [], [], [], []
        for v in range(2):
            center, ray = self._kp_rays[v]
            d, sdf_last, _, fin = self._early[v].take_or_trace(center, ray, self.static)
            pts = center + ray * d.reshape(1, -1, 1)                                             # Camera.py:136
            o = 1 - v
            uv = _to_pixels(_cam.cam2img(_cam.world2cam(pts, self.poses[o:o + 1]), self.views.intrinsic.unsqueeze(0)))
            errs.append((uv[0] - self.views.keypoints[o]).norm(dim=-1))
            sdfs.append(sdf_last.reshape(-1))
            surface.append(pts[0].detach())
            finish.append(fin.reshape(-1).bool())
        ret["reproj_error"] = torch.cat(errs).mean()
        ret["sdf_surf"] = torch.cat(sdfs).abs().mean()
        self._surface, self._finish = torch.stack(surface), torch.stack(finish)
        return self.w_reproj * ret["reproj_error"] + self.w_surf * ret["sdf_surf"]

    def step(self, rays_idx=None):
        self._picks.pick(rays_idx=rays_idx, device_picks=self.device_picks)
        return self.stage.step()

    def run(self, n_iters=None, picks=None):
        return self._run_logged(self.max_iter if n_iters is None else int(n_iters), None if picks is None else [(p,) for p in picks])

    @torch.no_grad()
    def triangulate(self):
        """-> (points [n,3], kept [n] bool): the mean of the two views' traced surface points of the LAST iteration; kept =
        within mean + 3 sigma of the two-view distance and (sdf_filter) finished in at least one view (Initialization.py:183-191).
        The caller adds `points[kept]` to its point set with the feature tracks (view 0 key point j, view 1 key point j)."""
        if self._surface is None:
            raise RuntimeError("ls2fm.stage.InitLoop.triangulate: run at least one step first")
        diff = (self._surface[0] - self._surface[1]).norm(dim=-1)
        kept = diff < diff.mean() + 3 * diff.std()
        if self.sdf_filter:
            kept = kept & (self._finish[0] | self._finish[1])
        return (self._surface[0] + self._surface[1]) / 2, kept


class GeoInitLoop(_LoggedLoop):
    """`Registration.geo_init_nf` (pipelines/Registration.py:133-296): a NEW view against registered ones, SDF field only, no
    render.  Per iteration ONE sphere tracing over the matched key points of every (new, registered) pair from both sides; for
    the matches without a 3-D point the two traced points are re-projected into the other view -- outliers by the finish flags
    and the 1x / 2x / 4x `reproj_max` bounds, as device-side masks (the reference's `(~mask).sum() > 0` is a select here) --,
    for the matches that have one the traced point is compared with it; sdf_surf over the tracks' last values and the existing
    points near the surface; eikonal over the existing points, the track points and the random along-ray points of
    `sphere_tracing` (fixed shape + mask, ls2fm.models.SDF); one backward; Adam over the SDF field; ExponentialLR with the
    reference's factor (lr_end / lr) ** (1 / max_iter) over its 5 * max_iter iterations.  `triangulate()` is the block after
    the loop.

    pairs: per registered view a dict  view (index into poses), kp_new [n,2], kp_src [n,2] (row j <-> row j: the inlier
    matches), point_id [n] long (index into xyzs of the 3-D point the new view's key point already has, -1: none)."""

    def __init__(self, opt, sdf_field, poses, intrinsic, new_view, pairs, xyzs, weights, lr_sdf, lr_sdf_end, max_iter, reproj_max=15.0,
                 capture=False):
        """capture=True: the first `step` records the whole iteration -- tracing, the fixed-shape sample points and their mask,
        three point-query nodes, every term, the backward, Adam with the schedule on the device -- into ONE hipGraph; later
        steps write the iteration's uniform draws into a persistent buffer and replay it."""
        get = _weight_lookup(weights)
        w = lambda k: _weight_factor(get(k))                                       # noqa: E731
        self.w_reproj, self.w_tracing, self.w_surf, self.w_eik = w("reproj_error"), w("tracing_loss"), w("sdf_surf"), w("eikonal_loss")
        self.sdf, self.intrinsic, self.xyzs = sdf_field, intrinsic, xyzs
        self.poses = (poses if poses.shape[-1] == 4 else _cam.lie.se3_to_SE3(poses)).detach()
        self.new_view, self.reproj_max = int(new_view), float(reproj_max)
        self.n_iters = 5 * int(max_iter)                                          # Registration.py:140
        self.pairs = []
        centers, rays = [[], []], [[], []]
        at = 0
        with torch.no_grad():
            for pr in pairs:
                n = pr["kp_new"].shape[0]
                c0, r0 = keypoint_rays(self.poses[self.new_view], intrinsic, pr["kp_new"])        # the new view's side (ret0)
                c1, r1 = keypoint_rays(self.poses[int(pr["view"])], intrinsic, pr["kp_src"])     # the registered view's side (ret1)
                centers[0].append(c0); rays[0].append(r0); centers[1].append(c1); rays[1].append(r1)
                pid = pr["point_id"].long()
                self.pairs.append(dict(view=int(pr["view"]), lo=at, hi=at + n, kp_new=pr["kp_new"], kp_src=pr["kp_src"], has=pid >= 0,
                                       target=xyzs[pid.clamp_min(0)], n_has=int((pid >= 0).sum())))
                at += n
            self.center = torch.cat([torch.cat(centers[0], dim=1), torch.cat(centers[1], dim=1)], dim=0)     # [2, sum n, 3]
            self.ray = torch.cat([torch.cat(rays[0], dim=1), torch.cat(rays[1], dim=1)], dim=0)
        self.n_frames = sum(1 for p in self.pairs if p["n_has"] > 0)
        self.params = [p for p in sdf_field.parameters() if p.requires_grad]
        self.optim = FusedAdam([dict(params=self.params, lr=lr_sdf)], lr=lr_sdf,
                               scheduled_gamma=(lr_sdf_end / lr_sdf) ** (1.0 / int(max_iter)))       # Registration.py:33
        self._one = torch.ones((), device=xyzs.device)
        self._last = None
        self._keys = ("loss_all", "reproj_error", "tracing_loss", "sdf_surf", "eikonal_loss")
        self.capture = bool(capture)
        self._graph = None
        self._u = torch.zeros(self.center.shape[0] * self.center.shape[1], device=xyzs.device)      # the draws of SDF.py:217

    def step(self, sample_u=None):
        """one iteration; sample_u [2 * n]: the uniform draws that place the along-ray eikonal points (parity tests replay the
        reference's); default: fresh device-side draws"""
        if not self.capture:
            ret, self._last = self._iteration(sample_u)
            return ret
        if sample_u is None:
            self._u.uniform_()
        else:
            self._u.copy_(sample_u.reshape(-1))
        if self._graph is None:
            self._graph = _capture_step(lambda: self._iteration(self._u), self.params, self.optim)
        ret, self._last = self._graph.replay()
        self.optim.replayed(1)
        return ret

    def _project(self, pts, view):
        return _to_pixels(_cam.cam2img(_cam.world2cam(pts.unsqueeze(0), self.poses[view:view + 1]), self.intrinsic.unsqueeze(0))[0])

    def _iteration(self, sample_u=None):
        for p in self.params:
            p.grad = None
        sdf = self.sdf
        d, sdf_last, sampled, fin = sdf.sphere_tracing(self.center, self.ray, sdf, static_trips=True, want_samples=True, sample_u=sample_u)
        pts = self.center + self.ray * d.reshape(2, -1, 1)                                         # Registration.py:190
        fin = fin.reshape(2, -1).bool()
        zero = torch.zeros((), device=pts.device)
        reproj, n_reproj, tracing, last = zero, zero, zero, []
        rmax = self.reproj_max
        for pr in self.pairs:
            p0, p1 = pts[0, pr["lo"]:pr["hi"]], pts[1, pr["lo"]:pr["hi"]]
            f0, f1 = fin[0, pr["lo"]:pr["hi"]], fin[1, pr["lo"]:pr["hi"]]
            e0 = (self._project(p0, pr["view"]) - pr["kp_src"]).norm(dim=-1)                      # new view's point in the registered view
            e1 = (self._project(p1, self.new_view) - pr["kp_new"]).norm(dim=-1)
            bad = ((f0 & (e0 > rmax)) & (f1 & (e1 > rmax))) | ((e0 > 2 * rmax) & (e1 > 2 * rmax)) | (e0 > 4 * rmax) | (e1 > 4 * rmax)
            keep = (~pr["has"]) & ~bad
            cnt = keep.sum()
            some = cnt > 0
            pair_err = ((e0 * keep).sum() + (e1 * keep).sum()) / (2 * cnt.clamp_min(1))
            reproj = reproj + torch.where(some, pair_err, zero)
            n_reproj = n_reproj + some
            dist = (pr["target"] - p0).norm(dim=-1)
            if pr["n_has"] > 0:
                tracing = tracing + (dist * pr["has"]).sum() / pr["n_has"]
            last.append((p0.detach(), p1.detach(), f0, f1, keep, dist.detach()))
        # the existing points: near-surface ones enter sdf_surf, all of them the eikonal term (Registration.py:257-262)
        sdf_exist = sdf.infer_sdf(self.xyzs).reshape(-1)
        near = sdf_exist.detach().abs() < float(sdf.sdf_threshold)
        grad_exist = sdf.gradient(self.xyzs).norm(dim=-1).reshape(-1)
        sdf_surf = ((sdf_exist.abs() * near).sum() + sdf_last.reshape(-1).abs().sum()) / (near.sum() + sdf_last.numel())
        live = sdf.last_sample_mask.reshape(-1)
        grad_sampled = sdf.gradient(sampled.reshape(-1, 3)).norm(dim=-1).reshape(-1)
        eik = ((grad_exist - 1).abs().sum() + ((grad_sampled - 1).abs() * live).sum()) / (grad_exist.numel() + live.sum())
        any_reproj = n_reproj > 0
        ret = dict(reproj_error=torch.where(any_reproj, reproj / n_reproj.clamp_min(1), zero),
                   tracing_loss=tracing / max(self.n_frames, 1), sdf_surf=sdf_surf, eikonal_loss=eik)
        ret["loss_all"] = (self.w_reproj * ret["reproj_error"] + self.w_tracing * ret["tracing_loss"] + self.w_surf * sdf_surf
                           + self.w_eik * eik)
        ret["loss_all"].backward(gradient=self._one)
        self.optim.step()
        return ret, last

    def run(self, n_iters=None, draws=None):
        return self._run_logged(self.n_iters if n_iters is None else int(n_iters), None if draws is None else [(u,) for u in draws])

    @torch.no_grad()
    def triangulate(self):
        """-> per pair (points [n,3], kept [n] bool): the block after the loop (Registration.py:271-294) on the LAST iteration's
        traced points -- a new match becomes a 3-D point (the mean of its two traced points) when the two agree within mean + std of
        the existing matches' tracing distances, or both tracks finished"""
        if self._last is None:
            raise RuntimeError("ls2fm.stage.GeoInitLoop.triangulate: run at least one step first")
        record = torch.cat([dist[pr["has"]] for pr, (_, _, _, _, _, dist) in zip(self.pairs, self._last)])
        thr = record.mean() + record.std()
        out = []
        for p0, p1, f0, f1, keep, _ in self._last:
            diff = (p0 - p1).norm(dim=-1)
            out.append(((p0 + p1) / 2, keep & ((diff <= thr) | (f0 & f1))))
        return out


class BALoop(_LoggedLoop):
    """`BA` in mode "sfm_refine" with several cameras (pipelines/BA.py:24-218; optim_split: rotation / translation parameters
    with their own rates, BA.py:66-75): per iteration the POINT side -- tracked points projected onto the surface
    (get_surface_pts), re-evaluated (infer_sdf), re-projected through the live poses against their key points (robust mean over
    |sdf| < 2 thr), the adaptive weight 10^1 when the error exceeds 10 px (BA.py:163-166) -- then the render side with the
    poses detached (BA.py:150-151), eikonal over mask_bg, sdf_surf over the points, tracing consistency; one backward; Adam over
    {rotations, translations, SDF field, radiance field}; ExponentialLR; the points are replaced by their projections
    (BA.py:181)."""

    def __init__(self, opt, renderer, sdf_field, rad_field, views, weights, lr_sdf, lr_sdf_end, lr_color, lr_pose_r, lr_pose_t,
                 max_iter, rand_rays, capture=False, static_trips=None, distributed=False, device_picks=False):
        """distributed=True: BASELINE.json configs[3] -- the render rays of the registered views sharded by view over the ranks of
        the process group, one gradient all-reduce per iteration (fields' flat buffer + the pose groups); the point side,
        re-projection and tracing consistency are evaluated on every rank (same inputs) with weight 1 / world in the backward"""
        get = _weight_lookup(weights)
        self.opt, self.sdf, self.views = opt, sdf_field, views
        self.max_iter, self.rand_rays = int(max_iter), int(rand_rays)
        se3 = views.poses if views.poses.shape[-1] == 6 else _cam.lie.SE3_to_se3(views.poses)
        self.rot = torch.nn.Parameter(se3[:, :3].detach().clone())
        self.trans = torch.nn.Parameter(se3[:, 3:].detach().clone())
        self.obs_view, self.obs_point, self.obs_uv, self.view_start = TrackedViews.observations(views, se3.device)
        self._k_host = host_intrinsic(views.intrinsic)
        # the loop's OWN copy of the points (BA.py:77): it is what gets projected and replaced every iteration, while the
        # tracing consistency keeps comparing against the point set's coordinates, which do not move during the loop (and not
        # after it either: Point3DSet.update_xyzs never runs its lazy map, SURVEY C-13)
        self.xyzs_all = views.xyzs.detach().clone()
        self.w_surf, self.w_reproj_lo = _weight_factor(get("sdf_surf")), _weight_factor(get("reproj_error"))
        self.sdf_threshold = float((float(opt.data.bound_max[0]) - float(opt.data.bound_min[0])) / 10 / int(opt.Res))
        static = _fused.available(sdf_field, views.images) if static_trips is None else static_trips
        self.tracing = TracingConsistency(sdf_field, views, get("tracing_loss"), None, static_trips=static)
        self.tracing.use_sdfs = False
        self.stage = RenderStage(opt, renderer, sdf_field, rad_field, weights=weights, lr=lr_sdf, lr_end=lr_sdf_end, max_iter=max_iter,
                                 lr_color=lr_color, capture=capture, extra_loss=self._extra, eikonal_over="bg",
                                 extra_params=[dict(params=[self.rot], lr=lr_pose_r), dict(params=[self.trans], lr=lr_pose_t)],
                                 extra_prepare=self._prepare, input_fn=self._inputs, share_gradients=bool(static),
                                 shard_views=bool(distributed), reducer="auto" if distributed else None)
        k = self.rand_rays // se3.shape[0]
        self._picks = _HostPicks(views.H * views.W, k, se3.device, tail=1, shared=distributed)
        self._idx, self._view = self._picks.dev[:k], self._picks.dev[k:]
        self.device_picks = bool(device_picks)
        self._keys = ("loss_all", "PSNR", "rgb_loss", "DC_loss", "eikonal_loss", "sdf_surf", "tracing_loss", "reproj_error", "w_reproj")
        self._render_poses = torch.zeros(se3.shape[0], 3, 4, device=se3.device)
        # the key-point rays of the tracing consistency come from the CAMERAS' own poses (Camera.get_pts3D -> get_pose,
        # Camera.py:131), which the loop only writes back after its last iteration (BA.py:184-185): fixed during the loop
        self._camera_poses = _cam.lie.se3_to_SE3(se3).detach()
        self._point_side = None            # (xyzs_new, sdfs) of `_prepare`, consumed by the same step's `_extra`
        self._w_hi = self._w_lo = None     # the adaptive weight's two values as device constants (torch-op branch of `_extra`)

    def _inputs(self):
        self.tracing.select(self._view, self._camera_poses)
        with torch.no_grad():            # the render poses are detached (BA.py:150-151): exponential + ray pick in one launch
            return _pick_rays(self.views, None, self._idx, se3=torch.cat([self.rot, self.trans], dim=1), poses_out=self._render_poses)

    def _prepare(self):
        """ahead of the render, as in BA.run_ba (BA.py:117-131 come before its render call): the tracing consistency's key-point
        tracing starts on a stream of its own, and the point side's two field queries are issued -- their autograd nodes then
        PRECEDE the render's, so that in the backward they run after it and add into its gradient buffer (ls2fm.fused: one
        gradient buffer per backward pass) instead of producing dense gradients of their own"""
        self.tracing.prepare()
        self._point_side = self._project_points()

    def _project_points(self):
        xyzs_new, _, sdfs = _point_side(self.sdf, self.xyzs_all[self.obs_point])
        return xyzs_new, sdfs

    def _extra(self, ret):
        """the terms BA.run_ba forms outside the render (BA.py:119-147) + the tracing consistency, already weighted"""
        xyzs_new, sdfs = self._project_points() if self._point_side is None else self._point_side
        self._point_side = None
        poses = _cam.se3_to_SE3_fused(torch.cat([self.rot, self.trans], dim=1))                  # [V,3,4]: the live poses
        if xyzs_new.is_cuda:
            # one fused node each way for the per-observation block (projection, pixel error, on-surface / finite mask, robust mean)
            reproj, _ = reprojection_term(xyzs_new, poses, self.view_start, self._k_host, self.obs_uv, sdfs, 2 * self.sdf_threshold)
        else:
            reproj = self._reproj_torch(xyzs_new, poses, sdfs)
        if xyzs_new.is_cuda and sdfs.dtype == torch.float32:
            # BA.py:160-170 as one node each way: sdf_surf, the adaptive weight, the weighted sum with the tracing loss
            on = 1.0 if self.w_reproj_lo else 0.0
            tl = self.tracing(ret, raw=True)           # unweighted on its fused path (then it IS ret["tracing_loss"]), else weighted
            raw = tl is ret.get("tracing_loss")
            surf, w_reproj, extra = _BATerms.apply(reproj, sdfs, tl if raw else None, 10.0, on, 10.0 * on, self.w_surf,
                                                   self.tracing.w_tracing if raw else 0.0)
            ret["reproj_error"], ret["w_reproj"], ret["sdf_surf"] = reproj, w_reproj, surf
            self._new_points = xyzs_new.detach()
            return extra if raw else extra + tl
        if self._w_hi is None or self._w_hi.device != reproj.device:       # constants once, not two fill kernels per iteration
            on = 1.0 if self.w_reproj_lo else 0.0
            self._w_hi, self._w_lo = torch.full((), 10.0 * on, device=reproj.device), torch.full((), on, device=reproj.device)
        w_reproj = torch.where(reproj.detach() > 10, self._w_hi, self._w_lo)                  # BA.py:163-166
        ret["reproj_error"], ret["w_reproj"] = reproj, w_reproj
        ret["sdf_surf"] = sdfs.abs().mean()
        self._new_points = xyzs_new.detach()
        return w_reproj * reproj + self.w_surf * ret["sdf_surf"] + self.tracing(ret)

    def _reproj_torch(self, xyzs_new, poses, sdfs):
        """the same term written with torch ops (the reference's lines: BA.py:126-147, 199-202)"""
        in_cam = _cam.world2cam(xyzs_new.unsqueeze(1), poses[self.obs_view])
        uv = _cam.cam2img(in_cam, self.views.intrinsic.expand(in_cam.shape[0], 3, 3))
        uv = _to_pixels(uv).squeeze(1)
        on_surface = (sdfs.abs() < 2 * self.sdf_threshold).squeeze(-1) & ~torch.isinf(uv).any(dim=-1)
        err = torch.where(on_surface, (uv - self.obs_uv).norm(dim=-1), torch.zeros((), device=uv.device))
        n = on_surface.sum()
        robust = torch.where(on_surface, 2 * torch.log(1 + err ** 2 / 4), torch.zeros((), device=uv.device))
        return torch.where(n > 0, 0.5 * robust.sum() / n.clamp_min(1) + 0.5 * err.sum() / n.clamp_min(1), torch.zeros((), device=uv.device))

    def step(self, rays_idx=None, view=None):
        self._picks.pick(self.rot.shape[0], rays_idx, view, self.device_picks)
        ret = self.stage.step()
        with torch.no_grad():
            self.xyzs_all[self.obs_point] = self._new_points                                     # BA.py:181
        return ret

    def run(self, n_iters=None, picks=None):
        return self._run_logged(self.max_iter if n_iters is None else int(n_iters), picks)

    def poses_se3(self):
        return torch.cat([self.rot, self.trans], dim=1).detach()


class TradBALoop:
    """`BA_Trad.BA` (pipelines/BA_Trad.py:16-130, the bundle adjustment behind `Ablate_config.ba_trad`): the explicit 3-D points
    and the se(3) poses of the picked views are the parameters; no field, no renderer, no `opt`.  Per iteration: the live poses
    `se3_to_SE3(cat(r, t))`, every observation of `util.get_idx3d_camset` (per picked view, every key point that has a 3-D point)
    projected with the FIRST camera's intrinsic, `reproj = 0.5 mean(2 log(1 + err^2 / 4)) + 0.5 mean(err)` over all of them, the
    weight 10^1 when `reproj > 10` else 10^0 (the reference's `.item()` decision: a select on the device), backward, Adam over
    {rotations: lr_pose_r, translations: lr_pose_t, points: lr_xyzs}, ExponentialLR with gamma = (lr_sdf_end / lr_sdf)^(1 / max_iter).

    views: `TrackedViews` (its `images` are not read; `poses` may be [V,6] se(3) parameters or [V,3,4]).  cam_pick: the views to
    adjust, in this order (`cam_pick_ids`; None: all; a single one halves max_iter, BA_Trad.py:39-41).  w_reproj is the exponent the
    reference keeps in `opt.loss_weight.ba.reproj_error`; the loop overwrites it before its first use, so it only names the state.

    On the device `run()` is ONE call of ls2fm_bundle_adjust_run (two launches per iteration, nothing read back); off the device the
    same iteration runs as torch ops (autograd, torch.optim.Adam, ExponentialLR) so that the bookkeeping is testable anywhere.

    State after `run()` / `step()`:
      poses_se3(), xyzs_all     the STEPPED state: after the last Adam step (what a resumed loop continues from; all points of the
                                set, the ones no picked view observes unchanged)
      written_back()            (se3 [V,6], xyzs [M,3], mean err): the state that ENTERED the last iteration and that iteration's
                                mean(err) -- what BA_Trad writes into its cameras / returns after the loop (BA_Trad.py:124-128);
                                a drop-in caller writes THIS back
    """

    def __init__(self, views, cam_pick=None, lr_pose_r=5e-3, lr_pose_t=1e-2, lr_xyzs=1e-2, lr_sdf=1e-4, lr_sdf_end=5e-5, max_iter=1000,
                 w_reproj=0):
        n_all = len(views.track_ids)
        self.cam_pick = list(range(n_all)) if cam_pick is None else [int(c) for c in cam_pick]
        if not self.cam_pick or any(c < 0 or c >= n_all for c in self.cam_pick):
            raise ValueError(f"cam_pick {self.cam_pick} does not select views of 0..{n_all - 1}")
        max_iter = int(max_iter)
        if cam_pick is not None and len(self.cam_pick) == 1:
            max_iter = max_iter // 2
        if max_iter < 1:
            raise ValueError("max_iter < 1")
        self.max_iter, self.it = max_iter, 0
        self.lrs = (float(lr_pose_r), float(lr_pose_t), float(lr_xyzs))
        self.gamma = (float(lr_sdf_end) / float(lr_sdf)) ** (1.0 / max_iter)
        self.w_reproj = w_reproj
        self.views = views
        dev = views.xyzs.device
        se3_all = views.poses if views.poses.shape[-1] == 6 else _cam.lie.SE3_to_se3(views.poses)
        self.se3 = se3_all[self.cam_pick].detach().float().clone().contiguous().to(dev)
        self.xyzs_all = views.xyzs.detach().float().clone().contiguous()
        self.obs_view, self.obs_point, obs_uv, self.view_start = TrackedViews.observations(views, dev, self.cam_pick)
        self.obs_uv = obs_uv.float().contiguous()
        self.intrinsic = views.intrinsic.detach().float().to(dev)
        self.se3_entering_last, self.xyzs_entering_last = self.se3.clone(), self.xyzs_all.clone()
        self._err_last = None
        self._keys = ("reproj_error", "w_reproj", "err_mean")
        if self.xyzs_all.is_cuda:
            self._init_device()
        else:
            self._init_torch()

    # ---- device path
    def _init_device(self):
        lib = _lib.load()
        V, P, n, dev = self.se3.shape[0], self.xyzs_all.shape[0], self.obs_point.shape[0], self.se3.device
        self._ws = _lib.workspace(lib.ls2fm_bundle_adjust_workspace_bytes(V, P, n), "ls2fm_bundle_adjust_workspace_bytes", dev)
        self._obs_point32 = self.obs_point.to(torch.int32).contiguous()
        _lib.check(lib.ls2fm_bundle_adjust_prepare(_lib.ptr(self.view_start), V, _lib.ptr(self._obs_point32), n, P, _lib.ptr(self._ws),
                                                   _lib.stream_ptr()), "ls2fm_bundle_adjust_prepare")
        self._k_host = host_intrinsic(self.intrinsic)
        self._m = [torch.zeros_like(self.se3), torch.zeros_like(self.se3), torch.zeros_like(self.xyzs_all), torch.zeros_like(self.xyzs_all)]

    def _run_device(self, n_iters):
        lib = _lib.load()
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TradBALoop.run cannot be captured into a graph: the per-iteration Adam / ExponentialLR scalars come "
                               "from the host's step count (a replay would repeat one iteration's scalars); call it eagerly")
        V, P, n = self.se3.shape[0], self.xyzs_all.shape[0], self.obs_point.shape[0]
        log = torch.empty(n_iters, 3, device=self.se3.device)
        _lib.check(lib.ls2fm_bundle_adjust_run(_lib.ptr(self.se3), _lib.ptr(self.xyzs_all), _lib.ptr(self.obs_uv), V, P, n, self._k_host,
                                               self.lrs[0], self.lrs[1], self.lrs[2], self.gamma, 1.0, 10.0, 10.0, _lib.ptr(self._m[0]),
                                               _lib.ptr(self._m[1]), _lib.ptr(self._m[2]), _lib.ptr(self._m[3]), self.it, n_iters,
                                               _lib.ptr(log), _lib.ptr(self.se3_entering_last), _lib.ptr(self.xyzs_entering_last),
                                               _lib.ptr(self._ws), _lib.stream_ptr()), "ls2fm_bundle_adjust_run")
        return log

    # ---- the same iteration as torch ops (BA_Trad.py:90-122)
    def _init_torch(self):
        self._r = torch.nn.Parameter(self.se3[:, :3].clone())
        self._t = torch.nn.Parameter(self.se3[:, 3:].clone())
        self._x = torch.nn.Parameter(self.xyzs_all)
        self._optim = torch.optim.Adam([dict(params=[self._r], lr=self.lrs[0]), dict(params=[self._t], lr=self.lrs[1]),
                                        dict(params=[self._x], lr=self.lrs[2])])
        self._sched = torch.optim.lr_scheduler.ExponentialLR(self._optim, gamma=self.gamma)

    def _run_torch(self, n_iters):
        rows = []
        for _ in range(n_iters):
            se3 = torch.cat([self._r, self._t], dim=1)
            self._optim.zero_grad()
            x = self._x[self.obs_point]
            in_cam = _cam.world2cam(x.unsqueeze(1), _cam.lie.se3_to_SE3(se3[self.obs_view]))
            uv = _cam.cam2img(in_cam, self.intrinsic.expand(in_cam.shape[0], 3, 3))
            uv = _to_pixels(uv).squeeze(1)
            err = (uv - self.obs_uv).norm(dim=-1)
            reproj = 0.5 * (2 * torch.log(1 + err ** 2 / 4)).mean() + 0.5 * err.mean()
            w = torch.where(reproj.detach() > 10, 10.0, 1.0)                     # BA_Trad.py:111-114 without the `.item()`
            self.se3_entering_last, self.xyzs_entering_last = se3.detach().clone(), self._x.detach().clone()
            (w * reproj).backward()
            self._optim.step()
            self._sched.step()
            rows.append(torch.stack([reproj.detach(), w.to(reproj.dtype), err.detach().mean()]))
        self.se3 = torch.cat([self._r, self._t], dim=1).detach()
        self.xyzs_all = self._x.detach()
        return torch.stack(rows)

    def run(self, n_iters=None):
        """the remaining iterations (or n_iters of them) -> logs: tensors [n] on the loop's device: reproj_error, w_reproj (the
        factor 10^w the loss was multiplied with), err_mean"""
        n_iters = self.max_iter - self.it if n_iters is None else int(n_iters)
        if n_iters < 1:
            raise ValueError(f"nothing to run: n_iters = {n_iters} (iteration {self.it} of {self.max_iter})")
        log = self._run_device(n_iters) if self.xyzs_all.is_cuda else self._run_torch(n_iters)
        self.it += n_iters
        self._err_last = log[-1, 2]
        return {k: log[:, q] for q, k in enumerate(self._keys)}

    def step(self):
        """one iteration -> its terms as 0-d tensors"""
        return {k: v[0] for k, v in self.run(1).items()}

    def poses_se3(self):
        return self.se3.detach()

    def written_back(self):
        if self._err_last is None:
            raise RuntimeError("TradBALoop.written_back: no iteration has run yet")
        return self.se3_entering_last, self.xyzs_entering_last, self._err_last


class LMBALoop:
    """Levenberg-Marquardt bundle adjustment with a Schur complement over explicit 3-D points and [R | t] poses (include/ls2fm.h
    states every rule: the pinhole residual in pixels, the loss `trivial` / `soft_l1` / `cauchy` as IRLS weights, per-block damping,
    the reduced camera system, the strict accept rule and the stopping rules; tests/ba_lm_restate.py repeats them in numpy).  All
    arithmetic is fp64.  The surface is TradBALoop's where that makes sense.

    views: `TrackedViews` or the mapper's view container (its `images` are not read; `poses` may be [V,6] se(3) parameters or
    [V,3,4]); cam_pick: the views to adjust, in this order (None: all; at most 128); constant_views: view indices (as in cam_pick)
    whose pose does not move.  A point with fewer than min_point_views observations among the picked views does not move either
    (its observations still constrain their cameras).  The intrinsic must be a pinhole K without skew.

    On the device `run()` is ONE call of ls2fm_bundle_adjust_lm_run (six launches per iteration, nothing read back; it can be
    captured into a graph, and a replay continues the loop); off the device the same iteration runs as torch fp64 ops (dense
    per-block tensors, torch.linalg.cholesky) so that the bookkeeping is testable anywhere.

    State after `run()` / `step()`: `poses` [V,3,4] and `xyzs_all` [M,3] (fp64; all points of the set, the ones no picked view
    observes unchanged), `poses_se3()`, `cost()` (0-d tensor), `stopped()` -> (reason, iterations), a host read; reason is one of
    "running", "gradient", "step", "lambda", "max_iter".

    camera: THE CAMERA BLOCK of include/ls2fm.h.  The [12] vector of ls2fm.undistort (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5,
    k6) shared by all views; the views' key points are then positions in the photographs AS TAKEN and `views.intrinsic` is not
    read.  refine: the words that move, names of CAMERA_WORDS; "f" moves fx with fy tied to it at the starting aspect fy / fx and
    excludes "fx" / "fy"; () only changes the residual model.  At most 126 views.  After `run()`, `camera` (fp64 [12] on the
    loop's device) holds the result.  One more launch per iteration (ls2fm_bundle_adjust_lm_run_camera).
    """
    LOSSES = ("trivial", "soft_l1", "cauchy")
    REASONS = ("running", "gradient", "step", "lambda")
    MAX_VIEWS = 128                      # LS2FM_BA_LM_MAX_VIEWS
    MAX_VIEWS_CAMERA = 126               # the camera's rows are two of the Cholesky's panels
    KEYS = ("cost", "cost_candidate", "lambda", "accepted", "grad_max", "step_max")
    CAMERA_WORDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")

    def __init__(self, views, cam_pick=None, constant_views=(), max_iter=50, loss="trivial", loss_scale=1.0, initial_lambda=1e-4,
                 grad_tol=1e-10, step_tol=1e-10, min_point_views=2, camera=None, refine=()):
        n_all = len(views.track_ids)
        self.cam_pick = list(range(n_all)) if cam_pick is None else [int(c) for c in cam_pick]
        if not self.cam_pick or any(c < 0 or c >= n_all for c in self.cam_pick) or len(set(self.cam_pick)) != len(self.cam_pick):
            raise ValueError(f"cam_pick {self.cam_pick} does not select distinct views of 0..{n_all - 1}")
        if len(self.cam_pick) > self.MAX_VIEWS:
            raise ValueError(f"LMBALoop: {len(self.cam_pick)} picked views; the dense reduced camera system serves at most {self.MAX_VIEWS}")
        refine = (refine,) if isinstance(refine, str) else tuple(refine)
        if camera is None and refine:
            raise ValueError("LMBALoop: refine names camera words but no camera is given")
        if camera is not None and len(self.cam_pick) > self.MAX_VIEWS_CAMERA:
            raise ValueError(f"LMBALoop: {len(self.cam_pick)} picked views; with a camera the reduced system serves at most "
                             f"{self.MAX_VIEWS_CAMERA}")
        unknown = [r for r in refine if r != "f" and r not in self.CAMERA_WORDS]
        if unknown:
            raise ValueError(f"LMBALoop: refine names {unknown}; the words are 'f' and {self.CAMERA_WORDS}")
        self.tie_focal = "f" in refine
        if self.tie_focal and ("fx" in refine or "fy" in refine):
            raise ValueError("LMBALoop: refine has 'f' (fy tied to fx) together with 'fx' / 'fy'")
        self.refine_mask = sum({1 << (0 if r == "f" else self.CAMERA_WORDS.index(r)) for r in refine})
        if loss not in self.LOSSES:
            raise ValueError(f"LMBALoop: loss {loss!r} is not one of {self.LOSSES}")
        if int(max_iter) < 1 or int(min_point_views) < 1:
            raise ValueError("LMBALoop: max_iter < 1 or min_point_views < 1")
        for name, v, positive in (("loss_scale", loss_scale, True), ("initial_lambda", initial_lambda, True), ("grad_tol", grad_tol, False),
                                  ("step_tol", step_tol, False)):
            if not (math.isfinite(v) and (v > 0 if positive else v >= 0)):
                raise ValueError(f"LMBALoop: {name} = {v!r} must be finite and {'positive' if positive else 'non-negative'}")
        self.max_iter, self.it = int(max_iter), 0
        self.loss, self.loss_scale, self.initial_lambda = loss, float(loss_scale), float(initial_lambda)
        self.grad_tol, self.step_tol, self.min_point_views = float(grad_tol), float(step_tol), int(min_point_views)
        self.views = views
        dev = views.xyzs.device
        self.camera = None
        if camera is not None:
            cam_host = torch.as_tensor(camera).detach().cpu().double()       # ONE host read when the loop is built: the aspect
            if tuple(cam_host.shape) != (len(self.CAMERA_WORDS),) or not bool(torch.isfinite(cam_host).all()) or \
                    float(cam_host[0]) == 0 or float(cam_host[1]) == 0:
                raise ValueError("LMBALoop: camera must be 12 finite words (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6), fx, fy != 0")
            self.aspect = float(cam_host[1]) / float(cam_host[0])
            self.camera = cam_host.to(dev).contiguous()
            self.k4 = None
        else:
            self._init_pinhole(views)
        p = views.poses.detach().to(dev).double()
        p = _cam.lie.se3_to_SE3(p) if p.shape[-1] == 6 else p
        self.poses = p[self.cam_pick].clone().contiguous()
        self.xyzs_all = views.xyzs.detach().double().clone().contiguous()
        self.obs_view, self.obs_point, obs_uv, self.view_start = TrackedViews.observations(views, dev, self.cam_pick)
        self.obs_uv = obs_uv.double().contiguous()
        if self.obs_point.numel() < 1 or any(views.track_ids[c].shape[0] < 1 for c in self.cam_pick):
            raise ValueError("LMBALoop: a picked view has no observation")
        const = {int(c) for c in constant_views}
        self.view_constant = torch.tensor([1 if c in const else 0 for c in self.cam_pick], dtype=torch.uint8).to(dev)
        self._stop_reason = None
        if self.xyzs_all.is_cuda:
            self._init_device()
        else:
            self._init_torch()

    def _init_pinhole(self, views):
        k_host = getattr(views, "host_intrinsic", None)
        k_host = (views.intrinsic.detach().cpu() if k_host is None else k_host).double()
        if tuple(k_host.shape) != (3, 3) or not bool(torch.isfinite(k_host).all()):
            raise ValueError(f"LMBALoop: the intrinsic must be a finite K [3, 3], got shape {tuple(k_host.shape)}")
        if k_host[0, 1] != 0 or k_host[1, 0] != 0:
            raise ValueError("LMBALoop: the intrinsic has skew; the solver serves a pinhole (fx, fy, cx, cy)")
        if k_host[2].tolist() != [0.0, 0.0, 1.0]:
            raise ValueError(f"LMBALoop: the intrinsic's last row is {k_host[2].tolist()}, not (0, 0, 1)")
        self.k4 = [float(k_host[0, 0]), float(k_host[1, 1]), float(k_host[0, 2]), float(k_host[1, 2])]

    # ---- device path
    def _init_device(self):
        lib = _lib.load()
        V, P, n, dev = self.poses.shape[0], self.xyzs_all.shape[0], self.obs_point.shape[0], self.poses.device
        if self.camera is not None:
            self._ws = _lib.workspace(lib.ls2fm_bundle_adjust_lm_camera_workspace_bytes(V, P, n),
                                      "ls2fm_bundle_adjust_lm_camera_workspace_bytes", dev)
        else:
            self._ws = _lib.workspace(lib.ls2fm_bundle_adjust_lm_workspace_bytes(V, P, n), "ls2fm_bundle_adjust_lm_workspace_bytes", dev)
        self._obs_point32 = self.obs_point.to(torch.int32).contiguous()
        status = lib.ls2fm_bundle_adjust_lm_prepare(_lib.ptr(self.view_start), V, _lib.ptr(self._obs_point32), n, P, _lib.ptr(self.view_constant),
                                                    self.min_point_views, _lib.ptr(self._ws), _lib.stream_ptr())
        if status == -1:                 # the sizes were checked above: what is left of "invalid argument" is the lists' content
            raise ValueError("LMBALoop: duplicate observations (a point observed twice by one view) or a point index outside the set")
        _lib.check(status, "ls2fm_bundle_adjust_lm_prepare")
        self._k_host = (ctypes.c_double * 4)(*self.k4) if self.camera is None else None
        self._opts = _lib.BALMOpts(self.LOSSES.index(self.loss), self.loss_scale, self.initial_lambda, self.grad_tol, self.step_tol,
                                   self.min_point_views)
        self._state = torch.zeros(8, dtype=torch.float64, device=dev)

    def _run_device(self, n_iters):
        lib = _lib.load()
        V, P, n = self.poses.shape[0], self.xyzs_all.shape[0], self.obs_point.shape[0]
        log = torch.empty(n_iters, 6, dtype=torch.float64, device=self.poses.device)
        if self.camera is not None:
            _lib.check(lib.ls2fm_bundle_adjust_lm_run_camera(_lib.ptr(self.poses), _lib.ptr(self.xyzs_all), _lib.ptr(self.camera),
                                                             _lib.ptr(self.obs_uv), V, P, n, self.refine_mask, int(self.tie_focal), self.aspect,
                                                             ctypes.byref(self._opts), n_iters, _lib.ptr(self._state), _lib.ptr(log),
                                                             _lib.ptr(self._ws), _lib.stream_ptr()), "ls2fm_bundle_adjust_lm_run_camera")
            return log
        _lib.check(lib.ls2fm_bundle_adjust_lm_run(_lib.ptr(self.poses), _lib.ptr(self.xyzs_all), _lib.ptr(self.obs_uv), V, P, n, self._k_host,
                                                  ctypes.byref(self._opts), n_iters, _lib.ptr(self._state), _lib.ptr(log), _lib.ptr(self._ws),
                                                  _lib.stream_ptr()), "ls2fm_bundle_adjust_lm_run")
        return log

    # ---- the same iteration as torch fp64 ops
    def _init_torch(self):
        key = self.obs_view * self.xyzs_all.shape[0] + self.obs_point
        if torch.unique(key).numel() != key.numel():
            raise ValueError("LMBALoop: duplicate observations (a point observed twice by one view)")
        if int(self.obs_point.min()) < 0 or int(self.obs_point.max()) >= self.xyzs_all.shape[0]:
            raise ValueError("LMBALoop: a point index outside the set")
        self._state = torch.zeros(8, dtype=torch.float64)
        self._point_const = torch.bincount(self.obs_point, minlength=self.xyzs_all.shape[0]) < self.min_point_views

    def _residuals(self, poses, X, camera=None):
        Pv = poses[self.obs_view]
        xc = (Pv[:, :, :3] @ X[self.obs_point][:, :, None])[..., 0] + Pv[:, :, 3]
        if camera is not None:
            xd, yd, _ = _distort_torch(camera.unbind(0), xc[:, 0] / xc[:, 2], xc[:, 1] / xc[:, 2])
            r = torch.stack([camera[0] * xd + camera[2] - self.obs_uv[:, 0], camera[1] * yd + camera[3] - self.obs_uv[:, 1]], dim=1)
        else:
            fx, fy, cx, cy = self.k4
            r = torch.stack([fx * xc[:, 0] / xc[:, 2] + cx - self.obs_uv[:, 0], fy * xc[:, 1] / xc[:, 2] + cy - self.obs_uv[:, 1]], dim=1)
        s, c2 = (r * r).sum(1), self.loss_scale ** 2
        if self.loss == "trivial":
            rho, w = s, torch.ones_like(s)
        elif self.loss == "soft_l1":
            q = torch.sqrt(1.0 + s / c2)
            rho, w = 2.0 * c2 * (q - 1.0), 1.0 / q
        else:
            rho, w = c2 * torch.log1p(s / c2), 1.0 / (1.0 + s / c2)
        return xc, r, rho, w

    @staticmethod
    def _damp(B, lam):
        d = torch.diagonal(B, dim1=-2, dim2=-1)
        return B + torch.diag_embed(lam * torch.maximum(d, 1e-12 * d.max(dim=-1, keepdim=True).values))

    @staticmethod
    def _pose_update(P, d):
        w = d[:, :3]
        th2 = (w * w).sum(1)
        big = th2 >= 1e-30
        th = torch.sqrt(torch.where(big, th2, torch.ones_like(th2)))
        A = torch.where(big, torch.sin(th) / th, torch.ones_like(th))
        B = torch.where(big, (1.0 - torch.cos(th)) / torch.where(big, th2, torch.ones_like(th2)), torch.zeros_like(th))
        K = torch.zeros(P.shape[0], 3, 3, dtype=P.dtype)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
        E = torch.eye(3, dtype=P.dtype) + A[:, None, None] * K + B[:, None, None] * (K @ K)
        C = E @ P
        C[:, :, 3] += d[:, 3:]
        return C

    @staticmethod
    def _camera_jacobians(cam, xc):
        """THE CAMERA BLOCK's Jacobians at camera points xc [n, 3]: J_proj = diag(fx, fy) J_dist [[1/z, 0, -x/z], [0, 1/z, -y/z]]
        [n, 2, 3] and J_k [n, 2, 12], all twelve columns (the caller masks and ties them)"""
        c = cam.unbind(0)
        z = xc[:, 2]
        xn, yn, iz = xc[:, 0] / z, xc[:, 1] / z, 1.0 / z
        xd, yd, shared = _distort_torch(c, xn, yn)
        ja, jb, jc_, jd = _jacobian_torch(c, shared, xn, yn)
        Jproj = torch.zeros(xc.shape[0], 2, 3, dtype=torch.float64)
        Jproj[:, 0, 0], Jproj[:, 0, 1], Jproj[:, 0, 2] = c[0] * (ja * iz), c[0] * (jb * iz), -(c[0] * ((ja * xn + jb * yn) * iz))
        Jproj[:, 1, 0], Jproj[:, 1, 1], Jproj[:, 1, 2] = c[1] * (jc_ * iz), c[1] * (jd * iz), -(c[1] * ((jc_ * xn + jd * yn) * iz))
        ku, kv = _jacobian_k_torch(c, shared, xn, yn, xd, yd)
        return Jproj, torch.stack([torch.stack(ku, dim=1), torch.stack(kv, dim=1)], dim=1)

    def _iterate_torch(self):
        st = self._state
        lam = float(st[0]) if float(st[0]) > 0 else self.initial_lambda
        if float(st[1]) != 0:
            return torch.tensor([float(st[3]), float(st[3]), lam, -1.0, 0.0, 0.0], dtype=torch.float64)
        V, P, ov, op = self.poses.shape[0], self.xyzs_all.shape[0], self.obs_view, self.obs_point
        vconst, pconst = self.view_constant.bool(), self._point_const
        cam = self.camera
        xc, r, rho, w = self._residuals(self.poses, self.xyzs_all, cam)
        n = xc.shape[0]
        x, y, z = xc[:, 0], xc[:, 1], xc[:, 2]
        Jproj = torch.zeros(n, 2, 3, dtype=torch.float64)
        if cam is not None:                    # THE CAMERA BLOCK: J_proj through the rule's Jacobian, and J_k masked and tied
            kmask = torch.tensor([bool(self.refine_mask >> k & 1) for k in range(12)])
            Jproj, Jk = self._camera_jacobians(cam, xc)
            if self.tie_focal:
                Jk[:, :, 0] = Jk[:, :, 0] + self.aspect * Jk[:, :, 1]
            Jk[:, :, ~kmask] = 0.0
        else:
            fx, fy = self.k4[0], self.k4[1]
            Jproj[:, 0, 0], Jproj[:, 0, 2], Jproj[:, 1, 1], Jproj[:, 1, 2] = fx / z, -fx * x / (z * z), fy / z, -fy * y / (z * z)
        skew = torch.zeros(n, 3, 3, dtype=torch.float64)
        skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 0], skew[:, 1, 2], skew[:, 2, 0], skew[:, 2, 1] = -z, y, z, -x, -y, x
        Jc = torch.cat([-(Jproj @ skew), Jproj], dim=2)
        Jp = Jproj @ self.poses[ov][:, :, :3]
        Jc[vconst[ov]] = 0.0
        Jp[pconst[op]] = 0.0
        U = torch.zeros(V, 6, 6, dtype=torch.float64).index_add_(0, ov, w[:, None, None] * (Jc.transpose(1, 2) @ Jc))
        gc = torch.zeros(V, 6, dtype=torch.float64).index_add_(0, ov, w[:, None] * (Jc.transpose(1, 2) @ r[:, :, None])[..., 0])
        Vp = torch.zeros(P, 3, 3, dtype=torch.float64).index_add_(0, op, w[:, None, None] * (Jp.transpose(1, 2) @ Jp))
        gp = torch.zeros(P, 3, dtype=torch.float64).index_add_(0, op, w[:, None] * (Jp.transpose(1, 2) @ r[:, :, None])[..., 0])
        W = w[:, None, None] * (Jc.transpose(1, 2) @ Jp)
        cost = 0.5 * float(rho.sum())
        free = ~pconst
        gmax = max(float(gc.abs().max()), float(gp[free].abs().max()) if bool(free.any()) else 0.0)
        if cam is not None:
            G = torch.einsum("n,nki,nkj->ij", w, Jk, Jk)
            gk = torch.einsum("n,nki,nk->i", w, Jk, r)
            Hd = torch.zeros(V, 6, 12, dtype=torch.float64).index_add_(0, ov, w[:, None, None] * (Jc.transpose(1, 2) @ Jk)).reshape(6 * V, 12)
            Yd = torch.zeros(P, 12, 3, dtype=torch.float64).index_add_(0, op, w[:, None, None] * (Jk.transpose(1, 2) @ Jp))
            if bool(kmask.any()):
                gmax = max(gmax, float(gk[kmask].abs().max()))
        pmax = max(float(self.poses[:, :, 3].abs().max()), float(self.xyzs_all[torch.unique(op)].abs().max()))
        cand, dmax, acc, done, reason, new_lam = float("nan"), 0.0, 0.0, 0.0, 0.0, lam
        if gmax <= self.grad_tol:
            done, reason, cand = 1.0, 1.0, cost
        else:
            step = None
            Vs, Us = self._damp(Vp, lam), self._damp(U, lam)
            finite = torch.isfinite(Vs).all() and torch.isfinite(Us).all() and torch.isfinite(W).all()
            if cam is not None:
                finite = finite and torch.isfinite(G).all() and torch.isfinite(Hd).all() and torch.isfinite(Yd).all()
            if bool(finite):
                eye3 = torch.eye(3, dtype=torch.float64).expand(P, 3, 3)
                L, info = torch.linalg.cholesky_ex(torch.where(free[:, None, None], Vs, eye3))
                if int(info.abs().max()) == 0:
                    Vinv = torch.where(free[:, None, None], torch.cholesky_inverse(L), torch.zeros_like(Vs))
                    S = torch.block_diag(*[torch.eye(6, dtype=torch.float64) if bool(vconst[v]) else Us[v] for v in range(V)])
                    b = torch.where(vconst[:, None], torch.zeros_like(gc), -gc).reshape(-1)
                    Wd = torch.zeros(V, 6, P, 3, dtype=torch.float64)          # dense [6 V, 3 P]: the CPU path is test-scale
                    Wd[ov, :, op, :] = W
                    Wd = Wd.reshape(6 * V, P, 3)
                    if cam is not None:    # the border: 12 more rows, the camera block damped as ONE block
                        S = torch.block_diag(S, self._damp(G, lam))
                        S[:6 * V, 6 * V:], S[6 * V:, :6 * V] = Hd, Hd.T
                        b = torch.cat([b, -gk])
                        Wd = torch.cat([Wd, Yd.transpose(0, 1)])
                    Y = torch.einsum("apk,pkl->apl", Wd, Vinv)
                    S = S - torch.einsum("apk,bpk->ab", Y, Wd)
                    b = b + torch.einsum("apk,pk->a", Y, gp)
                    if cam is not None:    # an unrefined word: the identity's row and column, right-hand side 0
                        off = 6 * V + torch.nonzero(~kmask)[:, 0]
                        S[off, :], S[:, off], b[off] = 0.0, 0.0, 0.0
                        S[off, off] = 1.0
                    Ls, info = torch.linalg.cholesky_ex(S)
                    if int(info) == 0:
                        dc = torch.cholesky_solve(b[:, None], Ls)[:, 0]
                        dp = -(Vinv @ (gp + torch.einsum("apk,a->pk", Wd, dc))[:, :, None])[..., 0]
                        step = (dc[:6 * V].reshape(V, 6), dp, dc[6 * V:])
            if step is None:
                new_lam = lam * 10.0
            else:
                dc, dp, dk = step
                cp = torch.where(vconst[:, None, None], self.poses, self._pose_update(self.poses, dc))
                cx = self.xyzs_all + dp
                ck = None
                if cam is not None:
                    ck = torch.where(kmask, cam + dk, cam)
                    if self.tie_focal:
                        ck[1] = self.aspect * ck[0]
                cand = 0.5 * float(self._residuals(cp, cx, ck)[2].sum())
                dmax = float(torch.fmax(dc.abs().max(), dp.abs().max()))
                if cam is not None and bool(kmask.any()):
                    dmax = max(dmax, float((dk.abs() / (1.0 + cam.abs()))[kmask].max()))
                if cand < cost:
                    acc, new_lam = 1.0, max(lam * 0.1, 1e-16)
                    self.poses, self.xyzs_all, self.camera = cp.contiguous(), cx.contiguous(), ck
                    if dmax <= self.step_tol * (1.0 + pmax):
                        done, reason = 1.0, 2.0
                else:
                    new_lam = lam * 10.0
        if not done and new_lam > 1e32:
            done, reason = 1.0, 3.0
        self._state = torch.tensor([new_lam, done, float(st[2]) + 1.0, cand if acc else cost, reason, gmax, dmax, acc], dtype=torch.float64)
        return torch.tensor([cost, cand, lam, acc, gmax, dmax], dtype=torch.float64)

    def _run_torch(self, n_iters):
        return torch.stack([self._iterate_torch() for _ in range(n_iters)])

    # ---- surface
    def run(self, n_iters=None):
        """the remaining iterations (or n_iters of them) -> the log's columns as tensors [n] on the loop's device: cost (entering),
        cost_candidate, lambda, accepted (1 / 0; -1 for an iteration after the stop), grad_max, step_max"""
        n_iters = self.max_iter - self.it if n_iters is None else int(n_iters)
        if n_iters < 1:
            raise ValueError(f"nothing to run: n_iters = {n_iters} (iteration {self.it} of {self.max_iter})")
        log = self._run_device(n_iters) if self.xyzs_all.is_cuda else self._run_torch(n_iters)
        self.it += n_iters
        return {k: log[:, q] for q, k in enumerate(self.KEYS)}

    def step(self):
        """one iteration -> its log entries as 0-d tensors"""
        return {k: v[0] for k, v in self.run(1).items()}

    def poses_se3(self):
        return _cam.lie.SE3_to_se3(self.poses)

    def cost(self):
        """the current cost, 1/2 sum rho (0-d tensor on the loop's device; before the first iteration: not yet evaluated, 0)"""
        return self._state[3]

    def mean_error(self):
        """mean pixel error |r| over the loop's observations at the current state (0-d tensor, torch ops, nothing read back)"""
        Pv = self.poses[self.obs_view]
        xc = (Pv[:, :, :3] @ self.xyzs_all[self.obs_point][:, :, None])[..., 0] + Pv[:, :, 3]
        if self.camera is not None:
            xd, yd, _ = _distort_torch(self.camera.unbind(0), xc[:, 0] / xc[:, 2], xc[:, 1] / xc[:, 2])
            u = self.camera[0] * xd + self.camera[2] - self.obs_uv[:, 0]
            v = self.camera[1] * yd + self.camera[3] - self.obs_uv[:, 1]
            return torch.sqrt(u * u + v * v).mean()
        u = self.k4[0] * xc[:, 0] / xc[:, 2] + self.k4[2] - self.obs_uv[:, 0]
        v = self.k4[1] * xc[:, 1] / xc[:, 2] + self.k4[3] - self.obs_uv[:, 1]
        return torch.sqrt(u * u + v * v).mean()

    def stopped(self):
        """(reason, iterations taken before the stop or so far) -- a host read"""
        st = self._state.tolist()
        reason = self.REASONS[int(st[4])]
        if reason == "running" and self.it >= self.max_iter:
            reason = "max_iter"
        return reason, int(st[2])
