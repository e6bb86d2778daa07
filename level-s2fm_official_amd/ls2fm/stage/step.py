"""The optimisation step the reference's stage drivers share:

    Initializer.run        pipelines/Initialization.py:149-179      BA.run_ba (mode != "sfm")   pipelines/BA.py:117-182
    Refine.run             pipelines/rendering_refine.py:78-96

each iteration of which is  `CameraSet.render` (pipelines/Camera.py:448-538: Renderer.forward, SDF.sphere_tracing, mask_bg /
mask_finish, rgb_loss / DC_loss / PSNR)  ->  compute_loss / summarize_loss (eikonal over mask_bg, 10^w weighted sum:
BA.py:186-218)  ->  loss.all.backward()  ->  Adam.step()  ->  ExponentialLR.step().

`surface_losses` is the point side of a BA iteration (BA.py:117-131, compute_loss "sfm" branch) on the fused point queries;
`render_losses` is that render-and-loss part for rays that are already picked (ray picking, poses, key points, COLMAP
bookkeeping are the drivers' camera-side logic: SURVEY section 2, out of scope); `RenderStage` adds the update and, with
`capture=True`, records the WHOLE step -- tracing kernel, point-query node of the traced depth, fused render with the loss
head inside, backward, Adam with the learning-rate schedule on the device -- into one hipGraph: a step is then a single
graph launch with no host synchronisation (the reference syncs at `mask_finish.sum() > 0`, at the tracing loop's
`.sum()` per trip and at `loss.item()`).
"""
from __future__ import annotations

import torch

from .. import dist as _dist
from .. import fused as _fused
from ..graph import CapturedStep
from ..losses import RenderLossHead, psnr
from ..optim import FusedAdam


def _weight_lookup(weights):
    """-> `key -> the exponent stored under it, or None`, for a dict or an options namespace of loss weights (or None)"""
    w = weights or {}
    return (lambda k: w.get(k)) if isinstance(w, dict) else (lambda k: getattr(w, k, None))


def _weight_factor(exponent):
    """the factor of a loss term whose weight the reference keeps as an exponent (summarize_loss, BA.py:204-218): 10^w, and 0 for
    a term that has none"""
    return 0.0 if exponent is None else 10.0 ** float(exponent)


_TRACE_STREAMS = {}


def _trace_stream(device, slot=0):
    """the stream(s) sphere tracings are launched on beside the render's forward: slot 0 the render rays', slots 1.. the key-point
    tracings of a loop's extra terms (latency-bound kernels of a few workgroups each: they overlap each other almost for free).
    None (= the current stream) inside a hipGraph capture under torch.distributed: the tracing max-reduces its trip count over the
    ranks on the stream it runs on, and a side-stream branch that forks again into RCCL's own stream is the depth-three fork tree
    that takes a capture down on ROCm 7.2 (csrc/streams.hip)."""
    if _dist.is_distributed() and torch.cuda.is_current_stream_capturing():
        return None
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if (idx, slot) not in _TRACE_STREAMS:
        _TRACE_STREAMS[(idx, slot)] = torch.cuda.Stream(device=idx)
    return _TRACE_STREAMS[(idx, slot)]


class _EarlyTrace:
    """A key-point sphere tracing launched AHEAD of the render on a stream of its own (the render does not depend on it), its
    results picked up where the loss term is formed.  Holds the call's autograd-node record until the next launch: that record
    owns every tensor the other stream touches (no record_stream under hipGraph capture, see ls2fm.fused.TracedDepthNode)."""

    def __init__(self, sdf_field, slot):
        self.sdf, self.slot = sdf_field, slot
        self.out = self.ready = self.node = None

    def launch(self, center, ray):
        side = _trace_stream(center.device, self.slot)
        self.out = self.sdf.sphere_tracing(center, ray, self.sdf, static_trips=True, launch_stream=side)
        self.node = getattr(self.sdf, "last_trace_node", None)
        self.ready = torch.cuda.Event()
        self.ready.record(side)

    def take(self):
        """-> the tracing's outputs (joined into the current stream), or None when nothing was launched"""
        if self.out is None:
            return None
        torch.cuda.current_stream(self.out[0].device).wait_event(self.ready)
        out, self.out = self.out, None
        return out

    def take_or_trace(self, center, ray, static_trips):
        """-> the early tracing's outputs when one was launched, else the same tracing done now, on the current stream"""
        early = self.take()
        return early if early is not None else self.sdf.sphere_tracing(center, ray, self.sdf, static_trips=static_trips)


def render_losses(opt, renderer, sdf_field, rad_field, head, centers, rays, rgbs_gt, static_trips=False, eikonal_over="bg"):
    """CameraSet.render(mode="train") after the ray pick + the render-side terms of compute_loss: -> the reference's `ret`
    keys (rgb, sdfs_volume, normals, depth_mlp, normal_mlp, mask_bg, rgb_loss, DC_loss, PSNR, tracing_loss) plus
    eikonal_loss (over mask_bg, BA.py:193-194), mse and `loss_all` (the head's 10^w weighted sum).
    centers, rays [B,R,3]; rgbs_gt [B,R,3].  The tracing runs first (it is independent of the render): its masks and depth
    are then inputs of the loss head that runs INSIDE the fused render (Renderer.forward_with_loss).
    eikonal_over: "bg" = over the rays of mask_bg (BA.py:193-194, Initialization.py:257-258), "all" = over every normal
    (rendering_refine.py:101-102)."""
    b, r = centers.shape[:2]
    ready = None
    if static_trips:
        # one fused node forms the traced depth AND the two masks of Camera.py:515-516 (uint8, as the loss head takes them):
        # as torch ops these lines were ~25 launch-bound elementwise kernels of the captured step.
        # The tracing (one latency-bound kernel of few workgroups, then the track evaluation) is independent of the render up to
        # the loss head inside shade_fwd: it runs on its own stream BESIDE the render's gather pass (L2-bound), and the forward
        # waits for its event only in front of shade_fwd.  (The autograd node itself belongs to the current stream -- its
        # backward runs there --; only the forward's kernels are launched on the other one.)
        side = _trace_stream(centers.device)
        d_points, sdf_last, _, _ = sdf_field.sphere_tracing(centers.reshape(1, -1, 3), rays.reshape(1, -1, 3), sdf_field, iter=0,
                                                            static_trips=True, rgbs_gt=rgbs_gt.reshape(-1, 3), launch_stream=side)
        mask_bg8, mask_dc8 = sdf_field.last_masks
        ready = torch.cuda.Event()
        ready.record(side)
        mask_bg, mask_finish = mask_bg8.view(b, r), mask_dc8.view(b, r)
        # the render's loss head evaluates mask_bg itself from the colours ("gt"): only the traced depth and mask_finish come out
        # of the tracing, and those are read by the loss REDUCTION behind the shading kernel -- the render waits for `ready` there
        head_bg = "gt"
    else:
        d_points, sdf_last, _, mask_finish = sdf_field.sphere_tracing(centers.reshape(1, -1, 3), rays.reshape(1, -1, 3), sdf_field,
                                                                     iter=0)
        gray = rgbs_gt.mean(dim=-1)
        mask_bg = (gray < 0.95) & (gray > 0.05)                               # Camera.py:515
        mask_finish = mask_finish.view(b, r) & mask_bg                        # Camera.py:516
        head_bg = mask_bg
    ret, losses = renderer.forward_with_loss(opt, centers, rays, sdf_field, rad_field, head, rgbs_gt, d_points=d_points.view(b, r),
                                             mask_finish=mask_finish, mask_eik=head_bg if eikonal_over == "bg" else None,
                                             mask_bg=head_bg, inputs_ready=ready,
                                             depth_node=getattr(sdf_field, "last_trace_node", None) if static_trips else None)
    if ready is not None:
        torch.cuda.current_stream(centers.device).wait_event(ready)       # join: later readers of the traced outputs, the backward
    if static_trips:
        mask_bg, mask_finish = mask_bg.view(torch.bool), mask_finish.view(torch.bool)      # 0 / 1 bytes: same storage, no kernel
    ret = dict(ret)
    ret.update(tracing_loss=0, mask_bg=mask_bg, mask_finish=mask_finish, d_points=d_points.view(b, r, 1),
               sdf_tracks=sdf_last.view(b, r, 1), rgb_loss=losses["rgb_loss"], DC_loss=losses["DC_loss"],
               eikonal_loss=losses["eikonal_loss"], mse=losses["mse"], PSNR=losses["PSNR"] if "PSNR" in losses else psnr(losses["mse"]),
               loss_all=losses["all"])
    return ret


def _point_side(sdf_field, xyzs):
    """BA.py:119-122: the tracked points projected onto the surface and re-evaluated there -> (xyzs_new, normals_value, sdfs [n,1]);
    two fused point-query nodes, issued HERE (their place against the render's node decides which backward owns the gradient
    buffer, ls2fm.fused.pass_gradient_sharing)"""
    xyzs_new, normals_value = sdf_field.get_surface_pts(xyzs)
    return xyzs_new, normals_value, sdf_field.infer_sdf(xyzs_new, mode="ret_sdf").view(-1, 1)


def surface_losses(opt, sdf_field, xyzs, res=None):
    """The POINT side of a bundle-adjustment iteration (pipelines/BA.py:117-131) and the "sfm" branch of BA.compute_loss
    (BA.py:199-202): tracked 3-D points are projected onto the surface, `xyzs_new, normals_value = get_surface_pts(xyzs)`,
    re-evaluated, `sdfs = infer_sdf(xyzs_new)`, and give  sdf_surf = L1(sdfs, 0),  eikonal_loss = L1(normals_value, 1)
    and  mask_surf = |sdfs| < 2 * (extent / 10 / opt.Res).  Every field evaluation is one fused point-query node
    (ls2fm_sdf_eval forward, ls2fm_sdf_points_bwd backward with the analytic double backward of the normal); the
    re-projection term the drivers add on top of `xyzs_new` is camera-side logic (world2cam / cam2img), out of scope."""
    xyzs_new, normals_value, sdfs = _point_side(sdf_field, xyzs)
    res = int(opt.Res) if res is None else int(res)
    sdf_threshold = (sdf_field.bound_max.reshape(-1)[0] - sdf_field.bound_min.reshape(-1)[0]) / 10 / res
    return dict(xyzs_new=xyzs_new, gradients=normals_value, sdfs=sdfs, mask_surf=sdfs.abs() < 2 * sdf_threshold,
                sdf_surf=sdfs.abs().mean(), eikonal_loss=(normals_value - 1).abs().mean())


class RenderStage:
    """render -> losses -> backward -> Adam + ExponentialLR over the two fields' parameters (and any extra ones, e.g. poses).

        stage = RenderStage(opt, renderer, sdf, rad, weights=opt.loss_weight.ba, lr=1e-2, lr_end=1e-4, max_iter=500)
        for it in range(500): ret = stage.step(centers, rays, rgbs_gt)

    capture=True: the first `step` call records the whole step into a hipGraph at the given batch shape; later calls copy
    the new rays into the captured input buffers and replay it (shapes must not change; no `.item()` anywhere).

    extra_loss: a callable `ret -> scalar tensor` evaluated inside the step and ADDED to `loss_all` before the backward -- the
    terms a driver forms outside the render (BA.run_ba's key-point re-projection error and, through `surface_losses`, its
    sdf_surf term: BA.py:119-147, 186-202), already weighted.  With capture=True it is recorded with the step: it must read
    its inputs from tensors that are updated in place and must not synchronise."""

    def __init__(self, opt, renderer, sdf_field, rad_field, weights=None, lr=1e-2, lr_end=1e-4, max_iter=1000, betas=(0.9, 0.999),
                 eps=1e-8, extra_params=(), capture=False, extra_loss=None, lr_color=None, eikonal_over="bg", reducer=None,
                 sharded=False, async_gather=False, extra_prepare=None, input_fn=None, share_gradients=False, shard_groups=1,
                 shard_views=False):
        """lr / lr_color: the reference's two field groups (`[{sdf_func.parameters(), lr_sdf}, {color_func.parameters(),
        lr_color}]`, BA.py:79-83; lr_color=None: one rate); extra_params: tensors (one more group at `lr`) or
        `{"params": [...], "lr": x}` dicts (the pose groups of BA.py:60-75).  ONE ExponentialLR factor for all groups,
        (lr_end / lr) ** (1 / max_iter), as the reference's scheduler (BA.py:87-88).
        reducer: an `ls2fm.dist.GradAllReducer` over the same parameters, called between backward and the update -- required
        when a process group is up (the fused loss head then divides by GLOBAL counts: without the reduction every rank would
        apply 1/world of its local gradient and the replicas would drift apart) -- or sharded=True: the update is
        `ls2fm.dist.ShardedAdam` (reduce-scatter of the flat gradient buffer, Adam on this rank's 1/world of the parameters,
        all-gather of the updated shards; async_gather: the all-gather runs on the communication stream until the next step's
        first parameter read; shard_groups >= 2: the exchange is pipelined by level groups of the two tables, `ShardedAdam`).
        Fields only: pose groups (extra_params) take the all-reduce form.
        reducer="auto": a GradAllReducer over this stage's parameters when a process group is up (else none).
        shard_views=True (with a process group of W ranks): the step's [B,R,3] batch is the GLOBAL one, identical on every rank,
        and rank r renders views r, r + W, ... of it (B % W == 0) -- BASELINE.json configs[3]: a BA step with the rays of 8
        registered views sharded over 8 GPUs; the loss head divides by global counts, the all-reduce sums the shards' gradients.
        `extra_loss` (terms formed outside the render: point side, re-projection, tracing consistency) is evaluated on every rank
        over the same inputs and enters the backward with weight 1 / W, so that the summed gradient is the single-process one;
        the returned `loss_all` is the global value on every rank.  capture=True under torch.distributed needs the RCCL ("nccl")
        backend: the step's collectives -- loss counts, trip count, gradient all-reduce -- are recorded into the hipGraph."""
        self.opt, self.renderer, self.sdf, self.rad = opt, renderer, sdf_field, rad_field
        dev = next(sdf_field.parameters()).device
        get = _weight_lookup(weights)
        self.head = RenderLossHead(dev, w_rgb=get("rgb"), w_eikonal=get("eikonal_loss"), w_dc=get("DC_Loss"))
        groups = [dict(params=[p for p in sdf_field.parameters() if p.requires_grad], lr=lr),
                  dict(params=[p for p in rad_field.parameters() if p.requires_grad], lr=lr if lr_color is None else lr_color)]
        loose = [p for p in extra_params if not isinstance(p, dict)]
        if loose:
            groups.append(dict(params=[p for p in loose if p.requires_grad], lr=lr))
        groups += [dict(g) for g in extra_params if isinstance(g, dict)]
        groups = [g for g in groups if g["params"]]
        self.params = [p for g in groups for p in g["params"]]
        self.gamma = (lr_end / lr) ** (1.0 / max_iter)                        # BA.py:87-88
        self.sharded = bool(sharded)
        if self.sharded:
            if len(groups) > 2 or capture:
                raise NotImplementedError("ls2fm.stage.RenderStage(sharded=True): the two field groups only, eager steps only "
                                          "(pose groups and captured steps take the all-reduce form: reducer=\"auto\")")
            self.optim = _dist.ShardedAdam.for_fields(sdf_field, rad_field, lr=lr, lr_color=lr_color, betas=betas, eps=eps,
                                                      scheduled_gamma=self.gamma, async_gather=async_gather, n_groups=shard_groups,
                                                      in_backward=False)       # (a traced-depth node rides in every step)
            self.params = list(self.optim.params)
        else:
            self.optim = FusedAdam(groups, lr=lr, betas=betas, eps=eps, scheduled_gamma=self.gamma)
        self.capture = capture
        self.extra_loss = extra_loss
        # called at the start of a step, before the render is enqueued: work of the extra terms that does not depend on the
        # render (their key-point tracings) starts here, on streams of its own, and runs beside the render's forward
        self.extra_prepare = extra_prepare
        # `() -> (centers, rays, rgbs_gt)` evaluated INSIDE the step (and inside its capture): a loop's ray pick and pose algebra
        # from device tensors it updates in place -- `step()` then takes no arguments and a captured iteration has no eager
        # preamble (the loops' ~50 launch-bound kernels of camera arithmetic per iteration were half of their time)
        self.input_fn = input_fn
        # one gradient buffer per backward pass (ls2fm.fused.pass_gradient_sharing): only for a caller whose extra terms issue
        # ALL their field queries in `extra_prepare`, i.e. ahead of the render (the loops below)
        self.share_gradients = bool(share_gradients)
        self.eikonal_over = eikonal_over
        if isinstance(reducer, str):
            if reducer != "auto":
                raise ValueError(f"ls2fm.stage.RenderStage: reducer={reducer!r}")
            reducer = _dist.GradAllReducer(self.params) if (_dist.is_distributed() and not self.sharded) else None
        self.reducer = reducer
        self.shard_views = bool(shard_views)
        self._graph = None
        self._table_versions = None
        self._one = torch.ones((), device=dev)

    def _eager(self, centers, rays, rgbs_gt, static_trips):
        if self.sharded:
            self.optim.wait_params()               # the previous step's all-gather (async_gather) before anything reads a parameter
        if _dist.is_distributed() and self.reducer is None and not self.sharded:
            raise RuntimeError("ls2fm.stage.RenderStage under torch.distributed needs reducer=GradAllReducer(stage.params): the loss "
                               "head normalises by global counts, the gradients must be summed over the ranks before the update")
        for p in self.params:
            p.grad = None
        world = 1
        if self.shard_views and _dist.is_distributed():
            import torch.distributed as tdist
            world, rank = tdist.get_world_size(), tdist.get_rank()
            if centers.shape[0] % world:
                raise RuntimeError(f"ls2fm.stage.RenderStage(shard_views=True): {centers.shape[0]} views over {world} ranks")
            if world > 1:                  # views rank, rank + world, ...: strided views of the global batch, made contiguous
                centers, rays, rgbs_gt = (t[rank::world].contiguous() for t in (centers, rays, rgbs_gt))
        if self.extra_prepare is not None and static_trips:
            self.extra_prepare()
        ret = render_losses(self.opt, self.renderer, self.sdf, self.rad, self.head, centers, rays, rgbs_gt, static_trips=static_trips,
                            eikonal_over=self.eikonal_over)
        loss_bwd = ret["loss_all"]
        if self.extra_loss is not None:
            ret["loss_extra"] = self.extra_loss(ret)
            # (replicated on every rank of a view-sharded step: 1 / world of it per rank in the backward, the whole in the log)
            total = ret["loss_all"] + ret["loss_extra"]
            loss_bwd = total if world == 1 else ret["loss_all"] + ret["loss_extra"] * (1.0 / world)
            ret["loss_all"] = total
        with _fused.pass_gradient_sharing(self.share_gradients and static_trips and self.extra_prepare is not None):
            loss_bwd.backward(gradient=self._one)
        if self.reducer is not None:
            self.reducer.all_reduce()
        self.optim.step()
        return ret

    def step(self, centers=None, rays=None, rgbs_gt=None):
        if centers is None:
            if self.input_fn is None:
                raise TypeError("ls2fm.stage.RenderStage.step(): centers, rays, rgbs_gt -- or construct the stage with input_fn")
            if not self.capture:
                centers, rays, rgbs_gt = self.input_fn()
            elif self._graph is None:
                return self._capture(lambda: self._eager(*self.input_fn(), static_trips=True))
            else:
                return self._replay()
        if not self.capture:
            # the static form (trip count stays on the device, traced depth + masks as one fused node) whenever the fused tracing
            # kernel serves this field: no host round trip per step, ~40 fewer launches; else the reference-shaped form
            static = _fused.available(self.sdf, centers)
            return self._eager(centers, rays, rgbs_gt, static_trips=static)
        if self._graph is None:
            self._in = (centers.detach().clone(), rays.detach().clone(), rgbs_gt.detach().clone())
            return self._capture(lambda: self._eager(*self._in, static_trips=True))
        srcs = (centers, rays, rgbs_gt)
        for dst, src in zip(self._in, srcs):
            if dst.shape != src.shape:
                raise RuntimeError("ls2fm.stage.RenderStage(capture=True): the batch shape is fixed by the first step")
        torch._foreach_copy_(list(self._in), [s.detach() for s in srcs])         # one launch for the three inputs
        return self._replay()

    def _replay(self):
        """one replay of the captured step.  The graph reads the entry-interleaved table copy WITHOUT checking it (inside a capture
        nothing can be checked): a foreign writer of a table since the last replay -- a checkpoint load, `load_state_dict`, another
        optimizer -- is detected here, on the host, through the tables' version counters, and costs one rebuild of the copy."""
        tabs = _fused.table_params(self.sdf, self.rad)
        if tabs is not None and [t._version for t in tabs] != self._table_versions:
            _fused.sync_mirror(self.sdf, self.rad)
        out = self._graph.replay()
        self.optim.replayed(1)
        self._table_versions = None if tabs is None else [t._version for t in tabs]
        return out

    # ---- checkpoint / resume (utils/util.py:198-259 stores `optim_*` / `sched_*` state dicts next to the fields')
    def state_dict(self):
        """the optimizer's state in torch's layout (per-parameter `step, exp_avg, exp_avg_sq`, per-group `lr`): with the device-
        resident schedule that IS the scheduler state -- ExponentialLR's only state is the current rate"""
        if self.sharded:
            raise NotImplementedError("ls2fm.stage.RenderStage.state_dict: use ShardedAdam.state_dict() (per-rank shards)")
        return {"optim": self.optim.state_dict(), "gamma": self.gamma}

    def load_state_dict(self, state):
        """resume: moments, step counts and rates are copied INTO the tensors this stage (and a captured graph of it) already
        owns; the next step -- eager or a replay -- continues the saved trajectory.  Load the fields' state dicts first."""
        self.optim.load_state_dict(state["optim"])
        self._table_versions = None            # the next replay re-checks the interleaved copy against the (reloaded) tables

    def _capture(self, fn):
        if _dist.is_distributed():
            import torch.distributed as tdist
            if tdist.get_backend() != "nccl" or self.sharded:
                raise NotImplementedError("ls2fm.stage.RenderStage(capture=True) under torch.distributed needs the RCCL (\"nccl\") "
                                          "backend and the all-reduce form (reducer=...): its collectives -- loss counts, trip count, "
                                          "gradient all-reduce -- are then recorded into the hipGraph; gloo moves tensors through "
                                          "the host, and the sharded update keeps per-rank state the snapshot around a capture does "
                                          "not cover.  Use capture=False")
        # the captured step's own Adam keeps the interleaved table copy current (ls2fm.fused): no rebuild inside the graph
        _fused.trust_mirror_in_capture(self.sdf, self.rad)
        self._graph = _capture_step(fn, self.params, self.optim)
        self._table_versions = None                     # the restore rewrote the tables behind the graph's back: _replay re-syncs
        return self._replay()


def _capture_step(fn, params, optim):
    """-> `fn` (one whole step over `params` / `optim`) recorded as a `CapturedStep`.  The capture warms the step up by running it
    for real: parameters, Adam state and the schedule are put back afterwards (in place: the graph holds their addresses), so
    that the caller's first replay is exactly one step"""
    snap = _snapshot_training_state(params, optim)
    graph = CapturedStep(fn, params=params)
    _restore_training_state(params, optim, snap)
    return graph


def _snapshot_training_state(params, opt):
    """parameters, Adam moments / step counts, learning rates and device schedules -- what a capture's warm-up steps change"""
    return dict(params=[p.detach().clone() for p in params],
                state=[({k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()} if p in opt.state else None)
                       for p in params],
                lrs=[float(g["lr"]) for g in opt.param_groups],
                sched={gi: t.clone() for gi, t in opt._sched.items()})


def _restore_training_state(params, opt, snap):
    """put a `_snapshot_training_state` back IN PLACE (a captured graph holds the addresses)"""
    with torch.no_grad():
        for p, old in zip(params, snap["params"]):
            p.copy_(old)
            torch.autograd.graph.increment_version(p)
        for p, old in zip(params, snap["state"]):
            st = opt.state.get(p)
            if not st:
                continue
            if old:
                st["step"] = old["step"]
                st["exp_avg"].copy_(old["exp_avg"])
                st["exp_avg_sq"].copy_(old["exp_avg_sq"])
            else:                       # state created by the warm-up: back to its initial value
                st["step"] = 0
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        for g, lr in zip(opt.param_groups, snap["lrs"]):
            g["lr"] = lr
        for gi, t in opt._sched.items():
            if gi in snap["sched"]:
                t.copy_(snap["sched"][gi])
            else:                       # schedule created by the warm-up: seeded from the step the group had BEFORE it
                steps = [int(old["step"]) for p, old in zip(params, snap["state"])
                         if old and any(p is q for q in opt.param_groups[gi]["params"])]
                t.copy_(torch.tensor([float(steps[0]) if steps else 0.0, snap["lrs"][gi], opt.scheduled_gamma, 0.0],
                                     dtype=torch.float64))

