"""Whole-image rendering: Camera.render_img_by_slices (pipelines/Camera.py:274-311 of the reference) without the slices.

The reference forms the rays of every pixel (get_center_and_ray) and runs Renderer.forward over them in rand_rays slices -- a path
built for training: each slice allocates the training workspace and writes the per-sample outputs and save streams nobody reads.
`render_image` renders all pixels of one or more views in ONE call of ls2fm_render_image (csrc/render_image.hip): rays formed
on the device from the pixel index, a bounded workspace walked in chunks, per-ray outputs only.  Every pixel's outputs are bit
for bit those of Renderer.forward on the ray `camera_rays` forms for it.

Configurations the fused kernels do not serve (bg_sdf, oversize tables, more samples than the shading kernels take) and CPU
tensors run the reference's own loop instead: get_center_and_ray + Renderer.forward per rand_rays slice + cat.

Rebinding the reference's method:   Camera.render_img_by_slices = ls2fm.image.render_img_by_slices

`trace_image` does the same for the depth and normal maps of Camera.get_depth (pipelines/Camera.py:216-253): one call of
ls2fm_trace_image (csrc/trace_image.hip) sphere-traces every pixel with the trip count K of a call over the view alone and returns
per-pixel outputs only -- no track, no re-evaluation of it, one normal query.  `get_depth` is the drop-in
(Camera.get_depth = ls2fm.image.get_depth); with grad enabled, on CPU tensors, for bg_sdf or several poses it runs the reference's
steps on this package's classes instead (get_center_and_ray, SDF.sphere_tracing, SDF.gradient).

`evaluate_views` is render_image followed by ls2fm.image_metrics.compare_images on its rgb: the PSNR / SSIM of the rendered views
against the photographs, per view, without leaving the device.
"""
from __future__ import annotations

import copy
import ctypes

import torch
import torch.nn.functional as torch_F

from . import _lib, fused
from ._lib import check, ptr, stream_ptr
from .options import Options
from .utils import camera


def _kinv_host(intr):
    """K^-1 as 9 host floats (utils.camera.host_inverse_intrinsic), remembered on the matrix per version: a call captured in a
    graph after an eager one reads no device value back"""
    key = (intr.data_ptr(), intr._version, tuple(intr.shape))
    memo = getattr(intr, "_ls2fm_kinv_host", None)
    if memo is None or memo[0] != key:
        memo = (key, camera.host_inverse_intrinsic(intr.detach().reshape(3, 3)))
        try:
            intr._ls2fm_kinv_host = memo
        except Exception:
            pass
    return memo[1]


def _image_size(opt, H, W):
    H = int(opt.H) if H is None else int(H)
    W = int(opt.W) if W is None else int(W)
    if H < 1 or W < 1:
        raise ValueError(f"ls2fm.image: image size {H} x {W}")
    return H, W


@torch.no_grad()
def render_image(renderer, opt, sdf_field, rad_field, pose, intr, H=None, W=None, opacity=False):
    """Render every pixel of V views.  pose [3,4] or [V,3,4] world-to-camera, intr [3,3] (or [1,3,3]); H, W default to
    opt.H, opt.W.  -> Options(rgb [V,HW,3], depth [V,HW,1], norm [V,HW,3][, opacity [V,HW,1]]), pixels row-major."""
    H, W = _image_size(opt, H, W)
    poses = pose.reshape(-1, 3, 4)
    plan = fused._plan(renderer, opt, sdf_field, rad_field) if poses.is_cuda else None
    if plan is None or not plan.ok:
        return _render_sliced(renderer, opt, sdf_field, rad_field, poses, intr, H, W, opacity)
    lib = _lib.load()
    fdesc, g1, g2, dual, _, _ = plan.cfg
    fused.bind_params(lib, plan, plan.ts)
    ws_bytes = plan.ws_bytes.get("image")
    if ws_bytes is None:
        ws_bytes = lib.ls2fm_render_image_workspace_bytes(ctypes.byref(fdesc), ctypes.byref(g1), ctypes.byref(g2) if dual else None)
        if ws_bytes < 0:
            check(int(ws_bytes), "ls2fm_render_image_workspace_bytes")
        plan.ws_bytes["image"] = ws_bytes
    dev = poses.device
    V = poses.shape[0]
    pc = poses if (poses.dtype == torch.float32 and poses.is_contiguous()) else poses.float().contiguous()
    rgb = torch.empty(V, H * W, 3, device=dev)
    depth = torch.empty(V, H * W, 1, device=dev)
    norm = torch.empty(V, H * W, 3, device=dev)
    op = torch.empty(V, H * W, 1, device=dev) if opacity else None
    ws = torch.empty(ws_bytes // 4, device=dev, dtype=torch.float32)
    check(lib.ls2fm_render_image(ctypes.byref(fdesc), ctypes.byref(g1), ctypes.byref(g2) if dual else None,
                                 ctypes.byref(plan.pstruct), ptr(pc), V, _kinv_host(intr), H, W, ptr(rgb), ptr(depth), ptr(norm),
                                 ptr(op), ptr(ws), stream_ptr()), "ls2fm_render_image")
    ret = Options(rgb=rgb, depth=depth, norm=norm)
    if opacity:
        ret.opacity = op
    return ret


def _render_sliced(renderer, opt, sdf_field, rad_field, poses, intr, H, W, opacity):
    """the reference's loop (Camera.py:284-306): every pixel's ray, then Renderer.forward per rand_rays slice"""
    if opacity:
        raise NotImplementedError("ls2fm.image.render_image: opacity is an output of the fused image kernels only; this "
                                  "configuration renders through Renderer.forward, which does not return it")
    grid = camera.mesh_grid(H=H, W=W, device=poses.device)
    center, ray = camera.get_center_and_ray(opt, poses, intr=intr.reshape(1, 3, 3), xy_grid=grid)
    bat = int(opt.Renderer.rand_rays)
    rgbs, depths, norms = [], [], []
    for start in range(0, center.shape[1], bat):
        out = renderer.forward(opt, center[:, start:start + bat], ray[:, start:start + bat], sdf_field, rad_field)
        B = out["depth_mlp"].shape[0]
        depths.append(out["depth_mlp"])
        norms.append(out["normal_mlp"].view(B, -1, 3))
        rgbs.append(out["rgb"].view(B, -1, 3))
    return Options(rgb=torch.cat(rgbs, dim=1), depth=torch.cat(depths, dim=1), norm=torch.cat(norms, dim=1))


@torch.no_grad()
def render_img_by_slices(camera_obj, sdf_func, color_func, Renderer, pose_input=None):
    """Drop-in for Camera.render_img_by_slices (same arguments, keys and shapes: depth [B,HW,1], norm [B,HW,3], rgb [B,HW,3]).
    `camera_obj` needs what the reference's method reads: get_pose(), intrinsic and opt."""
    opt = camera_obj.opt
    pose = camera_obj.get_pose() if pose_input is None else pose_input
    ret = render_image(Renderer, opt, sdf_func, color_func, pose, camera_obj.intrinsic, H=opt.H, W=opt.W)
    return Options(depth=ret.depth, norm=ret.norm, rgb=ret.rgb)


@torch.no_grad()
def evaluate_views(renderer, opt, sdf_field, rad_field, poses, intr, images, masks=None, H=None, W=None, return_render=False,
                   **compare_kw):
    """The PSNR / SSIM row of a results table without leaving the device: render_image on `poses`, then
    ls2fm.image_metrics.compare_images of its rgb with `images` ([V, H, W, 3] or [V, HW, 3]; masks [V, H, W] or None;
    compare_kw: data_range, window, k1, k2, full).  -> ImageScores, or (ImageScores, the render) with return_render=True."""
    from . import image_metrics
    H, W = _image_size(opt, H, W)
    ret = render_image(renderer, opt, sdf_field, rad_field, poses, intr, H=H, W=W)
    images = torch.as_tensor(images)
    scores = image_metrics.compare_images(ret.rgb, images.reshape(ret.rgb.shape), mask=masks, H=H, W=W, **compare_kw)
    return (scores, ret) if return_render else scores


# ------------------------------------------------------------------------------------------------ depth and normal maps
def can_trace_image(sdf_field, probe) -> bool:
    """the configurations ls2fm_trace_image serves: GPU tensors, the fused kernels' layer sizes, no background-sphere min"""
    opt = sdf_field.opt
    return fused.available(sdf_field, probe) and not (opt.data.inside == True and opt.data.bg_sdf == True)  # noqa: E712


@torch.no_grad()
def trace_image(sdf_field, pose, intr, H=None, W=None):
    """Sphere-trace every pixel of V views.  pose [3,4] or [V,3,4] world-to-camera, intr [3,3] (or [1,3,3]); H, W default to
    opt.H, opt.W.  -> Options(depth [V,HW,1], sdf_last [V,HW], finish [V,HW] bool, points [V,HW,3], gradient [V,HW,3],
    t_end_k [V,HW], trips int32 [V]), pixels row-major.  Each view's values are, bit for bit, those of
    SDF.sphere_tracing(static_trips=True) on the rays `camera_rays` forms for its pixels, and of SDF.gradient at `points`."""
    opt = sdf_field.opt
    H, W = _image_size(opt, H, W)
    poses = pose.reshape(-1, 3, 4)
    if not can_trace_image(sdf_field, poses):
        raise RuntimeError("ls2fm.image.trace_image: the fused tracing kernels do not serve this configuration (CPU tensors, "
                           "background sphere or non-reference layer sizes); ls2fm.image.get_depth runs the reference's steps")
    lib = _lib.load()
    keep, pstruct = fused._sdf_only_params(sdf_field)
    fdesc = fused.field_desc(opt)
    gdesc = sdf_field.embed_fn.embedder_obj.desc
    ws_bytes = lib.ls2fm_trace_image_workspace_bytes(ctypes.byref(fdesc), ctypes.byref(gdesc))
    if ws_bytes < 0:
        check(int(ws_bytes), "ls2fm_trace_image_workspace_bytes")
    dev = poses.device
    V = poses.shape[0]
    pc = poses if (poses.dtype == torch.float32 and poses.is_contiguous()) else poses.float().contiguous()
    depth = torch.empty(V, H * W, 1, device=dev)
    last = torch.empty(V, H * W, device=dev)
    finish = torch.empty(V, H * W, device=dev, dtype=torch.uint8)
    points = torch.empty(V, H * W, 3, device=dev)
    grad = torch.empty(V, H * W, 3, device=dev)
    t_end_k = torch.empty(V, H * W, device=dev)
    trips = torch.empty(V, device=dev, dtype=torch.int32)
    ws = torch.empty(ws_bytes // 4, device=dev, dtype=torch.float32)
    check(lib.ls2fm_trace_image(ctypes.byref(fdesc), ctypes.byref(gdesc), ctypes.byref(pstruct), ptr(pc), V, _kinv_host(intr), H, W,
                                float(sdf_field.sdf_threshold), int(sdf_field.iters_max), fused._finish_threshold(sdf_field),
                                ptr(depth), ptr(last), ptr(finish), ptr(points), ptr(grad), ptr(t_end_k), ptr(trips), ptr(ws),
                                stream_ptr()), "ls2fm_trace_image")
    return Options(depth=depth, sdf_last=last, finish=finish.view(torch.bool), points=points, gradient=grad, t_end_k=t_end_k,
                   trips=trips)


def _maps(depth_rows, sdf_last, finish, points, gradient, sampled, norm_hw):
    """the dictionary Camera.get_depth returns, from per-pixel rows: rows whose depth is infinite are dropped; the normal map is
    the normalised gradient, its length is `normals_value`"""
    keep = ~torch.isinf(depth_rows)
    pts = points[keep]
    grad = gradient[keep]
    return Options(depth=depth_rows[keep][:, None], mask_finish=finish, norms=torch_F.normalize(grad, dim=-1).view(1, *norm_hw, -1),
                   pts_surface=pts, normals_value=grad.norm(dim=-1, keepdim=True), sdf_surf=sdf_last, sample_pts=sampled.detach())


def depth_body(sdf_func, center, ray, norm_hw):
    """the reference's get_depth steps after the rays, on this package's classes: SDF.sphere_tracing (its random draws included),
    the surface points center + depth * ray and SDF.gradient there"""
    d_pts, sdf_last, sampled, finish = sdf_func.sphere_tracing(center, ray, sdf_func)
    keep = ~torch.isinf(d_pts)
    pts = center[keep] + d_pts[keep][:, None] * ray[keep]
    grad = sdf_func.gradient(pts)                # marks `pts` (requires_grad), as the reference's two calls do
    out = _maps(d_pts[keep], sdf_last, finish, pts, grad, sampled, norm_hw)
    out.pts_surface = pts
    return out


def _depth_device(opt, sdf_func, pose, intr, H, W, norm_hw):
    """get_depth's outputs from one ls2fm_trace_image call: the sample points are formed as SDF.sphere_tracing forms them, with the
    same draws (a device rand over the rays, a host randperm) -- the picked rays' tracks re-traced on their own, which gives the
    same points (a ray's track does not depend on the others), cut at the view's K"""
    t = trace_image(sdf_func, pose, intr, H=H, W=W)
    R = H * W
    dev = t.depth.device
    d_pts = t.depth.view(1, R)
    u = torch.rand_like(d_pts)
    pick = torch.randperm(R)[:4096]
    center, ray = camera.camera_rays(_kinv_host(intr), poses=pose.reshape(1, 3, 4), pix=torch.arange(R, device=dev), width=W)
    from .utils.custom_functions import RayAABBIntersector
    _, hits_t, _ = RayAABBIntersector.apply(center.view(-1, 3), ray.view(-1, 3), sdf_func.center.view(1, 3),
                                            sdf_func.half_size.view(1, 3), 1)
    near, far = hits_t[:, 0, 0].view(1, R), hits_t[:, 0, 1].view(1, R)
    t_up = 1.5 * t.t_end_k.view(1, R)
    t_up = torch.where(t_up > far, far, t_up)
    t_rand = (1 - u) * t_up + u * near
    pk = pick.to(dev)
    _, _, track, _, _ = fused.sphere_trace(sdf_func, center.view(-1, 3)[pk], ray.view(-1, 3)[pk], sync=False)
    k = max(int(t.trips[0]), 1)
    along = ray.mul_(t_rand[..., None]).add_(center)           # center + t_rand * ray, in place of the rays
    sampled = torch.cat([track[:, :k].reshape(1, -1, 3), along.view(1, -1, 3)], dim=1)
    out = _maps(d_pts.view(-1), t.sdf_last.view(-1), t.finish.view(-1, 1), t.points.view(-1, 3), t.gradient.view(-1, 3), sampled,
                norm_hw)
    out.pts_surface.requires_grad_(True)        # SDF.gradient marks its argument (the reference calls it on these points)
    return out


def _depth_maps(opt, sdf_func, pose, intr, norm_hw):
    """Camera.get_depth's body for the image size opt.H x opt.W: the device path where it serves (no graph wanted, one pose),
    else the reference's steps"""
    H, W = int(opt.H), int(opt.W)
    poses = pose.reshape(-1, 3, 4)
    if not torch.is_grad_enabled() and poses.shape[0] == 1 and can_trace_image(sdf_func, poses):
        return _depth_device(opt, sdf_func, poses, intr, H, W, norm_hw)
    center, ray = camera.get_center_and_ray(opt, pose, intr=intr)
    return depth_body(sdf_func, center, ray, norm_hw)


def get_depth(camera_obj, sdf_func, mode="train"):
    """Drop-in for Camera.get_depth (same keys, shapes and side effects): depth [N,1], mask_finish [HW,1], norms [1,H,W,3],
    pts_surface [N,3], normals_value [N,1], sdf_surf [HW], sample_pts [1, 4096 K + HW, 3].  mode="eval": a quarter of the
    image size (intrinsics divided by 4) under no_grad; opt.H, opt.W are left at opt.data.image_size.  `camera_obj` needs what
    the reference's method reads: get_pose(), intrinsic and opt."""
    opt = camera_obj.opt
    if mode == "eval":
        with torch.no_grad():
            pose = camera_obj.get_pose()
            factor = 4
            opt.H, opt.W = int(opt.H // factor), (opt.W // factor)
            intr = copy.deepcopy(camera_obj.intrinsic)
            for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):
                intr[i, j] /= factor
            ret = _depth_maps(opt, sdf_func, pose, intr, (int(opt.H), int(opt.W)))
            opt.H, opt.W = opt.data.image_size
        return ret
    size = opt.data.image_size
    return _depth_maps(opt, sdf_func, camera_obj.get_pose(), camera_obj.intrinsic, (int(size[0]), int(size[1])))
