"""Whole-image rendering: Camera.render_img_by_slices (pipelines/Camera.py:274-311 of the reference) without the slices.

The reference forms the rays of every pixel (get_center_and_ray) and runs Renderer.forward over them in rand_rays slices -- a path
built for training: each slice allocates the training workspace and writes the per-sample outputs and save streams nobody reads.
`render_image` renders all pixels of one or more views in ONE call of ls2fm_render_image (csrc/render_image.hip): rays formed
on the device from the pixel index, a bounded workspace walked in chunks, per-ray outputs only.  Every pixel's outputs are bit
for bit those of Renderer.forward on the ray `camera_rays` forms for it.

Configurations the fused kernels do not serve (bg_sdf, oversize tables, more samples than the shading kernels take) and CPU
tensors run the reference's own loop instead: get_center_and_ray + Renderer.forward per rand_rays slice + cat.

Rebinding the reference's method:   Camera.render_img_by_slices = ls2fm.image.render_img_by_slices
"""
from __future__ import annotations

import ctypes

import torch

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
