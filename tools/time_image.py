#!/usr/bin/env python
"""Whole-image rendering, two paths on the same weights and pose (no_grad), one JSON line per configuration:
  sliced  the reference's render_img_by_slices: rays of every pixel (camera_rays, so that both paths see the same rays), then
          Renderer.forward per 8192-ray slice, then cat
  image   ls2fm.image.render_image (one ls2fm_render_image call)
ms per image and M rays/s of each path, the growth of torch.cuda.max_memory_allocated over each call, max |delta| between them.
    python tools/time_image.py [--only dtu] [--reps 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd")]

import torch  # noqa: E402

from ls2fm import image  # noqa: E402
from ls2fm.models.RadF import RadF  # noqa: E402
from ls2fm.models.Renderer import Renderer  # noqa: E402
from ls2fm.models.SDF import SDF  # noqa: E402
from ls2fm.options import make_options  # noqa: E402
from ls2fm.utils import camera as cam  # noqa: E402

DEV = "cuda"
CONFIGS = {      # name: dataset, dual field, H, W, views
    "dtu": ("DTU", True, 1200, 1600, 1),
    "eth3d_single": ("ETH3D", False, 1033, 1551, 1),
    "bmvs_white": ("BlendedMVS", True, 576, 768, 1),
    "dtu_8views": ("DTU", True, 1200, 1600, 8),
}


def scene(ds, dual, n=128):
    enc = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16)
    opt = make_options(ds, device=DEV, dual_field=dual, sample_intvs=n, hash_encoding=enc)
    torch.manual_seed(0)
    sdf, rad, ren = SDF(opt).to(DEV), RadF(opt).to(DEV), Renderer(opt)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in (sdf, rad):
            for name, p in mod.named_parameters():
                if name.endswith("embedder_obj.params"):
                    p.copy_(((torch.rand(p.shape, generator=g) * 2 - 1) * 0.1).to(DEV))
                if name.endswith("mlp.0.weight_v") and "Rad_dec" not in name:
                    p[:, 3:] = (torch.randn(p[:, 3:].shape, generator=g) * 0.05).to(DEV)
    return opt, sdf, rad, ren


def views(opt, H, W, V):
    h = float(opt.data.bound_max[0])
    g = torch.Generator().manual_seed(3)
    se3 = torch.cat([0.15 * torch.randn(V, 3, generator=g), 0.1 * h * torch.randn(V, 3, generator=g)], dim=1)
    se3[:, 5] += 3.0 * h
    poses = cam.lie.se3_to_SE3(se3.to(DEV)).contiguous()
    intr = torch.tensor([[1.0 * W, 0.0, W / 2.0], [0.0, 1.0 * W, H / 2.0], [0.0, 0.0, 1.0]], device=DEV)
    return poses, intr


@torch.no_grad()
def sliced(ren, opt, sdf, rad, poses, intr, H, W, kinv):
    c, r = cam.camera_rays(kinv, poses=poses, pix=torch.arange(H * W, device=DEV), width=W)
    rgbs, depths, norms = [], [], []
    for s in range(0, H * W, 8192):
        out = ren.forward(opt, c[:, s:s + 8192], r[:, s:s + 8192], sdf, rad)
        rgbs.append(out["rgb"]), depths.append(out["depth_mlp"]), norms.append(out["normal_mlp"])
    return torch.cat(rgbs, dim=1), torch.cat(depths, dim=1), torch.cat(norms, dim=1)


def timed(fn, reps):
    out = fn()                                   # warm-up (plans, workspaces in the caching allocator)
    torch.cuda.synchronize()
    del out
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    grow = torch.cuda.max_memory_allocated() - base
    return out, min(ts), grow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for name, (ds, dual, H, W, V) in CONFIGS.items():
        if args.only and name != args.only:
            continue
        opt, sdf, rad, ren = scene(ds, dual)
        poses, intr = views(opt, H, W, V)
        kinv = cam.host_inverse_intrinsic(intr)
        reps = max(1, args.reps if V == 1 else args.reps // 2)
        ref, t_sl, m_sl = timed(lambda: sliced(ren, opt, sdf, rad, poses, intr, H, W, kinv), reps)
        img, t_im, m_im = timed(lambda: image.render_image(ren, opt, sdf, rad, poses, intr, H=H, W=W), reps)
        delta = max(float((img.rgb - ref[0]).abs().max()), float((img.depth - ref[1]).abs().max()),
                    float((img.norm - ref[2]).abs().max()))
        rays = V * H * W
        print(json.dumps({"config": name, "dataset": ds, "dual": dual, "H": H, "W": W, "views": V, "n_samples": 128,
                          "sliced_ms_per_image": round(t_sl / V, 3), "sliced_mrays_s": round(rays / t_sl / 1e3, 3),
                          "image_ms_per_image": round(t_im / V, 3), "image_mrays_s": round(rays / t_im / 1e3, 3),
                          "speedup": round(t_sl / t_im, 3), "sliced_peak_growth_mb": round(m_sl / 2**20, 1),
                          "image_peak_growth_mb": round(m_im / 2**20, 1), "max_abs_delta": delta}), flush=True)
        del ref, img
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
