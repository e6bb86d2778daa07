#!/usr/bin/env python
"""Times ls2fm.mesh_colors on the workload it was sized for -- the 512^3 sphere-plus-box mesh of tools/time_raster.py seen from 49
views of 1200 x 1600 x 3 -- and writes profiles/mesh_colors_time.json:
  photo_colors   end to end (a rasterisation per chunk of views, the vertex kernel per chunk, the finish), its rasterize share
                 apart (the same chunks rasterised alone), and the vertex kernel alone on depth maps already there -- against
                 the same rule as torch ops on the same GPU (ls2fm.mesh_colors.photo_colors_torch on those depth maps)
  field_colors   ls2fm_radiance_points at that mesh's vertex count on a DTU dual-field model of the reference's sizes (random
                 state) -- against the torch composition (ls2fm.mesh_colors.field_colors_composed)
Each pair is checked equal first (counts exactly and colours to 1e-6; rgb to the 1e-4 parity bar).  HIP events around windows of
--calls calls, the forms alternated inside every repetition, the median of --reps windows.
    python tools/time_mesh_colors.py [--res 512] [--views 49] [--height 1200] [--width 1600] [--reps 7] [--calls 3]"""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def field(dev):
    import torch
    from ls2fm.models.RadF import RadF
    from ls2fm.models.SDF import SDF
    from ls2fm.options import make_options
    enc = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16)
    opt = make_options("DTU", device=dev, dual_field=True, sample_intvs=128, hash_encoding=enc)
    torch.manual_seed(0)
    sdf, rad = SDF(opt).to(dev), RadF(opt).to(dev)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in (sdf, rad):
            for name, p in mod.named_parameters():
                if name.endswith("embedder_obj.params"):
                    p.copy_(((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1).to(dev))
                if name.endswith("mlp.0.weight_v") and "Rad_dec" not in name:
                    p[:, 3:] = (torch.randn(p[:, 3:].shape, generator=gen) * 0.05).to(dev)
    return opt, sdf, rad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_colors_time.json"))
    a = ap.parse_args()
    import torch
    from time_raster import alternated, scene
    from ls2fm import _posed, mesh_colors as MC, raster
    dev = "cuda:0"
    H, W, N = a.height, a.width, a.views
    verts, faces, poses, K = scene(a.res, N, H, W, dev)
    n_v, n_f = int(verts.shape[0]), int(faces.shape[0])
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    images = torch.stack([torch.stack([0.5 + 0.4 * torch.sin(6.0 * (c + 1) * xx + 4.0 * yy + 0.3 * i) for c in range(3)], dim=-1)
                          for i in range(N)]).contiguous()
    del yy, xx
    per_chunk = max(1, 2 ** 28 // (8 * H * W))
    chunks = [(s, min(s + per_chunk, N)) for s in range(0, N, per_chunk)]
    opt, sdf, rad = field(dev)
    rgb, g = MC.field_colors(opt, sdf, rad, verts, return_normals=True)
    depth = raster.rasterize(verts, faces, poses, K, H, W).depth
    kw = dict(normals=g, depth_tol=1e-2, power=1)

    # the forms agree first
    got = MC.photo_colors(verts, faces, poses, K, images, **kw)
    ref = MC.photo_colors_torch(verts, poses, K, images, depth, **kw)
    differ = int((got.count != ref.count).sum())
    close = torch.isclose(got.colors, ref.colors, rtol=1e-6, atol=1e-7, equal_nan=True)
    if differ or not bool(close.all()):
        raise SystemExit(f"photo_colors and its torch form differ: {differ} counts, {int((~close).sum())} colours")
    comp = MC.field_colors_composed(opt, sdf, rad, verts)
    gap = float((rgb - comp).abs().max() / comp.abs().max())
    if not gap < 1e-4:
        raise SystemExit(f"field_colors and the torch composition differ: {gap:.3e}")
    res = dict(volume=a.res, n_verts=n_v, n_faces=n_f, n_views=N, height=H, width=W, channels=3, views_per_chunk=per_chunk,
               vertices_seen=int((got.count > 0).sum()), mean_views_per_seen_vertex=float(got.count.sum()) / max(int((got.count > 0).sum()), 1),
               photo_colors_equal_torch=True, field_rgb_gap_kernel_vs_composition=gap)
    del got, ref, comp, close
    state = lambda: (torch.zeros(n_v, 4, dtype=torch.float64, device=dev), torch.zeros(n_v, dtype=torch.int32, device=dev))
    pose4 = _posed.views(poses, K, "time")

    def kernel_alone():
        st = state()
        MC.accumulate_views(st, verts, pose4, images, depth, None, g, 1e-3, 1e-2, 1)
        return MC.finish_colors(st, 3)

    forms = {
        "photo_colors": lambda: MC.photo_colors(verts, faces, poses, K, images, **kw),
        "rasterize_share": lambda: [raster.rasterize(verts, faces, poses[s:e], K, H, W).depth for s, e in chunks],
        "vertex_kernel_on_given_depth": kernel_alone,
        "photo_colors_torch_on_given_depth": lambda: MC.photo_colors_torch(verts, poses, K, images, depth, **kw),
        "field_colors": lambda: MC.field_colors(opt, sdf, rad, verts),
        "field_colors_torch": lambda: MC.field_colors_composed(opt, sdf, rad, verts),
    }
    res["times"] = alternated(forms, a.reps, a.calls)
    t = res["times"]
    res["torch_over_vertex_kernel"] = t["photo_colors_torch_on_given_depth"]["median_ms"] / t["vertex_kernel_on_given_depth"]["median_ms"]
    res["field_torch_over_kernel"] = t["field_colors_torch"]["median_ms"] / t["field_colors"]["median_ms"]
    res["rasterize_share_of_photo_colors"] = t["rasterize_share"]["median_ms"] / t["photo_colors"]["median_ms"]
    res["notes"] = "HIP-event windows only; no kernel trace and no counter run was made"
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
