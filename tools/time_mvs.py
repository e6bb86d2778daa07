#!/usr/bin/env python
"""Times ls2fm.mvs on the workload the other tools use -- 49 views of 1200 x 1600 of the sphere-plus-box mesh of tools/time_raster.py
from its ring of cameras, shaded into grey images by a procedural texture of world position through ls2fm.raster.rasterize's
barycentrics (off the mesh a pattern of the pixel, so every window does the full work) -- with S = 4 sources, D = 128 planes uniform
in inverse depth and w = 3, and writes profiles/mvs_time.json:
  sweep_one_reference   ls2fm_mvs_sweep for one reference view; the same with D / 2 planes (the scaling in D)
  sweep_all             every view as a reference, in plane_sweep's chunks
  sweep_torch_one_reference   the same rule as torch ops on the same GPU (ls2fm.mvs.plane_sweep_torch), checked bit-equal first
  filter, filter_torch  ls2fm_mvs_filter over the 49 swept depth maps, and its torch form, checked bit-equal first
  dense_reconstruct     sweep -> filter -> fusion into a --res^3 volume -> extract, end to end
Beside the kernel's time stands the byte floor -- per reference its image and S source images read once and 12 bytes per pixel
written -- as a time at 8.0 TB/s.  HIP events around windows of --calls calls, the forms alternated inside every repetition, the
median of --reps windows.
    python tools/time_mvs.py [--mesh-res 512] [--res 512] [--views 49] [--height 1200] [--width 1600] [--reps 5] [--calls 1]"""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

ROOFLINE = 8.0e12


def shade(verts, faces, poses, K, H, W, per_chunk=7):
    """grey float32 [V, H, W]: a texture of the world position under every pixel, a pattern of the pixel off the mesh"""
    import torch
    from ls2fm import raster
    out = []
    yy, xx = torch.meshgrid(torch.arange(H, device=verts.device).float(), torch.arange(W, device=verts.device).float(), indexing="ij")
    sky = 0.5 + 0.25 * torch.sin(0.9 * xx) * torch.sin(1.1 * yy)
    for s in range(0, poses.shape[0], per_chunk):
        r = raster.rasterize(verts, faces, poses[s:s + per_chunk], K, H, W, bary=True)
        hit = r.face_id >= 0
        corners = verts[faces.long()[r.face_id.clamp(min=0).long()]]                     # [v, H, W, 3 corners, 3]
        p = (r.bary[..., None] * corners).sum(dim=-2)
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        tex = 0.5 + 0.1 * (torch.sin(190.0 * x + 1.3) + torch.sin(230.0 * y + 0.7) + torch.sin(270.0 * z + 2.1)) \
            + 0.1 * torch.sin(61.0 * (x + y + z))
        out.append(torch.where(hit, tex, sky[None]))
        del r, corners, p
    return torch.cat(out).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-res", type=int, default=512)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--half-width", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_time.json"))
    a = ap.parse_args()
    import torch
    from time_raster import alternated, scene
    from ls2fm import mvs
    dev = "cuda:0"
    H, W, N, S, D, w = a.height, a.width, a.views, a.sources, a.planes, a.half_width
    verts, faces, poses, K = scene(a.mesh_res, N, H, W, dev)
    grey = shade(verts, faces, poses, K, H, W)
    sources = mvs.select_sources(poses, S, 3.0, 45.0, centre=(0.0, 0.0, 0.0))
    near, far = mvs.depth_range_from_points(verts[::97], poses, 0.05)
    depths = mvs.depth_planes(near, far, D)
    kw = dict(half_width=w, near=1e-3, min_var=1e-6, min_sources=2)
    one = torch.tensor([N // 2], device=dev)
    pick = lambda t: t[N // 2:N // 2 + 1]
    same = lambda x, y: bool(torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y))

    def bits_differ(got, ref):
        return sum(int(((g != r) & ~(g.isnan() & r.isnan()) if g.dtype == torch.float32 else g != r).sum()) for g, r in zip(got, ref))

    # the forms agree first, bit for bit (a NaN for a NaN)
    got = mvs.plane_sweep(grey, poses, K, pick(sources), pick(depths), refs=one, **kw)
    ref = mvs.plane_sweep_torch(grey, poses, K, pick(sources), pick(depths), refs=one, **kw)
    if bits_differ(got, ref):
        raise SystemExit(f"plane_sweep and its torch form differ on {bits_differ(got, ref)} entries of one reference")
    valid_share = float((got[2] >= 0).float().mean())
    depth, score, plane = mvs.plane_sweep(grey, poses, K, sources, depths, **kw)
    fkw = dict(near=1e-3, max_reproj=1.0, rel_depth=0.01, min_consistent=2)
    filtered, count = mvs.filter_depths(depth, poses, K, sources, **fkw)
    tf, tc = mvs.filter_depths_torch(depth, poses, K, sources, **fkw)
    if bits_differ((filtered, count), (tf, tc)):
        raise SystemExit(f"filter_depths and its torch form differ on {bits_differ((filtered, count), (tf, tc))} entries")
    # how good the depth maps are, against the rasteriser's
    from ls2fm import raster
    truth = raster.rasterize(verts, faces, pick(poses), K, H, W).depth[0]
    alive = torch.isfinite(pick(filtered)[0]) & torch.isfinite(truth)
    err = (pick(filtered)[0][alive] - truth[alive]).abs()
    spacing = float(pick(depths)[0].diff().abs().median())
    must_move = (1 + S) * 4 * H * W + 12 * H * W
    res = dict(n_views=N, height=H, width=W, sources=S, planes=D, half_width=w, taps=(2 * w + 1) ** 2,
               sweep_equals_torch_bit_for_bit=True, filter_equals_torch_bit_for_bit=True, valid_share_of_the_timed_reference=valid_share,
               survivors_share_of_the_timed_reference=float(torch.isfinite(pick(filtered)).float().mean()),
               survivors_on_the_mesh_median_abs_error=float(err.median()), median_plane_spacing=spacing,
               bytes_must_move_per_reference=must_move, roofline_bytes_per_s=ROOFLINE, roofline_ms_per_reference=must_move / ROOFLINE * 1e3)
    del tf, tc, ref, got, truth, alive, err
    opt = mvs.MvsOptions(half_width=w, min_var=1e-6, min_sources=2, n_planes=D)
    bounds = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    forms = {
        "sweep_one_reference": lambda: mvs.plane_sweep(grey, poses, K, pick(sources), pick(depths), refs=one, **kw),
        "sweep_one_reference_half_the_planes": lambda: mvs.plane_sweep(grey, poses, K, pick(sources), pick(depths)[:, ::2].contiguous(), refs=one, **kw),
        "sweep_torch_one_reference": lambda: mvs.plane_sweep_torch(grey, poses, K, pick(sources), pick(depths), refs=one, **kw),
        "sweep_all": lambda: mvs.plane_sweep(grey, poses, K, sources, depths, **kw),
        "filter": lambda: mvs.filter_depths(depth, poses, K, sources, **fkw),
        "filter_torch": lambda: mvs.filter_depths_torch(depth, poses, K, sources, **fkw),
        "dense_reconstruct": lambda: mvs.dense_reconstruct(grey, poses, K, bounds, 2.0 / (a.res - 1), sources=sources, depths=depths, options=opt),
    }
    t = res["times"] = alternated(forms, a.reps, a.calls)
    one_ms = t["sweep_one_reference"]["median_ms"]
    res["sweep_ms_per_reference_in_all"] = t["sweep_all"]["median_ms"] / N
    res["torch_over_kernel_one_reference"] = t["sweep_torch_one_reference"]["median_ms"] / one_ms
    res["filter_torch_over_kernel"] = t["filter_torch"]["median_ms"] / t["filter"]["median_ms"]
    res["half_the_planes_over_all"] = t["sweep_one_reference_half_the_planes"]["median_ms"] / one_ms
    res["kernel_over_roofline_one_reference"] = one_ms / res["roofline_ms_per_reference"]
    res["window_correlations_per_s"] = float(H) * W * D * S / (one_ms * 1e-3)
    mesh = mvs.dense_reconstruct(grey, poses, K, bounds, 2.0 / (a.res - 1), sources=sources, depths=depths, options=opt)
    res["dense_mesh_faces"] = int(mesh.faces.shape[0])
    res["notes"] = ("HIP-event windows only; no kernel trace and no counter run was made.  The one-reference forms include plane_sweep's "
                    "argument conversions (relative poses, a handful of small torch ops).")
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
