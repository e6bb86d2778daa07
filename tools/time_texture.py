#!/usr/bin/env python
"""Times ls2fm.texture on the workload it was sized for -- the 512^3 sphere-plus-box mesh of tools/time_raster.py simplified to about
100 000 faces, 49 views of 1200 x 1600 x 3, an atlas of 4096^2 -- and writes profiles/texture_time.json:
  build_atlas     size given, texel bisected (torch ops and 22 host reads; it has no other form)
  texels          ls2fm_texture_texels over the whole atlas -- against ls2fm.texture._texels_torch
  photo_texture   end to end (the texels per band, the rasterisations, the vertex-colour kernel per chunk, the finish) -- against the
                  same bands through ls2fm.mesh_colors.photo_colors_torch on the same depth maps
  render_views    all views: rasterize with barycentrics + ls2fm_texture_render -- against rasterize + render_textured_torch
The texels and the render are checked bit-equal to their torch forms first (NaN matching NaN); photo_texture's counts exactly and its
colours to 1e-6, the bar ls2fm.mesh_colors' own torch form is held to.  HIP events around windows of --calls calls, the forms
alternated inside every repetition, the median of --reps windows.
    python tools/time_texture.py [--res 512] [--faces 100000] [--views 49] [--height 1200] [--width 1600] [--size 4096] [--reps 5]"""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--faces", type=int, default=100000)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_time.json"))
    a = ap.parse_args()
    import torch
    from time_raster import alternated, scene
    from ls2fm import mesh_colors as MC, raster, simplify, texture as T
    dev = "cuda:0"
    H, W, N, S = a.height, a.width, a.views, a.size
    verts, faces, poses, K = scene(a.res, N, H, W, dev)
    full_faces = int(faces.shape[0])
    small = simplify.simplify_to_faces(verts, faces, a.faces)
    verts, faces = small.vertices, small.faces
    del small
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    images = torch.stack([torch.stack([0.5 + 0.4 * torch.sin(6.0 * (c + 1) * xx + 4.0 * yy + 0.3 * i) for c in range(3)], dim=-1)
                          for i in range(N)]).contiguous()
    del yy, xx
    atlas = T.build_atlas(verts, faces, size=S)
    kw = dict(depth_tol=1e-2, power=1)

    def bits_equal(x, y):
        return bool(((x == y) | (torch.isnan(x) & torch.isnan(y)) if x.dtype.is_floating_point else x == y).all())

    # the forms agree first
    got, ref = T.atlas_texels(atlas, verts, faces), T._texels_torch(atlas, verts, faces)
    if not all(bits_equal(g, r) for g, r in zip(got, ref)):
        raise SystemExit("ls2fm_texture_texels and its torch form differ")
    owned = int((got.face >= 0).sum())
    del got, ref
    depth = raster.rasterize(verts, faces, poses, K, H, W).depth
    bands = T._row_bands(S, 24 + 8 * 4 + 4 + 12, None)

    def photo_torch():
        out = []
        for r0, r1 in bands:
            tx = T.atlas_texels(atlas, verts, faces, (r0, r1))
            out.append(MC.photo_colors_torch(tx.point.view(-1, 3), poses, K, images, depth, normals=tx.normal.view(-1, 3), **kw))
        return torch.cat([o.colors for o in out]).view(S, S, 3), torch.cat([o.count for o in out]).view(S, S)
    tex = T.photo_texture(verts, faces, atlas, poses, K, images, **kw)
    tex_t, count_t = photo_torch()
    differ = int((tex.count != count_t).sum())
    close = torch.isclose(tex.texture, tex_t, rtol=1e-6, atol=1e-7, equal_nan=True)
    if differ or not bool(close.all()):
        raise SystemExit(f"photo_texture and its torch form differ: {differ} counts, {int((~close).sum())} colours")
    seen = int((tex.count > 0).sum())
    del tex_t, count_t, close
    chunks = [(s, min(s + 4, N)) for s in range(0, N, 4)]

    def render_torch():
        return [T.render_textured_torch(atlas, tex.texture, raster.rasterize(verts, faces, poses[s:e], K, H, W, bary=True)) for s, e in chunks]
    one = T.render_views(verts, faces, atlas, tex.texture, poses[:4], K, H, W, view_chunk=4)
    if not bits_equal(one, render_torch()[0]):
        raise SystemExit("ls2fm_texture_render and its torch form differ")
    del one
    res = dict(volume=a.res, faces_before_simplify=full_faces, n_verts=int(verts.shape[0]), n_faces=int(faces.shape[0]), n_views=N, height=H,
               width=W, channels=3, atlas_size=S, texel=atlas.texel, gutter=atlas.gutter, classes=[list(c) for c in atlas.classes],
               cells_area=T.layout(atlas.classes)[3], owned_texels=owned, texels_seen=seen, row_bands=len(bands),
               texels_bit_equal_torch=True, render_bit_equal_torch=True, photo_texture_counts_equal_colours_within_1e6_of_torch=True)
    forms = {
        "build_atlas": lambda: T.build_atlas(verts, faces, size=S),
        "texels": lambda: T.atlas_texels(atlas, verts, faces),
        "texels_torch": lambda: T._texels_torch(atlas, verts, faces),
        "photo_texture": lambda: T.photo_texture(verts, faces, atlas, poses, K, images, **kw),
        "photo_texture_on_given_depth": lambda: T.photo_texture(verts, faces, atlas, poses, K, images, depth=depth, **kw),
        "photo_texture_torch_on_given_depth": photo_torch,
        "render_views": lambda: T.render_views(verts, faces, atlas, tex.texture, poses, K, H, W, view_chunk=4),
        "render_views_torch": render_torch,
        "rasterize_bary_share": lambda: [raster.rasterize(verts, faces, poses[s:e], K, H, W, bary=True) for s, e in chunks],
    }
    res["times"] = alternated(forms, a.reps, a.calls)
    t = res["times"]
    ms = lambda k: t[k]["median_ms"]
    res["torch_over_texels"] = ms("texels_torch") / ms("texels")
    res["torch_over_photo_texture_on_given_depth"] = ms("photo_texture_torch_on_given_depth") / ms("photo_texture_on_given_depth")
    res["torch_over_render_views"] = ms("render_views_torch") / ms("render_views")
    res["texels_GB_per_s_written"] = 28.0 * S * S / (ms("texels") * 1e6)
    res["notes"] = "HIP-event windows only; no kernel trace and no counter run was made"
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
