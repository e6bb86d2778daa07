"""GPU: ls2fm_texture_texels and ls2fm_texture_render (csrc/mesh_texture.hip) through ls2fm.texture, every texel and every pixel by
their bits against the numpy restatement (tests/texture_restate.py); the torch forms, bands, reruns and replays; photo_texture end
to end on the restated sphere scene.  The rule itself is judged on the restatement (tests/test_texture_host.py)."""
import numpy as np
import pytest
import torch

import texture_restate as TR
import texture_scenes as TS
from test_hip_fuse import same

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def T():
    from ls2fm import texture
    return texture


def mesh_of(name):
    return TS.edge_mesh() if name == "edge" else TS.small_mesh(int(name))


def restated(name, texel, gutter, size):
    verts, faces = mesh_of(name)
    rot, cls = TR.classify(verts, faces, texel, gutter)
    order, table = TR.pack(cls, gutter)
    S = TR.smallest_size(table) if size is None else size
    return verts, faces, rot, cls, order, table, S


def replay(call, outputs):
    """capture `call` after a warm-up on a side stream; -> (graph, its outputs)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    return graph, outputs(out)


# mesh, texel, gutter, forced size, the size the case is there for.  1, 2 and 3 faces (3: an odd slot count, chart B of the last cell
# unowned); gutter 0, 1, 2; S = 8, 16, 64; edge: at least three classes, a zero-area face, a NaN vertex, a face index out of range;
# a forced size: an atlas with an unused tail
TEXEL_CASES = [("1", 1.0, 0, None, 8), ("1", 1.0, 1, None, 8), ("2", 1.0, 0, None, 8), ("2", 0.5, 2, None, 16), ("3", 1.0, 1, None, 16),
               ("3", 1.0, 0, 64, 64), ("edge", 4.0, 0, None, 64), ("edge", 4.0, 1, None, 64), ("edge", 8.0, 2, None, 64)]


@pytest.mark.parametrize("name,texel,gutter,size,S", TEXEL_CASES)
def test_texels_by_the_bits_of_the_restatement(T, name, texel, gutter, size, S):
    verts, faces, rot, cls, order, table, S_ = restated(name, texel, gutter, size)
    assert S_ == S
    if name == "edge":
        assert len(set(cls.tolist())) >= 3
    ref = TR.texels(verts, faces, order, rot, table, gutter, S)
    v, f = dev(verts), dev(faces)
    atlas = T.build_atlas(v, f, texel=texel, size=size, gutter=gutter)
    assert atlas.size == S and list(atlas.classes) == table
    same(atlas.rot, rot, "rot")
    same(atlas.order, order, "order")
    same(atlas.uv, ref["uv"], "the atlas's uv")
    uv = torch.full((len(faces), 3, 2), float("nan"), device=DEV)
    got = T.atlas_texels(atlas, v, f, uv=uv)
    torch.cuda.synchronize()
    for key in ("face", "point", "normal"):
        same(getattr(got, key), ref[key], key)
    same(uv, ref["uv"], "uv")
    assert (ref["face"] < 0).any() or name in ("2",)                         # every case but two full cells has unowned texels
    # the torch form on the device
    uv_t = torch.full_like(uv, float("nan"))
    form = T._texels_torch(atlas, v, f, uv=uv_t)
    for key in ("face", "point", "normal"):
        same(getattr(form, key), ref[key], f"{key}, torch form")
    same(uv_t, ref["uv"], "uv, torch form")
    # bands of 15 and 17 rows around the 16-texel tile, against one call; then a rerun
    uv_b = torch.full_like(uv, float("nan"))
    edges, at = [0], 0
    while at < S:
        at = min(S, at + (15 if len(edges) % 2 else 17))
        edges.append(at)
    parts = [T.atlas_texels(atlas, v, f, rows=(a, b), uv=uv_b) for a, b in zip(edges[:-1], edges[1:])]
    for key in ("face", "point", "normal"):
        same(torch.cat([getattr(p, key) for p in parts]), ref[key], f"{key}, bands")
    same(uv_b, ref["uv"], "uv, bands")
    again = T.atlas_texels(atlas, v, f)
    for key in ("face", "point", "normal"):
        same(getattr(again, key), ref[key], f"{key}, rerun")
    assert T.atlas_texels(atlas, v, f, rows=(3, 3)).face.shape == (0, S)


def test_texels_replay(T):
    verts, faces, rot, cls, order, table, S = restated("edge", 4.0, 1, None)
    ref = TR.texels(verts, faces, order, rot, table, 1, S)
    v, f = dev(verts), dev(faces)
    atlas = T.build_atlas(v, f, texel=4.0, gutter=1)
    uv = torch.full((len(faces), 3, 2), float("nan"), device=DEV)
    graph, out = replay(lambda: T.atlas_texels(atlas, v, f, uv=uv), lambda o: o)
    for _ in range(2):
        out.face.fill_(-7)
        out.point.fill_(-1.0)
        out.normal.fill_(-1.0)
        uv.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for key in ("face", "point", "normal"):
            same(getattr(out, key), ref[key], f"{key}, replay")
        same(uv, ref["uv"], "uv, replay")


def render_case(H, W, V, C, seed):
    """an edge-mesh atlas, a texture with a NaN texel under face 0's first corner, and a synthetic rasterisation: random faces
    and barycentrics, empty pixels, a face id out of range, barycentrics exactly on the vertices and on the edges of face 0"""
    verts, faces, rot, cls, order, table, S = restated("edge", 4.0, 1, None)
    uv = TR.chart_corners(order, rot, table, 1)
    rng = np.random.default_rng(seed)
    tex = rng.uniform(0, 1, (S, S, C)).astype(F32)
    tex[int(uv[0, 0, 1]), int(uv[0, 0, 0]), C - 1] = np.nan
    face_id = rng.integers(-1, len(faces) + 1, (V, H, W)).astype(np.int32)
    bary = rng.dirichlet([1, 1, 1], (V, H, W)).astype(F32)
    special = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0, 0.25, 0.75], [0.125, 0, 0.875]], F32)
    n = min(len(special), H * W)
    bary.reshape(V, -1, 3)[0, :n] = special[:n]
    face_id.reshape(V, -1)[0, :n] = 0
    if H * W > 8:
        face_id.reshape(V, -1)[0, 6], face_id.reshape(V, -1)[0, 7] = -1, len(faces)
    return verts, faces, uv, tex, face_id, bary


# image sizes 1 x 1, 15 x 17, 16 x 16, 33 x 31; V = 1 and 3; C = 1, 3, 4
RENDER_CASES = [(1, 1, 1, 3), (1, 1, 3, 1), (15, 17, 1, 1), (15, 17, 3, 4), (16, 16, 1, 3), (16, 16, 3, 4), (33, 31, 3, 3), (33, 31, 1, 4),
                (33, 31, 3, 1)]


@pytest.mark.parametrize("H,W,V,C", RENDER_CASES)
def test_render_by_the_bits_of_the_restatement(T, H, W, V, C):
    from ls2fm.options import Options
    verts, faces, uv, tex, face_id, bary = render_case(H, W, V, C, H + V + C)
    background = [0.1, 0.2, 0.3, 0.4][:C]
    ref = TR.render(face_id, bary, uv, tex, background)
    if H * W > 8:
        assert np.isnan(ref[0, 0, 0, C - 1]) and (ref.reshape(V, -1, C)[0, 6:8] == np.array(background, F32)).all()
    atlas = T.build_atlas(dev(verts), dev(faces), texel=4.0, gutter=1)
    ras = Options(face_id=dev(face_id), bary=dev(bary))
    call = lambda: T.render_textured(atlas, dev(tex), ras, background)
    got = call()
    torch.cuda.synchronize()
    same(got, ref, "render")
    same(call(), ref, "render, rerun")
    same(T.render_textured_torch(atlas, dev(tex), ras, background), ref, "render, torch form")


def test_render_replay(T):
    from ls2fm.options import Options
    verts, faces, uv, tex, face_id, bary = render_case(33, 31, 3, 3, 5)
    ref = TR.render(face_id, bary, uv, tex, (0.0, 0.5, 1.0))
    atlas = T.build_atlas(dev(verts), dev(faces), texel=4.0, gutter=1)
    ras, t = Options(face_id=dev(face_id), bary=dev(bary)), dev(tex)
    graph, out = replay(lambda: T.render_textured(atlas, t, ras, (0.0, 0.5, 1.0)), lambda o: o)
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        same(out, ref, "render, replay")


def test_photo_texture_end_to_end_on_the_sphere_scene(T):
    """the restated sphere scene: the texture and the counts by their bits (the texels' points through mesh_colors_restate, depth
    from the restated rasteriser), unowned texels at fill, view chunks x row bands against one call, and the render of the result
    scored against the photographs next to the vertex-colour render of the same mesh.
    Recorded on MI355X: textured 24.10 dB, vertex colours 14.39 dB (no threshold is set; the condition is the order)."""
    from ls2fm import image_metrics, mesh_colors, raster
    sc, at, ref = TS.sphere_scene(), TS.sphere_atlas(), TS.sphere_texture()
    v, f, poses, K, images = (dev(sc[k]) for k in ("verts", "faces", "poses", "intr", "images"))
    atlas = T.build_atlas(v, f, texel=sc["texel"], gutter=sc["gutter"])
    assert atlas.size == at["size"] and list(atlas.classes) == at["table"]
    same(atlas.uv, at["uv"], "uv")
    kw = dict(near=sc["near"], depth_tol=sc["depth_tol"], power=sc["power"], fill=TS.SPHERE_FILL)
    one = T.photo_texture(v, f, atlas, poses, K, images, **kw)
    torch.cuda.synchronize()
    same(one.count, ref["count"], "count")
    same(one.texture, ref["texture"], "texture")
    unowned = dev(at["face"] < 0)
    assert bool(unowned.any()) and bool((one.count[unowned] == 0).all())
    assert bool((one.texture[unowned] == torch.tensor(TS.SPHERE_FILL, device=DEV)).all())
    split = T.photo_texture(v, f, atlas, poses, K, images, view_chunk=4, row_chunk=50, **kw)
    same(split.texture, ref["texture"], "texture, 2 view chunks x 3 row bands")
    same(split.count, ref["count"], "count, 2 view chunks x 3 row bands")
    given = T.photo_texture(v, f, atlas, poses, K, images, depth=dev(sc["depth"]), view_chunk=5, **kw)
    same(given.texture, ref["texture"], "texture, depth maps given")
    # the consumer side: both renders against the photographs, over the pixels the mesh covers
    H, W = sc["H"], sc["W"]
    ras = raster.rasterize(v, f, poses, K, H, W, near=sc["near"], bary=True)
    textured = T.render_views(v, f, atlas, one.texture, poses, K, H, W, near=sc["near"])
    same(textured, TR.render(ras.face_id.cpu().numpy(), ras.bary.cpu().numpy(), at["uv"], ref["texture"], (0.0, 0.0, 0.0)), "render_views")
    vc = mesh_colors.photo_colors(v, f, poses, K, images, normals=v, **kw).colors
    covered = ras.face_id >= 0
    corner = vc[f.long()[torch.where(covered, ras.face_id, torch.zeros_like(ras.face_id)).long()]]          # [N, H, W, 3, 3]
    interpolated = torch.where(covered[..., None], (ras.bary[..., None] * corner).sum(dim=-2), torch.zeros_like(textured))
    psnr_t = float(image_metrics.psnr(textured, images, mask=covered).mean())
    psnr_v = float(image_metrics.psnr(interpolated, images, mask=covered).mean())
    print(f"PSNR against the photographs over the covered pixels: textured {psnr_t:.2f} dB, vertex colours {psnr_v:.2f} dB")
    assert psnr_t > psnr_v


def test_field_texture_and_texture_mesh_on_the_device(T):
    """the field head-on at the owned texels and fill elsewhere, whatever the bands; texture_mesh is the photographs where a view
    counts and that field texture elsewhere (two of the six views: the far side is unseen)"""
    from ls2fm import mesh_colors
    from test_hip_radiance_points import _field
    opt, sdf, rad = _field("DTU", True)
    sc, at = TS.sphere_scene(), TS.sphere_atlas()
    v, f, poses, K, images = (dev(sc[k]) for k in ("verts", "faces", "poses", "intr", "images"))
    atlas = T.build_atlas(v, f, texel=sc["texel"], gutter=sc["gutter"])
    S = atlas.size
    field = T.field_texture(opt, sdf, rad, v, f, atlas, fill=(0.1, 0.2, 0.3))
    owned = dev(at["face"] >= 0)
    want = mesh_colors.field_colors(opt, sdf, rad, dev(at["point"])[owned])
    same(field[owned], want, "the field at the owned texels")
    assert bool((field[~owned] == torch.tensor([0.1, 0.2, 0.3], device=DEV)).all())
    same(T.field_texture(opt, sdf, rad, v, f, atlas, fill=(0.1, 0.2, 0.3), row_chunk=37), field, "field_texture in bands")
    kw = dict(near=sc["near"], depth_tol=sc["depth_tol"], power=sc["power"])
    both = T.texture_mesh(opt, sdf, rad, v, f, atlas, poses[:2], K, images[:2], **kw)
    photo = T.photo_texture(v, f, atlas, poses[:2], K, images[:2], **kw)
    default = T.field_texture(opt, sdf, rad, v, f, atlas)
    seen = photo.count > 0
    assert bool(seen.any()) and bool((~seen & owned).any()) and torch.equal(both.count, photo.count)
    same(both.texture[seen], photo.texture[seen], "photographs where seen")
    same(both.texture[~seen], default[~seen], "the field elsewhere")


def test_refusals_and_empty_calls(T):
    from ls2fm import _lib
    lib = _lib.load()
    verts, faces, rot, cls, order, table, S = restated("3", 1.0, 1, None)
    v, f, o, r = dev(verts), dev(faces), dev(order), dev(rot)
    face = torch.empty(S, S, dtype=torch.int32, device=DEV)
    point, normal = torch.empty(S, S, 3, device=DEV), torch.empty(S, S, 3, device=DEV)
    p, s = _lib.ptr, _lib.stream_ptr()
    ks_, counts_ = [k for k, _ in table], [c for _, c in table]

    def texels(verts=v, n_verts=len(verts), faces_=f, n_faces=len(faces), order_=o, rot_=r, ks=ks_, counts=counts_, gutter=1, size=S, r0=0,
               r1=S, face_=face, point_=point, normal_=normal):
        n = len(ks)
        return lib.ls2fm_texture_texels(p(verts), n_verts, p(faces_), n_faces, p(order_), p(rot_), n, (_lib.c_int32 * n)(*ks),
                                        (_lib.c_int64 * n)(*counts), gutter, size, r0, r1, p(face_), p(point_), p(normal_), p(None), s)
    assert texels() == 0
    for kw in (dict(verts=None), dict(faces_=None), dict(order_=None), dict(rot_=None), dict(face_=None), dict(point_=None),
               dict(normal_=None), dict(n_verts=-1), dict(n_faces=-1), dict(size=0), dict(size=24), dict(size=65536), dict(size=2),
               dict(r0=-1), dict(r0=5, r1=4), dict(r1=S + 1), dict(gutter=-1), dict(gutter=3), dict(ks=ks_[::-1], counts=counts_[::-1]),
               dict(ks=[3, 3], counts=[1, 2]), dict(ks=[], counts=[]), dict(ks=list(range(12, 3, -1)), counts=[0] * 8 + [3]),
               dict(counts=counts_[:-1] + [counts_[-1] + 1]), dict(counts=[-1] + counts_[1:]), dict(size=8)):
        assert texels(**kw) == -1, kw
    assert texels(r0=4, r1=4, face_=None, point_=None, normal_=None) == 0
    tex, out = torch.rand(S, S, 3, device=DEV), torch.empty(2, 5, 7, 3, device=DEV)
    face_id = torch.zeros(2, 5, 7, dtype=torch.int32, device=DEV)
    bary = torch.full((2, 5, 7, 3), 1.0 / 3.0, device=DEV)
    uv = dev(TR.chart_corners(order, rot, table, 1))
    bg = (_lib.c_float * 4)(0.0, 0.0, 0.0, 0.0)

    def render(fid=face_id, b=bary, V=2, H=5, W=7, uv_=uv, n_faces=len(faces), t=tex, size=S, C=3, bg_=bg, out_=out):
        return lib.ls2fm_texture_render(p(fid), p(b), V, H, W, p(uv_), n_faces, p(t), size, C, bg_, p(out_), s)
    assert render() == 0
    for kw in (dict(fid=None), dict(b=None), dict(uv_=None), dict(t=None), dict(bg_=None), dict(out_=None), dict(V=-1), dict(H=0),
               dict(W=32769), dict(n_faces=-1), dict(size=12), dict(size=2), dict(C=0), dict(C=5)):
        assert render(**kw) == -1, kw
    assert render(V=0, fid=None, b=None, out_=None) == 0 and render(n_faces=0, uv_=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                          # no faces: the background everywhere
    with pytest.raises(ValueError):
        T.atlas_texels(T.build_atlas(v, f, texel=1.0), v, f, rows=(0, S + 1))
