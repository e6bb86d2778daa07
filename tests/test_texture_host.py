"""Host: THE ATLAS RULE judged by its properties on the numpy restatement (tests/texture_restate.py) and on ls2fm.texture's torch forms
on CPU tensors, which must give the restatement's bits; the files; and what a texture atlas is for, measured on the restated sphere
scene (tests/texture_scenes.py): the texture resolves a pattern that vertex colours of the same mesh cannot."""
import os
import re

import numpy as np
import pytest
import torch

import mc_restate
import texture_restate as TR
import texture_scenes as TS
from ls2fm import _lib, texture

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, ref, what):
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    r = np.asarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, f"{what}: {g.dtype} {g.shape} != {r.dtype} {r.shape}"
    view = {1: np.uint8, 4: np.int32, 8: np.int64}[g.dtype.itemsize]
    bad = g.view(view) != r.view(view)
    if g.dtype.kind == "f":
        bad &= ~(np.isnan(g) & np.isnan(r))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ, the first at {tuple(np.argwhere(bad)[0])}"


# ------------------------------------------------------------------------------------------------------------------ the footprint
ADMISSIBLE = [(1 << k, g) for g in range(4) for k in range(2, 7) if (1 << k) >= 2 * g + 4]


@pytest.mark.parametrize("p,g", ADMISSIBLE)
def test_every_bilinear_tap_of_a_chart_point_is_owned_by_its_face(p, g):
    """exhaustively in integers: the points of the closed chart triangle on a 41 x 41 barycentric grid (corners, legs and
    hypotenuse included), both charts of the cell; a tap has non-zero weight iff its fraction on each axis is non-zero"""
    n = 40
    L = p - 2 * g - 3
    assert L >= 1
    a, b = np.mgrid[0:n + 1, 0:n + 1]
    keep = a + b <= n
    a, b = a[keep], b[keep]
    for second in (False, True):
        # texel-index coordinates (a texel's centre at its index) times n: chart A's corner at (g, g), legs of L texels
        un, vn = n * g + a * L, n * g + b * L
        if second:
            un, vn = n * (p - 1) - un, n * (p - 1) - vn
        for du in (0, 1):
            for dv in (0, 1):
                live = ((un % n != 0) | (du == 0)) & ((vn % n != 0) | (dv == 0))       # the upper tap weighs the fraction
                tu, tv = un // n + du, vn // n + dv
                inside = (tu >= 0) & (tu <= p - 1) & (tv >= 0) & (tv <= p - 1)
                owned = inside & ((tu + tv > p - 1) if second else (tu + tv <= p - 1))
                assert owned[live].all(), (p, g, second, du, dv)


def test_the_footprint_fails_one_texel_closer():
    """the test above can fail: with legs of L + 2 texels a hypotenuse point taps the other chart"""
    p, g, n = 8, 1, 40
    L = p - 2 * g - 3 + 2
    a = np.arange(n + 1)
    un, vn = n * g + a * L, n * g + (n - a) * L
    tu, tv = un // n + (un % n != 0), vn // n + (vn % n != 0)
    assert ((tu + tv) > p - 1).any()


# ------------------------------------------------------------------------------------------------------------------ the packing
def random_table(rng, gutter):
    ks = TR.class_range(gutter)
    return [(k, int(rng.integers(0, 9)) if rng.random() < 0.7 else 0) for k in reversed(ks)]


@pytest.mark.parametrize("seed", range(6))
def test_packing_cells_align_nothing_is_owned_twice_and_the_area_fits(seed):
    rng = np.random.default_rng(seed)
    gutter = seed % 3
    ks = TR.class_range(gutter)
    cls = rng.choice(ks[:4], size=int(rng.integers(1, 60))).astype(np.int32)
    if seed == 1:
        cls[cls == ks[1]] = ks[2]                                        # an empty class between two used ones
        cls = np.concatenate([cls, [ks[0], ks[2], ks[2], ks[2]]]).astype(np.int32)
        assert (cls == ks[1]).sum() == 0 and (cls == ks[0]).sum() and (cls == ks[2]).sum()
    order, table = TR.pack(cls, gutter)
    assert (np.diff(cls[order]) <= 0).all() and sorted(order) == list(range(len(cls)))
    for k in ks:                                                          # stable: the faces of a class keep their order
        assert (np.diff(order[cls[order] == k]) > 0).all()
    starts, cells, slots, area = TR.layout(table)
    S = TR.smallest_size(table)
    assert area <= S * S and (S == 4 or area > (S // 2) ** 2)
    for (k, count), start, n in zip(table, starts, cells):
        for c in range(n):
            off = start + (c << (2 * k))
            assert off % (1 << (2 * k)) == 0                             # Morton alignment of every cell
            x0, y0 = TR.deinterleave(off)
            assert x0 % (1 << k) == 0 and y0 % (1 << k) == 0 and x0 + (1 << k) <= S and y0 + (1 << k) <= S
    slot, ii, jj, kk, x, y = TR.owners(table, gutter, S)
    owned = slot[slot >= 0]
    per_slot = np.bincount(owned, minlength=len(cls))
    pitch = 1 << cls[order].astype(np.int64)
    # every slot owns half a cell: the diagonal i + j = p - 1 goes to chart A
    want = np.where(np.arange(len(cls)) - np.repeat(slots, [t[1] for t in table]) & 1, pitch * (pitch - 1) // 2, pitch * (pitch + 1) // 2)
    assert np.array_equal(per_slot, want)
    assert len(owned) == want.sum() <= area                               # no texel twice: the counts add up to the owned texels


def test_an_odd_slot_count_leaves_chart_b_unowned_and_the_tail_is_empty():
    table = [(4, 0), (3, 3)]
    slot, *_ = TR.owners(table, 0, 32)
    assert set(np.unique(slot)) == {-1, 0, 1, 2}
    cell1 = slot[0:8, 8:16]
    assert (cell1 == 2).sum() == 36 and (cell1 == -1).sum() == 28
    assert (slot[8:] == -1).all() and (slot[:8, 16:] == -1).all()


def test_uv_corners_are_half_integers_inside_their_cell_and_match_the_texels():
    verts, faces = TS.edge_mesh()
    for gutter in (0, 1, 2):
        rot, cls = TR.classify(verts, faces, 0.25, gutter)
        order, table = TR.pack(cls, gutter)
        S = TR.smallest_size(table)
        uv = TR.chart_corners(order, rot, table, gutter)
        assert np.array_equal(uv, TR.texels(verts, faces, order, rot, table, gutter, S)["uv"])
        assert np.array_equal(uv * 2 % 2, np.ones_like(uv))               # half-integers
        pitch = (1 << cls.astype(np.int64))[:, None]
        lo = np.floor(uv.min(axis=1) / pitch) * pitch                      # the cell of the first corner holds all three
        assert ((uv >= lo[:, None]) & (uv < (lo + pitch)[:, None])).all()
        L = pitch[:, 0] - 2 * gutter - 3
        legs = np.abs(uv - uv[np.arange(len(rot)), rot][:, None]).sum(axis=2)
        assert np.array_equal(np.sort(legs, axis=1), np.stack([0 * L, L, L], axis=1).astype(F32))


def test_rotation_ties_and_class_thresholds_at_exact_equality():
    verts, faces = TS.edge_mesh()
    rot, cls = TR.classify(verts, faces, 0.25, 1)
    assert rot[9] == 2 and rot[11] == 0                                    # the hypotenuse wins; a three-way tie goes to vertex 0
    assert len(set(cls.tolist())) >= 3 and cls[5] == 3 and cls[7] == 3    # NaN vertex, index out of range: the smallest class
    # a leg of exactly L texel is inside the class, one ulp more is the next class: legs along x so the fp32 difference is exact
    texel, gutter = 0.25, 1
    for k in TR.class_range(gutter)[:-1]:
        leg = ((1 << k) - 2 * gutter - 3) * texel
        for value, want in ((leg, k), (float(np.nextafter(F32(leg), F32(1e9))), k + 1)):
            v = np.array([[0, 0, 0], [value, 0, 0], [0, value / 2, 0]], F32)
            assert TR.classify(v, [[0, 1, 2]], texel, gutter)[1][0] == want, (k, value)
    big = np.array([[0, 0, 0], [1e6, 0, 0], [0, 1, 0]], F32)
    assert TR.classify(big, [[0, 1, 2]], texel, gutter)[1][0] == 8          # longer than the largest class: the largest


# ------------------------------------------------------------------------------------------------------------------ the module on CPU
@pytest.mark.parametrize("gutter", [0, 1, 2])
def test_build_atlas_and_the_torch_forms_give_the_restatements_bits_on_cpu(gutter):
    verts, faces = TS.edge_mesh()
    rot, cls = TR.classify(verts, faces, 0.25, gutter)
    order, table = TR.pack(cls, gutter)
    S = TR.smallest_size(table)
    atlas = texture.build_atlas(torch.from_numpy(verts), torch.from_numpy(faces), texel=0.25, gutter=gutter)
    assert atlas.size == S and list(atlas.classes) == table and atlas.gutter == gutter
    same(atlas.rot, rot, "rot")
    same(atlas.order, order, "order")
    same(atlas.uv, TR.chart_corners(order, rot, table, gutter), "uv")
    ref = TR.texels(verts, faces, order, rot, table, gutter, S)
    uv = torch.full((len(faces), 3, 2), float("nan"))
    got = texture.atlas_texels(atlas, torch.from_numpy(verts), torch.from_numpy(faces), uv=uv)
    for name in ("face", "point", "normal"):
        same(getattr(got, name), ref[name], name)
    same(uv, ref["uv"], "uv of the texels")
    band = texture.atlas_texels(atlas, torch.from_numpy(verts), torch.from_numpy(faces), rows=(5, S - 3))
    same(band.point, ref["point"][5:S - 3], "a band")
    # the render: barycentrics on vertices, on edges and inside, an empty pixel, a face id out of range, a NaN texel
    rng = np.random.default_rng(gutter)
    tex = rng.uniform(0, 1, (S, S, 3)).astype(F32)
    tex[int(ref["uv"][0, 0, 1]), int(ref["uv"][0, 0, 0])] = np.nan
    face_id = rng.integers(-1, len(faces) + 1, (2, 9, 7)).astype(np.int32)
    bary = rng.dirichlet([1, 1, 1], (2, 9, 7)).astype(F32)
    bary[0, 0, :3] = np.eye(3, dtype=F32)
    bary[0, 1, :3] = [[0.5, 0.5, 0], [0, 0.25, 0.75], [0.125, 0, 0.875]]
    face_id[0, :2, :3] = 0
    want = TR.render(face_id, bary, ref["uv"], tex, (0.1, 0.2, 0.3))
    from ls2fm.options import Options
    got = texture.render_textured(atlas, torch.from_numpy(tex), Options(face_id=torch.from_numpy(face_id), bary=torch.from_numpy(bary)), (0.1, 0.2, 0.3))
    same(got, want, "render")
    assert np.isnan(want[0, 0, 0]).all() and (want[face_id < 0] == np.array([0.1, 0.2, 0.3], F32)).all()


def test_size_given_bisects_the_texel_in_a_fixed_number_of_host_reads(monkeypatch):
    verts, faces = TS.icosphere(2)
    v, f = torch.from_numpy(verts), torch.from_numpy(faces)
    reads = []
    hist = texture._histogram
    monkeypatch.setattr(texture, "_histogram", lambda cls, ks: reads.append(1) or hist(cls, ks))
    atlas = texture.build_atlas(v, f, size=256)
    assert len(reads) == 1 + texture.BISECT_STEPS
    _, _, _, area = texture.layout(atlas.classes)
    assert area <= 256 * 256 and atlas.size == 256
    # the texel found fits, and one a little finer (the next class for the longest faces) does not fit or is no different
    again = texture.build_atlas(v, f, texel=atlas.texel, size=256)
    assert again.classes == atlas.classes and torch.equal(again.uv, atlas.uv)
    finer = texture.build_atlas(v, f, texel=atlas.texel * 0.5)
    assert finer.size > 256
    with pytest.raises(ValueError):
        texture.build_atlas(v, f, texel=atlas.texel * 0.5, size=256)
    with pytest.raises(ValueError):
        texture.build_atlas(v, f, size=32)                                  # 160 cells of pitch 8 need 10240 texels
    with pytest.raises(ValueError):
        texture.build_atlas(v, f)
    with pytest.raises(ValueError):
        texture.build_atlas(v, f, texel=0.1, size=48)


def test_field_texture_fills_the_unowned_texels_and_evaluates_the_owned_ones(monkeypatch):
    """the masking logic with a stub evaluator on the CPU: the field sees the owned texels' points, in order, and nothing else"""
    verts, faces = TS.small_mesh(3)
    v, f = torch.from_numpy(verts), torch.from_numpy(faces)
    atlas = texture.build_atlas(v, f, texel=0.5, gutter=1)
    seen = []

    def stub(opt, sdf_field, rad_field, points, *a, **kw):
        seen.append(points.clone())
        return points * 0.5 + 0.25
    monkeypatch.setattr(texture.mesh_colors, "field_colors", stub)
    out = texture.field_texture(None, None, None, v, f, atlas, fill=(0.1, 0.2, 0.3), row_chunk=5)
    tx = texture.atlas_texels(atlas, v, f)
    owned = tx.face >= 0
    assert owned.any() and not owned.all() and len(seen) > 1
    assert torch.equal(torch.cat(seen), tx.point[owned])
    assert torch.equal(out[owned], tx.point[owned] * 0.5 + 0.25)
    assert torch.equal(out[~owned], torch.tensor([0.1, 0.2, 0.3]).expand(int((~owned).sum()), 3))


# ------------------------------------------------------------------------------------------------------------------ files
def test_png_and_obj_round_trip_byte_for_byte(tmp_path):
    verts, faces = TS.small_mesh(3)
    v, f = torch.from_numpy(verts), torch.from_numpy(faces)
    atlas = texture.build_atlas(v, f, texel=0.5, gutter=1)
    rng = np.random.default_rng(3)
    for C in (1, 2, 3, 4):
        img = rng.uniform(-0.1, 1.1, (5, 7, C)).astype(F32)
        img[0, 0, 0] = np.nan
        texture.write_png(tmp_path / f"a{C}.png", img)
        back = texture.read_png(tmp_path / f"a{C}.png")
        assert back.dtype == np.uint8 and np.array_equal(back, texture.texture_bytes(img))
        assert back[0, 0, 0] == 0 and back.min() == 0 and back.max() == 255       # a NaN becomes 0; the values are clipped
        texture.write_png(tmp_path / f"b{C}.png", back)
        assert (tmp_path / f"a{C}.png").read_bytes() == (tmp_path / f"b{C}.png").read_bytes()
    from ls2fm import mesh
    col = rng.uniform(-0.5, 1.5, (64, 3))
    assert np.array_equal(texture.texture_bytes(col[None].astype(F32))[0], mesh.color_bytes(col.astype(F32), 64))
    tex = rng.uniform(0, 1, (atlas.size, atlas.size, 3)).astype(F32)
    paths = texture.write_obj(tmp_path / "m.obj", v, f, atlas, tex)
    got = texture.read_obj(tmp_path / "m.obj")
    same(got["verts"], verts, "verts")
    same(got["faces"], faces, "faces")
    same(got["uv"], atlas.uv, "uv")
    assert got["size"] == atlas.size and np.array_equal(got["texture"], texture.texture_bytes(tex))
    second = texture.write_obj(tmp_path / "n", got["verts"], got["faces"], atlas, got["texture"])
    for a, b in zip(paths, second):
        assert open(a, "rb").read().replace(b"m.", b"n.").replace(b" m\n", b" n\n") == open(b, "rb").read(), (a, b)
    text = open(paths[0]).read()
    assert text.count("\nvt ") == 3 * len(faces) and re.search(r"^f \d+/\d+ \d+/\d+ \d+/\d+$", text, re.M)


def test_the_abi_stays_13_and_the_header_declares_the_new_calls():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    assert re.search(r"#define\s+LS2FM_ABI_VERSION\s+13\b", header) and _lib.ABI_VERSION == 13
    assert _lib.load().ls2fm_abi_version() == 13
    for name in ("ls2fm_texture_texels", "ls2fm_texture_render"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert "THE ATLAS RULE" in header and "THE TEXTURE RENDER RULE" in header


# ------------------------------------------------------------------------------------------------------------------ what it is for
def test_marching_cubes_winds_its_faces_outward():
    """weights="face" counts the views with cos > 0 of the chart normal (b - a) x (c - a): on a marching-cubes surface (negative
    inside) that normal points out of the surface, toward the cameras"""
    ax = np.linspace(-1.0, 1.0, 12)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (np.sqrt(X * X + Y * Y + Z * Z) - 0.5).astype(F32)
    sp = 2.0 / 11
    v, f = mc_restate.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-1.0, -1.0, -1.0))
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * v[f].mean(axis=1)).sum(axis=1) > 0).all()


def test_the_texture_resolves_a_pattern_the_vertex_colours_cannot():
    """on the restatement alone: the coarse sphere under six cameras, photographs of a pattern of 0.25 wavelength.  At 28 sample
    points per face the textured colour (the bilinear atlas sample) and the interpolated vertex colour are compared with the
    pattern at the radially projected point.  Measured: mean squared error 0.00097 against 0.0299, a ratio of 0.032."""
    sc, at, tex = TS.sphere_scene(), TS.sphere_atlas(), TS.sphere_texture()
    vc = TS.sphere_vertex_colors()
    assert at["size"] == 128 and (at["cls"] == 3).all()
    owned = at["face"] >= 0
    assert (tex["count"][owned] > 0).all()                                   # six axis cameras see every texel of a sphere
    assert (tex["texture"][~owned] == np.array(TS.SPHERE_FILL, F32)).all() and (tex["count"][~owned] == 0).all()
    v, f = sc["verts"], sc["faces"]
    B = TS.face_samples(6)
    bary = np.broadcast_to(B[None], (len(f), len(B), 3))
    P = (bary[..., None] * v[f][:, None].astype(np.float64)).sum(axis=2)
    truth = TS.pattern(P / np.linalg.norm(P, axis=-1, keepdims=True) * TS.SPHERE_R)
    x, y = TR.texture_point(bary, at["uv"][:, None])
    textured = TR.sample(tex["texture"], x, y).astype(np.float64)
    interpolated = (bary[..., None] * vc[f][:, None].astype(np.float64)).sum(axis=2)
    mse_t, mse_v = ((textured - truth) ** 2).mean(), ((interpolated - truth) ** 2).mean()
    print(f"texture mse {mse_t:.3e}, vertex colours {mse_v:.3e}, ratio {mse_t / mse_v:.4f}")
    assert mse_t < mse_v
