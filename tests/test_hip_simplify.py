"""GPU: ls2fm.simplify (csrc/mesh_simplify.hip) against the numpy restatement of THE CLUSTERING RULE (tests/simplify_restate.py) on
every vertex, face and cell of every scene of tests/simplify_scenes.py: keys, classes, counts, faces and vertex_map exactly, the
per-cell sums bit for bit in the stated order, vertices and colours by their bits (fp64 +, -, *, / and sqrt are IEEE on both sides
and nothing is contracted; no operation proved irreproducible)."""

import numpy as np
import pytest
import torch

import simplify_restate as R
import simplify_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENES = S.gpu_scenes()


@pytest.fixture(scope="module")
def SP():
    from ls2fm import simplify
    return simplify


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name, placement):
        if (name, placement) not in cache:
            sc = SCENES[name]
            cache[(name, placement)] = R.simplify(sc["verts"], sc["faces"], sc["cell"], sc["colors"], placement=placement)
        return cache[(name, placement)]
    return get


def on_device(sc):
    colors = None if sc["colors"] is None else torch.from_numpy(sc["colors"]).to(DEV)
    return torch.from_numpy(sc["verts"]).to(DEV), torch.from_numpy(sc["faces"]).to(DEV), colors


def run(SP, sc, placement):
    """simplify's own route, keeping the state -> (SimplifiedMesh, state)"""
    v, f, c = on_device(sc)
    code, reg = SP._options(placement, SP.DEFAULT_REG, "simplify")
    v, f, lib, ws_bytes = SP._prepare(v, f, "simplify")
    return SP._simplify_device(v, f, lib, ws_bytes, sc["cell"], c, code, reg)


def bits(t, kind):
    return t.detach().cpu().numpy().view(kind)


@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_simplify_matches_the_restatement(SP, restated, name, placement):
    sc, want = SCENES[name], restated(name, placement)
    got, st = run(SP, sc, placement)
    assert np.array_equal(st["vert_key"].cpu().numpy(), want["key"])
    assert np.array_equal(st["face_class"].cpu().numpy(), want["face_class"])
    assert (st["n_out"], st["n_surviving"], st["n_kept"]) == (len(want["vertices"]), want["n_surviving"], len(want["faces"]))
    assert np.array_equal(got.vertex_map.cpu().numpy(), want["vertex_map"])
    assert np.array_equal(got.faces.cpu().numpy(), want["faces"]) and got.faces.dtype == torch.int32
    assert np.array_equal(st["count"].cpu().numpy(), want["count"])
    sums = st["sums"].cpu().numpy()
    assert sums.shape == want["sums"].shape
    assert np.array_equal(sums.view(np.uint64), want["sums"].view(np.uint64))                  # the stated order, bit for bit
    bound = (want["n_terms"] + 16) * 2.0 ** -53 * want["abs_sums"]
    assert (np.abs(sums - want["own_sums"]) <= bound).all()                                     # and numpy's own order, to the bound
    assert np.array_equal(bits(got.vertices, np.uint32), want["vertices"].view(np.uint32))
    if sc["colors"] is None:
        assert got.colors is None
    else:
        assert np.array_equal(bits(got.colors, np.uint32), want["colors"].view(np.uint32))
    again, _ = run(SP, sc, placement)                                                           # a rerun gives the same bits
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", ["sphere_2.5", "sphere_dyadic_2", "soup_c3", "segments", "sized_256_512"])
def test_simplify_equals_the_torch_form(SP, restated, name):
    sc, want = SCENES[name], restated(name, "quadric")
    v, f, c = on_device(sc)
    got, st = run(SP, sc, "quadric")
    ref, sums, count = SP._simplify_torch(v, f, sc["cell"], c, return_sums=True)
    assert torch.equal(got.faces, ref.faces) and torch.equal(got.vertex_map, ref.vertex_map) and torch.equal(st["count"], count)
    bound = (want["n_terms"] + 16) * 2.0 ** -53 * want["abs_sums"]
    assert (np.abs(st["sums"].cpu().numpy() - sums.cpu().numpy()) <= bound).all()
    assert (got.vertices - ref.vertices).abs().max().item() <= 1e-5 * sc["cell"]


def test_public_calls(SP, restated):
    sc, want = SCENES["soup_c3"], restated("soup_c3", "quadric")
    v, f, c = on_device(sc)
    out = SP.simplify(v, f.long(), sc["cell"], colors=c)                                        # int64 faces are taken
    assert np.array_equal(bits(out.vertices, np.uint32), want["vertices"].view(np.uint32))
    assert np.array_equal(out.faces.cpu().numpy(), want["faces"])
    assert SP.count_faces(v, f, sc["cell"]) == want["n_surviving"]
    far = v.clone()
    far[0, 0] = 3.0e6
    with pytest.raises(ValueError, match="21 bits"):
        SP.simplify(far, f, sc["cell"])
    with pytest.raises(ValueError, match="21 bits"):
        SP.count_faces(far, f, sc["cell"])
    with pytest.raises(ValueError, match="outside"):
        SP.simplify(v, f + 1000, sc["cell"])
    with pytest.raises(ValueError, match="colors"):
        SP.simplify(v, f, sc["cell"], colors=c[:-1])


def test_simplify_to_faces(SP):
    v, f, _ = S.sphere_mesh(24, 8.3)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    out = SP.simplify_to_faces(tv, tf, 400)
    assert 0 < out.faces.shape[0] <= 400
    again = SP.simplify_to_faces(tv, tf, 400)
    assert torch.equal(out.faces, again.faces) and torch.equal(out.vertices.view(torch.int32), again.vertices.view(torch.int32))
    diagonal = float(np.sqrt(((v.max(axis=0).astype(np.float64) - v.min(axis=0)) ** 2).sum()))

    def count(cell):
        key, _, bad = R.vertex_keys(v, cell)
        return int((R.face_classes(key, f) == R.FACE_SURVIVES).sum()), int(bad.sum())
    want = R.simplify(v, f, SP._bisect_cell(count, diagonal, 400))
    assert np.array_equal(out.faces.cpu().numpy(), want["faces"])
    assert np.array_equal(bits(out.vertices, np.uint32), want["vertices"].view(np.uint32))


def _sphere_with_floater(pts):
    """the analytic field of tests/test_hip_mesh_components.py"""
    big = pts.norm(dim=1) - 0.3
    small = (pts - torch.tensor([0.5, 0.5, 0.5], device=pts.device)).norm(dim=1) - 0.05
    return torch.minimum(big, small)[:, None]


def test_the_mesh_export_simplifies_before_it_writes(SP, tmp_path):
    """get_surface_high_res_mesh(simplify=...) on the analytic field: the PLY read back equals simplify of the unsimplified export;
    simplify=None writes today's bytes"""
    from ls2fm import mesh
    from ls2fm.utils import plots
    plain, plain2, small, byfaces = (str(tmp_path / n) for n in ("plain.ply", "plain2.ply", "small.ply", "faces.ply"))
    kw = dict(resolution=64, grid_boundary=[-0.6, 0.6], take_components=True, backend="device")

    def export(path, **more):
        torch.manual_seed(0)
        return plots.get_surface_high_res_mesh(_sphere_with_floater, path=path, **kw, **more)
    full = export(plain)
    export(plain2, simplify=None)
    assert open(plain, "rb").read() == open(plain2, "rb").read()
    cell = 0.05
    out = export(small, simplify=cell)
    want = SP.simplify(full.vertices, full.faces, cell)
    gv, gf = mesh.read_ply_ascii(small)
    assert 0 < len(gf) < full.faces.shape[0] // 4 and isinstance(out, mesh.Mesh)
    assert np.array_equal(gv.view(np.uint32), bits(want.vertices, np.uint32)) and np.array_equal(gf, want.faces.cpu().numpy())
    assert torch.equal(out.faces, want.faces)
    export(byfaces, simplify={"faces": 500})
    assert 0 < len(mesh.read_ply_ascii(byfaces)[1]) <= 500
    with pytest.raises(ValueError, match="device"):
        plots.get_surface_high_res_mesh(_sphere_with_floater, path=small, simplify=cell, **dict(kw, backend="trimesh"))
    for bad in ({"faces": 10, "cell": 1.0}, {"cell": cell}, "0.05", True):
        with pytest.raises(ValueError, match="simplify="):
            SP.apply(full.vertices, full.faces, bad, "extract_mesh")


def _field(seed=0):
    """a freshly initialised DTU field with random tables and first-layer weights, as tests/test_hip_radiance_points.py builds it"""
    from ls2fm.models.RadF import RadF
    from ls2fm.models.SDF import SDF
    from ls2fm.options import make_options
    enc = dict(n_levels=8, n_features_per_level=2, log2_hashmap_size=14, base_resolution=16)
    opt = make_options("DTU", device="cuda", dual_field=True, sample_intvs=32, hash_encoding=enc)
    torch.manual_seed(seed)
    sdf, rad = SDF(opt).to("cuda"), RadF(opt).to("cuda")
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in (sdf, rad):
            for name, p in mod.named_parameters():
                if name.endswith("embedder_obj.params"):
                    p.copy_(((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1).to("cuda"))
                if name.endswith("mlp.0.weight_v") and "Rad_dec" not in name:
                    p[:, 3:] = (torch.randn(p[:, 3:].shape, generator=gen) * 0.05).to("cuda")
    return opt, sdf, rad


def test_extract_mesh_simplifies_before_it_colours_and_writes(SP, tmp_path):
    """extract_mesh(simplify=) on a field: None writes the bytes written without the keyword; a cell writes simplify of the
    marching-cubes mesh, vertices by their bits; {"faces": n} meets n; with colors= the colours are the field's at the SIMPLIFIED
    vertices; the skimage backend refuses the keyword"""
    from ls2fm import mesh, mesh_colors
    from ls2fm.utils import util
    opt, sdf, rad = _field()
    N = 32
    kw = dict(volume_size=2.0, N=N, backend="device")
    bare, none, small, auto, byfaces, coloured = (str(tmp_path / n) for n in ("bare.ply", "none.ply", "small.ply", "auto.ply", "faces.ply",
                                                                                "coloured.ply"))
    vol = util.extract_mesh(sdf, filepath=bare, **kw)
    util.extract_mesh(sdf, filepath=none, simplify=None, **kw)
    assert open(bare, "rb").read() == open(none, "rb").read()
    _, _, origin, sizes = util._lattice(2.0, N, None, None)
    v, f = mesh.marching_cubes(vol, level=0.0, spacing=[float(s) / N for s in sizes], origin=origin)
    v0, f0 = mesh.read_ply(bare)
    assert len(f0) > 100 and np.array_equal(v0.view(np.uint32), bits(v, np.uint32)) and np.array_equal(f0, f.cpu().numpy())
    cell = 3.0 * 2.0 / N
    want = SP.simplify(v, f, cell)
    util.extract_mesh(sdf, filepath=small, simplify=cell, **kw)
    gv, gf = mesh.read_ply(small)
    assert 0 < len(gf) < len(f0) // 2
    assert np.array_equal(gv.view(np.uint32), bits(want.vertices, np.uint32)) and np.array_equal(gf, want.faces.cpu().numpy())
    util.extract_mesh(sdf, volume_size=2.0, N=N, filepath=auto, simplify=cell)                   # "auto" goes to the device for it
    assert open(auto, "rb").read() == open(small, "rb").read()
    util.extract_mesh(sdf, filepath=byfaces, simplify={"faces": len(f0) // 4}, **kw)
    assert 0 < len(mesh.read_ply(byfaces)[1]) <= len(f0) // 4
    util.extract_mesh(sdf, filepath=coloured, simplify=cell, colors="field", rad_field=rad, **kw)
    cv, cf, cc = mesh.read_ply_colors(coloured)
    assert np.array_equal(cv.view(np.uint32), gv.view(np.uint32)) and np.array_equal(cf, gf)
    assert np.array_equal(cc, mesh.color_bytes(mesh_colors.field_colors(opt, sdf, rad, want.vertices), len(gv)))
    assert len(np.unique(cc, axis=0)) > 10
    with pytest.raises(ValueError, match="device"):
        util.extract_mesh(sdf, filepath=small, simplify=cell, **dict(kw, backend="skimage"))
