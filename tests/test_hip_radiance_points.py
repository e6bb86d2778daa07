"""GPU: ls2fm_radiance_points (csrc/radiance_points.hip) through ls2fm.mesh_colors: sdf and g by their bits against the existing
point queries, rgb against the CPU oracle and the torch composition at the project's parity bar, determinism and capture, the
configurations the kernel refuses, and the coloured-mesh exports built on it."""
import numpy as np
import pytest
import torch

import mesh_colors_restate as MR
import mesh_colors_scenes as S
from ls2fm import _lib, fused, mesh, mesh_colors
from ls2fm.models.RadF import RadF
from ls2fm.models.Renderer import Renderer  # noqa: F401  (the composition the kernel restates lives there)
from ls2fm.models.SDF import SDF
from ls2fm.options import make_options
from ls2fm.utils import plots, util

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 256          # LS2FM_RADIANCE_POINTS_TILE
PARITY = 1e-4       # the README's bar for fp32 results against the oracle


def _field(ds="DTU", dual=True, levels=8, log2=14, seed=0):
    """a field with random tables and first-layer weights, as the render tests build it"""
    enc = dict(n_levels=levels, n_features_per_level=2, log2_hashmap_size=log2, base_resolution=16)
    opt = make_options(ds, device=DEV, dual_field=dual, sample_intvs=32, hash_encoding=enc)
    torch.manual_seed(seed)
    sdf, rad = SDF(opt).to(DEV), RadF(opt).to(DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in (sdf, rad):
            for name, p in mod.named_parameters():
                if name.endswith("embedder_obj.params"):
                    p.copy_(((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1).to(DEV))
                if name.endswith("mlp.0.weight_v") and "Rad_dec" not in name:
                    p[:, 3:] = (torch.randn(p[:, 3:].shape, generator=gen) * 0.05).to(DEV)
    return opt, sdf, rad


def _points(opt, n=257, seed=5):
    """n points of the scene box: its eight corners, points on each of its six faces, the rest inside"""
    h = float(opt.data.bound_max[0])
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(n, 3, generator=g) * 2 - 1) * h * 0.999
    corners = torch.tensor([[sx, sy, sz] for sx in (-h, h) for sy in (-h, h) for sz in (-h, h)])
    p[:8] = corners
    for a in range(3):
        p[8 + 2 * a, a] = -h
        p[9 + 2 * a, a] = h
    d = torch.randn(n, 3, generator=g)
    d[::7] *= 3.0            # directions are a ray's: not unit
    return p, d


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _oracle(ds, dual, levels, log2, sdf, rad, p, d, dtype=torch.float32):
    """the oracle chain infer_sdf, sdf_gradient, fourier_embed, geometry_feat, radiance_mlp on the CPU -> (rgb, g)"""
    from oracle import fields as OF
    cfg = OF.dataset_config(ds, dual_field=dual, sample_intvs=32, n_levels=levels, log2_hashmap_size=log2)
    table = cfg.table()
    osd = {k: v.detach().cpu().to(dtype) for k, v in sdf.state_dict().items()}
    ord_ = {k: v.detach().cpu().to(dtype) for k, v in rad.state_dict().items()}
    p = p.detach().cpu().to(dtype)
    _, feats = OF.infer_sdf(p, osd, cfg, table, "ret_all")
    g = OF.sdf_gradient(p.clone(), osd, cfg, table).detach()
    v = -torch.nn.functional.normalize(g, dim=-1) if d is None else d.detach().cpu().to(dtype)
    geo = feats[..., 1:]
    if dual:
        geo = torch.cat([geo, OF.geometry_feat(p, ord_, cfg, table)[..., 1:]], dim=-1)
    with torch.no_grad():
        rgb = OF.radiance_mlp(torch.cat([p, g, OF.fourier_embed(v), geo.detach()], dim=-1), ord_)
    return rgb, g


@pytest.mark.parametrize("ds,dual", [("DTU", True), ("ETH3D", False), ("BlendedMVS", True)])
@pytest.mark.parametrize("given_dirs", [True, False])
def test_points_against_the_queries_the_oracle_and_the_composition(ds, dual, given_dirs):
    opt, sdf, rad = _field(ds, dual)
    p_cpu, d_cpu = _points(opt)
    p, d = p_cpu.to(DEV), (d_cpu.to(DEV) if given_dirs else None)
    o_rgb, o_g = _oracle(ds, dual, 8, 14, sdf, rad, p_cpu, d_cpu if given_dirs else None)
    comp_rgb, comp_g = mesh_colors.field_colors_composed(opt, sdf, rad, p, d, return_normals=True)
    assert mesh_colors.can_eval_field(opt, sdf, rad, p)
    for n in (0, 1, TILE - 1, TILE, TILE + 1, 257):
        rgb, g, s = mesh_colors.field_points(opt, sdf, rad, p[:n], None if d is None else d[:n])
        assert rgb.shape == (n, 3) and g.shape == (n, 3) and s.shape == (n,)
        if n == 0:
            continue
        q_sdf, _, q_g = fused.sdf_eval(sdf, p[:n], want_normal=True)
        assert torch.equal(s.view(torch.int32), q_sdf.reshape(-1).view(torch.int32)), f"sdf bits, n = {n}"
        assert torch.equal(g.view(torch.int32), q_g.view(torch.int32)), f"normal bits, n = {n}"
        assert bool(((rgb >= 0) & (rgb <= 1)).all())
        assert _rel(rgb, o_rgb[:n]) < PARITY, f"rgb against the oracle, n = {n}: {_rel(rgb, o_rgb[:n]):.2e}"
        assert _rel(g, o_g[:n]) < PARITY, f"g against the oracle, n = {n}: {_rel(g, o_g[:n]):.2e}"
        assert _rel(rgb, comp_rgb[:n]) < PARITY, f"rgb against the composition, n = {n}: {_rel(rgb, comp_rgb[:n]):.2e}"
    # the public call: any leading shape, the same bits
    rgb2, g2 = mesh_colors.field_colors(opt, sdf, rad, p.view(1, 257, 3), None if d is None else d.view(1, 257, 3), return_normals=True)
    assert rgb2.shape == (1, 257, 3) and torch.equal(rgb2[0], rgb) and torch.equal(g2[0], g)
    assert float((rgb.max(dim=0).values - rgb.min(dim=0).values).min()) > 1e-3, "the field's colour must vary over the points"


@pytest.mark.parametrize("kernel", ["1", "2"])
def test_sdf_and_normal_bits_against_each_point_query_kernel(kernel, monkeypatch):
    """ls2fm_sdf_eval picks the 16-lanes-per-point kernel at this size; LS2FM_POINTS_KERNEL forces the thread-per-point one (1),
    whose normal statements csrc/sdf_point.h's lane_normal repeats, or the 16-lane one (2)"""
    opt, sdf, rad = _field("BlendedMVS", True)
    p, _ = _points(opt)
    p = p.to(DEV)
    _, g, s = mesh_colors.field_points(opt, sdf, rad, p)
    monkeypatch.setenv("LS2FM_POINTS_KERNEL", kernel)
    q_sdf, _, q_g = fused.sdf_eval(sdf, p, want_normal=True)
    assert torch.equal(s.view(torch.int32), q_sdf.reshape(-1).view(torch.int32))
    assert torch.equal(g.view(torch.int32), q_g.view(torch.int32))


def test_one_direction_for_all_points_and_direction_dependence():
    opt, sdf, rad = _field("DTU", True)
    p, d = _points(opt)
    p = p.to(DEV)
    one = torch.tensor([0.3, -0.5, 0.8], device=DEV)
    a = mesh_colors.field_colors(opt, sdf, rad, p, one)
    b = mesh_colors.field_colors(opt, sdf, rad, p, one.expand(257, 3).contiguous())
    c = mesh_colors.field_colors(opt, sdf, rad, p, -one)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_rerun_and_graph_replay_are_bit_identical():
    opt, sdf, rad = _field("DTU", True)
    p, _ = _points(opt)
    p = p.to(DEV)
    call = lambda: mesh_colors.field_points(opt, sdf, rad, p)
    eager = call()
    again = call()
    for a, b in zip(eager, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(2):
        for t in out:
            t.fill_(-3.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, out):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bg_sdf_and_cpu_take_the_composition():
    opt, sdf, rad = _field("DTU", True)
    opt.data.bg_sdf = True
    p, d = _points(opt)
    p, d = p.to(DEV), d.to(DEV)
    assert not mesh_colors.can_eval_field(opt, sdf, rad, p)
    with pytest.raises(RuntimeError, match="composed"):
        mesh_colors.field_points(opt, sdf, rad, p)
    got, g = mesh_colors.field_colors(opt, sdf, rad, p, d, return_normals=True)
    want, wg = mesh_colors.field_colors_composed(opt, sdf, rad, p, d, return_normals=True)
    # the composition itself does not repeat its bits from call to call (its autograd normal), so: the parity bar, and the oracle
    print(f"bg_sdf: field_colors against the composition rgb {_rel(got, want):.2e}, g {_rel(g, wg):.2e}")
    assert got.shape == (257, 3) and _rel(got, want) < PARITY and _rel(g, wg) < PARITY
    from oracle import fields as OF
    cfg = OF.dataset_config("DTU", dual_field=True, sample_intvs=32, n_levels=8, log2_hashmap_size=14, bg_sdf=True)
    assert cfg.inside and float(opt.data.bg_rad) == cfg.bg_rad
    o_g = OF.sdf_gradient(p.cpu().clone(), {k: v.detach().cpu() for k, v in sdf.state_dict().items()}, cfg, cfg.table()).detach()
    assert _rel(g, o_g) < PARITY, "the composition applies the background sphere's min"
    # the library itself refuses the configuration before any device work
    lib = _lib.load()
    fdesc = fused.field_desc(opt)
    assert fdesc.bg_sdf == 1
    ts, dual = fused.param_tensors(sdf, rad)
    ps = fused._params_struct([t.detach().contiguous() for t in ts], dual, float(sdf.beta_speed))
    g1, g2 = sdf.embed_fn.embedder_obj.desc, rad.embed_fn.embedder_obj.desc
    import ctypes
    rgb = torch.empty(257, 3, device=DEV)
    ws = torch.empty(int(lib.ls2fm_radiance_points_workspace_bytes()), dtype=torch.uint8, device=DEV)
    st = lambda f, n=257, pts=p, out=rgb, w=ws: lib.ls2fm_radiance_points(ctypes.byref(f), ctypes.byref(g1), ctypes.byref(g2), ctypes.byref(ps), _lib.ptr(pts),
                                                                         _lib.ptr(None), n, _lib.ptr(out), _lib.ptr(None), _lib.ptr(None), _lib.ptr(w),
                                                                         _lib.stream_ptr())
    assert st(fdesc) == -2
    fdesc.bg_sdf = 0
    assert st(fdesc, n=-1) == -1 and st(fdesc, pts=None) == -1 and st(fdesc, out=None) == -1 and st(fdesc, w=None) == -4
    assert st(fdesc, n=0, pts=None, out=None, w=None) == 0 and st(fdesc) == 0
    torch.cuda.synchronize()


def test_extract_mesh_writes_the_field_colours(tmp_path):
    opt, sdf, rad = _field("DTU", True)
    bare, path = str(tmp_path / "bare.ply"), str(tmp_path / "field.ply")
    util.extract_mesh(sdf, volume_size=2.0, N=32, filepath=bare, backend="device")
    util.extract_mesh(sdf, volume_size=2.0, N=32, filepath=path, backend="device", colors="field", rad_field=rad)
    v0, f0 = mesh.read_ply(bare)
    v, f, c = mesh.read_ply_colors(path)
    assert len(v) > 100 and np.array_equal(v, v0) and np.array_equal(f, f0), "the geometry is what the bare call writes"
    want = mesh.color_bytes(mesh_colors.field_colors(opt, sdf, rad, torch.from_numpy(v).to(DEV)), len(v))
    assert c.shape == (len(v), 3) and np.array_equal(c, want)
    assert len(np.unique(c, axis=0)) > 10
    util.extract_mesh(sdf, volume_size=2.0, N=32, filepath=path, backend="device", colors=lambda a, b: torch.full((a.shape[0], 4), 0.5))
    assert mesh.read_ply_colors(path)[2].tolist() == [[128, 128, 128, 128]] * len(v)
    with pytest.raises(ValueError):
        util.extract_mesh(sdf, volume_size=2.0, N=32, filepath=path, backend="device", colors="field")


def test_high_res_mesh_writes_the_field_colours(tmp_path):
    opt, sdf, rad = _field("DTU", True)
    path = str(tmp_path / "high.ply")
    torch.manual_seed(0)
    m = plots.get_surface_high_res_mesh(sdf.infer_sdf, resolution=24, grid_boundary=(-1.0, 1.0), path=path, backend="device",
                                        colors="field", rad_field=rad)
    v, f, c = mesh.read_ply_colors(path)
    assert m is not None and len(v) == m.vertices.shape[0] and c.shape == (len(v), 3)
    want = mesh.color_bytes(mesh_colors.field_colors(opt, sdf, rad, m.vertices), len(v))
    assert np.array_equal(c, want)


def test_color_mesh_is_photographs_where_seen_and_the_field_elsewhere():
    sc = S.sphere_scene()
    opt, sdf, rad = _field("DTU", True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    verts, faces = dev(sc["verts"]), dev(sc["faces"])
    views = slice(0, 2)                                             # two cameras on one axis' ends leave a band unseen
    poses, intr, images = dev(sc["poses"][views]), dev(sc["intr"]), dev(sc["images"][views])
    got = mesh_colors.color_mesh(opt, sdf, rad, verts, faces, poses, intr, images, depth_tol=sc["depth_tol"], power=1)
    rgb, g = mesh_colors.field_colors(opt, sdf, rad, verts, return_normals=True)
    photo = mesh_colors.photo_colors(verts, faces, poses, intr, images, normals=g, depth_tol=sc["depth_tol"], power=1)
    seen = photo.count > 0
    assert torch.equal(got.count, photo.count) and 0 < int(seen.sum()) < len(seen)
    assert torch.equal(got.colors[seen], photo.colors[seen]) and torch.equal(got.colors[~seen], rgb[~seen])
    # and the photographs' part is the restatement's, with the field's normals
    ref = MR.vertex_colors(sc["verts"], sc["poses"][views], sc["intr"], sc["images"][views], sc["depth"][views], normals=g.cpu().numpy(),
                           near=1e-3, depth_tol=sc["depth_tol"], power=1, fallback=rgb.cpu().numpy())
    assert np.array_equal(got.count.cpu().numpy(), ref["count"])
    assert np.array_equal(got.colors.cpu().numpy().view(np.int32), ref["colors"].view(np.int32))
