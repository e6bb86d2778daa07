"""GPU: ls2fm_tsdf_integrate (csrc/tsdf_fusion.hip) through ls2fm.fusion, every lattice point's tsdf and weight by their bits against
the numpy restatement (tests/fusion_restate.py), and extract / fuse_mesh on top of it.  The rule itself, and that the scenes
meet its edges, is judged on the restatement (tests/test_fusion_host.py)."""
import numpy as np
import pytest
import torch

import fusion_restate as FR
import fusion_scenes as S
import mc_restate
import mesh_colors_scenes

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


@pytest.fixture(scope="module")
def FU():
    from ls2fm import fusion
    return fusion


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same(got, ref, what):
    """bit for bit; a NaN matches a NaN (its sign and payload are the one thing IEEE 754 leaves to the implementation)"""
    g, r = host(got), host(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, f"{what}: {g.dtype} {g.shape} != {r.dtype} {r.shape}"
    view = {4: np.int32, 8: np.int64}[g.dtype.itemsize]
    bad = g.view(view) != r.view(view)
    if g.dtype.kind == "f":
        bad &= ~(np.isnan(g) & np.isnan(r))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ, the first at {tuple(np.argwhere(bad)[0])}"


def volume(FU, sc):
    return FU.TsdfVolume(sc["shape"], sc["origin"], sc["voxel"], sc["trunc"], DEV)


def on_device(FU, sc, views=slice(None), vol=None, weighted=True, view_weight=None):
    """integrate the views `views` of a scene into a (fresh) device volume"""
    vol = volume(FU, sc) if vol is None else vol
    kw = dict(max_depth=sc["max_depth"], max_weight=sc["max_weight"], view_weight=dev(sc["view_weight"][views])) if weighted else {}
    if view_weight is not None:
        kw["view_weight"] = dev(view_weight)
    return FU.integrate(vol, dev(sc["depth"][views]), dev(sc["poses"][views]), dev(sc["intr"][views]), near=sc["near"], **kw)


def restated(sc, views=slice(None), weighted=True, view_weight=None):
    kw = dict(max_depth=sc["max_depth"], max_weight=sc["max_weight"], view_weight=sc["view_weight"][views]) if weighted else {}
    if view_weight is not None:
        kw["view_weight"] = view_weight
    return FR.fuse(sc["shape"], sc["origin"], sc["voxel"], sc["trunc"], sc["depth"][views], sc["poses"][views], sc["intr"][views],
                   near=sc["near"], **kw)


def check(vol, ref, what=""):
    torch.cuda.synchronize()
    same(vol.tsdf, ref[0], f"tsdf {what}")
    same(vol.weight, ref[1], f"weight {what}")


BX, BY, BZ = S.BRICK
# shape, H, W, V: nz = 1, 2, 63, 64, 65; nx and ny one below, at and one past the brick's sides; V = 0, 1, 3; 5 x 7 to 33 x 17
CASES = [((BX - 1, BY - 1, 1), 5, 7, 3), ((BX, BY + 1, 2), 5, 7, 1), ((BX + 1, BY, BZ - 1), 7, 5, 3), ((BX, BY, BZ), 17, 33, 3),
         ((BX + 1, BY + 1, BZ + 1), 17, 33, 3), ((BX + 1, BY - 1, BZ + 1), 33, 17, 1), ((BX - 1, BY + 1, BZ), 33, 17, 3),
         ((BX + 1, BY + 1, BZ + 1), 5, 7, 0), ((2 * BX + 1, 2 * BY + 1, 2 * BZ + 1), 33, 17, 3)]


@pytest.mark.parametrize("shape,H,W,V,nan_pose", [c + (False,) for c in CASES] + [c + (True,) for c in CASES if c[3] == 3])
def test_bits_of_the_restatement(FU, shape, H, W, V, nan_pose):
    sc = S.edge_scene(shape, H, W, 3, nan_pose)
    check(on_device(FU, sc, slice(0, V)), restated(sc, slice(0, V)))


def test_without_weights_and_bounds(FU):
    sc = S.edge_scene((BX + 1, BY + 1, BZ + 1), 17, 33)
    ref = restated(sc, weighted=False)
    check(on_device(FU, sc, weighted=False), ref)
    assert (ref[1] == 3).any() and (ref[0] == 1).any()


@pytest.mark.parametrize("weights", [(0.0, -1.0, np.nan), (np.nan, 0.75, -0.0), (2.0, np.inf, 0.25)])
def test_view_weights(FU, weights):
    sc = S.edge_scene((BX + 1, BY + 1, BZ + 1), 17, 33)
    w = np.array(weights, F32)
    ref = restated(sc, view_weight=w)
    check(on_device(FU, sc, view_weight=w), ref)
    if not (w > 0).any():
        assert not ref[1].any()


def test_one_view_per_call_a_rerun_and_a_replay(FU):
    sc = S.edge_scene((BX + 1, BY + 1, BZ + 1), 17, 33)
    ref = restated(sc)
    whole = on_device(FU, sc)
    check(whole, ref, "one call")
    split = volume(FU, sc)
    for i in range(3):
        on_device(FU, sc, slice(i, i + 1), vol=split)
    check(split, ref, "one view per call")
    check(on_device(FU, sc), ref, "rerun")
    # a captured call: the volume is the graph's own, cleared before every replay
    vol = volume(FU, sc)
    args = (dev(sc["depth"]), dev(sc["poses"]), dev(sc["intr"]))
    kw = dict(near=sc["near"], max_depth=sc["max_depth"], max_weight=sc["max_weight"], view_weight=dev(sc["view_weight"]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        FU.integrate(vol, *args, **kw)                              # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        FU.integrate(vol, *args, **kw)
    for _ in range(2):
        vol.tsdf.zero_()
        vol.weight.zero_()
        graph.replay()
        check(vol, ref, "replay")


def test_depth_as_trace_image_returns_it(FU):
    sc = S.edge_scene((BX + 1, BY + 1, BZ + 1), 17, 33)
    vol = volume(FU, sc)
    FU.integrate(vol, dev(sc["depth"]).reshape(3, 17 * 33, 1), dev(sc["poses"]), dev(sc["intr"]), near=sc["near"], H=17, W=33)
    check(vol, restated(sc, weighted=False))
    with pytest.raises(ValueError):
        FU.integrate(vol, dev(sc["depth"])[:2], dev(sc["poses"]), dev(sc["intr"]))
    with pytest.raises(RuntimeError):
        FU.integrate(vol, torch.from_numpy(sc["depth"]), dev(sc["poses"]), dev(sc["intr"]))


def test_extract_equals_the_restated_route(FU):
    """the analytic sphere: the device state by its bits, then extract's vertices and faces against marching cubes' restatement
    on the restated state with the same face filter"""
    sc = S.sphere_scene(24, 64)
    ref = FR.fuse(sc["shape"], sc["origin"], sc["voxel"], sc["trunc"], sc["depth"], sc["poses"], sc["intr"], near=sc["near"])
    vol = FU.integrate(volume(FU, sc), dev(sc["depth"]), dev(sc["poses"]), dev(sc["intr"]), near=sc["near"])
    check(vol, ref)
    for min_weight in (1.0, 2.0):
        v, f = FR.extract(ref[0], ref[1], sc["origin"], sc["voxel"], min_weight)
        out = FU.extract(vol, min_weight)
        assert out.faces.dtype == torch.int32 and len(f) > 500
        same(out.vertices, v, "vertices")
        same(out.faces, f, "faces")
    # the filter has work to do: the raw mesh at min_weight = 2 has faces on unobserved corners
    raw = np.where(ref[1] >= 2, ref[0], np.nan).astype(F32)
    assert not np.isfinite(mc_restate.marching_cubes(raw, 0.0, (sc["voxel"],) * 3, sc["origin"])[0]).all()


def test_fuse_mesh_on_the_marching_cubes_sphere(FU):
    """the marching-cubes sphere of radius 0.5 under its six cameras (tests/mesh_colors_scenes.py): every vertex of the re-fused
    mesh is finite and within one voxel of the sphere; the volume carries the bits of the restated route from the restated
    rasterisation; one view per chunk, and the bounds given, give the same mesh"""
    sc = mesh_colors_scenes.sphere_scene()
    voxel = 0.05
    args = [dev(sc[k]) for k in ("verts", "faces", "poses", "intr")]
    out, vol = FU.fuse_mesh(*args, sc["H"], sc["W"], voxel, near=sc["near"], return_volume=True)
    torch.cuda.synchronize()
    v = host(out.vertices).astype(np.float64)
    assert out.faces.shape[0] > 1000 and np.isfinite(v).all()
    assert (np.abs(np.linalg.norm(v, axis=1) - 0.5) <= voxel).all()
    assert vol.trunc == FU.TRUNC_VOXELS * voxel and min(vol.shape) >= 2
    lo = sc["verts"].min(axis=0).astype(np.float64) - vol.trunc
    assert np.allclose(vol.origin, lo, rtol=0, atol=1e-12)
    ref = FR.fuse(vol.shape, vol.origin, voxel, vol.trunc, sc["depth"], sc["poses"], sc["intr"], near=sc["near"])
    check(vol, ref)
    rv, rf = FR.extract(ref[0], ref[1], vol.origin, voxel)
    same(out.vertices, rv, "vertices")
    same(out.faces, rf, "faces")
    chunked = FU.fuse_mesh(*args, sc["H"], sc["W"], voxel, near=sc["near"], max_workspace_bytes=1)
    same(chunked.vertices, out.vertices, "vertices, one view per chunk")
    same(chunked.faces, out.faces, "faces, one view per chunk")
    again = FU.fuse_mesh(*args, sc["H"], sc["W"], voxel, near=sc["near"], bounds=(vol.origin, [o + voxel * (n - 1.5) for o, n in zip(vol.origin, vol.shape)]))
    same(again.vertices, out.vertices, "vertices, the bounds given")
    same(again.faces, out.faces, "faces, the bounds given")


def test_fuse_field_is_trace_image_where_integrate_extract(FU):
    """a converging field (the geometric initialisation, a small table) under three views: the volume and the mesh carry the bits
    of the restated route from trace_image's depth with the pixels that did not finish at +inf; one view per chunk likewise"""
    from ls2fm import image
    from test_hip_trace_image import _field, _views
    opt, sdf = _field("DTU", True, levels=8, log2=14, seed=7, table_amp=0.002, w_std=0.0)
    H, W = 24, 32
    poses, intr = _views(opt, H, W, V=3)
    lo, hi = [float(v) for v in opt.data.bound_min], [float(v) for v in opt.data.bound_max]
    voxel = (hi[0] - lo[0]) / 23
    out, vol = FU.fuse_field(sdf, poses, intr, H, W, voxel, (lo, hi), return_volume=True)
    t = image.trace_image(sdf, poses, intr, H=H, W=W)
    torch.cuda.synchronize()
    finish = host(t.finish).reshape(3, H, W)
    assert finish.any() and not finish.all(), "both kinds of pixel occur"
    depth = np.where(finish, host(t.depth).reshape(3, H, W), np.inf).astype(F32)
    ref = FR.fuse(vol.shape, vol.origin, voxel, vol.trunc, depth, host(poses), host(intr), near=1e-3)
    check(vol, ref)
    assert ref[1].any()
    rv, rf = FR.extract(ref[0], ref[1], vol.origin, voxel)
    same(out.vertices, rv, "vertices")
    same(out.faces, rf, "faces")
    chunked = FU.fuse_field(sdf, poses, intr, H, W, voxel, (lo, hi), max_workspace_bytes=1)
    same(chunked.vertices, rv, "vertices, one view per chunk")
    same(chunked.faces, rf, "faces, one view per chunk")


def test_refusals_and_empty_calls(FU):
    from ls2fm import _lib
    lib = _lib.load()
    sc = S.edge_scene((BX + 1, BY + 1, 4), 5, 7)
    tsdf = torch.zeros(sc["shape"], device=DEV)
    weight = torch.zeros(sc["shape"], device=DEV)
    from ls2fm import _posed
    poses, k4 = _posed.views(dev(sc["poses"]), dev(sc["intr"]), "test")
    depth = dev(sc["depth"])
    p, s = _lib.ptr, _lib.stream_ptr()
    origin = (3 * _lib.c_float)(*sc["origin"])
    inf, nan = float("inf"), float("nan")

    def call(t=tsdf, w=weight, shape=sc["shape"], og=origin, voxel=0.25, trunc=0.5, d=depth, ps=poses, k=k4, n_views=3, H=5, W=7,
             near=0.5, max_depth=inf, max_weight=inf):
        return lib.ls2fm_tsdf_integrate(p(t), p(w), *shape, og, voxel, trunc, p(d), p(ps), p(k), p(None), n_views, H, W, near, max_depth,
                                        max_weight, s)
    assert call() == 0
    torch.cuda.synchronize()
    before = (tsdf.clone(), weight.clone())
    assert bool(before[1].any())
    bad_origin = (3 * _lib.c_float)(0.0, nan, 0.0)
    for kw in (dict(t=None), dict(w=None), dict(d=None), dict(ps=None), dict(k=None), dict(og=None), dict(og=bad_origin),
               dict(shape=(-1, 3, 4)), dict(shape=(3, 3, 2 ** 24 + 1)), dict(n_views=-1), dict(H=0), dict(W=32769), dict(near=0.0),
               dict(near=nan), dict(near=inf), dict(voxel=0.0), dict(voxel=-0.25), dict(voxel=inf), dict(voxel=nan), dict(trunc=0.0),
               dict(trunc=inf), dict(trunc=nan), dict(max_depth=0.0), dict(max_depth=nan), dict(max_depth=-1.0), dict(max_weight=0.0),
               dict(max_weight=nan)):
        assert call(**kw) == -1, kw
    # an empty volume and no views: nothing is launched, nothing is touched
    for shape in ((0, 3, 4), (3, 0, 4), (3, 3, 0)):
        assert call(shape=shape, t=None, w=None) == 0
    assert call(n_views=0, d=None, ps=None, k=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(tsdf, before[0]) and torch.equal(weight, before[1])
    empty = FU.TsdfVolume((0, 3, 4), (0.0, 0.0, 0.0), 0.25, 0.5, DEV)
    FU.integrate(empty, depth, dev(sc["poses"]), dev(sc["intr"]))
    none = FU.integrate(volume(FU, sc), depth[:0], dev(sc["poses"][:0]), dev(sc["intr"][:0]))
    torch.cuda.synchronize()
    assert not bool(none.weight.any())
    with pytest.raises(ValueError):
        FU.integrate(volume(FU, sc), depth, dev(sc["poses"]), dev(sc["intr"]), max_depth=0.0)
