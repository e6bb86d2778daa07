"""CPU: THE FUSION RULE of include/ls2fm.h judged by its properties on the numpy restatement (tests/fuse_restate.py), so that the
GPU tests (tests/test_hip_fuse.py) can be exact comparisons against that restatement; ls2fm.mvs.fuse_depths_torch on CPU tensors
against it bit for bit; that the edge scene meets every edge; refusals."""
import os
import re

import numpy as np
import pytest

import fuse_restate as FR
import fuse_scenes as FS
import mvs_scenes as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(got, ref):
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, f"{g.dtype} {g.shape} != {r.dtype} {r.shape}"
    if g.dtype.kind != "f":
        return np.array_equal(g, r)
    return bool(((g.view(np.int32) == r.view(np.int32)) | (np.isnan(g) & np.isnan(r))).all())


def restate(sc, normals=True, colours=True, stats=None):
    return FR.fuse(sc["depth"], sc["poses"], sc["intr"], sc["sources"], normal=sc["normal"] if normals else None,
                   colour=sc["colour"] if colours else None, stats=stats, **FS.fuse_kw(sc))


def _torch(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def test_the_header_s_constants_are_the_python_copies():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    from ls2fm import mvs
    for name in ("FUSE_MAX_CHANNELS", "FUSE_TILE_W", "FUSE_TILE_H"):
        assert int(re.search(rf"#define\s+LS2FM_MVS_{name}\s+(\d+)", header).group(1)) == getattr(mvs, name), name
    assert mvs.FUSE_TILE_W * mvs.FUSE_TILE_H == 256
    # the sizes of the bit-for-bit tests: inside one tile, a whole tile, one pixel past each edge of it
    for side, tile in ((0, mvs.FUSE_TILE_H), (1, mvs.FUSE_TILE_W)):
        sizes = {hw[side] for hw in FS.EDGE_SIZES}
        assert {tile, tile + 1} <= sizes and min(sizes) < tile - 1, (side, tile)
    assert (mvs.FUSE_TILE_H, mvs.FUSE_TILE_W) in FS.EDGE_SIZES and (mvs.FUSE_TILE_H + 1, mvs.FUSE_TILE_W + 1) in FS.EDGE_SIZES
    assert FR.cos2_of(FS.EDGE_ANGLE) == F32(0.5)


EDGES = ["source entry equal to the view", "source entry outside [0, V)", "source listed twice", "d_s nan", "d_s zero", "d_s negative",
         "d_s inf", "reprojection at equality", "reprojection beyond", "depth at equality", "depth beyond", "normal angle at equality",
         "normal angle beyond", "a == 0", "a < 0", "a is NaN", "the partner's normal is zero", "the pixel's normal is zero",
         "the pixel's normal is NaN", "the pixel's normal is not of unit length", "suppressed: the only consistent partners are lower",
         "owner with higher partners only", "suppressed with partners of both kinds", "owner without a partner", "no depth",
         "a NaN colour in a row", "a NaN normal in a row"]


def test_the_edge_scene_meets_every_edge_of_the_fusion_rule():
    """the scene the GPU tests compare bit for bit: each edge the rule names occurs at some (pixel, source)"""
    stats = {}
    sc = FS.edge_scene(17, 33)
    out = restate(sc, stats=stats)
    for name in EDGES:
        assert stats.get(name, 0) > 0, name
    stats = {}
    restate(FS.edge_scene(17, 33, nan_pose=True), stats=stats)
    assert stats["c_z is NaN"] > 0
    sup = out["support"]
    bad = ~(np.isfinite(sc["depth"]) & (sc["depth"] > 0))
    assert not sup[bad].any() and set(np.unique(sup)) >= {0, 1, 2, 3}
    # the rows are the pixels with support > 0 in (view, py, px) order
    assert np.array_equal(out["pixel"], np.nonzero(sup.reshape(-1))[0]) and len(out["points"]) == len(out["pixel"])
    # an owner without a partner is its own back-projection: its normal is the pixel's, turned and normalised; a NaN stays in its row
    alone = sup.reshape(-1)[out["pixel"]] == 1
    n_in = sc["normal"].reshape(-1, 3)[out["pixel"]].astype(np.float64)
    with np.errstate(all="ignore"):
        unit = n_in / np.linalg.norm(n_in, axis=1, keepdims=True)
    ok = alone & np.isfinite(unit).all(axis=1)
    assert ok.any() and np.allclose(out["normals"][ok], unit[ok], atol=1e-6)
    assert np.isfinite(out["points"][np.isnan(out["normals"]).any(axis=1) & (out["pixel"] // (17 * 33) != 2)]).all()
    # without normals every geometric partner counts: no fewer suppressed pixels
    plain = restate(sc, normals=False)
    assert plain["normals"] is None and len(plain["pixel"]) < len(out["pixel"])


@pytest.fixture(scope="module")
def sphere():
    sc = FS.sphere_fused()
    return sc, restate(sc)


def pairwise(a, b):
    return np.linalg.norm(a[:, None].astype(np.float64) - b[None].astype(np.float64), axis=2)


def test_fused_points_lie_on_the_sphere(sphere):
    """contributors lie within one reprojected pixel of each other along a chord, delta = max_reproj 2.5 / f, so their mean lies
    within delta^2 / (2 R) = 1.5e-3 of the sphere (hw = 32); the restatement's own value: 3.4e-4"""
    sc, out = sphere
    delta = sc["max_reproj"] * S.SPHERE_D / sc["focal"]
    r = np.linalg.norm(out["points"].astype(np.float64), axis=1)
    print(f"worst distance to the sphere {np.abs(r - S.SPHERE_R).max():.3e}, bound {delta ** 2 / (2 * S.SPHERE_R):.3e}")
    assert np.abs(r - S.SPHERE_R).max() <= delta ** 2 / (2 * S.SPHERE_R)


def test_fusion_deduplicates(sphere):
    """at most one third of the filtered pixels give a row (the restatement: 546 of 2500), and no two fused points are closer than
    a quarter of a pixel's footprint (the restatement's closest pair: 0.44 footprint; 57 % of the unfused cloud's points have a
    neighbour within a quarter)"""
    sc, out = sphere
    alive = np.isfinite(sc["depth"])
    assert 3 * len(out["points"]) <= alive.sum()
    d = pairwise(out["points"], out["points"])
    np.fill_diagonal(d, np.inf)
    raw = pairwise(sc["world"][alive], sc["world"][alive])
    np.fill_diagonal(raw, np.inf)
    print(f"{len(out['points'])} rows of {alive.sum()} filtered pixels; closest pair {d.min() / sc['footprint']:.2f} footprint; unfused: "
          f"{(raw.min(axis=1) < 0.25 * sc['footprint']).mean():.0%} within a quarter")
    assert d.min() >= 0.25 * sc["footprint"]
    assert (raw.min(axis=1) < 0.25 * sc["footprint"]).mean() > 0.5, "the unfused cloud is the one that repeats its points"


COVERAGE_MEASURED = 1.30    # footprints: the restatement's worst case at hw = 32 (1.2984)


def test_every_filtered_pixel_is_covered(sphere):
    """every filtered pixel's world point has a fused point within twice the restatement's measured worst case"""
    sc, out = sphere
    alive = np.isfinite(sc["depth"])
    worst = pairwise(sc["world"][alive], out["points"]).min(axis=1).max() / sc["footprint"]
    print(f"worst distance of a filtered pixel to the fused cloud: {worst:.4f} footprints")
    assert worst <= 2 * COVERAGE_MEASURED


def test_fused_normals_are_radial_and_outward(sphere):
    """with the analytic normals in, every fused normal is within delta / R rad of the radial direction at its point, and outward"""
    sc, out = sphere
    P, N = out["points"].astype(np.float64), out["normals"].astype(np.float64)
    radial = P / np.linalg.norm(P, axis=1, keepdims=True)
    cosine = (N * radial).sum(axis=1)
    assert np.isfinite(N).all() and (cosine > 0).all()
    assert np.allclose(np.linalg.norm(N, axis=1), 1.0, atol=1e-6)
    delta = sc["max_reproj"] * S.SPHERE_D / sc["focal"]
    assert np.arccos(np.clip(cosine, -1, 1)).max() <= delta / S.SPHERE_R
    # toward the cameras, as normals_to_world leaves them: the owner's centre is on the normal's side
    centres = FR.cam_to_world(sc["poses"])[:, :, 3][out["pixel"] // (sc["H"] * sc["W"])]
    assert (((centres - P) * N).sum(axis=1) > 0).all()


def test_support_counts_the_contributors(sphere):
    sc, out = sphere
    sup = out["support"]
    rows = sup.reshape(-1)[out["pixel"]]
    print("support histogram", np.bincount(sup.reshape(-1), minlength=6).tolist())
    assert rows.min() >= 1 and rows.max() <= sc["sources"].shape[1] + 1
    # the colour of a row is the mean of its contributors' pixels: inside their range
    assert np.isfinite(out["colours"]).all()
    assert out["colours"].min() >= np.nanmin(sc["colour"]) and out["colours"].max() <= np.nanmax(sc["colour"])


def torch_form(sc, normals=True, colours=True, **kw):
    from ls2fm import mvs
    return mvs.fuse_depths_torch(_torch(sc["depth"]), _torch(sc["poses"]), _torch(sc["intr"]), _torch(sc["sources"]),
                                 normal=_torch(sc["normal"]) if normals else None, images=_torch(sc["colour"]) if colours else None,
                                 **FS.fuse_kw(sc), **kw)


def check_cloud(got, want, sc, what=""):
    """a FusedCloud of torch tensors against the restatement's dict"""
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    pixel = host(got.pixel)
    assert np.array_equal(pixel, want["pixel"]), f"pixel {what}"
    sup = np.zeros(want["support"].size, np.uint8)
    sup[pixel] = host(got.support)
    assert np.array_equal(sup.reshape(want["support"].shape), want["support"]), f"support {what}"
    for name, g in (("points", got.points), ("normals", got.normals), ("colours", got.colors)):
        if want[name] is None:
            assert g is None, f"{name} {what}"
        else:
            assert same_bits(host(g), want[name]), f"{name} {what}"
    assert np.array_equal(host(got.view), pixel // (sc["H"] * sc["W"])), f"view {what}"
    assert same_bits(host(got.centers), FR.cam_to_world(sc["poses"])[:, :, 3][host(got.view)]), f"centers {what}"


@pytest.mark.parametrize("H,W", FS.EDGE_SIZES)
@pytest.mark.parametrize("S_,C,nan_pose,normals,colours", [(5, 3, False, True, True), (2, 1, True, True, False), (1, 4, False, False, True),
                                                          (5, 4, True, False, False)])
def test_fuse_depths_torch_on_the_cpu_leaves_the_restatement_s_bits(H, W, S_, C, nan_pose, normals, colours):
    sc = FS.edge_scene(H, W, S_, C, nan_pose)
    check_cloud(torch_form(sc, normals, colours), restate(sc, normals, colours), sc)


def test_min_support_and_the_sphere_in_the_torch_form(sphere):
    sc, want = sphere
    got = torch_form(sc)
    check_cloud(got, want, sc, "sphere")
    few = torch_form(sc, min_support=4)
    keep = got.support >= 4
    assert 0 < int(keep.sum()) < len(want["pixel"]) and np.array_equal(few.pixel.numpy(), got.pixel[keep].numpy())
    assert same_bits(few.points.numpy(), got.points[keep].numpy()) and same_bits(few.centers.numpy(), got.centers[keep].numpy())


def test_refusals_and_argument_errors():
    import torch
    from ls2fm import mvs
    sc = FS.edge_scene(15, 17)
    d, pose, intr, src, n, c = (_torch(sc[k]) for k in ("depth", "poses", "intr", "sources", "normal", "colour"))
    # the kernel entry point refuses CPU tensors in ls2fm.mvs's name, and so does the route through the cloud
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.fuse_depths(d, pose, intr, src)
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.dense_reconstruct(d, pose, intr, ((-1, -1, -1), (1, 1, 1)), 0.1, surface="poisson")
    with pytest.raises(ValueError, match="surface"):
        mvs.dense_reconstruct(d, pose, intr, ((-1, -1, -1), (1, 1, 1)), 0.1, surface="median")
    for bad in (dict(max_normal_angle=-1.0), dict(max_normal_angle=91.0), dict(max_normal_angle=float("nan")), dict(min_support=0),
                dict(max_reproj=-1.0), dict(rel_depth=float("inf")), dict(near=0.0)):
        with pytest.raises(ValueError):
            mvs.fuse_depths_torch(d, pose, intr, src, **bad)
    with pytest.raises(ValueError):
        mvs.fuse_depths_torch(d, pose, intr, src[:3])
    with pytest.raises(ValueError):
        mvs.fuse_depths_torch(d, pose, intr, src, normal=n[:, :5])
    with pytest.raises(ValueError):
        mvs.fuse_depths_torch(d, pose, intr, src, images=torch.zeros(6, 15, 17, 5))
    with pytest.raises(ValueError):
        mvs.fuse_depths_torch(d, pose, intr, src, images=c[:3])
    opt = mvs.MvsOptions(max_normal_angle=30.0, min_support=2)
    assert opt.fuse()["max_normal_angle"] == 30.0 and opt.fuse()["min_support"] == 2 and opt.fuse()["rel_depth"] == opt.rel_depth
    # no views: an empty cloud
    empty = mvs.fuse_depths_torch(torch.zeros(0, 4, 5), torch.zeros(0, 3, 4), intr, torch.zeros(0, 2, dtype=torch.int32))
    assert empty.points.shape == (0, 3) and empty.pixel.shape == (0,) and empty.normals is None
