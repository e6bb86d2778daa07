"""CPU: THE SWEEP RULE and THE CONSISTENCY RULE of include/ls2fm.h judged by their properties on the numpy restatement
(tests/mvs_restate.py), so that the GPU tests (tests/test_hip_mvs.py) can be exact comparisons against that restatement; the torch
forms of ls2fm.mvs on CPU tensors against it bit for bit; the torch-op helpers; refusals."""
import os
import re

import numpy as np
import pytest

import mvs_restate as MR
import mvs_scenes as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sweep(sc, stats=None, **kw):
    return MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc.get("refs"), half_width=sc["half_width"],
                    near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"], stats=stats, **kw)


def bits(a):
    return np.asarray(a, F32).view(np.int32)


def same_bits(got, ref):
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype
    if g.dtype.kind != "f":
        return np.array_equal(g, r)
    return bool(((bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))).all())


def test_the_tile_of_the_scenes_is_the_header_s():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    assert int(re.search(r"#define\s+LS2FM_MVS_TILE\s+(\d+)", header).group(1)) == S.TILE
    from ls2fm import mvs
    for name in ("TILE", "MAX_HALF_WIDTH", "MAX_SOURCES", "MAX_PLANES"):
        assert int(re.search(rf"#define\s+LS2FM_MVS_{name}\s+(\d+)", header).group(1)) == getattr(mvs, name)


@pytest.mark.parametrize("last", [False, True])
def test_the_exact_scene_finds_the_plane_with_score_one(last):
    """every number dyadic, whole-pixel disparities: at every pixel that has a window the true plane wins, its windows agree bit for
    bit in every valid source, so cov == va == vb, sqrt(fl(v v)) == v and score == 1.0 exactly; the plane is the first or the last
    of `depths`, so nothing is refined and depth == d_k by its bits"""
    sc = S.exact_scene(last)
    depth, score, plane = sweep(sc)
    w, H, W = sc["half_width"], sc["H"], sc["W"]
    inner = np.zeros((H, W), bool)
    inner[w:H - w, w:W - w] = True
    assert np.array_equal(plane[0] >= 0, inner)
    assert (plane[0][inner] == sc["true_plane"]).all()
    assert np.array_equal(bits(score[0][inner]), bits(np.ones(inner.sum(), F32)))
    assert np.array_equal(bits(depth[0][inner]), bits(np.full(inner.sum(), 4.0, F32)))
    assert np.isnan(depth[0][~inner]).all() and np.isnan(score[0][~inner]).all()


@pytest.fixture(scope="module")
def sphere():
    sc = S.sphere_scene()
    depth, score, plane = sweep(sc)
    filtered, count = MR.filter_depths(depth, sc["poses"], sc["intr"], sc["sources"], near=sc["near"], max_reproj=sc["max_reproj"],
                                       rel_depth=sc["rel_depth"], min_consistent=sc["min_consistent"])
    return sc, depth, filtered, count


def test_the_swept_and_filtered_sphere_lies_within_one_plane_spacing(sphere):
    """5 cameras of 64 x 64, 48 planes uniform in depth: after sweep and filter the median |depth - analytic depth| over the
    survivors is at most one plane spacing (0.0149).  The bound is a condition.  The restatement's own values: 7657 survivors of
    8680 swept pixels, median error 0.0038 (printed below); the floor on the survivors is half of that count.  Every survivor's
    window lies on the sphere, so it sees the sphere."""
    sc, depth, filtered, count = sphere
    alive = np.isfinite(filtered)
    assert np.isfinite(sc["depth"][alive]).all(), "a survivor does not see the sphere"
    err = np.abs(filtered[alive].astype(np.float64) - sc["depth"][alive])
    print(f"sphere: {int(np.isfinite(depth).sum())} swept pixels, {int(alive.sum())} survivors, median error {np.median(err):.4f}, "
          f"plane spacing {sc['spacing']:.4f}")
    assert alive.sum() >= 7657 // 2
    assert np.median(err) <= sc["spacing"]
    assert np.array_equal(alive, np.isfinite(depth) & (count >= sc["min_consistent"]))
    assert same_bits(filtered[alive], depth[alive])


EDGES = ["reference tap not finite", "va == min_var", "va one ulp below min_var", "a view is reference and source", "x0 == 0", "x0 == -1",
         "x0 + 1 == W - 1", "x0 + 1 == W", "y0 == 0", "y0 == -1", "y0 + 1 == H - 1", "y0 + 1 == H", "c_z == near", "plane behind the source",
         "c_z is NaN", "source sample not finite", "vb == min_var", "vb one ulp below min_var", "source skipped", "count == min_sources - 1",
         "tie goes to the lower plane", "best plane at k = 0", "best plane at k = D - 1", "invalid neighbour", "den == 0", "refined",
         "pixel without a plane"]
FILTER_EDGES = ["pixel leaves the source image", "d_s nan", "d_s zero", "d_s negative", "d_s inf", "reprojection at equality",
                "reprojection beyond", "depth at equality", "depth beyond", "consistent"]


def test_the_edge_scenes_meet_every_edge_of_the_sweep_rule():
    """the scenes the GPU tests compare bit for bit: each edge the rule names occurs for some (pixel, plane, source)"""
    stats = {}
    patched = S.grid_scene(17, 33, 1, patches=True)
    depth, score, plane = sweep(patched, stats)
    for name in EDGES:
        if name not in ("c_z is NaN", "den == 0"):
            assert stats.get(name, 0) > 0, name
    # the claims did what they say: reference 0, the pixels of the two flat windows
    ya, xa = patched["claims"]["va_at"]
    yb, xb = patched["claims"]["va_below"]
    assert plane[0, ya, xa] >= 0 and plane[0, yb, xb] == -1
    stats = {}
    sweep(S.grid_scene(17, 33, 1, nan_pose=True), stats)
    assert stats["c_z is NaN"] > 0
    stats = {}
    sc = S.den_scene()
    depth, score, plane, scores = sweep(sc, stats, return_scores=True)
    y, x = sc["pixel"]
    assert stats["den == 0"] > 0 and plane[0, y, x] == 1 and depth[0, y, x] == sc["depths"][0, 1]
    assert scores[0, 0, y, x] == np.nextafter(F32(1), F32(0)) and scores[0, 1, y, x] == 1 and scores[0, 2, y, x] == 1


def test_the_filter_scene_meets_every_edge_of_the_consistency_rule():
    sc = S.filter_scene(17, 33)
    stats = {}
    filtered, count = MR.filter_depths(sc["depth"], sc["poses"], sc["intr"], sc["sources"], near=sc["near"], max_reproj=sc["max_reproj"],
                                       rel_depth=sc["rel_depth"], min_consistent=2, stats=stats)
    for name in FILTER_EDGES:
        assert stats.get(name, 0) > 0, name
    bad = ~(np.isfinite(sc["depth"]) & (sc["depth"] > 0))
    assert not count[bad].any() and np.isnan(filtered[bad]).all()
    assert set(np.unique(count)) >= {0, 1, 2, 3}
    # min_consistent 0 keeps every pixel as it is, more than S keeps none
    keep, _ = MR.filter_depths(sc["depth"], sc["poses"], sc["intr"], sc["sources"], near=sc["near"], min_consistent=0)
    assert same_bits(keep, sc["depth"])
    none, _ = MR.filter_depths(sc["depth"], sc["poses"], sc["intr"], sc["sources"], near=sc["near"], min_consistent=6)
    assert np.isnan(none).all()


def test_references_in_chunks_give_the_bits_of_one_call():
    sc = S.grid_scene(17, 33, 2)
    whole = sweep(sc)
    for r in range(3):
        part = MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"][r:r + 1], sc["depths"][r:r + 1], refs=sc["refs"][r:r + 1],
                        half_width=2, near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])
        for got, ref in zip(part, whole):
            assert same_bits(got[0], ref[r])


def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("H,W,w,nan_pose,patches", [(17, 33, 1, False, True), (15, 16, 2, True, False), (17, 33, 3, True, False),
                                                    (15, 16, 3, False, False), (17, 33, 4, False, False), (15, 16, 4, True, False)])
def test_plane_sweep_torch_on_the_cpu_leaves_the_restatement_s_bits(H, W, w, nan_pose, patches):
    from ls2fm import mvs
    sc = S.grid_scene(H, W, w, nan_pose=nan_pose, patches=patches)
    want = sweep(sc)
    got = mvs.plane_sweep_torch(_torch(sc["images"]), _torch(sc["poses"]), _torch(sc["intr"]), _torch(sc["sources"]), _torch(sc["depths"]),
                                refs=_torch(sc["refs"]), half_width=w, near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])
    assert (want[2] >= 0).any() and (want[2] < 0).any()
    for g, r in zip(got, want):
        assert same_bits(g.numpy(), r)


def test_plane_sweep_torch_on_the_den_scene():
    from ls2fm import mvs
    sc = S.den_scene()
    want = sweep(sc)
    got = mvs.plane_sweep_torch(_torch(sc["images"]), _torch(sc["poses"]), _torch(sc["intr"]), _torch(sc["sources"]), _torch(sc["depths"]),
                                refs=_torch(sc["refs"]), half_width=1, near=sc["near"], min_var=sc["min_var"], min_sources=1)
    for g, r in zip(got, want):
        assert same_bits(g.numpy(), r)


@pytest.mark.parametrize("H,W,S_,nan_pose,min_consistent", [(17, 33, 5, False, 2), (15, 16, 3, True, 1)])
def test_filter_depths_torch_on_the_cpu_leaves_the_restatement_s_bits(H, W, S_, nan_pose, min_consistent):
    from ls2fm import mvs
    sc = S.filter_scene(H, W, S_, nan_pose)
    kw = dict(near=sc["near"], max_reproj=sc["max_reproj"], rel_depth=sc["rel_depth"], min_consistent=min_consistent)
    want = MR.filter_depths(sc["depth"], sc["poses"], sc["intr"], sc["sources"], **kw)
    got = mvs.filter_depths_torch(_torch(sc["depth"]), _torch(sc["poses"]), _torch(sc["intr"]), _torch(sc["sources"]), **kw)
    assert want[1].any() and np.isfinite(want[0]).any() and np.isnan(want[0]).any()
    assert same_bits(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])


def test_relative_poses_equal_the_restatement_and_invert_each_other():
    import torch
    from ls2fm import mvs
    sc = S.sphere_scene()
    refs = np.arange(5)
    for back in (False, True):
        got = mvs.relative_poses(_torch(sc["poses"]), _torch(refs), _torch(sc["sources"]), back=back)
        assert got.dtype == torch.float32 and same_bits(got.numpy(), MR.relative_poses(sc["poses"], refs, sc["sources"], back=back))
    P = sc["poses"].astype(np.float64)
    to4 = lambda p: np.concatenate([p, [[0, 0, 0, 1]]])
    rel = MR.relative_poses(sc["poses"], refs, sc["sources"])
    assert np.allclose(to4(rel[1, 2]), to4(P[sc["sources"][1, 2]]) @ np.linalg.inv(to4(P[1])), atol=1e-6)
    back = MR.relative_poses(sc["poses"], refs, sc["sources"], back=True)
    assert np.allclose(to4(rel[1, 2]) @ to4(back[1, 2]), np.eye(4), atol=1e-6)


def test_the_torch_op_helpers():
    import torch
    from ls2fm import mvs
    sc = S.sphere_scene()
    poses = _torch(sc["poses"])
    # to_grey
    rgb = torch.rand(2, 5, 7, 3, generator=torch.Generator().manual_seed(0))
    grey = mvs.to_grey(rgb)
    want = (F32(0.299) * rgb.numpy()[..., 0] + F32(0.587) * rgb.numpy()[..., 1]) + F32(0.114) * rgb.numpy()[..., 2]
    assert grey.shape == (2, 5, 7) and same_bits(grey.numpy(), want) and mvs.to_grey(grey).data_ptr() == grey.data_ptr()
    # depth_planes: end points, monotone, uniform in inverse depth or in depth
    d = mvs.depth_planes(torch.tensor([1.0, 2.0]), torch.tensor([4.0, 3.0]), 7).double()
    assert d.shape == (2, 7) and torch.equal(d[:, 0], torch.tensor([1.0, 2.0]).double()) and torch.equal(d[:, -1], torch.tensor([4.0, 3.0]).double())
    assert (d[:, 1:] > d[:, :-1]).all() and torch.allclose((1 / d).diff(dim=1), (1 / d).diff(dim=1)[:, :1].expand(2, 6), atol=1e-6)
    lin = mvs.depth_planes(1.0, 4.0, 4, inverse=False)
    assert torch.equal(lin, torch.tensor([[1.0, 2.0, 3.0, 4.0]])) and torch.equal(mvs.depth_planes(1.5, 4.0, 1), torch.tensor([[1.5]]))
    # depth_range_from_points: the sphere's surface points seen from the 5 cameras; a view that looks away gets NaN
    g = torch.Generator().manual_seed(1)
    X = torch.nn.functional.normalize(torch.randn(500, 3, generator=g), dim=1) * 0.5
    near, far = mvs.depth_range_from_points(X, poses, margin=0.0)
    assert near.shape == (5,) and (near >= 2.0 - 1e-6).all() and (far <= 3.0 + 1e-6).all() and (near < far).all()
    wide = mvs.depth_range_from_points(X, poses, margin=0.1)
    assert torch.allclose(wide[0], near * 0.9) and torch.allclose(wide[1], far * 1.1)
    away = poses.clone()
    away[0, 2] = -away[0, 2]
    assert torch.isnan(mvs.depth_range_from_points(X, away)[0][0])
    # select_sources: the centre camera takes the four others (12 degrees); the outer ones take the centre first (12 degrees, then
    # about 17 degrees for the neighbours, 24 for the opposite one); the band cuts
    src = mvs.select_sources(poses, 4, min_angle=3.0, max_angle=45.0, centre=(0.0, 0.0, 0.0))
    assert src.dtype == torch.int32 and src.shape == (5, 4) and set(src[0].tolist()) == {1, 2, 3, 4}
    assert src[1].tolist()[0] == 0 and src[1].tolist()[3] == 2 and set(src[1].tolist()[1:3]) == {3, 4}
    assert torch.equal(mvs.select_sources(poses, 4, 3.0, 45.0), src), "the default centre is where the optical axes meet"
    cut = mvs.select_sources(poses, 6, min_angle=15.0, max_angle=20.0, centre=(0.0, 0.0, 0.0))
    assert cut.shape == (5, 6) and cut[0].tolist() == [-1] * 6 and set(cut[1].tolist()) == {3, 4, -1}


def test_refusals_and_argument_errors():
    import torch
    from ls2fm import mvs
    sc = S.grid_scene(15, 16)
    img, pose, intr, src, dep = (_torch(sc[k]) for k in ("images", "poses", "intr", "sources", "depths"))
    # the kernel entry points refuse CPU tensors in ls2fm.mvs's name
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.plane_sweep(img, pose, intr, src, dep, refs=_torch(sc["refs"]))
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.filter_depths(img, pose, intr, torch.zeros(6, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.dense_reconstruct(img, pose, intr, ((-1, -1, -1), (1, 1, 1)), 0.1)
    refs = _torch(sc["refs"])
    for bad in (dict(half_width=0), dict(half_width=6), dict(min_var=-1.0), dict(min_var=float("nan")), dict(min_sources=0),
                dict(min_sources=6), dict(near=0.0)):
        with pytest.raises(ValueError):
            mvs.plane_sweep_torch(img, pose, intr, src, dep, refs=refs, **bad)
    with pytest.raises(ValueError):
        mvs.plane_sweep_torch(img, pose, intr, src[:2], dep, refs=refs)
    with pytest.raises(ValueError):
        mvs.plane_sweep_torch(img, pose, intr, src, dep[:2], refs=refs)
    with pytest.raises(ValueError):
        mvs.plane_sweep_torch(img[:3], pose, intr, src, dep, refs=refs)
    for bad in (dict(max_reproj=-1.0), dict(rel_depth=float("inf")), dict(min_consistent=-1), dict(near=float("nan"))):
        with pytest.raises(ValueError):
            mvs.filter_depths_torch(img, pose, intr, torch.zeros(6, 2, dtype=torch.int32), **bad)
    with pytest.raises(ValueError):
        mvs.depth_planes(1.0, 2.0, 0)
    with pytest.raises(ValueError):
        mvs.to_grey(torch.zeros(2, 3, 4, 5))
