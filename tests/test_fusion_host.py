"""CPU: THE FUSION RULE of include/ls2fm.h judged by its properties on the numpy restatement (tests/fusion_restate.py), so that the
GPU tests (tests/test_hip_fusion.py) can be exact comparisons against that restatement; and ls2fm.fusion.extract's face filter."""
import os
import re
import types

import numpy as np
import pytest

import fusion_restate as FR
import fusion_scenes as S
import mc_restate

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fuse(sc, views=slice(None), state=None, weighted=False, **kw):
    if weighted:
        kw.update(max_depth=sc["max_depth"], max_weight=sc["max_weight"], view_weight=sc["view_weight"][views])
    state = FR.new_state(sc["shape"]) if state is None else state
    return FR.integrate(state, sc["origin"], sc["voxel"], sc["trunc"], sc["depth"][views], sc["poses"][views],
                        sc["intr"][views] if np.asarray(sc["intr"]).ndim == 3 else sc["intr"], near=sc["near"], **kw)


def bits(a):
    return np.asarray(a, F32).view(np.int32)


def test_the_brick_of_the_scenes_is_the_header_s():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    got = tuple(int(re.search(rf"#define\s+LS2FM_TSDF_BRICK_{a}\s+(\d+)", header).group(1)) for a in "XYZ")
    assert got == S.BRICK


def test_one_axis_camera_over_a_constant_depth_map_is_exact():
    """every number dyadic: in the frustum and up to D + trunc, tsdf == min(1, (D - c_z) / trunc) and weight == 1, exactly;
    every other lattice point keeps weight 0"""
    sc = S.constant_scene()
    tsdf, weight = fuse(sc)
    X = FR.lattice(sc["shape"], sc["origin"], sc["voxel"]).astype(np.float64).reshape(*sc["shape"], 3)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    f, c, H, W, D, tr = 8.0, 4.0, sc["H"], sc["W"], sc["D"], sc["trunc"]
    # 0 <= f x / z + c < W  <=>  0 <= f x + c z < W z for z > 0: products of dyadic numbers, exact in float64
    frustum = (z >= sc["near"]) & (f * x + c * z >= 0) & (f * x + c * z < W * z) & (f * y + c * z >= 0) & (f * y + c * z < H * z)
    fused = frustum & (z <= D + tr)
    assert fused.sum() > 100 and (frustum & ~fused).sum() > 20 and (~frustum).sum() > 100
    assert np.array_equal(weight, fused.astype(F32))
    expect = np.where(fused, np.minimum(1.0, (D - z) / tr), 0.0).astype(F32)
    assert np.array_equal(bits(tsdf), bits(expect))
    assert (expect[fused] == 1).any() and (expect[fused] == -1).any() and (expect[fused] == 0).any()


def test_the_weights_count_the_views():
    sc = S.sphere_scene(24, 64)
    both = fuse(sc, slice(0, 3, 2))                                     # views 0 and 2: their frusta cross
    singles = [fuse(sc, slice(i, i + 1))[1] for i in (0, 2)]
    assert np.array_equal(both[1], singles[0] + singles[1])
    assert set(np.unique(both[1])) == {0.0, 1.0, 2.0}


@pytest.mark.parametrize("nan_pose", [False, True])
def test_chunked_calls_give_the_bits_of_one_call(nan_pose):
    sc = S.edge_scene((3, 3, 65), 17, 33, 3, nan_pose)
    whole = fuse(sc, weighted=True)
    state = None
    for i in range(3):
        state = fuse(sc, slice(i, i + 1), state=state, weighted=True)
    split = fuse(sc, slice(2, 3), state=fuse(sc, slice(0, 2), weighted=True), weighted=True)
    for got in (state, split):
        assert np.array_equal(bits(got[0]), bits(whole[0])) and np.array_equal(bits(got[1]), bits(whole[1]))


def test_the_edge_scene_meets_every_edge_of_the_rule():
    """the scene the GPU tests compare bit for bit: each edge value the rule names occurs for some (lattice point, view)"""
    sc = S.edge_scene((3, 3, 65), 17, 33)
    stats = {}
    tsdf, weight = fuse(sc, weighted=True, stats=stats)
    for name in ("c_z == near", "behind the camera", "u == 0", "u == width", "v == height", "d nan", "d +inf", "d -inf", "d zero",
                 "d negative", "d == max_depth", "d one ulp above max_depth", "s == -trunc", "s one ulp below -trunc", "s == trunc",
                 "s > trunc", "max_weight reached exactly", "max_weight passed"):
        assert stats.get(name, 0) > 0, name
    assert np.isfinite(tsdf).all() and set(np.unique(weight)) == {0.0, 0.5, 1.0, 1.5}
    # the claims did what they say, in view 0 alone
    t0, w0 = fuse(sc, slice(0, 1), max_depth=sc["max_depth"])
    seen = {}
    for kind, idx, _ in sc["claims"]:
        seen.setdefault(kind, []).append((float(t0[idx]), float(w0[idx])))
    assert set(seen) == set(S.EDGE_KINDS)
    for kind in ("nan", "+inf", "-inf", "zero", "negative", "above_max_depth", "s_below_minus_trunc"):
        assert all(w == 0.0 for _, w in seen[kind]), kind
    assert all((t, w) == (-1.0, 1.0) for t, w in seen["s_eq_minus_trunc"])
    assert all((t, w) == (1.0, 1.0) for t, w in seen["s_eq_trunc"] + seen["s_beyond_trunc"])
    assert all(w == 1.0 for _, w in seen["max_depth"])
    # a NaN pose row: the view is skipped by every lattice point, the others are untouched by it
    bad = S.edge_scene((3, 3, 65), 17, 33, 3, True)
    stats = {}
    with_nan = fuse(bad, weighted=True, stats=stats)
    assert stats["c_z is NaN"] > 0
    w = bad["view_weight"].copy()
    w[1] = 0.0
    without = FR.fuse(sc["shape"], sc["origin"], sc["voxel"], sc["trunc"], sc["depth"], sc["poses"], sc["intr"], near=sc["near"],
                      max_depth=sc["max_depth"], max_weight=sc["max_weight"], view_weight=w)
    assert np.array_equal(bits(with_nan[0]), bits(without[0])) and np.array_equal(with_nan[1], without[1])


def test_view_weights_that_are_not_positive_skip_the_view():
    sc = S.edge_scene((3, 3, 65), 17, 33)
    kw = dict(near=sc["near"], max_depth=sc["max_depth"])
    args = (sc["shape"], sc["origin"], sc["voxel"], sc["trunc"])
    none = FR.fuse(*args, sc["depth"], sc["poses"], sc["intr"], view_weight=np.array([0.0, -1.0, np.nan], F32), **kw)
    assert not none[0].any() and not none[1].any()
    only = FR.fuse(*args, sc["depth"], sc["poses"], sc["intr"], view_weight=np.array([np.nan, 0.75, -0.0], F32), **kw)
    alone = FR.fuse(*args, sc["depth"][1:2], sc["poses"][1:2], sc["intr"][1:2], view_weight=np.array([0.75], F32), **kw)
    assert np.array_equal(bits(only[0]), bits(alone[0])) and np.array_equal(only[1], alone[1]) and only[1].any()


@pytest.mark.parametrize("n,hw,min_crossings", [(24, 64, 500), (32, 128, 1000)])
def test_the_fused_sphere_lies_within_one_voxel_of_the_sphere(n, hw, min_crossings):
    """six axis cameras, analytic depth maps, trunc = 3 voxels: every zero crossing on a lattice edge between two lattice points
    of weight >= 1 lies within one voxel of the sphere -- on the observed side and at the unobserved frontier behind the surface
    alike.  The bound is a condition.  The restatement's own worst values: 0.638 voxels at 24^3 with 64^2 images, 0.682 at 32^3
    with 128^2 (printed below)."""
    sc = S.sphere_scene(n, hw)
    tsdf, weight = fuse(sc)
    c = FR.crossings(tsdf, weight, sc["origin"], sc["voxel"])
    err = np.abs(np.linalg.norm(c, axis=1) - S.SPHERE_R) / sc["voxel"]
    print(f"fused sphere {n}^3, {hw}^2 images: {len(c)} crossings, worst {err.max():.3f} voxels, mean {err.mean():.3f}")
    assert len(c) >= min_crossings
    assert err.max() <= 1.0
    # and the extracted mesh is that surface
    v, f = FR.extract(tsdf, weight, sc["origin"], sc["voxel"])
    assert len(f) > min_crossings and np.isfinite(v).all()
    assert (np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - S.SPHERE_R) <= sc["voxel"]).all()


def _bad_vertices(vol, observed):
    """per marching-cubes vertex: one end of its lattice edge is unobserved"""
    owner, axis = mc_restate.vertex_owners(vol, 0.0)
    other = owner.copy()
    other[np.arange(len(axis)), axis] += 1
    return ~(observed[tuple(owner.T)] & observed[tuple(other.T)])


@pytest.mark.parametrize("hole", [(1, 1, 1), (0, 1, 1), (2, 2, 2), None])
def test_extract_drops_exactly_the_faces_on_an_unobserved_corner_s_crossing_edges(hole):
    """a hand-made 3 x 3 x 3 volume, tsdf = ix - 1 / 2 (the plane between ix = 0 and ix = 1), one lattice point unobserved: a not-below
    one next to the surface, a below one, one away from the surface, none"""
    tsdf = np.broadcast_to((np.arange(3, dtype=F32) - F32(0.5))[:, None, None], (3, 3, 3)).copy()
    weight = np.ones((3, 3, 3), F32)
    if hole is not None:
        weight[hole] = 0.5                                           # below min_weight = 1
    observed = weight >= 1
    vol = np.where(observed, tsdf, F32(np.nan))
    v_all, f_all = mc_restate.marching_cubes(vol, 0.0, spacing=(0.25,) * 3, origin=(0.0, 0.0, 0.0))
    bad = _bad_vertices(vol, observed)
    assert np.array_equal(bad, ~np.isfinite(v_all).all(axis=1)), "a vertex is not finite exactly when an end of its edge is unobserved"
    v, f, kept = FR.drop_non_finite(v_all, f_all)
    assert np.array_equal(kept, ~bad[f_all].any(axis=1))
    assert np.isfinite(v).all() and len(v) == len(np.unique(f_all[kept])) and np.array_equal(v[f], v_all[f_all[kept]])
    got_v, got_f = FR.extract(tsdf, weight, (0.0, 0.0, 0.0), 0.25)
    assert np.array_equal(got_v, v) and np.array_equal(got_f, f)
    full_v, full_f = mc_restate.marching_cubes(tsdf, 0.0, spacing=(0.25,) * 3, origin=(0.0, 0.0, 0.0))
    if hole in ((2, 2, 2), None):
        assert kept.all() and np.array_equal(v, full_v) and np.array_equal(f, full_f)
    else:
        assert 0 < kept.sum() < len(kept)
        assert (np.abs(v[:, 0] - 0.125) < 1e-7).all()                # what is left lies on the plane


def _cpu_volume(sc):
    """TsdfVolume refuses CPU devices: a plain object with its attributes, for the torch form"""
    import torch
    return types.SimpleNamespace(shape=tuple(sc["shape"]), origin=tuple(sc["origin"]), voxel=sc["voxel"], trunc=sc["trunc"],
                                 device=torch.device("cpu"), tsdf=torch.zeros(*sc["shape"]), weight=torch.zeros(*sc["shape"]))


@pytest.mark.parametrize("shape,H,W,nan_pose", [((5, 4, 67), 9, 11, False), ((3, 3, 130), 7, 5, True)])
def test_integrate_torch_on_the_cpu_leaves_the_restatement_s_bits(shape, H, W, nan_pose):
    """ls2fm.fusion.integrate_torch, the torch form the GPU tests and tools/time_fusion.py hold the kernel against, on CPU tensors
    against FR.fuse on the edge scene with its near, max_depth, view weights and max_weight: tsdf and weight equal as bits at
    every lattice point"""
    import torch
    from ls2fm import fusion
    sc = S.edge_scene(shape, H, W, nan_pose=nan_pose)
    want = fuse(sc, weighted=True)
    vol = fusion.integrate_torch(_cpu_volume(sc), torch.from_numpy(sc["depth"]), torch.from_numpy(np.asarray(sc["poses"], F32)),
                                 torch.from_numpy(np.asarray(sc["intr"], F32)), near=sc["near"], max_depth=sc["max_depth"],
                                 view_weight=[float(w) for w in sc["view_weight"]], max_weight=sc["max_weight"])
    assert want[1].any() and (want[1] == 0).any()
    for got, ref in ((vol.tsdf, want[0]), (vol.weight, want[1])):
        assert np.array_equal(got.numpy().view(np.uint32), np.asarray(ref, F32).view(np.uint32))


def test_public_entry_points_refuse_cpu_tensors():
    import torch
    from ls2fm import fusion
    # fusion's own arguments are refused in fusion's name, before the views are looked at
    with pytest.raises(RuntimeError, match=r"ls2fm\.fusion.*no CPU fallback"):
        fusion.integrate(types.SimpleNamespace(device=torch.device("cpu")), torch.ones(1, 8, 8), torch.zeros(1, 3, 4), torch.eye(3))
    with pytest.raises(RuntimeError):
        fusion.TsdfVolume((4, 4, 4), (0.0, 0.0, 0.0), 0.25, 0.5, "cpu")
    for bad in (dict(voxel=0.0), dict(trunc=float("inf")), dict(voxel=float("nan")), dict(origin=(0.0, float("nan"), 0.0)), dict(shape=(4, 4))):
        kw = dict(shape=(4, 4, 4), origin=(0.0, 0.0, 0.0), voxel=0.25, trunc=0.5, device="cuda")
        kw.update(bad)
        with pytest.raises(ValueError):
            fusion.TsdfVolume(**kw)
    with pytest.raises(RuntimeError):
        fusion.fuse_mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 3, 4), torch.eye(3), 8, 8, 0.1)
