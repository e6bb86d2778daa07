"""CPU: that stereo_views_scenes can tell right from wrong, judged on the numpy restatements (tests/mvs_restate.py,
tests/patchmatch_restate.py, tests/fuse_restate.py), so that the exact comparisons of tests/test_hip_stereo_views.py mean something:
the scene meets its claims; a view's intrinsics taken for another's, fx for fy, cx for cy or a rotation for its transpose change the
answer of every rule; the torch forms of ls2fm.mvs on CPU tensors leave the restatements' bits on it."""
import functools

import numpy as np
import pytest

import fuse_restate as FR
import mvs_restate as MR
import patchmatch_restate as PR
import stereo_views_scenes as VS

F32 = np.float32
PERTURB = dict(depth_perturb=0.02, normal_perturb=0.5, max_slope=1.0)


def differ(got, ref):
    """per entry: the bits differ, a NaN matching a NaN"""
    g, r = np.asarray(got, F32), np.asarray(ref, F32)
    return (g.view(np.int32) != r.view(np.int32)) & ~(np.isnan(g) & np.isnan(r))


def same_bits(got, ref):
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, f"{g.dtype} {g.shape} != {r.dtype} {r.shape}"
    if g.dtype.kind != "f":
        return np.array_equal(g, r)
    return not differ(g, r).any()


def sweep_kw(sc):
    return dict(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])


def filter_kw(fs):
    return dict(near=fs["near"], max_reproj=fs["max_reproj"], rel_depth=fs["rel_depth"])


def fuse_kw(fs):
    return dict(filter_kw(fs), max_normal_angle=fs["max_normal_angle"])


@functools.lru_cache(maxsize=None)
def swept(w, mutation=None):
    sc = VS.views_scene(17, 33, w)
    return MR.sweep(sc["images"], sc["poses"], mutated(sc["intr"], mutation), sc["sources"], sc["depths"], refs=sc["refs"], **sweep_kw(sc))


def mutated(intr, kind):
    """the mistakes one shared square-pixel K hides, made in the inputs"""
    K = np.array(intr, F32)
    if kind == "rolled by one view":
        K = np.roll(K, 1, axis=0)
    elif kind == "view 0's for every view":
        K[:] = K[0]
    elif kind == "fx for fy":
        K[:, 0, 0], K[:, 1, 1] = intr[:, 1, 1], intr[:, 0, 0]
    elif kind == "cx for cy":
        K[:, 0, 2], K[:, 1, 2] = intr[:, 1, 2], intr[:, 0, 2]
    else:
        assert kind is None
    return K


MUTATIONS = ["rolled by one view", "view 0's for every view", "fx for fy", "cx for cy"]


def test_the_scene_meets_its_claims():
    sc = VS.views_scene(17, 33, 3)
    K = sc["intr"]
    assert K.shape == (4, 3, 3) and (K[:, 0, 0] != K[:, 1, 1]).all()
    k4 = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (k4[a] != k4[b]).all(), (a, b)
    centre = np.array([33 / 2.0, 17 / 2.0])
    off = k4[:, 2:] - centre
    assert (off != np.round(off)).all() and (off != 0).all()
    sq = VS.views_scene(17, 17, 3)["intr"]
    assert (sq[:, 0, 2] != sq[:, 1, 2]).all(), "cx != cy even at a square image"
    # every relative rotation is general: nine non-zero entries, not symmetric
    every = np.arange(4)
    rel = MR.relative_poses(sc["poses"], every, np.tile(every, (4, 1)))
    for a in range(4):
        for b in range(4):
            if a != b:
                Rm = rel[a, b, :, :3]
                assert (np.abs(Rm) > 1e-3).all() and (np.abs(Rm - Rm.T)[np.triu_indices(3, 1)] > 1e-3).all(), (a, b)
    # the references and their rows
    refs, rows = sc["refs"], sc["sources"]
    assert (refs != np.arange(len(refs))).all()
    for rv, row in zip(refs, rows):
        real = row[row >= 0]
        assert (row == -1).any() and (real > rv).any() and len(set(real)) < len(real) and rv not in real
        assert (real < rv).any() or rv == 0, "views on both sides of every reference that has both"
    assert sum(0 < rv < 3 for rv in refs) >= 2
    assert np.isnan(sc["images"][0]).sum() == 1 and (sc["images"][1] == np.inf).sum() == 1 and (sc["images"][2] == -np.inf).sum() == 1
    assert np.isfinite(sc["images"]).sum() == sc["images"].size - 3
    # the planes: the true depths lie among them, and no row starts with one of them
    truth = sc["depth"][refs]
    lo, hi = truth.min(axis=(1, 2)), truth.max(axis=(1, 2))
    assert ((sc["depths"][:, 0] < lo) | (sc["depths"][:, 0] > hi)).all() and ((sc["depths"][:, 1:] > lo[:, None]) & (sc["depths"][:, 1:] < hi[:, None])).any(axis=1).all()
    assert sc["depths"].min() < truth.min() and truth.max() < sc["depths"].max()
    assert np.allclose(np.linalg.norm(sc["normal"], axis=1), 1.0) and (sc["normal"][:, 2] < -0.9).all()


@pytest.mark.parametrize("w", [3, 4])
def test_the_sweep_finds_scores_and_several_planes(w):
    depth, score, plane = swept(w)
    H, W = 17, 33
    windows = (H - 2 * w) * (W - 2 * w)
    for r in range(3):
        n = int(np.isfinite(score[r]).sum())
        print(f"w = {w}, reference {r}: {n} finite scores of {windows} windows, planes {np.unique(plane[r]).tolist()}")
        assert 4 * n >= windows
        assert np.isnan(score[r]).any() and len(set(np.unique(plane[r])) - {-1}) > 2
    # the sweep finds the plane: the median error is below the plane spacing
    truth = VS.views_scene(H, W, w)["depth"][VS.REFS]
    assert np.nanmedian(np.abs(depth - truth)) < 0.08


def changed_fraction(got, ref):
    """of the pixels where either float32 map is finite (trailing axes belong to the pixel), those whose bits differ"""
    g, r = np.asarray(got, F32), np.asarray(ref, F32)
    if g.ndim > 3:
        g, r = g.reshape(g.shape[:3] + (-1,)), r.reshape(r.shape[:3] + (-1,))
        either = np.isfinite(g).all(axis=-1) | np.isfinite(r).all(axis=-1)
        moved = differ(g, r).any(axis=-1)
    else:
        either, moved = np.isfinite(g) | np.isfinite(r), differ(g, r)
    assert either.sum() > 100
    return float(moved[either].sum()) / float(either.sum())


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("w", [3, 4])
def test_a_mistaken_intrinsics_row_changes_the_sweep(w, mutation):
    f = changed_fraction(swept(w, mutation)[1], swept(w)[1])
    print(f"sweep, w = {w}, intrinsics {mutation}: {f:.1%} of the scores change")
    assert f >= 0.5


@functools.lru_cache(maxsize=None)
def filtered(mutation=None):
    fs = VS.views_fusion(17, 33)
    return MR.filter_depths(fs["depth"], fs["poses"], mutated(fs["intr"], mutation), fs["filter_sources"], min_consistent=1, **filter_kw(fs))


def test_the_fusion_inputs_meet_the_edges_of_both_rules():
    import test_fuse_host as TF
    import test_mvs_host as TM
    fs = VS.views_fusion(17, 33)
    stats = {}
    out, count = MR.filter_depths(fs["depth"], fs["poses"], fs["intr"], fs["filter_sources"], min_consistent=2, stats=stats, **filter_kw(fs))
    # the equalities are the dyadic filter_scene's to meet; every other edge occurs here
    for name in TM.FILTER_EDGES:
        if "at equality" not in name:
            assert stats.get(name, 0) > 0, name
    assert set(np.unique(count)) >= {0, 1, 2, 3, 4} and np.isfinite(out).any()
    stats = {}
    cloud = FR.fuse(fs["depth"], fs["poses"], fs["intr"], fs["sources"], normal=fs["normal"], colour=fs["colour"], stats=stats, **fuse_kw(fs))
    for name in TF.EDGES:
        if "at equality" not in name:
            assert stats.get(name, 0) > 0, name
    assert set(np.unique(cloud["support"])) >= {0, 1, 2, 3}
    for v, row in enumerate(fs["sources"]):
        assert v in row or v % 2 == 1
        assert (row == -1).any() and len(set(row[row >= 0])) < (row >= 0).sum()


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_mistaken_intrinsics_row_changes_the_filter(mutation):
    """the filter's output is the input's depth or NaN, so a change is a pixel kept on one side only: counted over the pixels either
    side keeps at min_consistent = 1; the counts are compared over the same pixels"""
    (got, count), (ref, ref_count) = filtered(mutation), filtered()
    f = changed_fraction(got, ref)
    either = np.isfinite(got) | np.isfinite(ref)
    fc = float((count != ref_count)[either].mean())
    print(f"filter, intrinsics {mutation}: {f:.1%} of the kept pixels change, {fc:.1%} of their counts")
    assert f >= 0.5


@functools.lru_cache(maxsize=None)
def scored(w, t, mutation=None):
    """THE PLANE SCORE of the restated sweep's depth with the plane's true normal, the mutation in the score's intrinsics alone"""
    sc = VS.views_scene(17, 33, w)
    depth, normal = VS.views_state(sc, swept(w)[0])
    ps = PR.Scene(sc["images"], sc["poses"], mutated(sc["intr"], mutation), sc["sources"], sc["refs"], tap_step=t, **sweep_kw(sc))
    return PR.plane_score(ps, depth, normal)


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("w,t", [(3, 2), (4, 2)])
def test_a_mistaken_intrinsics_row_changes_the_plane_score(w, t, mutation):
    ref = scored(w, t)
    f = changed_fraction(scored(w, t, mutation), ref)
    print(f"plane score, w = {w}, t = {t}, intrinsics {mutation}: {f:.1%} of the scores change")
    assert f >= 0.5 and 4 * np.isfinite(ref).sum() >= 3 * (17 - 2 * w) * (33 - 2 * w)


def per_pixel(cloud, name, shape):
    out = np.full((int(np.prod(shape)), cloud[name].shape[1]), np.nan, F32)
    out[cloud["pixel"]] = cloud[name]
    return out.reshape(tuple(shape) + (-1,))


@functools.lru_cache(maxsize=None)
def fused(mutation=None, normals="true"):
    fs = VS.views_fusion(17, 33)
    normal = fs["normal"]
    if normals == "turned the wrong way":
        # R_v R_v n: what THE FUSION RULE's R_v^T turns into R_v n, the world normal of a kernel that took R_v for its transpose
        Rm = fs["poses"].astype(np.float64)[:, :, :3]
        normal = np.einsum("vij,vjk,vhwk->vhwi", Rm, Rm, normal.astype(np.float64)).astype(F32)
    return FR.fuse(fs["depth"], fs["poses"], mutated(fs["intr"], mutation), fs["sources"], normal=normal, colour=fs["colour"], **fuse_kw(fs))


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_mistaken_intrinsics_row_changes_the_fusion(mutation):
    got, ref = fused(mutation), fused()
    shape = ref["support"].shape
    f = changed_fraction(per_pixel(got, "points", shape), per_pixel(ref, "points", shape))
    n = int((got["support"] != ref["support"]).sum())
    print(f"fusion, intrinsics {mutation}: {f:.1%} of the points change, the support of {n} pixels")
    assert f >= 0.5 and n > 0


def test_a_rotation_taken_for_its_transpose_changes_the_fused_normals():
    got, ref = fused(normals="turned the wrong way"), fused()
    shape = ref["support"].shape
    a, b = per_pixel(got, "normals", shape), per_pixel(ref, "normals", shape)
    both = np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1)
    moved = differ(a, b).any(axis=-1) & both
    angle = np.degrees(np.arccos(np.clip((a[both].astype(np.float64) * b[both]).sum(axis=1), -1, 1)))
    print(f"{int(moved.sum())} of {int(both.sum())} emitted normals change, by {np.median(angle):.1f} degrees in the median")
    assert both.sum() > 100 and 2 * moved.sum() >= both.sum() and np.median(angle) > 1.0
    # and between two views the relative rotation's transpose fails the angle test elsewhere: the support changes
    assert (got["support"] != ref["support"]).any()


# -------------------------------------------------------------------------------------------------------------- the torch forms
def _torch(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("w", [3, 4])
def test_plane_sweep_torch_on_the_cpu_leaves_the_restatement_s_bits(w):
    from ls2fm import mvs
    sc = VS.views_scene(17, 33, w)
    got = mvs.plane_sweep_torch(*(_torch(sc[k]) for k in ("images", "poses", "intr", "sources", "depths")), refs=_torch(sc["refs"]), **sweep_kw(sc))
    for g, r in zip(got, swept(w)):
        assert same_bits(g.numpy(), r)


@pytest.mark.parametrize("min_consistent", [1, 2])
def test_filter_depths_torch_on_the_cpu_leaves_the_restatement_s_bits(min_consistent):
    from ls2fm import mvs
    fs = VS.views_fusion(17, 33)
    kw = dict(filter_kw(fs), min_consistent=min_consistent)
    want = MR.filter_depths(fs["depth"], fs["poses"], fs["intr"], fs["filter_sources"], **kw)
    got = mvs.filter_depths_torch(_torch(fs["depth"]), _torch(fs["poses"]), _torch(fs["intr"]), _torch(fs["filter_sources"]), **kw)
    assert np.isfinite(want[0]).any() and np.isnan(want[0]).any()
    assert same_bits(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])


@pytest.mark.parametrize("w,t", [(3, 2), (4, 2)])
def test_the_patchmatch_torch_forms_on_the_cpu_leave_the_restatement_s_bits(w, t):
    from ls2fm import mvs
    sc = VS.views_scene(17, 33, w)
    ps = PR.Scene(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["refs"], tap_step=t, **sweep_kw(sc))
    depth, normal = VS.views_state(sc, swept(w)[0], edges=True)
    score = PR.plane_score(ps, depth, normal)
    v = tuple(_torch(sc[k]) for k in ("images", "poses", "intr", "sources"))
    refs = _torch(sc["refs"])
    got = mvs.plane_score_torch(*v, _torch(depth), _torch(normal), refs=refs, tap_step=t, **sweep_kw(sc))
    assert same_bits(got.numpy(), score) and np.isfinite(score).any() and np.isnan(score).any()
    state = [_torch(depth).clone(), _torch(normal).clone(), got.clone()]
    lo, hi = sc["depths"].min(axis=1), sc["depths"].max(axis=1)
    for colour in (1, 0):
        PR.step(ps, depth, normal, score, colour, 1, 9, d_min=lo, d_max=hi, **PERTURB)
        mvs.patch_match_step_torch(*v, *state, colour, 1, _torch(lo), _torch(hi), refs=refs, seed=9, tap_step=t, **PERTURB, **sweep_kw(sc))
        for g, r in zip(state, (depth, normal, score)):
            assert same_bits(g.numpy(), r)


@pytest.mark.parametrize("normals,colours,C", [(True, True, 3), (False, True, 1), (True, False, 3)])
def test_fuse_depths_torch_on_the_cpu_leaves_the_restatement_s_bits(normals, colours, C):
    import test_fuse_host as TF
    from ls2fm import mvs
    fs = VS.views_fusion(17, 33, C)
    want = FR.fuse(fs["depth"], fs["poses"], fs["intr"], fs["sources"], normal=fs["normal"] if normals else None,
                   colour=fs["colour"] if colours else None, **fuse_kw(fs))
    got = mvs.fuse_depths_torch(_torch(fs["depth"]), _torch(fs["poses"]), _torch(fs["intr"]), _torch(fs["sources"]),
                                normal=_torch(fs["normal"]) if normals else None, images=_torch(fs["colour"]) if colours else None, **fuse_kw(fs))
    TF.check_cloud(got, want, fs)
    assert len(want["pixel"]) > 100
