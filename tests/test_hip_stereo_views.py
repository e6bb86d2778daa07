"""GPU: the stereo chain -- ls2fm_mvs_sweep, ls2fm_mvs_filter, ls2fm_mvs_plane_score, ls2fm_mvs_patchmatch_step, ls2fm_mvs_fuse_mark and
ls2fm_mvs_fuse_emit through ls2fm.mvs -- on stereo_views_scenes: four turned cameras with intrinsics of their own, references that
are not the identity, and source rows up to LS2FM_MVS_MAX_SOURCES.  Every output by its bits against the numpy restatements
(tests/mvs_restate.py, tests/patchmatch_restate.py, tests/fuse_restate.py): each kernel operation is one rounded fp32 (in the
fusion's sums, fp64) operation in the rule's order, so equality is the rule.  That the scene would show a view's intrinsics taken
for another's, or a rotation for its transpose, is judged on the restatements (tests/test_stereo_views_host.py)."""
import functools

import numpy as np
import pytest
import torch

import fuse_restate as FR
import mvs_restate as MR
import patchmatch_restate as PR
import stereo_views_scenes as VS
from test_hip_fuse import check as check_cloud
from test_hip_mvs import check as check_sweep
from test_hip_mvs import dev, same
from test_hip_patchmatch import check as check_state

pytestmark = pytest.mark.gpu
PERTURB = dict(depth_perturb=0.02, normal_perturb=0.5, max_slope=1.0)


@pytest.fixture(scope="module")
def MV():
    from ls2fm import mvs
    return mvs


def sweep_kw(sc, **over):
    return dict(dict(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"]), **over)


def filter_kw(fs):
    return dict(near=fs["near"], max_reproj=fs["max_reproj"], rel_depth=fs["rel_depth"])


def fuse_kw(fs):
    return dict(filter_kw(fs), max_normal_angle=fs["max_normal_angle"])


def views(sc):
    return (dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"])), dev(sc["refs"])


def d_range(sc):
    return sc["depths"].min(axis=1), sc["depths"].max(axis=1)


# ----------------------------------------------------------------------------------------------------------------------- sweep
@functools.lru_cache(maxsize=None)
def swept(H, W, w):
    sc = VS.views_scene(H, W, w)
    return MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], **sweep_kw(sc))


# 17 x 33 is one pixel past the sweep's 16 x 16 tile, PatchMatch's 16 x 32 and the fusion's 32 x 8; 32 x 48 has whole tiles
@pytest.mark.parametrize("H,W,w", [(17, 33, 2), (17, 33, 3), (17, 33, 4), (32, 48, 4)])
def test_sweep_bits_of_the_restatement(MV, H, W, w):
    sc = VS.views_scene(H, W, w)
    ref = swept(H, W, w)
    v, refs = views(sc)
    check_sweep(MV.plane_sweep(*v, dev(sc["depths"]), refs=refs, **sweep_kw(sc)), ref)
    assert (ref[2] >= 0).any() and (ref[2] < 0).any() and len(np.unique(ref[2])) > 3
    if (H, w) == (17, 3):
        check_sweep(MV.plane_sweep(*v, dev(sc["depths"]), refs=refs, max_workspace_bytes=1, **sweep_kw(sc)), ref, "one reference per chunk")


# ---------------------------------------------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("H,W,min_consistent", [(17, 33, 1), (17, 33, 2), (32, 48, 2)])
def test_filter_bits_of_the_restatement(MV, H, W, min_consistent):
    fs = VS.views_fusion(H, W)
    kw = dict(filter_kw(fs), min_consistent=min_consistent)
    rf, rc = MR.filter_depths(fs["depth"], fs["poses"], fs["intr"], fs["filter_sources"], **kw)
    f, c = MV.filter_depths(dev(fs["depth"]), dev(fs["poses"]), dev(fs["intr"]), dev(fs["filter_sources"]), **kw)
    torch.cuda.synchronize()
    same(c, rc, "count")
    same(f, rf, "filtered")
    assert set(np.unique(rc)) >= {0, 1, 2, 3, 4} and np.isfinite(rf).any() and np.isnan(rf).any()


# ------------------------------------------------------------------------------------------------------------------ PatchMatch
@functools.lru_cache(maxsize=None)
def scene_of(w, t):
    sc = VS.views_scene(17, 33, w)
    return PR.Scene(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["refs"], tap_step=t, **sweep_kw(sc))


@functools.lru_cache(maxsize=None)
def scored(w, t, edges):
    """THE PLANE SCORE of the restated sweep's depth with the plane's true normal in each reference's frame, plain or disturbed"""
    depth, normal = VS.views_state(VS.views_scene(17, 33, w), swept(17, 33, w)[0], edges)
    return depth, normal, PR.plane_score(scene_of(w, t), depth, normal)


WINDOWS = [(2, 1), (3, 1), (3, 2), (4, 1), (4, 2)]


@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("w,t", WINDOWS)
def test_plane_score_bits_of_the_restatement(MV, w, t, edges):
    sc = VS.views_scene(17, 33, w)
    depth, normal, want = scored(w, t, edges)
    v, refs = views(sc)
    got = MV.plane_score(*v, dev(depth), dev(normal), refs=refs, tap_step=t, **sweep_kw(sc))
    torch.cuda.synchronize()
    same(got, want, f"plane_score, w = {w}, t = {t}")
    # the plain state scores nearly wherever the sweep found its depth; the disturbances take scores away
    assert np.isnan(want).any() and 10 * np.isfinite(want).sum() >= (3 if edges else 9) * np.isfinite(swept(17, 33, w)[0]).sum()


@functools.lru_cache(maxsize=None)
def stepped(w, t, first):
    """from the disturbed state: the state after colour `first` and after the other colour"""
    depth, normal, score = (a.copy() for a in scored(w, t, True))
    lo, hi = d_range(VS.views_scene(17, 33, w))
    out = []
    for i, colour in enumerate((first, 1 - first)):
        PR.step(scene_of(w, t), depth, normal, score, colour, 2 * first, 4 + first, d_min=lo, d_max=hi, **PERTURB)
        out.append((depth.copy(), normal.copy(), score.copy()))
    return out


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("w,t", WINDOWS)
def test_patch_match_step_bits_of_the_restatement(MV, w, t, first):
    """both colours in both orders; the order 1, 0 at iteration 2 under another seed"""
    sc = VS.views_scene(17, 33, w)
    ref = stepped(w, t, first)
    v, refs = views(sc)
    depth, normal, score = (dev(a) for a in scored(w, t, True))
    lo, hi = (dev(a) for a in d_range(sc))
    for i, colour in enumerate((first, 1 - first)):
        out = MV.patch_match_step(*v, depth, normal, score, colour, 2 * first, lo, hi, refs=refs, seed=4 + first, tap_step=t, **PERTURB,
                                  **sweep_kw(sc))
        check_state(out, ref[i], f"after colour {colour}")
    before, after = scored(w, t, True)[2], ref[1][2]
    assert (np.isfinite(after).sum() > np.isfinite(before).sum()) and (after[np.isfinite(before)] > before[np.isfinite(before)]).any()


@functools.lru_cache(maxsize=None)
def looped():
    sc = VS.views_scene(17, 33, 3)
    return PR.patch_match(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], iterations=2, seed=3,
                          **PERTURB, **sweep_kw(sc))


def test_patch_match_equals_the_restated_loop(MV):
    """plane_sweep -> plane_score -> 2 iterations of both colours at w = 3, t = 1, and the same one reference per chunk"""
    sc = VS.views_scene(17, 33, 3)
    want = looped()
    v, refs = views(sc)
    for kw in ({}, dict(max_workspace_bytes=1)):
        got = MV.patch_match(*v, dev(sc["depths"]), refs=refs, iterations=2, seed=3, **PERTURB, **sweep_kw(sc), **kw)
        check_state(got, want, f"patch_match {kw}")
    assert np.isfinite(want[2]).any() and np.isnan(want[2]).any()
    # the loop turned the fronto-parallel start toward the plane: the median angle to the true normal, in each reference's frame
    truth = sc["normal"][sc["refs"]][:, None, None, :]
    alive = np.isfinite(want[2])
    unit = want[1].astype(np.float64) / np.linalg.norm(want[1].astype(np.float64), axis=-1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((unit * truth).sum(axis=-1), -1, 1)))
    start = np.degrees(np.arccos(np.clip(-truth[..., 2], -1, 1))).min()
    assert np.median(angle[alive]) < start


# ---------------------------------------------------------------------------------------------------------------------- fusion
@functools.lru_cache(maxsize=None)
def fused(H, W, C, normals, colours):
    fs = VS.views_fusion(H, W, C)
    return FR.fuse(fs["depth"], fs["poses"], fs["intr"], fs["sources"], normal=fs["normal"] if normals else None,
                   colour=fs["colour"] if colours else None, **fuse_kw(fs))


def fuse_on_device(MV, fs, normals=True, colours=True, **kw):
    return MV.fuse_depths(dev(fs["depth"]), dev(fs["poses"]), dev(fs["intr"]), dev(kw.pop("sources", fs["sources"])),
                          normal=dev(fs["normal"]) if normals else None, images=dev(fs["colour"]) if colours else None, **fuse_kw(fs), **kw)


@pytest.mark.parametrize("H,W,C,normals,colours", [(17, 33, 3, True, True), (17, 33, 1, True, True), (17, 33, 3, True, False),
                                                   (17, 33, 1, False, True), (17, 33, 3, False, False), (32, 48, 3, True, True),
                                                   (32, 48, 1, False, True)])
def test_fusion_bits_of_the_restatement(MV, H, W, C, normals, colours):
    fs = VS.views_fusion(H, W, C)
    want = fused(H, W, C, normals, colours)
    check_cloud(fuse_on_device(MV, fs, normals, colours), want, fs)
    assert (want["support"] == 0).any() and (want["support"] >= 3).any() and len(want["pixel"]) > 100
    if (H, C, normals, colours) == (17, 3, True, True):
        check_cloud(fuse_on_device(MV, fs, max_workspace_bytes=1), want, fs, "one view per chunk")


# ------------------------------------------------------------------------------------------------------- the longest source row
def test_the_longest_source_rows(MV):
    """S = LS2FM_MVS_MAX_SOURCES = 64 on the 4 views: the rows repeated, a -1 in every fifth place and at the end.  A view listed n
    times counts n times by all three rules, so with min_sources = min_consistent = 3 the repeats decide, and the filter's count and
    the fusion's support exceed the number of views"""
    assert MV.MAX_SOURCES == 64
    sc = VS.views_scene(17, 33, 2)
    rows = VS.long_rows(sc["sources"])
    assert rows.shape == (3, 64) and (rows[:, -3:] == -1).all() and (rows >= 0).sum(axis=1).min() > 40
    kw = sweep_kw(sc, min_sources=3)
    want = MR.sweep(sc["images"], sc["poses"], sc["intr"], rows, sc["depths"], refs=sc["refs"], **kw)
    short = MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], **kw)
    v, refs = views(sc)
    check_sweep(MV.plane_sweep(*v[:3], dev(rows), dev(sc["depths"]), refs=refs, **kw), want, "S = 64")
    # a pixel with one or two valid views has three or more valid entries among their repeats
    assert np.isfinite(want[1]).sum() > np.isfinite(short[1]).sum() > 0

    fs = VS.views_fusion(17, 33)
    rows = VS.long_rows(fs["filter_sources"])
    fkw = dict(filter_kw(fs), min_consistent=3)
    rf, rc = MR.filter_depths(fs["depth"], fs["poses"], fs["intr"], rows, **fkw)
    f, c = MV.filter_depths(dev(fs["depth"]), dev(fs["poses"]), dev(fs["intr"]), dev(rows), **fkw)
    torch.cuda.synchronize()
    same(c, rc, "count, S = 64")
    same(f, rf, "filtered, S = 64")
    _, few = MR.filter_depths(fs["depth"], fs["poses"], fs["intr"], fs["filter_sources"], **fkw)
    assert rc.max() > 4 and ((rc >= 3) & (few < 3) & (few > 0)).any(), "the repeats are what reaches min_consistent"

    rows = VS.long_rows(fs["sources"])
    want = FR.fuse(fs["depth"], fs["poses"], fs["intr"], rows, normal=fs["normal"], colour=fs["colour"], **fuse_kw(fs))
    check_cloud(fuse_on_device(MV, fs, sources=rows), want, fs, "S = 64")
    assert want["support"].max() > 4
    some = fuse_on_device(MV, fs, sources=rows, min_support=3)
    keep = want["support"].reshape(-1)[want["pixel"]] >= 3
    same(some.pixel, want["pixel"][keep], "pixel, min_support 3")
    same(some.points, want["points"][keep], "points, min_support 3")
