"""CPU: the host side of ls2fm.mapper -- the two new symbols and the unchanged ABI number, MapperOptions' refusals, the two rankings
on hand-made tables, the refusal of CPU tensors, the numpy restatement (tests/mapper_restate.py) on hand-computed cases, the
preconditions of the GPU tests' scenes (no decision within the restatement's margins of a threshold: the cap on such cases is
zero), and pose_graph()'s round trip through np.save."""
import io
import os
import re

import numpy as np
import pytest
import torch

import mapper_restate as MR
import mapper_scenes as MS
from conftest import ROOT
from ls2fm import _lib

NEW = ("ls2fm_view_scores_workspace_bytes", "ls2fm_view_scores", "ls2fm_update_observations_workspace_bytes", "ls2fm_update_observations")


@pytest.fixture(scope="module")
def M():
    from ls2fm import mapper
    return mapper


def test_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name + "(" in header and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert int(re.search(r"#define\s+LS2FM_ABI_VERSION\s+(\d+)", header).group(1)) == 13
    assert _lib.ABI_VERSION == 13 and lib.ls2fm_abi_version() == 13
    assert int(re.search(r"#define\s+LS2FM_VIEW_SCORE_MAX\s+(\d+)", header).group(1)) == MR.SCORE_MAX == 17895696
    for name, bit in (("BAD_START", 1), ("BAD_VIEW", 2), ("BAD_PIXEL", 4)):
        assert int(re.search(rf"#define\s+LS2FM_MAPPER_{name}\s+(\d+)", header).group(1)) == bit == getattr(MR, name)
    # refusals that need no device: counts out of range
    assert lib.ls2fm_view_scores_workspace_bytes(-1, 3, 0) < 0 and lib.ls2fm_view_scores_workspace_bytes(1, 0, 0) < 0
    assert lib.ls2fm_update_observations_workspace_bytes(1 << 31, 3, 0) < 0 and lib.ls2fm_update_observations_workspace_bytes(5, 3, 10) > 0


def test_options_defaults_and_refusals(M):
    o = M.MapperOptions()
    assert (o.init_min_num_inliers, o.init_min_tri_angle_deg, o.init_candidates, o.init_max_h_inlier_ratio) == (100, 16.0, 16, 0.8)
    assert (o.abs_pose_max_error_px, o.abs_pose_min_num_inliers, o.abs_pose_min_inlier_ratio, o.next_view_candidates) == (12.0, 30, 0.25, 4)
    assert (o.tri_max_error_px, o.tri_min_angle_deg) == (4.0, 1.5)
    assert (o.local_ba_views, o.local_ba_iters, o.global_ba_iters, o.global_ba_every, o.seed) == (6, 1000, 1000, 1, 0)
    assert o.ba_rates() == dict(lr_pose_r=5e-3, lr_pose_t=1e-2, lr_xyzs=1e-2, lr_sdf=1e-4, lr_sdf_end=5e-5)        # TradBALoop's
    bad = [dict(init_min_num_inliers=0), dict(init_min_tri_angle_deg=-1.0), dict(init_min_tri_angle_deg=91.0), dict(init_candidates=0),
           dict(abs_pose_max_error_px=0.0), dict(abs_pose_max_error_px=float("nan")), dict(abs_pose_min_num_inliers=2),
           dict(abs_pose_min_inlier_ratio=1.5), dict(init_max_h_inlier_ratio=-0.1), dict(next_view_candidates=0), dict(tri_max_error_px=float("inf")),
           dict(tri_min_angle_deg=100.0), dict(local_ba_views=1), dict(local_ba_iters=-1), dict(global_ba_iters=2.5),
           dict(global_ba_every=0), dict(seed=-3), dict(lr_xyzs=0.0), dict(next_view_candidates=True)]
    for kw in bad:
        with pytest.raises(ValueError, match=next(iter(kw))):
            M.MapperOptions(**kw)
    with pytest.raises(TypeError):
        M.reconstruct([{}, {}], np.eye(3), 4, 4, options=dict(seed=1))


def _tables(counts, n_views):
    """tables whose pair (a, b) has counts[(a, b)] kept matches and two masked ones"""
    tables = []
    for v in range(n_views):
        idx, msk = [], []
        for j in range(n_views):
            if j == v:
                continue
            c = counts.get((min(v, j), max(v, j)), 0)
            m = np.stack([np.arange(c + 2), np.arange(c + 2)], axis=1).astype(np.uint32) if c else np.zeros((0, 2), np.uint32)
            idx.append(m)
            msk.append(np.r_[np.ones(c, bool), np.zeros(2, bool)] if c else np.zeros(0, bool))
        tables.append(dict(kypts=np.zeros((50, 2)), indxes=idx, mask=msk))
    return tables


def test_init_pair_ranking(M):
    t = _tables({(0, 1): 12, (0, 2): 30, (1, 2): 30, (1, 3): 9, (2, 3): 30, (0, 3): 10}, 4)
    assert M.rank_init_pairs(t, 10, 16) == [(0, 2, 30), (1, 2, 30), (2, 3, 30), (0, 1, 12), (0, 3, 10)]      # ties: the lower (a, b)
    assert M.rank_init_pairs(t, 10, 2) == [(0, 2, 30), (1, 2, 30)]
    assert M.rank_init_pairs(t, 31, 16) == []
    assert M.rank_init_pairs(t, 1, 16)[-1] == (1, 3, 9)                                                    # masked rows do not count


def test_candidate_ranking(M):
    score = [900, 50, 700, 700, 0, 700, 5460]
    num = [40, 30, 30, 29, 0, 31, 1]
    reg = [True, False, False, False, False, False, False]
    assert M.rank_candidates(score, num, reg, 30) == [2, 5, 1]        # 0 registered, 3 and 6 see too few, 2 before 5 on the tie
    assert M.rank_candidates(score, num, reg, 1) == [6, 2, 3, 5, 1]
    assert M.rank_candidates(score, num, [True] * 7, 1) == []


def test_cpu_tensors_are_refused(M):
    tr = dict(track_start=torch.tensor([0, 2], dtype=torch.int32), obs_view=torch.tensor([0, 1], dtype=torch.int32))
    uv = torch.zeros(2, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        M.view_scores(tr, uv, torch.ones(2), torch.ones(1), torch.tensor([True, False]), (640, 480))
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        M.update_observations(tr, uv, torch.zeros(2, 3, 4, dtype=torch.float64), (600.0, 600.0, 320.0, 240.0), torch.tensor([True, True]),
                              torch.zeros(1, 3, dtype=torch.float64), torch.ones(1))
    with pytest.raises(ValueError, match="max_error_px"):
        M.update_observations(tr, uv, torch.zeros(2, 3, 4), (600.0, 600.0, 320.0, 240.0), [1, 1], torch.zeros(1, 3), [1], max_error_px=0.0)


def _one_view(pixels, size=(640.0, 480.0)):
    """view 0 registered, view 1 with the given pixels, one two-view track each"""
    n = len(pixels)
    uv = np.zeros((2 * n, 2))
    uv[1::2] = pixels
    return MR.view_scores((2 * np.arange(n + 1)), np.tile([0, 1], n), uv, np.ones(2 * n, bool), np.ones(n, bool), [True, False], size)


def test_restated_score_by_hand():
    score, num, status = _one_view([(100.0, 100.0)])
    assert score.tolist() == [0, 4 + 16 + 64 + 256 + 1024 + 4096] and score[1] == 5460 and num.tolist() == [0, 1] and status == 0
    score, num, _ = _one_view([(100.0, 100.0), (101.0, 101.5)])                 # cells of 10 x 7.5 px: both in cell (10, 13)
    assert score[1] == 5460 and num[1] == 2
    score, _, _ = _one_view([(100.0, 100.0), (111.0, 100.0)])                   # neighbours of one level-5 cell: (10, 13), (11, 13)
    assert score[1] == 5460 + 4096
    score, _, _ = _one_view([(0.0, 0.0), (639.0, 479.0)])                       # opposite corners: nothing shared at any level
    assert score[1] == 2 * 5460
    cx, cy = np.meshgrid(np.arange(64), np.arange(64))
    score, num, _ = _one_view(np.stack([(cx.ravel() + 0.5) * 10.0, (cy.ravel() + 0.5) * 7.5], axis=1))
    assert score[1] == 17895696 == MR.SCORE_MAX and num[1] == 4096
    # the clamp: on and beyond the borders
    assert [MR.cell(x, 640.0) for x in (-3.0, 0.0, 9.999, 10.0, 629.999, 630.0, 640.0, 1e9)] == [0, 0, 0, 1, 62, 63, 63, 63]
    score, num, status = _one_view([(float("nan"), 5.0)])
    assert score[1] == 0 and num[1] == 1 and status == MR.BAD_PIXEL


def test_restated_score_flags():
    t = MS.score_tables()["v3"]
    args = (t["track_start"], t["obs_view"], t["obs_uv"], t["obs_keep"])
    score, num, _ = MR.view_scores(*args, t["track_valid"], np.ones(3, bool), t["image_size"])
    assert not score.any() and not num.any()                                    # all registered
    score, num, _ = MR.view_scores(*args, t["track_valid"], np.zeros(3, bool), t["image_size"])
    assert not score.any() and not num.any()                                    # none registered: nothing is seen
    score, num, _ = MR.view_scores(*args, np.zeros_like(t["track_valid"]), t["registered"], t["image_size"])
    assert not score.any() and not num.any()                                    # no valid track
    score, num, _ = MR.view_scores(*args, t["track_valid"], t["registered"], t["image_size"])
    assert score[~t["registered"]].all() and (score[t["registered"]] == 0).all() and score.max() <= MR.SCORE_MAX


def test_restated_upkeep_by_hand():
    """two cameras a unit apart looking down z, a point at depth 2: e2 and the angle are known in closed form"""
    P = np.array([np.c_[np.eye(3), [0.0, 0.0, 0.0]], np.c_[np.eye(3), [-1.0, 0.0, 0.0]]])          # centres (0,0,0) and (1,0,0)
    intr = (100.0, 100.0, 50.0, 50.0)
    X = np.array([[0.5, 0.0, 2.0]])
    exact = np.array([[75.0, 50.0], [25.0, 50.0]])
    r = MR.update_observations(P, intr, [1, 1], [0, 2], [0, 1], exact + [[3.0, 0.0], [0.0, -3.9]], X, [1])
    assert r["obs_keep"].tolist() == [1, 1] and r["num_kept"].tolist() == [2] and r["track_valid"].tolist() == [True]
    assert abs(r["tri_angle"][0] - 2.0 * np.arctan(0.25)) < 1e-15
    r = MR.update_observations(P, intr, [1, 1], [0, 2], [0, 1], exact + [[3.0, 0.0], [0.0, -4.1]], X, [1])
    assert r["obs_keep"].tolist() == [1, 0] and r["track_valid"].tolist() == [False] and r["tri_angle"][0] == 0.0
    r = MR.update_observations(P, intr, [1, 0], [0, 2], [0, 1], exact, X, [1])                      # view 1 not registered
    assert r["obs_keep"].tolist() == [1, 0] and not r["track_valid"][0]
    r = MR.update_observations(P, intr, [1, 1], [0, 2], [0, 1], exact, X, [0])                      # the track was not valid
    assert r["obs_keep"].tolist() == [0, 0] and r["num_kept"].tolist() == [0]
    r = MR.update_observations(P, intr, [1, 1], [0, 2], [0, 1], exact, X, [1], min_tri_angle_deg=30.0)
    assert r["obs_keep"].tolist() == [1, 1] and not r["track_valid"][0]                             # 28.07 degrees
    r = MR.update_observations(P, intr, [1, 1], [0, 2], [0, 1], exact, -X, [1])                     # behind both
    assert r["obs_keep"].tolist() == [0, 0]


def test_upkeep_scenes_keep_clear_of_the_thresholds():
    """the GPU comparison is exact on EVERY track: no decision of any scene may lie within the margins (the cap is zero)"""
    for name, sc in MS.upkeep_scenes().items():
        res, mg = MR.update_observations(sc["poses"], sc["intr"], sc["registered"], sc["track_start"], sc["obs_view"], sc["obs_uv"],
                                         sc["X"], sc["track_valid"], margins=True)
        kept, T = int(res["obs_keep"].sum()), len(sc["track_valid"])
        print(f"[precondition] {name}: error margin {mg['error_px']:.3e} px, angle {mg['angle']:.3e} rad, depth {mg['depth']:.3e}; "
              f"{kept} of {len(res['obs_keep'])} observations kept, {int(res['track_valid'].sum())} of {T} tracks valid")
        assert mg["error_px"] > MS.ERR_MARGIN_PX and mg["angle"] > MS.ANGLE_MARGIN and mg["depth"] > MS.DEPTH_MARGIN, name
        for t in sc["lost"] + sc["behind"]:
            assert res["num_kept"][t] == 0 and not res["track_valid"][t], (name, t)
        if name == "one_view":
            assert not res["track_valid"].any() and res["num_kept"].max() <= 1
        else:
            # the scene decides both ways: observations dropped and kept, tracks dropped and kept
            assert 0 < kept < len(res["obs_keep"]) and 0 < int(res["track_valid"].sum()) < T or name in ("len2", "cap"), name
        if sc["low_parallax"].any():
            low = sc["low_parallax"] & sc["track_valid"]
            assert low.any() and not res["track_valid"][low].any(), name
    sc = MS.upkeep_scenes()["longest"]
    n = np.diff(sc["track_start"])
    res = MR.update_observations(sc["poses"], sc["intr"], sc["registered"], sc["track_start"], sc["obs_view"], sc["obs_uv"], sc["X"],
                                 sc["track_valid"])
    assert n.max() == 4096 and res["num_kept"][n == 4096].min() > 64 and res["num_kept"].max() > 3000


def test_edge_pixels_sit_on_counting_observations():
    """the pixels at 0, at W and H exactly, on cell borders, negative and far outside must reach the cell computation: each lies on
    an observation that counts, by the restatement's own rule, and the cells they must land in are the clamp's"""
    for name in ("v3", "v70"):
        t = MS.score_tables()[name]
        assert len(t["edge_obs"]) == len(t["edge_pixels"]) == 9 and len(set(t["edge_obs"].tolist())) == 9, name
        assert np.array_equal(t["obs_uv"][t["edge_obs"]], t["edge_pixels"]), name
        owner, _ = MR.track_of_observations(t["track_start"], len(t["obs_view"]))
        seen = np.zeros(len(t["track_valid"]), bool)
        for o in range(len(owner)):
            if t["track_valid"][owner[o]] and t["obs_keep"][o] and t["registered"][t["obs_view"][o]]:
                seen[owner[o]] = True
        for o in t["edge_obs"]:
            assert seen[owner[o]] and not t["registered"][t["obs_view"][o]], (name, o)
        cells = [(MR.cell(x, MS.W), MR.cell(y, MS.H)) for x, y in t["edge_pixels"]]
        assert cells == [(0, 0), (63, 63), (0, 0), (63, 63), (10, 10), (10, 63), (63, 63), (0, 0), (63, 0)], cells


def test_stride_scene_passes_the_capped_grid():
    """uo_angle's grid is capped at 4096 workgroups of 256 lanes: the tiled scene must number pairs beyond it, and keep clear of the
    thresholds like the others"""
    sc, tiled = MS.stride_scene()
    res, mg = MR.update_observations(sc["poses"], sc["intr"], sc["registered"], sc["track_start"], sc["obs_view"], sc["obs_uv"], sc["X"],
                                     sc["track_valid"], margins=True)
    assert mg["error_px"] > MS.ERR_MARGIN_PX and mg["angle"] > MS.ANGLE_MARGIN and mg["depth"] > MS.DEPTH_MARGIN
    m = np.minimum(res["num_kept"].astype(np.int64), 64)
    pairs = (m * (m - 1) // 2)[np.arange(MS.STRIDE_COPIES) % 16]
    first_beyond = int(np.searchsorted(np.cumsum(pairs), MS.PAIR_LANE_LIMIT, side="right"))
    print(f"[precondition] stride: {int(pairs.sum())} pairs against {MS.PAIR_LANE_LIMIT} lanes; tracks {first_beyond + 1} .. {MS.STRIDE_COPIES - 1} "
          f"lie wholly beyond; error margin {mg['error_px']:.3e} px")
    assert pairs.sum() > 2 * MS.PAIR_LANE_LIMIT and first_beyond < MS.STRIDE_COPIES - 100 and res["track_valid"].all()
    assert len(tiled["track_start"]) == MS.STRIDE_COPIES + 1


def test_pose_graph_round_trip(M):
    rec = M.Reconstruction([4, 1, 0, 3], np.array([True, True, False, True, True]), None, None, None, None, None, None, np.eye(3), 4, 4,
                           {}, [])
    buf = io.BytesIO()
    np.save(buf, rec.pose_graph())
    buf.seek(0)
    back = np.load(buf, allow_pickle=True)[:]
    assert back.dtype.kind == "i" and back.tolist() == [4, 1, 0, 3]
    assert [i for i in range(5) if i not in back] == [2]                         # what the reference's driver appends
