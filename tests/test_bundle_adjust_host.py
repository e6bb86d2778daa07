"""CPU: the classical bundle adjustment (ls2fm.stage.TradBALoop, the loop of the reference's pipelines/BA_Trad.py) against the
fixtures recorded from the reference's own `BA_Trad.BA` (tests/golden/make_golden_ba_trad.py): the fp64 restatement
(tests/ba_restate.py) against the reference's fp64 trajectory, the loop's torch path against its fp32 trajectory, the bookkeeping
(cam_pick, the observation list, unpicked points, the weight sequence), and the C ABI's refusals that return before any device
work.  Every tolerance is the fixture's own fp32-vs-fp64 gap times ba_restate.MARGIN."""
import ctypes

import numpy as np
import pytest
import torch

import ba_restate as BR
from ls2fm import _lib

# The restatement and the reference's fp64 run evaluate the same expressions in float64, in slightly different operation orders
# (autograd's vs the reference's graph, the series' powers): they differ by rounding only.  eps = 2.2e-16; a value passes through
# ~10^2 - 10^3 operations per iteration and Adam's m / sqrt(v) is O(1)-conditioned, so 20 iterations stay far below 1e-12
# (measured here: <= 9e-15).  Beyond ~60 iterations the loop itself amplifies rounding (Adam near its optimum jitters: the same
# two fp64 runs are 5e-7 apart at iteration 100 and saturate at the fp32 runs' distance by 300), so `long` is pinned over its
# first 50 iterations only.
RESTATE_TOL = 1e-12
LONG_PINNED = 50


def restated(g, n_iters):
    op, ov, uv, pick = BR.observation_list(g)
    return BR.run(g["se3"][pick].astype(np.float64), g["xyzs"], op, ov, uv, g["intrinsic"], n_iters, g["meta"]["iters"])


@pytest.mark.parametrize("case", BR.CASES)
def test_restatement_follows_the_reference_fp64_trajectory(case):
    g = BR.load_case(case)
    r = restated(g, g["meta"]["iters"])
    figures = {"reproj": np.abs(r["reproj"] / g["f64/reproj"] - 1).max(), "err_mean": np.abs(r["err_mean"] / g["f64/err_mean"] - 1).max(),
               "se3": np.abs(r["se3"] - np.concatenate([g["f64/r_final"], g["f64/t_final"]], 1)).max(),
               "xyzs": np.abs(r["xyzs"] - g["f64/xyzs_final"]).max(), "se3_written": np.abs(r["se3_written"] - g["f64/se3_written"]).max(),
               "xyzs_written": np.abs(r["xyzs_written"] - g["f64/xyzs_written"]).max(),
               "err_returned": abs(r["err_mean"][-1] / float(g["f64/err_returned"]) - 1)}
    print(case, figures)
    assert (r["weight"] == g["f64/weight"]).all()
    assert max(figures.values()) <= RESTATE_TOL, figures


def test_restatement_follows_the_long_run_while_rounding_is_not_amplified():
    g = BR.load_case("long")
    r = restated(g, LONG_PINNED)
    worst = max(np.abs(r["reproj"] / g["f64/reproj"][:LONG_PINNED] - 1).max(), np.abs(r["err_mean"] / g["f64/err_mean"][:LONG_PINNED] - 1).max())
    print("long, first", LONG_PINNED, "iterations:", worst)
    assert worst <= RESTATE_TOL, worst


@pytest.mark.parametrize("case", ["local", "heavy"])
def test_one_iteration_restatement_is_the_trajectory_s_first_step(case):
    """ba_restate.one_iteration (written on its own) against ba_restate.run's first iteration: the loss terms, and run's stepped
    parameters against Adam's first step formed from one_iteration's gradient -- the two restatements cannot drift apart"""
    g = BR.load_case(case)
    op, ov, uv, pick = BR.observation_list(g)
    se3 = g["se3"][pick].astype(np.float64)
    one = BR.one_iteration(se3, g["xyzs"], op, ov, uv, g["intrinsic"])
    r = BR.run(se3, g["xyzs"], op, ov, uv, g["intrinsic"], 1, g["meta"]["iters"])
    assert abs(one["reproj"] / r["reproj"][0] - 1) <= RESTATE_TOL and abs(one["err_mean"] / r["err_mean"][0] - 1) <= RESTATE_TOL
    assert one["weight"] == r["weight"][0] == g["f64/weight"][0]
    lrs = np.array([5e-3] * 3 + [1e-2] * 3)

    def stepped(p, grad, lr):                                   # m = 0.1 g, v = 0.001 g^2, both bias corrections at step 1
        gw = one["weight"] * grad
        return p - (lr / (1 - 0.9)) * (0.1 * gw) / (np.sqrt(0.001 * gw * gw) / np.sqrt(1 - 0.999) + 1e-8)
    assert np.abs(stepped(se3, one["d_se3"], lrs) - r["se3"]).max() <= RESTATE_TOL
    assert np.abs(stepped(g["xyzs"].astype(np.float64), one["d_points"], 1e-2) - r["xyzs"]).max() <= RESTATE_TOL
    unseen = np.setdiff1d(np.arange(g["xyzs"].shape[0]), op)
    assert not one["d_points"][unseen].any()


def test_synthetic_scene_holds_what_it_says():
    sc = BR.synthetic_scene()
    counts = [len(i) for i in sc["track_ids"]]
    assert tuple(counts) == BR.SCENE_COUNTS and {1, 255, 256, 257} <= set(counts) and max(counts) == 5000
    theta = np.linalg.norm(sc["se3"][:, :3].astype(np.float64), axis=1)
    assert theta[0] == 0 and not sc["se3"][0].any() and abs(theta[1] - 1e-4) < 1e-9 and abs(theta[6] - 3.0) < 1e-6
    seen = np.bincount(sc["obs_point"], minlength=BR.SCENE_POINTS)
    assert seen[0] == 7 and seen[1] == 1 and (seen == 1).sum() > 1000 and not seen[-BR.SCENE_UNSEEN:].any() and seen[:-BR.SCENE_UNSEEN].max() == 7
    assert all(len(np.unique(i)) == len(i) and not np.array_equal(i, np.sort(i)) for i in sc["track_ids"][2:])
    k0 = sc["zero_err_obs"][0]
    assert sc["obs_point"][k0] == 1 and sc["obs_view"][k0] == 0
    for dtype in (torch.float64, torch.float32):
        one = BR.one_iteration(sc["se3"], sc["xyzs"], sc["obs_point"], sc["obs_view"], sc["obs_uv"], sc["intrinsic"], dtype, sc["zero_err_obs"])
        assert one["u_z"].min() > 3.0 and np.isfinite(one["d_se3"]).all() and np.isfinite(one["d_points"]).all()
        assert not one["d_points"][1].any() and one["d_points"][0].all() and not one["d_points"][-BR.SCENE_UNSEEN:].any()
        assert one["weight"] == 1.0 and 1.0 < one["err_mean"] < 4.0
    # the key point of the pinned observation is within fp32 rounding of the float64 projection
    raw = BR.one_iteration(sc["se3"], sc["xyzs"], sc["obs_point"], sc["obs_view"], sc["obs_uv"], sc["intrinsic"])
    x = sc["xyzs"][1].astype(np.float64)
    uv = (sc["intrinsic"].astype(np.float64) @ x)[:2] / (x[2] + 1e-6)
    assert np.abs(uv - sc["obs_uv"][k0]).max() < 1e-4 and raw["err_mean"] > 0


@pytest.mark.parametrize("case", BR.CASES)
def test_loop_on_the_host_follows_the_reference_fp32_trajectory(case):
    g = BR.load_case(case)
    loop = BR.build_loop(g, "cpu")
    assert loop.max_iter == g["meta"]["iters"]                      # a single picked camera halves max_iter
    logs = loop.run()
    assert (logs["w_reproj"].double().numpy() == g["f32/weight"]).all(), "weight sequence"
    BR.assert_within_gap(case, BR.distances(g, logs, loop))
    # the written-back state is the one that ENTERED the last iteration, not the stepped one
    assert not torch.equal(loop.written_back()[0], loop.poses_se3())


@pytest.mark.parametrize("case", ["local", "single"])
def test_unpicked_points_do_not_move(case):
    g = BR.load_case(case)
    loop = BR.build_loop(g, "cpu")
    loop.run()
    unpicked = np.setdiff1d(np.arange(g["xyzs"].shape[0]), g["obs_point"])
    assert len(unpicked) > 0
    assert np.array_equal(loop.xyzs_all.numpy()[unpicked].view(np.uint32), g["xyzs"][unpicked].view(np.uint32))
    assert np.array_equal(loop.written_back()[1].numpy()[unpicked].view(np.uint32), g["xyzs"][unpicked].view(np.uint32))
    picked = np.unique(g["obs_point"])
    assert (loop.xyzs_all.numpy()[picked] != g["xyzs"][picked]).any(axis=1).all()          # every picked point did


def test_heavy_fixture_records_both_weights_away_from_the_threshold():
    g = BR.load_case("heavy")
    w = g["f32/weight"]
    assert w[0] == 10.0 and w[-1] == 1.0 and set(w.tolist()) == {1.0, 10.0}                # the switch is inside the window
    assert (np.diff(w) <= 0).all()
    # no recorded loss within the fp32 gap (times the margin) of the threshold: the weight sequence is decided by the arithmetic
    assert np.abs(g["f64/reproj"] - 10.0).min() > BR.MARGIN * float(g["gap/reproj"]) * 10.0
    assert (g["f32/weight"] == np.where(g["f32/reproj"] > 10, 10.0, 1.0)).all()


@pytest.mark.parametrize("case", BR.CASES + ("long",))
def test_cam_pick_order_and_observation_list_are_the_reference_s(case):
    g = BR.load_case(case)
    loop = BR.build_loop(g, "cpu")
    assert loop.cam_pick == [int(c) for c in g["cam_pick"]]
    assert np.array_equal(loop.obs_point.numpy(), g["obs_point"])
    assert np.array_equal(loop.obs_view.numpy(), g["obs_view"])
    assert np.array_equal(loop.obs_uv.numpy(), g["obs_uv"])
    assert np.array_equal(loop.view_start.numpy(), np.concatenate([[0], np.cumsum(np.bincount(g["obs_view"]))]))
    if case == "local":                                                 # the fixture has what the issue asks of it
        per_point = np.bincount(g["obs_point"], minlength=g["xyzs"].shape[0])
        assert (per_point == 1).any() and (per_point == 3).any() and (per_point == 0).any() and list(g["cam_pick"]) != sorted(g["cam_pick"])


def test_step_equals_run_and_resumes():
    g = BR.load_case("local")
    a, b = BR.build_loop(g, "cpu"), BR.build_loop(g, "cpu")
    la = a.run(6)
    lb = [b.step() for _ in range(6)]
    assert torch.equal(la["reproj_error"], torch.stack([r["reproj_error"] for r in lb]))
    assert torch.equal(a.poses_se3(), b.poses_se3()) and torch.equal(a.xyzs_all, b.xyzs_all)
    assert a.it == b.it == 6
    a.run()
    assert a.it == a.max_iter
    with pytest.raises(ValueError):
        a.run()
    with pytest.raises(ValueError):
        BR.build_loop(g, "cpu").run(0)


def test_c_abi_refusals_before_any_device_work():
    lib = _lib.load()
    assert lib.ls2fm_bundle_adjust_workspace_bytes(3, 10, 0) < 0                    # zero observations
    assert lib.ls2fm_bundle_adjust_workspace_bytes(0, 10, 5) < 0 and lib.ls2fm_bundle_adjust_workspace_bytes(3, 0, 5) < 0
    assert lib.ls2fm_bundle_adjust_workspace_bytes(3, 10, 5) > 0
    null, k = ctypes.c_void_p(0), (ctypes.c_float * 9)(*np.eye(3).ravel().tolist())
    assert lib.ls2fm_bundle_adjust_prepare(null, 3, null, 0, 10, null, null) == -1   # LS2FM_ERR_INVALID_ARGUMENT
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def run(n_obs, n_iters, ws):
        return lib.ls2fm_bundle_adjust_run(p, p, p, 1, 1, n_obs, k, 1e-3, 1e-3, 1e-3, 0.99, 1.0, 10.0, 10.0, p, p, p, p, 0, n_iters, p, p, p, ws, null)
    assert run(0, 5, p) == -1 and run(4, 0, p) == -1 and run(4, -3, p) == -1
    assert run(4, 5, null) == -4                                                      # LS2FM_ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="invalid argument|INVALID"):
        _lib.check(run(4, 0, p), "ls2fm_bundle_adjust_run")
