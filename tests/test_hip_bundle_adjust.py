"""GPU: the classical bundle adjustment on the device (csrc/bundle_adjust.hip behind ls2fm.stage.TradBALoop) against the fixtures
recorded from the reference's own `BA_Trad.BA` (tests/golden/stage_ba_trad_*.npz), with the bars of tests/ba_restate.py: the
fixture's fp32-vs-fp64 gap per quantity times MARGIN.  Single process, single stream."""
import ctypes
import types

import numpy as np
import pytest
import torch

import ba_restate as BR
from ls2fm import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def state(loop):
    return [t.clone() for t in (loop.poses_se3(), loop.xyzs_all, *loop.written_back(), *loop._m)]


def same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("case", BR.CASES)
def test_device_loop_follows_the_reference_fp32_trajectory(case):
    g = BR.load_case(case)
    loop = BR.build_loop(g, DEV)
    logs = loop.run()
    assert (logs["w_reproj"].double().cpu().numpy() == g["f32/weight"]).all(), "weight sequence"
    BR.assert_within_gap(case, BR.distances(g, logs, loop))
    unpicked = np.setdiff1d(np.arange(g["xyzs"].shape[0]), g["obs_point"])
    assert np.array_equal(loop.xyzs_all.cpu().numpy()[unpicked].view(np.uint32), g["xyzs"][unpicked].view(np.uint32))
    assert not loop._m[2][torch.as_tensor(unpicked, device=DEV)].any() and not loop._m[3][torch.as_tensor(unpicked, device=DEV)].any()


def test_long_run_stays_with_the_reference():
    g = BR.load_case("long")
    loop = BR.build_loop(g, DEV)
    logs = loop.run()
    assert loop.it == 1000
    BR.assert_within_gap("long", BR.distances(g, logs, loop))
    err = logs["err_mean"].double().cpu().numpy()
    print(f"[ba_trad long] mean err {err[0]:.4f} -> {err[-1]:.4f} (reference {g['f32/err_mean'][0]:.4f} -> {float(g['f32/err_returned']):.4f})")
    assert err[-1] < err[0]


def test_split_calls_and_steps_equal_one_call_bit_for_bit():
    g = BR.load_case("global")
    one, two, steps = BR.build_loop(g, DEV), BR.build_loop(g, DEV), BR.build_loop(g, DEV)
    l1 = one.run(20)
    l2 = [two.run(10), two.run(10)]
    l3 = [steps.step() for _ in range(20)]
    for k in l1:
        assert torch.equal(l1[k], torch.cat([l2[0][k], l2[1][k]])) and torch.equal(l1[k], torch.stack([r[k] for r in l3])), k
    assert same_bits(state(one), state(two)) and same_bits(state(one), state(steps))


def test_two_runs_are_bit_identical():
    g = BR.load_case("heavy")
    a, b = BR.build_loop(g, DEV), BR.build_loop(g, DEV)
    la, lb = a.run(), b.run()
    assert all(torch.equal(la[k], lb[k]) for k in la) and same_bits(state(a), state(b))


def test_observation_order_inside_a_view_matters_for_rounding_only():
    g = BR.load_case("global")
    a, b = BR.build_loop(g, DEV), BR.build_loop(g, DEV, shuffle_seed=5)
    assert not torch.equal(a.obs_point, b.obs_point) and torch.equal(a.view_start, b.view_start)
    la, lb = a.run(), b.run()
    f = lambda t: t.double().cpu().numpy()
    dist = {"reproj": (np.abs(f(lb["reproj_error"]) / f(la["reproj_error"]) - 1).max(), float(g["gap/reproj"]), 2.0 ** -23),
            "err_mean": (np.abs(f(lb["err_mean"]) / f(la["err_mean"]) - 1).max(), float(g["gap/err_mean"]), 2.0 ** -23),
            "se3_final": (np.abs(f(b.poses_se3()) - f(a.poses_se3())).max(), float(g["gap/se3_final"]), float(np.spacing(np.float32(f(a.poses_se3()).max())))),
            "xyzs_final": (np.abs(f(b.xyzs_all) - f(a.xyzs_all)).max(), float(g["gap/xyzs_final"]), float(np.spacing(np.float32(f(a.xyzs_all).max()))))}
    BR.assert_within_gap("global, shuffled", dist)
    assert torch.equal(la["w_reproj"], lb["w_reproj"])


def test_error_paths_return_their_codes_and_a_valid_call_still_works():
    from ls2fm import stage
    g = BR.load_case("local")
    lib = _lib.load()
    kp, ids = BR.tracked_lists(g)
    t = lambda a, **kw: torch.tensor(a, device=DEV, **kw)

    def views(kp, ids):           # (what the loop reads of a TrackedViews; the class itself pads key points and takes no empty view)
        return types.SimpleNamespace(poses=t(g["se3"]), intrinsic=t(g["intrinsic"]), keypoints=[t(k) for k in kp],
                                     track_ids=[t(i) for i in ids], xyzs=t(g["xyzs"]))
    empty_k, empty_i = np.zeros((0, 2), np.float32), np.zeros(0, np.int64)
    with pytest.raises(RuntimeError, match="ls2fm_bundle_adjust"):            # zero observations
        stage.TradBALoop(views([empty_k] * 6, [empty_i] * 6), max_iter=20)
    with pytest.raises(RuntimeError, match="ls2fm_bundle_adjust_prepare"):    # a picked view with none
        stage.TradBALoop(views([kp[0], empty_k] + kp[2:], [ids[0], empty_i] + ids[2:]), cam_pick=[0, 1, 2], max_iter=20)
    for bad in (g["xyzs"].shape[0], -1):                                      # obs_point out of range, either side
        ids_bad = [i.copy() for i in ids]
        ids_bad[3][7] = bad
        with pytest.raises(RuntimeError, match="ls2fm_bundle_adjust_prepare"):
            stage.TradBALoop(views(kp, ids_bad), max_iter=20)
    loop = BR.build_loop(g, DEV)
    V, P, n = loop.se3.shape[0], loop.xyzs_all.shape[0], loop.obs_point.shape[0]
    log = torch.zeros(4, 3, device=DEV)

    def run(n_iters, ws):
        return lib.ls2fm_bundle_adjust_run(_lib.ptr(loop.se3), _lib.ptr(loop.xyzs_all), _lib.ptr(loop.obs_uv), V, P, n, loop._k_host, 5e-3, 1e-2, 1e-2,
                                           0.97, 1.0, 10.0, 10.0, *[_lib.ptr(m) for m in loop._m], 0, n_iters, _lib.ptr(log),
                                           _lib.ptr(loop.se3_entering_last), _lib.ptr(loop.xyzs_entering_last), ws, _lib.stream_ptr())
    before = [loop.se3.clone(), loop.xyzs_all.clone()]
    assert run(0, _lib.ptr(loop._ws)) == -1 and run(-1, _lib.ptr(loop._ws)) == -1 and run(4, ctypes.c_void_p(0)) == -4
    with pytest.raises(RuntimeError, match="ls2fm_bundle_adjust_run"):
        _lib.check(run(0, _lib.ptr(loop._ws)), "ls2fm_bundle_adjust_run")
    # a workspace that prepare never filled for these sizes: nothing moves, the log is NaN
    blank = torch.zeros_like(loop._ws)
    assert run(2, _lib.ptr(blank)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(log[:2]).all() and same_bits(before, [loop.se3, loop.xyzs_all])
    with pytest.raises(ValueError):
        loop.run(0)
    # afterwards a valid call still works, and gives what an untouched loop gives
    fresh = BR.build_loop(g, DEV)
    la, lb = loop.run(), fresh.run()
    assert all(torch.equal(la[k], lb[k]) for k in la) and same_bits(state(loop), state(fresh))
    BR.assert_within_gap("local, after refusals", BR.distances(g, la, loop))


def test_run_refuses_cleanly_under_graph_capture():
    g = BR.load_case("local")
    loop, fresh = BR.build_loop(g, DEV), BR.build_loop(g, DEV)
    pad = torch.zeros(8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        pad.add_(1.0)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        pad.add_(1.0)                                   # (the graph is not empty)
        with pytest.raises(RuntimeError, match="cannot be captured"):
            loop.run(5)
    torch.cuda.synchronize()
    assert loop.it == 0
    la, lb = loop.run(), fresh.run()                    # nothing was enqueued or moved by the refused call
    assert all(torch.equal(la[k], lb[k]) for k in la) and same_bits(state(loop), state(fresh))


# ------------------------------------------------------------------------------------------------ one iteration against float64
W1 = float(np.float32(0.1))                     # adam_element.h's w1 = (float)(1 - beta1)
OMB2 = float(np.float32(1.0 - 0.999))           # (float)(1 - beta2)


def _scene_views(sc):
    t = lambda a: torch.tensor(a, device=DEV)
    return types.SimpleNamespace(poses=t(sc["se3"]), intrinsic=t(sc["intrinsic"]), keypoints=[t(k) for k in sc["keypoints"]],
                                 track_ids=[t(i) for i in sc["track_ids"]], xyzs=t(sc["xyzs"]))


def _one_iteration(name, loop, zero_err_obs=()):
    """ONE device iteration from zero moments against ba_restate.one_iteration in float64.  After it m = w1 (wt g) exactly as
    fp32 rounds it, so m / w1 is the kernel's gradient; the bars are within_f32_gap's (4 x the CPU fp32-vs-fp64 distance of the
    same formula on the same inputs, floored at one fp32 spacing).  Then Adam's own arithmetic on the device's m and v."""
    f = lambda t: t.detach().double().cpu().numpy()
    se3_0, xyzs_0 = f(loop.se3), f(loop.xyzs_all)
    args = (se3_0, xyzs_0, loop.obs_point.cpu().numpy(), loop.obs_view.cpu().numpy(), f(loop.obs_uv), f(loop.intrinsic))
    r64 = BR.one_iteration(*args, torch.float64, zero_err_obs)
    r32 = BR.one_iteration(*args, torch.float32, zero_err_obs)
    assert r64["u_z"].min() > 0.5 and r64["weight"] == r32["weight"]
    assert all(not m.any() for m in loop._m) and loop.it == 0
    logs = loop.run(1)
    m_se3, v_se3, m_pts, v_pts = (f(m) for m in loop._m)
    se3_1, xyzs_1 = f(loop.se3), f(loop.xyzs_all)
    assert all(np.isfinite(a).all() for a in (m_se3, v_se3, m_pts, v_pts, se3_1, xyzs_1))
    wt = float(logs["w_reproj"][0])
    assert wt == r64["weight"], f"{name}: weight {wt} vs {r64['weight']}"
    bad = [BR.within_f32_gap(name, "reproj", float(logs["reproj_error"][0]), r64["reproj"], r32["reproj"]),
           BR.within_f32_gap(name, "err_mean", float(logs["err_mean"][0]), r64["err_mean"], r32["err_mean"]),
           BR.within_f32_gap(name, "wt d_se3", m_se3 / W1, wt * r64["d_se3"], wt * r32["d_se3"]),
           BR.within_f32_gap(name, "wt d_points", m_pts / W1, wt * r64["d_points"], wt * r32["d_points"])]
    for q, what in ((slice(0, 3), "rotation"), (slice(3, 6), "translation")):      # printed only: the bar above is the issue's
        BR.within_f32_gap(name, "  " + what, m_se3[:, q] / W1, wt * r64["d_se3"][:, q], wt * r32["d_se3"][:, q])
    assert not any(bad), f"{name}: beyond the bar: {[b for b in bad if b]}"
    # points no view observes: untouched, moments zero; every other point has a gradient in float64 unless its err is 0
    unseen = np.setdiff1d(np.arange(xyzs_0.shape[0]), args[2])
    assert not m_pts[unseen].any() and not v_pts[unseen].any()
    assert np.array_equal(loop.xyzs_all.cpu().numpy()[unseen].view(np.uint32), xyzs_0.astype(np.float32)[unseen].view(np.uint32))
    # v = (1 - beta2) (wt g)^2: m / w1 carries one rounding of g (2^-24, squared 2^-23), v two of its own (2 x 2^-24) -> 2^-22
    for m, v, what in ((m_se3, v_se3, "poses"), (m_pts, v_pts, "points")):
        want = OMB2 * (m / W1) ** 2
        rel = np.abs(v - want) / np.maximum(want, 2.0 ** -126)
        print(f"[{name}] v of the {what}: max relative distance from (1 - beta2) (m / w1)^2 {rel.max():.3e} (bar 2^-22 = {2.0 ** -22:.3e})")
        assert rel.max() <= 2.0 ** -22 * 1.01, f"{name}: v of the {what}"
    # the step, in float64 from the device's m and v with the call's fp32 scalars (bundle_adjust.hip): five fp32 roundings in
    # sqrt, /, +, /, * (bar 8 x 2^-24 of the step) and the rounding of p itself (half a spacing of p)
    bc2_sqrt, eps = float(np.float32(np.sqrt(1.0 - 0.999 ** 1.0))), float(np.float32(1e-8))
    lr = np.array([loop.lrs[0]] * 3 + [loop.lrs[1]] * 3)
    for p0, p1, m, v, rate, what in ((se3_0, se3_1, m_se3, v_se3, lr, "poses"), (xyzs_0, xyzs_1, m_pts, v_pts, loop.lrs[2], "points")):
        size = np.float32(rate / (1.0 - 0.9 ** 1.0)).astype(np.float64)
        step = size * (m / (np.sqrt(v) / bc2_sqrt + eps))
        bar = 0.5 * np.spacing(np.maximum(np.abs(p0), np.abs(p1)).astype(np.float32)).astype(np.float64) + 8 * 2.0 ** -24 * np.abs(step)
        d = np.abs((p0 - p1) - step)
        print(f"[{name}] step of the {what}: max distance / bar {(d / bar).max():.3f}, largest step {np.abs(step).max():.3e}")
        assert (d <= bar).all(), f"{name}: step of the {what}: {(d / bar).max():.3f} bars"
    return dict(r64=r64, m_pts=m_pts, v_pts=v_pts, xyzs_0=xyzs_0, xyzs_1=xyzs_1, m_se3=m_se3)


@pytest.mark.parametrize("case", ["local", "global", "heavy"])
def test_one_iteration_gradients_match_float64_on_the_fixtures(case):
    """The yardstick: |float32 on the CPU - float64| of ba_restate.one_iteration per quantity (absolute, maxima over the elements;
    the bar is 4 x this, floored at one fp32 spacing of the largest magnitude, given in brackets), computed without a device:
                    reproj            err_mean          wt d_se3          wt d_points
        local       1.54e-06 (4.15)   1.96e-06 (4.75)   7.77e-05 (64.8)   2.91e-06 (0.263)
        global      4.68e-07 (3.71)   4.13e-07 (4.23)   4.03e-05 (29.3)   2.94e-06 (0.274)
        heavy       1.50e-07 (14.5)   7.07e-07 (20.3)   1.84e-04 (274)    8.77e-06 (1.11)     wt = 10
        synthetic   9.99e-08 (2.19)   2.21e-07 (2.52)   5.00e-04 (6.06)   2.24e-06 (0.0391)
    within_f32_gap prints the device's distance next to each when the test runs."""
    _one_iteration(case, BR.build_loop(BR.load_case(case), DEV))


def test_one_iteration_gradients_match_float64_on_the_synthetic_scene():
    """ba_restate.synthetic_scene: theta = 0 / 1e-4 / 3.0, views of 1, 255, 256, 257 and 5000 observations, points seen once, by
    every view and by none, shuffled lists, and one observation whose key point is the kernel's fp32 projection bit for bit."""
    from ls2fm import stage
    sc = BR.synthetic_scene()
    loop = stage.TradBALoop(_scene_views(sc), max_iter=20)
    assert loop.view_start.cpu().tolist() == np.concatenate([[0], np.cumsum(BR.SCENE_COUNTS)]).tolist()
    out = _one_iteration("synthetic", loop, sc["zero_err_obs"])
    # err == 0: no gradient for the point only that observation sees, nothing moves, everything finite (asserted above)
    assert not out["m_pts"][1].any() and not out["v_pts"][1].any() and np.array_equal(out["xyzs_0"][1], out["xyzs_1"][1])
    assert out["m_pts"][0].all() and out["m_se3"].all()
    # the same scene with every view's list reversed: list order changes rounding only (the same bars hold again)
    sc2 = dict(sc, keypoints=[k[::-1].copy() for k in sc["keypoints"]], track_ids=[i[::-1].copy() for i in sc["track_ids"]])
    k0 = BR.SCENE_COUNTS[0] - 1 - sc["zero_err_obs"][0]
    _one_iteration("synthetic, reversed lists", stage.TradBALoop(_scene_views(sc2), max_iter=20), [k0])
