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
