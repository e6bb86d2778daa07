"""GPU: THE CAMERA BLOCK of the Levenberg-Marquardt bundle adjustment on the device (csrc/bundle_adjust_lm.hip's CAMERA
instantiations behind ls2fm.stage.LMBALoop(camera=, refine=)) against the numpy restatement's route (a), with the bar of
tests/ba_lm_restate.py: 4 x the gap between its two routes, floor 16 fp64 spacings.  tests/test_bundle_adjust_lm_camera_host.py
asserts on the CPU that the scenes meet the conditions relied on here.  Single process, single stream."""
import numpy as np
import pytest
import torch

import ba_lm_camera_restate as CR
import ba_lm_restate as LR
from ls2fm import _lib, stage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOOP_ITERS = 8


def bits(loop, logs=None):
    out = [loop.poses.clone(), loop.xyzs_all.clone(), loop.camera.clone(), loop._state.clone()]
    return out + ([torch.stack([logs[k] for k in stage.LMBALoop.KEYS])] if logs is not None else [])


def same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["cam6", "cam3", "cam_partial", "cam_cap"])
def test_one_iteration(name):
    s, a, b = CR.reference(name, 1)
    loop = CR.build_loop(s, CR.REFINE[name], DEV, max_iter=1)
    logs = loop.run()
    assert a["log"][0, 3] == 1.0
    CR.check_against_routes(name, logs, loop, a, b)
    const = LR.point_constant(s["op"], s["X"].shape[0])
    assert np.array_equal(loop.xyzs_all.cpu().numpy()[const], s["X"][const])
    assert np.array_equal(loop.poses.cpu().numpy()[s["view_const"]], s["poses"][s["view_const"]])


@pytest.mark.parametrize("name", ["cam6", "cam_partial"])
def test_loop_row_by_row(name):
    s, a, b = CR.reference(name, LOOP_ITERS, **CR.LOOP_KW)
    loop = CR.build_loop(s, CR.REFINE[name], DEV, max_iter=LOOP_ITERS, **CR.LOOP_KW)
    logs = loop.run()
    CR.check_against_routes(name, logs, loop, a, b)
    assert loop.stopped() == ("step", a["state"]["iters"]) and float(loop.cost()) == float(logs["cost"][-1])


def test_rejected_steps_row_by_row():
    s, a, b = CR.reference("cam_reject", CR.REJECT_ITERS)
    assert a["log"][:, 3].tolist() == [1.0, 0.0, 1.0, 0.0]
    loop = CR.build_loop(s, CR.REFINE["cam_reject"], DEV, max_iter=CR.REJECT_ITERS)
    CR.check_against_routes("cam_reject", loop.run(), loop, a, b)


@pytest.mark.parametrize("case", list(CR.MASK_CASES))
def test_masks(case):
    refine, cam, kw = CR.MASK_CASES[case]
    s, a, b = CR.reference("cam6", CR.MASK_ITERS, refine=refine, cam=cam, **kw)
    lkw = dict(kw)
    if "c" in lkw:
        lkw["loss_scale"] = lkw.pop("c")
    loop = CR.build_loop(s, refine, DEV, max_iter=CR.MASK_ITERS, **lkw)
    CR.check_against_routes(f"cam6/{case}", loop.run(), loop, a, b)
    mask, tie = CR.mask_of(refine)
    got = loop.camera.cpu().numpy()
    still = ~mask.copy()
    still[1] = still[1] and not tie
    assert np.array_equal(got[still], s["cam"][still]) and (not mask.any() or not np.array_equal(got[mask], s["cam"][mask]))


def test_zero_distortion_and_no_refinement_is_the_pinhole_loop():
    s = CR.scene_of("cam6")
    p = dict(s, k4=s["cam"][:4])
    a, b = (LR.run(route, p["poses"], p["X"], p["op"], p["ov"], p["uv"], p["k4"], p["view_const"], CR.MASK_ITERS, **CR.LOOP_KW)
            for route in ("schur", "full"))
    pin = LR.build_loop(p, DEV, max_iter=CR.MASK_ITERS, **CR.LOOP_KW)
    LR.check_against_routes("cam6 pinhole", pin.run(), pin, a, b)
    loop = CR.build_loop(s, (), DEV, max_iter=CR.MASK_ITERS, **CR.LOOP_KW)
    LR.check_against_routes("cam6 zero distortion", loop.run(), loop, a, b)
    assert np.array_equal(loop.camera.cpu().numpy(), s["cam"])


def test_camera_only():
    s, a, b = CR.reference("cam6", 3, view_const=np.ones(6, bool), min_point_views=7)
    loop = CR.build_loop(s, CR.DEFAULT, DEV, max_iter=3, constant_views=range(6), min_point_views=7)
    CR.check_against_routes("cam6 camera only", loop.run(), loop, a, b)
    assert np.array_equal(loop.poses.cpu().numpy(), s["poses"]) and np.array_equal(loop.xyzs_all.cpu().numpy(), s["X"])
    assert not np.array_equal(loop.camera.cpu().numpy(), s["cam"])


def test_clean_scene_recovers_the_camera():
    s = CR.scene_of("cam6_clean")
    loop = CR.build_loop(s, CR.DEFAULT, DEV, max_iter=20)
    loop.run()
    cam = loop.camera.cpu().numpy()
    reason, iters = loop.stopped()
    print(f"[ba_lm camera] clean: f {cam[0]!r} k1 {cam[4]!r} k2 {cam[5]!r} after {iters} iterations ({reason})")
    assert reason in ("gradient", "step", "lambda") and iters <= 20
    assert abs(cam[0] - 500.0) <= 5e-4 and cam[1] == cam[0]
    assert abs(cam[4] + 0.2) <= 1e-4 and abs(cam[5] - 0.05) <= 1e-4


def test_runs_repeat_and_split_calls_equal_one():
    s = CR.scene_of("cam_partial")
    one, two, split = (CR.build_loop(s, CR.DEFAULT, DEV, max_iter=7, **CR.LOOP_KW) for _ in range(3))
    l1, l2 = one.run(), two.run()
    assert same_bits(bits(one, l1), bits(two, l2))
    la, lb = split.run(3), split.run(4)
    joined = {k: torch.cat([la[k], lb[k]]) for k in la}
    assert same_bits(bits(one, l1), bits(split, joined)) and split.it == 7


def test_run_is_capturable_and_a_replay_continues_the_loop():
    s = CR.scene_of("cam6")
    eager, graphed = (CR.build_loop(s, CR.DEFAULT, DEV, max_iter=6, **CR.LOOP_KW) for _ in range(2))
    logs = [eager.run(2) for _ in range(3)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    rows = []
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            captured = graphed.run(2)
        for _ in range(3):                                  # capture runs nothing: three replays are the three calls
            g.replay()
            rows.append({k: v.clone() for k, v in captured.items()})
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for want, got in zip(logs, rows):
        assert all(torch.equal(want[k].view(torch.int64), got[k].view(torch.int64)) for k in want)
    assert same_bits(bits(eager), bits(graphed))


def test_more_views_than_the_cap_are_refused_and_the_next_call_works():
    lib = _lib.load()
    V, n, P = 127, 254, 40
    assert lib.ls2fm_bundle_adjust_lm_camera_workspace_bytes(V, P, n) == -2
    assert lib.ls2fm_bundle_adjust_lm_camera_workspace_bytes(V - 1, P, n) > lib.ls2fm_bundle_adjust_lm_workspace_bytes(V - 1, P, n) > 0
    buf = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    opts = _lib.BALMOpts(0, 1.0, 1e-4, 1e-10, 1e-10, 2)
    import ctypes
    run = lambda V, mask, tie, aspect: lib.ls2fm_bundle_adjust_lm_run_camera(
        _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), V, P, n, mask, tie, aspect, ctypes.byref(opts), 1, _lib.ptr(buf),
        _lib.ptr(buf), _lib.ptr(buf), _lib.stream_ptr())
    assert run(127, 1, 0, 1.0) == -2                                        # refused before anything is launched
    assert run(6, 1 << 12, 0, 1.0) == -1 and run(6, 3, 1, 1.0) == -1 and run(6, 2, 1, 1.0) == -1 and run(6, 1, 1, float("nan")) == -1
    with pytest.raises(ValueError, match="126"):
        CR.build_loop(CR.scene_cam_cap(V=127), CR.DEFAULT, DEV)
    s, a, b = CR.reference("cam3", 1)
    loop = CR.build_loop(s, CR.REFINE["cam3"], DEV, max_iter=1)
    CR.check_against_routes("cam3 after the refusal", loop.run(), loop, a, b)


def test_a_zero_focal_length_moves_nothing():
    s = CR.scene_of("cam3")
    loop = CR.build_loop(s, CR.DEFAULT, DEV, max_iter=2)
    loop.camera[1] = 0.0                                                   # after the loop was built: found on the device
    before = bits(loop)
    logs = loop.run(2)
    assert all(bool(torch.isnan(v).all()) for v in logs.values())
    assert same_bits(before, bits(loop))
