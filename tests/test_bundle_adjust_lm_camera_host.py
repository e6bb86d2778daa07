"""CPU: THE CAMERA BLOCK of the Levenberg-Marquardt bundle adjustment (include/ls2fm.h).  The Jacobians against central differences,
the restatement's two routes on every scene the GPU tests use (they agree exactly in every decision: no decision hangs on
rounding), ls2fm.stage.LMBALoop's torch path against the routes, the recovery of a known camera, ls2fm.mapper.refine_camera, and
the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import ba_lm_camera_restate as CR
import ba_lm_restate as LR
from ls2fm import stage

LOOP_ITERS = 8


# ------------------------------------------------------------------------------------------------------------ Jacobians
def _numeric(f, x0, scale):
    """central differences of f: R^m -> R^(n, 2) with h = 1e-6 x the word's scale -> [n, 2, m]"""
    cols = []
    for k in range(len(x0)):
        h = 1e-6 * scale[k]
        xp, xm = x0.copy(), x0.copy()
        xp[k] += h
        xm[k] -= h
        cols.append((f(xp) - f(xm)) / (xp[k] - xm[k]))
    return np.stack(cols, axis=-1)


def _columns_close(name, J, Jn):
    """the bar: 1e-7 of the column's largest entry (truncation about 1e-12 and rounding about 1e-10 of it: a margin of 1000)"""
    for k in range(J.shape[-1]):
        top = np.abs(Jn[..., k]).max()
        err = np.abs(J[..., k] - Jn[..., k]).max()
        print(f"[ba_lm camera] {name} column {k}: largest {top:.3e}, against central differences {err:.3e}")
        assert err <= 1e-7 * top, (name, k, err, top)


@pytest.fixture(scope="module")
def jac_scene():
    s = dict(CR.scene_of("cam3"), cam=CR.CAM_RATIONAL)
    assert (CR.CAM_RATIONAL != 0).all()
    pc = np.zeros(s["X"].shape[0], bool)
    vc = np.zeros(3, bool)
    Jc, Jp, Jk = CR.jacobians(s["poses"], s["X"], s["op"], s["ov"], s["cam"], vc, pc, np.ones(12, bool), False, 1.0)
    return s, Jc, Jp, Jk


def test_camera_jacobian_against_central_differences(jac_scene):
    s, Jc, Jp, Jk = jac_scene
    f = lambda c: CR.project(s["poses"], s["X"], s["op"], s["ov"], c)
    # a word's scale: the pinhole words' own size in pixels; 1 for the distortion words, coefficients of terms of order one in the
    # normalised plane (their own size, 1e-3 for a tangential word, would make h 1e-9 and leave the difference to rounding)
    _columns_close("J_k", Jk, _numeric(f, s["cam"].copy(), np.concatenate([np.abs(s["cam"][:4]), np.ones(8)])))


def test_projection_jacobian_against_central_differences(jac_scene):
    s, Jc, Jp, Jk = jac_scene
    n = len(s["op"])
    # J_proj is the translation part of J_c: move every observation's camera point by the same dt
    def f(dt):
        poses = s["poses"].copy()
        poses[:, :, 3] += dt
        return CR.project(poses, s["X"], s["op"], s["ov"], s["cam"])
    _columns_close("J_proj", Jc[:, :, 3:], _numeric(f, np.zeros(3), np.ones(3)))
    # and J_p = J_proj R through one point at a time (a point's move reaches only its own observations)
    Jn = np.zeros((n, 2, 3))
    for p in np.unique(s["op"]):
        def g(x, p=p):
            X = s["X"].copy()
            X[p] = x
            return CR.project(s["poses"], X, s["op"], s["ov"], s["cam"])
        sel = s["op"] == p
        Jn[sel] = _numeric(g, s["X"][p].copy(), np.ones(3))[sel]
    _columns_close("J_p", Jp, Jn)


def test_torch_jacobian_k_is_the_restatement(jac_scene):
    from ls2fm.undistort import _distort_torch, _jacobian_k_torch
    s, Jc, Jp, Jk = jac_scene
    xc = np.einsum("nij,nj->ni", s["poses"][s["ov"]][:, :, :3], s["X"][s["op"]]) + s["poses"][s["ov"]][:, :, 3]
    x, y = torch.tensor(xc[:, 0] / xc[:, 2]), torch.tensor(xc[:, 1] / xc[:, 2])
    c = torch.tensor(s["cam"]).unbind(0)
    xd, yd, shared = _distort_torch(c, x, y)
    ku, kv = _jacobian_k_torch(c, shared, x, y, xd, yd)
    J = torch.stack([torch.stack(ku, 1), torch.stack(kv, 1)], 1).numpy()
    assert np.abs(J - Jk).max() <= 1e-12 * np.abs(Jk).max()


def test_the_library_s_jacobians_against_central_differences_of_its_own_projection(jac_scene):
    """the torch forms the loop composes (ls2fm.undistort's rule, its Jacobian and J_k, LMBALoop._camera_jacobians) differentiated
    on their own: a wrong column in the library fails here, whatever the restatement says"""
    from ls2fm.undistort import _distort_torch
    s, _, _, _ = jac_scene
    xc = np.einsum("nij,nj->ni", s["poses"][s["ov"]][:, :, :3], s["X"][s["op"]]) + s["poses"][s["ov"]][:, :, 3]

    def image(cam, pts):
        c = torch.tensor(cam).unbind(0)
        p = torch.tensor(pts)
        xd, yd, _ = _distort_torch(c, p[:, 0] / p[:, 2], p[:, 1] / p[:, 2])
        return torch.stack([c[0] * xd + c[2], c[1] * yd + c[3]], dim=1).numpy()
    Jproj, Jk = (t.numpy() for t in stage.LMBALoop._camera_jacobians(torch.tensor(s["cam"]), torch.tensor(xc)))
    _columns_close("library J_k", Jk, _numeric(lambda c: image(c, xc), s["cam"].copy(), np.concatenate([np.abs(s["cam"][:4]), np.ones(8)])))
    _columns_close("library J_proj", Jproj, _numeric(lambda d: image(s["cam"], xc + d), np.zeros(3), np.ones(3)))


# ------------------------------------------------------------------------------------- the scenes the GPU tests rely on
CASES = [("cam6", 1, {}), ("cam3", 1, {}), ("cam_partial", 1, {}), ("cam_cap", 1, {}), ("cam6", LOOP_ITERS, CR.LOOP_KW),
         ("cam_partial", LOOP_ITERS, CR.LOOP_KW)]


@pytest.mark.parametrize("name,iters,kw", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_routes_agree_and_the_torch_path_matches(name, iters, kw):
    s, a, b = CR.reference(name, iters, **kw)
    CR.routes_agree(f"{name}/{iters}", a, b)
    loop = CR.build_loop(s, CR.REFINE[name], max_iter=iters, **kw)
    logs = loop.run()
    CR.check_against_routes(f"{name}/{iters}", logs, loop, a, b)
    CR.within_half_the_bar(f"{name}/{iters}", logs, loop, a, b)
    if iters > 1:
        assert a["state"]["done"] and a["state"]["reason"] == 2 and (a["log"][:, 3] != 0).all()


def test_rejected_steps_row_by_row():
    s, a, b = CR.reference("cam_reject", CR.REJECT_ITERS)
    CR.routes_agree("cam_reject", a, b)
    assert a["log"][:, 3].tolist() == [1.0, 0.0, 1.0, 0.0]
    loop = CR.build_loop(s, CR.REFINE["cam_reject"], max_iter=CR.REJECT_ITERS)
    logs = loop.run()
    CR.check_against_routes("cam_reject", logs, loop, a, b)
    CR.within_half_the_bar("cam_reject", logs, loop, a, b)


@pytest.mark.parametrize("case", list(CR.MASK_CASES))
def test_masks_routes_agree_and_the_torch_path_matches(case):
    refine, cam, kw = CR.MASK_CASES[case]
    s, a, b = CR.reference("cam6", CR.MASK_ITERS, refine=refine, cam=cam, **kw)
    CR.routes_agree(f"cam6/{case}", a, b)
    lkw = dict(kw)
    if "c" in lkw:
        lkw["loss_scale"] = lkw.pop("c")
    loop = CR.build_loop(s, refine, max_iter=CR.MASK_ITERS, **lkw)
    logs = loop.run()
    CR.check_against_routes(f"cam6/{case}", logs, loop, a, b)
    CR.within_half_the_bar(f"cam6/{case}", logs, loop, a, b)
    mask, tie = CR.mask_of(refine)
    still = ~mask.copy()
    still[1] = still[1] and not tie
    assert np.array_equal(a["cam"][still], s["cam"][still])


def test_camera_only_and_the_pinhole_equivalent_agree_between_the_routes():
    s, a, b = CR.reference("cam6", 3, view_const=np.ones(6, bool), min_point_views=7)
    CR.routes_agree("cam6 camera only", a, b)
    loop = CR.build_loop(s, CR.DEFAULT, max_iter=3, constant_views=range(6), min_point_views=7)
    CR.check_against_routes("cam6 camera only", loop.run(), loop, a, b)
    assert np.array_equal(a["poses"], s["poses"]) and np.array_equal(a["X"], s["X"]) and not np.array_equal(a["cam"], s["cam"])
    # zero distortion, nothing refined: the camera routes are the pinhole routes up to rounding
    p = dict(s, k4=s["cam"][:4])
    pa, pb = (LR.run(route, p["poses"], p["X"], p["op"], p["ov"], p["uv"], p["k4"], p["view_const"], CR.MASK_ITERS, **CR.LOOP_KW)
              for route in ("schur", "full"))
    LR.routes_agree("cam6 pinhole", pa, pb)
    loop = CR.build_loop(s, (), max_iter=CR.MASK_ITERS, **CR.LOOP_KW)
    LR.check_against_routes("cam6 zero distortion", loop.run(), loop, pa, pb)


# --------------------------------------------------------------------------------------------------------- convergence
def test_clean_scene_recovers_the_camera_and_a_held_wrong_camera_does_not():
    s = CR.scene_of("cam6_clean")
    loop = CR.build_loop(s, CR.DEFAULT, max_iter=20)
    loop.run()
    cam = loop.camera.numpy()
    reason, iters = loop.stopped()
    print(f"[ba_lm camera] clean: f {cam[0]!r} k1 {cam[4]!r} k2 {cam[5]!r} after {iters} iterations ({reason})")
    assert reason in ("gradient", "step", "lambda") and iters <= 20
    assert abs(cam[0] - 500.0) <= 5e-4 and cam[1] == cam[0]
    assert abs(cam[4] + 0.2) <= 1e-4 and abs(cam[5] - 0.05) <= 1e-4
    held = CR.build_loop(s, (), max_iter=20)
    held.run()
    rms = CR.rms(s, held.poses.numpy(), held.xyzs_all.numpy(), held.camera.numpy())
    print(f"[ba_lm camera] clean, the wrong camera held: rms {rms:.3f} px")
    assert np.array_equal(held.camera.numpy(), s["cam"]) and rms > 0.5


def _reconstruction_of(s):
    """a hand-built ls2fm.mapper.Reconstruction of a dense scene: one track per point, the observations in track order, the key
    points as the wrong pinhole camera would have undistorted them (not at all: zero distortion)"""
    from ls2fm import mapper as M
    V, P = s["poses"].shape[0], s["X"].shape[0]
    order = np.lexsort((s["ov"], s["op"]))
    op, ov, uv = s["op"][order], s["ov"][order], s["uv"][order]
    ts = np.concatenate([[0], np.cumsum(np.bincount(op, minlength=P))])
    tracks = dict(track_start=torch.tensor(ts), obs_view=torch.tensor(ov))
    k = s["cam"]
    K = torch.tensor([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return M.Reconstruction(list(range(V)), np.ones(V, bool), torch.tensor(s["poses"]), torch.tensor(s["X"]), torch.ones(P, dtype=torch.bool),
                            torch.ones(len(op), dtype=torch.bool), tracks, torch.tensor(uv), K, 480, 640, {}, [])


def test_refine_camera_on_a_reconstruction():
    from ls2fm import mapper as M
    s = CR.scene_of("cam6_clean")
    rec = _reconstruction_of(s)
    cam, out = M.refine_camera(rec, max_iter=20, loss="trivial", loss_scale=1.0)
    c = cam.numpy()
    print(f"[ba_lm camera] refine_camera: f {c[0]!r} k1 {c[4]!r} k2 {c[5]!r}")
    assert abs(c[0] - 500.0) <= 5e-4 and abs(c[4] + 0.2) <= 1e-4 and abs(c[5] - 0.05) <= 1e-4
    K = np.asarray(out.intrinsic)
    assert K.shape == (3, 3) and K[0, 0] == c[0] and K[1, 1] == c[1] and K[0, 2] == c[2] and K[1, 2] == c[3]
    ov, ts = out.tracks["obs_view"].numpy(), out.tracks["track_start"].numpy()
    op = np.repeat(np.arange(len(ts) - 1), np.diff(ts))
    err = np.abs(LR.project(out.poses.numpy(), out.X.numpy(), op, ov, c[:4]) - out.obs_uv.numpy()).max()
    print(f"[ba_lm camera] refine_camera: the returned key points against the returned pinhole {err:.3e} px")
    assert err < 1e-6
    assert out.order == rec.order and torch.equal(out.poses[0], rec.poses[0])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    s = CR.scene_of("cam3")
    with pytest.raises(ValueError, match="126"):
        CR.build_loop(CR.scene_cam_cap(V=127), CR.DEFAULT)
    with pytest.raises(ValueError, match="'f'"):
        CR.build_loop(s, ("f", "fx"))
    with pytest.raises(ValueError, match="focal"):
        CR.build_loop(s, ("focal",))
    with pytest.raises(ValueError, match="no camera"):
        stage.LMBALoop(LR.views_of(LR.scene_small()), refine=("k1",))
    with pytest.raises(ValueError, match="12 finite"):
        stage.LMBALoop(CR.views_of(s), camera=torch.zeros(12, dtype=torch.float64))


def test_entry_points_refuse_before_any_device_work():
    from ls2fm import _lib
    lib = _lib.load()
    wb, wc = lib.ls2fm_bundle_adjust_lm_workspace_bytes, lib.ls2fm_bundle_adjust_lm_camera_workspace_bytes
    assert wc(127, 10, 500) == -2 and wc(0, 10, 500) == -1
    assert wc(126, 10, 500) > wb(126, 10, 500) > 0
    p, null = ctypes.c_void_p(8), ctypes.c_void_p(0)
    o = _lib.BALMOpts(0, 1.0, 1e-4, 1e-10, 1e-10, 2)
    run = lambda V, mask, tie, aspect, ws=p, cam=p: lib.ls2fm_bundle_adjust_lm_run_camera(p, p, cam, p, V, 10, 500, mask, tie, aspect,
                                                                                         ctypes.byref(o), 1, p, p, ws, null)
    assert run(127, 1, 0, 1.0) == -2
    assert run(6, 1 << 12, 0, 1.0) == -1                           # a mask bit >= 12
    assert run(6, 3, 1, 1.0) == -1 and run(6, 2, 1, 1.0) == -1     # tie_focal needs bit 0 set and bit 1 clear
    assert run(6, 1, 1, float("inf")) == -1 and run(6, 1, 0, float("nan")) == -1
    assert run(6, 1, 0, 1.0, cam=null) == -1
    assert run(6, 1, 0, 1.0, ws=null) == -4
