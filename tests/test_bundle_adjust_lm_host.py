"""CPU checks of the Levenberg-Marquardt bundle adjustment: the restatement's two routes agree on every scene the device tests use (and
the scenes meet the conditions those tests rely on), ls2fm.stage.LMBALoop's torch path matches the restatement per iteration, the
solver converges, constants stay constant, and the refusals of the class and of the C ABI (the library loads without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import ba_lm_restate as LR
import ba_restate as BR
from ls2fm import _lib, stage

LOOP_ITERS = 8


@pytest.mark.parametrize("name", ["edges", "single", "pair", "small"])
def test_routes_agree_and_loop_matches(name):
    s, a, b = LR.reference(name, LOOP_ITERS, **LR.LOOP_KW)
    LR.routes_agree(name, a, b)
    assert a["state"]["done"] and a["state"]["reason"] == 2 and (a["log"][:, 3] == -1).any()       # the stop and rows after it
    loop = LR.build_loop(s, max_iter=LOOP_ITERS, **LR.LOOP_KW)
    LR.check_against_routes(name, loop.run(), loop, a, b)


def test_edge_scene_has_what_the_device_test_needs():
    s = LR.scene_edges()
    counts = np.diff(s["view_start"]).tolist()
    assert counts == [60, 1, 255, 256, 257, 120, 90]
    per_point = np.bincount(s["op"], minlength=s["X"].shape[0])
    assert per_point[0] == 6 and (per_point == 0).sum() >= 40 and (per_point == 1).any() and (per_point >= 2).any()
    ids = LR.lists_of(s)[1]
    assert len(np.intersect1d(ids[2], ids[5])) == 0
    p = LR.scene_pair()
    assert len(np.intersect1d(p["op"][:40], p["op"][40:])) == 1 and not p["view_const"].any()


@pytest.mark.parametrize("loss", ["soft_l1", "cauchy"])
def test_robust_losses(loss):
    name = "small"
    s, a, b = LR.reference(name, LOOP_ITERS, loss=loss, c=1.5, **LR.LOOP_KW)
    LR.routes_agree(f"{name}/{loss}", a, b)
    loop = LR.build_loop(s, max_iter=LOOP_ITERS, loss=loss, loss_scale=1.5, **LR.LOOP_KW)
    LR.check_against_routes(f"{name}/{loss}", loop.run(), loop, a, b)
    t = LR.reference(name, LOOP_ITERS, **LR.LOOP_KW)[1]
    assert not np.allclose(t["log"][:, 0], a["log"][:, 0])                                   # the loss is felt


def test_cap_scene_one_iteration():
    s, a, b = LR.reference("cap", 1)
    LR.routes_agree("cap", a, b)
    assert s["poses"].shape[0] == stage.LMBALoop.MAX_VIEWS and a["log"][0, 3] == 1.0
    loop = LR.build_loop(s, max_iter=1)
    LR.check_against_routes("cap", loop.run(), loop, a, b)


def test_pivot_scene_rejects_on_cost_and_on_a_pivot():
    s, a, b = LR.reference("pivot", LR.PIVOT_ITERS, **LR.PIVOT_KW)
    LR.routes_agree("pivot", a, b)
    log = a["log"]
    on_pivot = np.isnan(log[:, 1]) & (log[:, 3] == 0)
    on_cost = ~np.isnan(log[:, 1]) & (log[:, 3] == 0)
    assert on_pivot.any() and on_cost.any() and (log[:, 3] == 1).any(), log
    assert (log[on_pivot, 2] < 2.0 ** -53).all()                                              # the damping that rounds away
    # no decision hangs on rounding: every candidate differs from the cost by far more than the routes' gap
    rel = np.abs(log[:, 1] - log[:, 0])[~np.isnan(log[:, 1])] / log[~np.isnan(log[:, 1]), 0]
    assert rel.min() > 1e-4, rel
    assert np.array_equal(a["poses"][-1], np.eye(3, 4)) and np.array_equal(b["poses"][-1], np.eye(3, 4))        # the extra view never moves
    loop = LR.build_loop(s, max_iter=LR.PIVOT_ITERS, **LR.PIVOT_KW)
    LR.check_against_routes("pivot", loop.run(), loop, a, b)


def test_noise_free_scene_converges_to_zero():
    s = LR.scene_small(seed=22, noise=0.0, exact_constants=True)
    loop = LR.build_loop(s, max_iter=50)
    logs = loop.run()
    n = s["op"].shape[0]
    reason, iters = loop.stopped()
    print(f"[ba_lm] noise-free: cost {float(logs['cost'][0]):.3e} -> {float(loop.cost()):.3e} in {iters} iterations ({reason})")
    assert float(loop.cost()) < 1e-16 * n and iters <= 50


def test_beats_adam_on_the_synthetic_scene():
    """ba_restate.synthetic_scene(): the final cost (1/2 sum |r|^2) is below what TradBALoop reaches in 1000 iterations.  Most points
    of that scene have ONE observation and Adam moves them, so the solver is allowed to as well (min_point_views = 1; their depth
    is held by the damping alone, which shows as rejected steps in the log -- the cost still falls below Adam's)"""
    sc = BR.synthetic_scene()
    V = len(sc["keypoints"])
    f32 = lambda a: torch.tensor(np.asarray(a))
    views = stage.TrackedViews(f32(sc["se3"]), f32(sc["intrinsic"]), torch.zeros(V, 1, 3), [f32(k) for k in sc["keypoints"]],
                               [f32(i) for i in sc["track_ids"]], f32(sc["xyzs"]), 1, 1)
    adam = stage.TradBALoop(views, max_iter=1000)
    adam.run()
    lm = stage.LMBALoop(views, max_iter=50, min_point_views=1)
    lm.run()
    k = sc["intrinsic"].astype(np.float64)
    k4 = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    uv = np.concatenate(sc["keypoints"]).astype(np.float64)
    cost = lambda poses, X: LR.cost_of(poses, X, sc["obs_point"], sc["obs_view"], uv, k4, "trivial", 1.0)
    adam_poses = BR.se3_to_SE3(adam.poses_se3().double()).numpy()
    c_adam, c_lm = cost(adam_poses, adam.xyzs_all.double().numpy()), cost(lm.poses.numpy(), lm.xyzs_all.numpy())
    print(f"[ba_lm] synthetic scene: cost Adam x 1000 {c_adam:.6e}, LM {c_lm:.6e} after {lm.stopped()}")
    assert c_lm < c_adam
    assert abs(c_lm - float(lm.cost())) <= 1e-9 * c_lm
    unseen = np.setdiff1d(np.arange(sc["xyzs"].shape[0]), sc["obs_point"])
    assert len(unseen) >= BR.SCENE_UNSEEN and np.array_equal(lm.xyzs_all.numpy()[unseen], sc["xyzs"][unseen].astype(np.float64))


def test_constants_do_not_move():
    s = LR.scene_small()
    loop = LR.build_loop(s, max_iter=4)
    loop.run()
    const = np.nonzero(s["view_const"])[0]
    assert len(const) == 2 and np.array_equal(loop.poses.numpy()[const], s["poses"][const])
    assert (loop.poses.numpy()[~s["view_const"]] != s["poses"][~s["view_const"]]).any(axis=(1, 2)).all()
    single = LR.point_constant(s["op"], s["X"].shape[0]) & (np.bincount(s["op"], minlength=s["X"].shape[0]) == 1)
    assert single.any() and np.array_equal(loop.xyzs_all.numpy()[single], s["X"][single])
    # their cameras still feel them: with ONE view every point has one observation, and the pose moves and the cost falls
    one = LR.scene_single()
    lone = LR.build_loop(one, max_iter=4)
    logs = lone.run()
    assert np.array_equal(lone.xyzs_all.numpy(), one["X"]) and not np.array_equal(lone.poses.numpy(), one["poses"])
    assert float(lone.cost()) < 0.5 * float(logs["cost"][0])
    # all views constant: points only; all points constant (min_point_views above every count): poses only
    pts = LR.build_loop(s, max_iter=3, constant_views=range(5))
    pts.run()
    assert np.array_equal(pts.poses.numpy(), s["poses"]) and not np.array_equal(pts.xyzs_all.numpy(), s["X"])
    pos = LR.build_loop(s, max_iter=3, min_point_views=6)
    pos.run()
    assert np.array_equal(pos.xyzs_all.numpy(), s["X"]) and not np.array_equal(pos.poses.numpy(), s["poses"])


@pytest.mark.parametrize("kind", ["points only", "poses only"])
def test_points_only_and_poses_only_routes_agree(kind):
    s, kw, a, b = LR.variant_reference(kind)
    LR.routes_agree(kind, a, b)
    assert (a["log"][:, 3] == 1).all()
    loop = LR.build_loop(s, max_iter=3, **kw)
    LR.check_against_routes(kind, loop.run(), loop, a, b)


def test_step_equals_run_and_resumes():
    s = LR.scene_small()
    a, b = LR.build_loop(s, max_iter=6), LR.build_loop(s, max_iter=6)
    la = a.run(3)
    lb = [b.step() for _ in range(3)]
    for k in stage.LMBALoop.KEYS:
        assert torch.equal(la[k], torch.stack([r[k] for r in lb])), k
    assert torch.equal(a.poses, b.poses) and torch.equal(a.xyzs_all, b.xyzs_all) and a.it == b.it == 3
    a.run()
    assert a.it == a.max_iter and a.stopped()[0] in ("max_iter", "step", "gradient")
    with pytest.raises(ValueError):
        a.run()
    with pytest.raises(ValueError):
        LR.build_loop(s).run(0)
    assert a.poses_se3().shape == (5, 6) and a.mean_error().dim() == 0


def test_refusals():
    s = LR.scene_small()
    v = LR.views_of(s)
    v.host_intrinsic = v.host_intrinsic.clone()
    v.host_intrinsic[0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        stage.LMBALoop(v)
    v = LR.views_of(s)
    v.host_intrinsic = v.host_intrinsic.clone()
    v.host_intrinsic[2, 2] = 2.0
    with pytest.raises(ValueError, match="last row"):
        stage.LMBALoop(v)
    v = LR.views_of(s)
    v.track_ids[1] = v.track_ids[1].clone()
    v.track_ids[1][3] = v.track_ids[1][7]
    with pytest.raises(ValueError, match="duplicate"):
        stage.LMBALoop(v)
    big = LR.scene((2,) * 129, 40, 1, constant=())
    with pytest.raises(ValueError, match="128"):
        stage.LMBALoop(LR.views_of(big))
    with pytest.raises(ValueError, match="loss"):
        stage.LMBALoop(LR.views_of(s), loss="huber")
    with pytest.raises(ValueError, match="cam_pick"):
        stage.LMBALoop(LR.views_of(s), cam_pick=[0, 0])


def test_c_abi_refusals_before_any_device_work():
    lib = _lib.load()
    wb = lib.ls2fm_bundle_adjust_lm_workspace_bytes
    assert wb(3, 10, 0) == -1 and wb(0, 10, 5) == -1 and wb(3, 0, 5) == -1
    assert wb(129, 10, 500) == -2 and wb(128, 10, 500) > 0                        # LS2FM_ERR_UNSUPPORTED above the cap
    assert wb(128, 10, 500) > 8 * (6 * 128) ** 2                                  # the reduced system lives in the workspace
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ls2fm_bundle_adjust_lm_prepare(null, 3, null, 0, 10, null, 2, null, null) == -1
    assert lib.ls2fm_bundle_adjust_lm_prepare(p, 129, p, 500, 10, p, 2, p, null) == -2
    assert lib.ls2fm_bundle_adjust_lm_prepare(p, 3, p, 5, 10, p, 0, p, null) == -1           # min_point_views < 1
    assert lib.ls2fm_bundle_adjust_lm_prepare(p, 3, p, 5, 10, p, 2, null, null) == -4        # LS2FM_ERR_WORKSPACE
    k = (ctypes.c_double * 4)(500.0, 500.0, 320.0, 240.0)

    def run(n_views=1, n_obs=4, n_iters=5, ws=p, loss=0, scale=1.0, lam=1e-4, k4=k):
        o = _lib.BALMOpts(loss, scale, lam, 1e-10, 1e-10, 2)
        return lib.ls2fm_bundle_adjust_lm_run(p, p, p, n_views, 1, n_obs, k4, ctypes.byref(o), n_iters, p, p, ws, null)
    assert run(n_obs=0) == -1 and run(n_iters=0) == -1 and run(n_iters=-3) == -1
    assert run(loss=3) == -1 and run(scale=0.0) == -1 and run(lam=float("nan")) == -1
    assert run(k4=(ctypes.c_double * 4)(0.0, 500.0, 1.0, 1.0)) == -1
    assert run(n_views=129) == -2
    assert run(ws=null) == -4
    assert ctypes.sizeof(_lib.BALMOpts) == 48
