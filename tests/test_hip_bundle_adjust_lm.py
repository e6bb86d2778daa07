"""GPU: the Levenberg-Marquardt bundle adjustment on the device (csrc/bundle_adjust_lm.hip behind ls2fm.stage.LMBALoop) against the
numpy restatement's route (a), with the bar of tests/ba_lm_restate.py: 4 x the gap between its two routes, floor 16 fp64 spacings.
tests/test_bundle_adjust_lm_host.py asserts on the CPU that the scenes meet the conditions relied on here (the routes agree exactly
in every decision, no decision hangs on rounding).  The step is compared through the state it produces (poses and points after the
iteration, at their own magnitude) and through the log's max |delta|: the device keeps delta itself in its workspace.
Single process, single stream."""
import ctypes

import numpy as np
import pytest
import torch

import ba_lm_restate as LR
from ls2fm import _lib, stage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOOP_ITERS = 8


def bits(loop, logs=None):
    out = [loop.poses.clone(), loop.xyzs_all.clone(), loop._state.clone()]
    return out + ([torch.stack([logs[k] for k in stage.LMBALoop.KEYS])] if logs is not None else [])


def same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["single", "pair", "edges", "cap"])
def test_one_iteration(name):
    s, a, b = LR.reference(name, 1, **({} if name == "cap" else LR.LOOP_KW))
    loop = LR.build_loop(s, DEV, max_iter=1, **({} if name == "cap" else LR.LOOP_KW))
    logs = loop.run()
    assert a["log"][0, 3] == 1.0
    LR.check_against_routes(name, logs, loop, a, b)
    unseen = np.setdiff1d(np.arange(s["X"].shape[0]), s["op"])
    assert np.array_equal(loop.xyzs_all.cpu().numpy()[unseen], s["X"][unseen])
    const = LR.point_constant(s["op"], s["X"].shape[0])
    assert np.array_equal(loop.xyzs_all.cpu().numpy()[const], s["X"][const])
    assert np.array_equal(loop.poses.cpu().numpy()[s["view_const"]], s["poses"][s["view_const"]])


@pytest.mark.parametrize("name", ["single", "pair", "edges", "small"])
def test_loop_row_by_row(name):
    s, a, b = LR.reference(name, LOOP_ITERS, **LR.LOOP_KW)
    loop = LR.build_loop(s, DEV, max_iter=LOOP_ITERS, **LR.LOOP_KW)
    logs = loop.run()
    LR.check_against_routes(name, logs, loop, a, b)
    assert loop.stopped() == ("step", a["state"]["iters"]) and float(loop.cost()) == float(logs["cost"][-1])


def test_more_views_than_the_cap_are_refused_and_the_next_call_works():
    lib = _lib.load()
    V, n, P = 129, 258, 40
    vs = torch.arange(0, n + 1, 2, dtype=torch.int32, device=DEV)
    op = (torch.arange(n, device=DEV) % P).to(torch.int32)
    vc = torch.zeros(V, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
    assert lib.ls2fm_bundle_adjust_lm_workspace_bytes(V, P, n) == -2
    assert lib.ls2fm_bundle_adjust_lm_prepare(_lib.ptr(vs), V, _lib.ptr(op), n, P, _lib.ptr(vc), 2, _lib.ptr(ws), _lib.stream_ptr()) == -2
    with pytest.raises(ValueError, match="128"):
        stage.LMBALoop(LR.views_of(LR.scene((2,) * 129, 40, 1, constant=()), DEV))
    s, a, b = LR.reference("pair", 1, **LR.LOOP_KW)
    loop = LR.build_loop(s, DEV, max_iter=1, **LR.LOOP_KW)
    LR.check_against_routes("pair after the refusal", loop.run(), loop, a, b)


def test_duplicate_observation_is_refused():
    v = LR.views_of(LR.scene_small(), DEV)
    v.track_ids[1] = v.track_ids[1].clone()
    v.track_ids[1][3] = v.track_ids[1][7]
    with pytest.raises(ValueError, match="duplicate"):
        stage.LMBALoop(v)


def test_rejections_on_cost_and_on_a_pivot():
    s, a, b = LR.reference("pivot", LR.PIVOT_ITERS, **LR.PIVOT_KW)
    loop = LR.build_loop(s, DEV, max_iter=LR.PIVOT_ITERS, **LR.PIVOT_KW)
    logs = loop.run()
    print("[ba_lm pivot] accepted", logs["accepted"].tolist(), "lambda", logs["lambda"].tolist())
    LR.check_against_routes("pivot", logs, loop, a, b)                      # flags and lambdas exactly, the rest within the bar
    assert np.array_equal(loop.poses.cpu().numpy()[-1], np.eye(3, 4))


@pytest.mark.parametrize("kind", ["points only", "poses only"])
def test_points_only_and_poses_only(kind):
    s, kw, a, b = LR.variant_reference(kind)
    loop = LR.build_loop(s, DEV, max_iter=3, **kw)
    LR.check_against_routes(kind, loop.run(), loop, a, b)
    if kind == "points only":
        assert np.array_equal(loop.poses.cpu().numpy(), s["poses"]) and not np.array_equal(loop.xyzs_all.cpu().numpy(), s["X"])
    else:
        assert np.array_equal(loop.xyzs_all.cpu().numpy(), s["X"]) and not np.array_equal(loop.poses.cpu().numpy(), s["poses"])


@pytest.mark.parametrize("loss", ["soft_l1", "cauchy"])
def test_robust_losses(loss):
    s, a, b = LR.reference("small", LOOP_ITERS, loss=loss, c=1.5, **LR.LOOP_KW)
    loop = LR.build_loop(s, DEV, max_iter=LOOP_ITERS, loss=loss, loss_scale=1.5, **LR.LOOP_KW)
    LR.check_against_routes(f"small/{loss}", loop.run(), loop, a, b)


def test_runs_repeat_and_split_calls_equal_one():
    s = LR.scene_edges()
    one, two, split = (LR.build_loop(s, DEV, max_iter=7, **LR.LOOP_KW) for _ in range(3))
    l1, l2 = one.run(), two.run()
    assert same_bits(bits(one, l1), bits(two, l2))
    la, lb = split.run(3), split.run(4)
    joined = {k: torch.cat([la[k], lb[k]]) for k in la}
    assert same_bits(bits(one, l1), bits(split, joined)) and split.it == 7


def test_permuted_observations_change_rounding_only():
    s, a, b = LR.reference("small", LOOP_ITERS, **LR.LOOP_KW)
    rng = np.random.default_rng(9)
    p = dict(s)
    perm = np.concatenate([s["view_start"][v] + rng.permutation(s["view_start"][v + 1] - s["view_start"][v]) for v in range(5)])
    p["op"], p["uv"] = s["op"][perm], s["uv"][perm]
    loop = LR.build_loop(p, DEV, max_iter=LOOP_ITERS, **LR.LOOP_KW)
    LR.check_against_routes("small, permuted", loop.run(), loop, a, b)


def test_run_is_capturable_and_a_replay_continues_the_loop():
    s = LR.scene_small()
    eager, graphed = (LR.build_loop(s, DEV, max_iter=6, **LR.LOOP_KW) for _ in range(2))
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


def test_unprepared_workspace_moves_nothing():
    s = LR.scene_small()
    loop = LR.build_loop(s, DEV, max_iter=3)
    before = bits(loop)
    loop._ws.zero_()
    logs = loop.run(2)
    assert all(bool(torch.isnan(v).all()) for v in logs.values())
    assert same_bits(before, bits(loop))


# ------------------------------------------------------------------------------------------------------------- the mapper
@pytest.fixture(scope="module")
def lm_ring():
    import mapper_scenes as MS
    import test_hip_mapper as TM
    import tracks_scenes as S
    from ls2fm import mapper as M
    sc = MS.ring_scene()
    run = lambda: M.reconstruct(sc["tables"], S.K, MS.H, MS.W, TM.options(M, ba_solver="lm"))
    rec = run()
    torch.cuda.synchronize()
    return sc, rec, run, M, TM


def test_mapper_with_lm_reconstructs_the_ring(lm_ring):
    sc, rec, run, M, TM = lm_ring
    import mapper_scenes as MS
    assert rec.registered.all() and sorted(rec.order) == list(range(MS.RING_VIEWS))
    keep = (rec.obs_keep & rec.track_valid[torch.bucketize(torch.arange(rec.obs_keep.numel(), device=DEV),
                                                           rec.tracks["track_start"].long()[1:], right=True)]).cpu().numpy()
    got = TM._accuracy(rec.poses.cpu().numpy(), sc["poses"], rec.X.cpu().numpy(), rec.tracks, rec.obs_uv.cpu().numpy(), keep)
    ctl = TM._control(M, sc)
    for name, g, c in zip(("rotation [rad]", "centre [units]", "reprojection [px]"), got, ctl):
        print(f"[mapper lm] ring accuracy: {name}: reconstruction {g:.4e}, control {c:.4e}, ratio {g / c:.3f} (bound 4)")
    for name, g, c in zip(("rotation", "centre", "reprojection"), got, ctl):
        assert g <= 4.0 * c, f"{name}: {g:.4e} against the control's {c:.4e}"
    again = run()
    assert again.order == rec.order
    assert torch.equal(again.poses, rec.poses) and torch.equal(again.X, rec.X) and torch.equal(again.obs_keep, rec.obs_keep)


def test_mapper_step_with_lm_makes_three_host_reads(lm_ring):
    sc, rec, run, M, TM = lm_ring
    import mapper_scenes as MS
    import tracks_scenes as S
    m = M._Mapper(sc["tables"], S.K, MS.H, MS.W, TM.options(M, ba_solver="lm"), DEV)
    with torch.cuda.device(m.dev):
        m.initialise()
        m.update()
        m.triangulate_new()
        m.adjust(None, True)
        m.update()
        torch.cuda.synchronize()
        with TM._ReadCounter() as reads:
            assert m.step(1)
    print(f"[mapper lm] one step: {reads.count} host reads {reads.where}")
    assert len(m.order) == 3 and reads.count == 3, reads.where
