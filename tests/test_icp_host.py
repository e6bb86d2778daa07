"""CPU: the ICP scenes (tests/icp_scenes.py) hold the conditions their kernels' failures need, the restatement (tests/icp_restate.py)
agrees with itself by its two solve routes and recovers the known transforms, ls2fm.metrics.icp(brute_force=True) -- the same rule as
torch ops -- follows it, and the refusals are raised."""
import inspect

import numpy as np
import pytest
import torch

import icp_restate as IR
import icp_scenes as S
import metrics_restate as MR
from ls2fm import metrics as MT


def test_scene_sizes_and_the_moves_of_the_registration_scenes():
    sc = S.scenes()
    assert set(sc) == set(S.NAMES)
    for name, c in sc.items():
        assert c["src"].dtype == np.float32 and c["dst"].dtype == np.float32 and len(c["dst"]) <= 4097
        assert len(c["src"]) <= 4096 or name == f"ragged_{S.LAUNCH_LANES + 1}"
        assert (c["normals"] is None) or c["normals"].shape == c["dst"].shape
    for name, scale in (("rigid", 1.0), ("similarity", 1.07), ("plane", 1.0)):
        c = sc[name]
        s, R, t = c["truth"]
        angle = np.degrees(np.arccos((np.trace(R) - 1) / 2))
        assert s == scale and abs(angle - 5.0) < 1e-9 and abs(np.linalg.norm(t) - 0.05 * c["extent"]) < 1e-9
        assert c["with_scale"] == (scale != 1.0) and (c["normals"] is not None) == (name == "plane")
        # the source is a subset of dst taken off by the inverse: the truth maps it back to fp32 accuracy
        assert np.abs(IR.apply(c["truth"], c["src"]) - c["dst"][c["pick"]]).max() < 1e-6
        # and the start is far enough that the first pairs are mostly wrong
        idx, _ = IR.pairs(c["src"], c["dst"], None)
        assert (idx != c["pick"]).mean() > 0.5
    n = sc["plane"]["normals"]
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    on_sphere = np.abs(np.linalg.norm(sc["plane"]["dst"], axis=1) - 1) < 1e-6
    assert on_sphere.sum() >= 2048 and np.abs(n[on_sphere] - sc["plane"]["dst"][on_sphere]).max() < 1e-6


def test_sliding_is_singular_exactly():
    c = S.scenes()["sliding"]
    acc = IR.accumulate(c["src"], c["dst"], c["normals"], c["init"], c["max_dist"])
    H, _ = IR.system(acc["sums"], False)
    assert acc["n_pairs"] == len(c["src"]) and not H[2].any() and not H[3].any() and not H[4].any() and H[5, 5] == acc["n_pairs"]
    assert IR.solve_chol(acc["sums"], False) is None and IR.solve_numpy(acc["sums"], False) is None
    # not only at the identity: the three columns are zero whatever p' is
    T = (1.0, S.rotation([1.0, 2.0, 3.0], 0.01), np.array([0.001, -0.002, 0.003]))
    assert IR.solve_chol(IR.accumulate(c["src"], c["dst"], c["normals"], T, None)["sums"], False) is None
    run = S.restated("sliding")
    assert run["status"] == IR.DEGENERATE and run["iterations"] == 0 and run["T"] is c["init"]


def test_partial_holds_its_three_cases():
    c = S.scenes()["partial"]
    _, pf = IR.transform(c["src"], c["init"])
    finite = np.isfinite(c["src"]).all(axis=1)
    assert np.array_equal(pf[finite].view(np.uint32), c["src"][finite].view(np.uint32))       # the identity start: p' = p exactly
    assert not np.isfinite(pf[~finite]).all(axis=1).any()                         # (0 x inf = NaN: such a row stays without a pair)
    idx, d2 = IR.pairs(pf, c["dst"], c["max_dist"])
    free, _ = IR.pairs(pf, c["dst"], None)
    lim = MR.max_d2_of(c["max_dist"])
    assert len(c["far_rows"]) * 2 >= len(c["src"]) - 2 and (idx[c["far_rows"]] == -1).all()
    _, far_d2 = MR.nearest(c["src"][np.setdiff1d(c["far_rows"], c["bad_rows"])], c["dst"], None)
    assert (far_d2 > 100 * lim).all()                                           # far outside the cut-off of anything
    assert not np.isfinite(c["src"][c["bad_rows"]]).all(axis=1).any() and (idx[c["bad_rows"]] == -1).all() and (free[c["bad_rows"]] == -1).all()
    assert np.isinf(d2[c["bad_rows"]]).all() and len(c["bad_rows"]) == 4
    tie = c["tie_row"]
    assert d2[tie] == lim and idx[tie] == len(c["dst"]) - 1                       # d2 == max_d2 exactly: it qualifies
    near = np.setdiff1d(np.arange(0, len(c["src"]) - 1, 2), c["bad_rows"])
    assert (idx[near] >= 0).all()                                               # and the half that stayed is all paired
    run = S.restated("partial")
    assert run["status"] == IR.CONVERGED and run["steps"][0]["n_pairs"] == len(near) + 1


def test_no_pairs_and_ragged():
    c = S.scenes()["no_pairs"]
    _, d2 = IR.pairs(c["src"], c["dst"], None)
    assert d2.min() > MR.max_d2_of(c["max_dist"])
    run = S.restated("no_pairs")
    assert run["status"] == IR.DEGENERATE and run["steps"][0]["n_pairs"] == 0 and not run["steps"][0]["sums"].any()
    assert S.RAGGED_SIZES[:4] == (1, 63, 65, 257) and S.RAGGED_SIZES[4] > S.LAUNCH_LANES
    for n in S.RAGGED_SIZES[:4]:
        assert len(S.scenes()[f"ragged_{n}"]["src"]) == n
    assert S.restated("ragged_1")["status"] == IR.DEGENERATE                     # one pair, six unknowns
    big, rigid = S.scenes()[f"ragged_{S.RAGGED_SIZES[4]}"]["src"], S.scenes()["rigid"]["src"]
    assert np.array_equal(big[:len(rigid)], rigid) and np.array_equal(big[-1], rigid[(len(big) - 1) % len(rigid)])


@pytest.mark.parametrize("name", S.WHOLE_RUNS)
def test_restatement_routes_agree_and_recover_the_transform(name):
    c = S.scenes()[name]
    a, b = S.restated(name), S.restated(name, "numpy")
    assert a["status"] == b["status"] == IR.CONVERGED and a["iterations"] == b["iterations"] <= 20
    assert np.abs(IR.flat(a["T"]) - IR.flat(b["T"])).max() < 1e-14
    for st in a["steps"]:
        assert np.abs(st["delta"]["chol"] - st["delta"]["numpy"]).max() <= 1e-13 * np.abs(st["delta"]["chol"]).max()
        assert st["n_pairs"] == len(c["src"]) and st["kappa"] < 100
    assert np.abs(IR.flat(a["T"]) - IR.flat(c["truth"])).max() < 1e-6
    # terms against a plain einsum of the Jacobians
    st = a["steps"][0]
    has = st["pair_idx"] >= 0
    _, pf = IR.transform(c["src"], c["init"])
    J, r = IR.jacobians(pf[has], c["dst"][st["pair_idx"][has]], None if c["normals"] is None else c["normals"][st["pair_idx"][has]])
    H, g = np.einsum("nra,nrb->ab", J, J), np.einsum("nra,nr->a", J, r)
    Hs, gs = IR.system(st["sums"], True)
    assert np.abs(H - Hs).max() <= 1e-12 * np.abs(H).max() and np.abs(g - gs).max() <= 1e-12 * np.abs(H).max()
    assert abs(st["sums"][35] - (r * r).sum()) <= 1e-12 * st["sums"][35] and (st["abs_sums"] >= np.abs(st["plain_sums"])).all()
    # the stated order of summation is one of the orders the any-order bound covers
    assert (np.abs(st["sums"] - st["plain_sums"]) <= (st["n_pairs"] + 16) * 2.0 ** -53 * st["abs_sums"]).all()


def test_ordered_sum_is_the_stated_order():
    """three sizes by hand: inside one wave the butterfly, across waves and workgroups the index order, past one launch the lane's
    own points first"""
    rng = np.random.default_rng(41)
    for n in (70, 600, IR.LANES * IR.MAX_GROUPS + 3):
        tm = rng.normal(size=(n, 2)) * 10.0 ** rng.integers(-8, 8, (n, 2))
        has = np.ones(n, bool)
        has[::7] = False
        groups = max(1, min(-(-n // 512), 512))
        lanes = groups * 512
        full = np.zeros((2 * lanes, 2))
        full[:n][has] = tm[has]
        lane = full[:lanes] + full[lanes:]                                     # a lane's first point, then its second
        want = np.zeros(2)
        for g in range(groups):
            row = None
            for w in range(8):
                v = lane[g * 512 + w * 64:g * 512 + (w + 1) * 64].copy()
                for o in (32, 16, 8, 4, 2, 1):
                    v = v + v[np.arange(64) ^ o]                              # lane i receives lane i ^ o
                row = v[0] if row is None else row + v[0]
            want = want + row
        assert np.array_equal(IR.ordered_sum(tm[has], has), want)


@pytest.mark.parametrize("name", ["rigid", "similarity", "plane", "sliding", "partial", "no_pairs", "ragged_1", "ragged_65"])
def test_brute_force_route_follows_the_restatement(name):
    c = S.scenes()[name]
    a = S.restated(name)
    res = MT.icp(torch.as_tensor(c["src"]), torch.as_tensor(c["dst"]), dst_normals=None if c["normals"] is None else torch.as_tensor(c["normals"]),
                 max_dist=c["max_dist"], with_scale=c["with_scale"], iters=c["iters"], tol_rot=c["tol_rot"], tol_trans=c["tol_trans"],
                 brute_force=True, return_pairs=True)
    assert res.status == a["status"] and res.iterations == a["iterations"]
    got = np.concatenate([[float(res.s)], res.R.numpy().reshape(-1), res.t.numpy()])
    assert np.abs(got - IR.flat(a["T"])).max() < 1e-12
    end = IR.accumulate(c["src"], c["dst"], c["normals"], a["T"], c["max_dist"])
    assert res.n_pairs == end["n_pairs"] and np.array_equal(res.pair_idx.numpy(), end["pair_idx"])
    if end["n_pairs"]:
        assert abs(res.rmse - np.sqrt(end["sums"][35] / end["n_pairs"])) < 1e-9 * max(res.rmse, 1e-12) + 1e-15
    else:
        assert np.isnan(res.rmse)
    if c["truth"] is not None:
        assert np.abs(got - IR.flat(c["truth"])).max() < 1e-6
        assert np.abs(res.apply(torch.as_tensor(c["src"])).numpy() - c["dst"][c["pick"]]).max() < 1e-6


def test_continuation_and_init_on_the_brute_force_route():
    c = S.scenes()["similarity"]
    src, dst = torch.as_tensor(c["src"]), torch.as_tensor(c["dst"])
    kw = dict(with_scale=True, tol_rot=c["tol_rot"], tol_trans=c["tol_trans"], brute_force=True)
    whole = MT.icp(src, dst, iters=5, **kw)
    first = MT.icp(src, dst, iters=2, **kw)
    second = MT.icp(src, dst, iters=3, state=first.state, **kw)
    assert second.iterations == 5 and torch.equal(whole.state, second.state)
    s, R, t = c["truth"]
    at_truth = MT.icp(src, dst, init=(s, torch.as_tensor(R), torch.as_tensor(t)), iters=0, **kw)
    assert at_truth.iterations == 0 and at_truth.status == MT.ICP_RUNNING and at_truth.n_pairs == len(c["src"]) and at_truth.rmse < 1e-6
    done = MT.icp(src, dst, iters=50, **kw)
    again = MT.icp(src, dst, iters=5, state=done.state, **kw)
    assert done.status == MT.ICP_CONVERGED and torch.equal(again.state, done.state)


def test_refusals():
    c = S.scenes()["rigid"]
    src, dst = torch.as_tensor(c["src"]), torch.as_tensor(c["dst"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.icp(src, dst)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        MT.icp(src[:, :2], dst, brute_force=True)
    with pytest.raises(ValueError, match="iters"):
        MT.icp(src, dst, iters=-1, brute_force=True)
    with pytest.raises(ValueError, match="iters"):
        MT.icp(src, dst, iters=MT.ICP_MAX_ITERS + 1, brute_force=True)
    with pytest.raises(ValueError, match="max_dist"):
        MT.icp(src, dst, max_dist=-0.5, brute_force=True)
    with pytest.raises(ValueError, match="tol_rot"):
        MT.icp(src, dst, tol_rot=-1.0, brute_force=True)
    with pytest.raises(ValueError, match="tol_rot"):
        MT.icp(src, dst, tol_trans=float("nan"), brute_force=True)
    with pytest.raises(ValueError, match="dst_normals"):
        MT.icp(src, dst, dst_normals=dst[:7], brute_force=True)
    with pytest.raises(ValueError, match="init"):
        MT.icp(src, dst, init=(1.0, torch.eye(4), torch.zeros(3)), brute_force=True)
    with pytest.raises(ValueError, match="state"):
        MT.icp(src, dst, state=torch.zeros(13, dtype=torch.float64), brute_force=True)


def test_signatures_and_defaults():
    ev = inspect.signature(MT.evaluate_mesh).parameters
    assert ev["init"].default is None and ev["icp"].default is None
    assert list(ev)[:9] == ["verts", "faces", "gt_points", "max_dist", "density", "thresholds", "generator", "brute_force", "return_points"]
    ic = inspect.signature(MT.icp).parameters
    assert list(ic)[:11] == ["src", "dst", "init", "dst_normals", "max_dist", "with_scale", "iters", "tol_rot", "tol_trans", "return_pairs",
                             "brute_force"]
    assert ic["iters"].default == 50 and ic["with_scale"].default is False and ic["tol_rot"].default == 1e-9 == MT.ICP_TOL_ROT
    assert ic["tol_trans"].default is None and MT.ICP_TOL_TRANS_REL == 1e-9 and ic["init"].default is None
    assert "1e-9" in MT.icp.__doc__ and "diagonal" in MT.icp.__doc__
