"""tests/terms_restate.py -- the float64 checker of tests/test_hip_loss_terms_edges.py -- held (a) to the torch-op forms of the same
terms that the loops keep for CPU tensors, in float64, value and gradients to 1e-12, and (b) to the condition that keeps the GPU
bar honest: on EVERY case the GPU file runs, the same statement evaluated in float32 on the CPU sits within EPS / 4 of the float64
one, for every compared quantity in the measure it is compared in.  (b) is a condition on the input builders, not a measurement:
the GPU test must not be able to pass on inputs where fp32 itself needs most of the bar.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import terms_restate as TR

F64 = torch.float64
TIGHT = 1e-12


def _leaf(a):
    return torch.tensor(np.asarray(a), dtype=F64).requires_grad_(True)


def _same(ref, pairs):
    bad = []
    for key, got in pairs.items():
        got = np.zeros_like(ref[key]) if got is None else got.detach().double().numpy().reshape(ref[key].shape)
        d = TR.distance(TR.KIND[key], got, ref[key])
        print(f"[terms host] {key:9s} loop's torch form - restatement (fp64) {d:.2e}")
        if not d <= TIGHT:
            bad.append((key, d))
    assert not bad, bad


@pytest.mark.parametrize("name", ["n65-sdf-most", "n1025-sdf-most", "n65-nosdf-one", "n2-sdf-most"])
def test_tracing_restatement_is_the_loops_cpu_branch(name):
    from ls2fm.stage.loops import TracingConsistency
    inp, ref, _ = TR.case("tracing", name)
    d = _leaf(inp["d"][None])
    sl = None if inp["sdf_last"] is None else _leaf(inp["sdf_last"])
    const = lambda k, *shape: torch.tensor(inp[k], dtype=F64).reshape(*shape)
    n = inp["d"].shape[0]
    me = SimpleNamespace(center=const("center", 1, n, 3), ray=const("ray", 1, n, 3), target=const("target", n, 3), live=const("live", n),
                         use_sdfs=sl is not None, w_tracing=inp["g_tl"], w_surf=inp["g_sd"], static=False,
                         _early=SimpleNamespace(take_or_trace=lambda c, r, s: (d, sl)))
    ret = {}
    TracingConsistency.__call__(me, ret).backward()
    pairs = {"tl": ret["tracing_loss"], "d_d": d.grad}
    if sl is not None:
        pairs.update(ss=ret["sdf_surf"], d_sdf=sl.grad)
    _same(ref, pairs)


@pytest.mark.parametrize("counts,masked", [([255, 256, 257], False), ([1, 0, 513, 2], False), ([300, 64], True), ([0, 1, 0], False)])
def test_reprojection_restatement_is_baloop_reproj_torch(counts, masked):
    """(without an infinite row: there `torch.where` after the norm hands autograd 0 x inf / inf = NaN)"""
    from ls2fm.stage.loops import BALoop
    inp = TR.reproject_inputs(counts, 7, masked=masked)
    ref = TR.reproject_term(inp, F64)
    x, poses = _leaf(inp["x"]), _leaf(inp["poses"])
    sdf = torch.zeros(len(inp["x"]), 1, dtype=F64) if inp["sdf"] is None else torch.tensor(inp["sdf"], dtype=F64)[:, None]
    me = SimpleNamespace(obs_view=torch.tensor(inp["obs_view"]), views=SimpleNamespace(intrinsic=torch.tensor(TR.K, dtype=F64)),
                         sdf_threshold=inp["bound"] / 2, obs_uv=torch.tensor(inp["obs_uv"], dtype=F64))
    reproj = BALoop._reproj_torch(me, x, poses, sdf)
    (inp["g"] * reproj).backward()
    if masked:
        on = ref["counted"]
        assert not on[1] and on[2] and 0 < on.sum() < on.size
    _same(ref, {"reproj": reproj, "d_x": x.grad, "d_poses": poses.grad})


@pytest.mark.parametrize("name", ["n65-below-add", "n65-at-noadd", "n1025-above-noadd", "n1025-at-add", "n1-above-add"])
def test_ba_terms_restatement_is_baloop_extra(name):
    from ls2fm.stage.loops import BALoop
    inp, ref, _ = TR.case("ba", name)
    r, s = _leaf(inp["reproj"]), _leaf(inp["sdfs"][:, None])
    a = None if inp["add"] is None else _leaf(inp["add"])
    me = SimpleNamespace(_point_side=(torch.zeros(1, 3, dtype=F64), s), rot=torch.zeros(1, 3, dtype=F64), trans=torch.zeros(1, 3, dtype=F64),
                         _reproj_torch=lambda *_: r, _w_hi=None, _w_lo=None, w_reproj_lo=1.0, w_surf=inp["w_surf"],
                         tracing=lambda ret: 0.0 if a is None else inp["w_add"] * a)
    ret = {}
    extra = BALoop._extra(me, ret)
    (inp["g"] * extra).backward()
    pairs = {"surf": ret["sdf_surf"], "w": ret["w_reproj"], "extra": extra, "d_reproj": r.grad, "d_sdfs": s.grad}
    if a is not None:
        pairs["d_add"] = a.grad
    _same(ref, pairs)


@pytest.mark.parametrize("name", ["S2-n65", "S4-n65", "S2-n1025"])
def test_match_restatement_is_the_torch_lines_of_the_two_view_initialisation(name):
    """the lines of InitLoop._extra as test_fused_match_term_matches_the_torch_lines writes them, for S segments"""
    from ls2fm.utils import camera as cam
    inp, ref, _ = TR.case("match", name)
    S, n = inp["d"].shape
    d, sl = [_leaf(inp["d"][v][None]) for v in range(S)], [_leaf(inp["sdf_last"][v]) for v in range(S)]
    const = lambda k, *shape: torch.tensor(inp[k], dtype=F64).reshape(*shape)
    cen, ray, kps, poses = const("center", S, 1, n, 3), const("ray", S, 1, n, 3), const("uv_obs", S, n, 2), const("poses", S, 3, 4)
    intr = torch.tensor(TR.K, dtype=F64)
    errs, sdfs, pts_all = [], [], []
    for v in range(S):
        pts = cen[v] + ray[v] * d[v].reshape(1, -1, 1)
        uv = cam.cam2img(cam.world2cam(pts, poses[v:v + 1]), intr.unsqueeze(0))
        uv = (uv / (uv[..., 2:] + 1e-6))[..., :2]
        errs.append((uv[0] - kps[v]).norm(dim=-1)); sdfs.append(sl[v].reshape(-1)); pts_all.append(pts[0].detach())
    re, ss = torch.cat(errs).mean(), torch.cat(sdfs).abs().mean()
    (inp["g0"] * re + inp["g1"] * ss).backward()
    _same(ref, {"re": re, "ss": ss, "surface": torch.cat(pts_all), "d_d": torch.stack([t.grad[0] for t in d]),
                "d_sdf": torch.stack([t.grad for t in sl])})


@pytest.mark.parametrize("name", ["n257-both", "n255-out", "n256-len", "n1-both"])
def test_surface_restatement_is_the_oracles_last_line(name, monkeypatch):
    """oracle.fields.get_surface_pts with its two field queries replaced by given leaves: what is left is its last line"""
    from oracle import fields as OF
    inp, ref, _ = TR.case("surface", name)
    nr, sd = _leaf(inp["normals"]), _leaf(inp["sdf"][:, None])
    monkeypatch.setattr(OF, "infer_sdf", lambda *a, **k: sd)
    monkeypatch.setattr(OF, "sdf_gradient", lambda *a, **k: nr)
    out, length = OF.get_surface_pts(torch.tensor(inp["p"], dtype=F64), None, None, None)
    loss = 0.0
    if inp["g_out"] is not None:
        loss = loss + (out * torch.tensor(inp["g_out"], dtype=F64)).sum()
    if inp["g_len"] is not None:
        loss = loss + (length[:, 0] * torch.tensor(inp["g_len"], dtype=F64)).sum()
    loss.backward()
    _same(ref, {"out": out, "length": length, "d_n": nr.grad, "d_sdf": sd.grad})


ALL_CASES = [(family, name) for family, (cases, _, _) in TR.FAMILIES.items() for name in cases]


@pytest.mark.parametrize("family,name", ALL_CASES, ids=[f"{f}-{n}" for f, n in ALL_CASES])
def test_float32_on_the_cpu_needs_at_most_a_quarter_of_the_bar(family, name):
    _, r64, r32 = TR.case(family, name)
    bad = []
    for key in r64:
        if key == "counted":
            assert np.array_equal(r64[key], r32[key])
            continue
        c = TR.distance(TR.KIND[key], r32[key], r64[key])
        print(f"[terms cap] {family:9s} {name:18s} {key:9s} cpu-fp32-fp64 {c:.3e}  cap {TR.EPS / 4:.1e}")
        if not c <= TR.EPS / 4:
            bad.append((key, c))
    assert not bad, bad


def test_the_special_rows_are_what_the_cases_say():
    inp, r64, _ = TR.case("tracing", "n65-sdf-most")
    assert r64["d_d"][5] == 0.0 and r64["d_sdf"][7] == 0.0 and inp["live"][5] == inp["live"][7] == 1.0 and inp["live"][-1] == 0.0
    assert (r64["d_d"][inp["live"] == 0] == 0).all() and 0.6 * 65 < inp["live"].sum() < 65
    assert TR.case("tracing", "n2049-sdf-one")[0]["live"].sum() == 1.0
    dead = TR.case("tracing", "n65-all_dead")[1]
    # (row 5 too: torch's norm backward at e = 0 is upstream x 0, and the upstream is NaN)
    assert np.isnan(dead["tl"]) and np.isnan(dead["ss"]) and np.isnan(dead["d_d"]).all() and np.isnan(dead["d_sdf"]).all()
    only_tl = TR.case("tracing", "n1025-only_tl")[1]
    assert (only_tl["d_sdf"] == 0).all() and (TR.case("tracing", "n1025-only_sd")[1]["d_d"] == 0).all() and only_tl["d_d"].any()
    for name in ("1-0-513-2", "300-64-masked"):
        inp, r64, _ = TR.case("reproject", name)
        row = inp["inf_row"]
        assert not r64["counted"][row] and (r64["d_x"][row] == 0).all() and r64["counted"][row - 1]
        assert np.isfinite(r64["d_poses"]).all() and np.isfinite(r64["reproj"])
    inp, r64, _ = TR.case("reproject", "300-64-masked")
    assert abs(inp["sdf"][1]) == np.float32(inp["bound"]) and not r64["counted"][1] and r64["counted"][2]
    empty = TR.case("reproject", "0-0")[1]
    assert empty["reproj"] == 0.0 and empty["d_x"].shape == (0, 3) and (empty["d_poses"] == 0).all()
    assert (TR.case("reproject", "1-0-513-2")[1]["d_poses"][1] == 0).all()
    assert TR.case("ba", "n65-at-noadd")[1]["w"] == 1.0 and TR.case("ba", "n65-below-add")[1]["w"] == 1.0
    assert TR.case("ba", "n1025-above-noadd")[1]["w"] == 10.0 and TR.case("ba", "n65-at-noadd")[1]["d_sdfs"][11] == 0.0


def test_distance_demands_exact_zeros_and_nans():
    one = np.array([1.0, 0.0, np.nan])
    assert TR.distance("elem", one, one) == 0.0
    assert TR.distance("elem", [1.0, 1e-30, np.nan], one) == float("inf")            # a zero not met
    assert TR.distance("elem", [1.0, 0.0, 0.0], one) == float("inf")                 # a NaN not met
    assert TR.distance("elem", [np.nan, 0.0, np.nan], one) == float("inf")           # a NaN invented
    rows = np.array([[1.0, 1e-3, 0.0], [0.0, 0.0, 0.0]])
    assert abs(TR.distance("row", rows + [[0.0, 1e-6, 1e-6], [0.0, 0.0, 0.0]], rows) - 1e-6) < 1e-12    # relative to the row's largest
    assert TR.distance("row", rows + [[0.0, 0.0, 0.0], [0.0, 1e-30, 0.0]], rows) == float("inf")
    assert TR.distance("view", np.zeros((2, 3, 4)), np.zeros((2, 3, 4))) == 0.0 and TR.distance("row", np.zeros((0, 3)), np.zeros((0, 3))) == 0.0
