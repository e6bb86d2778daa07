"""The fused loss-term kernels of the stage loops (csrc/reproject.hip through the autograd nodes of ls2fm.stage.terms, surface_pts
through the C ABI; csrc/loss_head.hip through the two-call loss head) at the shapes where a reduction kernel goes wrong -- fewer
rows than a wave, the grid-stride boundary of the 1024-thread workgroups and its second trip, one live row, no live row, empty
views, 1 .. 4 segments, an infinite projection, |sdf| exactly at the bound, absent upstreams, the loss head's cap at 512 workgroups
-- against tests/terms_restate.py evaluated in FLOAT64 (tests/test_terms_restate_host.py pins it to the loops' torch forms).

One relative bar, terms_restate.EPS = 2e-5, per element / per row / per view / on the value (terms_restate.distance), exact zeros
and NaNs where the reference has them.  The same statements in float32 on the CPU stay under EPS / 4 = 5e-6 on every case here
(held by the host test), so the bar cannot be met by inputs on which fp32 itself is lost.

Worst distance from float64 per kernel family and quantity over all cases below, on an MI355X -- device, then float32 on the CPU
over the same cases (how much of the bar is used; the CPU statement keeps its scalar terms in fp64, the device rounds them to
fp32: 0 against ~5e-8):
    tracing    tl 9.9e-08 / 9.9e-08   ss 3.7e-08 / 0         d_d 3.6e-07 / 3.6e-07    d_sdf 5.8e-08 / 5.8e-08
    ba         surf 5.4e-08 / 0       extra 4.6e-08 / 0      d_sdfs 2.9e-08 / 2.9e-08   w, d_reproj, d_add 0 / 0
    match      re 4.9e-08 / 5.0e-08   ss 4.5e-08 / 0         surface 5.8e-08 / 1.2e-07   d_d 4.1e-06 / 2.5e-06   d_sdf 3.1e-08 / 3.1e-08
    reproject  reproj 4.6e-07 / 1.1e-06   d_x 2.7e-06 / 2.4e-06   d_poses 1.5e-06 / 1.6e-06
    surface    out 7.4e-08 / 5.9e-08   length 8.7e-08 / 8.3e-08   d_n 3.4e-07 / 3.4e-07   d_sdf 1.9e-07 / 1.9e-07
The largest, match d_d at S = 2, n = 1024, is a fifth of the bar.  A row left out of a sum over 2049 moves a mean by ~5e-4, a
skipped second trip of match_term_fwd's grid-stride loop at n = 1025 by ~1e-3 (and leaves NaN rows in `surface`): 25 - 50 bars.
The loss-head cases reuse test_hip_loss_head._run and its bars (TOL = 2e-6 on the terms, 1e-5 on the gradients) unchanged."""
import numpy as np
import pytest
import torch

import terms_restate as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 3          # rows of NaN behind every surface_pts output: nothing is written past n


def _dev(a, grad=False):
    return torch.tensor(np.asarray(a), device=DEV).requires_grad_(grad)


def _host(t):
    return t.detach().double().cpu().numpy()


def _grad_of(leaf):
    return np.zeros(tuple(leaf.shape)) if leaf.grad is None else _host(leaf.grad)


# ------------------------------------------------------------------------------------------------------ one device run per family
def run_tracing(inp):
    from ls2fm.stage.terms import _TracingTerm
    n = inp["d"].shape[0]
    d = _dev(inp["d"][None], True)
    sl = None if inp["sdf_last"] is None else _dev(inp["sdf_last"], True)
    tl, ss = _TracingTerm.apply(_dev(inp["center"][None]), _dev(inp["ray"][None]), d, _dev(inp["target"]), _dev(inp["live"]), sl)
    loss = ([] if inp["g_tl"] is None else [inp["g_tl"] * tl]) + ([] if sl is None or inp["g_sd"] is None else [inp["g_sd"] * ss])
    sum(loss).backward()
    out = {"tl": _host(tl), "d_d": _grad_of(d).reshape(n)}
    if sl is not None:
        out.update(ss=_host(ss), d_sdf=_grad_of(sl))
    return out


def run_ba(inp):
    from ls2fm.stage.terms import _BATerms
    r, s = _dev(inp["reproj"], True), _dev(inp["sdfs"][:, None], True)
    a = None if inp["add"] is None else _dev(inp["add"], True)
    surf, w, extra = _BATerms.apply(r, s, a, inp["thresh"], inp["w_lo"], inp["w_hi"], inp["w_surf"], inp["w_add"])
    assert not surf.requires_grad and not w.requires_grad
    (inp["g"] * extra).backward()
    out = {"surf": _host(surf), "w": _host(w), "extra": _host(extra), "d_reproj": _grad_of(r), "d_sdfs": _grad_of(s)[:, 0]}
    assert s.grad.shape == s.shape
    if a is not None:
        out["d_add"] = _grad_of(a)
    return out


def _match_operands(inp):
    from ls2fm.stage.terms import host_intrinsic
    S, n = inp["d"].shape
    fixed = (_dev(inp["center"]), _dev(inp["ray"]), _dev(inp["uv_obs"]), _dev(inp["poses"]), host_intrinsic(torch.tensor(TR.K)), n)
    surface = torch.full((S * n, 3), float("nan"), device=DEV)
    return fixed, surface, [_dev(inp["d"][v][None], True) for v in range(S)], [_dev(inp["sdf_last"][v], True) for v in range(S)]


def run_match(inp):
    from ls2fm.stage.terms import _MatchTerm
    fixed, surface, d, sl = _match_operands(inp)
    re, ss = _MatchTerm.apply(fixed, surface, *d, *sl)
    (inp["g0"] * re + inp["g1"] * ss).backward()
    return {"re": _host(re), "ss": _host(ss), "surface": _host(surface), "d_d": np.stack([_grad_of(t)[0] for t in d]),
            "d_sdf": np.stack([_grad_of(t) for t in sl])}


def run_reproject(inp):
    from ls2fm import stage
    x, poses = _dev(inp["x"].reshape(-1, 3), True), _dev(inp["poses"], True)
    sdf = None if inp["sdf"] is None else _dev(inp["sdf"])
    got, counted = stage.reprojection_term(x, poses, _dev(inp["view_start"]), stage.host_intrinsic(torch.tensor(TR.K)),
                                           _dev(inp["obs_uv"].reshape(-1, 2)), sdf, inp["bound"])
    (inp["g"] * got).backward()
    return {"reproj": _host(got), "counted": counted.cpu().numpy(), "d_x": _grad_of(x), "d_poses": _grad_of(poses)}


def run_surface(inp):
    """ls2fm_surface_pts_fwd / _bwd through the C ABI; every output has GUARD rows of NaN behind its n rows"""
    from ls2fm import _lib
    lib, P = _lib.load(), _lib.ptr
    n = inp["sdf"].shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    opt = lambda a: None if a is None else _dev(a)
    p, nr, sd = _dev(inp["p"].reshape(-1, 3)), _dev(inp["normals"].reshape(-1, 3)), _dev(inp["sdf"])
    go, gl = opt(inp["g_out"]), opt(inp["g_len"])
    out, length, d_n, d_s = nan(n + GUARD, 3), nan(n + GUARD), nan(n + GUARD, 3), nan(n + GUARD)
    assert lib.ls2fm_surface_pts_fwd(P(p), P(nr), P(sd), n, P(out), P(length), _lib.stream_ptr()) == 0
    assert lib.ls2fm_surface_pts_bwd(P(nr), P(sd), P(length), n, P(go), P(gl), P(d_n), P(d_s), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    for t in (out, length, d_n, d_s):
        assert bool(torch.isnan(t[n:]).all()), "written past n"
    return {"out": _host(out[:n]), "length": _host(length[:n]), "d_n": _host(d_n[:n]), "d_sdf": _host(d_s[:n])}


RUN = {"tracing": run_tracing, "ba": run_ba, "match": run_match, "reproject": run_reproject, "surface": run_surface}


def _hold(family, name):
    inp, r64, r32 = TR.case(family, name)
    got = RUN[family](inp)
    assert set(got) == set(r64)
    bad = [TR.check(family, name, key, got[key], r64[key], r32[key]) for key in r64 if key != "counted"]
    assert not any(bad), [b for b in bad if b]
    return inp, got, r64


# --------------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(TR.TRACING_CASES))
def test_tracing_term_against_float64(name):
    inp, got, r64 = _hold("tracing", name)
    n, live = inp["d"].shape[0], inp["live"]
    if name == "n65-all_dead":
        assert np.isnan(got["tl"]) and np.isnan(got["ss"]) and np.isnan(got["d_d"]).all() and np.isnan(got["d_sdf"]).all()
        return
    assert (got["d_d"][live == 0] == 0).all()                                                   # dead rows: exactly 0
    special_live = "-one" not in name                        # ("one": the single live row is another one)
    if n >= 63 and inp["g_tl"] is not None:
        assert live[5] == special_live and got["d_d"][5] == 0.0                                 # the key point on its target
    if n >= 63 and inp["sdf_last"] is not None and inp["g_sd"] is not None:
        assert live[7] == special_live and got["d_sdf"][7] == 0.0 and (got["d_sdf"][live == 0] == 0).all()   # sign(0) = 0
    if inp["g_tl"] is None:
        assert (got["d_d"] == 0).all() and got["d_sdf"].any()
    if inp["sdf_last"] is not None and inp["g_sd"] is None:
        assert (got["d_sdf"] == 0).all() and got["d_d"].any()


@pytest.mark.parametrize("name", list(TR.BA_CASES))
def test_ba_terms_against_float64(name):
    inp, got, _ = _hold("ba", name)
    assert got["w"] == (10.0 if float(inp["reproj"]) > 10.0 else 1.0)                          # AT the threshold: the low weight
    assert got["d_reproj"] == inp["g"] * got["w"]
    if inp["sdfs"].shape[0] > 1:
        assert got["d_sdfs"][min(11, inp["sdfs"].shape[0] - 1)] == 0.0                            # sign(0) = 0


@pytest.mark.parametrize("name", list(TR.MATCH_CASES))
def test_match_term_against_float64(name):
    inp, got, _ = _hold("match", name)
    S, n = inp["d"].shape
    assert got["d_sdf"][S - 1, n // 2] == 0.0 and np.isfinite(got["surface"]).all()


def test_match_term_refuses_five_segments_and_launches_nothing():
    from ls2fm.stage.terms import _MatchTerm
    fixed, surface, d, sl = _match_operands(TR.match_inputs(5, 65, 35))
    with pytest.raises(RuntimeError, match="ls2fm_match_term_fwd"):
        _MatchTerm.apply(fixed, surface, *d, *sl)
    torch.cuda.synchronize()
    assert bool(torch.isnan(surface).all())


@pytest.mark.parametrize("name", list(TR.REPROJECT_CASES))
def test_reprojection_term_against_float64(name):
    inp, got, r64 = _hold("reproject", name)
    assert np.array_equal(got["counted"], r64["counted"])                                       # the fp32 decision, exactly
    off = ~r64["counted"]
    assert (got["d_x"][off] == 0).all()
    start = inp["view_start"]
    for v in range(len(start) - 1):
        if not r64["counted"][start[v]:start[v + 1]].any():
            assert (got["d_poses"][v] == 0).all()                                               # an empty view: exactly 0
    if inp["inf_row"] is not None:
        row = inp["inf_row"]
        assert off[row] and (got["d_x"][row] == 0).all() and np.isfinite(got["d_poses"]).all() and np.isfinite(got["reproj"])
    if inp["sdf"] is not None:
        assert abs(inp["sdf"][1]) == np.float32(inp["bound"]) and off[1] and not off[2]           # AT the bound: not counted
    if name == "0-0":
        assert got["reproj"] == 0.0 and got["d_x"].shape == (0, 3) and (got["d_poses"] == 0).all()


@pytest.mark.parametrize("name", list(TR.SURFACE_CASES))
def test_surface_pts_against_float64(name):
    _hold("surface", name)                    # (n = 0: status OK, and the NaN-filled outputs stay NaN -- run_surface's guard rows)


# -------------------------------------------------------------------------------------------------- the loss head, two-call form
def _far_from_one(LH, monkeypatch):
    """test_hip_loss_head._inputs with the LAST ray's normals 40 x longer: its 256 points then carry ~2 % of the eikonal mean, and
    they are exactly the points a workgroup reaches on its ninth trip when the grid is capped -- a forward that skipped the trip
    would miss the mean by ~2e-2 against TOL = 2e-6"""
    plain = LH._inputs

    def inputs(*a, **k):
        ret, gt, d_points = plain(*a, **k)
        ret["normals"][0, -1] *= 40.0
        return ret, gt, d_points
    monkeypatch.setattr(LH, "_inputs", inputs)


@pytest.mark.parametrize("n_rays", [4096, 4097])
def test_loss_head_at_and_above_the_workgroup_cap(n_rays, monkeypatch):
    """(4096, 256): 512 workgroups of 2048 points exactly, uncapped; (4097, 256): 513 wanted, capped to 512 -- the forward becomes a
    true grid-stride loop and workgroup 0 takes a ninth point per thread"""
    import test_hip_loss_head as LH
    _far_from_one(LH, monkeypatch)
    LH._run(n_rays, 256, 21, dict(finish=None, eik=None, bg=None), (3.0, 2.0, 0.5))
    from ls2fm.losses import RenderLossHead
    assert float(RenderLossHead.sums(DEV)[3]) == n_rays * 256


@pytest.mark.parametrize("empty", ["eik", "bg"])
def test_loss_head_empty_eikonal_or_background_mask(empty):
    """0 / 0 = NaN, as torch's mean of nothing: the eikonal term (and the total) or the MSE; the other terms and every gradient finite"""
    import test_hip_loss_head as LH
    masks = dict(finish=None, eik=None, bg=None)
    masks[empty] = 0.0
    LH._run(64, 8, 22, masks, (3.0, 2.0, 1.0))


# ----------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("family,name", [("tracing", "n2049-sdf-most"), ("ba", "n2049-above-add"), ("match", "S2-n2049"),
                                         ("reproject", "1-0-513-2"), ("surface", "n257-both")])
def test_two_runs_leave_the_same_bits(family, name):
    """the kernels' headers promise fixed-order sums"""
    inp = TR.case(family, name)[0]
    a, b = RUN[family](inp), RUN[family](inp)
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def test_loss_head_above_the_cap_leaves_the_same_bits():
    import test_hip_loss_head as LH
    from ls2fm.losses import RenderLossHead
    ret, gt, d_points = LH._inputs(4097, 256, 23)
    rp = {k: v.to(DEV) for k, v in ret.items()}
    head = RenderLossHead(DEV)
    a = head.terms(rp, gt.to(DEV), d_points=d_points.to(DEV))[0].clone()
    sums = RenderLossHead.sums(DEV).clone()
    for _ in range(2):
        assert torch.equal(a, head.terms(rp, gt.to(DEV), d_points=d_points.to(DEV))[0])
        assert torch.equal(sums, RenderLossHead.sums(DEV))
    assert float(sums[3]) == 4097 * 256 and float(sums[1]) == 3 * 4097
