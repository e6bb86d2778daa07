"""CPU: THE PLANE SCORE and THE PATCHMATCH STEP of include/ls2fm.h judged by their properties on the numpy restatement
(tests/patchmatch_restate.py), so that the GPU tests (tests/test_hip_patchmatch.py) can be exact comparisons against that
restatement; the torch forms of ls2fm.mvs on CPU tensors against it bit for bit; normals_to_world; refusals; the header's
constants."""
import functools
import os
import re

import numpy as np
import pytest

import mvs_restate as MR
import mvs_scenes as S
import patchmatch_restate as PR
import patchmatch_scenes as PS

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERTURB = dict(depth_perturb=0.02, normal_perturb=0.5, max_slope=1.0)


def bits(a):
    return np.asarray(a, F32).view(np.int32)


def same_bits(got, ref):
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype
    return bool(((bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))).all())


def sweep_kw(sc):
    return dict(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])


def scene_of(sc, t=1):
    return PR.Scene(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc.get("refs"), tap_step=t, **sweep_kw(sc))


def d_range(sc):
    return sc["depths"].min(axis=1), sc["depths"].max(axis=1)


def test_the_header_s_constants_are_the_python_copies():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    value = lambda name: int(re.search(rf"#define\s+LS2FM_MVS_{name}\s+(0x[0-9A-Fa-f]+|\d+)u?\b", header).group(1), 0)
    from ls2fm import mvs
    assert (value("PM_TILE_H"), value("PM_TILE_W")) == (mvs.PM_TILE_H, mvs.PM_TILE_W) == (PS.TILE_H, PS.TILE_W)
    assert value("PM_DRAWS") == mvs.PM_DRAWS == PR.N_DRAWS
    for name in ("MIX_A", "MIX_B", "MIX_SALT"):
        assert value(name) == getattr(mvs, name) == getattr(PR, name), name
    assert list(mvs.NEIGHBOURS) == PR.NEIGHBOURS
    # the header names the neighbours in the rule's text, in this order
    listed = re.search(r"the eight neighbours m = p \+ ([^:]*?) \(dx, dy\)", header).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r"\((-?\d+),(-?\d+)\)", listed)] == PR.NEIGHBOURS
    assert all((abs(dx) + abs(dy)) % 2 == 1 for dx, dy in PR.NEIGHBOURS), "every neighbour has the other colour"


@pytest.mark.parametrize("H,W,w", [(15, 16, 1), (17, 33, 2)])
def test_a_fronto_parallel_plane_scores_as_the_sweep_does(H, W, w):
    """n = (0, 0, -1), t = 1: g = -1 and d_q = d exactly, so the plane score at d_k is the sweep's score_k by its bits, at every
    pixel, plane and reference"""
    sc = S.grid_scene(H, W, w)
    scores = MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], return_scores=True, **sweep_kw(sc))[3]
    ps = scene_of(sc)
    R, D = sc["depths"].shape
    normal = np.zeros((R, H, W, 3), F32)
    normal[..., 2] = -1
    assert np.isfinite(scores).any() and np.isnan(scores).any()
    for k in range(D):
        depth = np.broadcast_to(sc["depths"][:, k, None, None], (R, H, W)).astype(F32)
        assert same_bits(PR.plane_score(ps, depth, normal), scores[:, k]), k


@functools.lru_cache(maxsize=None)
def edge_run(H, W, w, t, iterations=2):
    """the hand-made edge state through `iterations` iterations: the states before and after every half-sweep, and the stats"""
    sc = S.grid_scene(H, W, w)
    ps = scene_of(sc, t)
    depth, normal = (a.copy() for a in PS.edge_state(sc))
    stats = {}
    score = PR.plane_score(ps, depth, normal, stats)
    states = [(depth.copy(), normal.copy(), score.copy())]
    lo, hi = d_range(sc)
    for it in range(iterations):
        for colour in (0, 1):
            PR.step(ps, depth, normal, score, colour, it, 7, d_min=lo, d_max=hi, stats=stats, **PERTURB)
            states.append((depth.copy(), normal.copy(), score.copy()))
    return sc, ps, states, stats


RUNS = [(15, 16, 1, 1), (17, 33, 2, 2)]


@pytest.mark.parametrize("H,W,w,t", RUNS)
def test_a_step_leaves_the_other_colour_and_never_lowers_a_score(H, W, w, t):
    sc, ps, states, _ = edge_run(H, W, w, t)
    yy, xx = np.mgrid[0:H, 0:W]
    moved = 0
    for i, (before, after) in enumerate(zip(states[:-1], states[1:])):
        other = ((xx + yy) & 1) != i % 2
        for b, a in zip(before, after):
            assert same_bits(a[:, other], b[:, other]), "a pixel of the other colour changed"
        sb, sa = before[2], after[2]
        assert not (np.isnan(sa) & ~np.isnan(sb)).any(), "a score became NaN"
        keep = ~np.isnan(sb)
        assert (sa[keep] >= sb[keep]).all(), "a score fell"
        changed = bits(sa) != bits(sb)
        changed &= ~(np.isnan(sa) & np.isnan(sb))
        assert (sa[changed & keep] > sb[changed & keep]).all()
        # what did not improve kept its hypothesis by its bits
        still = ~changed
        assert same_bits(after[0][still], before[0][still]) and same_bits(after[1][still], before[1][still])
        moved += int(changed.sum())
    assert moved > 100


@pytest.mark.parametrize("H,W,w,t", RUNS)
def test_the_stored_scores_are_the_plane_scores_of_the_state(H, W, w, t):
    sc, ps, states, _ = edge_run(H, W, w, t)
    for depth, normal, score in states[1:]:
        assert same_bits(PR.plane_score(ps, depth, normal), score)


EDGES = ["depth is NaN", "depth is zero", "depth is negative", "depth is +inf", "normal not finite", "g_p == 0", "normal faces away",
         "g_q changes sign in the window", "count == min_sources - 1", "neighbour outside the image", "neighbour without a depth",
         "a candidate ties the incumbent", "a neighbour's plane wins", "no hypothesis to perturb", "the perturbed depth wins",
         "the perturbed normal wins", "both perturbations win", "the fresh hypothesis wins"]


def test_the_edge_states_meet_every_edge_of_both_rules():
    """the states the GPU tests compare bit for bit: each edge the rules name occurs at some pixel"""
    for H, W, w, t in RUNS:
        sc, ps, states, stats = edge_run(H, W, w, t)
        for name in EDGES:
            assert stats.get(name, 0) > 0, (name, H, W, w, t)
    # the claims of edge_state did what they say, on the first state's scores
    sc, ps, states, _ = edge_run(15, 16, 1, 1)
    depth, normal, score = states[0]
    bad_depth = ~(np.isfinite(depth) & (depth > 0))
    assert np.isnan(score[bad_depth]).all()
    kind = lambda k: np.stack([((np.mgrid[0:15, 0:16][1] + 3 * np.mgrid[0:15, 0:16][0] + r) % PS.N_NORMALS) == k for r in range(3)])
    for k in (3, 5, 7):
        assert np.isnan(score[kind(k)]).all(), k
    assert np.isnan(score[kind(9)]).all(), "a window the plane's horizon crosses has an invalid tap"
    assert np.isfinite(score[kind(0) & ~bad_depth]).any()
    # a tie keeps the incumbent: a constant fronto-parallel state on the true plane moves only where a candidate is strictly better
    flat_d = np.where(np.arange(3)[:, None, None] == 2, F32(0.25), F32(1.0)) * np.ones((3, 15, 16), F32)
    flat_n = np.zeros((3, 15, 16, 3), F32)
    flat_n[..., 2] = -1
    stats = {}
    s0 = PR.plane_score(ps, flat_d, flat_n)
    d1, n1, s1 = flat_d.copy(), flat_n.copy(), s0.copy()
    PR.step(ps, d1, n1, s1, 0, 0, 1, d_min=d_range(sc)[0], d_max=d_range(sc)[1], stats=stats, **PERTURB)
    assert stats["a candidate ties the incumbent"] > 0
    kept = bits(s1) == bits(s0)
    assert same_bits(d1[kept], flat_d[kept]) and kept.any()


def test_the_edge_state_meets_every_edge_without_a_centre_tap():
    """w = 3, t = 2: the taps at -3, -1, 1, 3, the one pattern that leaves the window's centre out -- every edge both rules name
    still occurs on the state the GPU tests compare at that pattern, but for one that no w >= 3 can meet: "neighbour outside the
    image".  The step visits the pixels that have a window, at least w from every border, and its farthest neighbour is 3 away."""
    sc, ps, states, stats = edge_run(17, 33, 3, 2)
    assert (0, 0) not in ps.offsets and len(ps.offsets) == 16
    assert max(max(abs(dx), abs(dy)) for dx, dy in PR.NEIGHBOURS) == 3 and stats["neighbour outside the image"] == 0
    for name in EDGES:
        if name != "neighbour outside the image":
            assert stats.get(name, 0) > 0, name
    assert np.isfinite(states[0][2]).any() and np.isnan(states[0][2]).any()


def test_the_draws():
    pixel = np.arange(4096)
    u = np.stack([PR.draw(3, 2, 1, pixel, j) for j in range(PR.N_DRAWS)])
    assert u.dtype == F32 and (u >= 0).all() and (u < 1).all()
    assert (u * F32(2.0 ** 24) == np.floor(u * F32(2.0 ** 24))).all(), "multiples of 2^-24"
    assert abs(float(u.mean()) - 0.5) < 0.01 and len(np.unique(u)) > 0.99 * u.size
    assert not np.array_equal(u[0], PR.draw(4, 2, 1, pixel, 0)), "two seeds differ"
    assert not np.array_equal(u[0], PR.draw(3, 5, 1, pixel, 0)) and not np.array_equal(u[0], PR.draw(3, 2, 2, pixel, 0))
    # the largest arguments wrap as 32-bit integers
    big = PR.draw(0xFFFFFFFF, 5, 2 ** 31 - 1, np.array([32768 * 32768 - 1]), 8)
    assert 0 <= big[0] < 1
    # the step draws by the VIEW index refs[r], not by r: reference 1 alone leaves the bits it has among three
    sc = S.grid_scene(15, 16, 1)
    lo, hi = d_range(sc)
    whole = [a.copy() for a in edge_run(15, 16, 1, 1)[2][0]]
    PR.step(scene_of(sc), *whole, 0, 0, 7, d_min=lo, d_max=hi, **PERTURB)
    part_sc = PR.Scene(sc["images"], sc["poses"], sc["intr"], sc["sources"][1:2], sc["refs"][1:2], **sweep_kw(sc))
    part = [a[1:2].copy() for a in edge_run(15, 16, 1, 1)[2][0]]
    PR.step(part_sc, *part, 0, 0, 7, d_min=lo[1:2], d_max=hi[1:2], **PERTURB)
    for p, w_ in zip(part, whole):
        assert same_bits(p[0], w_[1])
    assert np.isfinite(part[2]).any()
    # the schedule: rho 2^-iteration in fp64, rounded once
    assert PR.schedule(0.02, 0) == F32(0.02) and PR.schedule(0.02, 3) == F32(0.02 / 8) and PR.schedule(0.3, 2) == F32(np.float64(0.3) / 4)


def _errors(sc, truth_normal, seed):
    """one reference (view 0) from a 16-plane sweep through 4 iterations -> median |depth error| of the initial sweep, of the scene's
    own planes' sweep and of patch_match over the pixels valid before and after, and the median normal error in degrees"""
    refs = np.array([0])
    first, last = sc["depths"][0, 0], sc["depths"][0, -1]
    coarse = np.linspace(first, last, 16).astype(F32)[None]
    args = (sc["images"], sc["poses"], sc["intr"], sc["sources"][:1])
    d16 = MR.sweep(*args, coarse, refs=refs, **sweep_kw(sc))[0][0]
    fine = MR.sweep(*args, sc["depths"][:1], refs=refs, **sweep_kw(sc))[0][0]
    d, n, s = PR.patch_match(*args, coarse, refs=refs, iterations=4, seed=seed, **PERTURB, **sweep_kw(sc))
    truth = sc["depth"][0]
    both = np.isfinite(d16) & np.isfinite(d[0]) & np.isfinite(truth)
    med = lambda m, mask: float(np.median(np.abs(m[mask].astype(np.float64) - truth[mask])))
    unit = n[0][both].astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((unit * truth_normal[both]).sum(axis=1), -1.0, 1.0)))
    return med(d16, both), med(fine, both & np.isfinite(fine)), med(d[0], both), float(np.median(angle)), int(both.sum())


def test_patch_match_beats_its_initial_sweep_on_the_slanted_plane():
    """48 x 48, a plane tilted 30 degrees, 16 planes then 4 iterations: the median |depth error| must be strictly below the
    initial sweep's own and below that of a 48-plane sweep.  The restatement's own values, seeds 0, 1, 2: initial sweep 0.00401,
    48 planes 0.00384, patch_match 0.00094, 0.00094, 0.00093; normal error 1.87, 1.92, 1.96 degrees.  The normal's bound is twice the
    worst of the three seeds."""
    sc = PS.slanted_scene()
    e16, e48, epm, normal_deg, n = _errors(sc, sc["normal"][0], seed=0)
    print(f"slanted plane: {n} pixels, initial sweep {e16:.5f}, 48 planes {e48:.5f}, patch_match {epm:.5f}, normal {normal_deg:.2f} degrees")
    assert n > 1500
    assert epm < e16 and epm < e48
    assert normal_deg <= 2 * 1.96


def test_patch_match_beats_its_initial_sweep_on_the_sphere():
    """64 x 64, the sphere scene's view 0, 16 planes then 4 iterations: the median |depth error| strictly below the initial
    sweep's.  The restatement's own values, seeds 0, 1, 2: initial sweep 0.00476 (48 planes: 0.00433), patch_match 0.00214, 0.00219,
    0.00221; normal error 2.40, 2.39, 2.48 degrees.  The normal's bound is twice the worst of the three seeds."""
    sc = S.sphere_scene()
    K = sc["intr"].astype(np.float64)
    yy, xx = np.mgrid[0:sc["H"], 0:sc["W"]].astype(np.float64)
    rays = np.stack([(xx + 0.5 - K[0, 2]) / K[0, 0], (yy + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(xx)], axis=-1)
    point = rays * np.where(np.isfinite(sc["depth"][0]), sc["depth"][0], 1.0)[..., None]
    outward = point - np.array([0.0, 0.0, S.SPHERE_D])                  # view 0 looks down +z at the centre, SPHERE_D away
    outward /= np.linalg.norm(outward, axis=-1, keepdims=True)
    e16, e48, epm, normal_deg, n = _errors(sc, outward, seed=0)
    print(f"sphere: {n} pixels, initial sweep {e16:.5f}, 48 planes {e48:.5f}, patch_match {epm:.5f}, normal {normal_deg:.2f} degrees")
    assert n > 1500
    assert epm < e16
    assert normal_deg <= 2 * 2.48


def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("H,W,w,t,nan_pose", [(15, 16, 1, 1, False), (17, 33, 2, 2, True), (15, 16, 3, 1, False), (17, 33, 3, 2, False),
                                              (17, 33, 4, 2, True)])
def test_the_torch_forms_on_the_cpu_leave_the_restatement_s_bits(H, W, w, t, nan_pose):
    from ls2fm import mvs
    sc = S.grid_scene(H, W, w, nan_pose=nan_pose)
    ps = scene_of(sc, t)
    depth, normal = (a.copy() for a in PS.edge_state(sc))
    score = PR.plane_score(ps, depth, normal)
    v = tuple(_torch(sc[k]) for k in ("images", "poses", "intr", "sources"))
    refs = _torch(sc["refs"])
    got = mvs.plane_score_torch(*v, _torch(depth), _torch(normal), refs=refs, tap_step=t, **sweep_kw(sc))
    assert same_bits(got.numpy(), score) and np.isfinite(score).any() and np.isnan(score).any()
    state = [_torch(depth).clone(), _torch(normal).clone(), got.clone()]
    lo, hi = d_range(sc)
    for colour in (1, 0):
        PR.step(ps, depth, normal, score, colour, 1, 9, d_min=lo, d_max=hi, **PERTURB)
        out = mvs.patch_match_step_torch(*v, *state, colour, 1, _torch(lo), _torch(hi), refs=refs, seed=9, tap_step=t, **PERTURB, **sweep_kw(sc))
        assert all(o.data_ptr() == s.data_ptr() for o, s in zip(out, state)), "in place"
        for g, r in zip(state, (depth, normal, score)):
            assert same_bits(g.numpy(), r)


@pytest.mark.parametrize("H,W,w", [(4, 5, 2), (17, 33, 2)])
def test_the_torch_sweep_and_the_torch_plane_score_share_one_scene(H, W, w):
    """both torch forms run on one scene object: at one plane, n = (0, 0, -1) and t = 1 the sweep's score is the plane score by
    its bits, at an image smaller than the window (no pixel has one) and at one above the tiles"""
    import torch
    from ls2fm import mvs
    sc = S.grid_scene(H, W, w, D=1)
    v = tuple(_torch(sc[k]) for k in ("images", "poses", "intr", "sources"))
    refs, depths = _torch(sc["refs"]), _torch(sc["depths"])
    swept = mvs.plane_sweep_torch(*v, depths, refs=refs, **sweep_kw(sc))[1]
    normal = torch.zeros(len(refs), H, W, 3)
    normal[..., 2] = -1
    scored = mvs.plane_score_torch(*v, depths[:, 0, None, None].expand(-1, H, W), normal, refs=refs, tap_step=1, **sweep_kw(sc))
    assert same_bits(swept.numpy(), scored.numpy())
    assert np.isnan(swept.numpy()).all() if H < 2 * w + 1 else np.isfinite(swept.numpy()).any()
    assert same_bits(swept.numpy(), MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], **sweep_kw(sc))[1])


def test_normals_to_world_against_numpy():
    import torch
    from ls2fm import mvs
    sc = S.sphere_scene()
    rng = np.random.default_rng(3)
    normal = rng.standard_normal((2, 4, 5, 3)).astype(F32)
    normal[0, 1, 2] = np.nan
    refs = np.array([3, 1])
    got = mvs.normals_to_world(_torch(normal), _torch(sc["poses"]), _torch(refs))
    Rm = sc["poses"][refs][:, :, :3]
    want = np.empty_like(normal)
    for j in range(3):
        want[..., j] = (Rm[:, None, None, 0, j] * normal[..., 0] + Rm[:, None, None, 1, j] * normal[..., 1]) + Rm[:, None, None, 2, j] * normal[..., 2]
    assert got.dtype == torch.float32 and same_bits(got.numpy(), want)
    exact = np.einsum("rji,rhwj->rhwi", Rm.astype(np.float64), np.nan_to_num(normal).astype(np.float64))
    assert np.allclose(np.nan_to_num(got.numpy()), exact, atol=1e-5)
    every = mvs.normals_to_world(torch.zeros(5, 2, 2, 3), _torch(sc["poses"]))
    assert every.shape == (5, 2, 2, 3)
    with pytest.raises(ValueError):
        mvs.normals_to_world(torch.zeros(4, 2, 2, 3), _torch(sc["poses"]))
    with pytest.raises(ValueError):
        mvs.normals_to_world(torch.zeros(5, 2, 2), _torch(sc["poses"]))


def test_refusals_and_argument_errors():
    import torch
    from ls2fm import mvs
    sc = S.grid_scene(15, 16)
    img, pose, intr, src, dep = (_torch(sc[k]) for k in ("images", "poses", "intr", "sources", "depths"))
    refs = _torch(sc["refs"])
    depth, normal = (_torch(a) for a in PS.edge_state(sc))
    score = torch.zeros(3, 15, 16)
    lo, hi = (_torch(a) for a in d_range(sc))
    # the kernel entry points refuse CPU tensors in ls2fm.mvs's name
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.plane_score(img, pose, intr, src, depth, normal, refs=refs)
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.patch_match_step(img, pose, intr, src, depth, normal, score, 0, 0, lo, hi, refs=refs)
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.patch_match(img, pose, intr, src, dep, refs=refs)
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs.*no CPU fallback"):
        mvs.dense_reconstruct(img, pose, intr, ((-1, -1, -1), (1, 1, 1)), 0.1, stereo="patchmatch")
    with pytest.raises(ValueError):
        mvs.dense_reconstruct(img, pose, intr, ((-1, -1, -1), (1, 1, 1)), 0.1, stereo="semi-global")
    step = lambda **kw: mvs.patch_match_step_torch(img, pose, intr, src, depth.clone(), normal.clone(), score.clone(),
                                                   kw.pop("colour", 0), kw.pop("iteration", 0), kw.pop("lo", lo), kw.pop("hi", hi), refs=refs, **kw)
    step()
    for bad in (dict(tap_step=0), dict(tap_step=3), dict(colour=2), dict(colour=-1), dict(iteration=-1), dict(depth_perturb=-1.0),
                dict(depth_perturb=float("nan")), dict(normal_perturb=float("inf")), dict(max_slope=-0.5), dict(half_width=0),
                dict(half_width=6), dict(min_var=-1.0), dict(min_sources=0), dict(min_sources=6), dict(near=0.0), dict(lo=lo[:2])):
        with pytest.raises(ValueError):
            step(**bad)
    for bad in (dict(tap_step=3), dict(half_width=6), dict(near=float("nan"))):
        with pytest.raises(ValueError):
            mvs.plane_score_torch(img, pose, intr, src, depth, normal, refs=refs, **bad)
    with pytest.raises(ValueError):
        mvs.plane_score_torch(img, pose, intr, src, depth[:2], normal, refs=refs)
    with pytest.raises(ValueError):
        mvs.plane_score_torch(img, pose, intr, src, depth, normal[..., :2], refs=refs)
    with pytest.raises(ValueError):
        mvs.patch_match_step_torch(img, pose, intr, src, depth.double(), normal, score, 0, 0, lo, hi, refs=refs)      # not in place
    # the new options have defaults, and the sweep's are what they were
    opt = mvs.MvsOptions()
    assert opt.patchmatch()["iterations"] == 5 and opt.patchmatch()["tap_step"] == 1 and "iterations" not in opt.sweep()
    assert set(opt.sweep()) == {"half_width", "near", "min_var", "min_sources", "max_workspace_bytes"}
