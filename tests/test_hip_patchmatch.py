"""GPU: ls2fm_mvs_plane_score and ls2fm_mvs_patchmatch_step (csrc/mvs_patchmatch.hip) through ls2fm.mvs: depth, normal and score of
every pixel by their bits against the numpy restatement (tests/patchmatch_restate.py); patch_match and
dense_reconstruct(stereo="patchmatch") on top of them.  The rules themselves, and that the scenes meet their edges, are judged on
the restatement (tests/test_patchmatch_host.py)."""
import functools

import numpy as np
import pytest
import torch

import mvs_scenes as S
import patchmatch_restate as PR
import patchmatch_scenes as PS

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
PERTURB = dict(depth_perturb=0.02, normal_perturb=0.5, max_slope=1.0)


@pytest.fixture(scope="module")
def MV():
    from ls2fm import mvs
    return mvs


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same(got, ref, what):
    """bit for bit; a NaN matches a NaN"""
    g, r = host(got), host(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, f"{what}: {g.dtype} {g.shape} != {r.dtype} {r.shape}"
    bad = (g.view(np.int32) != r.view(np.int32)) & ~(np.isnan(g) & np.isnan(r))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ, the first at {tuple(np.argwhere(bad)[0])}"


def check(got, ref, what=""):
    torch.cuda.synchronize()
    for name, g, r in zip(("score", "depth", "normal"), (got[2], got[0], got[1]), (ref[2], ref[0], ref[1])):
        same(g, r, f"{name} {what}")


def sweep_kw(sc):
    return dict(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])


def views(sc, rows=slice(None)):
    refs = sc.get("refs")
    return (dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"][rows])), None if refs is None else dev(refs[rows])


def d_range(sc):
    return sc["depths"].min(axis=1), sc["depths"].max(axis=1)


@functools.lru_cache(maxsize=None)
def restated_steps(args, t, first, iteration, seed):
    """from the hand-made edge state: its scores, then the state after colour `first` and after the other colour"""
    sc = S.grid_scene(*args)
    ps = PR.Scene(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["refs"], tap_step=t, **sweep_kw(sc))
    depth, normal = (a.copy() for a in PS.edge_state(sc))
    score = PR.plane_score(ps, depth, normal)
    out = [(depth.copy(), normal.copy(), score.copy())]
    lo, hi = d_range(sc)
    for colour in (first, 1 - first):
        PR.step(ps, depth, normal, score, colour, iteration, seed, d_min=lo, d_max=hi, **PERTURB)
        out.append((depth.copy(), normal.copy(), score.copy()))
    return out


# H, W, w, S, R, t, nan_pose, first colour, iteration, seed.  The tile is 16 x 32: an image one below, equal to and one above it in
# each axis, and 32 x 48 (two tiles down, a part of a second across); every w, S, t and R of the lists with every image size; both
# colours start, iterations 0 and 3, two seeds, nan_pose (where enough sources remain for a score).  The state is edge_state's, on
# grid_scene's NaN and +-inf pixels.
CASES = [(15, 31, 1, 1, 1, 1, False, 0, 0, 0), (15, 31, 2, 3, 3, 2, False, 1, 3, 1), (15, 31, 5, 5, 3, 1, True, 0, 0, 1),
         (16, 32, 1, 5, 3, 2, False, 1, 3, 0), (16, 32, 2, 1, 1, 1, True, 0, 0, 1), (16, 32, 5, 3, 3, 2, False, 0, 3, 1),
         (17, 33, 1, 3, 1, 1, False, 1, 3, 1), (17, 33, 2, 5, 3, 1, True, 0, 0, 0), (17, 33, 5, 1, 3, 2, False, 1, 3, 0),
         (32, 48, 1, 5, 3, 1, True, 1, 0, 1), (32, 48, 2, 3, 1, 2, False, 0, 3, 0), (32, 48, 5, 1, 3, 1, False, 0, 0, 0),
         # w = 3 (the default) and w = 4 with both tap steps, each at two of the sizes; (3, 2) is the one pattern without a centre tap
         (15, 31, 3, 5, 3, 1, False, 0, 0, 0), (17, 33, 3, 3, 3, 1, True, 1, 3, 1), (16, 32, 3, 3, 1, 2, False, 1, 3, 0),
         (32, 48, 3, 5, 3, 2, False, 0, 0, 1), (15, 31, 4, 5, 3, 1, False, 1, 0, 1), (32, 48, 4, 1, 3, 1, False, 0, 3, 0),
         (16, 32, 4, 5, 3, 2, True, 0, 3, 1), (17, 33, 4, 3, 2, 2, False, 1, 0, 0)]


@pytest.mark.parametrize("H,W,w,S_,R,t,nan_pose,first,iteration,seed", CASES)
def test_bits_of_the_restatement(MV, H, W, w, S_, R, t, nan_pose, first, iteration, seed):
    args = (H, W, w, S_, R, 17, nan_pose, False)
    sc = S.grid_scene(*args)
    ref = restated_steps(args, t, first, iteration, seed)
    v, refs = views(sc)
    depth, normal = (dev(a) for a in PS.edge_state(sc))
    score = MV.plane_score(*v, depth, normal, refs=refs, tap_step=t, **sweep_kw(sc))
    check((depth, normal, score), ref[0], "plane_score")
    assert np.isnan(ref[0][2]).any() and np.isfinite(ref[0][2]).any()
    lo, hi = (dev(a) for a in d_range(sc))
    for i, colour in enumerate((first, 1 - first)):
        out = MV.patch_match_step(*v, depth, normal, score, colour, iteration, lo, hi, refs=refs, seed=seed, tap_step=t, **PERTURB, **sweep_kw(sc))
        assert all(o.data_ptr() == s.data_ptr() for o, s in zip(out, (depth, normal, score))), "the step works in place"
        check(out, ref[1 + i], f"after colour {colour}")


def test_plane_score_alone_on_a_swept_state(MV):
    """the state patch_match starts from: the sweep's depth with fronto-parallel normals, both tap steps"""
    import mvs_restate as MR
    args = (17, 33, 2, 5, 3, 17, False, False)
    sc = S.grid_scene(*args)
    depth = MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], **sweep_kw(sc))[0]
    normal = np.zeros(depth.shape + (3,), F32)
    normal[..., 2] = -1
    v, refs = views(sc)
    for t in (1, 2):
        ps = PR.Scene(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["refs"], tap_step=t, **sweep_kw(sc))
        want = PR.plane_score(ps, depth, normal)
        got = MV.plane_score(*v, dev(depth), dev(normal), refs=refs, tap_step=t, **sweep_kw(sc))
        torch.cuda.synchronize()
        same(got, want, f"plane_score, tap step {t}")
        assert np.isfinite(want).any()


def test_the_default_half_width_is_three(MV):
    """plane_sweep, plane_score, patch_match_step and patch_match called without half_width, against the restatements at 3"""
    import mvs_restate as MR
    args = (17, 33, 3, 5, 3, 17, False, False)
    sc = S.grid_scene(*args)
    kw = dict(near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])
    v, refs = views(sc)
    swept = MV.plane_sweep(*v, dev(sc["depths"]), refs=refs, **kw)
    want = MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], half_width=3, **kw)
    torch.cuda.synchronize()
    for name, g, r in zip(("depth", "score"), swept, want):
        same(g, r, f"{name} of the default sweep")
    assert np.array_equal(host(swept[2]), want[2]) and (want[2] >= 0).any()
    ref = restated_steps(args, 1, 0, 0, 0)
    depth, normal = (dev(a) for a in PS.edge_state(sc))
    score = MV.plane_score(*v, depth, normal, refs=refs, **kw)
    check((depth, normal, score), ref[0], "default plane_score")
    assert np.isfinite(ref[0][2]).any()
    lo, hi = (dev(a) for a in d_range(sc))
    for i, colour in enumerate((0, 1)):
        check(MV.patch_match_step(*v, depth, normal, score, colour, 0, lo, hi, refs=refs, seed=0, **PERTURB, **kw), ref[1 + i],
              f"default step, colour {colour}")
    loop = PR.patch_match(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], iterations=1, seed=2,
                          half_width=3, **PERTURB, **kw)
    check(MV.patch_match(*v, dev(sc["depths"]), refs=refs, iterations=1, seed=2, **PERTURB, **kw), loop, "default patch_match")
    assert np.isfinite(loop[2]).any()


def test_two_iterations_from_the_edge_state(MV):
    """the hand-made edge state of the scenes file through four half-sweeps: a state that moves under the kernel as it does
    under the restatement"""
    args = (17, 33, 1, 5, 3, 17, False, False)
    sc = S.grid_scene(*args)
    init = PS.edge_state(sc)
    want = PR.patch_match(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], iterations=2, init=init,
                          seed=5, **PERTURB, **sweep_kw(sc))
    v, refs = views(sc)
    got = MV.patch_match(*v, dev(sc["depths"]), refs=refs, iterations=2, init=tuple(dev(a) for a in init), seed=5, **PERTURB, **sweep_kw(sc))
    check(got, want, "two iterations from the edge state")
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()
    assert np.array_equal(np.isnan(want[0]), np.isnan(want[2])) and np.array_equal(np.isnan(want[1]).any(axis=-1), np.isnan(want[2]))


@functools.lru_cache(maxsize=None)
def restated_loop(args, t):
    sc = S.grid_scene(*args)
    return PR.patch_match(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc["refs"], iterations=2, seed=3,
                          tap_step=t, **PERTURB, **sweep_kw(sc))


LOOP = (17, 33, 2, 5, 3, 17, False, False)


def run_loop(MV, sc, rows=slice(None), t=1, **kw):
    v, refs = views(sc, rows)
    return MV.patch_match(*v, dev(sc["depths"][rows]), refs=refs, iterations=2, seed=3, tap_step=t, **PERTURB, **sweep_kw(sc), **kw)


@pytest.mark.parametrize("t", [1, 2])
def test_patch_match_equals_the_restated_loop(MV, t):
    """plane_sweep -> plane_score -> 2 iterations of both colours, against the same loop over the restatements"""
    check(run_loop(MV, S.grid_scene(*LOOP), t=t), restated_loop(LOOP, t), f"patch_match, tap step {t}")


def test_the_torch_form_on_the_device_gives_the_kernel_s_bits(MV):
    args = (17, 33, 2, 3, 3, 17, False, False)
    sc = S.grid_scene(*args)
    ref = restated_steps(args, 1, 0, 0, 0)
    v, refs = views(sc)
    depth, normal = (dev(a) for a in PS.edge_state(sc))
    score = MV.plane_score_torch(*v, depth, normal, refs=refs, **sweep_kw(sc))
    same(score, MV.plane_score(*v, depth, normal, refs=refs, **sweep_kw(sc)), "plane_score_torch against the kernel")
    lo, hi = (dev(a) for a in d_range(sc))
    kernel = [t.clone() for t in (depth, normal, score)]
    for i, colour in enumerate((0, 1)):
        got = MV.patch_match_step_torch(*v, depth, normal, score, colour, 0, lo, hi, refs=refs, seed=0, **PERTURB, **sweep_kw(sc))
        MV.patch_match_step(*v, *kernel, colour, 0, lo, hi, refs=refs, seed=0, **PERTURB, **sweep_kw(sc))
        check(got, kernel, f"torch form against the kernel, colour {colour}")
        check(got, ref[1 + i], f"torch form, colour {colour}")


def test_references_in_chunks_a_rerun_and_a_replay(MV):
    sc = S.grid_scene(*LOOP)
    ref = restated_loop(LOOP, 1)
    check(run_loop(MV, sc), ref, "one call")
    check(run_loop(MV, sc, max_workspace_bytes=1), ref, "one reference per chunk")
    for r in range(3):
        check(run_loop(MV, sc, slice(r, r + 1)), tuple(t[r:r + 1] for t in ref), f"reference {r} alone")
    check(run_loop(MV, sc), ref, "rerun")
    v, refs = views(sc)
    depths = dev(sc["depths"])
    run = lambda: MV.patch_match(*v, depths, refs=refs, iterations=2, seed=3, **PERTURB, **sweep_kw(sc))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                       # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        for t in out:
            t.fill_(7)
        graph.replay()
        check(out, ref, "replay")


def test_dense_reconstruct_with_patchmatch_finds_the_sphere(MV):
    """the sphere scene end to end from a 16-plane sweep: every vertex within two voxels of the sphere, the bound of the sweep's
    end-to-end test (tests/test_hip_mvs.py); the world normals are masked by the filter and point away from the centre's side that
    the cameras do not see"""
    sc = S.sphere_scene()
    opt = MV.MvsOptions(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"],
                        max_reproj=sc["max_reproj"], rel_depth=sc["rel_depth"], min_consistent=sc["min_consistent"])
    depths = np.broadcast_to(np.linspace(1.9, 2.6, 16).astype(F32), (5, 16)).copy()
    out, filtered, count, world = MV.dense_reconstruct(dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), sc["bounds"], sc["voxel"],
                                                       sources=dev(sc["sources"]), depths=dev(depths), options=opt, return_depth=True,
                                                       stereo="patchmatch")
    torch.cuda.synchronize()
    assert out.faces.shape[0] > 300
    r = np.linalg.norm(host(out.vertices).astype(np.float64), axis=1)
    assert (np.abs(r - S.SPHERE_R) <= 2 * sc["voxel"]).all()
    alive = np.isfinite(host(filtered))
    assert alive.sum() > 1000 and np.array_equal(np.isfinite(host(world)).all(axis=-1), alive)
    assert (host(world)[alive][:, 2] < 0).all(), "every camera stands on the -z side: the visible normals point there"
    # the default planes run too
    auto = MV.dense_reconstruct(dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), sc["bounds"], sc["voxel"], stereo="patchmatch",
                                options=MV.MvsOptions(half_width=2, min_var=sc["min_var"], iterations=2))
    assert auto.faces.shape[0] > 100 and bool(torch.isfinite(auto.vertices).all())


def test_refusals_and_empty_calls(MV):
    from ls2fm import _lib, _posed
    lib = _lib.load()
    sc = S.grid_scene(15, 16)
    img, src, refs = dev(sc["images"]), dev(sc["sources"]).int(), dev(sc["refs"]).int()
    poses, k4 = _posed.views(dev(sc["poses"]), dev(sc["intr"]), "test")
    rel = MV.relative_poses(poses, refs, src)
    depth, normal = (dev(a) for a in PS.edge_state(sc))
    score = torch.zeros(3, 15, 16, device=DEV)
    lo, hi = (dev(a) for a in d_range(sc))
    p, s = _lib.ptr, _lib.stream_ptr()
    inf, nan = float("inf"), float("nan")

    def score_(im=img, V=6, H=15, W=16, rf=refs, R=3, sr=src, S_=5, rl=rel, k=k4, w=1, t=1, near=0.5, min_var=0.01, min_sources=2,
               d=depth, n=normal, o=score):
        return lib.ls2fm_mvs_plane_score(p(im), V, H, W, p(rf), R, p(sr), S_, p(rl), p(k), w, t, near, min_var, min_sources, p(d), p(n), p(o), s)

    def step_(im=img, V=6, H=15, W=16, rf=refs, R=3, sr=src, S_=5, rl=rel, k=k4, w=1, t=1, near=0.5, min_var=0.01, min_sources=2,
              colour=0, iteration=0, seed=0, rho_d=0.02, rho_n=0.5, sigma=1.0, lo_=lo, hi_=hi, d=depth, n=normal, o=score):
        return lib.ls2fm_mvs_patchmatch_step(p(im), V, H, W, p(rf), R, p(sr), S_, p(rl), p(k), w, t, near, min_var, min_sources, colour,
                                             iteration, seed, rho_d, rho_n, sigma, p(lo_), p(hi_), p(d), p(n), p(o), s)
    shared = (dict(im=None), dict(rf=None), dict(sr=None), dict(rl=None), dict(k=None), dict(d=None), dict(n=None), dict(o=None),
              dict(V=-1), dict(V=0), dict(H=0), dict(W=32769), dict(R=-1), dict(S_=0), dict(S_=65), dict(w=0), dict(w=6), dict(t=0),
              dict(t=3), dict(near=0.0), dict(near=nan), dict(near=inf), dict(min_var=-1.0), dict(min_var=nan), dict(min_var=inf),
              dict(min_sources=0), dict(min_sources=6))
    assert score_() == 0 and step_() == 0
    for kw in shared:
        assert score_(**kw) == -1, kw
        assert step_(**kw) == -1, kw
    for kw in (dict(colour=-1), dict(colour=2), dict(iteration=-1), dict(rho_d=-1.0), dict(rho_d=nan), dict(rho_d=inf), dict(rho_n=-1.0),
               dict(rho_n=nan), dict(rho_n=inf), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(lo_=None), dict(hi_=None)):
        assert step_(**kw) == -1, kw
    assert score_(R=0, rf=None, d=None, n=None, o=None) == 0
    assert step_(R=0, rf=None, d=None, n=None, o=None, lo_=None, hi_=None) == 0
    torch.cuda.synchronize()
    # a reference outside [0, V): NaN scores, and the step leaves its state as it is
    v = (img, dev(sc["poses"]), dev(sc["intr"]), src[:2])
    out_refs = torch.tensor([0, 6], device=DEV)
    sc_ = MV.plane_score(*v, depth[:2], normal[:2], refs=out_refs, **sweep_kw(sc))
    assert np.isnan(host(sc_)[1]).all() and np.isfinite(host(sc_)[0]).any()
    before = [t[:2].clone() for t in (depth, normal)]
    state = [before[0].clone(), before[1].clone(), sc_.clone()]
    MV.patch_match_step(*v, *state, 0, 0, lo[:2], hi[:2], refs=out_refs, **sweep_kw(sc))
    torch.cuda.synchronize()
    same(state[0][1], before[0][1], "depth of a reference outside the views")
    same(state[1][1], before[1][1], "normal of a reference outside the views")
    assert np.isnan(host(state[2])[1]).all()
    # CPU tensors and bad arguments
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs"):
        MV.plane_score(img.cpu(), dev(sc["poses"]), dev(sc["intr"]), src, depth, normal, refs=refs)
    with pytest.raises(ValueError):
        MV.patch_match_step(*v[:3], src, depth, normal, score.double(), 0, 0, lo, hi, refs=refs)
    with pytest.raises(ValueError):
        MV.patch_match(*v[:3], src, dev(sc["depths"]), refs=refs, tap_step=3)
