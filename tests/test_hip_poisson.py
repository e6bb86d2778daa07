"""GPU: the screened Poisson solver (csrc/poisson.hip) through ls2fm.cloud_mesh against the numpy restatement
(tests/poisson_restate.py): every stage and the whole solve by the BITS of every lattice point, at both launch plans (the tail
kernel, and every level by its own launches), then poisson_from_cloud, extract, mesh_from_cloud(method="poisson") and trim on top.
tests/test_poisson_host.py asserts the properties of the rule and of the scenes that the tests here lean on."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_mesh_restate as CR
import cloud_mesh_scenes as MS
import poisson_restate as PR
import poisson_scenes as S
from test_hip_cloud_mesh import restated_mesh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (2, 2, 2): no neighbour on one side of any axis; (4, 4, 5) and (5, 4, 4) coarsen, (4, 4, 4) would not; even and odd sides together;
# then the sweep kernel's brick (2, 2, 128): brick and brick + 1 along axes 0 and 1 (a side of brick - 1 = 1 is no lattice), brick
# - 1, brick and brick + 1 along axis 2
STAGE_SHAPES = [(2, 2, 2), (4, 4, 5), (5, 4, 4), (9, 9, 9), (8, 8, 8), (17, 18, 20), (33, 20, 12), (3, 2, 5), (2, 3, 5), (3, 2, 127),
                (2, 3, 128), (2, 2, 129)]
SOLVE_SHAPES = [(9, 9, 9), (16, 16, 16), (17, 18, 20), (33, 20, 12)]      # tail only (729, and 4096 exactly); global levels above a tail


@pytest.fixture(scope="module")
def CM():
    from ls2fm import cloud_mesh
    return cloud_mesh


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(*tensors):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def same(got, exp):
    return all(CR.same_bits(g, e) for g, e in zip(host(*got), exp))


@pytest.fixture(scope="module")
def fields():
    """chi, b, W per stage shape: random, W >= 0 with empty stretches, some exact zeros and a negative zero in chi"""
    out = {}
    for t, shape in enumerate(STAGE_SHAPES):
        rng = np.random.default_rng(200 + t)
        chi, b = rng.normal(size=shape).astype(np.float32), rng.normal(size=shape).astype(np.float32)
        W = np.maximum(rng.normal(size=shape), 0.0).astype(np.float32) * np.float32(3.0)
        chi.reshape(-1)[::7] = 0.0
        chi.reshape(-1)[1] = -0.0
        out[shape] = chi, b, W
    return out


# ---------------------------------------------------------------------------------------------------------- the stages, by bits
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_splat_finish_and_right_hand_side(CM, shape):
    sc = S.small(shape, 400)
    V, W = PR.finish(PR.splat(sc["points"], sc["normals"], *S.lattice_of(sc)), shape)
    assert (W > 0).any()
    got = CM._poisson_splat_device(dev(sc["points"]), dev(sc["normals"]), *S.lattice_of(sc))
    assert same(got, (V, PR.rhs(V), W))


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_one_colour_of_one_sweep(CM, fields, shape):
    chi, b, W = fields[shape]
    for s in (1.0, 1.0 / 16.0):
        for screen in (4.0, 0.25):
            for colour in (0, 1):
                got = CM._poisson_sweep_colour_device(dev(chi), dev(b), dev(W), s, screen, colour)
                assert same((got,), (PR.sweep_colour(chi, b, W, s, screen, colour),)), (s, screen, colour)


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_residual_with_restriction_and_the_restricted_density(CM, fields, shape):
    chi, b, W = fields[shape]
    for s in (1.0, 1.0 / 16.0):
        got = CM._poisson_restrict_device(dev(chi), dev(b), dev(W), s, 4.0)
        assert same((got,), (PR.restrict(PR.residual(chi, b, W, s, 4.0)),)), s
    assert same((CM._poisson_restrict_device(dev(W)),), (PR.restrict(W),))


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_prolongation_with_correction(CM, fields, shape):
    chi = fields[shape][0]
    e = np.random.default_rng(9).normal(size=tuple((n + 1) // 2 for n in shape)).astype(np.float32)
    assert same((CM._poisson_prolong_device(dev(chi), dev(e)),), (PR.correct(chi, e),))


# ---------------------------------------------------------------------------------------------------------- the solve, by bits
@pytest.mark.parametrize("shape", SOLVE_SHAPES)
def test_the_solve_at_both_plans(CM, shape):
    sc = S.small(shape)
    p, n = dev(sc["points"]), dev(sc["normals"])
    levels = [int(np.prod(d)) for d in PR.level_shapes(shape)]
    assert (levels[0] <= 4096) == (shape in SOLVE_SHAPES[:2]) and len(levels) >= 2 and levels[1] <= 4096
    for screen in (0.25, 4.0):
        for gamma in (1, 2):
            for cycles in (0, 1, 3):
                exp = S.expected_small(shape, screen, cycles, gamma)
                for tail in (0, CM.POISSON_TAIL_POINTS):
                    got = CM._poisson_device(p, n, *S.lattice_of(sc), screen, cycles, gamma, tail_points=tail)
                    assert same(got, exp), (screen, gamma, cycles, tail)
    assert np.abs(S.expected_small(shape, 4.0, 3, 2)[0]).max() > 0


@pytest.mark.parametrize("name", S.NAMES)
def test_the_default_solve_on_every_scene(CM, name):
    """the C entry point on the scene as it stands: the NaN rows of `nan_rows`, the points on and outside the last cell and those
    outside the lattice add nothing; no points give chi = 0 and W = 0"""
    sc = S.scene(name)
    got = CM._poisson_device(dev(sc["points"]), dev(sc["normals"]), *S.lattice_of(sc), S.SCREEN, S.CYCLES, S.GAMMA)
    assert same(got, S.expected(name))
    if name == "empty":
        assert not host(got[0])[0].any() and not host(got[1])[0].any()


def test_reruns_and_graph_replay_repeat_the_bits(CM):
    sc = S.small((17, 18, 20))
    exp = S.expected_small((17, 18, 20), 4.0, 3, 2)
    p, n = dev(sc["points"]), dev(sc["normals"])
    run = lambda: CM._poisson_device(p, n, *S.lattice_of(sc), 4.0, 3, 2)        # noqa: E731
    assert same(run(), exp) and same(run(), exp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                        # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        out[0].fill_(7.0)
        out[1].fill_(-7.0)
        graph.replay()
        assert same(out, exp)


def test_a_workspace_that_is_too_small_is_refused(CM):
    from ls2fm import _lib
    sc = S.small((9, 9, 9))
    p, n = dev(sc["points"]), dev(sc["normals"])
    lib = _lib.load()
    need = lib.ls2fm_poisson_workspace_bytes(9, 9, 9)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    value, density = torch.empty((9, 9, 9), device=DEV), torch.empty((9, 9, 9), device=DEV)
    og = (ctypes.c_float * 3)(*sc["origin"])
    call = lambda size: lib.ls2fm_poisson_solve(_lib.ptr(p), _lib.ptr(n), len(p), 9, 9, 9, og, sc["voxel"], 4.0, 1, 2, _lib.ptr(value),   # noqa: E731
                                                _lib.ptr(density), _lib.ptr(ws), size, _lib.stream_ptr())
    assert call(need - 1) == -1 and call(need) == 0
    assert same((value, density), S.expected_small((9, 9, 9), 4.0, 1, 2))


def test_refusals_with_everything_else_in_order(CM):
    """real device arrays, a large enough workspace and ONE wrong option at a time: each check of the entry points refuses on its
    own, before anything is enqueued -- value, density and chi keep the bits they had.  (The host test can only pass NULL arrays,
    which are refused whatever the options are.)"""
    from ls2fm import _lib
    sc = S.small((9, 9, 9))
    p, n = dev(sc["points"]), dev(sc["normals"])
    lib = _lib.load()
    ws = torch.empty(lib.ls2fm_poisson_workspace_bytes(9, 9, 9) + 256, dtype=torch.uint8, device=DEV)
    value, density = torch.full((9, 9, 9), 7.0, device=DEV), torch.full((9, 9, 9), -7.0, device=DEV)
    og, nan3 = (ctypes.c_float * 3)(*sc["origin"]), (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
    good = dict(n=len(p), shape=(9, 9, 9), origin=og, voxel=sc["voxel"], screen=4.0, cycles=1, gamma=2, tail=4096, ws=_lib.ptr(ws),
                size=ws.numel() - 256)

    def solve(plan, **kw):
        a = dict(good, **kw)
        head = (_lib.ptr(p), _lib.ptr(n), a["n"], *a["shape"], a["origin"], a["voxel"], a["screen"], a["cycles"], a["gamma"])
        rest = (_lib.ptr(value), _lib.ptr(density), a["ws"], a["size"], _lib.stream_ptr())
        return lib.ls2fm_poisson_solve_plan(*head, a["tail"], *rest) if plan else lib.ls2fm_poisson_solve(*head, *rest)

    inf, nan = float("inf"), float("nan")
    bad = [dict(n=-1), dict(n=2 ** 31), dict(shape=(1, 9, 9)), dict(shape=(9, 9, 0)), dict(voxel=0.0), dict(voxel=inf), dict(voxel=nan),
           dict(origin=nan3), dict(origin=None), dict(cycles=-1), dict(gamma=0), dict(gamma=3), dict(screen=0.0), dict(screen=-1.0),
           dict(screen=inf), dict(screen=nan), dict(ws=None), dict(ws=ctypes.c_void_p(ws.data_ptr() + 16)), dict(size=good["size"] - 1)]
    for kw in bad:
        assert solve(False, **kw) == -1 and solve(True, **kw) == -1, kw
    for tail in (-1, 1, 4095, 8192):
        assert solve(True, tail=tail) == -1, tail
    chi = torch.full((9, 9, 9), 7.0, device=DEV)
    b, W, coarse = torch.ones((9, 9, 9), device=DEV), torch.ones((9, 9, 9), device=DEV), torch.full((5, 5, 5), 7.0, device=DEV)
    P, st = _lib.ptr, _lib.stream_ptr()
    for s, screen, colour in ((0.0, 4.0, 0), (2.0, 4.0, 0), (nan, 4.0, 0), (1.0, 0.0, 0), (1.0, inf, 0), (1.0, nan, 1), (1.0, 4.0, 2), (1.0, 4.0, -1)):
        assert lib.ls2fm_poisson_sweep_colour(P(chi), P(b), P(W), 9, 9, 9, s, screen, colour, st) == -1, (s, screen, colour)
    for s, screen in ((0.0, 4.0), (2.0, 4.0), (1.0, 0.0), (1.0, -4.0), (1.0, nan)):
        assert lib.ls2fm_poisson_restrict(P(chi), P(b), P(W), 9, 9, 9, s, screen, P(coarse), st) == -1, (s, screen)
    assert lib.ls2fm_poisson_restrict(P(chi), P(b), None, 9, 9, 9, 1.0, 4.0, P(coarse), st) == -1          # b without W
    assert lib.ls2fm_poisson_restrict(P(chi), P(b), P(W), 9, 1, 9, 1.0, 4.0, P(coarse), st) == -1
    assert lib.ls2fm_poisson_prolong(P(chi), 9, 9, 1, P(coarse), st) == -1
    torch.cuda.synchronize()
    assert bool((value == 7.0).all()) and bool((density == -7.0).all()) and bool((chi == 7.0).all()) and bool((coarse == 7.0).all())
    assert solve(False) == 0 and solve(True) == 0                                      # and the good call is accepted
    assert same((value, density), S.expected_small((9, 9, 9), 4.0, 1, 2))


# ------------------------------------------------------------------------------------------------------- the higher-level routes
def lattice_bounds(sc):
    lo = sc["origin"]
    return lo, tuple(o + (s - 1) * sc["voxel"] for o, s in zip(lo, sc["shape"]))      # dyadic: shape_for's shape is the scene's


@pytest.mark.parametrize("name", ["sphere", "capped", "two"])
def test_poisson_from_cloud_extract_and_mesh_from_cloud_against_the_restated_route(CM, name):
    sc = S.scene(name)
    p, n = dev(sc["points"]), dev(sc["normals"])
    kept_p, kept_n = host(*CM._oriented(p, n, "test"))                                  # the normalisation is torch's
    assert len(kept_p) == len(sc["points"]) and np.abs(np.linalg.norm(kept_n.astype(np.float64), axis=1) - 1).max() < 1e-6
    exp = PR.solve(kept_p, kept_n, *S.lattice_of(sc), S.SCREEN, S.CYCLES, S.GAMMA)
    vol = CM.poisson_from_cloud(p, n.double(), sc["voxel"], bounds=lattice_bounds(sc))
    assert vol.shape == sc["shape"] and vol.origin == sc["origin"] and vol.device == p.device and same((vol.value, vol.support), exp)
    v, f = restated_mesh(exp[0], exp[1], 0.0, sc["origin"], sc["voxel"])
    out, again = CM.mesh_from_cloud(p, n, voxel=sc["voxel"], bounds=lattice_bounds(sc), method="poisson", return_volume=True)
    assert isinstance(again, CM.PoissonVolume) and torch.equal(again.value, vol.value) and torch.equal(again.support, vol.support)
    for mesh in (out, CM.extract(vol)):
        gv, gf = host(mesh.vertices, mesh.faces)
        assert gf.dtype == np.int32 and np.array_equal(gv.view(np.uint32), v.view(np.uint32)) and np.array_equal(gf, f)
    assert np.isfinite(v).all() and (len(f) > 1000 if name != "two" else True)
    # rows the filter drops, and normals of any length: the same volume
    bad_p, bad_n = torch.cat([p[[0, 0, 0, 0]], p]), torch.cat([n[[0, 0, 0, 0]], n * 3.5])
    bad_p[0, 1], bad_n[1, 2], bad_n[2], bad_n[3, 0] = float("nan"), float("inf"), 0.0, float("nan")
    dropped = CM.poisson_from_cloud(bad_p, bad_n, sc["voxel"], bounds=lattice_bounds(sc))
    scaled = host(*CM._oriented(p, n * 3.5, "test"))
    assert same((dropped.value, dropped.support), PR.solve(scaled[0], scaled[1], *S.lattice_of(sc), S.SCREEN, S.CYCLES, S.GAMMA))


def test_the_default_bounds_are_the_box_grown_by_a_tenth_and_two_voxels(CM):
    sc = S.scene("crowded")
    p, n = dev(sc["points"]), dev(sc["normals"])
    lo, hi = sc["points"].min(axis=0).astype(np.float64), sc["points"].max(axis=0).astype(np.float64)
    margin = 0.1 * max(float(h) - float(l) for l, h in zip(lo, hi)) + 2.0 * sc["voxel"]
    lo, hi = [float(v) - margin for v in lo], [float(v) + margin for v in hi]
    shape = tuple(max(2, int(np.ceil((h - l) / sc["voxel"])) + 1) for l, h in zip(lo, hi))
    vol = CM.poisson_from_cloud(p, n, sc["voxel"], screen=1.0, cycles=2, gamma=1)
    assert vol.shape == shape and vol.origin == tuple(lo) and vol.screen == 1.0
    kept = host(*CM._oriented(p, n, "test"))
    assert same((vol.value, vol.support), PR.solve(kept[0], kept[1], shape, lo, sc["voxel"], 1.0, 2, 1))
    # poisson_residual is the restatement's figure, and more cycles lower it
    exp = PR.solve(kept[0], kept[1], shape, lo, sc["voxel"], 1.0, 2, 1)
    b, W = PR.system(kept[0], kept[1], shape, lo, sc["voxel"])
    figure = CM.poisson_residual(vol, p, n)
    assert abs(figure - PR.relative_residual(exp[0], b, W, 1.0)) <= 1e-6 * figure
    assert CM.poisson_residual(CM.poisson_from_cloud(p, n, sc["voxel"], screen=1.0, cycles=6), p, n) < 0.1 * figure


def edge_uses(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def test_the_capped_spheres_mesh_is_closed_and_the_local_surface_is_not(CM):
    sc = S.scene("capped")
    p, n = dev(sc["points"]), dev(sc["normals"])
    closed = CM.mesh_from_cloud(p, n, voxel=sc["voxel"], bounds=lattice_bounds(sc), method="poisson")
    uses = edge_uses(host(closed.faces)[0])
    assert len(uses) > 1000 and (uses == 2).all()
    local = CM.mesh_from_cloud(p, n, voxel=sc["voxel"], bounds=lattice_bounds(sc), method="mls")
    uses = edge_uses(host(local.faces)[0])
    assert (uses == 1).sum() > 20                                                       # an open rim around the hole


def test_trim_against_a_numpy_nearest_neighbour(CM):
    """the hemisphere's closed surface trimmed at 2 voxels: the faces with all three vertices within that distance of the cloud"""
    sc = S.scene("hemisphere")
    p, n = dev(sc["points"]), dev(sc["normals"])
    r = 2.0 * sc["voxel"]
    whole = CM.mesh_from_cloud(p, n, voxel=sc["voxel"], bounds=lattice_bounds(sc), method="poisson")
    v, f = host(whole.vertices, whole.faces)
    d = np.sqrt(((v.astype(np.float64)[:, None] - sc["points"].astype(np.float64)[None]) ** 2).sum(axis=2).min(axis=1))
    assert (np.abs(d - r) > 1e-5 * r).all()                                             # no vertex on the threshold: fp32 and fp64 agree
    near = d <= r
    keep = near[f].all(axis=1)
    assert 500 < keep.sum() < len(f) - 500
    used = np.zeros(len(v), bool)
    used[f[keep].reshape(-1)] = True
    trimmed = CM.mesh_from_cloud(p, n, voxel=sc["voxel"], bounds=lattice_bounds(sc), method="poisson", trim=r)
    gv, gf = host(trimmed.vertices, trimmed.faces)
    assert np.array_equal(gv.view(np.uint32), v[used].view(np.uint32)) and np.array_equal(gf, (np.cumsum(used) - 1)[f[keep]].astype(np.int32))
    assert (edge_uses(gf) == 1).any()                                                   # open again
    far = CM.mesh_from_cloud(p, n, voxel=sc["voxel"], bounds=lattice_bounds(sc), method="poisson", trim=1e3)
    assert torch.equal(far.vertices, whole.vertices) and torch.equal(far.faces, whole.faces)


def test_the_spheres_mesh_scores_below_a_voxel(CM):
    from ls2fm import metrics
    sc = S.scene("sphere")
    out = CM.mesh_from_cloud(dev(sc["points"]), dev(sc["normals"]), voxel=sc["voxel"], method="poisson")
    gt = dev((S.SPHERE_CENTRE + S.SPHERE_RADIUS * MS._fibonacci(40000)).astype(np.float32))
    score = metrics.evaluate_mesh(out.vertices, out.faces, gt, 3 * sc["voxel"], 0.25 * sc["voxel"], generator=torch.Generator(device=DEV).manual_seed(5))
    print(f"sphere mesh: accuracy {score['accuracy'] / sc['voxel']:.4f} voxel, completeness {score['completeness'] / sc['voxel']:.4f} voxel")
    assert score["accuracy"] < sc["voxel"] and score["completeness"] < sc["voxel"]
    assert score["n_completeness"] == score["n_gt"] and score["n_accuracy"] == score["n_pred"]
    v, f = out.vertices.double(), out.faces.long()
    signed = (v[f[:, 0]] * torch.linalg.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0     # outward normals give outward faces
    assert abs(float(signed) / (4.0 / 3.0 * np.pi * S.SPHERE_RADIUS ** 3) - 1.0) < 0.05
