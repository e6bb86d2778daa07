"""GPU: ls2fm_cloud_implicit (csrc/cloud_implicit.hip) through ls2fm.cloud_mesh against the numpy restatement
(tests/cloud_mesh_restate.py) on the scenes of tests/cloud_mesh_scenes.py, then implicit_from_cloud, extract and mesh_from_cloud on
top of it.

THE IMPLICIT RULE makes the volume a pure function of the cloud, the normals, the lattice, k, max_d2 and min_neighbors: the BITS of
value (NaN in exactly the same places) and of support are compared on every lattice point, at every launch plan (both bricks, with
and without the empty-brick test).  tests/test_cloud_mesh_host.py asserts the properties of the scenes that the tests here lean on."""
import numpy as np
import pytest
import torch

import cloud_mesh_restate as CR
import cloud_mesh_scenes as S
from test_hip_metrics import cell_sizes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLANS = [None] + [dict(brick=b, empty_test=e) for b in (0, 1) for e in (False, True)]


@pytest.fixture(scope="module")
def MT():
    from ls2fm import metrics
    return metrics


@pytest.fixture(scope="module")
def CM():
    from ls2fm import cloud_mesh
    return cloud_mesh


def dev(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def host(*tensors):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def kernel(CM, MT, points, normals, shape, origin, voxel, radius, k=S.K, least=S.MIN_NEIGHBORS, cell_size=None, plan=None, grid=None):
    p, n = dev(points), dev(normals)
    grid = MT.PointGrid(p, cell_size=cell_size) if grid is None else grid
    return CM._implicit_device(p, n, grid, tuple(shape), tuple(origin), float(voxel), k, MT.squared_cutoff(radius), least, plan)


def same(got, exp):
    got = host(*got)
    return CR.same_bits(got[0], exp[0]) and CR.same_bits(got[1], exp[1])


def lattice_of(sc):
    return sc["shape"], sc["origin"], sc["voxel"], sc["radius"]


# ------------------------------------------------------------------------------------------------------ the kernel, by bits
@pytest.mark.parametrize("name", S.NAMES)
def test_kernel_equals_restatement_at_three_cell_sizes_and_every_plan(CM, MT, name):
    sc = S.scene(name)
    exp = S.expected(name)
    sizes = cell_sizes(MT, dict(ref=sc["points"], cell_size=None)) if len(sc["points"]) else (None,)
    for h in sizes:
        grid = MT.PointGrid(dev(sc["points"]), cell_size=h)
        for plan in PLANS:
            got = kernel(CM, MT, sc["points"], sc["normals"], *lattice_of(sc), plan=plan, grid=grid)
            assert same(got, exp), f"{name} at cell size {h}, plan {plan}"


@pytest.mark.parametrize("name", ["sphere", "duplicates"])
def test_every_capacity_and_threshold(CM, MT, name):
    """k on both sides of the list capacities 8 / 16 / 32, min_neighbors 1, 3 and k"""
    sc = S.scene(name)
    grid = MT.PointGrid(dev(sc["points"]))
    for k in (1, 8, 9, 16, 17, 32):
        for least in sorted({1, 3, k}):
            for plan in (PLANS[1], PLANS[4]):
                got = kernel(CM, MT, sc["points"], sc["normals"], *lattice_of(sc), k=k, least=least, plan=plan, grid=grid)
                assert same(got, S.expected(name, k, least)), f"{name} at k = {k}, min_neighbors = {least}, plan {plan}"


def test_support_may_be_null(CM, MT):
    from ls2fm import _lib
    import ctypes
    sc = S.scene("duplicates")
    p, n = dev(sc["points"]), dev(sc["normals"])
    grid = MT.PointGrid(p)
    value = torch.empty(sc["shape"], dtype=torch.float32, device=DEV)
    og = (ctypes.c_float * 3)(*sc["origin"])
    _lib.check(_lib.load().ls2fm_cloud_implicit(_lib.ptr(p), _lib.ptr(n), *grid.c_args(n_first=True), *sc["shape"], og, sc["voxel"], S.K,
                                                float(MT.squared_cutoff(sc["radius"])), S.MIN_NEIGHBORS, _lib.ptr(value), None, _lib.stream_ptr()),
               "ls2fm_cloud_implicit")
    assert CR.same_bits(host(value)[0], S.expected("duplicates")[0])


@pytest.mark.parametrize("brick", [0, 1])
def test_lattice_shapes_on_both_sides_of_the_brick(CM, MT, brick):
    """per axis 2, brick - 1, brick and brick + 1 lattice points, one axis at a time, the lattice centred on the cloud"""
    sc = S.scene("duplicates")
    centre = np.array([0.2, -0.31, 0.43])
    grid = MT.PointGrid(dev(sc["points"]))
    rest = (5, 3, 6)
    for axis in range(3):
        b = CM.BRICKS[brick][axis]
        for side in sorted({2, max(b - 1, 1), b, b + 1}):
            shape = tuple(side if a == axis else rest[a] for a in range(3))
            origin = tuple(float(np.float32(centre[a] - 0.5 * (shape[a] - 1) * 2 * sc["voxel"])) for a in range(3))
            voxel = 2 * sc["voxel"]
            exp = CR.implicit(sc["points"], sc["normals"], shape, origin, voxel, sc["radius"], S.K, S.MIN_NEIGHBORS)
            assert np.isfinite(exp[0]).any()
            for empty in (False, True):
                got = kernel(CM, MT, sc["points"], sc["normals"], shape, origin, voxel, sc["radius"], plan=dict(brick=brick, empty_test=empty), grid=grid)
                assert same(got, exp), f"brick {brick}, lattice {shape}, empty test {empty}"


def test_exact_distances(CM, MT):
    """a dyadic cloud on a dyadic lattice (voxel 1 / 4, radius 1 / 2, max_d2 = 1 / 4 exactly), min_neighbors = 1: a lattice point
    that coincides with a cloud point (d2 = 0, weight 1), one that lists a neighbour at exactly d2 == max_d2 (weight 0) beside
    another, and one whose only neighbour sits at that distance (den == 0: NaN although n = 1 >= min_neighbors)"""
    points = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.75], [1.25, 1.0, 0.25]], np.float32)
    normals = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [1.0, 0.0, 0.0]], np.float32)
    shape, origin, voxel, radius = (7, 6, 5), (0.0, 0.0, 0.0), 0.25, 0.5
    idx, d2, count = CR.neighbours(points, shape, origin, voxel, radius, 4)
    idx, d2, count = (a.reshape(*shape, -1) for a in (idx, d2, count))
    exp = CR.implicit(points, normals, shape, origin, voxel, radius, 4, 1)
    assert d2[2, 2, 2, 0] == 0 and idx[2, 2, 2, 0] == 0 and np.isfinite(exp[0][2, 2, 2])
    assert idx[2, 2, 4].tolist()[:2] == [1, 0] and d2[2, 2, 4, 1] == np.float32(0.25) and np.isfinite(exp[0][2, 2, 4])
    assert count[0, 2, 2, 0] == 1 and d2[0, 2, 2, 0] == np.float32(0.25) and np.isnan(exp[0][0, 2, 2]) and exp[1][0, 2, 2] == 0
    for h in (None, 0.1, 8.0):
        for plan in PLANS:
            assert same(kernel(CM, MT, points, normals, shape, origin, voxel, radius, k=4, least=1, cell_size=h, plan=plan), exp), (h, plan)


def test_a_nan_normal_shows_exactly_where_its_point_is_listed(CM, MT):
    sc = S.scene("duplicates")
    normals = sc["normals"].copy()
    normals[17, 1] = np.nan
    listed = (S.lists("duplicates")[0][:, :S.K] == 17).any(axis=1).reshape(sc["shape"])
    clean = S.expected("duplicates", S.K, 1)
    exp = CR.implicit(sc["points"], normals, *lattice_of(sc), S.K, 1)
    assert listed.sum() > 20 and np.array_equal(np.isnan(exp[0]), np.isnan(clean[0]) | listed)
    for plan in PLANS:
        got = host(*kernel(CM, MT, sc["points"], normals, *lattice_of(sc), least=1, plan=plan))
        assert CR.same_bits(got[0], exp[0]) and CR.same_bits(got[1], clean[1])
        assert CR.same_bits(got[0][~listed], clean[0][~listed])


def test_lattices_outside_the_clouds_grid(CM, MT):
    """queries clamped to the grid's border cells: a lattice beside the cloud's box, within the radius of it on one side, and one
    wholly out of reach"""
    sc = S.scene("duplicates")
    hi = sc["points"].max(axis=0)
    beside = (float(hi[0]) + 0.25 * sc["voxel"], sc["origin"][1], sc["origin"][2])
    for origin, reach in ((beside, True), ((40.0, -50.0, 60.0), False), ((-1e30, 1e30, 0.0), False)):
        shape = (6, 17, 13)
        exp = CR.implicit(sc["points"], sc["normals"], shape, origin, sc["voxel"], sc["radius"], S.K, 1)
        assert np.isfinite(exp[0]).any() == reach
        for h in (None, 0.05):
            for plan in PLANS:
                assert same(kernel(CM, MT, sc["points"], sc["normals"], shape, origin, sc["voxel"], sc["radius"], least=1, cell_size=h, plan=plan), exp)


def test_reruns_and_graph_replay_repeat_the_bits(CM, MT):
    sc = S.scene("sphere")
    exp = S.expected("sphere")
    p, n = dev(sc["points"]), dev(sc["normals"])
    grid = MT.PointGrid(p)
    run = lambda: CM._implicit_device(p, n, grid, sc["shape"], sc["origin"], sc["voxel"], S.K, MT.squared_cutoff(sc["radius"]), S.MIN_NEIGHBORS)   # noqa: E731
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


# --------------------------------------------------------------------------------------------------------- the host side
def test_implicit_from_cloud_equals_the_kernel_on_the_filtered_cloud(CM, MT):
    sc = S.scene("duplicates")
    p, n = dev(sc["points"]), dev(sc["normals"])
    lo, hi = sc["points"].min(axis=0).astype(np.float64) - sc["radius"], sc["points"].max(axis=0).astype(np.float64) + sc["radius"]
    shape = tuple(max(2, int(np.ceil((h - l) / sc["voxel"])) + 1) for l, h in zip(lo, hi))
    exp = CR.implicit(sc["points"], sc["normals"], shape, lo, sc["voxel"], sc["radius"], S.K, S.MIN_NEIGHBORS)
    vol = CM.implicit_from_cloud(p, n, sc["voxel"])
    assert vol.shape == shape and vol.origin == tuple(lo) and vol.device == p.device and same((vol.value, vol.support), exp)
    grid = MT.PointGrid(p, cell_size=0.05)
    assert same(kernel(CM, MT, sc["points"], sc["normals"], shape, lo, sc["voxel"], sc["radius"], grid=grid), exp)
    again = CM.implicit_from_cloud(p, n.double(), sc["voxel"], grid=grid)               # a passed grid, normals of another float type
    assert same((again.value, again.support), exp)
    bad_p, bad_n = torch.cat([p[:5], p, p[:3]]), torch.cat([n[:5], n, n[:3]])
    bad_p[0, 0], bad_p[3, 2], bad_n[1, 1], bad_n[-1, 0], bad_n[-2, 2], bad_p[-3, 1] = (float("nan"), float("inf"), float("nan"), float("-inf"),
                                                                                   float("nan"), float("nan"))
    bad_p[2], bad_p[4] = p[0] + 10.0, p[0] - 10.0                                       # finite rows the filter keeps: far away
    bad_n[2], bad_n[4] = n[0], n[0]
    kept = torch.cat([bad_p[2:3], bad_p[4:5], p]), torch.cat([bad_n[2:3], bad_n[4:5], n])
    got = CM.implicit_from_cloud(bad_p, bad_n, sc["voxel"], bounds=(lo, hi), k=9, min_neighbors=2)
    ref = CM.implicit_from_cloud(kept[0], kept[1], sc["voxel"], bounds=(lo, hi), k=9, min_neighbors=2)
    exp9 = CR.implicit(host(kept[0])[0], host(kept[1])[0], shape, lo, sc["voxel"], sc["radius"], 9, 2)
    assert same((got.value, got.support), exp9) and same((ref.value, ref.support), exp9)
    # the torch form on the device: PointGrid.knn in chunks plus torch sums
    tv, ts = CM._implicit_torch(p, n, shape, lo, sc["voxel"], sc["radius"], S.K, S.MIN_NEIGHBORS, chunk=1000)
    assert same((tv, ts), exp)
    with pytest.raises(ValueError, match="the grid holds"):
        CM.implicit_from_cloud(p[:10], n[:10], sc["voxel"], grid=grid)


def restated_mesh(volume_np, support_np, min_support, origin, voxel):
    """the restated route: the restated volume -> mesh.marching_cubes -> the face filter in numpy"""
    from ls2fm import mesh
    vol = np.where(support_np >= np.float32(min_support), volume_np, np.float32(np.nan)).astype(np.float32)
    verts, faces = host(*mesh.marching_cubes(dev(vol), 0.0, spacing=(voxel,) * 3, origin=origin))
    good = np.isfinite(verts).all(axis=1)
    kept = faces[good[faces].all(axis=1)] if len(faces) else faces
    used = np.zeros(len(verts), bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    return verts[used], renumber[kept].astype(np.int32)


@pytest.mark.parametrize("name", ["sphere", "hemisphere", "cube", "few"])
def test_extract_and_mesh_from_cloud_against_the_restated_route(CM, name):
    sc = S.scene(name)
    exp = S.expected(name)
    lo = sc["origin"]
    hi = tuple(o + (s - 1) * sc["voxel"] for o, s in zip(lo, sc["shape"]))              # dyadic: volume_for's shape is the scene's
    for min_support in (0.0, 2.0):
        v, f = restated_mesh(exp[0], exp[1], min_support, lo, sc["voxel"])
        out, vol = CM.mesh_from_cloud(dev(sc["points"]), dev(sc["normals"]), voxel=sc["voxel"], bounds=(lo, hi), min_support=min_support,
                                      return_volume=True)
        assert vol.shape == sc["shape"] and same((vol.value, vol.support), exp)
        gv, gf = host(out.vertices, out.faces)
        assert gf.dtype == np.int32 and np.array_equal(gv.view(np.uint32), v.view(np.uint32)) and np.array_equal(gf, f)
        again = CM.extract(vol, min_support)
        assert torch.equal(again.vertices, out.vertices) and torch.equal(again.faces, out.faces)
        assert np.isfinite(gv).all() and (len(gf) > 1000 if name != "few" else len(gf) == 0)


def test_the_spheres_mesh_scores_below_a_voxel_and_goes_on_as_it_stands(CM, MT):
    from ls2fm import simplify
    sc = S.scene("sphere")
    out = CM.mesh_from_cloud(dev(sc["points"]), dev(sc["normals"]), voxel=sc["voxel"])
    gt = dev((S.SPHERE_CENTRE + S.SPHERE_RADIUS * S._fibonacci(40000)).astype(np.float32))
    score = MT.evaluate_mesh(out.vertices, out.faces, gt, 3 * sc["voxel"], 0.25 * sc["voxel"], generator=torch.Generator(device=DEV).manual_seed(5))
    print(f"sphere mesh: accuracy {score['accuracy'] / sc['voxel']:.4f} voxel, completeness {score['completeness'] / sc['voxel']:.4f} voxel")
    assert score["accuracy"] < sc["voxel"] and score["completeness"] < sc["voxel"]
    assert score["n_completeness"] == score["n_gt"] and score["n_accuracy"] == score["n_pred"]
    # outward normals give outward faces: a positive signed volume
    v, f = out.vertices.double(), out.faces.long()
    signed = (v[f[:, 0]] * torch.linalg.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0
    sphere = 4.0 / 3.0 * np.pi * S.SPHERE_RADIUS ** 3
    assert abs(float(signed) / sphere - 1.0) < 0.05
    small = simplify.simplify(out.vertices, out.faces, 2 * sc["voxel"])
    assert 0 < small.faces.shape[0] < out.faces.shape[0]


def test_estimated_normals_keep_the_sign_convention(CM):
    """mesh_from_cloud without normals: estimate_normals oriented toward a position outside each point (twice its offset from the
    centre) gives outward normals, so the value is negative inside the sphere and the faces look outward as with analytic normals"""
    sc = S.scene("sphere")
    p = dev(sc["points"])
    centre = dev(S.SPHERE_CENTRE.astype(np.float32))
    out, vol = CM.mesh_from_cloud(p, voxel=sc["voxel"], toward=centre + 2.0 * (p - centre), return_volume=True)
    X = CR.lattice_points(vol.shape, vol.origin, vol.voxel).astype(np.float64)
    value = host(vol.value)[0].reshape(-1)
    rho = np.linalg.norm(X - S.SPHERE_CENTRE, axis=1)
    inside, outside = np.isfinite(value) & (rho < S.SPHERE_RADIUS - sc["voxel"]), np.isfinite(value) & (rho > S.SPHERE_RADIUS + sc["voxel"])
    assert inside.sum() > 500 and outside.sum() > 500 and value[inside].mean() < 0 and (value[inside] < 0).all() and (value[outside] > 0).all()
    v, f = out.vertices.double(), out.faces.long()
    signed = (v[f[:, 0]] * torch.linalg.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0
    assert float(signed) > 0
    analytic = CM.mesh_from_cloud(p, dev(sc["normals"]), voxel=sc["voxel"])
    assert abs(out.faces.shape[0] / analytic.faces.shape[0] - 1.0) < 0.05
    inward = CM.mesh_from_cloud(p, voxel=sc["voxel"], toward=centre)                    # one position: inward normals, the sign turns
    v, f = inward.vertices.double(), inward.faces.long()
    assert float((v[f[:, 0]] * torch.linalg.cross(v[f[:, 1]], v[f[:, 2]])).sum()) < 0
    with pytest.raises(ValueError, match="toward is required"):
        CM.mesh_from_cloud(p, voxel=sc["voxel"])
