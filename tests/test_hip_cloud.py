"""GPU: ls2fm.cloud and metrics.PointGrid.knn -- the k-nearest-neighbour kernel (csrc/point_grid.hip, pg_knn) and the normals kernel
(csrc/cloud_normals.hip) against the numpy restatement (tests/cloud_restate.py) on the scenes of tests/metrics_scenes.py and
tests/cloud_scenes.py, then the outlier filters, normal consistency and ICP on estimated normals on top of them.

The K-NEIGHBOUR RULE makes a result a pure function of the inputs: indices, counts and the BITS of d2 are compared exactly on every
query of every scene.  The covariance of the NORMAL RULE is compared by its bits; normals and curvature are held, on every query,
to what numpy.linalg.eigh leaves on the same matrices (cloud_scenes.check_normals states the bound).  tests/test_cloud_host.py
asserts the properties of the new scenes that the tests here lean on."""
import numpy as np
import pytest
import torch

import cloud_restate as R
import cloud_scenes as S
import metrics_scenes as MS
from test_hip_metrics import cell_sizes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def MT():
    from ls2fm import metrics
    return metrics


@pytest.fixture(scope="module")
def CL():
    from ls2fm import cloud
    return cloud


def dev(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def host(*tensors):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


# ------------------------------------------------------------------------------------------------------------------- k-NN
@pytest.mark.parametrize("name", MS.NAMES)
def test_knn_equals_restatement_at_three_cell_sizes_and_every_capacity(MT, name):
    sc = MS.scenes()[name]
    ref, q = dev(sc["ref"]), dev(sc["q"])
    full = S.expected_knn(name)
    for h in cell_sizes(MT, sc):
        grid = MT.PointGrid(ref, cell_size=h)
        got = {k: host(*grid.knn(q, k, sc["max_dist"])) for k in S.KS}
        for k in S.KS:
            assert S.same_knn(got[k], S.prefix(full, k)), f"{name} at cell size {h}, k = {k}: {int((got[k][0] != full[0][:, :k]).sum())} indices differ"
        # the capacity does not show: 8 of capacity 8 are the first 8 of capacities 16 and 32
        for wide in (9, 32):
            assert np.array_equal(got[8][0], got[wide][0][:, :8]) and np.array_equal(got[8][1].view(np.uint32), got[wide][1][:, :8].view(np.uint32))
        # k = 1 is the nearest-neighbour query, by its bits
        idx, d2 = host(*grid.query(q, sc["max_dist"]))
        assert np.array_equal(got[1][0][:, 0], idx) and np.array_equal(got[1][1][:, 0].view(np.uint32), d2.view(np.uint32))
        assert np.array_equal(got[1][2], (idx >= 0).astype(np.int32))


def test_knn_small_clouds_and_launch_edges(MT, CL):
    sc = MS.scenes()["surface"]
    q = dev(sc["q"])
    for n in (0, 1, 3):                                                               # padding and counts
        got = host(*MT.PointGrid(dev(sc["ref"][:n])).knn(q[:300], 8))
        assert S.same_knn(got, R.knn(sc["q"][:300], sc["ref"][:n], 8)) and (got[2] == n).all() and (got[0][:, n:] == -1).all()
    grid = MT.PointGrid(dev(sc["ref"]))
    full = S.expected_knn("surface")
    for m in (1, 255, 256, 257):                                                      # both sides of a workgroup
        assert S.same_knn(host(*grid.knn(q[:m], 8)), tuple(x[:m] for x in S.prefix(full, 8)))
    assert S.same_knn(host(*CL.knn(q, dev(sc["ref"]), 16)), S.prefix(full, 16))       # the module's entry point
    assert S.same_knn(host(*CL.knn(q, grid, 16)), S.prefix(full, 16))
    idx, d2, count = grid.knn(q[:0], 8)
    assert idx.shape == (0, 8) and d2.shape == (0, 8) and count.shape == (0,)
    with pytest.raises(ValueError, match="k "):
        grid.knn(q, 33)
    with pytest.raises(ValueError, match="skip_own"):
        grid.knn(q[:5], 8, skip_own=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.knn(q.cpu(), 8)


@pytest.mark.parametrize("scene,max_dist", [("duplicates", None), ("loner", S.LONER_MAX_DIST)])
def test_knn_skip_own(MT, CL, scene, max_dist):
    """duplicates: a point's twin at another index stays its neighbour at d2 = 0; loner: a point whose only neighbours lie beyond
    max_dist comes back empty"""
    p = getattr(S, scene)()
    t = dev(p)
    for h in (None, 0.05):
        grid = MT.PointGrid(t, cell_size=h)
        for k in (1, 8, 17):
            exp = R.knn(p, p, k, max_dist, skip_own=True)
            assert S.same_knn(host(*grid.knn(t, k, max_dist, skip_own=True)), exp), f"{scene}, h = {h}, k = {k}"
    assert S.same_knn(host(*CL.knn(t, t, 8, max_dist, exclude_self=True)), R.knn(p, p, 8, max_dist, skip_own=True))
    with pytest.raises(ValueError, match="q is ref"):
        CL.knn(t.clone(), t, 8, exclude_self=True)


@pytest.mark.parametrize("name", ["ties", "cutoff", "nonfinite", "surface"])
def test_knn_batching_order_reruns_and_graph_replay_do_not_show(MT, name):
    sc = MS.scenes()[name]
    ref, q = dev(sc["ref"]), dev(sc["q"])
    grid = MT.PointGrid(ref, cell_size=sc["cell_size"])
    for k in (8, 17):
        exp = S.prefix(S.expected_knn(name), k)
        for sort in (False, True):
            assert S.same_knn(host(*grid.knn(q, k, sc["max_dist"], sort=sort)), exp)
            half = len(sc["q"]) // 2
            a, b = grid.knn(q[:half], k, sc["max_dist"], sort=sort), grid.knn(q[half:], k, sc["max_dist"], sort=sort)
            assert S.same_knn(host(*(torch.cat([x, y]) for x, y in zip(a, b))), exp)
        perm = torch.randperm(len(sc["q"]), generator=torch.Generator().manual_seed(3)).to(DEV)
        r = grid.knn(q[perm], k, sc["max_dist"])
        assert S.same_knn(host(*(torch.empty_like(x).index_copy_(0, perm, x) for x in r)), exp)
        assert S.same_knn(host(*MT.PointGrid(ref, cell_size=sc["cell_size"]).knn(q, k, sc["max_dist"])), exp)      # a second build, a rerun
    k, exp = 8, S.prefix(S.expected_knn(name), 8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        grid.knn(q, k, sc["max_dist"])                                                # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = grid.knn(q, k, sc["max_dist"])
    for _ in range(2):
        out[0].fill_(-7)
        out[1].fill_(-1.0)
        out[2].fill_(-7)
        graph.replay()
        assert S.same_knn(host(*out), exp)


# ---------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("name", MS.NAMES)
def test_normals_on_every_query_of_the_grid_scenes(MT, CL, name):
    """the scene's queries against its references at k = 16 (n = 0 .. 16 neighbours; collinear, coplanar and identical clouds
    among them): the covariance by its bits, the NaN pattern exactly, the eigenvector to eigh's own residual"""
    sc = MS.scenes()[name]
    ref, q = dev(sc["ref"]), dev(sc["q"])
    idx, _, count = MT.PointGrid(ref, cell_size=sc["cell_size"]).knn(q, S.K_NORMALS, sc["max_dist"])
    exp = S.prefix(S.expected_knn(name), S.K_NORMALS)
    assert np.array_equal(host(idx)[0], exp[0]) and np.array_equal(host(count)[0], exp[2])
    normal, curvature, cov = host(*CL.normals_from_neighbors(ref, idx, return_cov=True))
    S.check_normals(sc["ref"], exp[0], normal, curvature, cov)
    for n_few in (1, 2, 3):                                                           # lists of n = 1, 2, 3 entries
        few = idx[:, :n_few].contiguous()
        normal, curvature, cov = host(*CL.normals_from_neighbors(ref, few, return_cov=True))
        S.check_normals(sc["ref"], exp[0][:, :n_few], normal, curvature, cov)
        assert n_few == 3 or (np.isnan(normal).all() and np.isnan(curvature).all())


@pytest.mark.parametrize("name", ["plane", "sphere"])
def test_normals_of_the_two_surfaces(CL, name):
    """Every point of the scene, none left out.  Measured on the CPU (tests/test_cloud_host.py asserts the first): the eigen-gap
    (lambda_1 - lambda_0) / trace is at least 0.155 on the plane and 0.302 on the sphere; the restatement's two routes (Jacobi,
    eigh) differ by at most 6.0e-16 rad on the plane and 1.5e-15 rad on the sphere.  The device's normal is held to the Jacobi
    route within 4 x that angle (floor 2^-50 rad), the plane's normals to 2 degrees of the plane's axis (the restatement's worst:
    0.33), the sphere's to 10 degrees of the radius (2.18), and with toward = the centre they all point inward."""
    sc = {"plane": S.plane, "sphere": S.sphere}[name]()
    e = S.normals_expected(name)
    p = dev(sc["points"])
    idx, _, _ = CL.knn(p, p, S.K_NORMALS)
    assert np.array_equal(host(idx)[0], e["idx"])
    normal, curvature, cov = host(*CL.normals_from_neighbors(p, idx, return_cov=True))
    nj, _ = S.check_normals(sc["points"], e["idx"], normal, curvature, cov)
    worst = R.angle(normal, nj).max()
    print(f"{name}: device against the Jacobi route {worst:.3e} rad, the two routes {e['angle'].max():.3e} rad, gap {e['gap'].min():.3e}")
    assert worst <= max(4.0 * e["angle"].max(), 2.0 ** -50) and ((normal * nj).sum(axis=1) > 0).all()
    n64, c64 = CL.estimate_normals(p, S.K_NORMALS, return_curvature=True, dtype=torch.float64)
    assert np.array_equal(host(n64)[0], normal) and np.array_equal(host(c64)[0], curvature)
    n32, c32 = CL.estimate_normals(p, S.K_NORMALS, return_curvature=True)                 # float32: the rounding of the float64 result
    assert n32.dtype == torch.float32 and torch.equal(n32, n64.float()) and torch.equal(c32, c64.float())
    if name == "plane":
        assert np.degrees(R.angle(normal, sc["axis"][None, :])).max() < 2.0
    else:
        radial = sc["points"].astype(np.float64) - sc["centre"]
        assert np.degrees(R.angle(normal, radial)).max() < 10.0
        inward = host(CL.estimate_normals(p, S.K_NORMALS, toward=dev(sc["centre"].astype(np.float32)), dtype=torch.float64))[0]
        assert ((inward * radial).sum(axis=1) < 0).all() and np.array_equal(np.abs(inward), np.abs(normal))


def test_orientation(CL):
    p = dev(S.flat("z"))
    m = len(p)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=DEV)
    in_plane = torch.tensor([[9.0, -3.0, 0.5]], device=DEV)                           # toward - query has z = 0 exactly: the sign stays
    for toward in (in_plane, in_plane[0], in_plane.expand(m, 3)):
        assert bool((CL.estimate_normals(p, S.K_NORMALS, toward=toward, dtype=torch.float64) == up).all())
    each = torch.cat([p[:, :2], torch.zeros(m, 1, device=DEV)], dim=1)
    each[::2, 2] = 1.0                                                               # one position per point, alternately above and below
    n = CL.estimate_normals(p, S.K_NORMALS, toward=each, dtype=torch.float64)
    assert bool((n[::2] == up).all()) and bool((n[1::2] == -up).all())
    assert bool((CL.estimate_normals(p, S.K_NORMALS, toward=torch.tensor([[0.0, 0.0, -4.0]], device=DEV), dtype=torch.float64) == -up).all())
    for kind in ("diag_plus", "diag_minus"):                                          # two components of equal magnitude: the lower axis decides
        q = S.flat(kind)
        n = host(CL.estimate_normals(dev(q), S.K_NORMALS, dtype=torch.float64))[0]
        exp = R.normals(q, R.knn(q, q, S.K_NORMALS)[0])[0]
        assert (n[:, 0] > 0).all() and (np.abs(n[:, 0]) == np.abs(n[:, 1])).all() and (np.sign(n[:, 1]) == (1 if kind == "diag_plus" else -1)).all()
        assert np.abs(n - exp).max() <= 2.0 ** -50


def test_normals_chunks_rerun_and_graph_replay_repeat_the_bits(MT, CL):
    sc = S.sphere()
    p = dev(sc["points"])
    grid = MT.PointGrid(p)
    toward = dev(sc["centre"].astype(np.float32))

    def run(points_slice):
        idx, _, _ = grid.knn(points_slice, S.K_NORMALS)
        return CL.normals_from_neighbors(p, idx, points_slice, toward, return_cov=True)

    whole = host(*run(p))
    bits = lambda xs: [x.view(np.uint64) for x in xs]                                 # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))   # noqa: E731
    a, b = run(p[:777]), run(p[777:])
    assert same(host(*(torch.cat([x, y]) for x, y in zip(a, b))), whole)
    assert same(host(*run(p)), whole)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(p)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(p)
    for _ in range(2):
        for x in out:
            x.fill_(7.0)
        graph.replay()
        assert same(host(*out), whole)


# ------------------------------------------------------------------------------------------------- filters and consistency
def test_outlier_filters(CL):
    """the straggler scene: a dense patch and 20 planted points.  No point's mean distance lies within 1e-6 relative of the
    threshold mu + 2 sigma (the nearest is 0.57 of it away: tests/test_cloud_host.py asserts it), so the mask is the restatement's."""
    p = S.stragglers()
    t = dev(p)
    keep, mean = CL.statistical_outliers(t, S.STAT_K, S.STAT_RATIO)
    exp_keep, exp_mean, _ = R.statistical_outliers(p, S.STAT_K, S.STAT_RATIO)
    _, terms = R.mean_distances(p, S.STAT_K)
    keep, mean = host(keep, mean)
    assert keep.dtype == np.bool_ and mean.dtype == np.float64
    assert (np.abs(mean - exp_mean) <= (S.STAT_K + 16) * 2.0 ** -53 * terms).all()
    assert np.array_equal(keep, exp_keep) and keep[:-S.N_STRAGGLERS].all() and not keep[-S.N_STRAGGLERS:].any()
    for radius, least in ((0.03, 4), (0.07, 32), (0.021, 1)):
        got = host(CL.radius_outliers(t, radius, least))[0]
        exp = R.radius_outliers(p, radius, least)
        assert np.array_equal(got, exp) and 0 < exp.sum() < len(exp)
    lone = dev(S.loner())
    assert np.array_equal(host(CL.radius_outliers(lone, S.LONER_MAX_DIST, 1))[0], R.radius_outliers(S.loner(), S.LONER_MAX_DIST, 1))
    keep, mean = CL.statistical_outliers(lone[7:8], 5)
    assert not bool(keep[0]) and bool(torch.isnan(mean[0]))


def test_normal_consistency(MT, CL):
    p, n = S.cube()
    out = MT.normal_consistency(dev(p), dev(n), dev(p), dev(n), 0.1)
    assert out["accuracy"] == 1.0 and out["completeness"] == 1.0 and out["overall"] == 1.0
    assert out["n_accuracy"] == out["n_completeness"] == len(p)
    sc = MS.scenes()["surface"]
    pred, gt = sc["q"], sc["ref"]
    pn, gn = (host(CL.estimate_normals(dev(x), S.K_NORMALS))[0] for x in (pred, gt))
    got = MT.normal_consistency(dev(pred), dev(pn), dev(gt), dev(gn), MS.SURFACE_MAX_DIST)
    exp = R.normal_consistency(pred, pn, gt, gn, MS.SURFACE_MAX_DIST)
    assert got["n_accuracy"] == exp["n_accuracy"] < len(pred) and got["n_completeness"] == exp["n_completeness"]
    for key, m in (("accuracy", len(pred)), ("completeness", len(gt)), ("overall", len(pred))):
        assert abs(got[key] - exp[key]) <= (m + 2) * 2.0 ** -53 * exp[key]               # an fp64 sum of m terms in any order
    assert 0.9 < got["overall"] <= 1.0


def test_icp_on_estimated_normals(MT, CL):
    """the sphere scene as the fixed cloud, a copy moved by a small rigid offset (1.5 degrees, 0.014) as the moving one, 50
    iterations within max_dist 0.2.  Point to plane slides on a sphere (a rotation about the centre leaves the residual nearly
    unchanged), so the analytic-normal run itself ends 6.5e-5 (largest entry of R and t) from the point-to-point run, which finds
    the offset to 2e-10; four times that difference is the margin the run on estimated normals is held to, against the analytic
    run and against the true offset.  Measured on the device: analytic against estimated 6.5e-5, estimated against the truth
    4.1e-8 (the torch form on the CPU: 4.4e-5, 4.4e-5 and 6.0e-8)."""
    sc = S.sphere()
    pts = sc["points"].astype(np.float64)
    radial = pts - sc["centre"]
    analytic = (radial / np.linalg.norm(radial, axis=1, keepdims=True)).astype(np.float32)
    w = np.array([0.01, -0.02, 0.015])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Rm = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    t = np.array([0.01, 0.005, -0.008])
    src, dst = dev(((pts - t) @ Rm).astype(np.float32)), dev(sc["points"])              # dst = R src + t
    grid = MT.PointGrid(dst)
    estimated = CL.estimate_normals(dst, S.K_NORMALS, grid=grid)

    def run(normals):
        r = MT.icp(src, grid, dst_normals=normals, max_dist=0.2)
        return np.concatenate([r.R.cpu().numpy().reshape(-1), r.t.cpu().numpy()]), r

    truth = np.concatenate([Rm.reshape(-1), t])
    point, plane, est = run(None), run(dev(analytic)), run(estimated)
    margin = 4.0 * np.abs(point[0] - plane[0]).max()
    print(f"point to point against plane {margin / 4:.3e}, analytic against estimated {np.abs(plane[0] - est[0]).max():.3e}, "
          f"estimated against the truth {np.abs(est[0] - truth).max():.3e}")
    assert np.abs(point[0] - truth).max() < 1e-6 and point[1].status == MT.ICP_CONVERGED
    assert np.abs(plane[0] - est[0]).max() <= margin and np.abs(est[0] - truth).max() <= margin
    assert est[1].n_pairs == len(pts) and est[1].rmse < 1e-6
