"""GPU: ls2fm.metrics -- the point grid (csrc/point_grid.hip) against the numpy restatement (tests/metrics_restate.py) on the scenes
of tests/metrics_scenes.py, and Chamfer, evaluate_mesh and the mapper's pose errors on top of it.

The distance rule makes a nearest-neighbour result a pure function of the inputs, so the index and the BITS of d2 are compared
exactly, on every query of every scene, no query excluded; tests/test_metrics_host.py asserts that the scenes hold the cases a
wrong kernel fails.  Chamfer counts are exact and its means are held to (M + 2) 2^-53 relative: the bound of an fp64 sum of M
non-negative terms in any order plus one rounding of each square root."""
import numpy as np
import pytest
import torch

import metrics_restate as R
import metrics_scenes as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def MT():
    from ls2fm import metrics
    return metrics


def dev(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def host(idx, d2):
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy().view(np.uint32)


def want(name):
    idx, d2 = S.expected(name)
    return idx, d2.view(np.uint32)


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def cell_sizes(MT, sc):
    """a size that makes a single cell, the scene's own (the automatic one where it names none) and a quarter of it"""
    lo, hi = sc["ref"].min(axis=0), sc["ref"].max(axis=0)
    own = sc["cell_size"] if sc["cell_size"] is not None else MT.auto_cell_size(lo, hi, len(sc["ref"]))
    return 4.0 * max(float((hi - lo).max()), 1.0), own, own / 4


@pytest.mark.parametrize("name", S.NAMES)
def test_grid_equals_restatement_at_three_cell_sizes(MT, name):
    sc = S.scenes()[name]
    ref, q = dev(sc["ref"]), dev(sc["q"])
    exp = want(name)
    for i, h in enumerate(cell_sizes(MT, sc)):
        grid = MT.PointGrid(ref, cell_size=h)
        assert grid.n_cells == 1 or i > 0
        got = host(*grid.query(q, sc["max_dist"]))
        assert got[0].dtype == np.int32 and same(got, exp), f"{name} at cell size {h}: {int((got[0] != exp[0]).sum())} indices differ"
        # the grid itself: every reference once, in cell order
        assert int(grid.cell_start[-1]) == len(sc["ref"]) and bool((grid.cell_start[1:] >= grid.cell_start[:-1]).all())
        assert torch.equal(torch.sort(grid.sorted_index.long()).values, torch.arange(len(sc["ref"]), device=DEV))
        assert torch.equal(grid.sorted_xyz, ref[grid.sorted_index.long()])
    # the scene's own entry point, and the automatic cell size
    assert same(host(*MT.nearest_neighbors(q, ref, sc["max_dist"], cell_size=sc["cell_size"])), exp)
    assert same(host(*MT.nearest_neighbors(q, ref, sc["max_dist"])), exp)


@pytest.mark.parametrize("name", ["faces", "ties", "cutoff", "nonfinite", "surface"])
def test_batching_order_and_reruns_do_not_show(MT, name):
    sc = S.scenes()[name]
    ref, q = dev(sc["ref"]), dev(sc["q"])
    exp = want(name)
    grid = MT.PointGrid(ref, cell_size=sc["cell_size"])
    for sort in (False, True):
        assert same(host(*grid.query(q, sc["max_dist"], sort=sort)), exp)
        half = len(sc["q"]) // 2
        a, b = grid.query(q[:half], sc["max_dist"], sort=sort), grid.query(q[half:], sc["max_dist"], sort=sort)
        assert same(host(torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])), exp)
        r = grid.query(q.flip(0), sc["max_dist"], sort=sort)
        assert same(host(r[0].flip(0), r[1].flip(0)), exp)
    again = MT.PointGrid(ref, cell_size=sc["cell_size"])                       # a second build, a second query
    assert same(host(*again.query(q, sc["max_dist"])), exp)
    assert torch.equal(again.cell_start, grid.cell_start)


def test_nonfinite_queries_leave_the_finite_ones_alone(MT):
    sc = S.scenes()["nonfinite"]
    grid = MT.PointGrid(dev(sc["ref"]), cell_size=sc["cell_size"])
    finite = np.isfinite(sc["q"]).all(axis=1)
    mixed = host(*grid.query(dev(sc["q"])))
    alone = host(*grid.query(dev(sc["q"][finite])))
    assert np.array_equal(mixed[0][finite], alone[0]) and np.array_equal(mixed[1][finite], alone[1])
    assert (mixed[0][~finite] == -1).all() and (mixed[1][~finite] == np.float32(np.inf).view(np.uint32)).all()


def test_empty_sides_and_refusals(MT):
    ref = dev(S.scenes()["cutoff"]["ref"])
    idx, d2 = MT.PointGrid(ref).query(torch.zeros(0, 3, device=DEV))
    assert idx.numel() == 0 and d2.numel() == 0
    idx, d2 = MT.PointGrid(torch.zeros(0, 3, device=DEV)).query(ref[:7])
    torch.cuda.synchronize()
    assert idx.tolist() == [-1] * 7 and bool(torch.isinf(d2).all())
    with pytest.raises(ValueError, match="max_cells"):
        MT.PointGrid(ref, cell_size=1e-4)
    with pytest.raises(ValueError, match="NaN or infinite"):
        MT.PointGrid(torch.cat([ref, torch.full((1, 3), float("nan"), device=DEV)]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.PointGrid(ref).query(ref.cpu())
    with pytest.raises(ValueError, match="max_dist"):
        MT.PointGrid(ref).query(ref, max_dist=-1.0)


def test_captured_query_replays_to_the_eager_result(MT):
    sc = S.scenes()["cutoff"]
    grid = MT.PointGrid(dev(sc["ref"]), cell_size=sc["cell_size"])
    q = dev(sc["q"]).clone()
    exp = want("cutoff")
    eager = host(*grid.query(q, sc["max_dist"]))
    assert same(eager, exp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        grid.query(q, sc["max_dist"])                                          # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, d2 = grid.query(q, sc["max_dist"])
    for _ in range(2):
        idx.fill_(-7)
        d2.fill_(-1.0)
        graph.replay()
        assert same(host(idx, d2), eager)


def mean_bound(m):
    return (m + 2) * 2.0 ** -53


def check_chamfer(got, exp, m_pred, m_gt):
    assert got["n_accuracy"] == exp["n_accuracy"] and got["n_completeness"] == exp["n_completeness"]
    assert abs(got["accuracy"] - exp["accuracy"]) <= mean_bound(m_pred) * exp["accuracy"]
    assert abs(got["completeness"] - exp["completeness"]) <= mean_bound(m_gt) * exp["completeness"]
    assert abs(got["overall"] - exp["overall"]) <= mean_bound(max(m_pred, m_gt)) * exp["overall"]
    assert got["precision"] == exp["precision"] and got["recall"] == exp["recall"]                 # ratios of exact counts
    for a, b in zip(got["fscore"], exp["fscore"]):
        assert abs(a - b) <= 4 * 2.0 ** -53 * b


def test_chamfer_on_the_surface_scene(MT):
    sc = S.scenes()["surface"]
    pred, gt = sc["q"], sc["ref"]
    exp = R.chamfer(pred, gt, S.SURFACE_MAX_DIST, S.SURFACE_THRESHOLDS)
    got = MT.chamfer(dev(pred), dev(gt), S.SURFACE_MAX_DIST, S.SURFACE_THRESHOLDS)
    check_chamfer(got, exp, len(pred), len(gt))
    brute = MT.chamfer(dev(pred), dev(gt), S.SURFACE_MAX_DIST, S.SURFACE_THRESHOLDS, brute_force=True)
    assert brute["n_accuracy"] == got["n_accuracy"] and brute["n_completeness"] == got["n_completeness"]
    assert brute["precision"] == got["precision"] and brute["recall"] == got["recall"]
    check_chamfer(brute, exp, len(pred), len(gt))
    empty = MT.chamfer(torch.zeros(0, 3, device=DEV), dev(gt), S.SURFACE_MAX_DIST)
    assert empty["n_accuracy"] == 0 and empty["n_completeness"] == 0 and np.isnan(empty["accuracy"]) and np.isnan(empty["completeness"])


def test_evaluate_mesh_on_a_marching_cubes_sphere(MT):
    """a sphere of radius 0.6 from a 32^3 volume, against ground truth on a sphere of radius 0.61: the metric is restated in numpy on
    the very points the device sampled and kept, so the bound is the Chamfer bound -- no analytic tolerance"""
    from ls2fm import mesh
    g = torch.linspace(-1.0, 1.0, 32, device=DEV)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    verts, faces = mesh.marching_cubes((x * x + y * y + z * z).sqrt() - 0.6, 0.0, spacing=(2 / 31,) * 3, origin=(-1.0,) * 3)
    gt = S._sphere(np.random.default_rng(3), 4000, 0.61)
    gen = torch.Generator(device=DEV).manual_seed(5)
    density, max_dist, thresholds = 0.06, 0.1, (0.03, 0.05)
    out = MT.evaluate_mesh(verts, faces, dev(gt), max_dist, density, thresholds, generator=gen, return_points=True)
    pred_pts, gt_pts = out["pred_points"].cpu().numpy(), out["gt_points"].cpu().numpy()
    area = 4 * np.pi * 0.6 ** 2
    assert out["n_pred"] == len(pred_pts) and out["n_gt"] == len(gt_pts) and 0.3 * area / density ** 2 < out["n_pred"] < area / density ** 2
    assert np.array_equal(gt_pts, gt[R.voxel_downsample(gt, density)])
    assert len(R.voxel_downsample(pred_pts, density)) == len(pred_pts)                              # one point per voxel is left
    exp = R.chamfer(pred_pts, gt_pts, max_dist, thresholds)
    check_chamfer(out, exp, len(pred_pts), len(gt_pts))
    assert 0.005 < out["overall"] < 0.05 and out["n_accuracy"] == out["n_pred"]
    gen.manual_seed(5)
    again = MT.evaluate_mesh(verts, faces, dev(gt), max_dist, density, thresholds, generator=gen)
    assert again["overall"] == out["overall"] and again["n_pred"] == out["n_pred"]


def test_reconstruction_pose_errors_on_the_ring_scene():
    """the mapper's 8-view ring (tests/mapper_scenes.py): finite errors that agree with the restatement run on the same poses, to
    4 x the gap between the restatement's two alignment routes on them (floored at 1e-12 degrees / units)"""
    import mapper_scenes as MS
    import tracks_scenes as TS
    from ls2fm import mapper
    sc = MS.ring_scene()
    rec = mapper.reconstruct(sc["tables"], TS.K, MS.H, MS.W, mapper.MapperOptions(local_ba_iters=100, global_ba_iters=300, **TS.ba_rates()))
    out = rec.pose_errors(dev(sc["poses"]))
    poses, reg = rec.poses.cpu().numpy(), np.asarray(rec.registered, bool)
    a = R.pose_errors(poses, sc["poses"], registered=reg, route=R.umeyama_svd)
    b = R.pose_errors(poses, sc["poses"], registered=reg, route=R.umeyama_horn)
    assert out["n_views"] == int(reg.sum()) == MS.RING_VIEWS and out["n_unregistered"] == 0
    rot, centre = out["rot_err_deg"].numpy(), out["centre_err"].numpy()
    assert np.isfinite(rot).all() and np.isfinite(centre).all() and np.isfinite([out["ate_rmse"], out["scale"]]).all()
    gap = max(np.abs(a["rot_err_deg"] - b["rot_err_deg"]).max(), np.abs(a["centre_err"] - b["centre_err"]).max(), 1e-12)
    print(f"ring: rot {rot.max():.4f} deg, centre {centre.max():.5f}, ate {out['ate_rmse']:.5f}, scale {out['scale']:.5f}; route gap {gap:.2e}")
    assert np.abs(rot - a["rot_err_deg"]).max() <= 4 * gap and np.abs(centre - a["centre_err"]).max() <= 4 * gap
    assert abs(out["ate_rmse"] - a["ate_rmse"]) <= 4 * gap
