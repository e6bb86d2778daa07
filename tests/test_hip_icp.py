"""GPU: ls2fm.metrics.icp (csrc/icp.hip) against the numpy restatement (tests/icp_restate.py) on the scenes of tests/icp_scenes.py;
tests/test_icp_host.py asserts that the scenes hold the cases a wrong kernel fails.  No source point is excluded from a comparison.

Single steps are re-synchronised: the device takes one iteration from the restatement's transform T_k, so nothing carries over.
  pairs   index and the BITS of d2 equal on every source point, the count exact: p' and the walk are fixed sequences of operations
  sums    each of the 36 within (n_pairs + 16) 2^-53 sum |term| of the same terms added by numpy in ITS order: an fp64 sum of
          n_pairs terms in any order, plus slack for a differently associated term; sum |term| is the restatement's.  And equal,
          bit for bit, to the restatement's sums in the order the header states (lane, butterfly, waves, rows)
  update  (s, R, t) against the restatement's own update from its own sums, within max(4 x the gap between its two solve routes,
          7 kappa(H) 2^-52 |delta|), the textbook forward bound of a backward-stable solve, in 2-norms; kappa and delta are the
          restatement's.  That bound covers the solve alone -- seven roundings, where two orders of summation differ by up to
          n_pairs -- so it can hold only because the restatement adds in the stated order: with its sums in numpy's order the
          device's update was 2.3e-16 off under 1.2e-16 (similarity, step 5) and 2.8e-15 off under 2.8e-16 (262145 pairs, step 0).
Whole runs follow the same rule at their end: max(4 x the gap between the two routes' finals, 7 kappa 2^-52 |delta| of the last
step).  Status and iteration count are equal."""
import numpy as np
import pytest
import torch

import icp_restate as IR
import icp_scenes as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def MT():
    from ls2fm import metrics
    return metrics


def dev(a):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(DEV)


def state_of(T, MT):
    st = np.zeros(24)
    st[:13] = IR.flat(T)
    return torch.as_tensor(st).to(DEV)


class Device:
    """a scene on the device: the grid is built once"""

    def __init__(self, MT, name):
        self.MT, self.sc = MT, S.scenes()[name]
        self.src, self.normals = dev(self.sc["src"]), dev(self.sc["normals"])
        self.grid = MT.PointGrid(dev(self.sc["dst"]))
        self.m = len(self.sc["src"])

    def raw(self, state, iters, pairs=False, sums=False):
        """ls2fm_icp_run on `state` in place -> (pair_idx, pair_d2, sums) as asked"""
        from ls2fm import _lib
        lib, g, sc = _lib.load(), self.grid, self.sc
        ws = _lib.workspace(lib.ls2fm_icp_workspace_bytes(self.m), "ls2fm_icp_workspace_bytes", DEV)
        idx = torch.full((self.m,), -7, dtype=torch.int32, device=DEV) if pairs else None
        d2 = torch.full((self.m,), -1.0, dtype=torch.float32, device=DEV) if pairs else None
        out = torch.full((36,), float("nan"), dtype=torch.float64, device=DEV) if sums else None
        _lib.check(lib.ls2fm_icp_run(_lib.ptr(self.src), self.m, *g.c_args(), _lib.ptr(self.normals),
                                     float(self.MT.squared_cutoff(sc["max_dist"])),
                                     1 if sc["with_scale"] else 0, iters, sc["tol_rot"], sc["tol_trans"], _lib.ptr(state), _lib.ptr(out),
                                     _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(ws), _lib.stream_ptr()), "ls2fm_icp_run")
        return idx, d2, out

    def icp(self, **kw):
        sc = self.sc
        opts = dict(dst_normals=self.normals, max_dist=sc["max_dist"], with_scale=sc["with_scale"], iters=sc["iters"], tol_rot=sc["tol_rot"],
                    tol_trans=sc["tol_trans"])
        opts.update(kw)
        return self.MT.icp(self.src, self.grid, **opts)


def solve_bound(st):
    """7 kappa(H) 2^-52 |delta| of a restated step"""
    return 7 * st["kappa"] * 2.0 ** -52 * np.linalg.norm(st["delta"]["chol"])


def update_bound(st):
    """the tolerance of one step's updated transform, from the restatement's step"""
    gap = np.linalg.norm(IR.flat(st["T_new"]["chol"]) - IR.flat(st["T_new"]["numpy"]))
    return max(4 * gap, solve_bound(st))


@pytest.mark.parametrize("name", S.NAMES)
def test_single_steps_from_the_restatements_transforms(MT, name):
    d = Device(MT, name)
    steps = S.restated(name)["steps"][:S.SINGLE_STEPS]
    T = d.sc["init"]
    for k, st in enumerate(steps):
        # iters = 0: pairs and sums at T_k, the transform, the iteration count and the status untouched
        state = state_of(T, MT)
        before = state.clone()
        idx, d2, sums = d.raw(state, 0, pairs=True, sums=True)
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), st["pair_idx"]), f"{name} step {k}: {int((idx.cpu().numpy() != st['pair_idx']).sum())} pairs differ"
        assert np.array_equal(d2.cpu().numpy().view(np.uint32), st["pair_d2"].view(np.uint32)), f"{name} step {k}: d2 bits differ"
        got = state.cpu().numpy()
        assert np.array_equal(got[:13], before.cpu().numpy()[:13]) and got[15] == 0 and got[16] == 0 and not got[17:].any()
        assert got[14] == st["n_pairs"]
        sums = sums.cpu().numpy()
        bound = (st["n_pairs"] + 16) * 2.0 ** -53 * st["abs_sums"]
        err = np.abs(sums - st["plain_sums"])
        print(f"{name} step {k}: pairs {st['n_pairs']}, worst sum error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
              f"{int((sums != st['sums']).sum())} sums differ from the stated order's")
        assert (err <= bound).all(), f"{name} step {k}: sums {np.nonzero(err > bound)[0].tolist()} off by {err[err > bound]} (bound {bound[err > bound]})"
        assert np.array_equal(sums, st["sums"]), f"{name} step {k}: sums {np.nonzero(sums != st['sums'])[0].tolist()} are not the stated order's"
        assert got[13] == sums[35]
        # iters = 1 from the same T_k
        state = state_of(T, MT)
        d.raw(state, 1)
        got = state.cpu().numpy()
        assert got[16] == st["status"]["chol"] and got[15] == (0 if st["status"]["chol"] == IR.DEGENERATE else 1) and got[14] == st["n_pairs"]
        assert got[13] == sums[35]                                             # the same accumulate again: the same bits
        if st["status"]["chol"] == IR.DEGENERATE:
            assert np.array_equal(got[:13].view(np.uint64), IR.flat(T).view(np.uint64)), f"{name} step {k}: a degenerate step moved the transform"
            break
        diff, bound = np.linalg.norm(got[:13] - IR.flat(st["T_new"]["chol"])), update_bound(st)
        print(f"{name} step {k}: |delta| {np.linalg.norm(st['delta']['chol']):.2e}, kappa {st['kappa']:.1f}, update differs by {diff:.2e} "
              f"(bound {bound:.2e})")
        assert diff <= bound, f"{name} step {k}: the updated transform differs by {diff:.3e}, bound {bound:.3e}"
        T = st["T_new"]["chol"]


@pytest.mark.parametrize("name", S.WHOLE_RUNS)
def test_whole_runs_end_where_the_restatement_ends(MT, name):
    d = Device(MT, name)
    a, b = S.restated(name), S.restated(name, "numpy")
    res = d.icp(return_pairs=True)
    got = res.state.cpu().numpy()
    gap = np.linalg.norm(IR.flat(a["T"]) - IR.flat(b["T"]))
    bound = max(4 * gap, solve_bound(a["steps"][-1]))
    diff = np.linalg.norm(got[:13] - IR.flat(a["T"]))
    print(f"{name}: {res.iterations} iterations, status {res.status}, rmse {res.rmse:.3e}; final differs by {diff:.2e} (bound {bound:.2e}, gap {gap:.2e})")
    assert res.status == a["status"] == IR.CONVERGED and res.iterations == a["iterations"]
    assert diff <= bound
    # the closing evaluation belongs to the returned transform
    end = IR.accumulate(d.sc["src"], d.sc["dst"], d.sc["normals"], (got[0], got[1:10].reshape(3, 3), got[10:13]), d.sc["max_dist"])
    assert res.n_pairs == end["n_pairs"] and np.array_equal(res.pair_idx.cpu().numpy(), end["pair_idx"])
    assert np.array_equal(res.pair_d2.cpu().numpy().view(np.uint32), end["pair_d2"].view(np.uint32))
    assert abs(res.rmse - np.sqrt(end["sums"][35] / end["n_pairs"])) <= (end["n_pairs"] + 16) * 2.0 ** -53 * res.rmse
    # and the known transform is recovered to what the fp32 clouds allow
    assert np.abs(got[:13] - IR.flat(d.sc["truth"])).max() < 1e-6
    moved = res.apply(d.src).cpu().numpy()
    assert np.abs(moved - d.sc["dst"][d.sc["pick"]]).max() < 1e-6


def bits(t):
    return t.cpu().numpy().view(np.uint64 if t.dtype == torch.float64 else np.uint32)


@pytest.mark.parametrize("name", ["similarity", "plane", "partial"])
def test_two_runs_agree_bit_for_bit(MT, name):
    d = Device(MT, name)
    a, b = d.icp(return_pairs=True), d.icp(return_pairs=True)
    assert np.array_equal(bits(a.state), bits(b.state)) and np.array_equal(bits(a.evaluation), bits(b.evaluation))
    assert torch.equal(a.pair_idx, b.pair_idx) and np.array_equal(bits(a.pair_d2), bits(b.pair_d2))
    again = Device(MT, name).icp(return_pairs=True)                          # a second grid: the order inside its cells may differ
    assert np.array_equal(bits(a.state), bits(again.state)) and torch.equal(a.pair_idx, again.pair_idx)


@pytest.mark.parametrize("name,a,b", [("similarity", 3, 4), ("plane", 2, 2)])
def test_split_calls_continue_like_one_call(MT, name, a, b):
    d = Device(MT, name)
    whole = d.icp(iters=a + b)
    first = d.icp(iters=a)
    second = d.icp(iters=b, state=first.state)
    assert whole.iterations == a + b and first.iterations == a and second.iterations == a + b and whole.status == IR.RUNNING
    assert np.array_equal(bits(whole.state), bits(second.state))
    assert not np.array_equal(bits(whole.state), bits(first.state))


def test_a_captured_call_replays_to_the_eager_bits(MT):
    d = Device(MT, "similarity")
    eager = d.icp(iters=7, return_pairs=True)
    start = state_of(d.sc["init"], MT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d.icp(iters=7, state=start, read=False)                              # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = d.icp(iters=7, state=start, return_pairs=True, read=False)
    for _ in range(2):
        res.state.fill_(-3.0)
        res.pair_idx.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(res.state), bits(eager.state)) and np.array_equal(bits(res.evaluation), bits(eager.evaluation))
        assert torch.equal(res.pair_idx, eager.pair_idx) and np.array_equal(bits(res.pair_d2), bits(eager.pair_d2))
    assert res.read().iterations == 7 and res.rmse == eager.rmse


@pytest.mark.parametrize("name", ["plane", "sliding"])
def test_a_finished_state_is_left_alone(MT, name):
    """plane ends converged, sliding degenerate: a further call changes neither the state nor the pair arrays nor the sums"""
    d = Device(MT, name)
    done = d.icp()
    assert done.status == (IR.CONVERGED if name == "plane" else IR.DEGENERATE)
    state = done.state.clone()
    for iters in (0, 1, 5):
        idx, d2, sums = d.raw(state, iters, pairs=True, sums=True)
        torch.cuda.synchronize()
        assert np.array_equal(bits(state), bits(done.state))
        assert bool((idx == -7).all()) and bool((d2 == -1.0).all()) and bool(torch.isnan(sums).all())


@pytest.mark.parametrize("name", ["sliding", "no_pairs"])
def test_degenerate_scenes_keep_their_transform(MT, name):
    d = Device(MT, name)
    T = (1.0, S.rotation([1.0, 2.0, 3.0], 0.01), np.array([0.001, -0.002, 0.003])) if name == "sliding" else d.sc["init"]
    start = state_of(T, MT)
    res = d.icp(state=start, return_pairs=True)
    assert res.status == IR.DEGENERATE and res.iterations == 0
    assert np.array_equal(bits(res.state)[:13], bits(start)[:13])
    if name == "no_pairs":
        assert res.n_pairs == 0 and np.isnan(res.rmse) and bool((res.pair_idx == -1).all()) and bool(torch.isinf(res.pair_d2).all())
    else:
        assert res.n_pairs == d.m


def test_empty_clouds_are_degenerate_at_once(MT):
    sc = S.scenes()["rigid"]
    src, dst = dev(sc["src"]), dev(sc["dst"])
    for iters in (0, 5):
        res = MT.icp(torch.zeros(0, 3, device=DEV), dst, iters=iters, return_pairs=True)
        assert res.status == IR.DEGENERATE if iters else res.status == IR.RUNNING
        assert res.iterations == 0 and res.n_pairs == 0 and res.pair_idx.numel() == 0
        res = MT.icp(src, torch.zeros(0, 3, device=DEV), iters=iters, return_pairs=True)
        assert res.status == IR.DEGENERATE if iters else res.status == IR.RUNNING
        assert res.iterations == 0 and res.n_pairs == 0 and bool((res.pair_idx == -1).all()) and bool(torch.isinf(res.pair_d2).all())
        assert float(res.s) == 1.0 and torch.equal(res.R, torch.eye(3, dtype=torch.float64, device=DEV))
        assert int(res.evaluation[16]) == IR.DEGENERATE                        # the evaluation call itself: no pairs, degenerate at once


def test_refusals(MT):
    sc = S.scenes()["rigid"]
    d = Device(MT, "rigid")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.icp(d.src.cpu(), d.grid)
    with pytest.raises(ValueError, match="iters"):
        d.icp(iters=MT.ICP_MAX_ITERS + 1)
    with pytest.raises(ValueError, match="max_dist"):
        d.icp(max_dist=-1.0)
    with pytest.raises(ValueError, match="tol_rot"):
        d.icp(tol_rot=float("nan"))
    with pytest.raises(ValueError, match="dst_normals"):
        d.icp(dst_normals=d.src)
    from ls2fm import _lib
    lib, g = _lib.load(), d.grid
    state = state_of(sc["init"], MT)
    ws = _lib.workspace(lib.ls2fm_icp_workspace_bytes(d.m), "ls2fm_icp_workspace_bytes", DEV)

    def run(src=d.src, m=d.m, sorted_=g.sorted, cell_size=g.cell_size, max_d2=1.0, iters=1, tol=1e-9, st=state, work=ws):
        grid = list(g.c_args())
        grid[0], grid[4] = _lib.ptr(sorted_), cell_size                      # sorted and cell_size are what the refusals vary
        return lib.ls2fm_icp_run(_lib.ptr(src), m, *grid, None, max_d2, 0, iters, tol, 1e-9, _lib.ptr(st), None, None, None, _lib.ptr(work),
                                 _lib.stream_ptr())

    assert run() == 0
    torch.cuda.synchronize()
    before = bits(state).copy()
    for bad in (dict(src=None), dict(m=-1), dict(sorted_=None), dict(cell_size=0.0), dict(max_d2=float("nan")), dict(max_d2=-1.0),
                dict(iters=-1), dict(iters=MT.ICP_MAX_ITERS + 1), dict(tol=float("nan")), dict(tol=-1.0), dict(st=None)):
        assert run(**bad) == -1, bad                                          # LS2FM_ERR_INVALID_ARGUMENT
    assert run(work=None) != 0 and lib.ls2fm_icp_workspace_bytes(-1) < 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(state), before)                                # nothing was enqueued


@pytest.fixture(scope="module")
def sphere_mesh():
    from ls2fm import mesh
    g = torch.linspace(-1.0, 1.0, 32, device=DEV)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return mesh.marching_cubes((x * x + y * y + z * z).sqrt() - 0.6, 0.0, spacing=(2 / 31,) * 3, origin=(-1.0,) * 3)


GAUGE = (1.3, S.rotation([0.2, 1.0, -0.4], 0.7), np.array([0.4, -1.1, 2.0]))       # the mesh's frame -> the ground truth's
INIT_OFF = (1.01, S.rotation([1.0, 0.3, 0.5], np.radians(1.0)), np.array([0.01, -0.008, 0.012]))


def _eval_args():
    """ground truth on the true sphere, density, max_dist, thresholds"""
    import metrics_scenes
    return metrics_scenes._sphere(np.random.default_rng(3), 4000, 0.6), 0.06, 0.1, (0.03, 0.05)


def test_evaluate_mesh_registers_a_mesh_in_another_gauge(MT, sphere_mesh):
    """A marching-cubes sphere of radius 0.6 is taken into another gauge (scale 1.3, 0.7 rad, a shift) and scored against points of
    the true sphere with an init that is 1 % / 1 degree / 0.018 off the way back; the registration is a similarity, 30 iterations.
    The registered Chamfer `overall` must be no worse than MARGIN = 1.00 x the score of the mesh that never left the ground truth's
    frame, and the init alone must score worse than 1.04 x.  Both factors are the restatement's: the same scene restated in numpy on
    the CPU (1257 samples of a sphere of radius 0.5992, where marching cubes puts this surface, thinned at 0.06 against the same
    thinned ground truth, moved by INIT_OFF, registered by icp_restate.run with scale, scored by metrics_restate.chamfer), for three
    samples of the surface: init alone 1.079, 1.071, 1.089 x the unmoved score, registered 0.978, 0.980, 0.985 x -- below 1,
    because the fitted scale takes out the mesh's radius bias -- so 1.00 leaves twice the spread of the three."""
    verts, faces = sphere_mesh
    gt, density, max_dist, thresholds = _eval_args()
    gen = torch.Generator(device=DEV).manual_seed(5)
    unmoved = MT.evaluate_mesh(verts, faces, dev(gt), max_dist, density, thresholds, generator=gen)
    s, R, t = GAUGE
    away = ((verts.double().cpu().numpy() - t) @ R / s).astype(np.float32)         # GAUGE maps `away` back onto verts
    init = (s * INIT_OFF[0], INIT_OFF[1] @ R, INIT_OFF[0] * INIT_OFF[1] @ t + INIT_OFF[2])
    gen.manual_seed(5)
    off = MT.evaluate_mesh(dev(away), faces, dev(gt), max_dist, density, thresholds, generator=gen, init=init, icp=dict(iters=0, with_scale=True))
    gen.manual_seed(5)
    out = MT.evaluate_mesh(dev(away), faces, dev(gt), max_dist, density, thresholds, generator=gen, init=init, icp=dict(iters=30, with_scale=True),
                           return_points=True)
    print(f"overall: unmoved {unmoved['overall']:.5f}, init only {off['overall']:.5f}, registered {out['overall']:.5f}; "
          f"icp {out['icp_iterations']} iterations, status {out['icp_status']}, rmse {out['icp_rmse']:.5f}, pairs {out['icp_n_pairs']}")
    assert out["overall"] <= 1.00 * unmoved["overall"]
    assert off["overall"] > 1.04 * unmoved["overall"]                          # the scene needs the registration
    assert off["icp_iterations"] == 0 and out["icp_iterations"] > 0 and out["icp_n_pairs"] > 0.9 * out["n_pred"]
    # the returned transform is the whole one: it takes the mesh's own vertices onto the sphere
    moved = float(out["s"]) * (dev(away).double() @ out["R"].t()) + out["t"]
    assert float((moved.norm(dim=1) - 0.6).abs().max()) < 0.01
    assert out["pred_points"].shape[0] == out["n_pred"]


def test_evaluate_mesh_without_registration_is_what_it_was(MT, sphere_mesh):
    """init = icp = None: the steps of evaluate_mesh as they stood before it took the two arguments, written out here, give the
    same dict -- the same keys, the same bits"""
    from ls2fm import mesh
    import math
    verts, faces = sphere_mesh
    gt, density, max_dist, thresholds = _eval_args()
    gen = torch.Generator(device=DEV).manual_seed(5)
    got = MT.evaluate_mesh(verts, faces, dev(gt), max_dist, density, thresholds, generator=gen, init=None, icp=None)
    gen.manual_seed(5)
    count = int(math.ceil(float(mesh._face_areas64(verts, faces).sum()) / (density * density)))
    pts = mesh.sample_surface(verts, faces, count, generator=gen)
    pts = pts[MT.voxel_downsample(pts, density)]
    g = dev(gt).float()
    g = g[MT.voxel_downsample(g, density)]
    exp = MT.chamfer(pts, g, max_dist, thresholds=thresholds)
    exp.update(n_pred=int(pts.shape[0]), n_gt=int(g.shape[0]))
    assert list(got) == list(exp)
    for k in exp:
        assert got[k] == exp[k] or (isinstance(exp[k], float) and np.isnan(exp[k]) and np.isnan(got[k])), k
