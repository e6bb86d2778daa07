"""ls2fm.tracks on the device against tests/tracks_restate.py.

Integer outputs (labels, the track table, inliers, num_inliers, success, the winning pair) are compared EXACTLY on every track:
tests/test_tracks_host.py asserts that no decision of the restatement on these scenes comes within 1e-6 px / 1e-9 rad of its
threshold, so 0 tracks are excluded.

TOL: the tolerance of X, tri_angle and mean_error_px.  Measured, not guessed: the largest difference over these same scenes
between the restatement's two fp64 routes (one-sided / cyclic Jacobi against numpy.linalg svd / eigh) is 3.46e-13 (X, scene
"mixed"; tri_angle 8.4e-15, mean_error_px 2.4e-13); times 4, the margin DESIGN 3.8 uses for one more independent rounding path:
1.4e-12, absolute, in scene units / radians / pixels (tracks_scenes.TOL; tests/test_tracks_host.py recomputes the gap and holds it to
TOL / 4).  The kernel is never its own yardstick.

Two sets of scenes: tracks_scenes.gpu_scenes(), and more_gpu_scenes() for the shapes and options the first never reaches (a camera
per view, the striding grid, deep winning pairs, tracks without a pair, 4096 observations, the local optimisation's exits).  The
host tests assert, for each scene of the second set, the condition under which the device test here fails for a wrong kernel."""
import numpy as np
import pytest
import torch

import tracks_restate as R
import tracks_scenes as S

pytestmark = pytest.mark.gpu

TOL = S.TOL                 # 1.4e-12
DEV = "cuda:0"
SCENES = S.gpu_scenes() if torch.cuda.is_available() else {}
MORE = S.more_gpu_scenes() if torch.cuda.is_available() else {}       # name -> (scene, the options of its runs)
OUTPUTS = ("X", "inliers", "num_inliers", "success", "tri_angle", "mean_error_px", "best_pair")
_WANT = {}


@pytest.fixture(scope="module")
def TR():
    from ls2fm import tracks
    return tracks


@pytest.fixture(scope="module")
def restated():
    """the restatement of every scene, once"""
    return {name: R.triangulate_tracks(sc["poses"], sc["intr"], sc["track_start"], sc["obs_view"], sc["obs_uv"]) for name, sc in SCENES.items()}


def want(name, i=0):
    """the restatement of run i of scene `name` of the second set, computed when first asked for and shared"""
    if (name, i) not in _WANT:
        sc, options = MORE[name]
        _WANT[name, i] = R.triangulate_tracks(sc["poses"], sc["intr"], sc["track_start"], sc["obs_view"], sc["obs_uv"], **options[i])
    return _WANT[name, i]


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def run(TR, sc, track_start=None, obs_view=None, obs_uv=None, **kw):
    tracks = dict(track_start=dev(sc["track_start"] if track_start is None else track_start, torch.int32),
                  obs_view=dev(sc["obs_view"] if obs_view is None else obs_view, torch.int32))
    uv = dev(sc["obs_uv"] if obs_uv is None else obs_uv, torch.float64)
    out = TR.triangulate_tracks(tracks, None, dev(sc["poses"], torch.float64), dev(sc["intr"], torch.float64), obs_uv=uv, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bytes(a, b, tracks_a, tracks_b, start_a, start_b, what):
    """tracks_a of run a against tracks_b of run b (as many, in order): every output byte for byte"""
    for k in OUTPUTS:
        if k == "inliers":
            ia = np.concatenate([np.arange(start_a[t], start_a[t + 1]) for t in tracks_a])
            ib = np.concatenate([np.arange(start_b[t], start_b[t + 1]) for t in tracks_b])
            assert a[k][ia].tobytes() == b[k][ib].tobytes(), f"{what}: {k}"
        else:
            assert a[k][tracks_a].tobytes() == b[k][tracks_b].tobytes(), f"{what}: {k}"
    print(f"[tracks] {what}: {len(tracks_a)} tracks byte-equal in {len(OUTPUTS)} outputs")


def assert_empty(got, tracks, what):
    """what include/ls2fm.h defines for a track without a point: everything 0, best_pair -1"""
    assert (got["X"][tracks] == 0).all() and (got["num_inliers"][tracks] == 0).all() and not got["success"][tracks].any(), what
    assert (got["tri_angle"][tracks] == 0).all() and (got["mean_error_px"][tracks] == 0).all(), what
    assert (got["best_pair"][tracks] == -1).all(), what


def compare(got, want, what):
    for k in ("inliers", "num_inliers", "success", "best_pair"):
        assert np.array_equal(got[k].astype(np.int64), np.asarray(want[k]).astype(np.int64)), f"{what}: {k} differs"
    for k in ("X", "tri_angle", "mean_error_px"):
        d = float(np.abs(got[k] - want[k]).max()) if got[k].size else 0.0
        print(f"[tracks] {what}: {k} max difference {d:.3e} (TOL {TOL:.1e})")
        assert d <= TOL, f"{what}: {k} differs by {d:.3e}"


# ------------------------------------------------------------------------------------------------------------------ labels
def _graphs():
    i3, e3 = S.random_graph(1)                                        # 900 nodes / 500 edges: several workgroups, components across them
    p_start, p_edges = S.path_graph(4097)                             # 4097 views, the edges from the far end: the longest chain
    return {"random": (i3, e3), "path": S.path_graph(64), "star": S.star_graph(), "no_edges": (i3, np.zeros((0, 2), np.int32)),
            "isolated": (i3, e3[:40]), "contended": S.contended_graph(3), "path_4097_descending": (p_start, p_edges[::-1].copy()),
            "empty_images": (S.EMPTY_IMAGES, np.array([[4, 5], [8, 9]], np.int32))}


@pytest.mark.parametrize("graph", ["random", "path", "star", "no_edges", "isolated", "contended", "path_4097_descending", "empty_images"])
def test_labels_against_restatement(TR, graph):
    image_start, edges = _graphs()[graph]
    want = R.track_labels(image_start, edges)
    got = TR.track_labels(image_start, dev(edges, torch.int32)).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if graph == "no_edges":
        assert np.array_equal(got, np.arange(len(got)))
    # every edge twice and the list reversed: the same labels
    again = TR.track_labels(image_start, dev(np.concatenate([edges, edges])[::-1].copy(), torch.int32)).cpu().numpy()
    assert np.array_equal(again, want)


def test_contended_graph_track_table(TR):
    """20 000 nodes, 100 000 edges inside 400 components of 50: every wave of tl_hook unites into the same few trees"""
    image_start, edges = S.contended_graph(3)
    labels = R.track_labels(image_start, edges)
    want = R.build_tracks(image_start, labels)
    sizes = np.diff(want["track_start"])
    print(f"[tracks] contended: {len(sizes)} tracks of {sizes.min()} .. {sizes.max()} observations, {len(np.unique(labels))} components")
    assert len(sizes) == 400 and want["n_conflicts"] == 0
    got = TR.build_tracks(image_start, dev(edges, torch.int32))
    assert got["n_conflicts"] == 0 and np.array_equal(got["labels"].cpu().numpy(), labels)
    for k in ("track_start", "obs_node", "obs_view"):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want[k]), k


def test_label_refusals_with_empty_images(TR):
    """images without a key point: image_of must skip the repeated image_start entries"""
    start = S.EMPTY_IMAGES
    n = int(start[-1])
    good = np.array([[4, 5], [8, 9]], np.int32)                        # the last node of an image to the first of the next
    joined = [0, 1, 2, 3, 4, 4, 6, 7, 8, 8, 10, 11, 12, 13]
    assert R.track_labels(start, good).tolist() == joined
    for bad, bit in (([5, 8], 2), ([0, 4], 2), ([9, 13], 2), ([0, n], 1), ([n, 13], 1)):
        e = dev(np.concatenate([good, np.array([bad], np.int32)]), torch.int32)
        labels, status = TR.track_labels(start, e, return_status=True)
        assert int(status.item()) == bit == R.edge_status(start, e.cpu().numpy()), bad
        assert labels.cpu().tolist() == joined, bad                    # the bad edge joined nothing
        with pytest.raises(ValueError):
            TR.track_labels(start, e)
    # the whole graph as ONE image: every edge lies inside it
    labels, status = TR.track_labels([0, n], dev(good, torch.int32), return_status=True)
    assert int(status.item()) == 2 and labels.cpu().tolist() == list(range(n))
    with pytest.raises(ValueError):
        TR.track_labels([0, n], dev(good, torch.int32))


def test_track_table_and_planted_conflict(TR):
    image_start, edges = S.random_graph(2, n_views=3, n_kp=300, n_edges=260)
    # a planted conflict on two nodes no random edge touches... whatever else the random edges made
    edges = np.concatenate([edges, np.array([[0, 300], [300, 1]], np.int32)])
    want = R.build_tracks(image_start, R.track_labels(image_start, edges))
    got = TR.build_tracks(image_start, dev(edges, torch.int32))
    assert want["n_conflicts"] >= 1 and got["n_conflicts"] == want["n_conflicts"]
    for k in ("track_start", "obs_node", "obs_view"):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want[k]), k
    lab = got["labels"].cpu().numpy()
    assert lab[0] == lab[1] == lab[300] == 0 and 0 not in got["obs_node"].cpu().numpy()


def test_label_refusals_on_the_device(TR):
    image_start = np.array([0, 3, 6], np.int32)
    good = np.array([[0, 3], [1, 4]], np.int32)
    for bad, bit in ((np.array([[0, 6]], np.int32), 1), (np.array([[-1, 3]], np.int32), 1), (np.array([[0, 2]], np.int32), 2),
                     (np.array([[4, 4]], np.int32), 2)):
        e = dev(np.concatenate([good, bad]), torch.int32)
        labels, status = TR.track_labels(image_start, e, return_status=True)
        assert int(status.item()) == bit
        assert labels.cpu().tolist() == [0, 1, 2, 0, 1, 5]            # the bad edge joined nothing
        with pytest.raises(ValueError):
            TR.track_labels(image_start, e)
    # an int64 id that would wrap into range as int32 (2^32 + 3 -> 3) is reported, not joined
    wide = torch.tensor([[0, 3], [1, 4], [2, (1 << 32) + 3]], dtype=torch.int64, device=DEV)
    labels, status = TR.track_labels(image_start, wide, return_status=True)
    assert int(status.item()) == 1 and labels.cpu().tolist() == [0, 1, 2, 0, 1, 5]
    from ls2fm import _lib
    lib = _lib.load()
    assert lib.ls2fm_track_labels(None, 2, 6, None, 0, None, None, None) != 0
    assert lib.ls2fm_track_labels(_lib.ptr(dev(image_start)), 2, 1 << 31, None, 0, None, None, None) != 0
    assert lib.ls2fm_triangulate_tracks_workspace_bytes(1 << 31, 2) < 0 and lib.ls2fm_triangulate_tracks_workspace_bytes(4, 0) < 0


# ----------------------------------------------------------------------------------------------------------- triangulation
@pytest.mark.parametrize("name", ["len2", "len3", "len64", "len66", "mixed", "outliers"])
def test_triangulation_against_restatement(TR, restated, name):
    compare(run(TR, SCENES[name]), restated[name], name)


@pytest.mark.parametrize("name,i", [("per_view_intr", 0), ("per_view_intr", 1), ("deep_pair", 0), ("long_outliers", 0), ("longest", 0),
                                    ("lo_exits", 0), ("len3_b", 0)])
def test_second_set_against_restatement(TR, name, i):
    """tests/test_tracks_host.py pins what each scene reaches: a camera per view with fx != fy through the [V, 4] route, winning
    pairs up to q = 2015, more than 64 inliers with outliers among the first 64, 4096 observations at group 3 of a full wave and in
    a partial one, and the local optimisation's "fewer" exit and second refit"""
    sc, options = MORE[name]
    if name == "per_view_intr":
        assert sc["intr"].shape == (len(sc["poses"]), 4)
    compare(run(TR, sc, **options[i]), want(name, i), f"{name} {options[i]}")


def test_stride_of_the_hypothesis_grid(TR):
    """536 copies of 16 tracks of 64 observations: 1 080 576 hypotheses, more than tt_hyp's capped grid has lanes"""
    sc, _ = MORE["stride"]
    copies = 536
    start, view, uv = S.tile_tracks(sc, copies)
    # kMaxHypBlocks (4096) x kThreads (256) of csrc/tracks.hip: a hypothesis numbered at or above it is reached only by striding
    lane_limit = 4096 * 256
    beyond = np.nonzero(np.arange(copies) * S.PAIRS_64 >= lane_limit)[0]
    assert lane_limit == S.HYP_LANE_LIMIT and len(beyond) >= 8 and beyond[0] == 521
    got = run(TR, sc, track_start=start, obs_view=view, obs_uv=uv)
    base = want("stride")
    src = np.arange(copies) % 16
    tiled = {k: (np.tile(base[k], copies // 16 + 1)[:len(view)] if k == "inliers" else base[k][src]) for k in OUTPUTS}
    compare(got, tiled, "stride")
    assert got["success"][beyond].all()
    same_bytes(got, got, np.arange(16, copies), src[16:], start, start, "stride: every copy against the first")


def test_tracks_without_a_pair(TR):
    """tracks of 0 and 1 observations at the start of the table, across the scan round's boundary 1023 / 1024, alone in a wave, a
    whole wave of them and at the end: all outputs 0, best_pair -1, status 0, and their neighbours untouched"""
    sc, _ = MORE["short"]
    short = sc["short"]
    got = run(TR, sc)
    assert int(got["status"][0]) == 0 and not got["inliers"][np.repeat(short, np.diff(sc["track_start"]))].any()
    assert_empty(got, short, "short tracks")
    compare(got, want("short"), "short")
    keep = np.nonzero(~short)[0]
    start, view, uv, _ = S.permute_tracks(sc, keep)
    alone = run(TR, sc, track_start=start, obs_view=view, obs_uv=uv)
    same_bytes(got, alone, keep, np.arange(len(keep)), sc["track_start"], start, "short: ordinary tracks against the table without the short ones")
    # only such tracks: no hypothesis at all
    n = np.arange(19) % 2
    start = np.concatenate([[0], np.cumsum(n)])
    none = run(TR, sc, track_start=start, obs_view=sc["obs_view"][:n.sum()], obs_uv=sc["obs_uv"][:n.sum()])
    assert int(none["status"][0]) == 0 and not none["inliers"].any() and none["X"].shape == (19, 3)
    assert_empty(none, np.arange(19), "a table of short tracks only")
    none = run(TR, sc, track_start=np.zeros(6, np.int32), obs_view=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2)))
    assert int(none["status"][0]) == 0 and none["inliers"].shape == (0,)
    assert_empty(none, np.arange(5), "five tracks of no observation")


def test_one_observation_too_many(TR):
    """a track of LS2FM_TRACK_MAX_OBS + 1 = 4097 observations next to the one of 4096: refused by the status word, treated as empty,
    and the other tracks keep every bit"""
    sc, _ = MORE["longest"]
    start, view, uv, keep = S.with_overlong_track(sc, 4)
    assert np.diff(start)[4] == 4097 and np.diff(start)[3] == 4096
    got = run(TR, sc, track_start=start, obs_view=view, obs_uv=uv, validate=False)
    assert int(got["status"][0]) == 1                                 # LS2FM_TRACK_BAD_START
    assert_empty(got, np.array([4]), "the track of 4097")
    assert not got["inliers"][start[4]:start[5]].any()
    without = run(TR, sc)
    assert int(without["status"][0]) == 0
    same_bytes(got, without, keep, np.arange(len(keep)), start, sc["track_start"], "4097: the other tracks against the table without it")
    with pytest.raises(ValueError):
        run(TR, sc, track_start=start, obs_view=view, obs_uv=uv)


def test_outliers_and_low_parallax(TR):
    sc = SCENES["outliers"]
    got = run(TR, sc)
    assert int(sc["outlier"].sum()) >= 25 and not (got["inliers"] & sc["outlier"]).any()
    assert sc["low_parallax"].sum() == 6 and not got["success"][sc["low_parallax"]].any()
    assert (got["X"][sc["low_parallax"]] == 0).all()
    assert got["success"][~sc["low_parallax"]].all()
    # without an angle threshold the acceptance is the restatement's: the ring tracks as before, and of the coincident pairs those
    # whose noisy rays still meet in front of both cameras (four of the six here; the other two have no hypothesis left at all)
    free = run(TR, sc, min_tri_angle_deg=0.0)
    want = R.triangulate_tracks(sc["poses"], sc["intr"], sc["track_start"], sc["obs_view"], sc["obs_uv"], min_tri_angle_deg=0.0)
    for k in ("inliers", "num_inliers", "success", "best_pair"):
        assert np.array_equal(free[k].astype(np.int64), np.asarray(want[k]).astype(np.int64)), k
    assert free["success"][~sc["low_parallax"]].all() and free["success"][sc["low_parallax"]].sum() == 4
    assert (free["best_pair"][sc["low_parallax"]][~free["success"][sc["low_parallax"]]] == -1).all()


def test_noise_free_scene_recovers_the_planted_points(TR):
    sc = S.noise_free_scene()
    got = run(TR, sc)
    assert got["success"].all()
    # every pair counts every observation: the lowest must win (the host test asserts that the restated best_pair is 0 throughout)
    compare(got, want("noise_free"), "noise_free")
    d = float(np.abs(got["X"] - sc["points"]).max())
    print(f"[tracks] truth: max |X - planted| {d:.3e} (bound {TOL * S.EXTENT:.2e})")
    assert d <= TOL * S.EXTENT
    assert float(got["mean_error_px"].max()) <= TOL * S.F_PX


def test_bit_identity(TR):
    sc = SCENES["mixed"]
    full = run(TR, sc)
    again = run(TR, sc)
    for k in full:
        assert np.array_equal(full[k], again[k], equal_nan=True), f"rerun: {k}"
    ts = sc["track_start"]
    T = len(ts) - 1
    # one call per track: the four long tracks, sixty short ones and the low-parallax ones
    for t in list(range(0, 64)) + list(range(T - 5, T)):
        one = run(TR, sc, track_start=np.array([0, ts[t + 1] - ts[t]]), obs_view=sc["obs_view"][ts[t]:ts[t + 1]], obs_uv=sc["obs_uv"][ts[t]:ts[t + 1]])
        assert one["X"].tobytes() == full["X"][t:t + 1].tobytes(), f"track {t}: X"
        assert np.array_equal(one["inliers"], full["inliers"][ts[t]:ts[t + 1]]) and one["success"][0] == full["success"][t]
        assert one["tri_angle"].tobytes() == full["tri_angle"][t:t + 1].tobytes()
        assert one["mean_error_px"].tobytes() == full["mean_error_px"][t:t + 1].tobytes()
    perm = np.random.default_rng(0).permutation(T)
    start, view, uv, idx = S.permute_tracks(sc, perm)
    shuffled = run(TR, sc, track_start=start, obs_view=view, obs_uv=uv)
    for k in ("X", "num_inliers", "success", "tri_angle", "mean_error_px", "best_pair"):
        assert shuffled[k].tobytes() == full[k][perm].tobytes(), f"permutation: {k}"
    assert np.array_equal(shuffled["inliers"], full["inliers"][idx])


def test_triangulation_refusals_on_the_device(TR):
    sc = SCENES["len3"]
    ts = sc["track_start"].copy()
    ts[2] = ts[1] - 1                                                 # runs backwards
    out = run(TR, sc, track_start=ts, validate=False)
    assert int(out["status"][0]) & 1
    view = sc["obs_view"].copy()
    view[4] = 1000                                                    # no such view (track 1)
    out = run(TR, sc, obs_view=view, validate=False)
    assert int(out["status"][0]) == 2 and not out["inliers"][4]
    want = R.triangulate_tracks(sc["poses"], sc["intr"], sc["track_start"], sc["obs_view"], sc["obs_uv"])
    assert np.array_equal(out["success"][[0, 2, 3, 4]], want["success"][[0, 2, 3, 4]])       # the other tracks are untouched
    ts = sc["track_start"].copy()
    ts[-1] = len(sc["obs_view"]) + 7                                   # past the observations
    assert int(run(TR, sc, track_start=ts, validate=False)["status"][0]) & 1
    with pytest.raises(ValueError):
        run(TR, sc, obs_view=view)
    with pytest.raises(ValueError):
        run(TR, sc, max_error_px=float("nan"))
    from ls2fm import _lib
    assert _lib.load().ls2fm_triangulate_tracks(None, None, 1, None, 0, None, None, 0, 4.0, 1.5, None, None, None, None, None, None, None,
                                                None, None, None) != 0
    empty = run(TR, sc, track_start=np.array([0]), obs_view=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2)))
    assert empty["X"].shape == (0, 3) and int(empty["status"][0]) == 0


def test_call_is_capturable(TR):
    sc = SCENES["len3"]
    tracks = dict(track_start=dev(sc["track_start"], torch.int32), obs_view=dev(sc["obs_view"], torch.int32))
    args = (tracks, None, dev(sc["poses"], torch.float64), dev(sc["intr"], torch.float64))
    uv = dev(sc["obs_uv"], torch.float64)
    eager = TR.triangulate_tracks(*args, obs_uv=uv)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        TR.triangulate_tracks(*args, obs_uv=uv)                       # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = TR.triangulate_tracks(*args, obs_uv=uv)
    out["X"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["X"], eager["X"]) and torch.equal(out["inliers"], eager["inliers"])


def test_replay_of_a_captured_call_on_new_data(TR):
    """the captured call re-zeroes its own workspace: scene B (another seed, and one observation of a view that does not exist, so
    status 2) written into the captured inputs and replayed gives an eager run on B; scene A written back gives eager A"""
    a, b = SCENES["len3"], MORE["len3_b"][0]
    assert np.array_equal(a["track_start"], b["track_start"]) and a["poses"].shape == b["poses"].shape
    view_b = b["obs_view"].copy()
    view_b[4] = 1000                                                   # track 1
    inputs = {"A": (a["obs_view"], a["obs_uv"], a["poses"]), "B": (view_b, b["obs_uv"], b["poses"])}
    eager = {}
    for name, (view, uv, poses) in inputs.items():
        tracks = dict(track_start=dev(a["track_start"], torch.int32), obs_view=dev(view, torch.int32))
        out = TR.triangulate_tracks(tracks, None, dev(poses, torch.float64), dev(a["intr"], torch.float64), obs_uv=dev(uv, torch.float64),
                                    validate=False)
        eager[name] = {k: out[k].clone() for k in OUTPUTS + ("status",)}
    assert int(eager["A"]["status"].item()) == 0 and int(eager["B"]["status"].item()) == 2
    assert not torch.equal(eager["A"]["X"], eager["B"]["X"]) and not torch.equal(eager["A"]["num_inliers"], eager["B"]["num_inliers"])
    tracks = dict(track_start=dev(a["track_start"], torch.int32), obs_view=dev(a["obs_view"], torch.int32))
    poses, intr, uv = dev(a["poses"], torch.float64), dev(a["intr"], torch.float64), dev(a["obs_uv"], torch.float64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        TR.triangulate_tracks(tracks, None, poses, intr, obs_uv=uv)    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = TR.triangulate_tracks(tracks, None, poses, intr, obs_uv=uv)
    for name in ("B", "A", "B"):
        view_h, uv_h, poses_h = inputs[name]
        tracks["obs_view"].copy_(dev(view_h, torch.int32))
        uv.copy_(dev(uv_h, torch.float64))
        poses.copy_(dev(poses_h, torch.float64))
        g.replay()
        torch.cuda.synchronize()
        for k in OUTPUTS + ("status",):
            assert torch.equal(out[k], eager[name][k]), f"replay on {name}: {k}"
        print(f"[tracks] replay on {name}: {len(OUTPUTS) + 1} outputs equal the eager run, status {int(out['status'].item())}")


def test_end_to_end_tables_to_bundle_adjustment(TR):
    """tables -> edges_from_n_views -> build_tracks -> triangulate_tracks -> to_tracked_views -> TradBALoop(max_iter=20).run() at
    4 views x 400 key points, from poses a registration would hand over (0.004 rad / 0.03 units off).  The logged mean error does
    not rise at ANY iteration and ends below the noise level the scene planted (the mean length of the planted pixel noise).
    The loop runs at S.BA_LR_SCALE = 0.05 x its default learning rates: Adam's first steps move every parameter by its rate
    whatever the gradient, and the defaults (5e-3 rad is 3 px at f = 600) are sized for far cruder starts than a triangulation
    within 2 px -- with them the log of this scene doubles at its second iteration before it falls."""
    from ls2fm.stage import TradBALoop
    scene = S.match_scene(21, noise_px=1.0)
    poses = S.perturb_poses(scene["poses"], 5, 0.004, 0.03)
    image_start, edges = TR.edges_from_n_views(scene["tables"])
    tracks = TR.build_tracks(image_start, dev(edges, torch.int32))
    want = R.build_tracks(image_start, R.track_labels(image_start, edges))
    assert tracks["n_conflicts"] == scene["n_conflicts"] and np.array_equal(tracks["obs_node"].cpu().numpy(), want["obs_node"])
    tri = TR.triangulate_tracks(tracks, scene["keypoints"], dev(poses, torch.float64), S.INTR)
    assert int(tri["success"].sum()) >= 0.95 * tri["success"].numel()
    views = TR.to_tracked_views(tracks, tri, scene["keypoints"], dev(poses, torch.float32), dev(S.K, torch.float32), H=480, W=640)
    vis = TR.visible_points(tracks, tri, [0, 1]).cpu().tolist()
    assert vis[0] == vis[1] == 0 and min(vis[2:]) > 300
    log = TradBALoop(views, max_iter=20, **S.ba_rates()).run()
    err = log["err_mean"].cpu().numpy().astype(np.float64)
    noise = float(np.mean([np.linalg.norm(n, axis=1).mean() for n in scene["noise"]]))
    print(f"[tracks] end to end: mean error {err[0]:.3f} -> {err[-1]:.3f} px, largest step {np.diff(err).max():+.2e}, planted noise {noise:.3f} px")
    assert np.isfinite(err).all() and (np.diff(err) <= 0).all() and err[-1] < noise
