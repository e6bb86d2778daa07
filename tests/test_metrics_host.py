"""CPU: ls2fm.metrics against the numpy restatement (tests/metrics_restate.py) on the scenes of tests/metrics_scenes.py, and the
conditions under which those scenes catch a wrong grid kernel (tests/test_hip_metrics.py runs the kernel on them).

The nearest-neighbour results are compared EXACTLY -- the index and the bits of d2, on every query of every scene: the distance
rule makes them a pure function of the inputs.  Chamfer counts are exact and its means are held to (M + 2) 2^-53 relative, the
bound of an fp64 sum of M non-negative terms in any order plus one rounding of each square root."""
import numpy as np
import pytest
import torch

import metrics_restate as R
import metrics_scenes as S
from ls2fm import metrics as MT


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def mean_bound(m):
    return (m + 2) * 2.0 ** -53


def close(got, want, m):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= mean_bound(m) * abs(want)


# ---------------------------------------------------------------------------------------- what the scenes are there to catch
def test_faces_scene_has_winners_across_a_face():
    sc = S.scenes()["faces"]
    idx, _ = S.expected("faces")
    own, won = S.cells_of(sc["q"], sc["ref"], sc["cell_size"]), S.cells_of(sc["ref"][idx], sc["ref"], sc["cell_size"])
    ring = np.abs(own - won).max(axis=1)
    assert int((ring == 1).sum()) >= 64 and int((ring == 0).sum()) >= 64        # across the face, and one ulp short of it
    # references sit ON multiples of the cell size and one ulp on either side of them
    x = sc["ref"].astype(np.float64) / sc["cell_size"]
    on = (x == np.round(x)).any(axis=1).sum()
    assert on >= 64 and len(np.unique(S.cells_of(sc["ref"], sc["ref"], sc["cell_size"]), axis=0)) > 300


def test_ties_scene_has_minima_in_several_cells():
    sc = S.scenes()["ties"]
    idx, d2 = S.expected("ties")
    all_d2 = R.d2_matrix(sc["q"], sc["ref"])
    cells = S.cells_of(sc["ref"], sc["ref"], sc["cell_size"])
    own = S.cells_of(sc["q"], sc["ref"], sc["cell_size"])
    cell_id = (cells[:, 2] * 7 + cells[:, 1]) * 7 + cells[:, 0]
    spread = later = 0
    for m in range(len(sc["q"])):
        tied = np.nonzero(all_d2[m] == d2[m])[0]
        spread += len(np.unique(cells[tied], axis=0)) >= 2
        ring = np.abs(cells[tied] - own[m]).max(axis=1)
        # the winner (lowest index) sits in a later ring and a higher cell than another tied reference
        later += bool(((ring < ring[0]) & (cell_id[tied] < cell_id[tied[0]])).any()) and idx[m] == tied[0]
    assert spread >= 64 and later >= 64
    assert len(np.unique(sc["ref"], axis=0)) < len(sc["ref"])                  # exact duplicates


def test_cutoff_scene_has_both_outcomes_and_an_equality():
    sc = S.scenes()["cutoff"]
    idx, d2 = S.expected("cutoff")
    lim = R.max_d2_of(sc["max_dist"])
    assert (idx >= 0).sum() >= 20 and (idx < 0).sum() >= 20
    assert idx[0] == 400 and d2[0] == lim and idx[1] == -1 and np.isinf(d2[1])
    assert R.d2_matrix(sc["q"][1:2], sc["ref"])[0].min() > lim                 # one ulp beyond: nothing qualifies


def test_clusters_scene_crosses_empty_rings():
    sc = S.scenes()["clusters"]
    own, cells = S.cells_of(sc["q"], sc["ref"], sc["cell_size"]), S.cells_of(sc["ref"], sc["ref"], sc["cell_size"])
    nearest_ring = np.abs(own[:, None, :] - cells[None, :, :]).max(axis=2).min(axis=1)
    assert int(nearest_ring.min()) >= 9                                        # rings 0 .. 8 hold nothing, for every query


def test_outside_and_nonfinite_scenes_hold_what_they_name():
    sc = S.scenes()["outside"]
    q = sc["q"]
    assert ((q < -1).any(axis=1) | (q > 2).any(axis=1)).sum() >= 20
    nf = S.scenes()["nonfinite"]
    bad = ~np.isfinite(nf["q"]).all(axis=1)
    assert sorted(np.nonzero(bad)[0]) == sorted(nf["bad_rows"]) and np.isnan(nf["q"]).any() and np.isposinf(nf["q"]).any() \
        and np.isneginf(nf["q"]).any()
    idx, d2 = S.expected("nonfinite")
    assert (idx[bad] == -1).all() and np.isinf(d2[bad]).all() and (idx[~bad] >= 0).all()


# ------------------------------------------------------------------------------------------------- the torch forms, on the CPU
@pytest.mark.parametrize("name", S.NAMES)
def test_bruteforce_equals_restatement(name):
    sc = S.scenes()[name]
    want_idx, want_d2 = S.expected(name)
    for chunk in (None, 37):
        idx, d2 = MT.nearest_neighbors_bruteforce(torch.from_numpy(sc["q"]), torch.from_numpy(sc["ref"]), sc["max_dist"], chunk=chunk)
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32
        assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(bits(d2.numpy()), bits(want_d2))


def test_bruteforce_empty_sides():
    q, ref = torch.zeros(3, 3), torch.zeros(0, 3)
    idx, d2 = MT.nearest_neighbors_bruteforce(q, ref)
    assert idx.tolist() == [-1] * 3 and torch.isinf(d2).all()
    idx, d2 = MT.nearest_neighbors_bruteforce(ref, q)
    assert idx.numel() == 0 and d2.numel() == 0


def test_grid_refuses_cpu_tensors():
    sc = S.scenes()["cutoff"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.nearest_neighbors(torch.from_numpy(sc["q"]), torch.from_numpy(sc["ref"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.PointGrid(torch.from_numpy(sc["ref"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.chamfer(torch.from_numpy(sc["q"]), torch.from_numpy(sc["ref"]), 0.1)


def test_auto_cell_size_is_positive_for_every_extent():
    for rule in ("surface", "volume"):
        for lo, hi in (((0, 0, 0), (0, 0, 0)), ((1, 1, 1), (1, 2, 1)), ((0, 0, 0.25), (1, 1, 0.25)), ((0, 0, 0), (1, 2, 3)),
                       ((-1e6, 0, 0), (1e6, 1e-3, 1e6))):
            for n in (0, 1, 257, 2_000_000):
                h = MT.auto_cell_size(lo, hi, n, rule=rule)
                assert np.isfinite(h) and h > 0
                dims = MT.cell_dims((np.asarray(hi, np.float32) - np.asarray(lo, np.float32)), np.float32(1) / np.float32(h))
                assert np.prod(dims) <= 2 ** 25


def test_surface_scene_at_a_quarter_cell_scans_in_two_rounds():
    """pg_scan_sums scans 1024 block totals per round, each of 1024 cells: only a grid of more than 1024 x 1024 cells carries a
    sum into a second round.  The GPU tests build that grid from the surface scene at a quarter of its automatic cell size."""
    ref = S.scenes()["surface"]["ref"]
    lo, hi = ref.min(axis=0), ref.max(axis=0)
    h = np.float32(MT.auto_cell_size(lo, hi, len(ref)) / 4)
    dims = MT.cell_dims((hi - lo).astype(np.float32), np.float32(1) / h)
    assert 1024 * 1024 < np.prod(dims) <= 2 ** 25


@pytest.mark.parametrize("voxel", [0.05, 0.3, 7.0])
def test_voxel_downsample_equals_restatement(voxel):
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.uniform(-1.0, 1.0, (3000, 3)), rng.uniform(-1.0, 1.0, (40, 3)).repeat(3, axis=0),
                        np.array([[0.0, 0.0, 0.0], [-0.0, 0.3, -0.3], [0.3, 0.3, 0.3], [-1e-9, 0.0, 0.0]])]).astype(np.float32)
    got = MT.voxel_downsample(torch.from_numpy(p), voxel)
    want = R.voxel_downsample(p, voxel)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want) and 0 < len(want) < len(p)
    assert MT.voxel_downsample(torch.zeros(0, 3), voxel).numel() == 0


def test_voxel_downsample_refuses_what_21_bits_cannot_hold():
    p = torch.tensor([[0.0, 0.0, 0.0], [1.0e6, 0.0, 0.0]])
    assert MT.voxel_downsample(p, 1.0).tolist() == [0, 1]                      # 10^6 < 2^20
    with pytest.raises(ValueError, match="21 bits"):
        MT.voxel_downsample(p, 0.5)
    with pytest.raises(ValueError, match="21 bits"):
        MT.voxel_downsample(torch.tensor([[float("nan"), 0.0, 0.0]]), 1.0)


def check_chamfer(got, want, m_pred, m_gt):
    assert got["n_accuracy"] == want["n_accuracy"] and got["n_completeness"] == want["n_completeness"]
    assert close(got["accuracy"], want["accuracy"], m_pred) and close(got["completeness"], want["completeness"], m_gt)
    assert close(got["overall"], want["overall"], max(m_pred, m_gt))
    # the rates are ratios of exact integer counts
    assert got["precision"] == want["precision"] and got["recall"] == want["recall"]
    for a, b in zip(got["fscore"], want["fscore"]):
        assert close(a, b, 2)


def test_chamfer_bruteforce_equals_restatement():
    sc = S.scenes()["surface"]
    pred, gt = sc["q"], sc["ref"]
    want = R.chamfer(pred, gt, S.SURFACE_MAX_DIST, S.SURFACE_THRESHOLDS)
    assert 0 < want["n_accuracy"] < len(pred) and 0 < want["n_completeness"] < len(gt)       # the cut-off bites on both sides
    assert all(0 < p < 1 for p in want["precision"] + want["recall"])
    got = MT.chamfer(torch.from_numpy(pred), torch.from_numpy(gt), S.SURFACE_MAX_DIST, S.SURFACE_THRESHOLDS, brute_force=True)
    check_chamfer(got, want, len(pred), len(gt))
    # masks select the points that take part
    pm, gm = np.arange(len(pred)) % 3 != 0, np.arange(len(gt)) % 5 != 0
    want = R.chamfer(pred[pm], gt[gm], S.SURFACE_MAX_DIST, S.SURFACE_THRESHOLDS)
    got = MT.chamfer(torch.from_numpy(pred), torch.from_numpy(gt), S.SURFACE_MAX_DIST, S.SURFACE_THRESHOLDS, pred_mask=torch.from_numpy(pm),
                     gt_mask=torch.from_numpy(gm), brute_force=True)
    check_chamfer(got, want, int(pm.sum()), int(gm.sum()))


def test_chamfer_empty_side_gives_nan_and_zero():
    gt = torch.from_numpy(S.scenes()["surface"]["ref"][:50])
    for pred in (torch.zeros(0, 3), gt + 100.0):                               # no points; no point inside max_dist
        out = MT.chamfer(pred, gt, 0.1, (0.05,), brute_force=True)
        assert out["n_accuracy"] == 0 and out["n_completeness"] == 0
        assert np.isnan(out["accuracy"]) and np.isnan(out["completeness"]) and np.isnan(out["overall"])
    assert MT.chamfer(gt, gt, 0.1, brute_force=True)["overall"] == 0.0


# ------------------------------------------------------------------------------------------------------------- camera poses
def route_gap():
    """the largest difference between the restatement's two routes (SVD; Horn's quaternion) over the camera cases: in (s, R, t)
    of the alignment, and in the per-view errors and the ATE of pose_errors"""
    align = errs = 0.0
    for c in S.camera_cases().values():
        a, b = R.umeyama_svd(c["src"], c["dst"], c["with_scale"]), R.umeyama_horn(c["src"], c["dst"], c["with_scale"])
        align = max(align, abs(a[0] - b[0]), np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max())
        ea = R.pose_errors(c["est"], c["gt"], with_scale=c["with_scale"], route=R.umeyama_svd)
        eb = R.pose_errors(c["est"], c["gt"], with_scale=c["with_scale"], route=R.umeyama_horn)
        errs = max(errs, np.abs(ea["rot_err_deg"] - eb["rot_err_deg"]).max(), np.abs(ea["centre_err"] - eb["centre_err"]).max(),
                   abs(ea["ate_rmse"] - eb["ate_rmse"]), abs(ea["scale"] - eb["scale"]))
    return align, errs


def test_camera_cases_hold_what_they_name():
    cases = S.camera_cases()
    assert {len(c["est"]) for c in cases.values()} >= {8, 50} and any(not c["with_scale"] for c in cases.values())
    m = cases["mirrored"]
    mu_a, mu_b, xa, xb = R._moments(m["src"], m["dst"])
    U, D, Vt = np.linalg.svd(xb.T @ xa)
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0 and D[2] > 1e-3 * D[0] and D[1] > 2 * D[2]       # the determinant case, well apart
    s, Rm, t = R.umeyama_svd(m["src"], m["dst"])
    assert abs(np.linalg.det(Rm) - 1) < 1e-12
    for c in cases.values():
        e = R.pose_errors(c["est"], c["gt"], with_scale=c["with_scale"])
        assert 0.1 < e["rot_err_deg"].max() < 5.0 or not c["with_scale"]        # noisy poses: errors well above rounding


def test_align_sim3_and_pose_errors_equal_restatement():
    """Tolerance: 4 x the largest gap between the restatement's two routes on these inputs (the project's usual margin), recomputed
    here: 7.1e-15 for (s, R, t) of the alignment and 1.7e-13 for the pose errors (degrees and units of length) when this was written,
    against differences of 1.3e-15 and 1.7e-14 between ls2fm.metrics and the restatement."""
    gap_align, gap_err = route_gap()
    print(f"route gaps: alignment {gap_align:.3e}, pose errors {gap_err:.3e}")
    assert 0 < gap_align < 1e-10 and 0 < gap_err < 1e-9
    worst_a = worst_e = 0.0
    for name, c in S.camera_cases().items():
        s, Rm, t = MT.align_sim3(torch.from_numpy(c["src"]), torch.from_numpy(c["dst"]), with_scale=c["with_scale"])
        ws, wR, wt = R.umeyama_svd(c["src"], c["dst"], c["with_scale"])
        assert Rm.dtype == torch.float64 and abs(float(torch.linalg.det(Rm)) - 1) < 1e-12
        worst_a = max(worst_a, abs(s - ws), np.abs(Rm.numpy() - wR).max(), np.abs(t.numpy() - wt).max())
        reg = np.ones(len(c["est"]), bool)
        reg[[1, 4]] = False
        for registered in (None, reg):
            for est in (c["est"], np.concatenate([c["est"], np.tile([[[0.0, 0, 0, 1]]], (len(c["est"]), 1, 1))], axis=1)):      # [V,3,4], [V,4,4]
                got = MT.pose_errors(torch.from_numpy(est), torch.from_numpy(c["gt"]), with_scale=c["with_scale"],
                                     registered=None if registered is None else torch.from_numpy(registered))
                want = R.pose_errors(c["est"], c["gt"], with_scale=c["with_scale"], registered=registered)
                sel = reg if registered is not None else np.ones(len(reg), bool)
                assert got["n_views"] == int(sel.sum()) and got["n_unregistered"] == int((~sel).sum())
                assert np.isnan(got["rot_err_deg"].numpy()[~sel]).all() and np.isnan(got["centre_err"].numpy()[~sel]).all()
                worst_e = max(worst_e, np.abs(got["rot_err_deg"].numpy()[sel] - want["rot_err_deg"][sel]).max(),
                              np.abs(got["centre_err"].numpy()[sel] - want["centre_err"][sel]).max(), abs(got["ate_rmse"] - want["ate_rmse"]),
                              abs(got["scale"] - want["scale"]))
                r, cerr = want["rot_err_deg"][sel], want["centre_err"][sel]
                for key, val in (("rot_err_mean_deg", r.mean()), ("rot_err_max_deg", r.max()), ("centre_err_mean", cerr.mean()),
                                 ("centre_err_max", cerr.max())):
                    worst_e = max(worst_e, abs(got[key] - val))
    print(f"worst differences: alignment {worst_a:.3e}, pose errors {worst_e:.3e}")
    assert worst_a <= 4 * gap_align and worst_e <= 4 * gap_err


def test_pose_errors_without_alignment_and_refusals():
    c = S.camera_cases()["rigid8"]
    est = torch.from_numpy(c["est"])
    out = MT.pose_errors(est, est, align=False)
    assert out["ate_rmse"] == 0.0 and out["rot_err_max_deg"] == 0.0 and out["scale"] == 1.0
    with pytest.raises(ValueError, match="three"):
        MT.pose_errors(est[:2], est[:2])
    with pytest.raises(ValueError):
        MT.pose_errors(est, est[:5])


def test_reconstruction_pose_errors_is_the_thin_call():
    from ls2fm import mapper
    c = S.camera_cases()["similarity8"]
    reg = np.ones(8, bool)
    reg[3] = False
    rec = mapper.Reconstruction([0, 1], reg, torch.from_numpy(c["est"]), None, None, None, None, None, None, 4, 4, None, None)
    got, want = rec.pose_errors(torch.from_numpy(c["gt"])), MT.pose_errors(torch.from_numpy(c["est"]), torch.from_numpy(c["gt"]),
                                                                          registered=torch.from_numpy(reg))
    assert got["n_unregistered"] == 1 and got["ate_rmse"] == want["ate_rmse"] and torch.equal(got["rot_err_deg"][reg], want["rot_err_deg"][reg])
