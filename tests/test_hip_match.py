"""ls2fm.match on the device against the numpy restatement (tests/match_restate.py): everything is compared for EQUALITY.
Every fixture whose decisions are compared meets the restatement's margin condition (>= 1e-6 rad from both thresholds, asserted
by the generator); no row is left out of any comparison."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_restate as MR  # noqa: E402

pytestmark = pytest.mark.gpu

DIRS = (("best_ab", "best_j_ab", "second_ab"), ("best_ba", "best_j_ba", "second_ba"))


def _check_pair(matches, scores, ref, what):
    for names in DIRS:
        for k in names:
            got = scores[k].cpu().numpy().astype(np.int64)
            assert got.shape == ref[k].shape, f"{what}: {k} shape {got.shape} vs {ref[k].shape}"
            bad = np.nonzero(got != ref[k])[0]
            assert bad.size == 0, f"{what}: {k} differs on {bad.size} rows, first {bad[:5]}: {got[bad[:5]]} vs {ref[k][bad[:5]]}"
    got = matches.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == ref["matches"].shape and np.array_equal(got, ref["matches"]), \
        f"{what}: {got.shape[0]} matches vs {ref['matches'].shape[0]}"


@pytest.mark.parametrize("n_a,n_b", [(1, 1), (17, 300), (2000, 1800), (8192, 8191)])
def test_a_raw_integers_and_lists(n_a, n_b):
    from ls2fm.match import match_descriptors
    da, db, ref = MR.seeded_pair(n_a, n_b, seed=100 + n_a, shared=0.5 if n_a > 1 else 1.0)
    assert ref["margin"] >= MR.MIN_MARGIN
    if n_a >= 17:
        assert max(da.max(), db.max()) == 255
    print(f"[match] {n_a} x {n_b}: {len(ref['matches'])} matches, margin {ref['margin']:.3e} rad, largest byte {max(da.max(), db.max())}")
    matches, scores = match_descriptors([da, db], [[0, 1]], return_scores=True)
    _check_pair(matches[0], scores[0], ref, f"{n_a} x {n_b}")
    # device tensors in, no scores: the same lists
    again = match_descriptors([torch.from_numpy(da).cuda(), torch.from_numpy(db).cuda()])
    assert len(again) == 1 and torch.equal(again[0], matches[0])


def test_a_all_bytes_255():
    """the largest possible dot, 128 * 255^2, and saturated rows against ordinary ones"""
    from ls2fm.match import match_descriptors
    rng = np.random.default_rng(5)
    da = rng.integers(0, 256, size=(70, 128), dtype=np.uint8)
    db = rng.integers(0, 256, size=(45, 128), dtype=np.uint8)
    da[3] = 255
    db[7] = 255
    db[40] = 0
    ref = MR.match_pair(da, db)
    assert ref["best_ab"][3] == 128 * 255 * 255 and ref["best_j_ab"][3] == 7
    _, scores = match_descriptors([da, db], [[0, 1]], return_scores=True)
    for names in DIRS:                    # the raw integers only: random bytes are far above length 512, no decision is compared
        for k in names:
            assert np.array_equal(scores[0][k].cpu().numpy().astype(np.int64), ref[k]), k


def test_b_lane_map_every_element():
    """dot(i, j) = 64 i + j for a 64 x 64 block: unique per element and asymmetric.  a_i is 1 at k = 2 i and 16 at k = 2 i + 1
    (an identity spread over k), b_j holds (64 i + j) & 15 and (64 i + j) >> 4 there.  Every element is observed: (A, {b_j}) gives
    column j of the block as the best of A's rows, ({a_i}, B) gives row i as the best of B's rows in the other direction."""
    from ls2fm.match import match_descriptors
    A = np.zeros((64, 128), dtype=np.uint8)
    B = np.zeros((64, 128), dtype=np.uint8)
    i = np.arange(64)
    A[i, 2 * i], A[i, 2 * i + 1] = 1, 16
    v = 64 * i[:, None] + i[None, :]                      # v[i, j]
    B[:, 0::2] = (v & 15).T
    B[:, 1::2] = (v >> 4).T
    assert np.array_equal(MR.products(A, B), v) and not np.array_equal(v, v.T)
    images = [A, B] + [A[k:k + 1] for k in range(64)] + [B[k:k + 1] for k in range(64)]
    pairs = [[0, 2 + 64 + j] for j in range(64)] + [[2 + k, 1] for k in range(64)] + [[0, 1]]
    _, scores = match_descriptors(images, pairs, return_scores=True)
    cols = np.stack([scores[j]["best_ab"].cpu().numpy() for j in range(64)], axis=1)           # [i, j]
    rows = np.stack([scores[64 + k]["best_ba"].cpu().numpy() for k in range(64)], axis=0)      # [i, j]
    assert np.array_equal(cols, v), f"{int((cols != v).sum())} of 4096 elements differ (row side)"
    assert np.array_equal(rows, v), f"{int((rows != v).sum())} of 4096 elements differ (column side)"
    ref = MR.match_pair(A, B)
    for names in DIRS:
        for k in names:
            assert np.array_equal(scores[128][k].cpu().numpy().astype(np.int64), ref[k]), k


def test_c_ties_lowest_j_and_rejection():
    from ls2fm.match import match_descriptors
    da, db, ref0 = MR.seeded_pair(200, 700, seed=7)
    db = db.copy()
    # several copies of a descriptor of b that some row of a matches, across lanes, tiles and both sides of a 32-column boundary
    src = int(ref0["matches"][ref0["matches"][:, 1] > 401][0, 1])
    copies = [5, 31, 32, 33, 100, 401]
    db[copies] = db[src]
    ref = MR.match_pair(da, db)
    assert ref["margin"] >= MR.MIN_MARGIN
    tied = np.nonzero((ref["best_ab"] == ref["second_ab"]) & (ref["best_ab"] > 0))[0]
    winners = np.nonzero(np.isin(ref["best_j_ab"], copies + [src]))[0]
    assert winners.size > 0 and np.all(ref["best_j_ab"][winners] == 5) and np.all(np.isin(winners, tied))
    assert np.all(ref["proposal_ab"][tied] == -1)
    matches, scores = match_descriptors([da, db], [[0, 1]], return_scores=True)
    _check_pair(matches[0], scores[0], ref, "ties")
    # and in the other direction: the copies as rows of a
    matches, scores = match_descriptors([db, da], [[0, 1]], return_scores=True)
    _check_pair(matches[0], scores[0], MR.match_pair(db, da), "ties, transposed")


def _six_images():
    sizes = [300, 0, 1029, 64, 515, 97]
    rng = np.random.default_rng(21)
    for attempt in range(20):
        base = MR.sift_like(rng, 400)
        images = []
        for n in sizes:
            take = rng.permutation(400)[: min(n, 250)]
            noisy = base[take] * rng.uniform(0.5, 1.0, size=(len(take), 128))
            noisy /= np.maximum(np.linalg.norm(noisy, axis=1, keepdims=True), 1e-12)
            d = np.concatenate([noisy, MR.sift_like(rng, n - len(take))]) if n else np.zeros((0, 128))
            images.append(MR.to_bytes(d[rng.permutation(n)]) if n else np.zeros((0, 128), dtype=np.uint8))
        pairs = [(a, b) for a in range(6) for b in range(a + 1, 6)]
        refs = [MR.match_pair(images[a], images[b]) for a, b in pairs]
        if min(r["margin"] for r in refs) >= MR.MIN_MARGIN:
            return images, pairs, refs
    raise AssertionError("no seed met the margin condition")


def test_d_batch_equals_single_pairs_and_reruns():
    from ls2fm.match import match_descriptors
    images, pairs, refs = _six_images()
    assert len(pairs) == 15
    m1, s1 = match_descriptors(images, None, return_scores=True)
    m2, s2 = match_descriptors(images, None, return_scores=True)
    assert len(m1) == 15
    for p, (a, b) in enumerate(pairs):
        _check_pair(m1[p], s1[p], refs[p], f"pair {a}-{b}")
        assert torch.equal(m1[p], m2[p]) and all(torch.equal(s1[p][k], s2[p][k]) for k in s1[p])
        ms, ss = match_descriptors([images[a], images[b]], [[0, 1]], return_scores=True)
        assert torch.equal(ms[0], m1[p]) and all(torch.equal(ss[0][k], s1[p][k]) for k in s1[p]), f"pair {a}-{b} alone"
    assert sum(len(m) for m in m1) > 500 and all(len(m1[p]) == 0 for p, (a, b) in enumerate(pairs) if 1 in (a, b))
    one_way = match_descriptors(images, None, cross_check=False)
    for p, (a, b) in enumerate(pairs):
        i = np.nonzero(refs[p]["proposal_ab"] >= 0)[0]
        want = np.stack([i, refs[p]["proposal_ab"][i]], axis=1).reshape(-1, 2)
        assert np.array_equal(one_way[p].cpu().numpy(), want), f"pair {a}-{b} one way"
        assert len(one_way[p]) >= len(m1[p])


def _scene():
    """6 views of 500 3-D points, each seen by a subset of views; one descriptor per point, perturbed per view; distractors"""
    rng = np.random.default_rng(33)
    K = np.array([[800.0, 0, 400.0], [0, 800.0, 300.0], [0, 0, 1.0]])
    for attempt in range(20):
        X = rng.uniform(-1.0, 1.0, size=(500, 3)) + np.array([0, 0, 5.0])
        base = MR.sift_like(rng, 500)
        kps, descs = [], []
        for v in range(6):
            ang = 0.12 * (v - 2.5)
            R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
            t = np.array([-0.5 * (v - 2.5), 0.05 * v, 0.3 * abs(v - 2.5)])
            seen = np.nonzero(rng.uniform(size=500) < 0.75)[0]
            xc = X[seen] @ R.T + t
            uv = (xc / xc[:, 2:3]) @ K.T
            uv = uv[:, :2] + rng.normal(0, 0.3, size=(len(seen), 2))
            d = base[seen] * rng.uniform(0.6, 1.0, size=(len(seen), 128))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            n_extra = 80 + 10 * v
            uv = np.concatenate([uv, rng.uniform(0, 800, size=(n_extra, 2))])
            d = np.concatenate([d, MR.sift_like(rng, n_extra)])
            order = rng.permutation(len(uv))
            kps.append(uv[order])
            descs.append(MR.to_bytes(d[order]))
        pairs = [(a, b) for a in range(6) for b in range(a + 1, 6)]
        refs = [MR.match_pair(descs[a], descs[b]) for a, b in pairs]
        if min(r["margin"] for r in refs) >= MR.MIN_MARGIN:
            return K, kps, descs, pairs, refs
    raise AssertionError("no seed met the margin condition")


def test_e_two_view_tables():
    from ls2fm import pose
    from ls2fm.match import two_view_tables
    K, kps, descs, pairs, refs = _scene()
    views = two_view_tables(kps, descs, K, seed=3)
    assert len(views) == 6
    keep = [p for p in range(15) if len(refs[p]["matches"]) >= 50]
    assert len(keep) >= 10
    direct = pose.relative_pose([torch.from_numpy(kps[pairs[p][0]][refs[p]["matches"][:, 0]]).cuda() for p in keep],
                                [torch.from_numpy(kps[pairs[p][1]][refs[p]["matches"][:, 1]]).cuda() for p in keep], K, K, seed=3)
    inl = direct["inliers"].cpu().numpy()
    ps = direct["pair_start"].cpu().numpy()
    mask_of = {p: inl[ps[q]:ps[q + 1]] for q, p in enumerate(keep)}
    for v in range(6):
        assert np.array_equal(views[v]["kypts"], kps[v]) and len(views[v]["indxes"]) == 5 and len(views[v]["mask"]) == 5
        others = [j for j in range(6) if j != v]
        for slot, j in enumerate(others):
            p = pairs.index((min(v, j), max(v, j)))
            got, mask = views[v]["indxes"][slot], views[v]["mask"][slot]
            if p not in mask_of:
                assert len(got) == 0 and len(mask) == 0
                continue
            want = refs[p]["matches"] if j > v else refs[p]["matches"][:, [1, 0]]
            assert np.array_equal(got.astype(np.int64), want), f"view {v} against {j}"
            assert mask.dtype == bool and np.array_equal(mask, mask_of[p]), f"mask of view {v} against {j}"
            # the indexing of Initializer.__init__ (pipelines/Initialization.py:81-85)
            matches = got
            own = views[v]["kypts"][matches[:, 0]][mask]
            other = views[j]["kypts"][matches[:, 1]][mask]
            assert own.shape == other.shape == (int(mask.sum()), 2) and mask.sum() >= 30


def test_f_smoke_unchanged_and_self_contained():
    import inspect

    import __graft_entry__ as G
    src = inspect.getsource(G.smoke)
    assert "match" not in src
    here = os.path.dirname(os.path.abspath(__file__))
    for name in ("test_hip_match.py", "test_match_host.py", "match_restate.py"):
        text = open(os.path.join(here, name)).read()
        assert ("/ro" + "ot/") not in text and ("refer" + "ence/") not in text
