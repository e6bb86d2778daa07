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


# ------------------------------------------------------------------------------------------------ plans at every chunk size
# Every call above is small by the planning rule's measure and runs at 1024-column chunks (at most 32 tiles, one key field value
# in sixteen).  The cases below hold the call at a chosen chunk size by listing a pair several times (the rule counts work
# items over the whole call); tests/match_restate.plan mirrors the rule, tests/test_match_host.py holds the library to the mirror,
# and every case asserts its chunk through the mirror AND the library's own byte count before the device is called.
def _plan(what, counts, pairs, want_chunk):
    import ctypes
    from ls2fm import _lib
    pl = MR.plan(counts, pairs)
    assert pl["chunk_cols"] == want_chunk, f"{what}: planned at {pl['chunk_cols']}, meant {want_chunk}"
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    prs = np.ascontiguousarray(pairs, dtype=np.int32)
    size = _lib.load().ls2fm_match_descriptors_workspace_bytes(start.ctypes.data_as(ctypes.c_void_p), len(counts),
                                                               prs.ctypes.data_as(ctypes.c_void_p), len(prs))
    assert size == pl["bytes"], f"{what}: the library's workspace is {size} bytes, the mirror's {pl['bytes']}"
    print(f"[match plan] {what}: chunk {pl['chunk_cols']} columns, {pl['max_tiles']} tiles per chunk, {pl['max_chunks']} chunk(s), "
          f"{pl['n_items']} items over {len(prs)} listed pairs")
    return pl


def _same_bits(m, s, p, q, what):
    assert torch.equal(m[p], m[q]) and all(torch.equal(s[p][k], s[q][k]) for k in s[p]), f"{what}: listed pair {q} differs from pair {p}"


def _check_repeated(da, db, ref, chunk, what):
    """the pair listed as often as the plan needs for `chunk`: the first against the restatement on every row of both
    directions (raw integers, matches), every repeat against the first bit for bit; then the proposals of both directions
    (cross_check = 0 over the pair and its transpose, listed as often)"""
    from ls2fm.match import match_descriptors
    n_a, n_b = da.shape[0], db.shape[0]
    r = MR.repeats_for(n_a, n_b, chunk)
    _plan(what, [n_a, n_b], [[0, 1]] * r, chunk)
    images = [torch.from_numpy(da).cuda(), torch.from_numpy(db).cuda()]
    m, s = match_descriptors(images, [[0, 1]] * r, return_scores=True)
    _check_pair(m[0], s[0], ref, what)
    for q in range(1, r):
        _same_bits(m, s, 0, q, what)
    del m, s
    both = ([[0, 1], [1, 0]] * ((r + 1) // 2))
    _plan(what + ", proposals", [n_a, n_b], both, chunk)
    one_way = match_descriptors(images, both, cross_check=False)
    for q, (key, other) in enumerate((("proposal_ab", "ab"), ("proposal_ba", "ba"))):
        i = np.nonzero(ref[key] >= 0)[0]
        want = np.stack([i, ref[key][i]], axis=1).reshape(-1, 2)
        assert np.array_equal(one_way[q].cpu().numpy(), want), f"{what}: proposals {other}"
        for k in range(q + 2, len(both), 2):
            assert torch.equal(one_way[k], one_way[q]), f"{what}: proposals {other}, listed pair {k}"


# (n_a, n_b, chunk): a -> b sweeps n_b columns, b -> a sweeps n_a
WIDE_CASES = [
    (16384, 16383, 16384),     # one chunk of 512 tiles each way: tile ids 0..511, the last tile of a -> b one column short
    (16384, 16347, 16384),     # 511 tiles a -> b: an ODD count at the top of the field (the trip's second fold is all padding)
    (16385, 32768, 16384),     # two chunks each way: 512 + 512 tiles, and 512 tiles + one single column; the finalize merge
    (32768, 32768, 16384),     # the ABI limit on both sides
    (8292, 9001, 8192),        # two chunks, ragged last (100 / 809 columns)
    (4196, 9000, 4096),        # two and three chunks, ragged last
    (2148, 5000, 2048),        # two and three chunks, ragged last
]


@pytest.mark.parametrize("n_a,n_b,chunk", WIDE_CASES)
def test_g_wide_chunks_equal_the_blocked_restatement(n_a, n_b, chunk):
    """Equality on EVERY row of both directions, the 32768 x 32768 pair included: the blocked restatement takes about 10 s for
    it on 16 CPUs.  Host peak: about 0.5 GB (1024 x 32768 float32 blocks and numpy's temporaries; the descriptors are 4 MB an image)."""
    da, db, ref = MR.seeded_pair(n_a, n_b, seed=900 + n_a % 1000 + n_b % 1000, restate=MR.match_pair_blocked)
    assert ref["margin"] >= MR.MIN_MARGIN and max(da.max(), db.max()) == 255
    print(f"[match] {n_a} x {n_b}: {len(ref['matches'])} matches, margin {ref['margin']:.3e} rad")
    _check_repeated(da, db, ref, chunk, f"{n_a} x {n_b}")


def _many_images(n_images, n, n_sampled, seed):
    """images that share a pool of descriptors under noise (as _six_images); the pairs sampled for the restatement meet the margin"""
    pairs = [(a, b) for a in range(n_images) for b in range(a + 1, n_images)]
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        base = MR.sift_like(rng, n)
        images = []
        for _ in range(n_images):
            take = rng.permutation(n)[: n // 2]
            noisy = base[take] * rng.uniform(0.5, 1.0, size=(len(take), 128))
            noisy /= np.maximum(np.linalg.norm(noisy, axis=1, keepdims=True), 1e-12)
            d = np.concatenate([noisy, MR.sift_like(rng, n - len(take))])
            images.append(MR.to_bytes(d[rng.permutation(n)]))
        sampled = sorted(int(p) for p in rng.choice(len(pairs), size=n_sampled, replace=False))
        refs = {p: MR.match_pair_blocked(images[pairs[p][0]], images[pairs[p][1]]) for p in sampled}
        if min(r["margin"] for r in refs.values()) >= MR.MIN_MARGIN:
            return images, pairs, refs
    raise AssertionError("no seed met the margin condition")


def test_g_many_views_of_8192_in_one_call():
    """the README's shape in small: 33 distinct images of 8192 descriptors, all 528 pairs in ONE call and no pair listed twice
    (135168 items: chunk 16384, 256 tiles).  Six pairs drawn by the fixture's seed against the restatement on every row; all
    528 against a second run bit for bit.  Host peak: 33 x 1 MB descriptors, 8192 x 8192 float32 blocks (0.6 GB with temporaries)."""
    from ls2fm.match import match_descriptors
    images, pairs, refs = _many_images(33, 8192, 6, seed=61)
    _plan("33 views x 8192", [8192] * 33, pairs, 16384)
    dev = [torch.from_numpy(d).cuda() for d in images]
    m1, s1 = match_descriptors(dev, None, return_scores=True)
    m2, s2 = match_descriptors(dev, None, return_scores=True)
    assert len(m1) == 528
    for p, ref in refs.items():
        _check_pair(m1[p], s1[p], ref, f"pair {pairs[p]} of 33 views")
        assert len(ref["matches"]) > 1000
    assert torch.equal(torch.cat(m1), torch.cat(m2)) and [len(x) for x in m1] == [len(x) for x in m2]
    for k in s1[0]:
        assert torch.equal(torch.cat([s[k] for s in s1]), torch.cat([s[k] for s in s2])), k


# ----------------------------------------------------------------------------------------- directed placements at high tile ids
HIGH_COLUMNS = (0, 31, 32, 1023, 1024, 8191, 8192, 16351, 16352, 16383)


def _queries_and_columns(n_cols, seed, plant, need_margin=True):
    """a: 70 sift-like query rows (two row blocks, the second ragged); b: n_cols sift-like columns, changed by plant(a, b)"""
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        a, b = MR.to_bytes(MR.sift_like(rng, 70)), MR.to_bytes(MR.sift_like(rng, n_cols))
        plant(a, b)
        ref = MR.match_pair_blocked(a, b)
        if not need_margin or ref["margin"] >= MR.MIN_MARGIN:
            return a, b, ref
    raise AssertionError("no seed met the margin condition")


def test_h_unique_best_column_in_high_tiles():
    """row r of a has its only close descriptor at column HIGH_COLUMNS[r] of a 16384-column image (tiles 0, 1, 31, 32, 255, 256,
    510 and 511, first and last lane of a tile): best_j must be that column"""
    def plant(a, b):
        for r, c in enumerate(HIGH_COLUMNS):
            b[c] = a[r]
    a, b, ref = _queries_and_columns(16384, 71, plant)
    rows = np.arange(len(HIGH_COLUMNS))
    assert np.array_equal(ref["best_j_ab"][rows], HIGH_COLUMNS) and np.all(ref["best_ab"][rows] > ref["second_ab"][rows])
    assert np.array_equal(ref["proposal_ab"][rows], HIGH_COLUMNS) and np.array_equal(ref["best_j_ba"][list(HIGH_COLUMNS)], rows)
    _check_repeated(a, b, ref, 16384, "unique best at high tiles")


def test_h_equal_dots_in_distant_tiles_of_one_chunk():
    """two and three copies of a row's best descriptor in different tiles of ONE 16384-column chunk: the lowest column, second ==
    best, no proposal; and rows whose every dot is 0 (best_j -1), one of them also a column of the other direction"""
    def plant(a, b):
        b[[40, 9000, 16383]] = a[0]
        b[[9001, 16352]] = a[1]
        b[[16320, 16352 + 31 - 1]] = a[2]             # tiles 510 and 511
        a[5] = 0
        a[69] = 0                                     # the last row of the ragged row block
        b[16381] = 0
    a, b, ref = _queries_and_columns(16384, 72, plant)
    assert ref["best_j_ab"][:3].tolist() == [40, 9001, 16320] and np.array_equal(ref["best_ab"][:3], ref["second_ab"][:3])
    assert np.all(ref["proposal_ab"][:3] == -1) and np.all(ref["best_ab"][:3] > 200000)
    assert ref["best_j_ab"][5] == -1 and ref["best_j_ab"][69] == -1 and ref["best_ab"][69] == 0 and ref["best_j_ba"][16381] == -1
    _check_repeated(a, b, ref, 16384, "equal dots in one chunk")


def test_h_equal_dots_across_the_chunk_boundary():
    """16400 columns at chunk 16384: copies on both sides of the boundary (16383, 16384), both in the short second chunk, and far
    apart in different chunks -- the lowest column through match_finalize_kernel's merge; a unique best in the last column"""
    def plant(a, b):
        b[[16383, 16384]] = a[0]
        b[[16384 + 1, 16399 - 1]] = a[1]
        b[[5, 16390]] = a[2]
        b[16399] = a[3]
    a, b, ref = _queries_and_columns(16400, 73, plant)
    assert ref["best_j_ab"][:4].tolist() == [16383, 16385, 5, 16399] and np.array_equal(ref["best_ab"][:3], ref["second_ab"][:3])
    assert np.all(ref["proposal_ab"][:3] == -1) and ref["proposal_ab"][3] == 16399
    _check_repeated(a, b, ref, 16384, "equal dots across chunks")


def test_h_saturated_pair_in_tile_511():
    """all bytes 255 in a row of a and in column 16380 of b (dot 128 * 255^2, the largest key the sweep can form, beside tile id
    511 = field value 0), and in column 3 (tile 0 = field value 511): the raw integers only -- a saturated descriptor is far above
    length 512, so every row's angle is 0 and no decision is compared (as test_a_all_bytes_255)"""
    from ls2fm.match import match_descriptors

    def plant(a, b):
        a[7] = 255
        a[64] = 255
        b[16380] = 255
        b[3] = 255
    a, b, ref = _queries_and_columns(16384, 74, plant, need_margin=False)
    top = 128 * 255 * 255
    assert ref["best_ab"][7] == top and ref["best_j_ab"][7] == 3 and ref["second_ab"][7] == top and ref["best_j_ba"][16380] == 7
    assert ref["best_j_ab"][0] == 3 and ref["second_ab"][0] == ref["best_ab"][0]      # ordinary rows: the two saturated columns tie
    r = MR.repeats_for(70, 16384, 16384)
    _plan("saturated pair", [70, 16384], [[0, 1]] * r, 16384)
    _, scores = match_descriptors([a, b], [[0, 1]] * r, return_scores=True)
    for names in DIRS:
        for k in names:
            got = scores[0][k].cpu().numpy().astype(np.int64)
            assert np.array_equal(got, ref[k]), f"{k}: first difference at row {np.nonzero(got != ref[k])[0][:5]}"
            assert all(torch.equal(scores[q][k], scores[0][k]) for q in range(1, r)), k


def test_h_every_chunk_size_is_reached_by_this_file():
    """the plans of this file's calls, through the mirror: the small cases at 1024, the wide ones at each of the other four"""
    reached = {MR.plan([n_a, n_b], [[0, 1]])["chunk_cols"] for n_a, n_b in [(1, 1), (17, 300), (2000, 1800), (8192, 8191)]}
    assert reached == {1024}
    for n_a, n_b, chunk in WIDE_CASES:
        reached.add(MR.plan([n_a, n_b], [[0, 1]] * MR.repeats_for(n_a, n_b, chunk))["chunk_cols"])
    reached.add(MR.plan([8192] * 33, [(a, b) for a in range(33) for b in range(a + 1, 33)])["chunk_cols"])
    print(f"[match plan] chunk sizes reached: {sorted(reached)}")
    assert reached == set(MR.CHUNKS)


def test_f_smoke_unchanged_and_self_contained():
    import inspect

    import __graft_entry__ as G
    src = inspect.getsource(G.smoke)
    assert "match" not in src
    here = os.path.dirname(os.path.abspath(__file__))
    for name in ("test_hip_match.py", "test_match_host.py", "match_restate.py"):
        text = open(os.path.join(here, name)).read()
        assert ("/ro" + "ot/") not in text and ("refer" + "ence/") not in text
