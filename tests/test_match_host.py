"""Descriptor matching, host side (no GPU): the C ABI's symbols and refusals, assemble_n_views against a literal restatement of
preparation/main.py:177-247's index arithmetic, and the numpy restatement (tests/match_restate.py) on hand-built cases."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_restate as MR  # noqa: E402

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


def _lib():
    from ls2fm import _lib
    return _lib.load()


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exported():
    from ls2fm import _lib
    lib = _lib.load()
    for name in ("ls2fm_match_descriptors_workspace_bytes", "ls2fm_match_descriptors"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ls2fm.h")).read()
    assert "ls2fm_match_descriptors(" in header and "LS2FM_MATCH_MAX_DESCRIPTORS 32768" in header
    assert lib.ls2fm_abi_version() == 13


def test_workspace_query_and_refusals():
    lib = _lib()
    start, c_start = _i32([0, 100, 100, 300])
    pairs, c_pairs = _i32([[0, 1], [0, 2], [1, 2]])
    n = lib.ls2fm_match_descriptors_workspace_bytes(c_start, 3, c_pairs, 3)
    assert n > 300 * 128
    null = ctypes.c_void_p(0)
    assert lib.ls2fm_match_descriptors_workspace_bytes(null, 3, c_pairs, 3) == INVALID
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_start, 3, null, 3) == INVALID
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_start, 0, c_pairs, 3) == INVALID
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_start, 3, c_pairs, -1) == INVALID
    bad, c_bad = _i32([[0, 3]])
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_start, 3, c_bad, 1) == INVALID            # pair index out of range
    bad2, c_bad2 = _i32([[-1, 0]])
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_start, 3, c_bad2, 1) == INVALID
    down, c_down = _i32([0, 100, 50, 300])
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_down, 3, c_pairs, 3) == INVALID           # not rising
    off, c_off = _i32([1, 100, 100, 300])
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_off, 3, c_pairs, 3) == INVALID            # not from 0
    big, c_big = _i32([0, 32769, 32800])
    one, c_one = _i32([[0, 1]])
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_big, 2, c_one, 1) == UNSUPPORTED          # above COLMAP's cap
    cap, c_cap = _i32([0, 32768, 32800])
    assert lib.ls2fm_match_descriptors_workspace_bytes(c_cap, 2, c_one, 1) > 0


def test_call_refusals_enqueue_nothing():
    """every refusal is decided from the host arrays before the first runtime call: the calls below pass pointers that are
    not device memory and a NULL stream, and return without touching either"""
    lib = _lib()
    start, c_start = _i32([0, 64, 128])
    pairs, c_pairs = _i32([[0, 1]])
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(1 << 20)      # 16-byte aligned, never dereferenced on a refusal

    def call(desc=fake, st=c_start, n_img=2, pr=c_pairs, n_pr=1, ratio=0.8, dist=0.7, idx=fake, num=fake, ws=fake):
        return lib.ls2fm_match_descriptors(desc, st, n_img, pr, n_pr, ratio, dist, 1, idx, num, null, null, null, ws, null)

    assert call(desc=null) == INVALID
    assert call(st=null) == INVALID
    assert call(pr=null) == INVALID
    assert call(idx=null) == INVALID
    assert call(num=null) == INVALID
    assert call(n_img=0) == INVALID
    assert call(ratio=float("nan")) == INVALID
    assert call(dist=-1.0) == INVALID
    assert call(desc=ctypes.c_void_p((1 << 20) + 4)) == INVALID
    assert call(ws=null) == WORKSPACE
    bad, c_bad = _i32([[0, 2]])
    assert call(pr=c_bad) == INVALID
    big, c_big = _i32([0, 40000, 40100])
    assert call(st=c_big) == UNSUPPORTED
    assert call(n_pr=0) == OK            # no pairs: nothing to do


# ------------------------------------------------------------------------------------------------------- assemble_n_views
def _main_py_tables(keypoints, matches, masks_in):
    """preparation/main.py:177-247's arithmetic, literally (names as there), with the documented deviation for empty pairs"""
    n = len(keypoints)
    matches_full, mask_inlier = [], []
    it = iter(zip(matches, masks_in))
    for idx_i in range(n):
        for idx_ij in range(n - idx_i - 1):
            m, k = next(it)
            if len(m) < 50:
                matches_full.append(np.uint32(np.array([])))
                mask_inlier.append(np.zeros(0, dtype=bool))
            else:
                matches_full.append(m)
                mask_inlier.append(k)
    views = []
    for iter_ind in range(n):
        other_indx = [j for j in range(n) if j != iter_ind]
        tem_indx = [int((2 * n - iter_ind - 1) * iter_ind / 2 + j - iter_ind - 1) if j > iter_ind
                    else int((2 * n - j - 1) * j / 2 + iter_ind - j - 1) for j in other_indx]
        matches_new = [matches_full[tem_indx[i]] if (i >= iter_ind) | (len(matches_full[tem_indx[i]]) == 0)
                       else np.concatenate([matches_full[tem_indx[i]][:, 1:], matches_full[tem_indx[i]][:, :1]], axis=-1)
                       for i in range(len(tem_indx))]
        views.append(dict(kypts=keypoints[iter_ind], indxes=matches_new, mask=[mask_inlier[t] for t in tem_indx]))
    return views


def test_assemble_n_views_against_main_py():
    from ls2fm.match import assemble_n_views, exhaustive_pairs
    rng = np.random.default_rng(3)
    n = 5
    counts = [300, 280, 260, 310, 290]
    keypoints = [rng.uniform(0, 640, size=(c, 2)) for c in counts]
    pairs = exhaustive_pairs(n)
    assert pairs.tolist() == [[a, b] for a in range(n) for b in range(a + 1, n)]
    matches, masks = [], []
    for q, (a, b) in enumerate(pairs):
        m = {3: 0, 6: 37}.get(q, 60 + 7 * q)                    # one empty pair, one below 50
        i = np.sort(rng.choice(counts[a], size=m, replace=False))
        j = rng.choice(counts[b], size=m, replace=False)
        matches.append(np.stack([i, j], axis=1).astype(np.uint32).reshape(-1, 2))
        masks.append(rng.uniform(size=m) < 0.7)
    got = assemble_n_views(keypoints, matches, masks)
    want = _main_py_tables(keypoints, matches, masks)
    assert len(got) == n
    for v in range(n):
        assert np.array_equal(got[v]["kypts"], want[v]["kypts"])
        assert len(got[v]["indxes"]) == n - 1 and len(got[v]["mask"]) == n - 1
        for g, w, gm, wm in zip(got[v]["indxes"], want[v]["indxes"], got[v]["mask"], want[v]["mask"]):
            assert g.shape == w.shape and np.array_equal(g, w)
            assert gm.dtype == bool and np.array_equal(gm, wm) and len(gm) == len(g)
    # the two filtered pairs are empty in both of their views, and the own-index column is column 0
    assert len(got[0]["indxes"][3]) == 0 and len(got[4]["indxes"][0]) == 0          # pair 3 = (0, 4)
    assert len(got[1]["indxes"][3]) == 0 and len(got[4]["indxes"][1]) == 0          # pair 6 = (1, 4), 37 matches
    assert np.array_equal(got[2]["indxes"][0][:, 0], matches[1][:, 1]) and got[2]["indxes"][0][:, 0].max() < counts[2]
    with pytest.raises(ValueError):
        assemble_n_views(keypoints, matches[:-1], masks[:-1])


# ------------------------------------------------------------------------------------------------ the restatement by hand
def _unit(k, value=200):
    """`value` in the four slots 4k .. 4k + 3: two such descriptors with 255 have dot 260100 (angle 0.125)"""
    d = np.zeros(128, dtype=np.uint8)
    d[4 * k:4 * k + 4] = value
    return d


def test_restatement_tied_maximum_rejects():
    a = np.stack([_unit(0, 255), _unit(1, 255)])
    b = np.stack([_unit(0, 255), _unit(0, 255), _unit(1, 255)])         # b0 == b1: row 0 has a tied maximum
    r = MR.match_pair(a, b)
    assert r["best_ab"][0] == 4 * 255 * 255 and r["second_ab"][0] == r["best_ab"][0] and r["best_j_ab"][0] == 0     # the lowest j
    assert r["proposal_ab"][0] == -1                                    # angle(best) >= 0.8 angle(second)
    assert r["proposal_ab"][1] == 2 and r["matches"].tolist() == [[1, 2]]


def test_restatement_zero_descriptor_has_no_match():
    a = np.stack([np.zeros(128, dtype=np.uint8), _unit(5, 255)])
    b = np.stack([_unit(5, 255), _unit(6, 255)])
    r = MR.match_pair(a, b)
    assert r["best_ab"][0] == 0 and r["best_j_ab"][0] == -1 and r["proposal_ab"][0] == -1
    assert r["best_ba"][1] == 0 and r["proposal_ba"][1] == -1
    assert r["matches"].tolist() == [[1, 0]]


def _dot_pair(best, second):
    """a [1,128], b [2,128] with dot(a, b0) = best and dot(a, b1) = second exactly (a = 128 in 16 slots + 1 in one)"""
    a = np.zeros(128, dtype=np.uint8)
    a[:16] = 128
    a[16] = 1

    def col(d):
        q, r = divmod(d, 128)
        c = np.zeros(128, dtype=np.uint8)
        full, rest = divmod(q, 255)
        assert full < 16
        c[:full] = 255
        c[full] = rest
        c[16] = r
        return c
    b = np.stack([col(best), col(second)])
    assert (a.astype(np.int64) @ b.astype(np.int64).T).tolist() == [best, second]
    return a[None], b


def test_restatement_thresholds_inside_and_outside():
    # max_distance 0.7: acos(d / 262144) <= 0.7  <=>  d >= 262144 cos 0.7 (not an integer)
    edge = 262144 * np.cos(0.7)
    for best, want in ((int(np.ceil(edge)), 0), (int(np.floor(edge)), -1)):
        a, b = _dot_pair(best, 0)
        r = MR.match_pair(a, b, cross_check=False)
        assert r["best_ab"][0] == best and r["proposal_ab"][0] == want
    # ratio 0.8 at best = 250000 (angle 0.30500...): the second dot at which angle(best) = 0.8 angle(second)
    best = 250000
    edge = 262144 * np.cos(np.arccos(best / 262144) / 0.8)
    lo, hi = int(np.floor(edge)), int(np.ceil(edge))
    assert lo < hi < best
    a, b = _dot_pair(best, lo)
    assert MR.match_pair(a, b, cross_check=False)["proposal_ab"][0] == 0        # second a little further: accepted
    a, b = _dot_pair(best, hi)
    assert MR.match_pair(a, b, cross_check=False)["proposal_ab"][0] == -1       # second a little closer: rejected
    # a dot above 262144 has angle 0 (the min with 1)
    assert MR.angle(300000) == 0.0


def test_restatement_cross_check_removes_one_sided():
    # a0 and a1 both point at b0; b0 prefers a1
    a = np.stack([_unit(0, 230) + _unit(1, 30), _unit(0, 250)])
    b = np.stack([_unit(0, 255), _unit(9, 255)])
    r = MR.match_pair(a, b, cross_check=False)
    assert r["matches"].tolist() == [[0, 0], [1, 0]]
    r = MR.match_pair(a, b, cross_check=True)
    assert r["proposal_ba"][0] == 1 and r["matches"].tolist() == [[1, 0]]


def test_seeded_fixture_meets_margin_and_truth():
    da, db, ref = MR.seeded_pair(400, 360, seed=11)
    assert ref["margin"] >= MR.MIN_MARGIN
    assert max(da.max(), db.max()) == 255
    assert 100 < len(ref["matches"]) <= 360 and np.all(np.diff(ref["matches"][:, 0]) > 0)


# ------------------------------------------------------------------------------------------- the planning rule and its mirror
def _exhaustive(n):
    return [[a, b] for a in range(n) for b in range(a + 1, n)]


# (images, pairs, the chunk the rule gives by hand).  Items of a pair at chunk c: ceil(n_a / 64) ceil(n_b / c) + ceil(n_b / 64) ceil(n_a / c)
PLAN_TABLE = [
    ([100, 100, 300], _exhaustive(3), 1024),                    # tiny: halves all the way down
    ([8192, 8191], [[0, 1]], 1024),                             # 256 items at 16384, 2048 at 1024: the suite's largest pair so far
    ([16384, 16384], [[0, 1]] * 16, 16384),                     # 16 x 512 = 8192 items: exactly the target, stays
    ([16384, 16384, 16320], [[0, 1]] * 15 + [[0, 2]], 8192),    # 15 x 512 + 511 = 8191: one item short, halves once (15 x 1024 + 1022)
    ([16384, 16384, 64], [[0, 1]] * 16 + [[2, 2]], 16384),      # 8194: one pair of two items above
    ([16385, 32768], [[0, 1]] * 6, 16384),                      # 6 x (257 x 2 + 512 x 2) = 9228
    ([16385, 32768], [[0, 1]] * 5, 8192),                       # 7690 -> at 8192: 5 x (257 x 4 + 512 x 3) = 12820
    ([8292, 8292], [[0, 1]] * 16, 8192),                        # 16 x 260 = 4160 -> 16 x 520 = 8320
    ([8292, 8292], [[0, 1]] * 15, 4096),                        # 15 x 520 = 7800: one repeat short -> 15 x 780
    ([4196, 4196], [[0, 1]] * 32, 4096),                        # 32 x 132 = 4224 -> 32 x 264 = 8448
    ([4196, 4196], [[0, 1]] * 31, 2048),                        # 31 x 264 = 8184: eight items short -> 31 x 396
    ([2148, 2148], [[0, 1]] * 61, 2048),                        # 61 x 68 = 4148 -> 61 x 136 = 8296
    ([2148, 2148], [[0, 1]] * 60, 1024),                        # 60 x 136 = 8160 -> 60 x 204 (and 1024 is the floor)
    ([8192] * 33, _exhaustive(33), 16384),                      # the README's shape in small: 528 x 256 items
    ([0, 5000, 0], _exhaustive(3), 1024),                       # empty images: no items at any chunk
]


def _telling_neighbours(counts, pairs, want):
    """the neighbouring chunk sizes at which some job of the call has another number of chunks, so another byte count"""
    widest = max([0] + [max(counts[a], counts[b]) for a, b in pairs if counts[a] and counts[b]])
    return [c for c in (want // 2, want * 2) if c in MR.CHUNKS and min(c, want) < widest]


@pytest.mark.parametrize("row", range(len(PLAN_TABLE)))
def test_plan_mirror_equals_the_library_workspace_query(row):
    """ls2fm_match_descriptors_workspace_bytes against tests/match_restate.plan.  The partial array holds one entry per (row,
    chunk), so where an image is wider than the next smaller chunk the byte count differs between chunk sizes (asserted where
    it applies): equal bytes then show the library chose the chunk the mirror chose, and the table pins the mirror by hand."""
    counts, pairs, want = PLAN_TABLE[row]
    got = MR.plan(counts, pairs)
    assert got["chunk_cols"] == want, got
    start, c_start = _i32(np.concatenate([[0], np.cumsum(counts)]))
    prs, c_pairs = _i32(pairs)
    size = _lib().ls2fm_match_descriptors_workspace_bytes(c_start, len(counts), c_pairs, len(pairs))
    assert size == got["bytes"], (size, got)
    for c in _telling_neighbours(counts, pairs, want):
        assert MR.plan(counts, pairs, force_chunk=c)["bytes"] != size, c


def test_plan_table_lands_on_every_chunk_size_and_both_sides_of_the_target():
    chunks = {MR.plan(c, p)["chunk_cols"] for c, p, _ in PLAN_TABLE}
    assert chunks == set(MR.CHUNKS)
    for chunk in MR.CHUNKS:                                      # and at each, a row whose byte count tells it from both neighbours
        assert any(w == chunk and len(_telling_neighbours(c, p, w)) == (1 if chunk in (1024, 16384) else 2) for c, p, w in PLAN_TABLE), chunk
    items = [MR.plan(c, p, force_chunk=16384)["n_items"] for c, p, _ in PLAN_TABLE]
    assert {8191, 8192, 8194} <= set(items)
    assert MR.repeats_for(16384, 16383, 16384) == 16 and MR.repeats_for(2148, 2148, 2048) == 61


@pytest.mark.parametrize("n_a,n_b,seed,block", [(400, 360, 11, 64), (200, 700, 7, 1024), (17, 300, 117, 7), (1, 1, 101, 1024), (2000, 1800, 2100, 333)])
def test_blocked_restatement_equals_the_full_one(n_a, n_b, seed, block):
    da, db, ref = MR.seeded_pair(n_a, n_b, seed=seed, shared=0.5 if n_a > 1 else 1.0)
    db = db.copy()
    if n_b > 500:                                                # the fixture of test_c_ties: a tied maximum in distant blocks
        db[[5, 31, 32, 33, 100, 401]] = db[int(ref["matches"][ref["matches"][:, 1] > 401][0, 1])]
        ref = MR.match_pair(da, db)
    got = MR.match_pair_blocked(da, db, block=block)
    assert set(got) == set(ref) and got["margin"] == ref["margin"]
    for k in ref:
        if k != "margin":
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    empty = MR.match_pair_blocked(da, np.zeros((0, 128), dtype=np.uint8))
    full = MR.match_pair(da, np.zeros((0, 128), dtype=np.uint8))
    assert all(np.array_equal(empty[k], full[k]) for k in full if k != "margin") and len(empty["matches"]) == 0
