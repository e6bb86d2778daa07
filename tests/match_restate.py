"""The descriptor-matching rule of include/ls2fm.h ("Descriptor matching") in numpy: COLMAP's CPU SIFT matcher with its
defaults, written from the stated rule and not from the kernel.  Test infrastructure: the checker of tests/test_hip_match.py.

Products: a float32 matmul cast to int64 (every product and partial sum is an integer below 2^24, so float32 is exact; a row
sample is asserted against an int64 matmul).  Best: first-maximum argmax.  Second: the maximum after masking the winner.
Comparisons: fp64 arccos.  `margin` is the smallest distance of any row's two comparisons from equality (radians): fixtures
whose decisions are compared must keep it >= MIN_MARGIN, so the decision is the same in COLMAP's fp32, here and on the device.
"""
import numpy as np

MIN_MARGIN = 1e-6


def products(da, db):
    """exact integer dot products [n_a, n_b] (int64)"""
    da = np.ascontiguousarray(da, dtype=np.uint8).reshape(-1, 128)
    db = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1, 128)
    d = (da.astype(np.float32) @ db.astype(np.float32).T).astype(np.int64)
    if da.shape[0] and db.shape[0]:
        rows = np.unique(np.linspace(0, da.shape[0] - 1, min(da.shape[0], 16)).astype(np.int64))
        assert np.array_equal(d[rows], da[rows].astype(np.int64) @ db.astype(np.int64).T), "float32 products are not exact"
    return d


def angle(d):
    return np.arccos(np.minimum(np.asarray(d, dtype=np.float64) / 262144.0, 1.0))


def decide(best, j, second, max_ratio=0.8, max_distance=0.7):
    """the two comparisons on a row's raw integers (best, its column j, second) -> (best, best_j, second, proposal, margin)"""
    ab, as_ = angle(best), angle(second)
    has = best > 0
    ok = has & ~(ab > max_distance) & ~(ab >= max_ratio * as_)
    best_j = np.where(has, j, -1)
    margins = np.minimum(np.abs(ab - max_distance), np.abs(ab - max_ratio * as_))[has]
    return best, best_j, second, np.where(ok, j, -1), (float(margins.min()) if margins.size else np.inf)


def one_way(d, max_ratio=0.8, max_distance=0.7):
    """d [n, m] int64 -> (best, best_j, second, proposal, margin) per row; best_j / proposal are -1 where there is none"""
    n, m = d.shape
    if m == 0 or n == 0:
        z = np.zeros(n, dtype=np.int64)
        return z, z - 1, z.copy(), z - 1, np.inf
    rows = np.arange(n)
    j = np.argmax(d, axis=1)                          # the first maximum: the lowest j
    best = np.maximum(d[rows, j], 0)
    masked = d.copy()
    masked[rows, j] = -1
    second = np.maximum(masked.max(axis=1), 0) if m > 1 else np.zeros(n, dtype=np.int64)
    return decide(best, j, second, max_ratio, max_distance)


def match_pair(da, db, max_ratio=0.8, max_distance=0.7, cross_check=True):
    """-> dict(matches int64 [M,2] in increasing i, the raw integers of both directions, margin)"""
    d = products(da, db)
    return _assemble(one_way(d, max_ratio, max_distance), one_way(d.T, max_ratio, max_distance), cross_check)


def _assemble(ab, ba, cross_check):
    b_ab, j_ab, s_ab, p_ab, m_ab = ab
    b_ba, j_ba, s_ba, p_ba, m_ba = ba
    i = np.nonzero(p_ab >= 0)[0]
    if cross_check:
        i = i[p_ba[p_ab[i]] == i]
    matches = np.stack([i, p_ab[i]], axis=1).astype(np.int64).reshape(-1, 2)
    return dict(matches=matches, best_ab=b_ab, best_j_ab=j_ab, second_ab=s_ab, proposal_ab=p_ab, best_ba=b_ba, best_j_ba=j_ba,
                second_ba=s_ba, proposal_ba=p_ba, margin=min(m_ab, m_ba))


# ------------------------------------------------------------------------------------------- the same rule over row blocks
BLOCK_ROWS = 1024


def one_way_blocked(da, db, max_ratio=0.8, max_distance=0.7, block=BLOCK_ROWS):
    """one_way over the rows of da against the columns db without holding the product matrix: `block` rows at a time, the
    products kept in float32 (exact: integers below 2^24; the first and last row of every block are asserted against int64).
    Peak: block x n_b float32 twice (the block and numpy's temporaries), 256 MB at 1024 x 32768."""
    da = np.ascontiguousarray(da, dtype=np.uint8).reshape(-1, 128)
    db = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1, 128)
    n, m = da.shape[0], db.shape[0]
    if m == 0 or n == 0:
        z = np.zeros(n, dtype=np.int64)
        return z, z - 1, z.copy(), z - 1, np.inf
    fbt = np.ascontiguousarray(db.astype(np.float32).T)
    ibt = db.astype(np.int64).T
    best, j, second = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        d = da[r0:r1].astype(np.float32) @ fbt
        for r in (r0, r1 - 1):
            assert np.array_equal(d[r - r0].astype(np.int64), da[r].astype(np.int64) @ ibt), "float32 products are not exact"
        rows = np.arange(r1 - r0)
        jj = np.argmax(d, axis=1)                     # the first maximum: the lowest j
        best[r0:r1] = d[rows, jj].astype(np.int64)
        d[rows, jj] = -1.0
        if m > 1:
            second[r0:r1] = np.maximum(d.max(axis=1), 0.0).astype(np.int64)
        j[r0:r1] = jj
    return decide(best, j, second, max_ratio, max_distance)


def match_pair_blocked(da, db, max_ratio=0.8, max_distance=0.7, cross_check=True, block=BLOCK_ROWS):
    """match_pair's outputs, both directions by one_way_blocked (the b -> a direction recomputes the transposed products)"""
    return _assemble(one_way_blocked(da, db, max_ratio, max_distance, block), one_way_blocked(db, da, max_ratio, max_distance, block),
                     cross_check)


# ------------------------------------------------------------------------------------------------ the planning rule, mirrored
WAVE_ROWS, TILE_COLS, MAX_CHUNK, MIN_CHUNK, TARGET_ITEMS = 64, 32, 16384, 1024, 8192
CHUNKS = (1024, 2048, 4096, 8192, 16384)
JOB_BYTES = 40           # one directed job: eight int32 and one int64


def plan(counts, pairs, force_chunk=None):
    """the plan of one ls2fm_match_descriptors call, from the rule csrc/match.hip states: a work item is one wave = 64 rows of a
    directed job against one chunk of its columns; chunks start at 16384 columns and halve while the call has fewer than 8192
    items, down to 1024.  Workspace: the job table (2 P + 1 entries), the pairs' first-row prefix (P + 1 int32), per descriptor
    128 * sum (int32) and the 128 signed bytes, per directed row the proposal (int32), per (directed row, chunk) one 16-byte
    partial -- each array rounded up to 256 bytes.
    -> dict(chunk_cols, n_items, n_rows, n_parts, bytes, max_chunks, max_tiles); force_chunk: the layout at that chunk instead"""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    na, nb = counts[pairs[:, 0]], counts[pairs[:, 1]]
    up = lambda x, q: (x + q - 1) // q

    def items_at(chunk):
        return int((up(na, WAVE_ROWS) * up(nb, chunk) + up(nb, WAVE_ROWS) * up(na, chunk)).sum())
    chunk = MAX_CHUNK
    while chunk > MIN_CHUNK and items_at(chunk) < TARGET_ITEMS:
        chunk //= 2
    if force_chunk is not None:
        chunk = int(force_chunk)
    P, N = pairs.shape[0], int(counts.sum())
    n_rows = int((na + nb).sum())
    n_parts = int((na * up(nb, chunk) + nb * up(na, chunk)).sum())
    al = lambda b: (b + 255) // 256 * 256
    size = al(JOB_BYTES * (2 * P + 1)) + al(4 * (P + 1)) + al(4 * N) + al(128 * N) + al(4 * n_rows) + al(16 * n_parts)
    widest = int(max(na.max(), nb.max())) if P else 0
    return dict(chunk_cols=chunk, n_items=items_at(chunk), n_rows=n_rows, n_parts=n_parts, bytes=size,
                max_chunks=up(widest, chunk), max_tiles=up(min(widest, chunk), TILE_COLS))


def repeats_for(n_a, n_b, chunk):
    """the smallest number of times the pair (n_a, n_b) is listed in one call for the plan to land on `chunk`"""
    for r in range(1, 4097):
        got = plan([n_a, n_b], [[0, 1]] * r)["chunk_cols"]
        if got == chunk:
            return r
        if got > chunk:
            break
    raise AssertionError(f"no repeat count of a {n_a} x {n_b} pair plans at chunk {chunk}")


# ------------------------------------------------------------------------------------------------------------ seeded fixtures
def sift_like(rng, n):
    """gamma-distributed histograms, clipped at 0.2 of the norm, normalised to length 512, rounded to bytes (float64 [n,128])"""
    h = rng.gamma(0.6, 1.0, size=(n, 128))
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    h = np.minimum(h, 0.2)
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    return h


def to_bytes(h):
    return np.clip(np.rint(h * 512.0), 0, 255).astype(np.uint8)


def seeded_pair(n_a, n_b, seed, shared=0.5, loud=True, restate=None):
    """two images that share `shared` of the smaller one's descriptors under multiplicative noise 0.5 - 1.0; loud: a few
    descriptors are concentrated so that bytes up to 255 occur.  Tries seeds from `seed` on until the restatement's margin is
    >= MIN_MARGIN (asserted) -> (da, db, restated result).  restate: match_pair (default) or match_pair_blocked"""
    restate = restate or match_pair
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        n_s = int(min(n_a, n_b) * shared)
        base = sift_like(rng, n_s)
        a = np.concatenate([base, sift_like(rng, n_a - n_s)])
        noisy = base * rng.uniform(0.5, 1.0, size=base.shape)
        noisy /= np.maximum(np.linalg.norm(noisy, axis=1, keepdims=True), 1e-12)
        b = np.concatenate([noisy, sift_like(rng, n_b - n_s)])
        da, db = to_bytes(a[rng.permutation(n_a)]), to_bytes(b[rng.permutation(n_b)])
        if loud:
            for d in (da, db):
                k = max(1, d.shape[0] // 50)
                rows = rng.choice(d.shape[0], size=k, replace=False)
                d[rows, rng.integers(0, 128, size=k)] = 255
                d[rows[: (k + 1) // 2], rng.integers(0, 128, size=(k + 1) // 2)] = rng.integers(128, 256, size=(k + 1) // 2)
        ref = restate(da, db)
        if ref["margin"] >= MIN_MARGIN:
            return da, db, ref
    raise AssertionError("no seed met the margin condition")
