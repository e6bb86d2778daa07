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
    ab, as_ = angle(best), angle(second)
    has = best > 0
    ok = has & ~(ab > max_distance) & ~(ab >= max_ratio * as_)
    best_j = np.where(has, j, -1)
    margins = np.minimum(np.abs(ab - max_distance), np.abs(ab - max_ratio * as_))[has]
    return best, best_j, second, np.where(ok, j, -1), (float(margins.min()) if margins.size else np.inf)


def match_pair(da, db, max_ratio=0.8, max_distance=0.7, cross_check=True):
    """-> dict(matches int64 [M,2] in increasing i, the raw integers of both directions, margin)"""
    d = products(da, db)
    b_ab, j_ab, s_ab, p_ab, m_ab = one_way(d, max_ratio, max_distance)
    b_ba, j_ba, s_ba, p_ba, m_ba = one_way(d.T, max_ratio, max_distance)
    i = np.nonzero(p_ab >= 0)[0]
    if cross_check:
        i = i[p_ba[p_ab[i]] == i]
    matches = np.stack([i, p_ab[i]], axis=1).astype(np.int64).reshape(-1, 2)
    return dict(matches=matches, best_ab=b_ab, best_j_ab=j_ab, second_ab=s_ab, proposal_ab=p_ab, best_ba=b_ba, best_j_ba=j_ba,
                second_ba=s_ba, proposal_ba=p_ba, margin=min(m_ab, m_ba))


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


def seeded_pair(n_a, n_b, seed, shared=0.5, loud=True):
    """two images that share `shared` of the smaller one's descriptors under multiplicative noise 0.5 - 1.0; loud: a few
    descriptors are concentrated so that bytes up to 255 occur.  Tries seeds from `seed` on until the restatement's margin is
    >= MIN_MARGIN (asserted) -> (da, db, restated result)"""
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
        ref = match_pair(da, db)
        if ref["margin"] >= MIN_MARGIN:
            return da, db, ref
    raise AssertionError("no seed met the margin condition")
