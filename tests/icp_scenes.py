"""Deterministic scenes for the ICP tests (numpy only; N, M <= 4096 but for the one ragged size that has to pass a whole launch),
each built for one way the kernels go wrong.  scenes() -> name -> dict(src float32 [M, 3], dst float32 [N, 3], normals (float32
[N, 3] of dst, or None: point to point), max_dist, with_scale, init (the transform the run starts from), truth (the transform that
maps src onto its points of dst, or None), iters, tol_rot, tol_trans).  restated(name) is the restatement's run by its two solve
routes, computed once and shared; callers do not write into it.  tests/test_icp_host.py asserts, per scene, the condition under
which a wrong kernel fails it."""
import functools

import numpy as np

import icp_restate as IR

F32 = np.float32
N_DST, N_SRC = 4096, 1500
TOL = 1e-7                     # the runs' stop: above the floor that the fp32 rounding of p' leaves in delta, far below the start
LAUNCH_LANES = 512 * 512       # one pass of icp_accumulate (include/ls2fm.h): the lanes stride over more source points than this


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def surface(rng, n):
    """n points on a unit sphere at the origin and on the surface of the box [0.7, 1.7] x [-0.4, 0.5] x [-0.3, 0.9] next to it
    (no symmetry left), with their outward normals"""
    n_s = n // 2
    v = rng.normal(size=(n_s, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    lo, hi = np.array([0.7, -0.4, -0.3]), np.array([1.7, 0.5, 0.9])
    n_b = n - n_s
    p = rng.uniform(lo, hi, (n_b, 3))
    e = hi - lo
    area = np.array([e[1] * e[2], e[0] * e[2], e[0] * e[1]])
    axis = rng.choice(3, n_b, p=area / area.sum())
    side = rng.integers(0, 2, n_b)
    nb = np.zeros((n_b, 3))
    p[np.arange(n_b), axis] = np.where(side == 1, hi[axis], lo[axis])
    nb[np.arange(n_b), axis] = np.where(side == 1, 1.0, -1.0)
    pts = np.concatenate([v, p]).astype(F32)
    return pts, np.concatenate([v, nb]).astype(F32)


def inverse_apply(T, pts):
    """the points that T maps onto pts"""
    s, R, t = T
    return ((np.asarray(pts, np.float64) - t) @ R) / s


@functools.lru_cache(maxsize=None)
def _base():
    rng = np.random.default_rng(31)
    dst, normals = surface(rng, N_DST)
    pick = np.sort(rng.permutation(N_DST)[:N_SRC])
    extent = float(np.linalg.norm(dst.max(axis=0) - dst.min(axis=0)))
    R = rotation([0.3, -0.5, 0.8], np.radians(5.0))
    shift = np.array([0.6, -0.64, 0.48]) * 0.05 * extent          # a unit vector times 5 % of the extent
    return dst, normals, pick, extent, R, shift


def _rigid(scale=1.0, with_normals=False):
    dst, normals, pick, extent, R, shift = _base()
    truth = (scale, R, shift)
    src = inverse_apply(truth, dst[pick]).astype(F32)
    return dict(src=src, dst=dst, normals=normals if with_normals else None, max_dist=None, with_scale=scale != 1.0, init=IR.identity(),
                truth=truth, iters=50, tol_rot=TOL, tol_trans=TOL, pick=pick, extent=extent)


def _sliding():
    """a flat patch z = 0.25 with normals (0, 0, 1): J = [p.y, -p.x, 0, 0, 0, 1, p.z], three columns exactly zero, the third pivot 0"""
    rng = np.random.default_rng(32)
    dst = rng.uniform(0.0, 1.0, (1024, 3))
    dst[:, 2] = 0.25
    normals = np.zeros((1024, 3), F32)
    normals[:, 2] = 1.0
    src = dst[::2] + np.array([0.01, -0.02, 0.03])
    return dict(src=src.astype(F32), dst=dst.astype(F32), normals=normals, max_dist=None, with_scale=False, init=IR.identity(), truth=None,
                iters=5, tol_rot=TOL, tol_trans=TOL)


PARTIAL_CUTOFF = 0.125         # float32(0.125)^2 = 0.015625 exactly


def _partial():
    """the rigid scene 1 degree and 1 % off under a cut-off of 0.125, with the identity as the start (so p' = p exactly at the
    first step).  Half the source is moved 20 units away, outside the cut-off of anything; rows 5, 70, 133 and 640 hold NaN or
    infinite coordinates; the last source point has one reference within reach, exactly 0.125 away along x: d2 == max_d2."""
    dst, normals, pick, extent, _, _ = _base()
    truth = (1.0, rotation([0.3, -0.5, 0.8], np.radians(1.0)), np.array([0.6, -0.64, 0.48]) * 0.01 * extent)
    src = inverse_apply(truth, dst[pick]).astype(F32)
    src[1::2] += F32(20.0)
    bad = {5: (np.nan, 0.5, 0.5), 70: (0.5, np.inf, 0.5), 133: (-np.inf, np.nan, 0.1), 640: (0.1, 0.2, np.nan)}
    for row, v in bad.items():
        src[row] = np.array(v, F32)
    src = np.concatenate([src, np.array([[0.5, 0.5, 5.0]], F32)])
    dst = np.concatenate([dst, np.array([[0.625, 0.5, 5.0]], F32)])
    return dict(src=src, dst=dst, normals=None, max_dist=PARTIAL_CUTOFF, with_scale=False, init=IR.identity(), truth=None, iters=50,
                tol_rot=TOL, tol_trans=TOL, bad_rows=np.array(sorted(bad)), far_rows=np.arange(1, N_SRC, 2), tie_row=len(src) - 1)


def _no_pairs():
    sc = _rigid()
    sc.update(max_dist=1e-4, iters=5, truth=None)
    return sc


RAGGED_SIZES = (1, 63, 65, 257, LAUNCH_LANES + 1)


def _ragged(n):
    """the first n source points of the rigid scene; past its 1500 the points repeat (a pair is a function of the point alone)"""
    sc = _rigid()
    reps = -(-n // N_SRC)
    sc.update(src=np.tile(sc["src"], (reps, 1))[:n].copy(), iters=50 if n <= 4096 else 6, truth=None)
    return sc


@functools.lru_cache(maxsize=None)
def scenes():
    out = dict(rigid=_rigid(), similarity=_rigid(scale=1.07), plane=_rigid(with_normals=True), sliding=_sliding(), partial=_partial(),
               no_pairs=_no_pairs())
    out.update({f"ragged_{n}": _ragged(n) for n in RAGGED_SIZES})
    return out


NAMES = ("rigid", "similarity", "plane", "sliding", "partial", "no_pairs") + tuple(f"ragged_{n}" for n in RAGGED_SIZES)
WHOLE_RUNS = ("rigid", "similarity", "plane")
SINGLE_STEPS = 6               # k = 0 ... 5


@functools.lru_cache(maxsize=None)
def restated(name, route="chol"):
    """IR.run's dict of the scene, following the stated Cholesky order ("chol") or numpy.linalg.solve ("numpy"); every step
    holds both routes' delta and T_new from the transform it started at.  The one ragged size past 4096 stops after SINGLE_STEPS."""
    sc = scenes()[name]
    return IR.run(sc["src"], sc["dst"], sc["normals"], sc["init"], sc["max_dist"], sc["with_scale"], sc["iters"], sc["tol_rot"],
                  sc["tol_trans"], route=route)
