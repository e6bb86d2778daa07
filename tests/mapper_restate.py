"""numpy fp64 restatement of the two device calls of ls2fm.mapper (include/ls2fm.h, "The incremental mapper's two per-step device
calls"): the visibility-pyramid score of every view and the upkeep of the observation and point state.  Written for this project
from the rules in the header, not from the kernels: the score builds every level's grid by integer division of the cell
coordinates (no bit masks, no shifts), the upkeep walks the tracks one by one.  The geometry (pixel error, depth, centre, angle)
is tracks_restate's.

`update_observations(..., margins=True)` also returns how close any decision came to its threshold (pixel error against
max_error_px, depth against DBL_EPSILON, a track's largest angle against min_tri_angle), as tracks_restate._Margins reports them:
the tests assert that their scenes keep clear of the thresholds, so that the integer outputs can be compared exactly."""
import math

import numpy as np

import tracks_restate as R

GRID = 64
LEVELS = 6
SCORE_MAX = sum(16 ** l for l in range(1, LEVELS + 1))          # 17 895 696
BAD_START, BAD_VIEW, BAD_PIXEL = 1, 2, 4


def track_of_observations(track_start, n_obs):
    """[n_obs]: the track that owns each observation (-1: none), and the status bits of the table"""
    ts = np.asarray(track_start, np.int64)
    owner = np.full(n_obs, -1, np.int64)
    status = 0
    for t in range(len(ts) - 1):
        a, b = int(ts[t]), int(ts[t + 1])
        if not (0 <= a <= b <= n_obs and b - a <= R.MAX_OBS):
            status |= BAD_START
            continue
        owner[a:b] = t
    return owner, status


def cell(x, size):
    q = (64.0 * x) / size
    if q >= 63.0:
        return 63
    return int(math.floor(q)) if q > 0.0 else 0


def pyramid_score(cells):
    """cells: an iterable of (cx, cy) of the finest level -> sum over l = 1 .. 6 of 4^l x (distinct cells of level l)"""
    total = 0
    for l in range(1, LEVELS + 1):
        side = GRID >> l                                        # finest cells per side of a level-l cell
        total += 4 ** l * len({(cx // side, cy // side) for cx, cy in cells})
    return total


def view_scores(track_start, obs_view, obs_uv, obs_keep, track_valid, registered, image_size):
    """-> (score int64 [V], num_visible int32 [V], status)"""
    view = np.asarray(obs_view, np.int64)
    uv = np.asarray(obs_uv, np.float64).reshape(-1, 2)
    keep = np.asarray(obs_keep).astype(bool)
    valid = np.asarray(track_valid).astype(bool)
    reg = np.asarray(registered).astype(bool)
    V = len(reg)
    size = np.broadcast_to(np.asarray(image_size, np.float64).reshape(-1, 2), (V, 2))
    owner, status = track_of_observations(track_start, len(view))
    bad_view = (view < 0) | (view >= V)
    if bad_view.any():
        status |= BAD_VIEW
        owner = np.where(bad_view, -1, owner)
    seen = np.zeros(len(valid), bool)
    for o in range(len(view)):
        t = owner[o]
        if t >= 0 and valid[t] and keep[o] and reg[view[o]]:
            seen[t] = True
    cells = [[] for _ in range(V)]
    num = np.zeros(V, np.int32)
    for o in range(len(view)):
        t = owner[o]
        if t < 0 or not seen[t] or reg[view[o]]:
            continue
        v = view[o]
        num[v] += 1
        if not np.isfinite(uv[o]).all():
            status |= BAD_PIXEL
            continue
        cells[v].append((cell(uv[o, 0], size[v, 0]), cell(uv[o, 1], size[v, 1])))
    score = np.array([pyramid_score(c) for c in cells], np.int64)
    return score, num, status


def update_observations(poses, intrinsics, registered, track_start, obs_view, obs_uv, X, track_valid, max_error_px=4.0,
                        min_tri_angle_deg=1.5, margins=False):
    """-> dict(obs_keep uint8 [n_obs], track_valid bool [T], num_kept int32 [T], tri_angle [T], status) and, with margins=True,
    dict(error_px, angle, depth): the closest any decision came to its threshold"""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    V = len(poses)
    intr = np.asarray(intrinsics, np.float64).reshape(-1, 4)
    if len(intr) == 1:
        intr = np.repeat(intr, V, axis=0)
    reg = np.asarray(registered).astype(bool)
    view = np.asarray(obs_view, np.int64)
    uv = np.asarray(obs_uv, np.float64).reshape(-1, 2)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    valid_in = np.asarray(track_valid).astype(bool)
    T = len(valid_in)
    thr2 = float(max_error_px) * float(max_error_px)
    min_angle = float(min_tri_angle_deg) * (math.pi / 180.0)
    mg = R._Margins(float(max_error_px), min_angle)
    owner, status = track_of_observations(track_start, len(view))
    if ((view < 0) | (view >= V)).any():
        status |= BAD_VIEW
    C = R.centres(poses)
    keep = np.zeros(len(view), np.uint8)
    for o in range(len(view)):
        t, v = owner[o], view[o]
        if t < 0 or not (0 <= v < V) or not valid_in[t] or not reg[v]:
            continue
        e2, z = R.observe(poses[v][None], intr[v][None], uv[o][None], X[t][None])
        mg.errors(e2, z)
        keep[o] = 1 if (z[0, 0] > R.DBL_EPS and e2[0, 0] <= thr2) else 0
    num = np.zeros(T, np.int32)
    ang = np.zeros(T)
    out_valid = np.zeros(T, bool)
    ts = np.asarray(track_start, np.int64)
    for t in range(T):
        obs = np.nonzero((owner == t) & (keep == 1))[0]
        num[t] = len(obs)
        first = view[obs[:R.HYP_OBS]]
        best = 0.0
        if len(first) >= 2:
            pp = np.array(R.pair_list(len(first)), np.int64)
            a = R.tri_angle(C[first[pp[:, 0]]], C[first[pp[:, 1]]], X[t])
            a = a[~np.isnan(a)]
            best = float(a.max()) if len(a) else 0.0
            mg.angles(best)
        ang[t] = best
        out_valid[t] = num[t] >= 2 and best >= min_angle
    res = dict(obs_keep=keep, track_valid=out_valid, num_kept=num, tri_angle=ang, status=status)
    if margins:
        return res, dict(error_px=mg.error_px, angle=mg.angle, depth=mg.depth)
    return res
