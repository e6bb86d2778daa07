"""Seeded inputs for the mapper tests (numpy only).  Score tables are made directly (no geometry: the score reads pixels and flags);
the upkeep scenes are tracks_scenes.track_scene variants with imperfect points and poses; the reconstruction scenes are
match_scene-style tables over a ring arc, given their poses."""
import functools

import numpy as np

import tracks_scenes as S

W, H = 640, 480                 # W != H
ERR_MARGIN_PX, ANGLE_MARGIN, DEPTH_MARGIN = 1e-6, 1e-9, 1e-6      # the preconditions of tests/test_tracks_host.py


# ------------------------------------------------------------------------------------------------------------ score tables
def counting_observations(start, view, keep, valid, reg):
    """the indices of the observations that count: their track is valid and has a kept observation in a registered view, and their
    own view is not registered"""
    start, view = np.asarray(start, np.int64), np.asarray(view, np.int64)
    track_of = np.searchsorted(start[1:], np.arange(len(view)), side="right")
    seen = np.zeros(len(start) - 1, bool)
    np.logical_or.at(seen, track_of, np.asarray(keep, bool) & np.asarray(reg, bool)[view])
    seen &= np.asarray(valid, bool)
    return np.nonzero(seen[track_of] & ~np.asarray(reg, bool)[view])[0]


def score_table(seed, V, T, big=None, empty=None, single=None, max_len=5, reg_share=0.4, registered=None):
    """T tracks over V views: every track sees `big` (a view with T key points) plus 1 .. max_len - 1 of the ordinary views; `empty`
    is in no track, `single` only in track 0.  Pixels reach 10 % beyond the image on every side; a handful sit at 0, at W and H
    exactly, on cell borders, negative and far outside.  obs_keep ~ 80 %, track_valid ~ 85 %, registered ~ reg_share (big, empty
    and single never).  -> dict(track_start, obs_view, obs_uv, obs_keep, track_valid, registered, image_size)"""
    rng = np.random.default_rng(seed)
    special = [v for v in (big, empty, single) if v is not None]
    ordinary = [v for v in range(V) if v not in special]
    start, view = [0], []
    for t in range(T):
        k = int(rng.integers(1, min(max_len, len(ordinary) + 1))) if big is not None else int(rng.integers(2, min(max_len, len(ordinary)) + 1))
        vs = rng.choice(ordinary, k, replace=False).tolist()
        if big is not None:
            vs.append(big)
        if single is not None and t == 0:
            vs.append(single)
        view += sorted(vs)
        start.append(len(view))
    n = len(view)
    uv = np.stack([rng.uniform(-0.1 * W, 1.1 * W, n), rng.uniform(-0.1 * H, 1.1 * H, n)], axis=1)
    edge = [(0.0, 0.0), (float(W), float(H)), (-5.0, -7.0), (W + 100.0, H + 3.0), (100.0, 75.0), (10.0 * W / 64, 63.0 * H / 64),
            (np.nextafter(float(W), 0.0), np.nextafter(float(H), 0.0)), (-0.0, 1e-300), (1e300, -1e300)]
    if registered is None:
        reg = rng.uniform(size=V) < reg_share
        reg[special] = False
        reg[ordinary[0]] = True
    else:
        reg = np.asarray(registered, bool)
    keep, valid = rng.uniform(size=n) < 0.8, rng.uniform(size=T) < 0.85
    if single is not None and registered is None:                # track 0 is seen, so that `single` has its one counting key point
        valid[0] = True
        keep[:start[1]] = True
        reg[min(v for v in view[:start[1]] if v in ordinary)] = True
    # every edge pixel on an observation that COUNTS (an unregistered view of a seen track), spread over the counting ones: the
    # kernel then computes a cell for each of them (tests/test_mapper_host.py asserts that they count)
    counting = counting_observations(start, view, keep, valid, reg)
    edge_obs = counting[(np.arange(len(edge)) * (len(counting) // len(edge)))] if len(counting) >= len(edge) else np.zeros(0, np.int64)
    for o, p in zip(edge_obs, edge):
        uv[o] = p
    return dict(track_start=np.array(start, np.int32), obs_view=np.array(view, np.int32), obs_uv=uv, obs_keep=keep, track_valid=valid,
                registered=reg, image_size=(float(W), float(H)), edge_obs=edge_obs, edge_pixels=np.array(edge))


def grid_table(full):
    """view 0 registered, view 1 not; 4096 tracks of two observations.  full: view 1's pixels at the centres of all 64 x 64 cells
    (score LS2FM_VIEW_SCORE_MAX); else all inside one cell (score 5460)"""
    T = 64 * 64
    cx, cy = np.meshgrid(np.arange(64), np.arange(64))
    if full:
        p1 = np.stack([(cx.ravel() + 0.5) * W / 64, (cy.ravel() + 0.5) * H / 64], axis=1)
    else:
        p1 = np.stack([330.0 + 0.002 * cx.ravel(), 200.0 + 0.001 * cy.ravel()], axis=1)
    uv = np.zeros((2 * T, 2))
    uv[0::2] = 1.0
    uv[1::2] = p1
    return dict(track_start=(2 * np.arange(T + 1)).astype(np.int32), obs_view=np.tile([0, 1], T).astype(np.int32), obs_uv=uv,
                obs_keep=np.ones(2 * T, bool), track_valid=np.ones(T, bool), registered=np.array([True, False]),
                image_size=(float(W), float(H)))


@functools.lru_cache(maxsize=None)
def score_tables():
    """name -> table.  Cached: callers do not write into them."""
    out = {
        "v3": score_table(1, 3, 60, max_len=3),
        # 70 views (more than a wave has lanes): view 5 has 5000 key points (a workgroup's worth many times over), view 9 none,
        # view 33 one
        "v70": score_table(2, 70, 5000, big=5, empty=9, single=33),
        "one_cell": grid_table(False),
        "every_cell": grid_table(True),
        "all_registered": score_table(3, 6, 80, registered=np.ones(6, bool)),
        "none_registered": score_table(4, 6, 80, registered=np.zeros(6, bool)),
    }
    empty = dict(out["v3"])
    empty.update(track_start=np.zeros(1, np.int32), obs_view=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2)), obs_keep=np.zeros(0, bool),
                 track_valid=np.zeros(0, bool))
    out["no_tracks"] = empty
    return out


def permuted(table, seed):
    """the table with its tracks in a random order -> table"""
    T = len(table["track_start"]) - 1
    perm = np.random.default_rng(seed).permutation(T)
    start, view, uv, idx = S.permute_tracks(table, perm)
    out = dict(table)
    out.update(track_start=start, obs_view=view, obs_uv=uv, obs_keep=table["obs_keep"][idx], track_valid=table["track_valid"][perm])
    return out


# ----------------------------------------------------------------------------------------------------------- upkeep scenes
def upkeep_scene(seed, lengths, n_views=72, noise_px=0.5, n_outlier_tracks=0, n_low_parallax=0, rot_rad=0.002, trans=0.01,
                 point_noise=0.004, reg_share=0.7, behind=(), lost=(), registered=None, keep_valid=()):
    """A track_scene with what a mapper holds in the middle of a run: poses perturbed by perturb_poses(rot_rad, trans), points off
    their planted places by point_noise, ~reg_share of the views registered (view 0 and the twins always), ~90 % of the tracks
    valid.  Track t of `behind` has its point moved behind its first view; track t of `lost` has it moved a unit away, so that it
    loses every observation.  Adds X, track_valid, registered to the scene."""
    sc = S.track_scene(seed, lengths, n_views=n_views, noise_px=noise_px, n_outlier_tracks=n_outlier_tracks, n_low_parallax=n_low_parallax)
    rng = np.random.default_rng(seed + 5000)
    sc["true_poses"] = sc["poses"]
    sc["poses"] = S.perturb_poses(sc["poses"], seed + 1, rot_rad, trans)
    T = len(sc["track_start"]) - 1
    X = sc["points"] + rng.normal(0.0, point_noise, (T, 3))
    for t in behind:
        v = sc["obs_view"][sc["track_start"][t]]
        P = sc["poses"][v]
        X[t] = -P[:, :3].T @ P[:, 3] * 1.5                                    # beyond the camera's centre, seen from the origin
    for t in lost:
        X[t] = X[t] + np.array([0.6, -0.7, 0.4])
    V = len(sc["poses"])
    if registered is None:
        reg = rng.uniform(size=V) < reg_share
        reg[[0, V - 2, V - 1]] = True
    elif isinstance(registered, str):                                          # "first": only the view of the very first observation
        reg = np.zeros(V, bool)
        reg[sc["obs_view"][0]] = True
    else:
        reg = np.asarray(registered, bool)
    valid = rng.uniform(size=T) < 0.9
    valid[list(behind) + list(lost) + list(keep_valid)] = True
    sc.update(X=X, track_valid=valid, registered=reg, behind=list(behind), lost=list(lost))
    return sc


LONGEST = [5, 64, 65, 4096, 2, 2, 3, 5, 64, 65, 4096, 2]          # both sides of the pair cap, LS2FM_TRACK_MAX_OBS in a full and a partial wave


@functools.lru_cache(maxsize=None)
def upkeep_scenes():
    mixed = [2, 2, 3, 64, 65] + list(np.random.default_rng(7).integers(2, 7, 600))
    return {
        "len2": upkeep_scene(51, [2] * 9, reg_share=1.0),
        "mixed": upkeep_scene(52, mixed, n_low_parallax=5, behind=(5, 40), lost=(6, 41, 300)),
        "outliers": upkeep_scene(53, [8] * 20 + [12] * 20, n_outlier_tracks=25, n_low_parallax=6, reg_share=0.85, behind=(3,)),
        "cap": upkeep_scene(54, [64, 65, 64, 65, 66, 70], reg_share=1.0),
        "longest": upkeep_scene(55, LONGEST, n_views=4200, reg_share=0.97, rot_rad=0.001, trans=0.005,
                                keep_valid=(1, 2, 3, 8, 9, 10), lost=(7,)),
        "one_view": upkeep_scene(56, [3] * 10 + [6] * 5, registered="first"),
    }


PAIR_LANE_LIMIT = 4096 * 256    # kMaxPairBlocks x kThreads of csrc/mapper.hip: uo_angle reaches a pair numbered at or above it only by striding
STRIDE_COPIES = 1100


@functools.lru_cache(maxsize=None)
def stride_scene():
    """16 distinct tracks of 64 observations, every view registered and every track valid, tiled to 1100 tracks (track t a copy of
    track t mod 16): ~2.2 million pairs against the 1 048 576 lanes of uo_angle's capped grid, so the later copies are reached only
    by striding -> (the 16-track scene, dict of the tiled track_start, obs_view, obs_uv, X, track_valid)"""
    sc = upkeep_scene(57, [64] * 16, reg_share=1.0, keep_valid=tuple(range(16)))
    start, view, uv = S.tile_tracks(sc, STRIDE_COPIES)
    src = np.arange(STRIDE_COPIES) % 16
    return sc, dict(track_start=start, obs_view=view, obs_uv=uv, X=sc["X"][src], track_valid=sc["track_valid"][src])


# --------------------------------------------------------------------------------------------------- reconstruction scenes
def tables_scene(seed, poses, n_kp=260, n_points=400, noise_px=0.5, n_conflicts=3, miss=0.1, wrong_share=0.02, cut_view=None):
    """match_scene's tables (tracks_scenes.match_scene: shuffled key points, missed matches, masked wrong matches, planted accepted
    conflicts in pair (0, 1)) over given poses.  cut_view: a view whose every table entry keeps no match (its masks all False)."""
    rng = np.random.default_rng(seed)
    n_views = len(poses)
    points = rng.uniform(-1.0, 1.0, (n_points, 3))
    point_of, kps = [], []
    for v in range(n_views):
        ids = rng.permutation(n_points)[:n_kp]
        point_of.append(ids)
        kps.append(S.project(poses[v], points[ids]) + rng.normal(0.0, noise_px, (n_kp, 2)))
    full, masks = {}, {}
    for a in range(n_views):
        for b in range(a + 1, n_views):
            where_b = {p: k for k, p in enumerate(point_of[b].tolist())}
            rows = [(k, where_b[p]) for k, p in enumerate(point_of[a].tolist()) if p in where_b and rng.uniform() >= miss]
            m = np.array(rows, np.int64).reshape(-1, 2)
            mask = np.ones(len(m), bool)
            wrong = rng.choice(len(m), int(round(wrong_share * len(m))), replace=False)
            m[wrong, 1] = rng.integers(0, n_kp, len(wrong))
            mask[wrong] = False
            if (a, b) == (0, 1) and n_conflicts:
                good = np.nonzero(mask)[0]
                pick = rng.choice(len(good) // 2, n_conflicts, replace=False)
                extra = [(m[good[2 * i], 0], m[good[2 * i + 1], 1]) for i in pick]
                m = np.concatenate([m, np.array(extra, np.int64)])
                mask = np.concatenate([mask, np.ones(len(extra), bool)])
            if cut_view in (a, b):
                mask = np.zeros(len(m), bool)
            order = rng.permutation(len(m))
            full[(a, b)], masks[(a, b)] = m[order].astype(np.uint32), mask[order]
    tables = []
    for v in range(n_views):
        idx, msk = [], []
        for j in range(n_views):
            if j == v:
                continue
            m = full[(min(v, j), max(v, j))]
            idx.append(m if j > v else m[:, [1, 0]])
            msk.append(masks[(min(v, j), max(v, j))])
        tables.append(dict(kypts=kps[v], indxes=idx, mask=msk))
    return dict(tables=tables, poses=np.asarray(poses), keypoints=kps, point_of=point_of, points=points)


RING_VIEWS, RING_ARC = 8, 105.0         # 15 degrees between neighbours: every pair of the arc shares most points, rotations stay far from pi


@functools.lru_cache(maxsize=None)
def ring_scene(cut=False):
    """8 views on a 105 degree arc, 400 points, 260 key points per view, 0.5 px noise, masked wrong matches, planted conflicts;
    cut: a ninth view, beyond the arc's end, whose table entries keep no match"""
    poses = S.ring(RING_VIEWS + (1 if cut else 0), arc_deg=RING_ARC * (RING_VIEWS if cut else RING_VIEWS - 1) / (RING_VIEWS - 1),
                   rng=np.random.default_rng(77))
    return tables_scene(78, poses, cut_view=RING_VIEWS if cut else None)


@functools.lru_cache(maxsize=None)
def collapsed_scene():
    """a ring of arc 0 without the height jitter: six cameras at one place looking the same way.  Every pair matches, no pair has
    parallax: a legitimately degenerate input, no initial pair exists"""
    return tables_scene(79, S.ring(6, arc_deg=0.0), n_conflicts=0)
