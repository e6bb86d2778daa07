"""Seeded synthetic scenes for the track tests (numpy only): points in a box, cameras on a ring (or an arc of it) looking in, exact
projections plus Gaussian pixel noise, a planted share of wrong observations moved by at least 20 px, planted conflicts, and planted
low-parallax tracks seen only by two nearly coincident cameras.  One pinhole camera for all views, except in per_view_scene."""
import functools

import numpy as np

F_PX, CX, CY = 600.0, 320.0, 240.0
INTR = (F_PX, F_PX, CX, CY)
K = np.array([[F_PX, 0.0, CX], [0.0, F_PX, CY], [0.0, 0.0, 1.0]])
RADIUS = 6.0                # of the ring; the points lie in [-1, 1]^3
EXTENT = 2.0 * np.sqrt(3.0)  # the box's diagonal
# Tolerance of X, tri_angle and mean_error_px in the GPU tests: 4 x the largest difference, over gpu_scenes() and more_gpu_scenes()
# below at the options of every device run, between the restatement's Jacobi route and its numpy.linalg route (3.46e-13, X of scene
# "mixed"; the second set stays below it, 1.1e-13 at most).  tests/test_tracks_host.py recomputes that difference and holds it to
# TOL / 4, so a changed seed or scene cannot leave the tolerance behind its measurement.
TOL = 1.4e-12


def look_at(centre, target=np.zeros(3)):
    """world-to-camera [3,4] of a camera at `centre` looking at `target`, y down"""
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.c_[R, -R @ centre]


def ring(n_views, arc_deg=360.0, jitter=None, rng=None):
    """poses [V,3,4]: cameras on a ring of radius RADIUS in the xy plane, heights jittered so that no three centres align"""
    ang = np.radians(arc_deg) * np.arange(n_views) / (n_views if arc_deg >= 360.0 else max(n_views - 1, 1))
    out = []
    for k, a in enumerate(ang):
        h = 0.0 if rng is None else rng.uniform(-0.5, 0.5)
        out.append(look_at(np.array([RADIUS * np.cos(a), RADIUS * np.sin(a), h])))
    return np.array(out)


def project(P, X):
    """pixels of points X [n,3] in camera P [3,4] (or P [n,3,4] row by row)"""
    P = np.asarray(P, np.float64)
    if P.ndim == 2:
        c = X @ P[:, :3].T + P[:, 3]
    else:
        c = np.einsum("nij,nj->ni", P[:, :, :3], X) + P[:, :, 3]
    return np.stack([F_PX * c[:, 0] / c[:, 2] + CX, F_PX * c[:, 1] / c[:, 2] + CY], axis=1)


def track_scene(seed, lengths, n_views=72, noise_px=0.5, n_outlier_tracks=0, n_low_parallax=0, min_outlier_len=6):
    """A track table made directly: track t of lengths[t] observations sees point t from lengths[t] distinct ring views (rising).
    n_outlier_tracks of the tracks with >= min_outlier_len observations get one or two observations moved by 20 .. 60 px;
    n_low_parallax extra two-view tracks are seen only by the two nearly coincident cameras appended after the ring.
    -> dict(poses [V,3,4], intr (4,), track_start, obs_view, obs_uv, points [T,3], outlier bool [n_obs], low_parallax bool [T],
    noise_px)"""
    rng = np.random.default_rng(seed)
    poses = ring(n_views, rng=rng)
    twin0 = look_at(np.array([0.3, -RADIUS, 0.2]))
    twin1 = look_at(np.array([0.3 + 0.01, -RADIUS, 0.2]))                 # ~0.1 degree of parallax at the box
    poses = np.concatenate([poses, twin0[None], twin1[None]])
    lengths = list(lengths)
    T = len(lengths) + n_low_parallax
    points = rng.uniform(-1.0, 1.0, (T, 3))
    start, view, uv, outlier = [0], [], [], []
    candidates = [t for t, n in enumerate(lengths) if n >= min_outlier_len]
    with_outliers = set(rng.choice(candidates, n_outlier_tracks, replace=False).tolist()) if n_outlier_tracks else set()
    for t in range(T):
        if t < len(lengths):
            vs = np.sort(rng.choice(n_views, lengths[t], replace=False))
        else:
            vs = np.array([n_views, n_views + 1])
        p = project(poses[vs], np.repeat(points[t][None], len(vs), axis=0)) + rng.normal(0.0, noise_px, (len(vs), 2)) * (noise_px > 0)
        bad = np.zeros(len(vs), bool)
        if t in with_outliers:
            bad[rng.choice(len(vs), rng.integers(1, 3), replace=False)] = True
            a = rng.uniform(0.0, 2.0 * np.pi, bad.sum())
            p[bad] += rng.uniform(20.0, 60.0, bad.sum())[:, None] * np.stack([np.cos(a), np.sin(a)], axis=1)
        view += vs.tolist()
        uv += p.tolist()
        outlier += bad.tolist()
        start.append(len(view))
    low = np.zeros(T, bool)
    low[len(lengths):] = True
    return dict(poses=poses, intr=np.array(INTR), track_start=np.array(start, np.int32), obs_view=np.array(view, np.int32),
                obs_uv=np.array(uv, np.float64).reshape(-1, 2), points=points, outlier=np.array(outlier, bool), low_parallax=low,
                noise_px=noise_px)


def permute_tracks(scene, perm):
    """the same tracks in the order perm -> (track_start, obs_view, obs_uv, obs_map: new observation -> old observation)"""
    ts = scene["track_start"]
    idx = np.concatenate([np.arange(ts[t], ts[t + 1]) for t in perm]) if len(perm) else np.zeros(0, np.int64)
    start = np.concatenate([[0], np.cumsum([ts[t + 1] - ts[t] for t in perm])]).astype(np.int32)
    return start, scene["obs_view"][idx], scene["obs_uv"][idx], idx


def match_scene(seed, n_views=4, n_kp=400, n_points=500, noise_px=0.5, arc_deg=40.0, n_conflicts=3, miss=0.1, wrong_share=0.02):
    """`n_views.npy`-style tables of a synthetic match graph: every view detects n_kp of the n_points (shuffled key point order);
    a pair's matches are the points both views detected, minus a share `miss`, plus a share `wrong_share` of wrong matches whose
    mask is False (the two-view RANSAC's rejects), plus n_conflicts accepted wrong matches in the first pair that tie two points
    together (each makes one component with two key points in one image).
    -> dict(tables, poses, keypoints (list of [n_kp,2]), point_of (list of [n_kp] point ids), points, noise (list of [n_kp,2]),
    n_conflicts)"""
    rng = np.random.default_rng(seed)
    poses = ring(n_views, arc_deg=arc_deg, rng=rng)
    points = rng.uniform(-1.0, 1.0, (n_points, 3))
    point_of, kps, noises = [], [], []
    for v in range(n_views):
        ids = rng.permutation(n_points)[:n_kp]
        nz = rng.normal(0.0, noise_px, (n_kp, 2))
        point_of.append(ids)
        noises.append(nz)
        kps.append(project(poses[v], points[ids]) + nz)
    full, masks = {}, {}
    planted = 0
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
                # an accepted wrong match: key point k of view a to the view-b key point of ANOTHER point that view a also matched
                # correctly: the component then holds two key points of view a
                good = np.nonzero(mask)[0]
                pick = rng.choice(len(good) // 2, n_conflicts, replace=False)
                extra = [(m[good[2 * i], 0], m[good[2 * i + 1], 1]) for i in pick]
                m = np.concatenate([m, np.array(extra, np.int64)])
                mask = np.concatenate([mask, np.ones(len(extra), bool)])
                planted = len(extra)
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
    return dict(tables=tables, poses=poses, keypoints=kps, point_of=point_of, points=points, noise=noises, n_conflicts=planted)


def random_graph(seed, n_views=3, n_kp=300, n_edges=500):
    """random edges between key points of different views -> (image_start int32 [V + 1], edges int32 [E, 2])"""
    rng = np.random.default_rng(seed)
    image_start = (np.arange(n_views + 1) * n_kp).astype(np.int32)
    va = rng.integers(0, n_views, n_edges)
    vb = (va + rng.integers(1, n_views, n_edges)) % n_views
    edges = np.stack([image_start[va] + rng.integers(0, n_kp, n_edges), image_start[vb] + rng.integers(0, n_kp, n_edges)], axis=1)
    return image_start, edges.astype(np.int32)


def path_graph(n_views=64):
    """one key point per view, chained view to view: the longest pointer chain"""
    image_start = np.arange(n_views + 1, dtype=np.int32)
    return image_start, np.stack([np.arange(n_views - 1), np.arange(1, n_views)], axis=1).astype(np.int32)


def star_graph(n_views=40, n_kp=5):
    """key point 2 of the last view matched to key point 1 of every other view"""
    image_start = (np.arange(n_views + 1) * n_kp).astype(np.int32)
    hub = image_start[n_views - 1] + 2
    return image_start, np.stack([np.full(n_views - 1, hub), image_start[:n_views - 1] + 1], axis=1).astype(np.int32)


# the scenes the GPU tests triangulate (tests/test_tracks_host.py asserts their precondition; tests/test_hip_tracks.py compares)
def gpu_scenes():
    mixed_lengths = [2, 3, 64, 66] + list(np.random.default_rng(7).integers(2, 6, 2000))
    return {
        "len2": track_scene(11, [2] * 5),
        "len3": track_scene(12, [3] * 5),
        "len64": track_scene(13, [64]),
        "len66": track_scene(14, [66]),
        "mixed": track_scene(15, mixed_lengths, n_outlier_tracks=0, n_low_parallax=5),
        "outliers": track_scene(16, [8] * 20 + [12] * 20, n_outlier_tracks=25, n_low_parallax=6),
    }


# ------------------------------------------------------------------------------------------------------------------------
# The second set: the shapes and options the first set never reaches.  more_gpu_scenes() is iterated by tests/test_tracks_host.py
# (precondition, Jacobi-against-LAPACK gap, the conditions that pin each scene) and by tests/test_hip_tracks.py (the device).
HYP_LANE_LIMIT = 4096 * 256     # kMaxHypBlocks x kThreads of csrc/tracks.hip: tt_hyp reaches a hypothesis numbered at or above it
                                # only by striding
PAIRS_64 = 64 * 63 // 2         # the hypotheses of a track of >= 64 observations


def displace(scene, obs, rng):
    """move the observations `obs` by 20 .. 60 px in a random direction and mark them as planted outliers (in place)"""
    obs = np.asarray(obs, np.int64)
    a = rng.uniform(0.0, 2.0 * np.pi, len(obs))
    scene["obs_uv"][obs] += rng.uniform(20.0, 60.0, len(obs))[:, None] * np.stack([np.cos(a), np.sin(a)], axis=1)
    scene["outlier"][obs] = True
    return scene


def per_view_scene(seed):
    """a camera of its own for every view, fx != fy: the observations of a one-camera scene re-expressed view by view,
    u' = fx_v (u - CX) / F_PX + cx_v and v' likewise; intr [V, 4]"""
    sc = track_scene(seed, [8] * 20 + [12] * 20 + [2, 3, 5] * 10, n_outlier_tracks=20, n_low_parallax=3)
    rng = np.random.default_rng(seed + 1000)
    V = len(sc["poses"])
    intr = np.stack([rng.uniform(400.0, 900.0, V), rng.uniform(400.0, 900.0, V), rng.uniform(200.0, 440.0, V),
                     rng.uniform(150.0, 330.0, V)], axis=1)
    k = intr[sc["obs_view"]]
    uv = sc["obs_uv"]
    sc["obs_uv"] = np.stack([k[:, 0] * (uv[:, 0] - CX) / F_PX + k[:, 2], k[:, 1] * (uv[:, 1] - CY) / F_PX + k[:, 3]], axis=1)
    sc["intr"] = intr
    return sc


def tile_tracks(scene, copies):
    """the scene's tracks `copies` times over, then cut to `copies` tracks: track t is a copy of track t mod T
    -> (track_start, obs_view, obs_uv)"""
    T = len(scene["track_start"]) - 1
    return permute_tracks(scene, np.arange(copies) % T)[:3]


def deep_pair_scene(seed):
    """tracks whose first `moved` observations are wrong, so that the winning pair lies deep in the pair range: lengths 64, 66 and
    200 with 1, 31 and 61 moved, and one track of 66 with 62 moved, whose only clean pair among its first 64 is (62, 63).
    Noise 0.2 px, for a run at max_error_px = 1: at 4 px some of the ~1900 pairs of 62 wrong observations gather four inliers by
    chance, tie with the clean pair and win by their lower index on every seed tried."""
    moved = [L for L in (1, 31, 61) for _ in range(3)] + [62]
    sc = track_scene(seed, [64, 66, 200] * 3 + [66], n_views=220, noise_px=0.2)
    obs = np.concatenate([np.arange(s, s + L) for s, L in zip(sc["track_start"][:-1], moved)])
    sc["moved"] = np.array(moved)
    return displace(sc, obs, np.random.default_rng(seed + 1000))


SHORT_TRACKS = 1032
# tracks of 0 or 1 observations: three at the very start, four across 1023 / 1024 (the boundary of tt_prepare's scan round), singles
# inside ordinary waves of eight, the whole wave 200 .. 207, and the last two
SHORT_AT = [0, 1, 2, 13, 42, 107, 200, 201, 202, 203, 204, 205, 206, 207, 517, 1022, 1023, 1024, 1025, 1030, 1031]


def short_scene(seed):
    """1032 tracks of 2 .. 7 observations with tracks of 0 and 1 observations (alternating) at SHORT_AT; short bool [T]"""
    lengths = np.random.default_rng(seed + 1000).integers(2, 8, SHORT_TRACKS)
    lengths[SHORT_AT] = np.arange(len(SHORT_AT)) % 2
    sc = track_scene(seed, lengths.tolist())
    sc["short"] = lengths < 2
    return sc


def long_outlier_scene(seed):
    """tracks of 200 and 1000 observations over 1100 views, 12 of each track's first 64 observations wrong"""
    sc = track_scene(seed, [200, 1000], n_views=1100)
    rng = np.random.default_rng(seed + 1000)
    obs = np.concatenate([s + np.sort(rng.choice(64, 12, replace=False)) for s in sc["track_start"][:-1]])
    return displace(sc, obs, rng)


LONGEST = [5, 5, 5, 4096, 5, 5, 5, 5, 3, 4096, 2]       # 4096 = LS2FM_TRACK_MAX_OBS at group 3 of a full wave and in a partial last wave


def longest_scene(seed):
    return track_scene(seed, LONGEST, n_views=4200)


def with_overlong_track(scene, at):
    """the scene's table with a track of 4097 observations (one more than LS2FM_TRACK_MAX_OBS; the origin seen from views
    0 .. 4096) inserted as track `at` -> (track_start, obs_view, obs_uv, keep: the tracks of the result that are the scene's)"""
    n = 4097
    ts = scene["track_start"].astype(np.int64)
    cut = int(ts[at])
    vs = np.arange(n)
    start = np.concatenate([ts[:at + 1], ts[at:] + n]).astype(np.int32)
    view = np.concatenate([scene["obs_view"][:cut], vs, scene["obs_view"][cut:]]).astype(np.int32)
    uv = np.concatenate([scene["obs_uv"][:cut], project(scene["poses"][vs], np.zeros((n, 3))), scene["obs_uv"][cut:]])
    return start, view, uv, np.delete(np.arange(len(start) - 1), at)


LO_FEWER_SEED = 0           # the first seed of 0 .. 49 on which a track of lo_scene leaves the local optimisation by "fewer"


def lo_scene(seed=LO_FEWER_SEED):
    return track_scene(seed, [8] * 40, noise_px=0.7)


def noise_free_scene():
    return track_scene(17, [2, 3, 4, 5, 6, 7, 8] * 6, noise_px=0.0)


@functools.lru_cache(maxsize=None)
def more_gpu_scenes():
    """name -> (scene, the options of every device run of it).  What is restated: "stride" is the 16 distinct tracks, which the
    device test tiles to 536.  Cached: callers do not write into the scenes."""
    default = {}
    return {
        "per_view_intr": (per_view_scene(31), [default, dict(max_error_px=1.0)]),
        "stride": (track_scene(32, [64] * 16, n_outlier_tracks=4), [default]),
        "deep_pair": (deep_pair_scene(34), [dict(max_error_px=1.0)]),
        "short": (short_scene(34), [default]),
        "long_outliers": (long_outlier_scene(35), [default]),
        "longest": (longest_scene(40), [default]),
        "lo_exits": (lo_scene(), [dict(max_error_px=1.0)]),
        "noise_free": (noise_free_scene(), [default]),
        "len3_b": (track_scene(37, [3] * 5), [default]),
    }


def contended_graph(seed, n_views=50, n_points=400, n_edges=100000):
    """every view sees every point (key points shuffled per view); edges between observations of one point in two views: 250
    edges per component of 50 nodes, every lane of a wave uniting into the same few trees -> (image_start, edges)"""
    rng = np.random.default_rng(seed)
    image_start = (np.arange(n_views + 1) * n_points).astype(np.int32)
    where = np.stack([rng.permutation(n_points) for _ in range(n_views)])          # where[v, p]: the key point of point p in view v
    p = rng.integers(0, n_points, n_edges)
    va = rng.integers(0, n_views, n_edges)
    vb = (va + rng.integers(1, n_views, n_edges)) % n_views
    edges = np.stack([image_start[va] + where[va, p], image_start[vb] + where[vb, p]], axis=1)
    return image_start, edges.astype(np.int32)


EMPTY_IMAGES = np.array([0, 0, 5, 5, 5, 9, 9, 14, 14], np.int32)     # images 0, 2, 3, 5 and 7 have no key point


def perturb_poses(poses, seed, rot_rad, trans):
    """every pose but the first turned by rot_rad about a random axis and shifted by `trans` in a random direction: the imperfect
    poses a registration hands to bundle adjustment"""
    rng = np.random.default_rng(seed)
    out = [np.array(poses[0], np.float64)]
    for P in np.asarray(poses, np.float64)[1:]:
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w)
        W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        dR = np.eye(3) + np.sin(rot_rad) * W + (1.0 - np.cos(rot_rad)) * (W @ W)
        d = rng.normal(size=3)
        out.append(np.c_[dR @ P[:, :3], dR @ P[:, 3] + trans * d / np.linalg.norm(d)])
    return np.array(out)


# The classical loop's default rates times this: at the defaults Adam's first steps (each parameter moves by its rate) outweigh
# the residual a triangulated start has left, and the logged error rises before it falls
BA_LR_SCALE = 0.05


def ba_rates():
    """TradBALoop's learning rates for a start from triangulated tracks: its defaults (lr_pose_r 5e-3, lr_pose_t 1e-2, lr_xyzs 1e-2)
    times BA_LR_SCALE"""
    return dict(lr_pose_r=5e-3 * BA_LR_SCALE, lr_pose_t=1e-2 * BA_LR_SCALE, lr_xyzs=1e-2 * BA_LR_SCALE)
