"""Deterministic scenes for the stereo chain under cameras that share nothing (numpy only).  Each returns a dict or arrays; callers
do not write into them.

views_scene(H, W, w)     4 turned cameras, each with its own fx != fy and an off-centre principal point, over a tilted textured plane;
                         references that are not the identity, source rows with a -1, a repeat and views on both sides: the inputs of
                         THE SWEEP RULE, THE PLANE SCORE and THE PATCHMATCH STEP where a view's intrinsics or a rotation's transpose
                         taken for another's would show.
views_state(sc, depth)   a state for PatchMatch on that scene: a depth map with the plane's true camera-frame normal, plain or with
                         patchmatch_scenes.edge_state's disturbances, the horizon normals formed with each reference's own intrinsics.
views_fusion(H, W, C)    the inputs of THE CONSISTENCY RULE and THE FUSION RULE on the same cameras.
long_rows(rows, S)       source rows padded to S entries with repeats and -1."""
import functools

import numpy as np

import mvs_scenes as S
import patchmatch_scenes as PS
from raster_scenes import look_at

F32 = np.float32
NAN = np.nan
V = 4
EYES = [(0.0, 0.0, -2.0), (0.16, 0.03, -1.96), (-0.14, 0.05, -2.03), (0.04, -0.12, -2.06)]
TARGETS = [(0.03, 0.02, 0.0), (-0.02, 0.04, 0.0), (0.05, -0.03, 0.0), (-0.04, -0.02, 0.0)]
ROLLS = [3.0, 7.0, -5.0, 11.0]                                          # degrees about the optical axis
PLANE_NORMAL = (0.3, -0.2, -1.0)                                        # through the origin; normalised below
# per view fx, fy and the principal point's offset from the image centre, in pixels
FOCALS = [(44.0, 36.5), (37.25, 43.5), (46.5, 39.75), (35.0, 41.5)]
CENTRES = [(0.3, -0.45), (-0.6, 0.35), (0.7, 0.55), (-0.35, -0.7)]
TEXTURE_SCALE = 0.45                                                    # sphere_texture's waves span several pixels of a window
REFS = [1, 2, 0]            # refs[r] != r in every row
# per reference: a -1, one view twice, and views below and above it (view 0 has none below)
SOURCES = [[2, -1, 0, 3, 2], [3, -1, 0, 1, 3], [1, -1, 2, 3, 1]]
DEPTHS = [1.75, 1.87, 1.99, 2.11, 2.23, 2.35, 2.47, 2.6, 1.63]
ANGLE = 30.0                # degrees: views_fusion's max_normal_angle
# a view's camera-frame normal n with the unit vector e across it: lengths other than 1, zero, NaN, flipped, 50 degrees off (beyond
# ANGLE against the true normal), 20 degrees off (within it)
NORMAL_KINDS = 9


def _rolled(pose, deg):
    a = np.deg2rad(deg)
    turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return (turn @ pose.astype(np.float64)).astype(F32)


@functools.lru_cache(maxsize=None)
def cameras(H, W):
    """poses float32 [4, 3, 4], intr float32 [4, 3, 3], and in float64 from those rounded values: the eyes [4, 3], the pixel rays
    [4, H, W, 3], the plane's normal in each camera's frame [4, 3] and the depth of every pixel's hit point [4, H, W]"""
    poses = np.stack([_rolled(look_at(e, t), r) for e, t, r in zip(EYES, TARGETS, ROLLS)])
    intr = np.zeros((V, 3, 3), F32)
    for v, ((fx, fy), (ox, oy)) in enumerate(zip(FOCALS, CENTRES)):
        intr[v] = [[fx, 0, W / 2.0 + ox], [0, fy, H / 2.0 + oy], [0, 0, 1]]
    nw = np.asarray(PLANE_NORMAL, np.float64)
    nw /= np.linalg.norm(nw)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    eyes, rays, normal, depth = np.empty((V, 3)), np.empty((V, H, W, 3)), np.empty((V, 3)), np.empty((V, H, W))
    for v in range(V):
        P, K = poses[v].astype(np.float64), intr[v].astype(np.float64)
        Rm = P[:, :3]
        eyes[v] = -Rm.T @ P[:, 3]
        rays[v] = np.stack([(xx + 0.5 - K[0, 2]) / K[0, 0], (yy + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(xx)], axis=-1)
        normal[v] = Rm @ nw
        depth[v] = -(nw @ eyes[v]) / (rays[v] @ normal[v])             # the ray z (xn, yn, 1) meets n_w . (R^T c + eye) = 0
    assert (depth > 0).all() and (rays @ normal[:, None, :, None])[..., 0].max() < 0
    return poses, intr, eyes, rays, normal, depth


@functools.lru_cache(maxsize=None)
def views_scene(H=17, W=33, w=3):
    """The image of a pixel is sphere_texture at TEXTURE_SCALE times the point its centre's ray hits, through that view's own K;
    a NaN in view 0, +inf in view 1, -inf in view 2, placed as grid_scene places them.  `depth` [4, H, W] and `normal` [4, 3] are the
    analytic depth and the plane's normal in each camera's frame (float64).  The planes DEPTHS are rolled per reference so that no
    row starts inside the true depths' range (about 1.73 to 2.54)."""
    poses, intr, eyes, rays, normal, depth = cameras(H, W)
    images = np.empty((V, H, W), F32)
    for v in range(V):
        X = (rays[v] * depth[v][..., None]) @ poses[v].astype(np.float64)[:, :3] + eyes[v]
        images[v] = S.sphere_texture(TEXTURE_SCALE * X)
    images[0, H - 3, W // 2] = np.nan
    images[1, H - 2, 3] = np.inf
    images[2, 1, W - 3] = -np.inf
    base = np.array(DEPTHS, F32)
    depths = np.stack([np.roll(base, 1), np.roll(base, 2), base[::-1]])      # they start at 1.63, 2.6 and 1.63
    return dict(images=images, poses=poses, intr=intr, refs=np.array(REFS), sources=np.array(SOURCES), depths=depths, depth=depth,
                normal=normal, half_width=w, near=0.5, min_var=1e-4, min_sources=2, H=H, W=W)


def long_rows(rows, S_=64):
    """rows [R, S0] -> [R, S_]: each row repeated until S_ - 3 entries (its -1 with it), then -1"""
    rows = np.asarray(rows)
    reps = -(-S_ // rows.shape[1])
    out = np.tile(rows, (1, reps))[:, :S_].copy()
    out[:, S_ - 3:] = -1
    return out


def views_state(sc, depth, edges=False):
    """depth float32 [R, H, W] (a copy of `depth`) and normal float32 [R, H, W, 3]: the plane's normal in each reference's frame.
    edges: patchmatch_scenes.edge_state's patterns written over both -- depths NaN, 0, negative and +inf; normals (1, 0, -xn_p), whose
    g_p is 0, (1, 0, -(xn_p + 1 / 32)), whose g changes sign inside the window, (0, 0, 1), which faces away, and one with a NaN --
    where xn_p comes from the intrinsics of the reference's own view."""
    refs, H, W = sc["refs"], sc["H"], sc["W"]
    depth = np.array(depth, F32)
    normal = np.empty((len(refs), H, W, 3), F32)
    yy, xx = np.mgrid[0:H, 0:W]
    for r, rv in enumerate(refs):
        normal[r] = sc["normal"][rv].astype(F32)
        if not edges:
            continue
        K = sc["intr"][rv]
        xn = ((xx.astype(F32) + F32(0.5)) - K[0, 2]) / K[0, 0]
        pick = np.asarray(PS.EDGE_DEPTHS, F32)[(3 * xx + 5 * yy + 2 * r) % len(PS.EDGE_DEPTHS)]
        depth[r] = np.where(pick == 1, depth[r], pick)
        kind = (xx + 3 * yy + r) % PS.N_NORMALS
        zero, away, bad, sign = kind == 3, kind == 5, kind == 7, kind == 9
        normal[r][zero] = np.stack([np.ones(zero.sum(), F32), np.zeros(zero.sum(), F32), -xn[zero]], axis=1)
        normal[r][away] = (0, 0, 1)
        normal[r][bad] = (0, np.nan, -1)
        normal[r][sign] = np.stack([np.ones(sign.sum(), F32), np.zeros(sign.sum(), F32), -(xn[sign] + F32(1 / 32))], axis=1)
    return depth, normal


def fusion_rows(S_=5):
    """fuse_scenes.edge_scene's source rows for 4 views: lower and higher partners, the view itself, a -1 and a view twice"""
    rows = []
    for v in range(V):
        o = [j for j in range(V) if j != v]
        rows.append(([(v + 1) % V] if S_ == 1 else [o[0], -1, v if v % 2 == 0 else o[2], o[-1], o[0]])[:S_])
    return np.asarray(rows)


@functools.lru_cache(maxsize=None)
def views_fusion(H=17, W=33, C=3):
    """All 4 views of views_scene's cameras.  depth: the analytic depth times mvs_scenes.FILTER_VALUES in filter_scene's pattern (a
    depth doubled or a quarter too far, NaN, 0, -1, inf).  normal: the plane's camera-frame normal in a pattern of NORMAL_KINDS.
    colour: random with NaNs.  sources: fusion_rows (the view itself in a row: what the fusion skips); filter_sources: for the
    consistency filter every other view, the first of them twice, and a -1."""
    poses, intr, eyes, rays, nc, depth64 = cameras(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.empty((V, H, W), F32)
    normal = np.empty((V, H, W, 3), F32)
    off50, off20 = np.tan(np.deg2rad(50.0)), np.tan(np.deg2rad(20.0))
    for v in range(V):
        pick = np.asarray(S.FILTER_VALUES, F32)[(3 * xx + 5 * yy + 2 * v) % len(S.FILTER_VALUES)]
        depth[v] = pick * depth64[v].astype(F32)
        n = nc[v]
        e = np.cross(n, (0.0, 1.0, 0.0))
        e /= np.linalg.norm(e)
        table = np.asarray([n, 2 * n, n, (0, 0, 0), n, (NAN, n[1], n[2]), -n, n + off50 * e, 0.5 * (n + off20 * e)], F32)
        assert len(table) == NORMAL_KINDS
        normal[v] = table[(xx + 4 * yy + 3 * v) % NORMAL_KINDS]
    rng = np.random.default_rng(100 * H + W + C)
    colour = (rng.integers(0, 256, size=(V, H, W, C)) / 256.0).astype(F32)
    for v in range(V):
        for i in range(0, H, 2):
            colour[v, i, (2 * i + v) % W, (i + v) % C] = NAN
    sources = fusion_rows()
    others = [[j for j in range(V) if j != v] for v in range(V)]
    filter_sources = np.asarray([[o[0], -1, o[1], o[2], o[0]] for o in others])
    return dict(depth=depth, poses=poses, intr=intr, sources=sources, filter_sources=filter_sources, normal=normal, colour=colour,
                near=0.5, max_reproj=0.75, rel_depth=0.008, max_normal_angle=ANGLE, H=H, W=W)
