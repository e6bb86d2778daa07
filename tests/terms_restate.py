"""Plain torch statements of the loss terms a stage loop forms outside the render (csrc/reproject.hip: the re-projection term,
the tracing-consistency term, BA's loss lines, the explicit-match terms, SDF.get_surface_pts' last line), written from the header
comments of that file and the reference lines they cite; the checker of tests/test_hip_loss_terms_edges.py, pinned to the loops'
own torch-op forms by tests/test_terms_restate_host.py.

Every statement takes numpy float32 inputs and a `dtype`, forms the term in that dtype and returns the values and, by autograd,
the gradients as float64 numpy arrays.  Three things are the same whatever the dtype, because the kernels do them so:
  * DECISIONS are taken in float32 -- the counted mask `|sdf| < bound` (bound rounded to fp32) and "projection not infinite", the
    adaptive weight `reproj > thresh` -- and the values are then formed in `dtype` GIVEN the decision;
  * the `+ 1e-6` of the projection is the fp32 constant widened (a row built to be infinite in fp32 is infinite in fp64 too);
  * a scalar term forms its per-element values in `dtype` and SUMS them in float64 (the kernels' sums are fp64, fixed order).
The re-projection statement selects the counted rows BEFORE it forms the norm: `torch.where` after the norm (BALoop._reproj_torch)
hands autograd 0 x inf / inf = NaN for an infinite row, where the kernel writes 0.

Also the input builders (well-conditioned BY CONSTRUCTION, so that fp32 itself needs a small part of the bar -- the host test
holds every case to EPS / 4), the case lists the GPU file runs, and the comparison: ONE relative bar EPS against float64,
  per element       for scalars-per-row (d_d, d_sdf, d_sdfs, length),
  per row           relative to the row's own largest entry, for 3-vectors (d_x, surface, out, d_n),
  per view          relative to the view's own largest entry, for d_poses,
  the value itself  for the scalar terms (a mean of non-negative per-element values each within eps is within eps),
exact zero where the reference is exactly zero (dead / uncounted rows, sign(0), empty views), NaN where it is NaN."""
import functools

import numpy as np
import torch

EPS = 2e-5                                     # the bar test_hip_camera_rays.py / test_hip_reproject.py hold these gradients to
C6 = float(np.float32(1e-6))                   # the projection's guard as the kernels hold it
K = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]], dtype=np.float32)      # (last row (0, 0, 1))


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(grad)


def _np(t):
    return None if t is None else t.detach().double().numpy()


def _grad(leaf):
    """a leaf's gradient; a leaf nothing reached has the zero gradient"""
    return np.zeros(tuple(leaf.shape)) if leaf.grad is None else _np(leaf.grad)


def _sum64(per_element):
    return per_element.double().sum()


def _project(pts, R, t, Kt):
    """x_c = R x + t ;  u = K x_c ;  uv = u_xy / (u_z + 1e-6)   (R [m,3,3], t [m,3] per row)"""
    xc = (R @ pts.unsqueeze(-1)).squeeze(-1) + t
    u = xc @ Kt.transpose(-1, -2)
    return u[..., :2] / (u[..., 2:] + C6)


# ------------------------------------------------------------------------------------------------------------ the five terms
def tracing_term(inp, dtype):
    """surface_i = center_i + ray_i d_i ;  tracing = sum_i |target_i - surface_i| live_i / sum(live) ;  sdf_surf = sum_i
    |sdf_last_i| live_i / sum(live) ;  loss = g_tl tracing + g_sd sdf_surf (an absent upstream: that term is not in the loss)
    -> tl, ss, d_d, d_sdf"""
    d = _t(inp["d"], dtype, True)
    live = _t(inp["live"], dtype)
    e = _t(inp["target"], dtype) - (_t(inp["center"], dtype) + _t(inp["ray"], dtype) * d[:, None])
    total = _sum64(live)
    tl = _sum64(torch.linalg.vector_norm(e, dim=-1) * live) / total
    out = {"tl": _np(tl)}
    loss = [] if inp["g_tl"] is None else [inp["g_tl"] * tl]
    sl = None
    if inp["sdf_last"] is not None:
        sl = _t(inp["sdf_last"], dtype, True)
        ss = _sum64(sl.abs() * live) / total
        out["ss"] = _np(ss)
        if inp["g_sd"] is not None:
            loss.append(inp["g_sd"] * ss)
    sum(loss).backward()
    out["d_d"] = _grad(d)
    if sl is not None:
        out["d_sdf"] = _grad(sl)
    return out


def ba_terms(inp, dtype):
    """sdf_surf = mean |sdfs| ;  w = reproj > thresh ? w_hi : w_lo (decided in fp32, no gradient) ;  extra = w reproj + w_surf
    sdf_surf + w_add add ;  loss = g extra -> surf, w, extra, d_reproj, d_sdfs, d_add"""
    r = _t(inp["reproj"], dtype, True)
    s = _t(inp["sdfs"], dtype, True)
    w = inp["w_hi"] if np.float32(inp["reproj"]) > np.float32(inp["thresh"]) else inp["w_lo"]
    surf = _sum64(s.abs()) / s.numel()
    extra = w * r.double() + inp["w_surf"] * surf
    a = None
    if inp["add"] is not None:
        a = _t(inp["add"], dtype, True)
        extra = extra + inp["w_add"] * a.double()
    (inp["g"] * extra).backward()
    out = {"surf": _np(surf), "w": np.float64(w), "extra": _np(extra), "d_reproj": _grad(r), "d_sdfs": _grad(s)}
    if a is not None:
        out["d_add"] = _grad(a)
    return out


def match_term(inp, dtype):
    """pts = center + ray d, projected through the OTHER view's pose (one per segment) ;  reproj_error = mean || uv(pts) - key
    point || ,  sdf_surf = mean |sdf_last| over the S n points together ;  loss = g0 reproj_error + g1 sdf_surf
    -> re, ss, surface [S n,3], d_d [S,n], d_sdf [S,n]"""
    S, n = inp["d"].shape
    d = _t(inp["d"], dtype, True)
    sl = _t(inp["sdf_last"], dtype, True)
    pts = _t(inp["center"], dtype) + _t(inp["ray"], dtype) * d.reshape(-1, 1)
    pose = _t(inp["poses"], dtype).repeat_interleave(n, dim=0)
    uv = _project(pts, pose[:, :, :3], pose[:, :, 3], _t(K, dtype))
    re = _sum64(torch.linalg.vector_norm(uv - _t(inp["uv_obs"], dtype), dim=-1)) / (S * n)
    ss = _sum64(sl.abs()) / (S * n)
    (inp["g0"] * re + inp["g1"] * ss).backward()
    return {"re": _np(re), "ss": _np(ss), "surface": _np(pts), "d_d": _grad(d), "d_sdf": _grad(sl)}


def reproject_mask(inp):
    """the counted mask as the kernels decide it: in float32"""
    f = torch.float32
    view = torch.tensor(inp["obs_view"])
    pose = _t(inp["poses"], f)[view]
    uv = _project(_t(inp["x"], f), pose[:, :, :3], pose[:, :, 3], _t(K, f))
    on = ~torch.isinf(uv).any(dim=-1)
    if inp["sdf"] is not None:
        on = on & (_t(inp["sdf"], f).abs() < torch.tensor(np.float32(inp["bound"])))
    return on


def reproject_term(inp, dtype):
    """err = || uv(R_v x + t_v) - key point || over the COUNTED observations ;  reproj = 0.5 mean(2 log(1 + err^2 / 4)) + 0.5
    mean(err), 0 when none is counted ;  loss = g reproj -> reproj, counted [n] bool, d_x [n,3], d_poses [V,3,4]"""
    x = _t(inp["x"], dtype, True)
    poses = _t(inp["poses"], dtype, True)
    on = reproject_mask(inp)
    rows = torch.nonzero(on).reshape(-1)
    count = int(rows.numel())
    if count == 0:
        return {"reproj": np.float64(0.0), "counted": on.numpy(), "d_x": _grad(x), "d_poses": _grad(poses)}
    pose = poses[torch.tensor(inp["obs_view"])[rows]]
    uv = _project(x[rows], pose[:, :, :3], pose[:, :, 3], _t(K, dtype))
    err = torch.linalg.vector_norm(uv - _t(inp["obs_uv"], dtype)[rows], dim=-1)
    reproj = 0.5 * _sum64(2 * torch.log(1 + err ** 2 / 4)) / count + 0.5 * _sum64(err) / count
    (inp["g"] * reproj).backward()
    return {"reproj": _np(reproj), "counted": on.numpy(), "d_x": _grad(x), "d_poses": _grad(poses)}


def surface_pts(inp, dtype):
    """out = p - n / |n|.detach() * sdf ,  length = |n| ;  loss = <g_out, out> + <g_len, length> (an absent upstream: that output
    is not in the loss) -> out [n,3], length [n], d_n [n,3], d_sdf [n]"""
    nr = _t(inp["normals"], dtype, True)
    sd = _t(inp["sdf"], dtype, True)
    length = torch.linalg.vector_norm(nr, dim=-1)
    out = _t(inp["p"], dtype) - nr / length.detach()[:, None] * sd[:, None]
    loss = 0.0 * length.sum()
    if inp["g_out"] is not None:
        loss = loss + (out * _t(inp["g_out"], dtype)).sum()
    if inp["g_len"] is not None:
        loss = loss + (length * _t(inp["g_len"], dtype)).sum()
    if nr.shape[0] > 0:
        loss.backward()
    return {"out": _np(out), "length": _np(length), "d_n": _grad(nr), "d_sdf": _grad(sd)}


# ------------------------------------------------------------------------------------------------------------ input builders
def _unit(rng, n, k=3):
    v = rng.normal(size=(n, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rotations(rng, n, angle):
    """n rotations by up to `angle` rad about random axes (Rodrigues, float64)"""
    axis = _unit(rng, n)
    th = rng.uniform(-angle, angle, size=n)
    Wm = np.zeros((n, 3, 3))
    Wm[:, 0, 1], Wm[:, 0, 2], Wm[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    Wm -= Wm.transpose(0, 2, 1)
    return np.eye(3) + np.sin(th)[:, None, None] * Wm + (1 - np.cos(th))[:, None, None] * (Wm @ Wm)


def _keypoints(rng, pts, R, t, lo=2.0, hi=8.0):
    """the exact projection of pts [m,3] through (R, t) [m,3,3], [m,3] plus an offset of lo .. hi px in a random direction: the
    pixel error neither cancels nor vanishes"""
    xc = np.einsum("mab,mb->ma", R, pts) + t
    u = xc @ K.astype(np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = u[:, :2] / (u[:, 2:] + C6)
    return uv + _unit(rng, len(pts), 2) * rng.uniform(lo, hi, size=(len(pts), 1))


def tracing_inputs(n, seed, live="all", with_sdf=True, special=True, g_tl=0.75, g_sd=0.25):
    """unit rays, depths in [1, 3], target = surface + a ray + b perp with |a| in [0.5, 1], b in [0, 1]: neither e nor e . ray
    cancels.  live: "all" | "one" (exactly one live row) | "most" (~80 % live, the last row dead) | "none".  special (n >= 63):
    row 5 sits exactly on its target (every operand a small dyadic number: e = 0 in any precision) and sdf_last[7] = 0; both live"""
    rng = np.random.default_rng(seed)
    center = rng.normal(size=(n, 3)) * 0.5
    ray = _unit(rng, n).astype(np.float32).astype(np.float64)
    d = rng.uniform(1.0, 3.0, size=n)
    perp = np.cross(ray, _unit(rng, n))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    a = rng.uniform(0.5, 1.0, size=(n, 1)) * rng.choice([-1.0, 1.0], size=(n, 1))
    target = center + ray * d[:, None] + a * ray + rng.uniform(0.0, 1.0, size=(n, 1)) * perp
    sdf_last = rng.uniform(0.005, 0.05, size=n) * rng.choice([-1.0, 1.0], size=n)
    lv = {"all": np.ones(n), "none": np.zeros(n), "one": np.zeros(n), "most": (rng.uniform(size=n) > 0.2).astype(np.float64)}[live]
    if live == "one":
        lv[(2 * n) // 3] = 1.0
    if live == "most":
        lv[0], lv[-1] = 1.0, 0.0
    if special and n >= 63:
        center[5], ray[5], d[5], target[5] = (0.25, -0.5, 0.75), (0.0, 0.0, 1.0), 2.0, (0.25, -0.5, 2.75)
        sdf_last[7] = 0.0
        if live == "most":
            lv[5] = lv[7] = 1.0
    f = np.float32
    return {"center": center.astype(f), "ray": ray.astype(f), "d": d.astype(f), "target": target.astype(f), "live": lv.astype(f),
            "sdf_last": sdf_last.astype(f) if with_sdf else None, "g_tl": g_tl, "g_sd": g_sd if with_sdf else None}


W_SURF, W_ADD = float(np.float32(10.0 ** 1.5)), float(np.float32(10.0 ** 0.5))


def ba_inputs(n, seed, error=12.0, with_add=True):
    """SDF values of ~1e-2 with one exact zero (n > 1); the error below (3.5), at (10) or above (12) the threshold of 10"""
    rng = np.random.default_rng(seed)
    s = rng.normal(size=n) * 0.01
    if n > 1:
        s[min(11, n - 1)] = 0.0
    return {"reproj": np.float32(error), "sdfs": s.astype(np.float32), "add": np.float32(0.37) if with_add else None, "thresh": 10.0,
            "w_lo": 1.0, "w_hi": 10.0, "w_surf": W_SURF, "w_add": W_ADD if with_add else 0.0, "g": 2.0}


def match_inputs(S, n, seed):
    """S segments of n traced key points; the other view's camera sees every surface point at depth >= 3; key points = exact
    projection + 2 .. 8 px; one exact zero among the last SDF values"""
    rng = np.random.default_rng(seed)
    m = S * n
    f = np.float32
    center = rng.normal(size=(m, 3)) * 0.2
    d = rng.uniform(1.0, 3.0, size=m)
    R = _rotations(rng, S, 0.3)
    t = np.concatenate([rng.normal(size=(S, 2)) * 0.3, rng.uniform(7.0, 8.0, size=(S, 1))], axis=1)       # |pts| < 4: depth > 3
    poses = np.concatenate([R, t[:, :, None]], axis=2).astype(f)
    P = poses.astype(np.float64).repeat(n, axis=0)
    c32, d32 = center.astype(f), d.astype(f)
    d64 = d32.astype(np.float64)

    def image_of(rays, depth):
        xc = np.einsum("mab,mb->ma", P[:, :, :3], c32.astype(np.float64) + rays * depth[:, None]) + P[:, :, 3]
        u = xc @ K.astype(np.float64).T
        return u[:, :2] / (u[:, 2:] + C6)

    # d err / d d = (e / |e|) . (d uv / d d): well-conditioned when the image of the point MOVES as it slides along its ray (a ray
    # that points at the other camera does not: redrawn) and the key point's offset is within 60 degrees of that motion
    r32 = np.zeros((m, 3), dtype=f)
    todo = np.ones(m, dtype=bool)
    while todo.any():
        r32[todo] = _unit(rng, int(todo.sum())).astype(f)
        rays = r32.astype(np.float64)
        motion = (image_of(rays, d64 + 1e-4) - image_of(rays, d64 - 1e-4)) / 2e-4
        todo = np.linalg.norm(motion, axis=1) < 4.0                                                   # px per unit of depth
    along = motion / np.linalg.norm(motion, axis=1, keepdims=True)
    turn = rng.uniform(-np.pi / 3, np.pi / 3, size=m)
    offset = np.stack([np.cos(turn) * along[:, 0] - np.sin(turn) * along[:, 1], np.sin(turn) * along[:, 0] + np.cos(turn) * along[:, 1]], axis=1)
    uv = image_of(rays, d64) + offset * (rng.uniform(2.0, 8.0, size=(m, 1)) * rng.choice([-1.0, 1.0], size=(m, 1)))
    s = rng.normal(size=(S, n)) * 0.01
    s[S - 1, n // 2] = 0.0
    return {"center": c32, "ray": r32, "uv_obs": uv.astype(f), "poses": poses, "d": d32.reshape(S, n), "sdf_last": s.astype(f),
            "g0": 0.5, "g1": 2.0}


def reproject_inputs(counts, seed, masked=False, inf_view=None):
    """observations sorted by view, counts[v] of view v; camera depths in [3, 6]; key points = exact projection + 2 .. 8 px.
    masked: SDF values against the bound 0.03 (fp32) -- about a third clearly outside, the rest clearly inside, row 1 EXACTLY at
    the bound (not counted) and row 2 the next float below it (counted).  inf_view: that view's pose is the identity and its LAST
    observation has x_z = -float32(1e-6), x_x != 0: u_z + 1e-6 = 0 exactly, its projection is infinite (not counted)."""
    rng = np.random.default_rng(seed)
    V, n = len(counts), int(sum(counts))
    f = np.float32
    R = _rotations(rng, V, 0.4)
    t = np.concatenate([rng.normal(size=(V, 2)) * 0.3, rng.uniform(3.5, 4.5, size=(V, 1))], axis=1)
    if inf_view is not None:
        R[inf_view], t[inf_view] = np.eye(3), 0.0
    poses = np.concatenate([R, t[:, :, None]], axis=2).astype(f)
    view = np.concatenate([np.full(c, v, dtype=np.int64) for v, c in enumerate(counts)]) if n else np.zeros(0, dtype=np.int64)
    P = poses.astype(np.float64)[view]
    xc = np.stack([rng.uniform(-1.5, 1.5, size=n), rng.uniform(-1.0, 1.0, size=n), rng.uniform(3.0, 6.0, size=n)], axis=1)
    x = np.einsum("mba,mb->ma", P[:, :, :3], xc - P[:, :, 3]).astype(f)                       # R^T (x_c - t)
    if inf_view is not None:
        x[int(np.sum(counts[:inf_view + 1])) - 1] = (0.3, 0.2, -np.float32(1e-6))
    uv = _keypoints(rng, x.astype(np.float64), P[:, :, :3], P[:, :, 3]) if n else np.zeros((0, 2))
    uv = np.where(np.isfinite(uv), uv, 10.0)
    sdf, bound = None, float("inf")
    if masked:
        bound = float(f(0.03))
        mag = np.where(rng.uniform(size=n) < 0.3, rng.uniform(0.04, 0.06, size=n), rng.uniform(0.0, 0.02, size=n))
        sdf = (mag * rng.choice([-1.0, 1.0], size=n)).astype(f)
        sdf[1], sdf[2] = f(0.03), -np.nextafter(f(0.03), f(0.0))
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return {"x": x, "poses": poses, "obs_view": view, "view_start": start, "obs_uv": uv.astype(f), "sdf": sdf, "bound": bound, "g": 3.0,
            "inf_row": None if inf_view is None else int(start[inf_view + 1]) - 1}


def surface_inputs(n, seed, g_out=True, g_len=True):
    """normals of length 0.5 .. 2, SDF values of ~5e-2, upstreams of ~1; the upstream of `out` is a normal + b perp with |a| in
    [0.5, 1], b in [0, 1]: d sdf = -<g_out, normal / |normal|> does not cancel"""
    rng = np.random.default_rng(seed)
    f = np.float32
    unit = _unit(rng, n)
    nr = unit * rng.uniform(0.5, 2.0, size=(n, 1))
    perp = np.cross(unit, _unit(rng, n))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    go = unit * rng.uniform(0.5, 1.0, size=(n, 1)) * rng.choice([-1.0, 1.0], size=(n, 1)) + perp * rng.uniform(0.0, 1.0, size=(n, 1))
    return {"p": rng.normal(size=(n, 3)).astype(f), "normals": nr.astype(f), "sdf": (rng.normal(size=n) * 0.05).astype(f),
            "g_out": go.astype(f) if g_out else None, "g_len": rng.normal(size=n).astype(f) if g_len else None}


# ------------------------------------------------------------------------------------------------------------------ the cases
TT_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
TRACING_CASES = {}
for _n in TT_SIZES:
    for _sdf in (False, True):
        for _live in ("all", "one", "most"):
            if _n == 1 and _live != "all":                        # (n = 1: "one" is "all", "most" is the all-dead case below)
                continue
            TRACING_CASES[f"n{_n}-{'sdf' if _sdf else 'nosdf'}-{_live}"] = dict(n=_n, seed=1000 + _n, live=_live, with_sdf=_sdf)
TRACING_CASES["n1025-only_tl"] = dict(n=1025, seed=41, live="most", g_sd=None)          # upstream on one term only
TRACING_CASES["n1025-only_sd"] = dict(n=1025, seed=42, live="most", g_tl=None)
TRACING_CASES["n65-all_dead"] = dict(n=65, seed=43, live="none")                        # 0 / 0: NaN terms, NaN-for-NaN gradients

BA_CASES = {f"n{_n}-above-add": dict(n=_n, seed=2000 + _n) for _n in (1, 63, 65, 1023, 1024, 1025, 2049)}
BA_CASES.update({"n65-below-add": dict(n=65, seed=51, error=3.5), "n65-at-noadd": dict(n=65, seed=52, error=10.0, with_add=False),
                 "n1025-above-noadd": dict(n=1025, seed=53, with_add=False), "n1025-at-add": dict(n=1025, seed=54, error=10.0)})

MATCH_CASES = {f"S{_s}-n65": dict(S=_s, n=65, seed=3000 + _s) for _s in (1, 2, 3, 4)}
MATCH_CASES.update({f"S2-n{_n}": dict(S=2, n=_n, seed=3100 + _n) for _n in (1, 1023, 1024, 1025, 2049)})

REPROJECT_CASES = {
    "1": dict(counts=[1], seed=61), "0-1-0": dict(counts=[0, 1, 0], seed=62), "255-256-257": dict(counts=[255, 256, 257], seed=63),
    "1-0-513-2": dict(counts=[1, 0, 513, 2], seed=64, inf_view=3), "0-0": dict(counts=[0, 0], seed=65),
    "300-64-masked": dict(counts=[300, 64], seed=66, masked=True, inf_view=1)}

SURFACE_CASES = {f"n{_n}-{_u}": dict(n=_n, seed=4000 + _n, g_out=_u != "len", g_len=_u != "out")
                 for _n in (0, 1, 255, 256, 257) for _u in ("both", "out", "len")}

FAMILIES = {"tracing": (TRACING_CASES, tracing_inputs, tracing_term), "ba": (BA_CASES, ba_inputs, ba_terms),
            "match": (MATCH_CASES, match_inputs, match_term), "reproject": (REPROJECT_CASES, reproject_inputs, reproject_term),
            "surface": (SURFACE_CASES, surface_inputs, surface_pts)}
# how each compared quantity is measured
KIND = {"tl": "scalar", "ss": "scalar", "d_d": "elem", "d_sdf": "elem", "surf": "scalar", "w": "scalar", "extra": "scalar",
        "d_reproj": "scalar", "d_sdfs": "elem", "d_add": "scalar", "re": "scalar", "surface": "row", "reproj": "scalar", "d_x": "row",
        "d_poses": "view", "out": "row", "length": "elem", "d_n": "row"}


@functools.lru_cache(maxsize=None)
def case(family, name):
    """-> (inputs, float64 statement, float32 statement) of one case, evaluated once and shared (read-only)"""
    cases, build, term = FAMILIES[family]
    inp = build(**cases[name])
    return inp, term(inp, torch.float64), term(inp, torch.float32)


# ------------------------------------------------------------------------------------------------------------- the comparison
def distance(kind, got, ref):
    """the largest relative distance of `got` from `ref` in the measure of `kind`; inf where exact zero or NaN is not met"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    if kind in ("scalar", "elem"):
        got, ref = got.reshape(-1, 1), ref.reshape(-1, 1)
    elif kind == "row":
        got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    else:
        got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    if (np.isnan(got) != np.isnan(ref)).any():
        return float("inf")
    got, ref = np.where(np.isnan(ref), 0.0, got), np.where(np.isnan(ref), 0.0, ref)
    scale = np.abs(ref).max(axis=1)
    diff = np.abs(got - ref).max(axis=1)
    zero = scale == 0.0
    if (diff[zero] != 0.0).any():
        return float("inf")
    return float((diff[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0


def check(family, name, key, got, ref64, ref32, bar=EPS):
    """one quantity of one case against float64: prints the device's and the CPU-fp32 statement's distance, returns the failure
    or None"""
    d, c = distance(KIND[key], got, ref64), distance(KIND[key], ref32, ref64)
    print(f"[terms] {family:9s} {name:18s} {key:9s} device-fp64 {d:.3e}  cpu-fp32-fp64 {c:.3e}  bar {bar:.1e}")
    return None if d <= bar else (family, name, key, d)
