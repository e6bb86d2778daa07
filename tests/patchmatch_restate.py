"""THE PLANE SCORE and THE PATCHMATCH STEP of include/ls2fm.h (ls2fm_mvs_plane_score, ls2fm_mvs_patchmatch_step) restated in plain
numpy for this project: float32 arrays over a set of pixels of one reference view, the references, candidates, sources and window
taps in loops, so that every fp32 operation rounds once, in the order the header gives.  The lift, the relative poses, the
window's sums and the sample of a camera point are mvs_restate's, the camera point, projection and usable rule raster_restate's.  Test infrastructure only."""
import numpy as np

import mvs_restate as MR
import raster_restate as R

F32 = np.float32
NAN = F32(np.nan)
U64 = np.uint64
MASK = U64(0xFFFFFFFF)
MIX_A, MIX_B, MIX_SALT = 0x21F0AAAD, 0x735A2D97, 0x9E3779B9     # LS2FM_MVS_MIX_A, _B, _SALT
NEIGHBOURS = [(0, -1), (-1, 0), (1, 0), (0, 1), (0, -3), (-3, 0), (3, 0), (0, 3)]
N_DRAWS = 9


# ------------------------------------------------------------------------------------------------------------------- the draws
def mix(x):
    """the 32-bit finaliser of the header on uint64 arrays that hold 32-bit values"""
    x = np.asarray(x, U64) & MASK
    x = x ^ (x >> U64(16))
    x = (x * U64(MIX_A)) & MASK
    x = x ^ (x >> U64(15))
    x = (x * U64(MIX_B)) & MASK
    return x ^ (x >> U64(15))


def draw(seed, view, iteration, pixel, j):
    """u_j float32 in [0, 1) of the pixels `pixel` (py W + px) of view `view`"""
    h = mix(U64((int(seed) + MIX_SALT) & 0xFFFFFFFF))
    h = mix(h + U64(int(view)))
    h = mix(h + U64(int(iteration)))
    h = mix(h + np.asarray(pixel, U64))
    u = (mix(h + U64(int(j))) >> U64(8)).astype(F32) * F32(2.0 ** -24)
    assert u.dtype == F32
    return u


def schedule(rho, iteration):
    """rho 2^-iteration, formed in fp64 and rounded once"""
    return F32(np.float64(rho) * 2.0 ** -int(iteration))


def normalise(x, y, z):
    s = (x * x + y * y) + z * z
    root = np.sqrt(s.astype(np.float64)).astype(F32)
    assert s.dtype == F32
    return x / root, y / root, z / root


# ------------------------------------------------------------------------------------------------------------------ the context
class Scene:
    """the inputs of both rules and, per reference, what does not depend on the hypothesis: the lift and step 1's ma, va"""

    def __init__(self, images, poses, intr, sources, refs=None, half_width=3, tap_step=1, near=1e-3, min_var=1e-6, min_sources=1):
        self.img = np.asarray(images, F32)
        self.V, self.H, self.W = self.img.shape
        self.refs = np.arange(self.V) if refs is None else np.asarray(refs, np.int64).reshape(-1)
        self.sources = np.asarray(sources, np.int64).reshape(len(self.refs), -1)
        self.k4 = R.intr4(intr, self.V)
        self.rel = MR.relative_poses(poses, self.refs, self.sources)
        self.w, self.t, self.near, self.mv, self.min_sources = int(half_width), int(tap_step), near, F32(min_var), int(min_sources)
        side = range(0, 2 * self.w + 1, self.t)
        self.offsets = [(j - self.w, i - self.w) for i in side for j in side]            # (dx, dy), dy outer
        self.picked = [i * (2 * self.w + 1) + j for i in side for j in side]               # their places among MR.taps
        self.n = F32(len(self.offsets))
        yy, xx = np.mgrid[0:self.H, 0:self.W]
        w = self.w
        self.has_window = (xx >= w) & (xx <= self.W - 1 - w) & (yy >= w) & (yy <= self.H - 1 - w)
        self.per_ref = {}

    def reference(self, r):
        """xn [W], yn [H], ma, va, pixel_ok [H, W] of reference r (None for a view outside [0, V))"""
        if r not in self.per_ref:
            rv = int(self.refs[r])
            if not 0 <= rv < self.V:
                self.per_ref[r] = None
                return None
            with np.errstate(all="ignore"):
                _, finite, ma, va = MR.window_stats(self.img[rv], self.w, self.picked)
                xn, yn = MR.lift(self.k4[rv], self.H, self.W)
            self.per_ref[r] = dict(rv=rv, xn=xn[0], yn=yn[:, 0], ma=ma, va=va, pixel_ok=self.has_window & finite & ~(va < self.mv))
        return self.per_ref[r]


def _note(stats):
    if stats is None:
        return lambda name, m: None
    return lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(np.count_nonzero(m)))


# --------------------------------------------------------------------------------------------------------------- THE PLANE SCORE
def score_pixels(sc, r, py, px, d, n, stats=None):
    """THE PLANE SCORE of the hypotheses (d [N], n [N, 3]) at the pixels (px, py) of reference r -> float32 [N]"""
    note = _note(stats)
    N = len(py)
    ref = sc.reference(r)
    if ref is None or N == 0:
        return np.full(N, NAN, F32)
    d, n = np.asarray(d, F32), np.asarray(n, F32).reshape(N, 3)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        xp, yp = ref["xn"][px], ref["yn"][py]
        gp = (nx * xp + ny * yp) + nz
        pixel_ok = ref["pixel_ok"][py, px]
        normal_ok = np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz)
        depth_ok = np.isfinite(d) & (d > 0)
        ok = pixel_ok & depth_ok & normal_ok & (gp < 0)
        note("depth is NaN", pixel_ok & np.isnan(d))
        note("depth is zero", pixel_ok & (d == 0))
        note("depth is negative", pixel_ok & (d < 0))
        note("depth is +inf", pixel_ok & (d == np.inf))
        note("normal not finite", pixel_ok & depth_ok & ~normal_ok)
        note("g_p == 0", pixel_ok & depth_ok & normal_ok & (gp == 0))
        note("normal faces away", pixel_ok & depth_ok & normal_ok & (gp > 0))
        h = gp * d
        a, pts, any_sign = [], [], np.zeros(N, bool)
        for dx, dy in sc.offsets:
            qx, qy = np.clip(px + dx, 0, sc.W - 1), np.clip(py + dy, 0, sc.H - 1)
            xq, yq = ref["xn"][qx], ref["yn"][qy]
            gq = (nx * xq + ny * yq) + nz
            dq = h / gq
            tap_ok = (gq < 0) & np.isfinite(dq)
            any_sign |= ~(gq < 0)
            a.append(sc.img[ref["rv"]][qy, qx])
            pts.append((xq * dq, yq * dq, dq, tap_ok))
        note("g_q changes sign in the window", ok & any_sign)
        ma, va = ref["ma"][py, px], ref["va"][py, px]
        total, count = np.zeros(N, F32), np.zeros(N, np.int64)
        for s in range(sc.sources.shape[1]):
            sv = int(sc.sources[r, s])
            if not 0 <= sv < sc.V:
                continue
            b = [np.where(tap_ok, MR.sample(sc.img[sv], sc.rel[r, s], sc.k4[sv], X, Y, Z, sc.near), NAN) for X, Y, Z, tap_ok in pts]
            sb, finite = np.zeros(N, F32), np.ones(N, bool)
            for bi in b:
                sb = sb + bi
                finite &= np.isfinite(bi)
            mb = sb / sc.n
            vb, cov = np.zeros(N, F32), np.zeros(N, F32)
            for ai, bi in zip(a, b):
                vb = vb + (bi - mb) * (bi - mb)
                cov = cov + (ai - ma) * (bi - mb)
            valid = ok & finite & ~(vb < sc.mv)
            ncc = cov / np.sqrt((va * vb).astype(np.float64)).astype(F32)
            assert ncc.dtype == F32 and cov.dtype == F32 and mb.dtype == F32
            total = np.where(valid, total + ncc, total)
            count += valid
        note("count == min_sources - 1", ok & (count == sc.min_sources - 1))
        return np.where(ok & (count >= sc.min_sources), total / count.astype(F32), NAN)


def plane_score(sc, depth, normal, stats=None):
    """THE PLANE SCORE of a state at every pixel: depth [R, H, W], normal [R, H, W, 3] -> score float32 [R, H, W]"""
    depth, normal = np.asarray(depth, F32), np.asarray(normal, F32)
    out = np.full(depth.shape, NAN, F32)
    yy, xx = np.mgrid[0:sc.H, 0:sc.W]
    py, px = yy.reshape(-1), xx.reshape(-1)
    for r in range(len(sc.refs)):
        out[r] = score_pixels(sc, r, py, px, depth[r].reshape(-1), normal[r].reshape(-1, 3), stats).reshape(sc.H, sc.W)
    return out


# ----------------------------------------------------------------------------------------------------------- THE PATCHMATCH STEP
def step(sc, depth, normal, score, colour, iteration, seed, depth_perturb, normal_perturb, max_slope, d_min, d_max, stats=None):
    """one half-sweep of one colour, in place on depth [R, H, W], normal [R, H, W, 3], score [R, H, W] (float32 arrays).
    depth_perturb and normal_perturb are the values before the schedule."""
    note = _note(stats)
    assert depth.dtype == F32 and normal.dtype == F32 and score.dtype == F32
    rho_d, rho_n, sigma = schedule(depth_perturb, iteration), schedule(normal_perturb, iteration), F32(max_slope)
    d_min, d_max = np.asarray(d_min, F32).reshape(-1), np.asarray(d_max, F32).reshape(-1)
    yy, xx = np.mgrid[0:sc.H, 0:sc.W]
    mine = sc.has_window & (((xx + yy) & 1) == int(colour))
    py, px = yy[mine], xx[mine]
    N = len(py)
    one, two = F32(1), F32(2)
    with np.errstate(all="ignore"):
        for r in range(len(sc.refs)):
            ref = sc.reference(r)
            if ref is None or N == 0:
                continue
            best_d, best_n, best_s = depth[r][py, px].copy(), normal[r][py, px].copy(), score[r][py, px].copy()
            u = [draw(seed, ref["rv"], iteration, py * sc.W + px, j) for j in range(N_DRAWS)]
            xp, yp = ref["xn"][px], ref["yn"][py]

            def consider(cd, cn, active, name):
                nonlocal best_d, best_n, best_s
                s = np.full(N, NAN, F32)
                if active.any():
                    s[active] = score_pixels(sc, r, py[active], px[active], cd[active], cn[active], stats)
                note("a candidate ties the incumbent", active & (s == best_s))
                better = active & ~np.isnan(s) & (np.isnan(best_s) | (s > best_s))
                note(name, better)
                best_d = np.where(better, cd, best_d)
                best_n = np.where(better[:, None], cn, best_n)
                best_s = np.where(better, s, best_s)

            # 1. the eight neighbours
            for dx, dy in NEIGHBOURS:
                mx, my = px + dx, py + dy
                inside = (mx >= 0) & (mx < sc.W) & (my >= 0) & (my < sc.H)
                cx_, cy_ = np.clip(mx, 0, sc.W - 1), np.clip(my, 0, sc.H - 1)
                dm, nm = depth[r][cy_, cx_], normal[r][cy_, cx_]
                has = np.isfinite(dm) & (dm > 0)
                note("neighbour outside the image", ~inside)
                note("neighbour without a depth", inside & ~has)
                gm = (nm[:, 0] * ref["xn"][cx_] + nm[:, 1] * ref["yn"][cy_]) + nm[:, 2]
                gpm = (nm[:, 0] * xp + nm[:, 1] * yp) + nm[:, 2]
                cd = (gm * dm) / gpm
                assert cd.dtype == F32
                consider(cd, nm, inside & has, "a neighbour's plane wins")
            # 2. to 4.: perturbations about the best so far, skipped without a hypothesis
            have = ~np.isnan(best_s)
            note("no hypothesis to perturb", ~have)

            def deeper(j):
                return best_d * (one + rho_d * (two * u[j] - one))

            def turned(j):
                x = best_n[:, 0] + rho_n * (two * u[j] - one)
                y = best_n[:, 1] + rho_n * (two * u[j + 1] - one)
                return np.stack(normalise(x, y, best_n[:, 2]), axis=1)

            consider(deeper(0), best_n, have, "the perturbed depth wins")
            consider(best_d, turned(1), have, "the perturbed normal wins")
            consider(deeper(3), turned(4), have, "both perturbations win")
            # 5. a fresh hypothesis
            lo, hi = one / d_min[r], one / d_max[r]
            fd = one / (lo + u[6] * (hi - lo))
            fn = np.stack(normalise(sigma * (two * u[7] - one), sigma * (two * u[8] - one), np.full(N, -1, F32)), axis=1)
            assert fd.dtype == F32 and fn.dtype == F32
            consider(fd, fn, np.ones(N, bool), "the fresh hypothesis wins")
            depth[r][py, px], normal[r][py, px], score[r][py, px] = best_d, best_n, best_s


def patch_match(images, poses, intr, sources, depths, refs=None, iterations=5, init=None, seed=0, depth_perturb=0.02, normal_perturb=0.5,
                max_slope=1.0, tap_step=1, half_width=3, near=1e-3, min_var=1e-6, min_sources=1, stats=None):
    """ls2fm.mvs.patch_match restated -> depth [R, H, W], normal [R, H, W, 3], score [R, H, W]"""
    sc = Scene(images, poses, intr, sources, refs, half_width, tap_step, near, min_var, min_sources)
    depths = np.asarray(depths, F32)
    depths = np.broadcast_to(depths, (len(sc.refs), depths.shape[-1]))
    if init is None:
        depth = MR.sweep(images, poses, intr, sources, depths, refs=refs, half_width=half_width, near=near, min_var=min_var,
                         min_sources=min_sources)[0]
        normal = np.zeros(depth.shape + (3,), F32)
        normal[..., 2] = -1
    else:
        depth, normal = np.array(init[0], F32), np.array(init[1], F32)
    score = plane_score(sc, depth, normal, stats)
    for it in range(int(iterations)):
        for colour in (0, 1):
            step(sc, depth, normal, score, colour, it, seed, depth_perturb, normal_perturb, max_slope, depths[:, 0], depths[:, -1], stats)
    dead = np.isnan(score)
    depth[dead] = NAN
    normal[dead] = NAN
    return depth, normal, score
