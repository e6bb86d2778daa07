"""numpy restatement of THE POISSON RULE of include/ls2fm.h, written for this project (no device, no torch): every lattice operation
is one float32 numpy operation in the order the rule states, the fixed-point sums of the splat go through np.add.at on int64.  The
stages are functions of their own (splat, finish, rhs, sweep_colour, residual, restrict, prolong) so that the kernels can be held to
each by bits; solve runs the cycles.  assemble is the fp64 matrix of the same equations, a reference independent of the cycle."""
import numpy as np

F32 = np.float32
TO_FIXED = 2.0 ** 32
COARSEST_SWEEPS, PRE_SWEEPS, POST_SWEEPS = 32, 2, 2


def level_shapes(shape):
    """the shapes of the levels: a coarse side is (n + 1) // 2; level l + 1 exists while level l has min >= 4 and max >= 5"""
    out = [tuple(int(s) for s in shape)]
    while min(out[-1]) >= 4 and max(out[-1]) >= 5:
        out.append(tuple((n + 1) // 2 for n in out[-1]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the splat
def splat(points, normals, shape, origin, voxel):
    """int64 [4, n0 n1 n2]: the fixed-point sums of w N_0, w N_1, w N_2 and w over the eight corners of every point's cell"""
    P, N = np.asarray(points, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    n = np.array(shape, np.int64)
    acc = np.zeros((4, int(np.prod(n))), np.int64)
    if len(P) == 0:
        return acc
    with np.errstate(all="ignore"):
        u = (P - np.asarray(origin, F32)[None]) / F32(voxel)
        i = np.floor(u)
        f = u - i
        ok = np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1) & (u >= F32(0)).all(axis=1) & (u < (n - 1).astype(F32)[None]).all(axis=1)
    i, f, N = i[ok].astype(np.int64), f[ok], N[ok].astype(np.float64)
    assert f.dtype == F32
    for dx in (0, 1):
        wx = f[:, 0] if dx else F32(1) - f[:, 0]
        for dy in (0, 1):
            wxy = wx * (f[:, 1] if dy else F32(1) - f[:, 1])
            for dz in (0, 1):
                w = (wxy * (f[:, 2] if dz else F32(1) - f[:, 2])).astype(np.float64)
                at = ((i[:, 0] + dx) * n[1] + (i[:, 1] + dy)) * n[2] + (i[:, 2] + dz)
                for a in range(3):
                    np.add.at(acc[a], at, np.rint(w * N[:, a] * TO_FIXED).astype(np.int64))
                np.add.at(acc[3], at, np.rint(w * TO_FIXED).astype(np.int64))
    return acc


def finish(acc, shape):
    """(V float32 [3, n0, n1, n2], W float32 [n0, n1, n2]) of the sums"""
    out = (acc.astype(np.float64) * (1.0 / TO_FIXED)).astype(F32).reshape(4, *shape)
    return out[:3], out[3]


def _axis(axis, s):
    idx = [slice(None)] * 3
    idx[axis] = s
    return tuple(idx)


def rhs(V):
    """b float32 [n0, n1, n2]: per axis the edge targets g = 0.5 (V_a[i] + V_a[i + e_a]) and their difference, a missing edge 0"""
    shape = V.shape[1:]
    t = []
    for a in range(3):
        g = F32(0.5) * (V[a][_axis(a, slice(0, -1))] + V[a][_axis(a, slice(1, None))])
        pad = np.zeros(tuple(s + (1 if x == a else 0) for x, s in enumerate(shape)), F32)
        pad[_axis(a, slice(1, -1))] = g
        t.append(pad[_axis(a, slice(0, -1))] - pad[_axis(a, slice(1, None))])
    return (t[0] + t[1]) + t[2]


# -------------------------------------------------------------------------------------------------------------- the operator
def neighbour_sum(chi):
    """(N, deg) float32: the existing neighbours in the order -0, +0, -1, +1, -2, +2 from the first that exists, and their count"""
    N, deg, has = np.zeros_like(chi), np.zeros(chi.shape, F32), np.zeros(chi.shape, bool)
    for a in range(3):
        for lo, hi in ((slice(1, None), slice(0, -1)), (slice(0, -1), slice(1, None))):
            nb, ex = np.zeros_like(chi), np.zeros(chi.shape, bool)
            nb[_axis(a, lo)] = chi[_axis(a, hi)]
            ex[_axis(a, lo)] = True
            with np.errstate(all="ignore"):
                N = np.where(ex, np.where(has, N + nb, nb), N)
            has |= ex
            deg = deg + ex.astype(F32)
    return N, deg


def parity(shape):
    i = np.indices(shape).sum(axis=0)
    return i & 1


def level_scale(level):
    return F32(4.0 ** -level)


def sweep_colour(chi, b, W, s, a, colour):
    """one colour of one red-black Gauss-Seidel sweep -> the new chi (a copy)"""
    s, a = F32(s), F32(a)
    N, deg = neighbour_sum(chi)
    with np.errstate(all="ignore"):
        new = (b + s * N) / (s * deg + a * W)
    return np.where(parity(chi.shape) == colour, new, chi).astype(F32)


def sweep(chi, b, W, s, a):
    return sweep_colour(sweep_colour(chi, b, W, s, a, 0), b, W, s, a, 1)


def residual(chi, b, W, s, a):
    s, a = F32(s), F32(a)
    N, deg = neighbour_sum(chi)
    with np.errstate(all="ignore"):
        return (b - (s * (deg * chi - N) + (a * W) * chi)).astype(F32)


# --------------------------------------------------------------------------------------------------------------- the transfers
def _restrict_axis(r, axis):
    r = np.moveaxis(r, axis, 0)
    n = r.shape[0]
    nc, m = (n + 1) // 2, n // 2
    with np.errstate(all="ignore"):
        acc = F32(0.5) * r[0::2]
        acc[1:] = acc[1:] + F32(0.25) * r[1:2 * nc - 2:2]
        c = np.full((m, 1, 1), 0.25, F32)
        if n % 2 == 0:
            c[-1] = 0.5
        acc[:m] = acc[:m] + c * r[1::2]
    return np.moveaxis(acc, 0, axis)


def restrict(r):
    """the transpose of the prolongation, halved per axis, axes 0, 1, 2 in turn; no renormalisation at the boundary"""
    for axis in range(3):
        r = _restrict_axis(r, axis)
    return np.ascontiguousarray(r, F32)


def _prolong_axis(e, axis, n):
    e = np.moveaxis(e, axis, 0)
    nc = e.shape[0]
    out = np.empty((n,) + e.shape[1:], F32)
    out[0::2] = e
    k = np.arange(n // 2)
    with np.errstate(all="ignore"):
        out[1::2] = F32(0.5) * (e[k] + e[np.minimum(k + 1, nc - 1)])
    return np.moveaxis(out, 0, axis)


def prolong(e, shape):
    for axis in range(3):
        e = _prolong_axis(e, axis, shape[axis])
    return np.ascontiguousarray(e, F32)


def correct(chi, e):
    with np.errstate(all="ignore"):
        return (chi + prolong(e, chi.shape)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ the cycle
def densities(W):
    """W of every level: W_{l + 1} = R W_l"""
    out = [np.ascontiguousarray(W, F32)]
    for _ in level_shapes(W.shape)[1:]:
        out.append(restrict(out[-1]))
    return out


def cycle(level, chi, b, Ws, a, gamma):
    s = level_scale(level)
    if level == len(Ws) - 1:
        for _ in range(COARSEST_SWEEPS):
            chi = sweep(chi, b, Ws[level], s, a)
        return chi
    for _ in range(PRE_SWEEPS):
        chi = sweep(chi, b, Ws[level], s, a)
    for _ in range(gamma):
        coarse_b = restrict(residual(chi, b, Ws[level], s, a))
        chi = correct(chi, cycle(level + 1, np.zeros_like(coarse_b), coarse_b, Ws, a, gamma))
    for _ in range(POST_SWEEPS):
        chi = sweep(chi, b, Ws[level], s, a)
    return chi


def solve_lattice(b, W, screen=4.0, cycles=8, gamma=2, history=None):
    """chi after `cycles` calls of cycle(0) from zero; history: a list that receives max |r| before the first and after every cycle"""
    Ws = densities(W)
    chi = np.zeros_like(b)
    if history is not None:
        history.append(float(np.abs(residual(chi, b, W, 1.0, screen)).max()))
    for _ in range(cycles):
        chi = cycle(0, chi, b, Ws, F32(screen), gamma)
        if history is not None:
            history.append(float(np.abs(residual(chi, b, W, 1.0, screen)).max()))
    return chi


def system(points, normals, shape, origin, voxel):
    """(b, W) of a cloud on a lattice"""
    V, W = finish(splat(points, normals, shape, origin, voxel), shape)
    return rhs(V), np.ascontiguousarray(W)


def solve(points, normals, shape, origin, voxel, screen=4.0, cycles=8, gamma=2):
    """(value, density) float32 [n0, n1, n2]: what ls2fm_poisson_solve writes"""
    b, W = system(points, normals, shape, origin, voxel)
    return solve_lattice(b, W, screen, cycles, gamma), W


def relative_residual(chi, b, W, screen):
    """max |r| / max |b| at level 0 (0 when b vanishes): what cloud_mesh.poisson_residual reports"""
    top = float(np.abs(b).max())
    return float(np.abs(residual(chi, b, W, 1.0, screen)).max()) / top if top > 0 else 0.0


# ----------------------------------------------------------------------------------------------------- the independent reference
def assemble(b, W, screen):
    """(A, b) fp64 of the level-0 equations (deg_i + screen W_i) chi_i - sum of the neighbours = b_i, dense"""
    shape = b.shape
    total = b.size
    index = np.arange(total).reshape(shape)
    A = np.zeros((total, total))
    for a in range(3):
        i, j = index[_axis(a, slice(0, -1))].reshape(-1), index[_axis(a, slice(1, None))].reshape(-1)
        A[i, j] -= 1.0
        A[j, i] -= 1.0
        A[i, i] += 1.0
        A[j, j] += 1.0
    A[np.arange(total), np.arange(total)] += float(F32(screen)) * W.reshape(-1).astype(np.float64)
    return A, b.reshape(-1).astype(np.float64)
