"""THE FUSION RULE of include/ls2fm.h (ls2fm_tsdf_integrate) and ls2fm.fusion.extract restated in plain numpy for this project:
float32 arrays over the lattice points, the views in a loop, so that every fp32 operation rounds once, in the order the header
gives.  The camera point, projection and usable rule are raster_restate's; marching cubes is mc_restate's.  Test infrastructure
only."""
import numpy as np

import mc_restate
import raster_restate as R

F32 = np.float32


def lattice(shape, origin, voxel):
    """X float32 [nx ny nz, 3]: X[a] = fl32(fl32((float) i[a] * voxel) + origin[a]), row-major with axis 2 fastest"""
    og = np.asarray(origin, F32)
    axes = [np.arange(n, dtype=np.int64).astype(F32) * F32(voxel) + og[a] for a, n in enumerate(shape)]
    assert all(t.dtype == F32 for t in axes)
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def new_state(shape):
    return np.zeros(shape, F32), np.zeros(shape, F32)


def integrate(state, origin, voxel, trunc, depth, poses, intr, near=1e-3, max_depth=np.inf, view_weight=None, max_weight=np.inf,
              stats=None):
    """extend state = (tsdf float32 [nx, ny, nz], weight float32 [nx, ny, nz]) in place by the views given -> state.  stats: a
    dict that collects, by name, how many (point, view) pairs met each edge of the rule (the tests assert their scenes are live)"""
    tsdf, weight = state
    shape = tsdf.shape
    X = lattice(shape, origin, voxel)
    depth = np.asarray(depth, F32)
    N, H, W = depth.shape
    poses = np.asarray(poses, F32).reshape(-1, 3, 4)
    k4 = R.intr4(intr, N)
    tr, md, mw = F32(trunc), F32(max_depth), F32(max_weight)
    T, Wt = tsdf.reshape(-1), weight.reshape(-1)
    with np.errstate(all="ignore"):
        for n in range(N):
            # 3. the view's weight (first here: it does not depend on the point)
            w = F32(1.0) if view_weight is None else F32(view_weight[n])
            if not w > 0:
                continue
            # 1. usable, in the image, pixel
            cz, u, v, usable = R.project(X, poses[n], k4[n], near)
            ok = usable & (u >= F32(0)) & (u < F32(W)) & (v >= F32(0)) & (v < F32(H))
            image = ok.copy()
            px = np.where(ok, np.floor(u), 0).astype(np.int64)
            py = np.where(ok, np.floor(v), 0).astype(np.int64)
            # 2. depth at the nearest pixel
            d = depth[n, py, px]
            ok &= np.isfinite(d) & (d > F32(0)) & (d <= md)
            # 4. projective distance
            s = d - cz
            if stats is not None:
                note = lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(np.count_nonzero(m)))
                note("c_z == near", image & (cz == F32(near)))
                note("behind the camera", cz < 0)
                note("u == 0", image & (u == 0))
                note("u == width", usable & (u == F32(W)))
                note("v == height", usable & (v == F32(H)))
                for name, m in (("d nan", np.isnan(d)), ("d +inf", d == np.inf), ("d -inf", d == -np.inf), ("d zero", d == 0),
                                ("d negative", np.isfinite(d) & (d < 0)), ("d == max_depth", d == md),
                                ("d one ulp above max_depth", d == np.nextafter(md, F32(np.inf)))):
                    note(name, image & m)
                note("s == -trunc", ok & (s == -tr))
                note("s one ulp below -trunc", ok & (s == np.nextafter(-tr, F32(-np.inf))))
                note("s == trunc", ok & (s == tr))
                note("s > trunc", ok & (s > tr))
                note("c_z is NaN", np.isnan(cz))
            ok &= ~(s < -tr)
            # 5. - 8.
            val = np.fmin(F32(1.0), s / tr)
            Wn = Wt + w
            if stats is not None:
                note("max_weight reached exactly", ok & (Wn == mw))
                note("max_weight passed", ok & (Wn > mw))
                note("integrated", ok)
            Tn = (Wt * T + w * val) / Wn
            assert s.dtype == F32 and val.dtype == F32 and Wn.dtype == F32 and Tn.dtype == F32
            T[ok] = Tn[ok]
            Wt[ok] = np.fmin(Wn, mw)[ok]
    return state


def fuse(shape, origin, voxel, trunc, depth, poses, intr, **kw):
    """a fresh volume with all the views integrated -> (tsdf, weight)"""
    return integrate(new_state(shape), origin, voxel, trunc, depth, poses, intr, **kw)


def drop_non_finite(verts, faces):
    """ls2fm.fusion.extract's step 3: the faces with a non-finite vertex coordinate go, then the vertices no face uses, both in
    their order -> (verts float32, faces int32, kept_faces bool [F])"""
    verts, faces = np.asarray(verts, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    good = np.isfinite(verts).all(axis=1)
    keep = good[faces].all(axis=1)
    kept = faces[keep]
    used = np.zeros(len(verts), bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    return verts[used], renumber[kept].astype(np.int32), keep


def extract(tsdf, weight, origin, voxel, min_weight=1.0):
    """-> (verts float32 [V, 3], faces int32 [F, 3])"""
    with np.errstate(invalid="ignore"):
        vol = np.where(weight >= F32(min_weight), tsdf, F32(np.nan)).astype(F32)
        v, f = mc_restate.marching_cubes(vol, 0.0, spacing=(voxel,) * 3, origin=origin)
    v, f, _ = drop_non_finite(v, f)
    return v, f


def crossings(tsdf, weight, origin, voxel, min_weight=1.0):
    """the zero crossings on lattice edges between two points of weight >= min_weight (one below 0, one not) -> float64 [n, 3],
    placed by linear interpolation"""
    shape = tsdf.shape
    X = lattice(shape, origin, voxel).astype(np.float64).reshape(*shape, 3)
    T = tsdf.astype(np.float64)
    seen = weight >= F32(min_weight)
    out = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = seen[lo] & seen[hi] & ((T[lo] < 0) != (T[hi] < 0))
        t = (0.0 - T[lo][cross]) / (T[hi][cross] - T[lo][cross])
        out.append(X[lo][cross] + t[:, None] * (X[hi][cross] - X[lo][cross]))
    return np.concatenate(out)
