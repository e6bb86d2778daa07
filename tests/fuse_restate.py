"""THE FUSION RULE of include/ls2fm.h (ls2fm_mvs_fuse_mark, ls2fm_mvs_fuse_emit) restated in plain numpy for this project: float32
arrays over the pixels of one view for the walk, float64 for the sums, the views and their sources in loops, so that every
operation rounds once, in the order the header gives.  Steps 1 to 7 of THE CONSISTENCY RULE are mvs_restate.filter_depths' lines,
the projection is raster_restate's.  Test infrastructure only."""
import math

import numpy as np

import mvs_restate as MR
import raster_restate as R

F32 = np.float32
F64 = np.float64


def cos2_of(max_normal_angle):
    """what ls2fm.mvs.fuse_depths passes: cos^2 of the angle in degrees, formed in float64 and rounded once"""
    return F32(math.cos(math.radians(float(max_normal_angle))) ** 2)


def cam_to_world(poses):
    """float32 [V, 3, 4] = P^-1, formed in float64 in relative_poses' order (the identity composed with P^-1) and rounded once"""
    P = np.asarray(poses, F32).reshape(-1, 3, 4).astype(F64)
    eye = np.broadcast_to(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), P.shape)
    with np.errstate(all="ignore"):
        return MR.compose(eye, P).astype(F32)


def _dot(a, b):
    out = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    assert out.dtype == a[0].dtype
    return out


def fuse(depth, poses, intr, sources, normal=None, colour=None, near=1e-3, max_reproj=1.0, rel_depth=0.01, max_normal_angle=60.0,
         cos2=None, stats=None):
    """-> dict(support uint8 [V, H, W], points float32 [M, 3], normals float32 [M, 3] or None, colours float32 [M, C] or None,
    pixel int64 [M]).  stats: a dict that collects, by name, how often each edge of the rule was met"""
    depth = np.asarray(depth, F32)
    V, H, W = depth.shape
    sources = np.asarray(sources, np.int64).reshape(V, -1)
    if normal is not None:
        normal = np.asarray(normal, F32).reshape(V, H * W, 3)
    if colour is not None:
        colour = np.asarray(colour, F32).reshape(V, H * W, -1)
        assert 1 <= colour.shape[2] <= 4
    k4 = R.intr4(intr, V)
    refs = np.arange(V)
    rel, back = MR.relative_poses(poses, refs, sources), MR.relative_poses(poses, refs, sources, back=True)
    c2w = cam_to_world(poses).astype(F64)
    mr, rd = F32(max_reproj), F32(rel_depth)
    c2 = cos2_of(max_normal_angle) if cos2 is None else F32(cos2)
    reproj2 = mr * mr
    note = (lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(np.count_nonzero(m)))) if stats is not None else None
    uc = np.broadcast_to(np.arange(W).astype(F32)[None, :] + F32(0.5), (H, W)).reshape(-1)
    vc = np.broadcast_to(np.arange(H).astype(F32)[:, None] + F32(0.5), (H, W)).reshape(-1)
    support = np.zeros((V, H * W), np.int64)
    rows = dict(points=[], normals=[], colours=[], pixel=[])

    def world(v, X, Y, d):
        m = c2w[v]
        X, Y, d = X.astype(F64), Y.astype(F64), d.astype(F64)
        return [((m[i, 0] * X + m[i, 1] * Y) + m[i, 2] * d) + m[i, 3] for i in range(3)]

    def unit(v, n):
        m = c2w[v]
        n = [n[:, j].astype(F64) for j in range(3)]
        g = [(m[i, 0] * n[0] + m[i, 1] * n[1]) + m[i, 2] * n[2] for i in range(3)]
        length = np.sqrt(_dot(g, g))
        return [gi / length for gi in g]

    with np.errstate(all="ignore"):
        for r in range(V):
            d = depth[r].reshape(-1)
            has = np.isfinite(d) & (d > 0)
            fx, fy, cx, cy = k4[r]
            X, Y = ((uc - cx) / fx) * d, ((vc - cy) / fy) * d
            dz = rd * d
            count, lower, higher = np.zeros(H * W, np.int64), np.zeros(H * W, bool), np.zeros(H * W, bool)
            point = [np.zeros(H * W, F64) + w for w in world(r, X, Y, d)]
            if normal is not None:
                nr = [normal[r][:, j] for j in range(3)]
                rr = _dot(nr, nr)
                nsum = [np.zeros(H * W, F64) + g for g in unit(r, normal[r])]
                if note:
                    note("the pixel's normal is zero", has & (rr == 0))
                    note("the pixel's normal is NaN", has & np.isnan(rr))
                    note("the pixel's normal is not of unit length", has & np.isfinite(rr) & (rr != 0) & (rr != 1))
            if colour is not None:
                csum = np.zeros((H * W, colour.shape[2]), F64) + colour[r].astype(F64)
            seen = set()
            for s in range(sources.shape[1]):
                sv = int(sources[r, s])
                if not 0 <= sv < V or sv == r:
                    if note:
                        note("source entry equal to the view", sv == r)
                        note("source entry outside [0, V)", sv != r)
                    continue
                if note:
                    note("source listed twice", sv in seen)
                seen.add(sv)
                # steps 1 to 7 of THE CONSISTENCY RULE
                cz, u, v, usable = R.project(np.stack([X, Y, d], axis=1), rel[r, s], k4[sv], near)
                ok = usable & (u >= 0) & (u < F32(W)) & (v >= 0) & (v < F32(H))
                sx, sy = np.where(ok, np.floor(u), 0).astype(np.int64), np.where(ok, np.floor(v), 0).astype(np.int64)
                at = sy * W + sx
                ds = depth[sv].reshape(-1)[at]
                if note:
                    landed = has & ok
                    note("d_s nan", landed & np.isnan(ds))
                    note("d_s zero", landed & (ds == 0))
                    note("d_s negative", landed & (ds < 0))
                    note("d_s inf", landed & np.isinf(ds))
                    note("c_z is NaN", has & np.isnan(cz))
                ok = has & ok & np.isfinite(ds) & (ds > 0)
                sfx, sfy, scx, scy = k4[sv]
                Xs = (((sx.astype(F32) + F32(0.5)) - scx) / sfx) * ds
                Ys = (((sy.astype(F32) + F32(0.5)) - scy) / sfy) * ds
                z2, u2, v2, usable2 = R.project(np.stack([Xs, Ys, ds], axis=1), back[r, s], k4[r], near)
                du, dv = u2 - uc, v2 - vc
                e = du * du + dv * dv
                dd = np.abs(z2 - d)
                assert e.dtype == F32 and dd.dtype == F32 and dz.dtype == F32
                good = ok & usable2 & (e <= reproj2) & (dd <= dz)
                if note:
                    note("reprojection at equality", ok & usable2 & (e == reproj2) & (dd <= dz))
                    note("reprojection beyond", ok & usable2 & (e > reproj2))
                    note("depth at equality", ok & usable2 & (e <= reproj2) & (dd == dz))
                    note("depth beyond", ok & usable2 & (dd > dz))
                # the normal test
                if normal is not None:
                    ns = [normal[sv][at, j] for j in range(3)]
                    B = back[r, s]
                    turned = [(B[i, 0] * ns[0] + B[i, 1] * ns[1]) + B[i, 2] * ns[2] for i in range(3)]
                    a = _dot(nr, turned)
                    ss = _dot(turned, turned)
                    lhs, rhs = a * a, c2 * (rr * ss)
                    assert lhs.dtype == F32 and rhs.dtype == F32
                    agree = (a > 0) & (lhs >= rhs)
                    if note:
                        note("normal angle at equality", good & (a > 0) & (lhs == rhs) & (rhs > 0))
                        note("normal angle beyond", good & (a > 0) & (lhs < rhs))
                        note("a == 0", good & (a == 0))
                        note("a < 0", good & (a < 0))
                        note("a is NaN", good & np.isnan(a))
                        note("the partner's normal is zero", good & (ss == 0))
                    good = good & agree
                # ownership and the sums
                count += good
                lower |= good & (sv < r)
                higher |= good & (sv > r)
                for i, w in enumerate(world(sv, Xs, Ys, ds)):
                    point[i] = np.where(good, point[i] + w, point[i])
                if normal is not None:
                    for i, g in enumerate(unit(sv, normal[sv][at])):
                        nsum[i] = np.where(good, nsum[i] + g, nsum[i])
                if colour is not None:
                    csum = np.where(good[:, None], csum + colour[sv][at].astype(F64), csum)
            owner = has & ~lower
            support[r] = np.where(owner, 1 + count, 0)
            if note:
                note("suppressed: the only consistent partners are lower", has & lower & ~higher)
                note("owner with higher partners only", owner & higher)
                note("suppressed with partners of both kinds", has & lower & higher)
                note("owner without a partner", owner & (count == 0))
                note("no depth", ~has)
                if colour is not None:
                    note("a NaN colour in a row", owner & np.isnan(csum).any(axis=1))
            n = support[r][owner].astype(F64)
            rows["points"].append(np.stack([p[owner] / n for p in point], axis=1).astype(F32))
            if normal is not None:
                t = [g[owner] for g in nsum]
                length = np.sqrt(_dot(t, t))
                rows["normals"].append(np.stack([ti / length for ti in t], axis=1).astype(F32))
                if note:
                    note("a NaN normal in a row", np.isnan(rows["normals"][-1]).any(axis=1))
            if colour is not None:
                rows["colours"].append((csum[owner] / n[:, None]).astype(F32))
            rows["pixel"].append(r * H * W + np.nonzero(owner)[0].astype(np.int64))
    out = dict(support=support.astype(np.uint8).reshape(V, H, W), points=np.concatenate(rows["points"]).reshape(-1, 3),
               normals=None if normal is None else np.concatenate(rows["normals"]).reshape(-1, 3),
               colours=None if colour is None else np.concatenate(rows["colours"]).reshape(-1, colour.shape[2]),
               pixel=np.concatenate(rows["pixel"]) if V else np.zeros(0, np.int64))
    assert out["points"].dtype == F32 and out["pixel"].dtype == np.int64
    return out
