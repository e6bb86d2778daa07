"""The rasterisation rule of include/ls2fm.h (ls2fm_rasterize, ls2fm_mesh_mask_votes) and clean_mesh's selection, restated in
numpy for this project: float32 arrays so that every fp32 operation rounds once, int64 coverage, float64 depth, and the minimum of
the 64-bit key.  Faces are visited one at a time in index order; the rule makes the order irrelevant.  Test infrastructure only."""
import numpy as np

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS = np.uint32(0x7F800000)


def intr4(intr, n):
    """(fx, fy, cx, cy) float32 [n, 4] of K [3, 3] or [n, 3, 3]"""
    K = np.asarray(intr, F32).reshape(-1, 3, 3)
    K = np.broadcast_to(K, (n, 3, 3))
    return np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1).astype(F32)


def project(verts, pose, k4, near):
    """camera z, u, v (float32 [n]) and usable (bool [n]) of every vertex in one view"""
    X = np.asarray(verts, F32)
    P = np.asarray(pose, F32).reshape(3, 4)
    fx, fy, cx, cy = (F32(t) for t in k4)
    with np.errstate(all="ignore"):
        c = [((P[r, 0] * X[:, 0] + P[r, 1] * X[:, 1]) + P[r, 2] * X[:, 2]) + P[r, 3] for r in range(3)]
        assert all(t.dtype == F32 for t in c)
        u = fx * (c[0] / c[2]) + cx
        v = fy * (c[1] / c[2]) + cy
        usable = np.isfinite(c[2]) & (c[2] >= F32(near)) & (np.abs(u) <= F32(65536)) & (np.abs(v) <= F32(65536))
    assert u.dtype == F32 and v.dtype == F32
    return c[2], u, v, usable


def snap(u, usable):
    with np.errstate(all="ignore"):
        s = np.rint(u * F32(256))
    return np.where(usable, s, 0).astype(np.int64)


def setup(verts, faces, pose, k4, near):
    """per face of one view: drawn bool [F], snapped corners int64 [F, 3, 2], A int64 [F], reciprocal depths float64 [F, 3]"""
    verts, faces = np.asarray(verts, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    z, u, v, usable = project(verts, pose, k4, near)
    n = len(verts)
    in_range = ((faces >= 0) & (faces < n)).all(axis=1)
    idx = np.where(in_range[:, None], faces, 0) if n else np.zeros_like(faces)
    if n == 0:
        F = len(faces)
        return np.zeros(F, bool), np.zeros((F, 3, 2), np.int64), np.zeros(F, np.int64), np.ones((F, 3))
    ok = in_range & usable[idx].all(axis=1)
    UV = np.stack([snap(u, usable)[idx], snap(v, usable)[idx]], axis=-1)            # [F, 3, 2]
    A = (UV[:, 1, 0] - UV[:, 0, 0]) * (UV[:, 2, 1] - UV[:, 0, 1]) - (UV[:, 1, 1] - UV[:, 0, 1]) * (UV[:, 2, 0] - UV[:, 0, 0])
    drawn = ok & (A != 0)
    with np.errstate(all="ignore"):
        r = np.float64(1.0) / z.astype(np.float64)[idx]
    return drawn, UV, A, r


def box(UV, H, W):
    """the clipped box (x0, x1, y0, y1) of the pixels whose centres lie inside the corners' bounds; empty when x0 > x1 or y0 > y1"""
    umin, umax, vmin, vmax = UV[:, 0].min(), UV[:, 0].max(), UV[:, 1].min(), UV[:, 1].max()
    return (max(int(-((128 - umin) // 256)), 0), min(int((umax - 128) // 256), W - 1),
            max(int(-((128 - vmin) // 256)), 0), min(int((vmax - 128) // 256), H - 1))


def weights(UV, A, px, py):
    """w int64 [3, ...] and the coverage mask of the pixels (px, py) (int arrays that broadcast against each other) for one face"""
    s = 1 if A > 0 else -1
    X = 256 * np.asarray(px, np.int64) + 128
    Y = 256 * np.asarray(py, np.int64) + 128
    w, cov = [], True
    for p, q in ((1, 2), (2, 0), (0, 1)):                                # w_a = s E_bc, w_b = s E_ca, w_c = s E_ab
        dx, dy = s * (UV[q, 0] - UV[p, 0]), s * (UV[q, 1] - UV[p, 1])
        e = dx * (Y - UV[p, 1]) - dy * (X - UV[p, 0])
        owns = dy > 0 or (dy == 0 and dx > 0)
        cov = cov & ((e > 0) | ((e == 0) & owns))
        w.append(e)
    return np.stack(w), cov


def depth_terms(w, r):
    """num float64 and the three products w_i r_i, every operation rounded once"""
    t = [w[i].astype(np.float64) * r[i] for i in range(3)]
    return (t[0] + t[1]) + t[2], t


def rasterize(verts, faces, poses, intr, H, W, near=1e-3, return_counts=False):
    """-> dict(face_id int32 [N, H, W], depth float32 [N, H, W], bary float32 [N, H, W, 3], face_hits int32 [F]); with
    return_counts also counts int32 [N, H, W] (how many faces cover each pixel), ties bool [N, H, W] (a second covering face
    had the winner's depth bits), on_edge bool [N, H, W] (some covering face had a zero weight there: a pixel centre on an edge),
    drawn bool [N, F] and box_pixels int64 [N, F] (the clipped box size of every drawn face, 0 otherwise)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    poses = np.asarray(poses, F32).reshape(-1, 3, 4)
    N, F = len(poses), len(faces)
    k4 = intr4(intr, N)
    keys = np.full((N, H, W), EMPTY, np.uint64)
    counts = np.zeros((N, H, W), np.int32)
    ties = np.zeros((N, H, W), bool)
    on_edge = np.zeros((N, H, W), bool)
    drawn_all = np.zeros((N, F), bool)
    box_pixels = np.zeros((N, F), np.int64)
    bary = np.zeros((N, H, W, 3), F32)
    setups = []
    for n in range(N):
        drawn, UV, A, r = setup(verts, faces, poses[n], k4[n], near)
        setups.append((drawn, UV, A, r))
        drawn_all[n] = drawn
        for f in np.nonzero(drawn)[0]:
            x0, x1, y0, y1 = box(UV[f], H, W)
            if x0 > x1 or y0 > y1:
                continue
            box_pixels[n, f] = (x1 - x0 + 1) * (y1 - y0 + 1)
            w, cov = weights(UV[f], A[f], np.arange(x0, x1 + 1)[None, :], np.arange(y0, y1 + 1)[:, None])
            if not cov.any():
                continue
            num, _ = depth_terms(w, r[f])
            with np.errstate(all="ignore"):
                z = (np.float64(abs(int(A[f]))) / num).astype(F32)
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            key = np.where(cov, key, EMPTY)
            tile = keys[n, y0:y1 + 1, x0:x1 + 1]
            if return_counts:
                counts[n, y0:y1 + 1, x0:x1 + 1] += cov
                on_edge[n, y0:y1 + 1, x0:x1 + 1] |= cov & (w == 0).any(axis=0)
                same = cov & (tile != EMPTY) & ((tile >> np.uint64(32)) == (key >> np.uint64(32)))
                lower = cov & ((key >> np.uint64(32)) < (tile >> np.uint64(32)))
                t = ties[n, y0:y1 + 1, x0:x1 + 1]
                t[lower] = False
                t |= same
            np.minimum(tile, key, out=tile)
    hit = keys != EMPTY
    face_id = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32), INF_BITS).astype(np.uint32).view(F32)
    for n in range(N):
        drawn, UV, A, r = setups[n]
        for f in np.unique(face_id[n][hit[n]]):
            ys, xs = np.nonzero(face_id[n] == f)
            w, _ = weights(UV[f], A[f], xs, ys)                                  # [3, k]
            num, t = depth_terms(w, r[f])
            bary[n, ys, xs] = np.stack([(t[i] / num).astype(F32) for i in range(3)], axis=1)
    out = dict(face_id=face_id, depth=depth, bary=bary,
               face_hits=np.bincount(face_id[hit].astype(np.int64), minlength=F).astype(np.int32))
    if return_counts:
        out.update(counts=counts, ties=ties & hit, on_edge=on_edge, drawn=drawn_all, box_pixels=box_pixels)
    return out


def mask_votes(verts, poses, intr, masks, near=1e-3):
    """(seen, inside) int32 [n]"""
    verts = np.asarray(verts, F32)
    poses = np.asarray(poses, F32).reshape(-1, 3, 4)
    masks = np.asarray(masks)
    N, H, W = masks.shape
    k4 = intr4(intr, N)
    seen, inside = np.zeros(len(verts), np.int32), np.zeros(len(verts), np.int32)
    for n in range(N):
        _, u, v, usable = project(verts, poses[n], k4[n], near)
        with np.errstate(all="ignore"):
            ok = usable & (u >= F32(0)) & (u < F32(W)) & (v >= F32(0)) & (v < F32(H))
            px = np.where(ok, np.floor(u), 0).astype(np.int64)
            py = np.where(ok, np.floor(v), 0).astype(np.int64)
        seen += ok
        inside += ok & (masks[n, py, px] != 0)
    return seen, inside


def dilate(masks, d):
    """binary dilation by a (2 d + 1)-square, zero outside the image: what max_pool2d(kernel 2 d + 1, stride 1, padding d) gives"""
    m = np.asarray(masks) != 0
    if d <= 0:
        return m
    N, H, W = m.shape
    pad = np.zeros((N, H + 2 * d, W + 2 * d), bool)
    pad[:, d:d + H, d:d + W] = m
    out = np.zeros_like(m)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            out |= pad[:, dy:dy + H, dx:dx + W]
    return out


def clean_mesh(verts, faces, poses, intr, masks=None, H=None, W=None, dilate_px=0, max_outside=0, min_seen=1, visibility=True,
               min_pixels=1, near=1e-3):
    """-> (kept_faces bool [F], new verts float32, new faces int32): the selection before any largest-component step"""
    verts, faces = np.asarray(verts, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    keep_v = np.ones(len(verts), bool)
    if masks is not None:
        m = dilate(masks, dilate_px)
        H = m.shape[1] if H is None else H
        W = m.shape[2] if W is None else W
        seen, inside = mask_votes(verts, poses, intr, m, near)
        keep_v = (seen >= min_seen) & (seen - inside <= max_outside)
    keep_f = keep_v[faces].all(axis=1)
    if visibility:
        keep_f &= rasterize(verts, faces, poses, intr, H, W, near)["face_hits"] >= min_pixels
    kept = faces[keep_f]
    used = np.zeros(len(verts), bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    return keep_f, verts[used], renumber[kept].astype(np.int32)
