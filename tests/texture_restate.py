"""THE ATLAS RULE and THE TEXTURE RENDER RULE of include/ls2fm.h (ls2fm_texture_texels, ls2fm_texture_render, ls2fm.texture.build_atlas)
restated in numpy for this project: float32 arrays so that every fp32 operation rounds once, float64 where the rule says fp64, in the
order the header gives.  The colour of a texel is mesh_colors_restate's rule at the texel's point.  Test infrastructure only."""
import numpy as np

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ the atlas
def class_range(gutter, max_pitch=256):
    """the admissible classes k, ascending: 2^k >= 2 gutter + 4 and 2^k <= max_pitch"""
    k = 0
    while (1 << k) < 2 * gutter + 4:
        k += 1
    return list(range(k, int(max_pitch).bit_length()))


def thresholds(texel, gutter, ks):
    """((2^k - 2 gutter - 3) texel)^2 in Python floats: the largest squared leg class k holds"""
    out = []
    for k in ks:
        t = ((1 << k) - 2 * gutter - 3) * float(texel)
        out.append(t * t)
    return out


def corners(verts, faces):
    """float32 [F, 3, 3]: the corners of every face, NaN for a face with an index outside [0, V); and which faces those are not"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((faces >= 0) & (faces < len(verts))).all(axis=1)
    P = np.full((len(faces), 3, 3), np.nan, F32)
    if len(verts):
        P[in_range] = verts[faces[in_range]]
    return P, in_range


def classify(verts, faces, texel, gutter=1, max_pitch=256):
    """-> rot int32 [F] (the vertex opposite the longest edge, ties to the lowest index), cls int32 [F]"""
    P, _ = corners(verts, faces)
    ks = class_range(gutter, max_pitch)

    def edge(a, b):                                  # fp32 difference, fp64 squared length
        d = (P[:, b] - P[:, a]).astype(F64)
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(all="ignore"):
        e = [edge(1, 2), edge(2, 0), edge(0, 1)]     # e[i] lies opposite vertex i
        rot = np.zeros(len(P), np.int32)
        best = e[0].copy()
        up = e[1] > best
        rot[up], best[up] = 1, e[1][up]
        up = e[2] > best
        rot[up] = 2
        legs = [np.maximum(e[1], e[2]), np.maximum(e[2], e[0]), np.maximum(e[0], e[1])]
        l2 = np.choose(rot, legs)
        cls = np.full(len(P), ks[-1], np.int32)
        for k, thr in reversed(list(zip(ks, thresholds(texel, gutter, ks)))):
            cls[l2 <= F64(thr)] = k
    cls[~np.isfinite(P).all(axis=(1, 2))] = ks[0]
    return rot, cls


def pack(cls, gutter=1, max_pitch=256):
    """-> order int32 [F] (order[slot] = face: stable by class, descending), table [(k, count)] over every admissible k, descending"""
    cls = np.asarray(cls, np.int64)
    order = np.argsort(-cls, kind="stable").astype(np.int32)
    table = [(k, int((cls == k).sum())) for k in reversed(class_range(gutter, max_pitch))]
    return order, table


def layout(table):
    """per class of the table: Morton offset of its first cell, its cells, its first slot; and the total area in texels"""
    starts, cells, slots = [], [], []
    at, slot = 0, 0
    for k, count in table:
        starts.append(at)
        cells.append((count + 1) // 2)
        slots.append(slot)
        at += cells[-1] << (2 * k)
        slot += count
    return starts, cells, slots, at


def smallest_size(table):
    S = 4
    while S * S < layout(table)[3]:
        S *= 2
    return S


def interleave(x, y):
    """Morton code: bit b of x at bit 2 b, bit b of y at bit 2 b + 1"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    m = np.zeros(np.broadcast(x, y).shape, np.int64)
    for b in range(16):
        m |= ((x >> b) & 1) << (2 * b)
        m |= ((y >> b) & 1) << (2 * b + 1)
    return m


def deinterleave(m):
    m = np.asarray(m, np.int64)
    x, y = np.zeros(m.shape, np.int64), np.zeros(m.shape, np.int64)
    for b in range(16):
        x |= ((m >> (2 * b)) & 1) << b
        y |= ((m >> (2 * b + 1)) & 1) << b
    return x, y


def owners(table, gutter, S, rows=None):
    """per texel of the rows [r0, r1): slot int64 (-1: unowned), chart-local (i', j') and the class k"""
    r0, r1 = (0, S) if rows is None else rows
    y, x = np.mgrid[r0:r1, 0:S].astype(np.int64)
    m = interleave(x, y)
    starts, cells, slots, _ = layout(table)
    c = np.full(m.shape, -1, np.int64)
    for i, s in enumerate(starts):
        c[m >= s] = i
    tab = lambda v: np.asarray(v, np.int64)[c]
    k = tab([t[0] for t in table])
    p = np.int64(1) << k
    cell = (m - tab(starts)) >> (2 * k)
    i, j = x & (p - 1), y & (p - 1)
    B = i + j > p - 1
    slot = tab(slots) + 2 * cell + B
    owned = (cell < tab(cells)) & (slot < tab(slots) + tab([t[1] for t in table]))
    return np.where(owned, slot, -1), np.where(B, p - 1 - i, i), np.where(B, p - 1 - j, j), k, x, y


def texels(verts, faces, order, rot, table, gutter, S, rows=None, uv=None):
    """-> dict(face int32 [rows, S], point float32 [rows, S, 3], normal float32 [rows, S, 3], uv float32 [F, 3, 2]: the entries the
    corner texels of these rows hold are written into `uv` (NaN-filled when not given)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_f = len(faces)
    uv = np.full((n_f, 3, 2), np.nan, F32) if uv is None else uv
    slot, ii, jj, k, x, y = owners(table, gutter, S, rows)
    owned = slot >= 0
    face = np.full(slot.shape, -1, np.int32)
    point = np.full(slot.shape + (3,), np.nan, F32)
    normal = np.full(slot.shape + (3,), np.nan, F32)
    if not owned.any():
        return dict(face=face, point=point, normal=normal, uv=uv)
    f = np.asarray(order, np.int64)[slot[owned]]
    face[owned] = f
    P, _ = corners(verts, faces)
    r = np.asarray(rot, np.int64)[f]
    a, b, c = P[f, r], P[f, (r + 1) % 3], P[f, (r + 2) % 3]
    g = np.int64(gutter)
    L = ((np.int64(1) << k[owned]) - 2 * g - 3).astype(F32)
    with np.errstate(all="ignore"):
        s = ((ii[owned] - g).astype(F32) / L)[:, None]
        t = ((jj[owned] - g).astype(F32) / L)[:, None]
        d1, d2 = b - a, c - a
        X = (a + s * d1) + t * d2
        n = np.stack([d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1], d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2],
                      d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]], axis=1)
    assert X.dtype == F32 and n.dtype == F32
    point[owned], normal[owned] = X, n
    Li = (np.int64(1) << k[owned]) - 2 * g - 3
    io, jo, xo, yo = ii[owned], jj[owned], x[owned], y[owned]
    for q, (ci, cj) in enumerate(((g, g), (g + Li, g), (g, g + Li))):
        at = (io == ci) & (jo == cj)
        uv[f[at], (r[at] + q) % 3] = np.stack([xo[at].astype(F32) + F32(0.5), yo[at].astype(F32) + F32(0.5)], axis=1)
    return dict(face=face, point=point, normal=normal, uv=uv)


def chart_corners(order, rot, table, gutter):
    """uv float32 [F, 3, 2] from the packing alone: the cell's origin by de-interleaving its Morton offset"""
    n_f = len(order)
    uv = np.zeros((n_f, 3, 2), F32)
    starts, cells, slots, _ = layout(table)
    for (k, count), start, slot0 in zip(table, starts, slots):
        p, L = 1 << k, (1 << k) - 2 * gutter - 3
        for s in range(count):
            f = int(order[slot0 + s])
            x0, y0 = (int(v) for v in deinterleave((start + ((s // 2) << (2 * k)))))
            for q, (ci, cj) in enumerate(((gutter, gutter), (gutter + L, gutter), (gutter, gutter + L))):
                if s % 2:
                    ci, cj = p - 1 - ci, p - 1 - cj
                uv[f, (int(rot[f]) + q) % 3] = (x0 + ci + 0.5, y0 + cj + 0.5)
    return uv


# ------------------------------------------------------------------------------------------------------------------ the render
def sample(texture, x, y):
    """bilinear about the texel centres at the float32 points (x, y), taps clamped to the texture: float32 [..., C]"""
    tex = np.asarray(texture, F32)
    S = tex.shape[0]
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    with np.errstate(all="ignore"):
        def axis(u):
            s = u - F32(0.5)
            u0 = np.floor(s)
            t = s - u0
            u0 = np.where(np.isnan(u0), F32(-1), np.minimum(np.maximum(u0, F32(-1)), F32(S))).astype(np.int64)
            return np.clip(u0, 0, S - 1), np.clip(u0 + 1, 0, S - 1), t[..., None]
        x0, x1, tx = axis(x)
        y0, y1, ty = axis(y)
        b00, b10, b01, b11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
        r0 = b00 + tx * (b10 - b00)
        r1 = b01 + tx * (b11 - b01)
        out = r0 + ty * (r1 - r0)
    assert out.dtype == F32
    return out


def texture_point(bary, uv3):
    """x, y float32 of the barycentrics [..., 3] over the corners uv3 [..., 3, 2]: ((w0 x0 + w1 x1) + w2 x2)"""
    w, c = np.asarray(bary, F32), np.asarray(uv3, F32)
    with np.errstate(all="ignore"):
        xy = (w[..., 0, None] * c[..., 0, :] + w[..., 1, None] * c[..., 1, :]) + w[..., 2, None] * c[..., 2, :]
    assert xy.dtype == F32
    return xy[..., 0], xy[..., 1]


def render(face_id, bary, uv, texture, background):
    """-> float32 [V, H, W, C]"""
    face_id = np.asarray(face_id, np.int64)
    tex = np.asarray(texture, F32)
    C = tex.shape[2]
    out = np.empty(face_id.shape + (C,), F32)
    out[...] = np.asarray(background, F32)[:C]
    ok = (face_id >= 0) & (face_id < len(uv))
    if ok.any():
        x, y = texture_point(np.asarray(bary, F32)[ok], np.asarray(uv, F32)[face_id[ok]])
        out[ok] = sample(tex, x, y)
    return out
