"""THE CLUSTERING RULE of include/ls2fm.h (ls2fm.simplify, csrc/mesh_simplify.hip) restated in numpy, step for step in fp64: the judge
of the GPU tests (tests/test_hip_simplify.py), itself judged by the rule's properties in tests/test_simplify_host.py.  Every sum
follows the stated order: lane l of a 64-lane wave adds a segment's entries l, l + 64, ... in order, then the xor butterfly
32 ... 1 adds the lanes."""
import numpy as np

F32, F64 = np.float32, np.float64
KEY_BITS = 21
BIAS = 1 << (KEY_BITS - 1)
INVALID_KEY = np.int64(-1)
N_SUMS = 13
FACE_INVALID, FACE_COLLAPSED, FACE_SURVIVES = 0, 1, 2


def vertex_keys(verts, cell):
    """-> (key int64 [V], valid bool [V], bad bool [V]); an invalid or bad vertex has INVALID_KEY"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    finite = np.isfinite(v).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.floor(v.astype(F64) / F64(F32(cell)))
        fits = ((k >= -BIAS) & (k < BIAS)).all(axis=1)
    valid = finite & fits
    kb = np.where(valid[:, None], k, 0.0).astype(np.int64) + BIAS
    key = np.where(valid, (kb[:, 0] << (2 * KEY_BITS)) | (kb[:, 1] << KEY_BITS) | kb[:, 2], INVALID_KEY)
    return key, valid, finite & ~fits


def cell_centres(key, cell):
    k = np.stack([(key >> (2 * KEY_BITS)) & (2 * BIAS - 1), (key >> KEY_BITS) & (2 * BIAS - 1), key & (2 * BIAS - 1)], axis=1) - BIAS
    return (k.astype(F64) + 0.5) * F64(F32(cell))


def face_classes(key, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fk = key[f]
    valid = (fk != INVALID_KEY).all(axis=1)
    distinct = (fk[:, 0] != fk[:, 1]) & (fk[:, 1] != fk[:, 2]) & (fk[:, 0] != fk[:, 2])
    return np.where(valid, np.where(distinct, FACE_SURVIVES, FACE_COLLAPSED), FACE_INVALID).astype(np.uint8)


def wave_sums(segment, terms, n_segments):
    """terms [n, Q] whose rows belong to segments `segment` [n] (ascending; the rows of one segment in their order) -> [n_segments, Q]
    in the stated order: 64 running sums from +0, then s_l <- s_l + s_(l xor o) for o = 32 ... 1, lane 0's result"""
    terms = np.asarray(terms, F64)
    if n_segments > 4096:                                                # 4096 segments at a time: the lanes' sums are [., 64, Q]
        cuts = np.searchsorted(segment, np.arange(0, n_segments + 4096, 4096))
        return np.concatenate([wave_sums(segment[lo:hi] - s, terms[lo:hi], min(4096, n_segments - s))
                               for s, lo, hi in zip(range(0, n_segments, 4096), cuts[:-1], cuts[1:])])
    start = np.searchsorted(segment, np.arange(n_segments))
    at = np.arange(len(segment)) - start[segment]
    lane, row = at % 64, at // 64
    acc = np.zeros((n_segments, 64, terms.shape[1]), F64)
    with np.errstate(all="ignore"):
        for r in range(int(row.max()) + 1 if len(row) else 0):
            sel = row == r
            acc[segment[sel], lane[sel]] = acc[segment[sel], lane[sel]] + terms[sel]
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def chol_solve3(A, g, lam):
    """csrc/lm_math.h chol_solve at size 3, operation for operation: (A + lam I) x = -g; A [n, 6], g [n, 3], lam [n] -> (x, ok)"""
    with np.errstate(all="ignore"):
        L00, L10, L20 = A[:, 0] + lam * 1.0, A[:, 1] + 0.0, A[:, 2] + 0.0
        L11, L21, L22 = A[:, 3] + lam * 1.0, A[:, 4] + 0.0, A[:, 5] + lam * 1.0
        ok = L00 > 0
        l00 = np.sqrt(np.where(L00 > 0, L00, 1.0))
        L10, L20 = L10 / l00, L20 / l00
        d = L11 - L10 * L10
        ok = ok & (d > 0)
        l11 = np.sqrt(np.where(d > 0, d, 1.0))
        L21 = (L21 - L20 * L10) / l11
        d = (L22 - L20 * L20) - L21 * L21
        ok = ok & (d > 0)
        l22 = np.sqrt(np.where(d > 0, d, 1.0))
        z0 = -g[:, 0] / l00
        z1 = (-g[:, 1] - L10 * z0) / l11
        z2 = ((-g[:, 2] - L20 * z0) - L21 * z1) / l22
        x2 = z2 / l22
        x1 = (z1 - L21 * x2) / l11
        x0 = ((z0 - L10 * x1) - L20 * x2) / l00
    x = np.stack([x0, x1, x2], axis=1)
    return x, ok & np.isfinite(x).all(axis=1)


def rotate_smallest_first(tri):
    lead = np.argmin(tri, axis=1)
    return np.take_along_axis(tri, (lead[:, None] + np.arange(3)[None, :]) % 3, axis=1)


def simplify(verts, faces, cell, colors=None, placement="quadric", reg=2.0 ** -2):
    """-> a dict: the rule's every intermediate and the output (vertices, faces, vertex_map, colors)"""
    v32 = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cell64 = F64(F32(cell))
    n_ch = 0 if colors is None else np.asarray(colors).shape[1]
    vd = v32.astype(F64)
    key, valid, bad = vertex_keys(v32, cell)
    cls = face_classes(key, f)
    surviving = cls == FACE_SURVIVES
    out_key = np.unique(key[f[surviving]].reshape(-1))                   # ascending
    n_out = len(out_key)
    at = np.searchsorted(out_key, key)
    at_c = np.minimum(at, max(n_out - 1, 0))
    in_out = valid & (out_key[at_c] == key) if n_out else np.zeros(len(key), bool)
    vertex_map = np.where(in_out, at_c, -1).astype(np.int32)
    centre = cell_centres(out_key, cell)
    # 4. vertices of the output cells, ascending index inside a cell
    vi = np.nonzero(in_out)[0]
    vi = vi[np.argsort(vertex_map[vi], kind="stable")]
    seg_v = vertex_map[vi].astype(np.int64)
    terms_v = [vd[vi] - centre[seg_v]] + ([] if colors is None else [np.asarray(colors, F32).astype(F64)[vi]])
    terms_v = np.concatenate(terms_v, axis=1) if len(vi) else np.zeros((0, 3 + n_ch))
    count = np.bincount(seg_v, minlength=n_out).astype(np.int32)
    # 3. contributing corners of the output cells, ascending 3 f + k inside a cell
    fk = key[f]
    contributes = np.stack([cls != FACE_INVALID, (cls != FACE_INVALID) & (fk[:, 1] != fk[:, 0]),
                            (cls != FACE_INVALID) & (fk[:, 2] != fk[:, 0]) & (fk[:, 2] != fk[:, 1])], axis=1).reshape(-1)
    corner_cell = vertex_map[f].reshape(-1).astype(np.int64)
    ci = np.nonzero(contributes & (corner_cell >= 0))[0]
    ci = ci[np.argsort(corner_cell[ci], kind="stable")]
    seg_c = corner_cell[ci]
    fc = f[ci // 3]
    g = centre[seg_c] if len(ci) else np.zeros((0, 3))
    with np.errstate(all="ignore"):
        pa, pb, pc = vd[fc[:, 0]] - g, vd[fc[:, 1]] - g, vd[fc[:, 2]] - g
        u, w = pb - pa, pc - pa
        n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        d = (n0 * pa[:, 0] + n1 * pa[:, 1]) + n2 * pa[:, 2]
        terms_c = np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, d * n0, d * n1, d * n2, d * d], axis=1)
    # 5. the sums in the stated order
    sums = np.concatenate([wave_sums(seg_c, terms_c, n_out), wave_sums(seg_v, terms_v, n_out)], axis=1)
    # numpy's own order, and the sum of magnitudes, per sum: what the summation bound is taken against
    def own(seg, terms, fn):
        out = np.zeros((n_out, terms.shape[1]))
        for c in range(n_out if len(seg) else 0):
            lo, hi = np.searchsorted(seg, [c, c + 1])
            out[c] = fn(terms[lo:hi]).sum(axis=0)
        return out
    with np.errstate(all="ignore"):
        own_sums = np.concatenate([own(seg_c, terms_c, lambda t: t), own(seg_v, terms_v, lambda t: t)], axis=1)
        abs_sums = np.concatenate([own(seg_c, terms_c, np.abs), own(seg_v, terms_v, np.abs)], axis=1)
    n_terms = np.concatenate([np.repeat(np.bincount(seg_c, minlength=n_out)[:, None], 10, axis=1),
                              np.repeat(count.astype(np.int64)[:, None], 3 + n_ch, axis=1)], axis=1)
    # 6. placement
    with np.errstate(all="ignore"):
        m = count.astype(F64)
        mean = sums[:, 10:13] / m[:, None]
        x, solved = mean, np.zeros(n_out, bool)
        if placement == "quadric":
            t = (sums[:, 0] + sums[:, 3]) + sums[:, 5]
            lam = F64(reg) * t
            y, ok = chol_solve3(sums[:, :6], -(sums[:, 6:9] + lam[:, None] * mean), lam)
            solved = ok & (t != 0) & np.isfinite(t) & (np.abs(y) <= cell64 / 2.0).all(axis=1)
            x = np.where(solved[:, None], y, mean)
        elif placement != "mean":
            raise ValueError(placement)
        vertices = (centre + x).astype(F32)
        out_colors = None if colors is None else (sums[:, N_SUMS:] / m[:, None]).astype(F32)
    # 7. faces
    tri = vertex_map[f[surviving]].astype(np.int64)
    if len(tri):
        _, first = np.unique(rotate_smallest_first(tri), axis=0, return_index=True)
        out_faces = tri[np.sort(first)].astype(np.int32)
    else:
        out_faces = np.zeros((0, 3), np.int32)
    return dict(key=key, valid=valid, n_bad=int(bad.sum()), face_class=cls, n_surviving=int(surviving.sum()), out_key=out_key,
                centre=centre, sums=sums, count=count, own_sums=own_sums, abs_sums=abs_sums, n_terms=n_terms, x=x, solved=solved,
                vertices=vertices, colors=out_colors, faces=out_faces, vertex_map=vertex_map)
