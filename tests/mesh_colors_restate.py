"""THE VERTEX COLOUR RULE of include/ls2fm.h (ls2fm_mesh_vertex_colors, ls2fm_mesh_vertex_colors_finish) restated in plain numpy
for this project: vertex by vertex and view by view, numpy scalars so that every fp32 and every fp64 operation rounds once, in the
order the header gives.  The camera point, projection and usable rule are raster_restate's.  Test infrastructure only."""
import numpy as np

import raster_restate as R

F32, F64 = np.float32, np.float64


def new_state(n_verts, channels):
    return np.zeros((n_verts, channels + 1), F64), np.zeros(n_verts, np.int32)


def accumulate(state, verts, poses, intr, images, depth, masks=None, normals=None, near=1e-3, depth_tol=1e-2, power=1,
               terms=None):
    """extend state = (sums float64 [V, C + 1], count int32 [V]) in place by the views given.  terms: a float64 [V, C + 1] array
    that collects sum |term| per entry (the scale of the rounding bound the torch form is held to), or None."""
    sums, count = state
    verts = np.asarray(verts, F32).reshape(-1, 3)
    poses = np.asarray(poses, F32).reshape(-1, 3, 4)
    images = np.asarray(images, F32)
    N, H, W, C = images.shape
    depth = np.asarray(depth, F32).reshape(N, H, W)
    k4 = R.intr4(intr, N)
    tol = F32(depth_tol)
    nrm = None if normals is None else np.asarray(normals, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for n in range(N):
            P = poses[n]
            cz, u, v, usable = R.project(verts, P, k4[n], near)
            for i in range(len(verts)):
                # 1. usable, in the image, pixel
                if not (usable[i] and u[i] >= F32(0) and u[i] < F32(W) and v[i] >= F32(0) and v[i] < F32(H)):
                    continue
                px, py = int(np.floor(u[i])), int(np.floor(v[i]))
                # 2. mask
                if masks is not None and masks[n, py, px] == 0:
                    continue
                # 3. visible: fp32, the product and the sum each rounded once
                d = depth[n, py, px]
                if not (np.isfinite(d) and cz[i] <= F32(d + F32(tol * d))):
                    continue
                # 4. weight
                w = F64(1.0)
                if nrm is not None:
                    X = verts[i]
                    c = [F64(F32(F32(F32(F32(P[r, 0] * X[0]) + F32(P[r, 1] * X[1])) + F32(P[r, 2] * X[2])) + P[r, 3])) for r in range(3)]
                    m = [(F64(P[r, 0]) * F64(nrm[i, 0]) + F64(P[r, 1]) * F64(nrm[i, 1])) + F64(P[r, 2]) * F64(nrm[i, 2]) for r in range(3)]
                    dot = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]
                    mm = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                    cc = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
                    cos = (-dot) / (mm * cc)
                    if not (cos > 0 and np.isfinite(cos)):
                        continue
                    for _ in range(int(power)):
                        w = w * cos
                # 5. sample
                x, y = F64(u[i]) - F64(0.5), F64(v[i]) - F64(0.5)
                x0f, y0f = np.floor(x), np.floor(y)
                fx, fy = x - x0f, y - y0f
                x0, x1 = min(max(int(x0f), 0), W - 1), min(max(int(x0f) + 1, 0), W - 1)
                y0, y1 = min(max(int(y0f), 0), H - 1), min(max(int(y0f) + 1, 0), H - 1)
                for ch in range(C):
                    a00, a10 = F64(images[n, y0, x0, ch]), F64(images[n, y0, x1, ch])
                    a01, a11 = F64(images[n, y1, x0, ch]), F64(images[n, y1, x1, ch])
                    r0 = a00 + fx * (a10 - a00)
                    r1 = a01 + fx * (a11 - a01)
                    s = r0 + fy * (r1 - r0)
                    # 6. accumulate
                    sums[i, ch] = sums[i, ch] + w * s
                    if terms is not None:
                        terms[i, ch] += abs(w * s)
                sums[i, C] = sums[i, C] + w
                if terms is not None:
                    terms[i, C] += abs(w)
                count[i] += 1
    return state


def finish(state, fill=(0.5, 0.5, 0.5), fallback=None):
    """color float32 [V, C]"""
    sums, count = state
    C = sums.shape[1] - 1
    vals = [float(fill)] * C if np.isscalar(fill) else [float(t) for t in fill]
    vals = (vals + [1.0] * C)[:C]
    out = np.empty((len(count), C), F32)
    with np.errstate(all="ignore"):
        for i in range(len(count)):
            for ch in range(C):
                if count[i] > 0:
                    out[i, ch] = F32(sums[i, ch] / sums[i, C])
                else:
                    out[i, ch] = F32(fallback[i][ch]) if fallback is not None else F32(vals[ch])
    return out


def vertex_colors(verts, poses, intr, images, depth, masks=None, normals=None, near=1e-3, depth_tol=1e-2, power=1,
                  fill=(0.5, 0.5, 0.5), fallback=None, return_terms=False):
    """-> dict(colors float32 [V, C], sums float64 [V, C + 1], count int32 [V]) (and terms, with return_terms)"""
    images = np.asarray(images, F32)
    n_v = len(np.asarray(verts).reshape(-1, 3))
    state = new_state(n_v, images.shape[3])
    terms = np.zeros_like(state[0]) if return_terms else None
    accumulate(state, verts, poses, intr, images, depth, masks, normals, near, depth_tol, power, terms)
    out = dict(colors=finish(state, fill, fallback), sums=state[0], count=state[1])
    if return_terms:
        out["terms"] = terms
    return out


def vertex_normals(verts, faces):
    """area-weighted vertex normals in float64 -> float32 [V, 3] (test scenes only: any normals serve the rule)"""
    v = np.asarray(verts, F64)
    f = np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], fn)
    return out.astype(F32)
