"""SIFT descriptor matching on the device and the driver's `n_views.npy` tables: the part of the reference's
preparation/main.py between "images with features" and LevelS2fM.load_matches.

`match_descriptors` is `colmap exhaustive_matcher` (main.py:98, whose raw matches :30-37 read back): COLMAP's CPU SIFT matcher
with its defaults (ratio test 0.8, distance 0.7, cross check) for ALL image pairs in one call of ls2fm_match_descriptors
(csrc/match.hip: exact integer products on the i8 matrix cores, the top-2 reduction as their epilogue).  `assemble_n_views`
writes the per-view layout of main.py:177-247; `two_view_tables` chains the matcher, the < 50 filter (:193-194), ONE
ls2fm.pose.relative_pose call (without an intrinsic matrix: ONE ls2fm.pose.fundamental_matrix call) over the surviving pairs for
the inlier masks (:209-213) and the assembly.  Every rule is stated in
include/ls2fm.h; tests/match_restate.py repeats the matcher in numpy.

There is no CPU path for the matcher: a missing device or library raises.  `assemble_n_views` is plain numpy.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

MAX_DESCRIPTORS = 32768      # LS2FM_MATCH_MAX_DESCRIPTORS


def exhaustive_pairs(n_views):
    """all (a, b) with a < b in main.py's order (:177-182): a rising, b rising inside a -> int32 [n (n - 1) / 2, 2]"""
    return np.array([(a, b) for a in range(n_views) for b in range(a + 1, n_views)], dtype=np.int32).reshape(-1, 2)


def _descriptor_array(descriptors, dev):
    """list of uint8 [n_v,128] (torch or numpy, any device) -> ([N,128] uint8 on dev, image_start int32 numpy [V+1])"""
    parts = []
    for d in descriptors:
        t = torch.as_tensor(d)
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 128:
            if not (t.dtype == torch.uint8 and t.numel() == 0):
                raise ValueError(f"ls2fm.match: descriptors must be uint8 [n,128], got {t.dtype} {tuple(t.shape)}")
            t = t.reshape(0, 128)
        parts.append(t)
    counts = [int(t.shape[0]) for t in parts]
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    if len({t.device for t in parts}) == 1:
        flat = torch.cat(parts).to(dev)                 # moved once
    else:
        flat = torch.cat([t.to(dev) for t in parts])
    return flat.contiguous(), start


def match_descriptors(descriptors, pairs=None, max_ratio=0.8, max_distance=0.7, cross_check=True, return_scores=False):
    """COLMAP's SIFT matcher over P image pairs in one device call.  descriptors: list of uint8 [n_v,128] (device, CPU or
    numpy; moved once); pairs [P,2] image indices (first, second) or None for every a < b in main.py's order.
    -> list of int64 [M_p,2] tensors (row of the first image, row of the second; increasing first), on the device.
    return_scores=True: (matches, scores) with scores a list of dicts best_ab / best_j_ab / second_ab [n_a] and best_ba /
    best_j_ba / second_ba [n_b] (int32): the raw integers of both directions."""
    descriptors = list(descriptors)
    dev = _lib.find_device("ls2fm.match", descriptors)
    if len(descriptors) == 0:
        raise ValueError("ls2fm.match: no images")
    flat, start = _descriptor_array(descriptors, dev)
    V = len(descriptors)
    if pairs is None:
        pairs = exhaustive_pairs(V)
    pairs = np.ascontiguousarray(torch.as_tensor(pairs).cpu().numpy().reshape(-1, 2).astype(np.int32))
    P = pairs.shape[0]
    if P == 0:
        return ([], []) if return_scores else []
    if pairs.min() < 0 or pairs.max() >= V:
        raise ValueError(f"ls2fm.match: pair index outside [0, {V})")
    counts = np.diff(start).astype(np.int64)
    n_a, n_b = counts[pairs[:, 0]], counts[pairs[:, 1]]
    first = np.concatenate([[0], np.cumsum(n_a)])
    rows = np.concatenate([[0], np.cumsum(n_a + n_b)])
    lib = _lib.load()
    c_start = start.ctypes.data_as(ctypes.c_void_p)
    c_pairs = pairs.ctypes.data_as(ctypes.c_void_p)
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.ls2fm_match_descriptors_workspace_bytes(c_start, V, c_pairs, P), "ls2fm_match_descriptors_workspace_bytes",
                            dev, 16)
        index = torch.empty(int(first[-1]), dtype=torch.int32, device=dev)
        num = torch.empty(P, dtype=torch.int32, device=dev)
        raw = [torch.empty(int(rows[-1]), dtype=torch.int32, device=dev) for _ in range(3)] if return_scores else [None] * 3
        check(lib.ls2fm_match_descriptors(ptr(flat), c_start, V, c_pairs, P, float(max_ratio), float(max_distance),
                                          1 if cross_check else 0, ptr(index), ptr(num), ptr(raw[0]), ptr(raw[1]), ptr(raw[2]),
                                          ptr(ws), stream_ptr()), "ls2fm_match_descriptors")
        # the compacted lists: one nonzero over all pairs, split by the (host-known) row ranges
        hit = torch.nonzero(index >= 0).reshape(-1)
        first_t = torch.as_tensor(first, device=dev)
        pair_of = torch.searchsorted(first_t, hit, right=True) - 1
        both = torch.stack([hit - first_t[pair_of], index[hit].to(torch.int64)], dim=1)
        per_pair = num.cpu().tolist()                    # the one synchronising read: the list lengths
    matches = list(torch.split(both, per_pair))
    if not return_scores:
        return matches
    scores = []
    for p in range(P):
        r0, na, nb = int(rows[p]), int(n_a[p]), int(n_b[p])
        scores.append(dict(best_ab=raw[0][r0:r0 + na], best_j_ab=raw[1][r0:r0 + na], second_ab=raw[2][r0:r0 + na],
                           best_ba=raw[0][r0 + na:r0 + na + nb], best_j_ba=raw[1][r0 + na:r0 + na + nb],
                           second_ba=raw[2][r0 + na:r0 + na + nb]))
    return matches, scores


def assemble_n_views(keypoints, pair_matches, pair_masks, min_matches=50):
    """The `n_views.npy` layout of preparation/main.py:177-247 (pure host function).  keypoints: list of [n_v,2] arrays;
    pair_matches / pair_masks: one [M,2] index array and one bool [M] array per pair a < b in main.py's order (exhaustive_pairs).
    Pairs with fewer than min_matches matches become empty (:193-194).  -> list over views of dict(kypts, indxes, mask): indxes
    is the list over the OTHER views in increasing view index of [M,2] arrays with the view's own keypoint index in column 0
    (the column swap of :241), mask the inlier masks in the same order.
    One deviation: the mask of an empty pair is an empty bool array (main.py:224-227 copies the previous pair's shape, which no
    consumer reads)."""
    n = len(keypoints)
    if len(pair_matches) != n * (n - 1) // 2 or len(pair_masks) != len(pair_matches):
        raise ValueError(f"ls2fm.match.assemble_n_views: {len(pair_matches)} pairs / {len(pair_masks)} masks for {n} views")
    full, masks = [], []
    for m, k in zip(pair_matches, pair_masks):
        m = np.asarray(m.cpu() if torch.is_tensor(m) else m).reshape(-1, 2)
        k = np.asarray(k.cpu() if torch.is_tensor(k) else k).reshape(-1).astype(bool)
        if len(m) < min_matches:
            full.append(np.zeros((0,), dtype=np.uint32))        # main.py:194: np.uint32(np.array([]))
            masks.append(np.zeros((0,), dtype=bool))
        else:
            if len(k) != len(m):
                raise ValueError(f"ls2fm.match.assemble_n_views: mask of {len(k)} for {len(m)} matches")
            full.append(m.astype(np.uint32))
            masks.append(k)
    views = []
    for v in range(n):
        idx, msk = [], []
        for j in range(n):
            if j == v:
                continue
            lo, hi = min(v, j), max(v, j)
            q = (2 * n - lo - 1) * lo // 2 + hi - lo - 1       # the pair's place in main.py's order (:237)
            m = full[q]
            idx.append(m if (j > v or len(m) == 0) else m[:, [1, 0]])
            msk.append(masks[q])
        kp = keypoints[v]
        views.append(dict(kypts=np.asarray(kp.cpu() if torch.is_tensor(kp) else kp), indxes=idx, mask=msk))
    return views


def two_view_tables(keypoints, descriptors, intrinsic=None, min_matches=50, max_ratio=0.8, max_distance=0.7, cross_check=True, seed=0,
                    return_configs=False, **ransac_options):
    """main.py:98-247 without COLMAP: match_descriptors over every pair -> the < min_matches filter -> ONE
    ls2fm.pose.relative_pose call over all surviving pairs for the inlier masks (the call main.py:209-213 makes per pair) ->
    assemble_n_views.  keypoints: list of [n_v,2] pixel arrays; descriptors: list of uint8 [n_v,128]; intrinsic: K [3,3] or
    (fx, fy, cx, cy), one camera for all views (main.py's single_camera), or None when there is no calibration: the masks then
    come from ONE ls2fm.pose.fundamental_matrix call.  **ransac_options go to that estimator.  -> the list np.save would write
    as n_views.npy.  return_configs=True: (that list, config int32 numpy [n (n - 1) / 2]) with ls2fm.pose.two_view_geometry's
    verdict of every pair in main.py's order (DEGENERATE for the filtered ones), from one more pass over the surviving pairs."""
    from . import pose
    n = len(keypoints)
    if len(descriptors) != n:
        raise ValueError(f"ls2fm.match.two_view_tables: {len(descriptors)} descriptor sets for {n} views")
    matches = match_descriptors(descriptors, None, max_ratio, max_distance, cross_check)
    pairs = exhaustive_pairs(n)
    dev = matches[0].device if matches else torch.device("cuda", torch.cuda.current_device())
    kps = [torch.as_tensor(np.asarray(k.cpu() if torch.is_tensor(k) else k), dtype=torch.float64).reshape(-1, 2).to(dev) for k in keypoints]
    keep = [p for p in range(len(matches)) if matches[p].shape[0] >= min_matches]
    masks = [np.zeros((0,), dtype=bool) for _ in matches]
    configs = np.full(len(matches), pose.DEGENERATE, dtype=np.int32)
    if keep:
        uv0 = [kps[pairs[p, 0]][matches[p][:, 0]] for p in keep]
        uv1 = [kps[pairs[p, 1]][matches[p][:, 1]] for p in keep]
        if intrinsic is None:
            out = pose.fundamental_matrix(uv0, uv1, seed=seed, **ransac_options)
        else:
            out = pose.relative_pose(uv0, uv1, intrinsic, intrinsic, seed=seed, **ransac_options)
        inl = out["inliers"].cpu().numpy()
        ps = out["pair_start"].cpu().numpy()
        for q, p in enumerate(keep):
            masks[p] = inl[ps[q]:ps[q + 1]].copy()
        if return_configs:
            geo = pose.two_view_geometry(uv0, uv1, intrinsic, intrinsic, seed=seed)
            configs[keep] = geo["config"].cpu().numpy()
    tables = assemble_n_views(keypoints, [m.cpu().numpy() for m in matches], masks, min_matches)
    return (tables, configs) if return_configs else tables
