#!/usr/bin/env python
"""Descriptor matching timings -> profiles/match_time.json.  HIP events around work that ends in a synchronise, every timed shape
warmed up first, median of repeats; the new path (ls2fm.match.match_descriptors, one call for all pairs) and the baseline are
ALTERNATED inside the same run and the spread of both is reported.  Fails (no fallback) when there is no GPU.

  shapes    one pair 2000 x 2000 and 8192 x 8192; 49 views x 8192 exhaustive (1176 pairs) as one call and as 1176 calls;
            49 views x 2000
  baseline  what a user of the library had before ls2fm.match, written here and not in the library: per pair an fp32
            torch.matmul of the two descriptor sets (exact: every partial sum is an integer below 2^24), the two largest per row
            and per column (torch.topk), the same fp64 thresholds and the cross check
  beside    achieved integer ops/s (2 x 128 x n_a x n_b per pair, per direction swept) against the i8 MFMA peak, and the numpy
            restatement's time for one 8192 x 8192 pair on the host CPU -- a checker's time, NOT COLMAP's (COLMAP is absent)
  --trace-only   warm up and run the 49 x 8192 one-call shape once: the body of a kernel-trace run of its own

    python tools/time_match.py [--out profiles/match_time.json] [--reps 5] [--views 49]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd"), os.path.join(ROOT, "tests")]

from ls2fm import match  # noqa: E402

I8_PEAK_OPS = 256 * 4 * 2.4e9 * 2048      # 256 CUs x 4 SIMDs x 2.4 GHz x 2048 ops / clk (v_mfma_i32_32x32x32_i8: 65536 ops in 32 cycles): 5.0e15


def views_like_sift(rng, n_views, n, dev):
    """n_views images of n SIFT-like descriptors; a third of each image is shared with its neighbours under noise"""
    import match_restate as MR
    base = MR.sift_like(rng, n)
    out = []
    for v in range(n_views):
        d = MR.sift_like(rng, n)
        k = n // 3
        idx = rng.permutation(n)[:k]
        noisy = base[idx] * rng.uniform(0.5, 1.0, size=(k, 128))
        d[:k] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
        out.append(torch.from_numpy(MR.to_bytes(d[rng.permutation(n)])).to(dev))
    return out


def baseline_pair(fa, fb, max_ratio=0.8, max_distance=0.7):
    d = fa @ fb.T                                                     # the n_a x n_b product, written and re-read
    props = []
    for dim in (1, 0):
        k = min(2, d.shape[dim])
        top, idx = torch.topk(d, k, dim=dim)
        best, j = (top[:, 0], idx[:, 0]) if dim == 1 else (top[0], idx[0])
        second = ((top[:, 1] if dim == 1 else top[1]) if k == 2 else torch.zeros_like(best))
        ab = torch.acos(torch.clamp(best.double() / 262144.0, max=1.0))
        as_ = torch.acos(torch.clamp(second.double() / 262144.0, max=1.0))
        ok = (best > 0) & ~(ab > max_distance) & ~(ab >= max_ratio * as_)
        props.append(torch.where(ok, j, torch.full_like(j, -1)))
    i = torch.nonzero(props[0] >= 0).reshape(-1)
    jj = props[0][i]
    keep = props[1][jj] == i
    return torch.stack([i[keep], jj[keep]], dim=1)


def baseline(floats, pairs):
    return [baseline_pair(floats[a], floats[b]) for a, b in pairs]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(new, old, reps):
    new(); old()                                                     # warm-up of both, this shape
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(reps):
        tn.append(event_ms(new))
        to.append(event_ms(old))
    return dict(new_ms=float(np.median(tn)), baseline_ms=float(np.median(to)), new_runs_ms=tn, baseline_runs_ms=to,
                new_spread=float((max(tn) - min(tn)) / np.median(tn)), baseline_spread=float((max(to) - min(to)) / np.median(to)),
                baseline_over_new=float(np.median(to) / np.median(tn)))


def shape_row(name, descs, pairs, reps, check=True):
    floats = [d.float() for d in descs]
    if check:                                                        # the two paths agree on this shape
        got, want = match.match_descriptors(descs, pairs), baseline(floats, pairs[:8])
        assert all(torch.equal(g, w) for g, w in zip(got, want)), f"{name}: new path and baseline disagree"
    row = alternate(lambda: match.match_descriptors(descs, pairs), lambda: baseline(floats, pairs), reps)
    ops = sum(2 * 2 * 128 * descs[a].shape[0] * descs[b].shape[0] for a, b in pairs)      # both directions are swept
    row.update(shape=name, pairs=len(pairs), swept_int_ops=ops, new_ops_per_s=ops / (row["new_ms"] * 1e-3),
               fraction_of_i8_peak=ops / (row["new_ms"] * 1e-3) / I8_PEAK_OPS)
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("runs_ms")}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--skip-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_match.py needs an MI355X: there is no CPU path to time")
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    big = views_like_sift(rng, args.views, 8192, dev)
    all_pairs = match.exhaustive_pairs(args.views).tolist()
    if args.trace_only:
        match.match_descriptors(big, all_pairs)
        torch.cuda.synchronize()
        match.match_descriptors(big, all_pairs)
        torch.cuda.synchronize()
        return
    res = dict(device=torch.cuda.get_device_name(0), unit="ms, median of repeats (HIP events), new path and baseline alternated",
               reps=args.reps, i8_peak_ops_per_s=I8_PEAK_OPS, shapes=[])
    small = views_like_sift(rng, args.views, 2000, dev)
    res["shapes"].append(shape_row("one pair 2000 x 2000", small[:2], [[0, 1]], args.reps))
    res["shapes"].append(shape_row("one pair 8192 x 8192", big[:2], [[0, 1]], args.reps))
    res["shapes"].append(shape_row(f"{args.views} views x 2000, one call", small, all_pairs, args.reps))
    res["shapes"].append(shape_row(f"{args.views} views x 8192, one call", big, all_pairs, max(2, args.reps // 2)))

    def singles():
        for a, b in all_pairs:
            match.match_descriptors([big[a], big[b]], [[0, 1]])
    singles()
    torch.cuda.synchronize()
    t = [event_ms(singles) for _ in range(max(2, args.reps // 2))]
    res["views_x_8192_as_single_calls"] = dict(pairs=len(all_pairs), ms=float(np.median(t)), runs_ms=t)
    print(res["views_x_8192_as_single_calls"], flush=True)
    if not args.skip_cpu:
        import match_restate as MR
        da, db = big[0].cpu().numpy(), big[1].cpu().numpy()
        t0 = time.perf_counter()
        r = MR.match_pair(da, db)
        res["cpu_numpy_restatement_8192x8192"] = dict(note="tests/match_restate.py on the host CPU, one run: a checker's time, NOT COLMAP's",
                                                      ms=(time.perf_counter() - t0) * 1e3, matches=int(len(r["matches"])), threads=os.cpu_count())
        print(res["cpu_numpy_restatement_8192x8192"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
