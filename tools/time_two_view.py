#!/usr/bin/env python
"""Two-view geometry timings (HIP events, one warm-up, median of repeats) -> profiles/two_view_time.json:
  one pair of 2000 correspondences at outlier ratio {0.3, 0.7} through ls2fm.pose.fundamental_matrix, ls2fm.pose.homography and,
  as the scale, ls2fm.pose.relative_pose ON THE SAME INPUTS with the same RANSAC options (COLMAP's two-view defaults:
  max_error_px 4, confidence 0.999, min_inlier_ratio 0.25, trials 100 - 10 000); 40 pairs of 2000 in one call against 40
  single-pair calls for each of the three; ls2fm.pose.two_view_geometry over the 40 pairs with and without intrinsics.
Every call synchronises once per RANSAC round (the host reads one word), so the figures are wall-clock of the whole call as a
caller sees it, measured between HIP events on the caller's stream.
    python tools/time_two_view.py [--out profiles/two_view_time.json] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd"), os.path.join(ROOT, "tests")]

from ls2fm import pose  # noqa: E402

from time_relative_pose import INTR, scene, timed  # noqa: E402

OPTS = dict(max_error_px=4.0, confidence=0.999, min_inlier_ratio=0.25, min_num_trials=100, max_num_trials=10000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    K = torch.tensor(INTR, dtype=torch.float64, device=dev)
    calls = {"fundamental_matrix": lambda a, b, k: pose.fundamental_matrix(a, b, **OPTS),
             "homography": lambda a, b, k: pose.homography(a, b, **OPTS),
             "relative_pose": lambda a, b, k: pose.relative_pose(a, b, k, k, **OPTS)}
    res = dict(device=torch.cuda.get_device_name(0), unit="ms, median of repeats (HIP events), whole call", reps=args.reps, options=OPTS,
               scene="tools/time_relative_pose.scene: general 3-D scene, sigma 0.5 px, outliers uniform over 640 x 480", single_pair=[])
    for ratio in (0.3, 0.7):
        uv0, uv1 = scene(rng, 2000, ratio)
        a, b = torch.from_numpy(uv0).to(dev), torch.from_numpy(uv1).to(dev)
        for name, fn in calls.items():
            r = fn(a, b, K)
            med, all_ = timed(lambda: fn(a, b, K), args.reps)
            row = dict(call=name, n=2000, outlier_ratio=ratio, ms=med, runs_ms=all_, trials=int(r["trials"][0]),
                       num_inliers=int(r["num_inliers"][0]), success=bool(r["success"][0]))
            res["single_pair"].append(row)
            print(row, flush=True)
    pairs = [scene(rng, 2000, ratio) for ratio in np.linspace(0.2, 0.7, 40)]
    us = [torch.from_numpy(p[0]).to(dev) for p in pairs]
    vs = [torch.from_numpy(p[1]).to(dev) for p in pairs]
    Ks = K.expand(40, 4).contiguous()
    res["batch_40x2000"] = {}
    for name, fn in calls.items():
        med_b, _ = timed(lambda: fn(us, vs, Ks), args.reps)

        def singles():
            for u, v in zip(us, vs):
                fn(u, v, K)
        med_s, _ = timed(singles, args.reps)
        res["batch_40x2000"][name] = dict(one_call_ms=med_b, forty_calls_ms=med_s, speedup=med_s / med_b)
        print(name, res["batch_40x2000"][name], flush=True)
    res["two_view_geometry_40x2000_ms"] = dict(
        with_intrinsics=timed(lambda: pose.two_view_geometry(us, vs, Ks, Ks), args.reps)[0],
        without_intrinsics=timed(lambda: pose.two_view_geometry(us, vs), args.reps)[0])
    print(res["two_view_geometry_40x2000_ms"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
