#!/usr/bin/env python
"""Relative pose timings (HIP events, one warm-up, median of repeats) -> profiles/relative_pose_time.json:
  one pair at N in {200, 2000, 20000} x outlier ratio {0.3, 0.7} (ls2fm.pose.relative_pose, pycolmap 0.3.0's defaults as we read
  them: max_error_px 4, confidence 0.999, trials 1000 - 100 000); 40 pairs of 2000 in one call against 40 single-pair calls;
  the pycolmap shim end to end (numpy in, numpy out) and ls2fm.pose.triangulate of 100 000 points.
The only CPU figure is the numpy restatement (tests/relpose_restate.py) of one pair of 200 at 0.3: pycolmap is not available.
    python tools/time_relative_pose.py [--out profiles/relative_pose_time.json] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd"), os.path.join(ROOT, "tests")]

from ls2fm import pose  # noqa: E402
from ls2fm.utils import pycolmap_compat  # noqa: E402

INTR = (600.0, 600.0, 320.0, 240.0)


def scene(rng, n, ratio, sigma=0.5):
    w = rng.normal(size=3)
    w *= np.radians(rng.uniform(5, 20)) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    R = pose.qvec_to_rotmat(np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * w / th]))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 10, n)], axis=1)
    X2 = X @ R.T + t
    uv0 = np.stack([600 * X[:, 0] / X[:, 2] + 320, 600 * X[:, 1] / X[:, 2] + 240], axis=1) + rng.normal(size=(n, 2)) * sigma
    uv1 = np.stack([600 * X2[:, 0] / X2[:, 2] + 320, 600 * X2[:, 1] / X2[:, 2] + 240], axis=1) + rng.normal(size=(n, 2)) * sigma
    k = int(round(ratio * n))
    idx = rng.choice(n, k, replace=False)
    uv1[idx] = rng.uniform((0, 0), (640, 480), (k, 2))
    return uv0, uv1


def timed(fn, reps):
    fn()                                              # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relative_pose_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    K = torch.tensor(INTR, dtype=torch.float64, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), unit="ms, median of repeats (HIP events)", reps=args.reps, single_pair=[])
    for n, ratio in [(n, r) for n in (200, 2000, 20000) for r in (0.3, 0.7)]:
        uv0, uv1 = scene(rng, n, ratio)
        a, b = torch.from_numpy(uv0).to(dev), torch.from_numpy(uv1).to(dev)
        r = pose.relative_pose(a, b, K, K)
        med, all_ = timed(lambda: pose.relative_pose(a, b, K, K), args.reps)
        row = dict(n=n, outlier_ratio=ratio, ms=med, runs_ms=all_, trials=int(r["trials"][0]), num_inliers=int(r["num_inliers"][0]),
                   success=bool(r["success"][0]))
        res["single_pair"].append(row)
        print(row, flush=True)
    pairs = [scene(rng, 2000, ratio) for ratio in np.linspace(0.2, 0.7, 40)]
    us = [torch.from_numpy(p[0]).to(dev) for p in pairs]
    vs = [torch.from_numpy(p[1]).to(dev) for p in pairs]
    Ks = K.expand(40, 4).contiguous()
    med_b, _ = timed(lambda: pose.relative_pose(us, vs, Ks, Ks), args.reps)

    def singles():
        for u, v in zip(us, vs):
            pose.relative_pose(u, v, K, K)
    med_s, _ = timed(singles, args.reps)
    res["batch_40x2000"] = dict(one_call_ms=med_b, forty_calls_ms=med_s, speedup=med_s / med_b)
    print(res["batch_40x2000"], flush=True)
    uv0, uv1 = scene(rng, 2000, 0.5)
    cam = pycolmap_compat.Camera(model="SIMPLE_PINHOLE", width=640, height=480, params=[600.0, 320.0, 240.0])
    res["shim_end_to_end_2000_ratio0.5_ms"], _ = timed(lambda: pycolmap_compat.essential_matrix_estimation(uv0, uv1, cam, cam), args.reps)
    uv0, uv1 = scene(rng, 100000, 0.0)
    a, b = torch.from_numpy(uv0).to(dev), torch.from_numpy(uv1).to(dev)
    P0 = torch.tensor([[600.0, 0, 320, 0], [0, 600, 240, 0], [0, 0, 1, 0]], dtype=torch.float64, device=dev)
    res["triangulate_100000_ms"], _ = timed(lambda: pose.triangulate(P0, P0, a, b), args.reps)
    import relpose_restate as RR
    uv0, uv1 = scene(rng, 200, 0.3)
    t0 = time.perf_counter()
    r = RR.relative_pose(uv0, uv1, INTR, INTR)
    res["cpu_numpy_restatement"] = dict(note="tests/relpose_restate.py on the host CPU, one run; NOT pycolmap (absent)", n=200,
                                        outlier_ratio=0.3, ms=(time.perf_counter() - t0) * 1e3, trials=r["trials"])
    print(res["shim_end_to_end_2000_ratio0.5_ms"], res["triangulate_100000_ms"], res["cpu_numpy_restatement"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
