#!/usr/bin/env python
"""Absolute pose timings (HIP events, median of repeats) -> profiles/absolute_pose_time.json:
  one view at N in {200, 2000, 20000} x outlier ratio {0.3, 0.7}, and N = 2000 at 0.88 (several rounds)
  (ls2fm.pose.absolute_pose, max_error_px 3, pycolmap's defaults otherwise); 40 views of 2000 in one call against 40
  single-view calls; the pycolmap shim end to end (numpy in, numpy out, the copies included: absolute_pose_estimation +
  pose_refinement, as Registration.PnP calls them).
The only baseline is the numpy restatement (tests/pose_restate.py) on the CPU, one view of 2000 at each outlier ratio: pycolmap
itself is not available, so no pycolmap number is quoted.
    python tools/time_absolute_pose.py [--out profiles/absolute_pose_time.json] [--reps 5]"""
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
    q = rng.normal(size=4)
    R = pose.qvec_to_rotmat(q / np.linalg.norm(q))
    t = rng.normal(size=3) * 0.5
    z = rng.uniform(3, 8, n)
    pc = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], axis=1)
    xyz = (pc - t) @ R
    uv = np.stack([600 * pc[:, 0] / z + 320, 600 * pc[:, 1] / z + 240], axis=1) + rng.normal(size=(n, 2)) * sigma
    k = int(round(ratio * n))
    idx = rng.choice(n, k, replace=False)
    ang = rng.uniform(0, 2 * np.pi, k)
    uv[idx] += np.stack([np.cos(ang), np.sin(ang)], axis=1) * rng.uniform(20, 200, k)[:, None]
    return uv, xyz


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absolute_pose_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    K = torch.tensor(INTR, dtype=torch.float64, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), unit="ms, median of repeats (HIP events)", reps=args.reps, single_view=[])
    for n, ratio in [(n, r) for n in (200, 2000, 20000) for r in (0.3, 0.7)] + [(2000, 0.88)]:    # 0.88: several rounds
        uv, xyz = scene(rng, n, ratio)
        u, x = torch.from_numpy(uv).to(dev), torch.from_numpy(xyz).to(dev)
        r = pose.absolute_pose(u, x, K, max_error_px=3.0)
        med, all_ = timed(lambda: pose.absolute_pose(u, x, K, max_error_px=3.0), args.reps)
        row = dict(n=n, outlier_ratio=ratio, ms=med, runs_ms=all_, trials=int(r["trials"][0]), num_inliers=int(r["num_inliers"][0]))
        res["single_view"].append(row)
        print(row, flush=True)
    views = [scene(rng, 2000, ratio) for ratio in np.linspace(0.2, 0.7, 40)]
    us = [torch.from_numpy(v[0]).to(dev) for v in views]
    xs = [torch.from_numpy(v[1]).to(dev) for v in views]
    Ks = K.expand(40, 4).contiguous()
    med_b, _ = timed(lambda: pose.absolute_pose(us, xs, Ks, max_error_px=3.0), args.reps)

    def singles():
        for u, x in zip(us, xs):
            pose.absolute_pose(u, x, K, max_error_px=3.0)
    med_s, _ = timed(singles, args.reps)
    res["batch_40x2000"] = dict(one_call_ms=med_b, forty_calls_ms=med_s, speedup=med_s / med_b)
    print(res["batch_40x2000"], flush=True)
    uv, xyz = scene(rng, 2000, 0.5)
    cam = pycolmap_compat.Camera(model="SIMPLE_PINHOLE", width=640, height=480, params=[600.0, 320.0, 240.0])

    def shim():
        a = pycolmap_compat.absolute_pose_estimation(uv, xyz, cam, max_error_px=3.0)
        pycolmap_compat.pose_refinement(a["tvec"], a["qvec"], uv, xyz, a["inliers"], cam)
    med_shim, _ = timed(shim, args.reps)
    res["shim_end_to_end_2000_ratio0.5_ms"] = med_shim
    import pose_restate as PR
    base = []
    for ratio in (0.3, 0.7):
        uv, xyz = scene(rng, 2000, ratio)
        t0 = time.perf_counter()
        r = PR.absolute_pose(uv, xyz, INTR, max_error_px=3.0)
        base.append(dict(n=2000, outlier_ratio=ratio, ms=(time.perf_counter() - t0) * 1e3, trials=r["trials"]))
    res["cpu_baseline_numpy_restatement"] = dict(note="tests/pose_restate.py on the host CPU, one run; NOT pycolmap (absent)",
                                                 rows=base)
    print(res["shim_end_to_end_2000_ratio0.5_ms"], base, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
