#!/usr/bin/env python
"""SIFT extraction timings -> profiles/sift_time.json.  HIP events around the whole call (ls2fm.features.extract: conversion,
the library call(s), the one synchronising read of the counts), every timed shape warmed up first, median of repeats with the
spread.  Fails (no fallback) when there is no GPU.  None of these is a pass/fail bar: nothing exists to compare against (the
parent has no such path, COLMAP is not installed).

  shapes    one 1200 x 1600 image; `--views` (49) such images as one call and as that many calls
  beside    the bytes the blur kernels must move at least (every level read once and written once, the DoG planes written once)
            over the blur kernels' time, against the 8.0 TB/s of the project's roofline -- the kernel time comes from a
            kernel-trace run of its own (`--trace-only` is that run's body; pass the summed blur time with --blur-ms)
  images    procedural (tests/sift_scenes.py), one seed per view

    python tools/time_sift.py [--out profiles/sift_time.json] [--reps 5] [--views 49] [--blur-ms X]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd"), os.path.join(ROOT, "tests")]

from ls2fm import features  # noqa: E402

ROOFLINE_BYTES_PER_S = 8.0e12


def images(n, h, w, dev):
    """n procedural images; the generator's smoothing is slow on the host at this size, so a 300 x 400 scene is up-sampled 4x
    bilinearly on the device and a fine seeded noise is added (features at every octave)"""
    import sift_scenes as SC
    out = []
    for v in range(n):
        small = torch.from_numpy(SC.scene(h // 4, w // 4, 100 + v, shapes=80)).to(dev)
        big = torch.nn.functional.interpolate(small[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        g = torch.Generator(device="cpu").manual_seed(v)
        noise = torch.nn.functional.avg_pool2d(torch.randn(1, 1, h + 2, w + 2, generator=g), 3, stride=1)[0, 0].to(dev)
        out.append((big + 0.05 * noise).clamp(0, 1).contiguous())
    return out


def blur_bytes(h, w, first_octave=-1, num_octaves=4):
    """least bytes of the blur kernels for one image: per level one read and one write of a plane, per DoG plane one write"""
    up = 2 if first_octave == -1 else 1
    oh, ow, total = h * up, w * up, 0
    for k in range(num_octaves):
        if min(oh, ow) < 8:
            break
        launches = 6 if k == 0 else 5               # the first level of a later octave is a down-sampling, not a blur
        total += 4 * oh * ow * (2 * launches + 5)
        oh, ow = oh // 2, ow // 2
    return total


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--blur-ms", type=float, default=None, help="summed sift_blur_kernel time of ONE image from a kernel trace")
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_sift.py needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    if args.trace_only:
        one = images(1, args.height, args.width, dev)
        features.extract(one)
        torch.cuda.synchronize()
        features.extract(one)
        torch.cuda.synchronize()
        return
    imgs = images(args.views, args.height, args.width, dev)
    counts = [int(k.shape[0]) for k, _ in features.extract(imgs)]
    res = dict(device=torch.cuda.get_device_name(0), height=args.height, width=args.width, views=args.views,
               rows_per_view=dict(min=min(counts), median=float(np.median(counts)), max=max(counts)))
    res["one_image"] = timed(lambda: features.extract(imgs[:1]), args.reps)
    res["views_one_call"] = timed(lambda: features.extract(imgs), args.reps)
    res["views_separate_calls"] = timed(lambda: [features.extract([i]) for i in imgs], args.reps)
    res["blur_least_bytes_one_image"] = blur_bytes(args.height, args.width)
    if args.blur_ms:
        rate = res["blur_least_bytes_one_image"] / (args.blur_ms * 1e-3)
        res["blur"] = dict(kernel_ms_one_image=args.blur_ms, bytes_per_s=rate, share_of_roofline=rate / ROOFLINE_BYTES_PER_S)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
