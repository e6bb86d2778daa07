#!/usr/bin/env python
"""Classical bundle adjustment timings (HIP events around the whole loop, one warm-up loop, median of repeats)
-> profiles/bundle_adjust_time.json, on two shapes:
  local   4 views, ~4 x 10^3 observations of 1.2 x 10^3 points, 500 iterations
  global  49 views, ~10^5 observations of 2 x 10^4 points, 1000 iterations
for three ways to run the SAME loop (BA_Trad.run_ba's arithmetic):
  device    ls2fm.stage.TradBALoop.run(): one C call, two launches per iteration, nothing read back
  eager     what the library offered before: reprojection_term + se3_to_SE3_fused + torch.optim.Adam + ExponentialLR, with the
            reference's `.item()` per iteration deciding the weight
  captured  the same iteration without the `.item()` (the weight is a device select), recorded once in a CapturedStep and replayed;
            its optimizer is FusedAdam with the schedule on the device -- the strongest captured form the library had
Reported per variant: ms per loop, ms per iteration, kernel launches per iteration (counted with torch.profiler over 3 iterations
for the torch variants; 2 by construction for the device loop).
    python tools/time_bundle_adjust.py [--out profiles/bundle_adjust_time.json] [--reps 5] [--shapes local global]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd")]

from ls2fm import stage  # noqa: E402
from ls2fm.graph import CapturedStep  # noqa: E402
from ls2fm.optim import FusedAdam  # noqa: E402
from ls2fm.utils import camera as _cam  # noqa: E402

SHAPES = dict(local=dict(views=4, points=1200, per_view=1000, iters=500), global_=dict(views=49, points=20000, per_view=2040, iters=1000))
LR = dict(lr_pose_r=5e-3, lr_pose_t=1e-2, lr_xyzs=1e-2, lr_sdf=1e-4, lr_sdf_end=5e-5)


def scene(V, P, per_view, seed, dev):
    """V views on an arc around a blob of P points, per_view of them seen in each view (1 px noise), perturbed start"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (P, 3)) * [1.5, 1.0, 1.0]
    K = np.array([[520.0, 0, 320], [0, 520.0, 240], [0, 0, 1]])
    poses, kp, ids = [], [], []
    for v in range(V):
        ang = -0.6 + 1.2 * v / max(V - 1, 1)
        eye = np.array([5 * np.sin(ang), 0.3 * (v % 2), -5 * np.cos(ang)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross([0, 1.0, 0], fwd); right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        poses.append(np.concatenate([R, (-R @ eye)[:, None]], 1))
        sel = rng.choice(P, per_view, replace=False)
        u = (pts[sel] @ R.T + poses[-1][:, 3]) @ K.T
        kp.append(torch.tensor(u[:, :2] / u[:, 2:] + rng.normal(size=(per_view, 2)), dtype=torch.float32, device=dev))
        ids.append(torch.tensor(sel, device=dev))
    se3 = _cam.lie.SE3_to_se3(torch.tensor(np.stack(poses), dtype=torch.float32)) + 0.004 * torch.randn(V, 6, generator=torch.Generator().manual_seed(seed))
    xyzs = torch.tensor(pts + 0.02 * rng.normal(size=pts.shape), dtype=torch.float32, device=dev)
    return stage.TrackedViews(se3.to(dev), torch.tensor(K, dtype=torch.float32, device=dev), torch.zeros(V, 1, 3, device=dev), kp, ids, xyzs, 1, 1)


class TorchLoop:
    """the loop from the pieces the library had before ls2fm_bundle_adjust_run"""

    def __init__(self, views, iters, captured):
        ref = stage.TradBALoop(views, max_iter=iters, **LR)              # (bookkeeping only: the observation list)
        self.ref, self.iters, self.captured = ref, iters, captured
        self.r = torch.nn.Parameter(ref.se3[:, :3].clone())
        self.t = torch.nn.Parameter(ref.se3[:, 3:].clone())
        self.x = torch.nn.Parameter(ref.xyzs_all.clone())
        groups = [dict(params=[self.r], lr=LR["lr_pose_r"]), dict(params=[self.t], lr=LR["lr_pose_t"]), dict(params=[self.x], lr=LR["lr_xyzs"])]
        self.hi, self.lo = torch.full((), 10.0, device=ref.se3.device), torch.full((), 1.0, device=ref.se3.device)
        if captured:
            self.optim = FusedAdam(groups, scheduled_gamma=ref.gamma)
            for p in (self.r, self.t, self.x):
                p.grad = torch.zeros_like(p)
            self.graph = CapturedStep(self.iteration, params=[self.r, self.t, self.x])
        else:
            self.optim = torch.optim.Adam(groups)
            self.sched = torch.optim.lr_scheduler.ExponentialLR(self.optim, gamma=ref.gamma)

    def iteration(self):
        ref = self.ref
        if not self.captured:
            self.optim.zero_grad()
        poses = _cam.se3_to_SE3_fused(torch.cat([self.r, self.t], dim=1))
        reproj, _ = stage.reprojection_term(self.x[ref.obs_point], poses, ref.view_start, ref._k_host, ref.obs_uv)
        if self.captured:
            w = torch.where(reproj.detach() > 10, self.hi, self.lo)
            for p in (self.r, self.t, self.x):
                p.grad.zero_()
        else:
            w = 10.0 if reproj.item() > 10 else 1.0                      # BA_Trad.py:111-114
        (w * reproj).backward()
        self.optim.step()
        if not self.captured:
            self.sched.step()
        return reproj

    def run(self, n=None):
        for _ in range(self.iters if n is None else n):
            if self.captured:
                self.graph.replay()
            else:
                self.iteration()


def launches_per_iteration(loop):
    from torch.profiler import ProfilerActivity, profile
    loop.run(2)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loop.run(3)
        torch.cuda.synchronize()
    n = sum(e.count for e in prof.key_averages() if getattr(e, "device_time_total", 0) > 0 or getattr(e, "cuda_time_total", 0) > 0)
    return n / 3.0


def timed(make, reps):
    make().run()                                      # warm-up loop: allocator pools, lazy library state
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        loop = make()                                 # construction (CSR build, capture) is outside the timed span
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loop.run()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_adjust_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["local", "global"])
    ap.add_argument("--variants", nargs="*", default=["device", "captured", "eager"])
    args = ap.parse_args()
    dev = "cuda:0"
    res = dict(device=torch.cuda.get_device_name(0), unit="ms, median of repeats (HIP events around the whole loop)", reps=args.reps, shapes={})
    for name in args.shapes:
        sh = SHAPES["global_" if name == "global" else name]
        views = scene(sh["views"], sh["points"], sh["per_view"], 7, dev)
        makers = dict(device=lambda: stage.TradBALoop(views, max_iter=sh["iters"], **LR),
                      captured=lambda: TorchLoop(views, sh["iters"], True), eager=lambda: TorchLoop(views, sh["iters"], False))
        row = dict(views=sh["views"], points=sh["points"], observations=sh["views"] * sh["per_view"], iterations=sh["iters"])
        for variant in args.variants:
            med, runs = timed(makers[variant], args.reps)
            launches = 2.0 if variant == "device" else launches_per_iteration(makers[variant]())
            row[variant] = dict(ms_per_loop=med, ms_per_iteration=med / sh["iters"], runs_ms=runs, launches_per_iteration=launches)
            print(name, variant, row[variant], flush=True)
        res["shapes"][name] = row
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
