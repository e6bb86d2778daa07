#!/usr/bin/env python
"""Times ls2fm.stage.LMBALoop (Levenberg-Marquardt with a Schur complement, csrc/bundle_adjust_lm.hip) against ls2fm.stage.TradBALoop
(Adam, 1000 iterations) and writes profiles/ba_lm_time.json.  HIP events on the stream around windows of whole loops, the two solvers
alternated window by window after a warm-up loop each, median of --reps windows; construction (prepare, the CSR) is outside the span.
  local    4 views, 4000 observations of 1200 points            (the shapes of tools/time_bundle_adjust.py)
  global   49 views, ~10^5 observations of 2 x 10^4 points
  cap      128 views x 800 observations of 2 x 10^4 points: what balm_schur's lookups and the one-workgroup solve cost at the cap
Per shape: time to the stop of each solver, its iterations, the final mean reprojection error of each, and the LM kernels' shares
from the library's opt-in event pairs (a separate, serialised run: the pairs perturb the loop they measure).
Then `reconstruct` on the 49 x 8192 ring of tools/time_mapper.py with both solvers: end to end (host clock around work that ends in
a synchronise, the first run apart), the time inside `adjust`, registered views, final mean error.
    python tools/time_ba_lm.py [--reps 7] [--shapes local global cap] [--no-reconstruct] [--views 49] [--kp 8192]"""
import argparse, importlib.util, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "level-s2fm_official_amd"), ROOT):
    sys.path.insert(0, p)
from ls2fm import _lib, profile, stage  # noqa: E402

W, H = 640, 480
SHAPES = dict(local=dict(views=4, points=1200, per_view=1000), global_=dict(views=49, points=20000, per_view=2040),
              cap=dict(views=128, points=20000, per_view=800))
ADAM_ITERS = 1000


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mean_error(views, poses, X):
    """mean pixel error of a state over the scene's observations (torch ops on the device)"""
    probe = stage.LMBALoop(views, max_iter=1)
    probe.poses, probe.xyzs_all = poses.double().contiguous(), X.double().contiguous()
    return float(probe.mean_error())


def window(make):
    loop = make()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loop.run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), loop


def time_shape(views, reps, lm_kw):
    from ls2fm.utils import camera as cam
    make_lm = lambda: stage.LMBALoop(views, constant_views=(0,), max_iter=50, **lm_kw)
    make_adam = lambda: stage.TradBALoop(views, max_iter=ADAM_ITERS)
    for make in (make_lm, make_adam):                       # warm-up: allocator pools, lazy library state
        make().run()
    torch.cuda.synchronize()
    t_lm, t_adam = [], []
    for _ in range(reps):                                   # alternated windows
        ms, lm = window(make_lm)
        t_lm.append(ms)
        ms, adam = window(make_adam)
        t_adam.append(ms)
    reason, iters = lm.stopped()
    se3, xyz, _ = adam.written_back()
    row = dict(lm=dict(ms_to_stop=statistics.median(t_lm), windows_ms=t_lm, stop=reason, iterations=iters, cost=float(lm.cost()),
                       mean_error_px=mean_error(views, lm.poses, lm.xyzs_all), options=dict(constant_views=[0], max_iter=50, **lm_kw)),
               adam=dict(ms_per_loop=statistics.median(t_adam), windows_ms=t_adam, iterations=ADAM_ITERS,
                         mean_error_px=mean_error(views, cam.lie.se3_to_SE3(se3.double()), xyz)))
    lib = _lib.load()                                       # the kernels' shares: event pairs around every launch, a run of its own
    lib.ls2fm_profile_reset()
    lib.ls2fm_profile_enable(1)
    make_lm().run()
    torch.cuda.synchronize()
    times = profile.kernel_times(lib)
    lib.ls2fm_profile_enable(0)
    lib.ls2fm_profile_reset()
    total = sum(t[2] for t in times.values()) or 1.0
    row["lm"]["kernels"] = {k: dict(avg_us=round(v[0], 2), launches=v[1], share=round(v[2] / total, 4)) for k, v in times.items() if k.startswith("balm_")}
    return row


class _AdjustClock:
    def __init__(self, mapper):
        self.ms, fn = 0.0, mapper.adjust

        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            self.ms += (time.perf_counter() - t0) * 1e3
            return out
        mapper.adjust = run


def time_reconstruct(views, kp):
    import tracks_scenes as S
    from ls2fm import mapper as M
    scene = S.match_scene(31, n_views=views, n_kp=kp, n_points=int(kp * 1.5), arc_deg=360.0, n_conflicts=50, miss=0.6)
    out = {}
    for solver in ("lm", "adam"):
        opt = M.MapperOptions(ba_solver=solver, **S.ba_rates())
        walls = []
        for _ in range(3):                                  # the first run is the warm-up and is reported apart
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = M.reconstruct(scene["tables"], S.K, H, W, opt, device="cuda:0")
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        m = M._Mapper(scene["tables"], S.K, H, W, opt, "cuda:0")
        clock = _AdjustClock(m)
        with torch.cuda.device(m.dev):
            m.initialise(); m.update(); m.triangulate_new(); m.adjust(None, True); m.update()
            n = 0
            while len(m.order) < m.V:
                n += 1
                if not m.step(n):
                    break
            torch.cuda.synchronize()
        out[solver] = dict(first_run_ms=walls[0], wall_ms=statistics.median(walls[1:]), warm_runs_ms=walls[1:], ba_ms=clock.ms,
                           registered=int(rec.registered.sum()), valid_points=int(rec.track_valid.sum()),
                           last_ba_error_px=rec.log[-1]["ba_error"] if rec.log else None)
        print("reconstruct", solver, out[solver], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", nargs="*", default=["local", "global", "cap"])
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--kp", type=int, default=8192)
    ap.add_argument("--no-reconstruct", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_lm_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_ba_lm.py needs an MI355X: nothing is timed without one")
    scenes = _tool("time_bundle_adjust")
    res = dict(device=torch.cuda.get_device_name(0), unit="ms, median of windows (HIP events around the whole loop), solvers alternated",
               reps=a.reps, shapes={})
    for name in a.shapes:
        sh = SHAPES["global_" if name == "global" else name]
        views = scenes.scene(sh["views"], sh["points"], sh["per_view"], 7, "cuda:0")
        row = dict(views=sh["views"], points=sh["points"], observations=sh["views"] * sh["per_view"])
        row.update(time_shape(views, a.reps, dict(loss="trivial")))
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
    if not a.no_reconstruct:
        res["reconstruct"] = dict(views=a.views, keypoints_per_view=a.kp, **time_reconstruct(a.views, a.kp))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
