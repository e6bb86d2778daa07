#!/usr/bin/env python
"""Times ONE iteration of ls2fm.stage.LMBALoop with THE CAMERA BLOCK (camera=, refine=("f", "k1", "k2"); csrc/bundle_adjust_lm.hip's
CAMERA instantiations and balm_border) against one iteration of the pinhole loop (the CAMERA = false instantiations, the text and
the bits of the loop before the camera block) on the 49-view problem tools/time_ba_lm.py builds, and against the torch fp64 form of the
same iteration on the CPU (host clock, a warm-up run, median of --torch-reps runs).  Writes profiles/ba_lm_camera_time.json.
HIP events on the stream around windows of one `run(1)` of a fresh loop (seven resp. six launches and the two that finish a call), the forms alternated window by window after a warm-up each,
median of --reps windows; construction (prepare, the CSR) is outside the span.  The launches' shares come from the library's opt-in
event pairs, a separate serialised run (the pairs perturb what they measure).  The key points of the camera form are the pinhole
scene's, distorted by a known camera (k1 = -0.2, k2 = 0.05); the loop starts from the pinhole with zero distortion.
    python tools/time_ba_lm_camera.py [--reps 15] [--torch-reps 5] [--no-torch]"""
import argparse, importlib.util, json, os, statistics, sys, time, types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "level-s2fm_official_amd"), ROOT):
    sys.path.insert(0, p)
from ls2fm import _lib, profile, stage, undistort  # noqa: E402

VIEWS, POINTS, PER_VIEW = 49, 20000, 2040
REFINE = ("f", "k1", "k2")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def window(make):
    loop = make()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loop.run(1)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def shares(make):
    lib = _lib.load()
    lib.ls2fm_profile_reset()
    lib.ls2fm_profile_enable(1)
    make().run(1)
    torch.cuda.synchronize()
    times = profile.kernel_times(lib)
    lib.ls2fm_profile_enable(0)
    lib.ls2fm_profile_reset()
    total = sum(t[2] for k, t in times.items() if k.startswith("balm_")) or 1.0
    return {k: dict(avg_us=round(v[0], 2), launches=v[1], share=round(v[2] / total, 4)) for k, v in times.items() if k.startswith("balm_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_lm_camera_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_ba_lm_camera.py needs an MI355X: nothing is timed without one")
    views = _tool("time_bundle_adjust").scene(VIEWS, POINTS, PER_VIEW, 7, "cuda:0")
    K = views.intrinsic.detach().double().cpu()
    k4 = torch.stack([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    true = torch.cat([k4, torch.tensor([-0.2, 0.05, 0, 0, 0, 0, 0, 0], dtype=torch.float64)])
    start = torch.cat([k4, torch.zeros(8, dtype=torch.float64)])
    raw = types.SimpleNamespace(poses=views.poses, intrinsic=None, xyzs=views.xyzs, track_ids=views.track_ids,
                                keypoints=[undistort.distort_points(k.double(), true.to(k.device), out_intr=k4)[0] for k in views.keypoints])
    make_pin = lambda: stage.LMBALoop(views, constant_views=(0,), max_iter=1)
    make_cam = lambda: stage.LMBALoop(raw, constant_views=(0,), max_iter=1, camera=start.to("cuda:0"), refine=REFINE)
    for make in (make_pin, make_cam):
        make().run(1)
    torch.cuda.synchronize()
    t_pin, t_cam = [], []
    for _ in range(a.reps):
        t_pin.append(window(make_pin))
        t_cam.append(window(make_cam))
    res = dict(device=torch.cuda.get_device_name(0), unit="ms, median of windows (HIP events around one run(1)), forms alternated",
               baseline="the pinhole loop of THIS build: its CAMERA = false instantiations have the parent commit's text and register "
                        "counts, and left the parent build's bits on the GPU (poses, points, state, log of 8 iterations): DESIGN 3.30",
               reps=a.reps, views=VIEWS, points=POINTS, observations=VIEWS * PER_VIEW, refine=list(REFINE),
               pinhole=dict(ms=statistics.median(t_pin), windows_ms=t_pin, kernels=shares(make_pin)),
               camera=dict(ms=statistics.median(t_cam), windows_ms=t_cam, kernels=shares(make_cam)))
    res["camera_over_pinhole"] = res["camera"]["ms"] / res["pinhole"]["ms"]
    if not a.no_torch:                                       # the torch fp64 form of the same iteration, on the CPU, host clock
        cpu = types.SimpleNamespace(poses=raw.poses.cpu(), intrinsic=None, xyzs=raw.xyzs.cpu(), track_ids=[t.cpu() for t in raw.track_ids],
                                    keypoints=[k.cpu() for k in raw.keypoints])
        make_cpu = lambda: stage.LMBALoop(cpu, constant_views=(0,), max_iter=1, camera=start, refine=REFINE)
        make_cpu().run(1)                                    # warm-up: allocator, LAPACK's threads
        t_cpu = []
        for _ in range(a.torch_reps):
            loop = make_cpu()
            t0 = time.perf_counter()
            loop.run(1)
            t_cpu.append((time.perf_counter() - t0) * 1e3)
        res["torch_fp64_cpu"] = dict(ms=statistics.median(t_cpu), windows_ms=t_cpu, clock="host, around one run(1) after a warm-up run")
        res["torch_over_camera"] = res["torch_fp64_cpu"]["ms"] / res["camera"]["ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
