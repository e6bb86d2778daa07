#!/usr/bin/env python
"""Times ls2fm.image_metrics.compare_images on the workload it was sized for -- 49 views of 1200 x 1600 x 3 against as many
photographs, the 11-tap Gaussian window -- and writes profiles/image_metrics_time.json:
  kernel        ls2fm_image_compare without the map, and with it (ssim_map: 8 bytes per window and channel written)
  torch         the same rule as a user would write it on the same GPU (ls2fm.image_metrics._compare_torch: grouped conv2d in
                fp64), over --torch-views views at a time (its intermediates are 5 fp64 planes per channel, several times over)
  host          what a user has today: the copy to the host plus the scipy route (gaussian_filter of the five moments, fp64) on
                --host-views views with 16 threads, scaled to all views (said so in the result)
HIP events around windows of --calls calls, the forms alternated inside every repetition, the median of --reps windows; the
kernel and the torch form are checked equal (to the map tolerance of the tests) first.  Next to the kernel's time stands what it
must move -- both images once -- and that at 8.0 TB/s.
    python tools/time_image_metrics.py [--views 49] [--height 1200] [--width 1600] [--reps 7] [--calls 3]"""
import argparse, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT):
    sys.path.insert(0, p)

ROOFLINE = 8.0e12


def alternated(forms, reps, calls):
    """one warm call each, then `reps` rounds that give every form one window of `calls` calls between two HIP events
    -> name -> dict(median_ms, min_ms, max_ms per call)"""
    import torch
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for rep in range(reps):
        print(f"repetition {rep + 1} of {reps}", file=sys.stderr, flush=True)
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=reps, calls_per_window=calls) for k, v in times.items()}


def host_route(a, b, views, threads=16):
    """copy `views` views to the host, then the scipy route on `threads` threads (one view and moment per task) -> seconds"""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from scipy import ndimage as ndi
    t0 = time.perf_counter()
    x, y = a[:views].cpu().numpy().astype(np.float64), b[:views].cpu().numpy().astype(np.float64)
    copied = time.perf_counter()

    def moment(job):
        v, m = job
        p = (x[v], y[v], x[v] * x[v], y[v] * y[v], x[v] * y[v])[m]
        return ndi.gaussian_filter(p, sigma=(1.5, 1.5, 0), truncate=3.5, mode="constant")[5:-5, 5:-5]

    with ThreadPoolExecutor(threads) as pool:
        out = list(pool.map(moment, [(v, m) for v in range(views) for m in range(5)]))
    c1, c2 = 1e-4, 9e-4
    for v in range(views):
        mx, my, xx, yy, xy = out[5 * v:5 * v + 5]
        s = ((2 * mx * my + c1) * (2 * (xy - mx * my) + c2)) / ((mx * mx + my * my + c1) * ((xx - mx * mx) + (yy - my * my) + c2))
        float(s.mean()), float(((x[v] - y[v]) ** 2).mean())
    return copied - t0, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--torch-views", type=int, default=7)
    ap.add_argument("--host-views", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_metrics_time.json"))
    a = ap.parse_args()
    import torch
    from ls2fm import image_metrics as IM
    dev = "cuda:0"
    N, H, W, C = a.views, a.height, a.width, 3
    gen = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(6.0 * (c + 1) * xx + 4.0 * yy) for c in range(C)], dim=-1)
    x = (base[None] + 0.03 * torch.randn(N, H, W, C, device=dev, generator=gen)).clamp(0, 1)
    y = (x + 0.05 * torch.randn(N, H, W, C, device=dev, generator=gen)).clamp(0, 1)
    tv = min(a.torch_views, N)

    def torch_form(full=False):
        parts = [IM._compare_torch(x[s:s + tv], y[s:s + tv], full=full) for s in range(0, N, tv)]
        return parts

    # the two forms agree first: the map of the first chunk to the tests' tolerance, the counts exactly
    k = IM.compare_images(x[:tv], y[:tv], full=True)
    t = IM._compare_torch(x[:tv], y[:tv], full=True)
    gap = float((k.ssim_map - t.ssim_map).abs().max())
    if not (gap <= 4 * 8.63e-13 and torch.equal(k.count, t.count) and torch.equal(k.ssim_count, t.ssim_count)):
        raise SystemExit(f"the kernel and the torch form differ: map gap {gap:.3e}")
    del k, t
    must_move = 2 * N * H * W * C * 4
    res = dict(n_views=N, height=H, width=W, channels=C, n_taps=11, pixel_channels=N * H * W * C, map_gap_kernel_vs_torch=gap,
               bytes_must_move=must_move, roofline_bytes_per_s=ROOFLINE, roofline_ms=must_move / ROOFLINE * 1e3,
               torch_views_per_call=tv)
    forms = {
        "kernel": lambda: IM.compare_images(x, y),
        "kernel_with_map": lambda: IM.compare_images(x, y, full=True),
        "torch": lambda: torch_form(),
    }
    res["times"] = alternated(forms, a.reps, a.calls)
    for name in ("kernel", "kernel_with_map"):
        res["times"][name]["share_of_roofline"] = res["roofline_ms"] / res["times"][name]["median_ms"]
    res["torch_over_kernel"] = res["times"]["torch"]["median_ms"] / res["times"]["kernel"]["median_ms"]
    s = IM.compare_images(x, y)
    p, q = s.mean()
    res["mean_psnr"], res["mean_ssim"] = float(p), float(q)
    hv = min(a.host_views, N)
    try:
        copy_s, total_s = host_route(x, y, hv)
        res["host"] = dict(views_measured=hv, threads=16, copy_ms=copy_s * 1e3, total_ms=total_s * 1e3,
                           scaled_to_all_views_ms=total_s * 1e3 * N / hv, scaled=True, measured_once=True)
    except ImportError:
        res["host"] = "not measured: scipy is not installed"
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
