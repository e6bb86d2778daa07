#!/usr/bin/env python
"""Times ls2fm.undistort on the workload the other tools use -- 49 photographs of 1200 x 1600 x 3 taken through a barrel lens
(f = 1000, k1 = -0.25, k2 = 0.08 with tangential terms), undistorted under the camera's own pinhole at the photograph's size, plus
49 x 8192 key points -- and writes profiles/undistort_time.json:
  undistort_images, undistort_images_nearest   the launch alone through the C entry point, outputs allocated once
  undistort_images_WxH     the same launch of variant builds with another workgroup tile (tools/build_variant.sh undistort_wN
                           "-DLS2FM_UNDISTORT_AB_TILE_W=N" undistort.hip -> tools/ab/lib_undistort_wN.so; 256 x 1 is a linear run of one
                           row); only the variants that were built are timed, each checked bit-equal to the library first
  undistort_images_torch   the same rule as torch ops on the same GPU, checked bit-equal first (on the first --torch-views views:
                           the torch form holds a dozen [V, H, W, C] temporaries), scaled to all views
  copy                     torch's copy of the photographs: the same bytes, source once and output once
  undistort_points, distort_points, undistort_points_torch   the key points, iters = 10
Beside the times stand the bytes the launch must move -- the photographs once, the output and valid once -- as a time at the copy
rate measured here, at 6.29 TB/s (the copy rate of the README) and at 8.0 TB/s nominal, and the compiler's VGPR and scratch figures
of the kernels (hipcc -Rpass-analysis, when hipcc is there).  HIP events around windows of --calls calls, the forms alternated inside
every repetition, the median of --reps windows.
    python tools/time_undistort.py [--views 49] [--height 1200] [--width 1600] [--points 8192] [--reps 5] [--calls 1]"""
import argparse, ctypes, glob, json, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

NOMINAL, MEASURED_COPY = 8.0e12, 6.29e12


def kernel_resources():
    """VGPRs, SGPRs, scratch and occupancy of the kernels as the compiler reports them, or None without hipcc"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "level-s2fm_official_amd", "csrc", "undistort.hip")
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -munsafe-fp-atomics -Rpass-analysis=kernel-resource-usage".split()
    out = subprocess.run([hipcc, *flags, "-c", src, "-o", os.devnull], capture_output=True, text=True).stderr
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            cur = rows.setdefault(re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "").replace("void ", "")), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--torch-views", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_time.json"))
    a = ap.parse_args()
    import torch
    from time_raster import alternated
    from ls2fm import _lib, undistort as U
    dev = "cuda:0"
    V, H, W, C, T = a.views, a.height, a.width, 3, min(a.torch_views, a.views)
    f = 1000.0 * W / 1600.0
    cam64 = U.camera_from_colmap("OPENCV", [f, f, W / 2.0, H / 2.0, -0.25, 0.08, 1e-3, -5e-4])
    cam = cam64.to(torch.float32).expand(V, 12).contiguous().to(dev)
    k4 = cam[:, :4].contiguous()
    gen = torch.Generator(device=dev).manual_seed(0)
    images = torch.rand((V, H, W, C), device=dev, generator=gen)
    nan = [float("nan")] * C
    fill = (ctypes.c_float * C)(*nan)
    p, lib = _lib.ptr, _lib.load()
    out = torch.empty((V, H, W, C), device=dev)
    valid = torch.empty((V, H, W), dtype=torch.uint8, device=dev)

    def differ(x, y):
        return int(((x != y) & ~(x.isnan() & y.isnan()) if x.dtype.is_floating_point else x != y).sum()) if x.shape == y.shape else -1

    def launch(library, mode):
        def run():
            status = library.ls2fm_undistort_images(p(images), V, H, W, C, p(cam), p(k4), H, W, mode, fill, p(out), p(valid), _lib.stream_ptr())
            assert status == 0, status
        return run

    # bit-equal first: both modes against the torch form on the first T views
    wrong = {}
    for mode, name in ((U.UNDISTORT_BILINEAR, "bilinear"), (U.UNDISTORT_NEAREST, "nearest")):
        launch(lib, mode)()
        ref, rv = U._undistort_images_torch(images[:T], cam[:T], k4[:T], H, W, mode, nan)
        wrong[name] = (differ(out[:T], ref), differ(valid[:T], rv))
        del ref, rv
    if any(any(w) for w in wrong.values()):
        raise SystemExit(f"ls2fm_undistort_images and its torch form differ: {wrong}")
    launch(lib, U.UNDISTORT_BILINEAR)()
    torch.cuda.synchronize()
    library_out, library_valid = out.clone(), valid.clone()
    valid_share = float(library_valid.float().mean())
    forms = {"undistort_images": launch(lib, U.UNDISTORT_BILINEAR), "undistort_images_nearest": launch(lib, U.UNDISTORT_NEAREST)}
    tiles = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tools", "ab", "lib_undistort_w*.so"))):
        tw = int(re.search(r"lib_undistort_w(\d+)\.so", path).group(1))
        variant = ctypes.CDLL(path)
        variant.ls2fm_undistort_images.restype, variant.ls2fm_undistort_images.argtypes = _lib._SIGNATURES["ls2fm_undistort_images"]
        run = launch(variant, U.UNDISTORT_BILINEAR)
        out.fill_(9)
        valid.fill_(9)
        run()
        torch.cuda.synchronize()
        wrong = (differ(out, library_out), differ(valid, library_valid))
        if any(wrong):
            raise SystemExit(f"the {tw} x {256 // tw} tile and the library's differ: {wrong}")
        tiles[f"{tw}x{256 // tw}"] = True
        forms[f"undistort_images_{tw}x{256 // tw}"] = run
    del library_out, library_valid
    forms["undistort_images_torch"] = lambda: U._undistort_images_torch(images[:T], cam[:T], k4[:T], H, W, U.UNDISTORT_BILINEAR, nan)
    forms["copy"] = lambda: out.copy_(images)

    # key points
    N = V * a.points
    uv = torch.rand((N, 2), device=dev, generator=gen, dtype=torch.float64) * torch.tensor([W, H], device=dev, dtype=torch.float64)
    vs = (torch.arange(V + 1, device=dev) * a.points).to(torch.int32)
    cam_d = cam64.expand(V, 12).contiguous().to(dev)
    k_d = cam_d[:, :4].contiguous()
    got, res = U.undistort_points(uv, cam_d, vs, k_d)
    ref, rr = U._camera_points_torch(uv, vs, cam_d, k_d, U.CAMERA_UNDISTORT, 10)
    wrong = (differ(got, ref), differ(res, rr))
    if any(wrong):
        raise SystemExit(f"ls2fm_camera_points and its torch form differ: {wrong}")
    worst_residual_px = float(res.max().sqrt())
    forms["undistort_points"] = lambda: U.undistort_points(uv, cam_d, vs, k_d)
    forms["distort_points"] = lambda: U.distort_points(uv, cam_d, vs, k_d)
    forms["undistort_points_torch"] = lambda: U._camera_points_torch(uv, vs, cam_d, k_d, U.CAMERA_UNDISTORT, 10)

    must_move = V * H * W * (4 * C + 4 * C + 1)
    res = dict(n_views=V, height=H, width=W, channels=C, points=N, iters=10, library_tile=f"{U.UNDISTORT_TILE_W}x{U.UNDISTORT_TILE_H}",
               camera=cam64.tolist(), valid_share=valid_share, worst_point_residual_px=worst_residual_px,
               kernel_equals_torch_bit_for_bit=True, torch_views=T, variant_tiles_equal_the_library_bit_for_bit=tiles,
               bytes_must_move=must_move, nominal_bytes_per_s=NOMINAL, readme_copy_bytes_per_s=MEASURED_COPY,
               floor_ms_at_nominal=must_move / NOMINAL * 1e3, floor_ms_at_readme_copy_rate=must_move / MEASURED_COPY * 1e3,
               kernel_resources=kernel_resources())
    t = res["times"] = alternated(forms, a.reps, a.calls)
    kernel = t["undistort_images"]["median_ms"]
    copy_rate = 2 * V * H * W * 4 * C / (t["copy"]["median_ms"] * 1e-3)
    res["copy_bytes_per_s_measured_here"] = copy_rate
    res["floor_ms_at_the_copy_rate_measured_here"] = must_move / copy_rate * 1e3
    res["kernel_bytes_per_s"] = must_move / (kernel * 1e-3)
    res["kernel_over_floor_at_readme_copy_rate"] = kernel / res["floor_ms_at_readme_copy_rate"]
    res["kernel_over_floor_at_the_copy_rate_measured_here"] = kernel / res["floor_ms_at_the_copy_rate_measured_here"]
    res["torch_ms_scaled_to_all_views"] = t["undistort_images_torch"]["median_ms"] * V / T
    res["torch_over_kernel"] = res["torch_ms_scaled_to_all_views"] / kernel
    res["points_torch_over_kernel"] = t["undistort_points_torch"]["median_ms"] / t["undistort_points"]["median_ms"]
    res["notes"] = ("HIP-event windows only; no kernel trace and no counter run was made.  bytes_must_move is reasoned, not counted: the "
                    "photographs read once, the output and valid written once; the four taps of a pixel are taken to hit in cache after "
                    "their first use.  What bounds the launch is judged from its rate against the copy's on the same buffers, not from "
                    "counters.  kernel_resources is the compiler's report.  The torch form runs on torch_views views and is scaled by "
                    "views / torch_views.  undistort_points and distort_points include the allocation and NaN fill of their outputs.")
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
