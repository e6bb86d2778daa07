#!/usr/bin/env python3
"""Time the device path of get_surface_high_res_mesh phase by phase on the sphere-initialised DTU field, and the components +
extraction call alone on the N^3 extract_mesh mesh.

Phases (synchronised host clocks around each; the median over `--repeats` after one warm-up round), in the order
ls2fm.utils.plots._high_res_device runs them:
  coarse_sweep     the 100^3 uniform lattice through the field
  coarse_mc        marching cubes on it
  components       ls2fm.mesh.largest_component on the coarse mesh
  sampling         ls2fm.mesh.sample_surface(., 10000) + the principal frame + the fitted axes
  fitted_sweep     the rotated resolution-class lattice through the field
  fitted_mc        marching cubes on it + the vertices mapped back through the frame
  ply_write        the ASCII PLY of the final mesh
plus `total`: get_surface_high_res_mesh(backend="device") as called.  On the extract_mesh mesh: HIP events around
largest_component (count, the counts' read-back, emit) and around connected_components, median of `--repeats`.
  python tools/time_high_res_mesh.py [--resolution 512] [--out profiles/high_res_mesh_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-s2fm_official_amd"))

import torch  # noqa: E402

from ls2fm import mesh  # noqa: E402
from ls2fm.models.SDF import SDF  # noqa: E402
from ls2fm.options import make_options  # noqa: E402
from ls2fm.utils import plots, util  # noqa: E402


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def phases(sdf, resolution, ply_path):
    """one run of the device path, phase by phase -> ({phase: ms}, sizes)"""
    out, sizes = {}, {}
    clock = [0.0]

    def start():
        torch.cuda.synchronize()
        clock[0] = time.perf_counter()

    def stop(name):
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - clock[0]) * 1e3

    f = sdf.infer_sdf
    start()
    axes = plots.uniform_axes(100, [-0.6, 0.6])
    z = plots.sdf_on_lattice(f, axes)
    stop("coarse_sweep")
    start()
    sp = float(axes[0][2] - axes[0][1])
    verts, faces = mesh.marching_cubes(plots._mc_volume(z, axes), 0.0, (sp, sp, sp),
                                       (float(axes[0][0]), float(axes[1][0]), float(axes[2][0])))
    stop("coarse_mc")
    sizes["coarse_faces"] = int(faces.shape[0])
    start()
    verts, faces = mesh.largest_component(verts, faces)
    stop("components")
    start()
    cloud = mesh.sample_surface(verts, faces, 10000)
    mean, vecs = plots._principal_frame(cloud)
    axes2, _, _ = plots.fitted_axes(((cloud - mean) @ vecs.t()).cpu(), resolution)
    stop("sampling")
    sizes["fitted_lattice"] = list(plots._lattice_shape(axes2))
    start()
    z2 = plots.sdf_on_lattice(f, axes2, rotation=vecs, offset=mean)
    stop("fitted_sweep")
    start()
    sp2 = float(axes2[0][2] - axes2[0][1])
    verts, faces = mesh.marching_cubes(plots._mc_volume(z2, axes2), 0.0, (sp2, sp2, sp2))
    first = plots.lattice_on_device(axes2, z2.device, 0, 1) @ vecs + mean
    verts = verts @ vecs + first[0]
    stop("fitted_mc")
    del z2
    sizes["final_verts"], sizes["final_faces"] = int(verts.shape[0]), int(faces.shape[0])
    start()
    mesh.write_ply(ply_path, verts, faces, encoding="ascii")
    stop("ply_write")
    sizes["ply_bytes"] = os.path.getsize(ply_path)
    return out, sizes


def event_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--mc-n", type=int, default=512, help="lattice side of the extract_mesh mesh for the components timing")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_high_res_mesh.py measures on the GPU; there is none here")
    torch.manual_seed(0)
    sdf = SDF(make_options("DTU", device="cuda")).to("cuda")
    result = {"device": torch.cuda.get_device_name(0), "resolution": args.resolution}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mesh.ply")
        phases(sdf, args.resolution, path)                                   # warm-up
        runs = []
        for _ in range(args.repeats):
            torch.manual_seed(1)
            ms, sizes = phases(sdf, args.resolution, path)
            runs.append(ms)
        result["phases"] = {k: stats([r[k] for r in runs]) for k in runs[0]}
        result["sizes"] = sizes
        wall = []
        for _ in range(args.repeats):
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t = time.perf_counter()
            plots.get_surface_high_res_mesh(sdf.infer_sdf, resolution=args.resolution, grid_boundary=[-0.6, 0.6], level=0.,
                                            take_components=True, path=path, backend="device")
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t) * 1e3)
        result["total"] = stats(wall)
    # components on the N^3 extract_mesh mesh
    n, size = args.mc_n, 2.0
    vol = util.sdf_volume(sdf, size, n)
    _, _, origin, sizes = util._lattice(size, n, None, None)
    verts, faces = mesh.marching_cubes(vol, 0.0, [s / n for s in sizes], origin)
    del vol
    result["extract_mesh_mesh"] = {
        "N": n, "n_verts": int(verts.shape[0]), "n_faces": int(faces.shape[0]),
        "largest_component": event_ms(lambda: mesh.largest_component(verts, faces), 2, 10),
        "connected_components": event_ms(lambda: mesh.connected_components(faces, verts.shape[0]), 2, 10),
    }
    print(json.dumps(result, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
