#!/usr/bin/env python3
"""Time marching cubes (ls2fm_marching_cubes_count / _emit) on the sweep of a sphere-initialised DTU field, and extract_mesh end to end.

Per size: HIP events around each call on the current stream, `--warmup` untimed rounds, the median (and min / max) over `--repeats`.
  sweep       ls2fm_sdf_volume over the N^3 lattice (for scale)
  count       classification + tile scan (2 launches)
  emit        vertices + faces (2 launches)
  mc          ls2fm.mesh.marching_cubes as a user calls it: count, the counts' read-back, allocation, emit (events around all of it)
  extract     util.extract_mesh(backend="device") wall time: sweep + marching cubes + PLY write to `--ply-dir`
  python tools/mc_time.py [--sizes 256 512] [--out profiles/mc_time.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-s2fm_official_amd"))

import torch  # noqa: E402

from ls2fm import _lib, mesh  # noqa: E402
from ls2fm.models.SDF import SDF  # noqa: E402
from ls2fm.options import make_options  # noqa: E402
from ls2fm.utils import util  # noqa: E402


def timed(fn, warmup, repeats):
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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ply-dir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mc_time.py measures on the GPU; there is none here")
    lib = _lib.load()
    torch.manual_seed(0)
    opt = make_options("DTU", device="cuda")
    sdf = SDF(opt).to("cuda")
    rows = []
    for n in args.sizes:
        size = 2.0
        vol = util.sdf_volume(sdf, size, n)
        _, _, origin, sizes = util._lattice(size, n, None, None)
        sp = (ctypes.c_float * 3)(*[s / n for s in sizes])
        og = (ctypes.c_float * 3)(*origin)
        ws = torch.empty(lib.ls2fm_marching_cubes_workspace_bytes(n, n, n), dtype=torch.uint8, device="cuda")
        counts = torch.empty(2, dtype=torch.int64, device="cuda")

        def count():
            _lib.check(lib.ls2fm_marching_cubes_count(_lib.ptr(vol), n, n, n, 0.0, _lib.ptr(ws), _lib.ptr(counts), _lib.stream_ptr()),
                       "count")

        count()
        nv, nf = (int(v) for v in counts.cpu())
        verts = torch.empty(nv, 3, device="cuda")
        faces = torch.empty(nf, 3, dtype=torch.int32, device="cuda")

        def emit():
            _lib.check(lib.ls2fm_marching_cubes_emit(_lib.ptr(vol), n, n, n, 0.0, sp, og, _lib.ptr(ws), _lib.ptr(verts),
                                                     _lib.ptr(faces), _lib.stream_ptr()), "emit")

        row = {"N": n, "n_verts": nv, "n_faces": nf, "workspace_bytes": ws.numel(),
               "sweep": timed(lambda: util.sdf_volume(sdf, size, n), args.warmup, args.repeats),
               "count": timed(count, args.warmup, args.repeats),
               "emit": timed(emit, args.warmup, args.repeats),
               "mc": timed(lambda: mesh.marching_cubes(vol, 0.0, [s / n for s in sizes], origin), args.warmup, args.repeats)}
        row["count_plus_emit_ms"] = row["count"]["median_ms"] + row["emit"]["median_ms"]
        with tempfile.TemporaryDirectory(dir=args.ply_dir) as d:
            path = os.path.join(d, "surface.ply")
            util.extract_mesh(sdf, volume_size=size, N=n, filepath=path, backend="device")           # warm-up
            wall = []
            for _ in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                util.extract_mesh(sdf, volume_size=size, N=n, filepath=path, backend="device")
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t) * 1e3)
            row["extract_mesh_wall_ms"] = {"median_ms": statistics.median(wall), "min_ms": min(wall), "max_ms": max(wall),
                                           "repeats": 3, "ply_bytes": os.path.getsize(path)}
        del ws, verts, faces, vol
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
