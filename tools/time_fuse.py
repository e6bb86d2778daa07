#!/usr/bin/env python
"""Times ls2fm.mvs.fuse_depths on the workload the other tools use -- 49 depth and normal maps of 1200 x 1600 rasterised from the
sphere-plus-box mesh of tools/time_raster.py on its ring of cameras (the depth of ls2fm.raster.rasterize, the face normal under
every pixel turned into the camera's frame and toward the camera, a colour of that normal), S = 4 sources, the maps filtered by
filter_depths (min_consistent = 2) first -- and writes profiles/fuse_time.json:
  fuse_depths          the whole call: both launches, torch's prefix sums, the row count's host read, the outputs' allocation
  mark, emit           each launch alone over all views, through the C entry points, `row` prepared once
  mark_WxH, emit_WxH   the same two launches of variant builds with another workgroup tile (tools/build_variant.sh fuse_wN
                       "-DLS2FM_MVS_FUSE_AB_TILE_W=N" mvs_fuse.hip -> tools/ab/lib_fuse_wN.so; 256 x 1 is a linear run of one row);
                       only the variants that were built are timed, each checked bit-equal to the library first
  fuse_depths_torch    the same rule as torch ops on the same GPU, checked bit-equal first
  depths_to_cloud, depths_to_cloud_voxel_downsample   the unfused cloud, and thinned to one point per voxel, for context
Beside the launches' times stand the bytes they must move -- every array they read once, what they write once -- as a time at
8.0 TB/s, and the compiler's VGPR and scratch figures of the two kernels (hipcc -Rpass-analysis, when hipcc is there).  HIP events
around windows of --calls calls, the forms alternated inside every repetition, the median of --reps windows.
    python tools/time_fuse.py [--mesh-res 512] [--views 49] [--height 1200] [--width 1600] [--reps 5] [--calls 1]"""
import argparse, ctypes, glob, json, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

ROOFLINE = 8.0e12


def maps(verts, faces, poses, K, H, W, per_chunk=7):
    """depth float32 [V, H, W] (+inf off the mesh), normal float32 [V, H, W, 3] in each camera's frame and toward it, colour [V, H, W, 3]"""
    import torch
    from ls2fm import raster
    depth, normal, colour = [], [], []
    xn = ((torch.arange(W, device=verts.device).float() + 0.5) - K[0, 2]) / K[0, 0]
    yn = ((torch.arange(H, device=verts.device).float() + 0.5) - K[1, 2]) / K[1, 1]
    for s in range(0, poses.shape[0], per_chunk):
        P = poses[s:s + per_chunk]
        r = raster.rasterize(verts, faces, P, K, H, W)
        corners = verts[faces.long()[r.face_id.clamp(min=0).long()]]                     # [v, H, W, 3 corners, 3]
        n = torch.linalg.cross(corners[..., 1, :] - corners[..., 0, :], corners[..., 2, :] - corners[..., 0, :])
        n = n / n.norm(dim=-1, keepdim=True).clamp(min=1e-30)
        nc = torch.einsum("vij,vhwj->vhwi", P[:, :, :3], n)
        away = (nc[..., 0] * xn[None, None, :] + nc[..., 1] * yn[None, :, None] + nc[..., 2]) > 0
        nc = torch.where(away[..., None], -nc, nc)
        hit = (r.face_id >= 0)[..., None]
        normal.append(torch.where(hit, nc, torch.tensor([0.0, 0.0, -1.0], device=verts.device)))
        colour.append(torch.where(hit, 0.5 + 0.5 * n, torch.zeros_like(n)))
        depth.append(r.depth)
        del r, corners, n, nc
    return torch.cat(depth).contiguous(), torch.cat(normal).contiguous(), torch.cat(colour).contiguous()


def kernel_resources():
    """VGPRs, SGPRs, scratch and occupancy of the two kernels as the compiler reports them, or None without hipcc"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "level-s2fm_official_amd", "csrc", "mvs_fuse.hip")
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -munsafe-fp-atomics -Rpass-analysis=kernel-resource-usage".split()
    out = subprocess.run([hipcc, *flags, "-c", src, "-o", os.devnull], capture_output=True, text=True).stderr
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: \S*?(mvs_fuse_[a-z]+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-res", type=int, default=512)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--voxel", type=float, default=2.0 / 511)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_time.json"))
    a = ap.parse_args()
    import torch
    from time_raster import alternated, scene
    from ls2fm import _lib, _posed, cloud, metrics, mvs
    dev = "cuda:0"
    H, W, N, S = a.height, a.width, a.views, a.sources
    verts, faces, poses, K = scene(a.mesh_res, N, H, W, dev)
    raw, normal, colour = maps(verts, faces, poses, K, H, W)
    del verts, faces
    sources = mvs.select_sources(poses, S, 3.0, 45.0, centre=(0.0, 0.0, 0.0))
    fkw = dict(near=1e-3, max_reproj=1.0, rel_depth=0.01)
    depth, _ = mvs.filter_depths(raw, poses, K, sources, min_consistent=2, **fkw)
    del raw
    kw = dict(normal=normal, images=colour, max_normal_angle=60.0, **fkw)

    def differ(x, y):
        if x is None or y is None:
            return int(x is not y)
        return int(((x != y) & ~(x.isnan() & y.isnan()) if x.dtype.is_floating_point else x != y).sum()) if x.shape == y.shape else -1

    names = ("points", "normals", "colors", "support", "view", "pixel", "centers")
    got = mvs.fuse_depths(depth, poses, K, sources, **kw)
    ref = mvs.fuse_depths_torch(depth, poses, K, sources, **kw)
    wrong = {n: differ(getattr(got, n), getattr(ref, n)) for n in names}
    if any(wrong.values()):
        raise SystemExit(f"fuse_depths and its torch form differ: {wrong}")
    del ref
    M, pixels = int(got.pixel.shape[0]), int(torch.isfinite(depth).sum())
    hist = torch.bincount(got.support.long(), minlength=S + 2).tolist()

    # the two launches alone, through the C entry points
    p, lib = _lib.ptr, _lib.load()
    poses_c, k4 = _posed.views(poses, K, "time_fuse")
    src = sources.to(torch.int32).contiguous()
    every = torch.arange(N, device=dev)
    rel, back = mvs.relative_poses(poses_c, every, src), mvs.relative_poses(poses_c, every, src, back=True)
    c2w = mvs.cam_to_world(poses_c)
    cos2 = 0.25
    support = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    out = [torch.zeros((M, 3), device=dev), torch.zeros((M, 3), device=dev), torch.zeros((M, 3), device=dev),
           torch.zeros((M,), dtype=torch.int64, device=dev)]
    shared = (p(src), S, p(rel), p(back), p(k4))
    tail = (fkw["near"], fkw["max_reproj"], fkw["rel_depth"], cos2, 0, N)

    def launches(library):
        def mark():
            status = library.ls2fm_mvs_fuse_mark(p(depth), p(normal), N, H, W, *shared, *tail, p(support), _lib.stream_ptr())
            assert status == 0, status

        def emit():
            status = library.ls2fm_mvs_fuse_emit(p(depth), p(normal), p(colour), 3, N, H, W, *shared, p(c2w), *tail, p(support), p(row), M,
                                                 *(p(t) for t in out), _lib.stream_ptr())
            assert status == 0, status
        return mark, emit

    mark, emit = launches(lib)
    mark()
    gives = support.reshape(-1).clamp(max=1)
    row = gives.cumsum(dim=0, dtype=torch.int64)
    row -= gives
    del gives
    emit()
    torch.cuda.synchronize()
    wrong = [differ(x, y) for x, y in zip(out, (got.points, got.normals, got.colors, got.pixel))]
    if any(wrong):
        raise SystemExit(f"the launches alone and fuse_depths differ: {wrong}")
    forms = {"fuse_depths": lambda: mvs.fuse_depths(depth, poses, K, sources, **kw), "mark": mark, "emit": emit}
    tiles = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tools", "ab", "lib_fuse_w*.so"))):
        tw = int(re.search(r"lib_fuse_w(\d+)\.so", path).group(1))
        variant = ctypes.CDLL(path)
        for name in ("ls2fm_mvs_fuse_mark", "ls2fm_mvs_fuse_emit"):
            getattr(variant, name).restype, getattr(variant, name).argtypes = _lib._SIGNATURES[name]
        vm, ve = launches(variant)
        support.fill_(9)
        for t in out:
            t.fill_(9)
        vm()
        ve()
        torch.cuda.synchronize()
        wrong = [differ(x, y) for x, y in zip(out, (got.points, got.normals, got.colors, got.pixel))]
        if any(wrong):
            raise SystemExit(f"the {tw} x {256 // tw} tile and the library's differ: {wrong}")
        tiles[f"{tw}x{256 // tw}"] = True
        forms[f"mark_{tw}x{256 // tw}"], forms[f"emit_{tw}x{256 // tw}"] = vm, ve
    forms["fuse_depths_torch"] = lambda: mvs.fuse_depths_torch(depth, poses, K, sources, **kw)
    forms["depths_to_cloud"] = lambda: cloud.depths_to_cloud(depth, poses, K)
    forms["depths_to_cloud_voxel_downsample"] = lambda: (lambda pts: pts[metrics.voxel_downsample(pts, a.voxel)])(cloud.depths_to_cloud(depth, poses, K)[0])
    thin = forms["depths_to_cloud_voxel_downsample"]()
    # a pixel without a depth reads nothing but its depth; a pixel without a row nothing but its support
    mark_bytes = N * H * W * (4 + 1) + pixels * 12
    gather_bytes = pixels * S * (4 + 12)
    emit_bytes = N * H * W * 1 + M * (8 + 4 + 12 + 12) + M * (12 + 12 + 12 + 8)
    res = dict(n_views=N, height=H, width=W, sources=S, channels=3, library_tile=f"{mvs.FUSE_TILE_W}x{mvs.FUSE_TILE_H}",
               filtered_pixels=pixels, fused_rows=M, rows_over_filtered_pixels=M / max(pixels, 1), support_histogram=hist,
               voxel_downsampled_points=int(thin.shape[0]), voxel=a.voxel, fuse_equals_torch_bit_for_bit=True,
               variant_tiles_equal_the_library_bit_for_bit=tiles, roofline_bytes_per_s=ROOFLINE,
               mark_bytes_must_move=mark_bytes, mark_roofline_ms=mark_bytes / ROOFLINE * 1e3,
               mark_bytes_if_every_partner_gather_missed=mark_bytes + gather_bytes,
               emit_bytes_must_move=emit_bytes, emit_roofline_ms=emit_bytes / ROOFLINE * 1e3, kernel_resources=kernel_resources())
    del thin
    t = res["times"] = alternated(forms, a.reps, a.calls)
    res["mark_over_roofline"] = t["mark"]["median_ms"] / res["mark_roofline_ms"]
    res["emit_over_roofline"] = t["emit"]["median_ms"] / res["emit_roofline_ms"]
    res["torch_over_fuse_depths"] = t["fuse_depths_torch"]["median_ms"] / t["fuse_depths"]["median_ms"]
    res["notes"] = ("HIP-event windows only; no kernel trace and no counter run was made.  The byte figures are reasoned, not counted: "
                    "mark reads every depth, the normal of every pixel with a depth, and writes support; emit reads every support, and "
                    "per row its row index, depth, normal and colour (36 bytes) and writes 44; the partners' gathers are taken to hit "
                    "in cache (mark_bytes_if_every_partner_gather_missed: S gathers of 16 bytes per pixel with a depth on top).  Both "
                    "launches are far from the byte floor: most lanes have no depth or no row and leave at once, the others run a "
                    "dependent chain of divisions and gathers per source, emit in fp64.  kernel_resources is the compiler's report.  "
                    "mark and emit alone run at cos2 = 0.25 (60 degrees) over all views in one launch each; fuse_depths adds the prefix "
                    "sums, the allocations and the host read of the row count.")
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
