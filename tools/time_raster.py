#!/usr/bin/env python
"""Times ls2fm.raster on the workload it was sized for -- the marching-cubes mesh of a sphere-plus-box SDF sampled at 512^3, seen
from 49 views of 1200 x 1600 on a ring around it -- and writes profiles/raster_time.json:
  rasterize    face_id and depth alone, with face_hits, and with barycentrics and face_hits
  mask_votes   against its plain-torch form (ls2fm.raster.mask_votes_torch), the two checked equal first
  clean_mesh   end to end (votes, the rasterisation of the whole mesh, the re-indexing, its host reads), with and without masks
HIP events around windows of --calls calls, the forms alternated inside every repetition, the median of --reps windows.  Next to
each rasterize time stands what the call must move -- faces and vertices once per view, the z-buffer twice (its memset and the
resolve's read) -- and that as a share of 8.0 TB/s.  The masks are the mesh's own silhouettes, eroded by nothing.
    python tools/time_raster.py [--res 512] [--views 49] [--height 1200] [--width 1600] [--reps 7] [--calls 3]"""
import argparse, json, math, os, statistics, sys

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
    for _ in range(reps):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=reps, calls_per_window=calls) for k, v in times.items()}


def scene(res, n_views, H, W, dev):
    """the mesh, world-to-camera poses [n, 3, 4] on a tilted ring of radius 2.6 looking at the origin, and K"""
    import torch
    from ls2fm import mesh
    g = torch.linspace(-1.0, 1.0, res, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    sdf = (x * x + y * y + z * z).sqrt() - 0.55
    for c, h in (((0.45, -0.1, 0.2), (0.3, 0.25, 0.35)),):
        q = torch.stack([(x - c[0]).abs() - h[0], (y - c[1]).abs() - h[1], (z - c[2]).abs() - h[2]], dim=-1)
        sdf = torch.minimum(sdf, q.clamp(min=0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0))
        del q
    del x, y, z
    verts, faces = mesh.marching_cubes(sdf, 0.0, spacing=(2.0 / (res - 1),) * 3, origin=(-1.0,) * 3)
    del sdf
    poses = []
    for i in range(n_views):
        a = 2 * math.pi * i / n_views
        eye = torch.tensor([2.6 * math.cos(a), 0.9 * math.sin(3 * a), 2.6 * math.sin(a)], dtype=torch.float64)
        fz = -eye / eye.norm()
        fx = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), fz)
        fx = fx / fx.norm()
        R = torch.stack([fx, torch.linalg.cross(fz, fx), fz])
        poses.append(torch.cat([R, -(R @ eye)[:, None]], dim=1))
    f = 1400.0 * W / 1600.0
    K = torch.tensor([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    return verts, faces, torch.stack(poses).float().to(dev), K.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_time.json"))
    a = ap.parse_args()
    import torch
    from ls2fm import raster
    dev = "cuda:0"
    H, W, N = a.height, a.width, a.views
    verts, faces, poses, K = scene(a.res, N, H, W, dev)
    n_v, n_f = int(verts.shape[0]), int(faces.shape[0])
    first = raster.rasterize(verts, faces, poses, K, H, W, hits=True)
    covered = first.face_id >= 0
    masks = covered.to(torch.uint8)
    hits = first.face_hits
    per_chunk = max(1, 2 ** 28 // (8 * H * W))
    must_move = N * (12 * n_f + 12 * n_v) + 2 * 8 * N * H * W
    res = dict(volume=a.res, n_verts=n_v, n_faces=n_f, n_views=N, height=H, width=W, views_per_chunk=per_chunk,
               covered_pixels_per_view=float(covered.sum()) / N, faces_seen=int((hits > 0).sum()),
               pixels_per_seen_face=float(hits.sum()) / max(int((hits > 0).sum()), 1),
               bytes_must_move=must_move, roofline_bytes_per_s=ROOFLINE, roofline_ms=must_move / ROOFLINE * 1e3)
    del first, covered
    seen, inside = raster.mask_votes(verts, poses, K, masks)
    ts, ti = raster.mask_votes_torch(verts, poses, K, masks)
    if not (torch.equal(seen, ts) and torch.equal(inside, ti)):
        raise SystemExit(f"mask_votes and its torch form differ on {int(((seen != ts) | (inside != ti)).sum())} vertices")
    res["mask_votes_equal_torch"] = True
    forms = {
        "rasterize": lambda: raster.rasterize(verts, faces, poses, K, H, W),
        "rasterize_hits": lambda: raster.rasterize(verts, faces, poses, K, H, W, hits=True),
        "rasterize_bary_hits": lambda: raster.rasterize(verts, faces, poses, K, H, W, bary=True, hits=True),
        "mask_votes": lambda: raster.mask_votes(verts, poses, K, masks),
        "mask_votes_torch": lambda: raster.mask_votes_torch(verts, poses, K, masks),
        "clean_mesh": lambda: raster.clean_mesh(verts, faces, poses, K, masks=masks, dilate=2),
        "clean_mesh_no_masks": lambda: raster.clean_mesh(verts, faces, poses, K, H=H, W=W),
    }
    res["times"] = alternated(forms, a.reps, a.calls)
    for k in ("rasterize", "rasterize_hits", "rasterize_bary_hits"):
        res["times"][k]["share_of_roofline"] = res["roofline_ms"] / res["times"][k]["median_ms"]
    res["mask_votes_torch_over_hip"] = res["times"]["mask_votes_torch"]["median_ms"] / res["times"]["mask_votes"]["median_ms"]
    out, kept = raster.clean_mesh(verts, faces, poses, K, masks=masks, dilate=2)
    res["clean_mesh_kept_faces"] = int(kept.sum())
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
