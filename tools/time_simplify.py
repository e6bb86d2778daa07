#!/usr/bin/env python
"""Times ls2fm.simplify on the workload it was sized for -- the marching-cubes mesh of the sphere-plus-box SDF of tools/time_raster.py
sampled at 512^3 (835 k faces) -- at cells of 2, 4 and 8 voxels, and writes profiles/simplify_time.json:
  simplify          end to end: the keys, two sorts, the marks, the segment sums, the solve, the face sorts, the one host read
  sums_kernel       the segment-sum kernel alone (ls2fm_mesh_simplify_place, stage SUMS) on the state of a finished call
  simplify_torch    the same rule as torch ops with index_add_ in fp64 on the same GPU (ls2fm.simplify._simplify_torch); checked
                    first: faces and vertex_map equal, vertices within 1e-5 of the cell
  simplify_to_faces one call at --target faces
Beside the kernel's time stand the bytes the rule must move -- per contributing corner its sorted record (4 + 8 bytes), the face's three
indices and the three gathered vertices (12 + 36), per vertex its sorted record and itself (16 + 12), per output cell its sums -- and that
as a share of 8.0 TB/s.  HIP events around windows of --calls calls, the forms alternated inside every repetition, the median of
--reps windows.
    python tools/time_simplify.py [--res 512] [--cells 2 4 8] [--target 100000] [--reps 5] [--calls 3]"""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

ROOFLINE = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0], help="cell sizes in voxels")
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_time.json"))
    a = ap.parse_args()
    import torch
    from time_raster import alternated, scene
    from ls2fm import _lib, simplify as SP
    dev = "cuda:0"
    verts, faces, _, _ = scene(a.res, 1, 8, 8, dev)
    voxel = 2.0 / (a.res - 1)
    lib = _lib.load()
    code, reg = SP._options("quadric", SP.DEFAULT_REG, "simplify")
    res = dict(volume=a.res, mesh_verts=int(verts.shape[0]), mesh_faces=int(faces.shape[0]), voxel=voxel, reg=reg,
               roofline_bytes_per_s=ROOFLINE, cells={})
    for cv in a.cells:
        cell = SP._cell32(cv * voxel, "time")
        v, f, _, ws_bytes = SP._prepare(verts, faces, "simplify")
        out, st = SP._simplify_device(v, f, lib, ws_bytes, cell, None, code, reg)
        ref = SP._simplify_torch(verts, faces, cell)
        if not (torch.equal(out.faces, ref.faces) and torch.equal(out.vertex_map, ref.vertex_map)):
            raise SystemExit(f"simplify and its torch form differ in faces or vertex_map at cell {cv} voxels")
        worst = float((out.vertices - ref.vertices).abs().max())
        if not worst <= 1e-5 * cell:
            raise SystemExit(f"simplify and its torch form differ by {worst} in a vertex at cell {cv} voxels")
        n_corners = int((st["sorted_corner_head"] != 2 ** 31 - 1).sum())
        n_in = int((out.vertex_map >= 0).sum())
        must_move = n_corners * (12 + 12 + 36) + n_in * (16 + 12) + st["n_out"] * (8 + 8 * SP.N_SUMS + 4)
        forms = {
            "simplify": lambda: SP.simplify(verts, faces, cell),
            "sums_kernel": lambda: SP._place(lib, st, SP._STAGE_SUMS),
            "simplify_torch": lambda: SP._simplify_torch(verts, faces, cell),
        }
        t = alternated(forms, a.reps, a.calls)
        k_ms = t["sums_kernel"]["median_ms"]
        res["cells"][f"{cv:g}"] = dict(cell=cell, out_verts=st["n_out"], surviving_faces=st["n_surviving"], out_faces=st["n_kept"],
                                      contributing_corners=n_corners, vertices_in_output_cells=n_in, worst_vertex_difference_to_torch=worst,
                                      times=t, bytes_must_move=must_move, roofline_ms=must_move / ROOFLINE * 1e3,
                                      sums_kernel_share_of_roofline=must_move / ROOFLINE * 1e3 / k_ms,
                                      torch_over_simplify=t["simplify_torch"]["median_ms"] / t["simplify"]["median_ms"])
        del st, out, ref
    target = SP.simplify_to_faces(verts, faces, a.target)
    res["simplify_to_faces"] = dict(target=a.target, out_faces=int(target.faces.shape[0]), out_verts=int(target.vertices.shape[0]),
                                    times=alternated({"simplify_to_faces": lambda: SP.simplify_to_faces(verts, faces, a.target)}, a.reps, 1))
    res["notes"] = ("HIP-event windows only; no kernel trace and no counter run was made.  What bounds the sums kernel is read from its "
                    "ISA (DESIGN 3.21): one wave per output cell, dependent gathers (sorted record -> face -> three vertices) and 13 "
                    "fp64 butterflies of six steps; latency, not bandwidth.")
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
