#!/usr/bin/env python
"""Times the screened Poisson route of ls2fm.cloud_mesh on the 2 M-point sphere cloud of tools/time_metrics.py (radius 100) with its
analytic normals, into lattices of 256^3 and 512^3 over the default bounds (the box grown by a tenth and two voxels), and writes
profiles/poisson_time.json:
  solve    per lattice: the clear and the finish (ls2fm_poisson_splat without points), the same with the splat (the difference is
           the splat), one level-0 sweep (both colours, ls2fm_poisson_sweep_colour), ls2fm_poisson_solve at 0, 1, 2 and 8 cycles (the
           difference of 2 and 1 is one whole cycle), both launch plans at 2 cycles (first checked to leave the same bits), the tail
           kernel's time per visit (a 16^3 lattice, which it runs alone: 8 cycles against 0), poisson_from_cloud and
           mesh_from_cloud end to end with method="poisson" next to method="mls" on the same lattice, poisson_residual of the
           default solve, and the launches of a cycle at both plans.  The level-0 sweep is stated twice against the measured copy rate
           of 6.29 TB/s: as a share of the least it must move (chi, b and W once and half of chi written: 3.5 floats a lattice
           point) and of the cache lines its two launches fetch (every line of chi, b and W once per colour: 7 floats).
           HIP events around windows, the forms ALTERNATED inside every repetition, median over the windows.
  torch    _poisson_torch (the same rule as plain torch ops) on the same GPU on growing lattices, each checked bit-equal against
           the kernels first, up to the largest a forecast fits into the step's budget (three times the last: the torch form is bound by
           its launches on the coarse levels, and a doubled side adds one level)
Every step is a child process under its own time limit; a step that fails or runs out ends the run (the record says which).
    python tools/time_poisson.py [--n 2000000] [--sides 256,512] [--reps 5] [--steps solve,torch]"""
import argparse, json, os, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

from time_metrics import RADIUS, alternated, sphere          # noqa: E402  the cloud and the timing loop of tools/time_metrics.py

LIMITS = dict(solve=420, torch=300)                          # seconds per step
TORCH_BUDGET_S = 120.0
COPY_RATE = 6.29e12                                          # bytes / s: the measured copy rate of an MI355X
SCREEN, CYCLES, GAMMA = 4.0, 8, 2


def workload(a, side):
    """the cloud, its normals and a lattice of `side` points per axis over the default bounds of poisson_from_cloud"""
    import torch
    pts = sphere(a.n, RADIUS, 1)
    nrm = (pts.astype(np.float64) / np.linalg.norm(pts.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    voxel = 2.4 * RADIUS / (side - 5)                        # 2 R + 2 (0.1 * 2 R + 2 voxels) = (side - 1) voxels
    half = 0.5 * (side - 1) * voxel
    return torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(nrm).to("cuda:0"), voxel, ((-half,) * 3, (half,) * 3)


def same_bits(x, y):
    import torch
    return all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(x, y))


def launches_per_cycle(shape, gamma, tail_points):
    """kernel launches of one cycle(0): a sweep is two, a visit of a level below adds the residual-restriction and the prolongation"""
    from ls2fm import cloud_mesh as CM
    totals = [int(np.prod(s)) for s in CM.poisson_levels(shape)]

    def cycle(level):
        if tail_points and totals[level] <= tail_points:
            return 1
        if level == len(totals) - 1:
            return 2 * CM.POISSON_COARSEST_SWEEPS
        return 4 * CM.POISSON_EDGE_SWEEPS + gamma * (2 + cycle(level + 1))
    return cycle(0)


def step_solve(a):
    import torch
    from ls2fm import cloud_mesh as CM
    res = dict(n=a.n, sphere_radius=RADIUS, screen=SCREEN, gamma=GAMMA, lattices=[])
    for side in a.sides:
        p, n, voxel, bounds = workload(a, side)
        shape, origin = CM._lattice(bounds, voxel)
        total = int(np.prod(shape))
        rec = dict(lattice=list(shape), voxel=voxel, levels=[list(s) for s in CM.poisson_levels(shape)],
                   launches_per_cycle={f"tail_{t}": launches_per_cycle(shape, GAMMA, t) for t in (0, CM.POISSON_TAIL_POINTS)})
        solve = lambda cycles, tail=None: CM._poisson_device(p, n, shape, origin, voxel, SCREEN, cycles, GAMMA, tail)      # noqa: E731
        first = solve(2)
        if not (same_bits(solve(2, 0), first) and same_bits(solve(2, CM.POISSON_TAIL_POINTS), first)):
            raise SystemExit(f"the launch plans leave different bits at {shape}")
        rec["plans_leave_the_same_bits"] = True
        del first
        volume = CM.poisson_from_cloud(p, n, voxel, bounds=bounds)
        rec["residual_after_8_cycles"] = CM.poisson_residual(volume, p, n)
        out = CM.extract(volume)
        rec["mesh"] = dict(vertices=int(out.vertices.shape[0]), faces=int(out.faces.shape[0]))
        _, b, W = CM._poisson_splat_device(p, n, shape, origin, voxel)
        chi = volume.value.clone()
        none = p[:0]
        forms = {
            "clear_and_finish": lambda: CM._poisson_splat_device(none, none, shape, origin, voxel),
            "clear_splat_and_finish": lambda: CM._poisson_splat_device(p, n, shape, origin, voxel),
            "sweep_level0": lambda: [CM._poisson_sweep_colour_device(chi, b, W, 1.0, SCREEN, c) for c in (0, 1)],
            **{f"solve_{c}_cycles": (lambda c=c: solve(c)) for c in (0, 1, 2, CYCLES)},
            "solve_2_cycles_without_tail": lambda: solve(2, 0),
            "poisson_from_cloud": lambda: CM.poisson_from_cloud(p, n, voxel, bounds=bounds),
            "mesh_from_cloud_poisson": lambda: CM.mesh_from_cloud(p, n, voxel=voxel, bounds=bounds, method="poisson"),
            "mesh_from_cloud_mls": lambda: CM.mesh_from_cloud(p, n, voxel=voxel, bounds=bounds, method="mls"),
        }
        rec["forms"] = t = alternated(forms, a.reps)
        ms = lambda k: t[k]["median_ms"]                                                                                  # noqa: E731
        rec["splat_ms"] = ms("clear_splat_and_finish") - ms("clear_and_finish")
        rec["cycle_ms"] = ms("solve_2_cycles") - ms("solve_1_cycles")
        # the least a sweep must move: chi, b and W once and half of chi written, 3.5 floats a lattice point.  What its two launches
        # fetch: every cache line of chi, b and W once PER COLOUR (a colour uses every second float of a line) and half of chi written
        for key, floats in (("least", 3.5), ("fetched_lines", 2 * 3.5)):
            rec[f"sweep_level0_{key}_bytes"] = floats * 4 * total
            rec[f"sweep_level0_{key}_share_of_copy_rate"] = floats * 4 * total / COPY_RATE / (ms("sweep_level0") / 1e3)
        res["lattices"].append(rec)
        print(json.dumps(rec), flush=True)
        del volume, out, b, W, chi
        torch.cuda.empty_cache()
    # the tail kernel alone: a lattice it runs by itself
    p, n, voxel, bounds = workload(a, 16)
    shape, origin = CM._lattice(bounds, voxel)
    t = alternated({f"solve_{c}_cycles": (lambda c=c: CM._poisson_device(p, n, shape, origin, voxel, SCREEN, c, GAMMA)) for c in (0, CYCLES)},
                   a.reps, calls=8)
    res["tail"] = dict(lattice=list(shape), levels=[list(s) for s in CM.poisson_levels(shape)], forms=t,
                       visit_ms=(t[f"solve_{CYCLES}_cycles"]["median_ms"] - t["solve_0_cycles"]["median_ms"]) / CYCLES)
    return res


def step_torch(a):
    import torch
    from ls2fm import cloud_mesh as CM
    res, side = dict(sizes=[]), 32
    while side <= max(a.sides):
        p, n, voxel, bounds = workload(a, side)
        shape, origin = CM._lattice(bounds, voxel)
        want = CM._poisson_device(p, n, shape, origin, voxel, SCREEN, CYCLES, GAMMA)
        t0 = time.perf_counter()
        got = CM._poisson_torch(p, n, shape, origin, voxel, SCREEN, CYCLES, GAMMA)
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        if not same_bits(got, want):
            raise SystemExit(f"the torch form and the kernels differ at a lattice of {side}^3")
        t = alternated({"poisson_torch": lambda: CM._poisson_torch(p, n, shape, origin, voxel, SCREEN, CYCLES, GAMMA),
                        "kernels": lambda: CM._poisson_device(p, n, shape, origin, voxel, SCREEN, CYCLES, GAMMA)}, 3 if first_s < 5 else 1)
        res["sizes"].append(dict(side=side, equal=True, **t))
        print(json.dumps(res["sizes"][-1]), flush=True)
        if 3 * t["poisson_torch"]["median_ms"] / 1e3 * (5 if first_s < 5 else 3) > TORCH_BUDGET_S:      # the next size: one level more
            break
        side *= 2
    res["largest_side"] = res["sizes"][-1]["side"]
    return res


STEPS = dict(solve=step_solve, torch=step_torch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--sides", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", default="solve,torch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_time.json"))
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --step-out")
    ap.add_argument("--step-out")
    a = ap.parse_args()
    sides = a.sides
    a.sides = [int(s) for s in sides.split(",")]
    if a.step:
        rec = STEPS[a.step](a)
        with open(a.step_out, "w") as f:
            json.dump(rec, f)
        return
    res = dict(n=a.n, sides=a.sides, reps=a.reps)
    for name in a.steps.split(","):
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--sides", sides,
                   "--reps", str(a.reps), "--step", name, "--step-out", tmp.name]
            t0 = time.perf_counter()
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                res[name] = dict(failed=True, returncode=rc, limit_s=LIMITS[name])
                print(f"step {name} ended with status {rc}: nothing further is started", file=sys.stderr)
                break
            res[name] = json.load(open(tmp.name))
            res[name]["step_wall_s"] = time.perf_counter() - t0
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    sys.exit(1 if any(isinstance(v, dict) and v.get("failed") for v in res.values()) else 0)


if __name__ == "__main__":
    main()
