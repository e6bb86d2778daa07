#!/usr/bin/env python
"""Times ls2fm.cloud on the 2 M-point sphere cloud of tools/time_metrics.py (radius 100, ~0.25 between neighbours), the cloud
queried against itself, and writes profiles/cloud_time.json:
  grid     PointGrid.query (the floor: one neighbour), PointGrid.knn at k = 8 / 16 / 32 (walked in cell order and, at 16, as given;
           also at 9 and 17, which differ from 8 and 16 by the list capacity that runs),
           the normals kernel alone on a stored list, estimate_normals at k = 16 (knn + normals on a built grid), statistical_outliers
           (k = 20) and radius_outliers (8 within 0.6).  HIP events around windows of --calls calls, the forms ALTERNATED inside every
           repetition, median over the windows.  knn(8) is first checked to be the first 8 columns of knn(32).
  torch    _knn_torch + _normals_torch (the torch forms) on the same GPU at growing sizes, each checked against the kernels first
           (indices and d2 bits equal; whether the covariance bits are equal is recorded), up to the largest a quadratic forecast
           fits into the step's budget
  kdtree   scipy.spatial.cKDTree.query(k=16, workers=16) at the full size on the host, if scipy imports
Every step is a child process under its own time limit; a step that fails or runs out ends the run (the record says which).
    python tools/time_cloud.py [--n 2000000] [--reps 5] [--steps grid,torch,kdtree]"""
import argparse, json, os, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

from time_metrics import RADIUS, alternated, sphere          # noqa: E402  the cloud and the timing loop of tools/time_metrics.py

LIMITS = dict(grid=420, torch=300, kdtree=420)               # seconds per step
TORCH_BUDGET_S = 40.0
RADIUS_FILTER, MIN_NEIGHBORS = 0.6, 8


def step_grid(a):
    import torch
    from ls2fm import cloud, metrics as MT
    p = torch.from_numpy(sphere(a.n, RADIUS, 1)).to("cuda:0")
    g = MT.PointGrid(p)
    occ = int((g.cell_start[1:] > g.cell_start[:-1]).sum())
    res = dict(n=a.n, radius=RADIUS, cell_size=g.cell_size, dim=list(g.dim), cells=g.n_cells, occupied_cells=occ,
               points_per_occupied_cell=a.n / max(occ, 1))
    wide, narrow = g.knn(p, 32), g.knn(p, 8)
    if not (torch.equal(wide[0][:, :8], narrow[0]) and torch.equal(wide[1][:, :8].view(torch.int32), narrow[1].view(torch.int32))):
        raise SystemExit("knn(8) is not the first 8 columns of knn(32)")
    res["capacity_does_not_show"] = True
    res["mean_distance_to_16th"] = float(g.knn(p, 16)[1][:, 15].double().sqrt().mean())
    del wide, narrow
    idx16 = g.knn(p, 16)[0]
    keep_s, keep_r = cloud.statistical_outliers(p, 20)[0], cloud.radius_outliers(p, RADIUS_FILTER, MIN_NEIGHBORS)
    res["kept"] = dict(statistical=int(keep_s.sum()), radius=int(keep_r.sum()))
    forms = {"query": lambda: g.query(p), "build": lambda: MT.PointGrid(p, cell_size=g.cell_size)}
    for k in (8, 9, 16, 17, 32):                      # 9 and 17: one neighbour more, the next list capacity
        forms[f"knn{k}"] = lambda k=k: g.knn(p, k)
    forms["knn16_as_given"] = lambda: g.knn(p, 16, sort=False)
    forms["knn16_skip_own_as_given"] = lambda: g.knn(p, 16, skip_own=True)
    forms["normals_kernel16"] = lambda: cloud.normals_from_neighbors(p, idx16)
    forms["estimate_normals16"] = lambda: cloud.estimate_normals(p, 16, grid=g)
    forms["statistical_outliers20"] = lambda: cloud.statistical_outliers(p, 20)
    forms["radius_outliers8"] = lambda: cloud.radius_outliers(p, RADIUS_FILTER, MIN_NEIGHBORS)
    res["forms"] = alternated(forms, a.reps, calls=a.calls)
    return res


def step_torch(a):
    import torch
    from ls2fm import cloud, metrics as MT
    pts = sphere(a.n, RADIUS, 1)
    res, n = dict(sizes=[]), 8192
    while n <= a.n:
        p = torch.from_numpy(pts[:n]).to("cuda:0")
        g = MT.PointGrid(p)
        want = g.knn(p, 16)
        cov = cloud.normals_from_neighbors(p, want[0], return_cov=True)[2]
        t0 = time.perf_counter()
        got = cloud._knn_torch(p, p, 16)
        cov_t = cloud._normals_torch(p, got[0])[2]
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        if not (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)) and torch.equal(got[2], want[2])):
            raise SystemExit(f"the torch form and the kernel differ at n = {n}")
        cov_equal = bool(torch.equal(cov_t.view(torch.int64), cov.view(torch.int64)))
        t = alternated({"knn_torch16": lambda: cloud._knn_torch(p, p, 16), "normals_torch16": lambda: cloud._normals_torch(p, want[0]),
                        "grid_build_knn16": lambda: MT.PointGrid(p).knn(p, 16), "normals_kernel16": lambda: cloud.normals_from_neighbors(p, want[0])},
                       3 if first_s < 5 else 1)
        res["sizes"].append(dict(n=n, equal=True, covariance_bits_equal=cov_equal, **t))
        print(json.dumps(res["sizes"][-1]), flush=True)
        spent = (t["knn_torch16"]["median_ms"] + t["normals_torch16"]["median_ms"]) / 1e3
        if 4 * spent * (4 if first_s < 5 else 2) > TORCH_BUDGET_S:               # the next size: four times the work, warm call + repetitions
            break
        n *= 2
    res["largest_n"] = res["sizes"][-1]["n"]
    return res


def step_kdtree(a):
    try:
        from scipy.spatial import cKDTree
        import scipy
    except ImportError as e:
        return dict(available=False, reason=f"scipy does not import here: {e}")
    pts = sphere(a.n, RADIUS, 1)
    t0 = time.perf_counter()
    tree = cKDTree(pts)
    t1 = time.perf_counter()
    d, _ = tree.query(pts, k=16, workers=16)
    t2 = time.perf_counter()
    return dict(available=True, scipy=scipy.__version__, workers=16, cpus=os.cpu_count(), build_ms=(t1 - t0) * 1e3, query16_ms=(t2 - t1) * 1e3,
                mean_distance_to_16th=float(np.mean(d[:, 15])))


STEPS = dict(grid=step_grid, torch=step_torch, kdtree=step_kdtree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4, help="calls per timed window of the grid forms")
    ap.add_argument("--steps", default="grid,torch,kdtree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_time.json"))
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --step-out")
    ap.add_argument("--step-out")
    a = ap.parse_args()
    if a.step:
        rec = STEPS[a.step](a)
        with open(a.step_out, "w") as f:
            json.dump(rec, f)
        return
    res = dict(n=a.n, reps=a.reps)
    for name in a.steps.split(","):
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--reps", str(a.reps),
                   "--calls", str(a.calls), "--step", name, "--step-out", tmp.name]
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
