#!/usr/bin/env python
"""Times ls2fm.metrics' nearest-neighbour query on two clouds of 2 M points on a sphere surface at DTU-like density (radius 100,
~0.25 between neighbours; the queries on a sphere 0.3 larger) and writes profiles/metrics_time.json:
  grid        PointGrid build and query per automatic cell-size rule ("surface", "volume"), with and without max_dist, with the
              queries walked in cell order or as given.  HIP events around windows of --calls calls, the forms ALTERNATED inside every
              repetition, median over the windows.  All forms are checked to give the same bytes first.
  bruteforce  nearest_neighbors_bruteforce on the same GPU at growing sizes (n x n), each checked equal to the grid first, up to the
              largest that a quadratic forecast fits into the step's budget; the grid at that size beside it
  kdtree      scipy.spatial.cKDTree (build + query, workers=16) at the full size on the host, if scipy imports
Every step is a child process under its own time limit; a step that fails or runs out ends the run (the record says which).
    python tools/time_metrics.py [--n 2000000] [--reps 5] [--steps grid,bruteforce,kdtree]"""
import argparse, json, os, statistics, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT):
    sys.path.insert(0, p)

RADIUS, OFFSET, MAX_DIST = 100.0, 0.3, 20.0
LIMITS = dict(grid=420, bruteforce=300, kdtree=420)          # seconds per step
BRUTE_BUDGET_S = 60.0                                         # the largest brute-force size is forecast to fit into this


def sphere(n, radius, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return (radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def clouds(n):
    return sphere(n, RADIUS, 1), sphere(n, RADIUS + OFFSET, 2)          # reference, queries


def alternated(forms, reps, calls=1):
    """forms: name -> callable.  One warm call each, then `reps` rounds that give every form one window, in turn: HIP events around
    `calls` calls in a row (enough of them that a window is tens of milliseconds) -> name -> dict(median_ms, min_ms, max_ms PER
    CALL over the windows, reps, calls_per_window)"""
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


def step_grid(a):
    import torch
    from ls2fm import metrics as MT
    dev = "cuda:0"
    ref_h, q_h = clouds(a.n)
    ref, q = torch.from_numpy(ref_h).to(dev), torch.from_numpy(q_h).to(dev)
    lo, hi = ref_h.min(axis=0), ref_h.max(axis=0)
    res = dict(n_ref=a.n, n_query=a.n, radius=RADIUS, offset=OFFSET, max_dist=MAX_DIST, rules={})
    grids, first = {}, None
    for rule in ("surface", "volume"):
        h = MT.auto_cell_size(lo, hi, a.n, rule=rule)
        grids[rule] = g = MT.PointGrid(ref, cell_size=h)
        occ = (g.cell_start[1:] > g.cell_start[:-1]).sum()
        res["rules"][rule] = dict(cell_size=h, dim=list(g.dim), cells=g.n_cells, occupied_cells=int(occ),
                                  points_per_occupied_cell=a.n / max(int(occ), 1))
        for sort in (False, True):
            for md in (None, MAX_DIST):
                out = tuple(t.cpu() for t in g.query(q, md, sort=sort))
                if first is None:
                    first = out
                if not (torch.equal(out[0], first[0]) and torch.equal(out[1].view(torch.int32), first[1].view(torch.int32))):
                    raise SystemExit(f"rule {rule}, sort {sort}, max_dist {md}: the result differs from the first form's")
    res["forms_agree"] = True
    res["mean_distance"] = float(first[1].double().sqrt().mean())
    forms = {}
    for rule, g in grids.items():
        h = g.cell_size
        forms[f"{rule}/build"] = lambda h=h: MT.PointGrid(ref, cell_size=h)
        for sort in (False, True):
            for md in (None, MAX_DIST):
                forms[f"{rule}/query{'_sorted' if sort else ''}{'_max_dist' if md else ''}"] = lambda g=g, md=md, sort=sort: g.query(q, md, sort=sort)
    for k, v in alternated(forms, a.reps, calls=a.calls).items():
        rule, name = k.split("/")
        res["rules"][rule][name] = v
    return res


def step_bruteforce(a):
    import torch
    from ls2fm import metrics as MT
    dev = "cuda:0"
    ref_h, q_h = clouds(a.n)
    res, n, spent = dict(sizes=[]), 16384, 0.0
    while n <= a.n:
        ref, q = torch.from_numpy(ref_h[:n]).to(dev), torch.from_numpy(q_h[:n]).to(dev)
        g = MT.PointGrid(ref)
        want = g.query(q)
        t0 = time.perf_counter()
        got = MT.nearest_neighbors_bruteforce(q, ref)
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        if not (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))):
            raise SystemExit(f"brute force and grid differ at n = {n}")
        t = alternated({"bruteforce": lambda: MT.nearest_neighbors_bruteforce(q, ref), "grid_build_query": lambda: MT.PointGrid(ref).query(q)},
                       3 if first_s < 5 else 1)
        res["sizes"].append(dict(n=n, equal=True, **t))
        spent = t["bruteforce"]["median_ms"] / 1e3
        print(json.dumps(res["sizes"][-1]), flush=True)
        if 4 * spent * (4 if first_s < 5 else 2) > BRUTE_BUDGET_S:           # the next size: four times the work, warm call + repetitions
            break
        n *= 2
    last = res["sizes"][-1]
    res["largest_n"] = last["n"]
    res["quadratic_forecast_full_size_s"] = last["bruteforce"]["median_ms"] / 1e3 * (a.n / last["n"]) ** 2
    return res


def step_kdtree(a):
    try:
        from scipy.spatial import cKDTree
        import scipy
    except ImportError as e:
        return dict(available=False, reason=f"scipy does not import here: {e}")
    ref_h, q_h = clouds(a.n)
    t0 = time.perf_counter()
    tree = cKDTree(ref_h)
    t1 = time.perf_counter()
    d, i = tree.query(q_h, k=1, workers=16)
    t2 = time.perf_counter()
    d, i = tree.query(q_h, k=1, workers=16, distance_upper_bound=MAX_DIST)
    t3 = time.perf_counter()
    return dict(available=True, scipy=scipy.__version__, workers=16, cpus=os.cpu_count(), build_ms=(t1 - t0) * 1e3, query_ms=(t2 - t1) * 1e3,
                query_max_dist_ms=(t3 - t2) * 1e3, mean_distance=float(np.mean(d)))


STEPS = dict(grid=step_grid, bruteforce=step_bruteforce, kdtree=step_kdtree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=25, help="calls per timed window of the grid forms")
    ap.add_argument("--steps", default="grid,bruteforce,kdtree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_time.json"))
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
    if "grid" in res and "bruteforce" in res and "sizes" in res.get("bruteforce", {}) and "rules" in res.get("grid", {}):
        last = res["bruteforce"]["sizes"][-1]
        res["bruteforce_over_grid_at_largest_n"] = last["bruteforce"]["median_ms"] / last["grid_build_query"]["median_ms"]
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    sys.exit(1 if any(isinstance(v, dict) and v.get("failed") for v in res.values()) else 0)


if __name__ == "__main__":
    main()
