#!/usr/bin/env python
"""Times one ICP iteration of ls2fm.metrics on the sphere clouds of tools/time_metrics.py (2 M moving points on a sphere 0.3 larger
than the 2 M fixed ones) and writes profiles/icp_time.json:
  query      PointGrid.query alone on the moved points: the floor, the walk is the same
  fused      one iteration of ls2fm_icp_run (icp_accumulate + icp_solve, csrc/icp.hip), nothing read back
  torch_ops  the same iteration as plain torch ops on the same GPU (ls2fm.metrics._icp_torch_step: the transform, PointGrid.query,
             the gather, the reductions, a host read for the solve), checked first to give the same pairs and the same update
each with the source as given and with the source put into the grid's cell order once, outside the timing (what PointGrid.query's
sort does per call).  HIP events around windows of --calls calls, the forms ALTERNATED inside every repetition, medians over the
windows.  The run is a child process under its own time limit.
    python tools/time_icp.py [--n 2000000] [--reps 5] [--calls 10]"""
import argparse, json, os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "level-s2fm_official_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

LIMIT_S = 420


def step(a):
    import numpy as np
    import torch
    from ls2fm import _lib, metrics as MT
    from time_metrics import alternated, clouds, RADIUS, OFFSET
    dev = "cuda:0"
    ref_h, src_h = clouds(a.n)
    ref = torch.from_numpy(ref_h).to(dev)
    grid = MT.PointGrid(ref)
    lib = _lib.load()
    tol_trans = MT.ICP_TOL_TRANS_REL * float(np.linalg.norm(grid.box_max.astype(np.float64) - grid.origin.astype(np.float64)))
    state0 = MT._icp_state(None, None, dev)
    ws = _lib.workspace(lib.ls2fm_icp_workspace_bytes(a.n), "ls2fm_icp_workspace_bytes", dev)
    res = dict(n_src=a.n, n_dst=a.n, radius=RADIUS, offset=OFFSET, max_dist=None, with_scale=False, cell_size=grid.cell_size, forms={})
    forms = {}
    for order in ("as_given", "cell_order"):
        src = torch.from_numpy(src_h).to(dev)
        if order == "cell_order":
            src = src[grid.cell_order(src)].contiguous()
        src64 = src.to(torch.float64)
        state = state0.clone()

        def run(st, iters, idx=None, d2=None, src=src):
            _lib.check(lib.ls2fm_icp_run(_lib.ptr(src), a.n, *grid.c_args(), None, float("inf"), 0, iters, MT.ICP_TOL_ROT, tol_trans,
                                         _lib.ptr(st), None, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(ws), _lib.stream_ptr()), "ls2fm_icp_run")

        def neighbours(p):
            return grid.query(p, None, sort=False)

        def fused(state=state, run=run):
            state.copy_(state0)
            run(state, 1)

        def torch_ops(state=state, src64=src64):
            state.copy_(state0)
            MT._icp_torch_step(src64, ref, None, state, neighbours, False, MT.ICP_TOL_ROT, tol_trans, True)

        # the identity start: p' = p exactly, so the floor queries the source itself
        def query(src=src):
            grid.query(src, None, sort=False)

        # the two forms of the iteration agree before anything is timed: the same pairs, the same update
        idx = torch.empty(a.n, dtype=torch.int32, device=dev)
        d2 = torch.empty(a.n, dtype=torch.float32, device=dev)
        ev = state0.clone()
        run(ev, 0, idx, d2)
        want = grid.query(src, None, sort=False)
        if not (torch.equal(idx, want[0]) and torch.equal(d2.view(torch.int32), want[1].view(torch.int32))):
            raise SystemExit(f"{order}: the fused iteration's pairs differ from PointGrid.query's")
        fused()
        a_state = state.clone()
        torch_ops()
        diff = float((a_state[:13] - state[:13]).abs().max())
        if not (diff < 1e-10 and float(a_state[15]) == float(state[15]) == 1.0):
            raise SystemExit(f"{order}: the fused update and the torch-op update differ by {diff}")
        res[f"{order}_update_difference"] = diff
        res[f"{order}_pairs"] = int(ev[14])
        forms[f"{order}/query"], forms[f"{order}/fused"], forms[f"{order}/torch_ops"] = query, fused, torch_ops
    res["forms_agree"] = True
    for k, v in alternated(forms, a.reps, calls=a.calls).items():
        res["forms"][k] = v
    for order in ("as_given", "cell_order"):
        q, f, t = (res["forms"][f"{order}/{k}"]["median_ms"] for k in ("query", "fused", "torch_ops"))
        res[f"{order}_fused_over_query"] = f / q
        res[f"{order}_torch_ops_over_fused"] = t / f
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_time.json"))
    ap.add_argument("--step-out", help="(internal) run the measurement in this process and write its record there")
    a = ap.parse_args()
    if a.step_out:
        with open(a.step_out, "w") as f:
            json.dump(step(a), f)
        return
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--reps", str(a.reps),
               "--calls", str(a.calls), "--step-out", tmp.name]
        rc = subprocess.run(cmd).returncode
        res = dict(failed=True, returncode=rc, limit_s=LIMIT_S) if rc != 0 else json.load(open(tmp.name))
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    sys.exit(1 if res.get("failed") else 0)


if __name__ == "__main__":
    main()
