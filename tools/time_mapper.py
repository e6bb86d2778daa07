#!/usr/bin/env python
"""Times ls2fm.mapper on a synthetic ring scene (tests/tracks_scenes.match_scene, default 49 views x 8192 key points) and writes
profiles/mapper_time.json.  Device events on the stream around windows of --batch calls, the kernel form and the torch form alternated window by window
after three warm-up calls each, per-call median over --reps windows; `reconstruct` three times with a host clock around work that
ends in a synchronise, the first run reported apart as the warm-up.
  view_scores           ls2fm_view_scores against the same score as torch ops on the device (`unique` over cell ids per level)
  update_observations   ls2fm_update_observations against its torch-op form (projection, masks, index_add_; the angle over the first
                        64 kept observations by a padded [T, m, m] pair tensor)
  reconstruct           end to end, with the time spent per stage (each stage synchronised: the breakdown run is a second run)
Both torch forms are checked against the kernels' results on the timed inputs before anything is timed.
    python tools/time_mapper.py [--views 49] [--kp 8192] [--reps 7] [--batch 50] [--ba-iters 1000] [--no-reconstruct]"""
import argparse, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "level-s2fm_official_amd"), ROOT):
    sys.path.insert(0, p)
import tracks_scenes as S           # noqa: E402
from ls2fm import mapper as M, tracks as TR  # noqa: E402

W, H = 640, 480


def timed_pair(fn_a, fn_b, reps, batch):
    """two forms of one computation, alternated: per repetition one window of `batch` calls of each between device events
    -> (dict, dict) of milliseconds PER CALL: the median, the smallest and the largest window"""
    out = ([], [])
    for fn in (fn_a, fn_b):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in enumerate((fn_a, fn_b)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / batch)
    return tuple(dict(median_ms=statistics.median(o), min_ms=min(o), max_ms=max(o), reps=reps, calls_per_window=batch) for o in out)


def torch_scores(track_of, view, uv, keep, valid, reg, V):
    """the rule of ls2fm_view_scores as index operations: one `unique` over (view, level, cell) ids"""
    T = valid.numel()
    seen = torch.zeros(T, dtype=torch.int64, device=view.device).index_add_(0, track_of, (valid[track_of] & keep & reg[view]).long()) > 0
    counting = seen[track_of] & ~reg[view]
    num = torch.zeros(V, dtype=torch.int64, device=view.device).index_add_(0, view, counting.long())
    v = view[counting]
    q = 64.0 * uv[counting] / torch.tensor([float(W), float(H)], dtype=torch.float64, device=view.device)
    c = torch.where(q >= 63.0, torch.full_like(q, 63.0), torch.where(q > 0.0, torch.floor(q), torch.zeros_like(q))).long()
    score = torch.zeros(V, dtype=torch.int64, device=view.device)
    for l in range(1, 7):
        side = 64 >> l
        ids = torch.unique((v * 64 + c[:, 0] // side) * 64 + c[:, 1] // side)
        score.index_add_(0, ids // 4096, torch.full_like(ids, 4 ** l))
    return score, num


def torch_update(track_of, first, view, uv, poses, intr, reg, X, valid, thr2, min_angle):
    """the rule of ls2fm_update_observations as torch ops; first: the offset of every observation's track"""
    T = valid.numel()
    P = poses[view]
    x = X[track_of]
    c = (P[:, :, :3] @ x[:, :, None])[:, :, 0] + P[:, :, 3]
    du = intr[0] * (c[:, 0] / c[:, 2]) + intr[2] - uv[:, 0]
    dv = intr[1] * (c[:, 1] / c[:, 2]) + intr[3] - uv[:, 1]
    keep = valid[track_of] & reg[view] & (c[:, 2] > 2.220446049250313e-16) & (du * du + dv * dv <= thr2)
    num = torch.zeros(T, dtype=torch.int64, device=view.device).index_add_(0, track_of, keep.long())
    # the rank of a kept observation inside its track, the first 64 into a padded [T, 64] table of views
    cs = torch.cumsum(keep.long(), 0)
    rank = cs - 1 - (cs - keep.long())[first]
    sel = keep & (rank < 64)
    m = int(min(64, int(num.max())))
    slot = torch.full((T, max(m, 1)), -1, dtype=torch.int64, device=view.device)
    slot[track_of[sel], rank[sel]] = view[sel]
    C = -(poses[:, :, :3].transpose(1, 2) @ poses[:, :, 3:])[:, :, 0]
    ray = X[:, None, :] - C[slot.clamp(min=0)]
    ray = ray / ray.norm(dim=-1, keepdim=True)
    ang = torch.zeros(T, dtype=torch.float64, device=view.device)
    for t0 in range(0, T, 16384):                                # [chunk, m, m] cosines
        r = ray[t0:t0 + 16384]
        a = torch.acos((r @ r.transpose(1, 2)).clamp(-1.0, 1.0))
        a = torch.minimum(a, np.pi - a)
        ok = (slot[t0:t0 + 16384] >= 0)
        a = torch.where(ok[:, :, None] & ok[:, None, :] & torch.isfinite(a), a, torch.zeros_like(a))
        ang[t0:t0 + 16384] = a.flatten(1).max(dim=1).values
    return keep, (num >= 2) & (ang >= min_angle), num, ang


class _Clock:
    """host clock per stage of _Mapper, each stage ended by a synchronise"""

    def __init__(self, mapper):
        self.ms = {}
        for name in ("initialise", "update", "triangulate_new", "adjust", "step"):
            setattr(mapper, name, self._wrap(name, getattr(mapper, name)))

    def _wrap(self, name, fn):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--kp", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50, help="calls per timed window")
    ap.add_argument("--ba-iters", type=int, default=1000)
    ap.add_argument("--no-reconstruct", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapper_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_mapper.py needs an MI355X: nothing is timed without one")
    dev = "cuda:0"
    scene = S.match_scene(31, n_views=a.views, n_kp=a.kp, n_points=int(a.kp * 1.5), arc_deg=360.0, n_conflicts=50, miss=0.6)
    image_start, edges = TR.edges_from_n_views(scene["tables"])
    poses = torch.as_tensor(scene["poses"]).to(dev)
    kp = torch.as_tensor(np.concatenate(scene["keypoints"])).to(dev)
    tracks = TR.build_tracks(image_start, torch.as_tensor(edges).to(dev))
    tri = TR.triangulate_tracks(tracks, kp, poses, S.INTR)
    uv, view = tri["obs_uv"], tracks["obs_view"].long()
    ts = tracks["track_start"].long()
    T, n_obs, V = ts.numel() - 1, view.numel(), a.views
    track_of = torch.bucketize(torch.arange(n_obs, device=dev), ts[1:], right=True)
    reg = torch.zeros(V, dtype=torch.bool, device=dev)
    reg[: V // 2] = True                                           # the middle of a run: half the views registered
    intr = torch.as_tensor(S.INTR, dtype=torch.float64, device=dev)
    valid, X = tri["success"], tri["X"]
    res = dict(views=V, keypoints_per_view=a.kp, tracks=T, observations=n_obs, valid_tracks=int(valid.sum()), registered=V // 2)

    up = M.update_observations(tracks, uv, poses, intr, reg, X, valid)
    want = torch_update(track_of, ts[:-1][track_of], view, uv, poses, intr, reg, X, valid, 16.0, np.radians(1.5))
    res["update_check"] = dict(obs_keep_differ=int((up["obs_keep"] != want[0]).sum()), track_valid_differ=int((up["track_valid"] != want[1]).sum()),
                               tri_angle_max_diff=float((up["tri_angle"] - want[3]).abs().max()))
    sc = M.view_scores(tracks, uv, up["obs_keep"], up["track_valid"], reg, (W, H))
    want = torch_scores(track_of, view, uv, up["obs_keep"], up["track_valid"], reg, V)
    res["score_check"] = dict(score_differ=int((sc[0] != want[0]).sum()), num_visible_differ=int((sc[1].long() != want[1]).sum()))
    size = torch.tensor([[float(W), float(H)]], dtype=torch.float64, device=dev).expand(V, 2).contiguous()
    first = ts[:-1][track_of]
    res["view_scores"], res["view_scores_torch"] = timed_pair(
        lambda: M.view_scores(tracks, uv, up["obs_keep"], up["track_valid"], reg, size, validate=False),
        lambda: torch_scores(track_of, view, uv, up["obs_keep"], up["track_valid"], reg, V), a.reps, a.batch)
    res["update_observations"], res["update_observations_torch"] = timed_pair(
        lambda: M.update_observations(tracks, uv, poses, intr, reg, X, valid, validate=False),
        lambda: torch_update(track_of, first, view, uv, poses, intr, reg, X, valid, 16.0, np.radians(1.5)), a.reps, a.batch)
    print(json.dumps(res, indent=1), flush=True)

    if not a.no_reconstruct:
        opt = M.MapperOptions(local_ba_iters=a.ba_iters, global_ba_iters=a.ba_iters, **S.ba_rates())
        walls = []
        for _ in range(3):                                       # the first run is the warm-up and is reported apart
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = M.reconstruct(scene["tables"], S.K, H, W, opt, device=dev)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        res["reconstruct"] = dict(first_run_ms=walls[0], wall_ms=statistics.median(walls[1:]), warm_runs_ms=walls[1:], registered=int(rec.registered.sum()), valid_points=int(rec.track_valid.sum()),
                                  ba_iters=a.ba_iters, last_ba_error_px=rec.log[-1]["ba_error"] if rec.log else None)
        m = M._Mapper(scene["tables"], S.K, H, W, opt, dev)
        clock = _Clock(m)
        with torch.cuda.device(m.dev):
            m.initialise()
            m.update()
            m.triangulate_new()
            m.adjust(None, True)
            m.update()
            before = dict(clock.ms)
            n = 0
            while len(m.order) < m.V:
                n += 1
                if not m.step(n):
                    break
        stages = dict(clock.ms)
        # a step contains its update / triangulate / adjust calls: what is left is scoring, ranking, absolute pose and refinement
        stages["step_scoring_and_pose"] = stages.pop("step") - sum(stages[k] - before[k] for k in ("update", "triangulate_new", "adjust"))
        res["reconstruct"]["stages_ms"] = stages
        res["reconstruct"]["steps"] = n
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
