#!/usr/bin/env python
"""Times ls2fm.tracks on a 49-view x 8192-key-point scene of tests/tracks_scenes.py (HIP events on the stream, warm, median of
repeated calls) and writes profiles/tracks_time.json:
  batched     one build_tracks + one triangulate_tracks call
  before      what a user had before: the restatement's union-find on the host plus one ls2fm.pose.triangulate call per view pair
  per_1000    triangulate_tracks as one call per 1000 tracks
    python tools/time_tracks.py [--views 49] [--kp 8192] [--reps 7]"""
import argparse, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "level-s2fm_official_amd"), ROOT):
    sys.path.insert(0, p)
import tracks_restate as R          # noqa: E402
import tracks_scenes as S           # noqa: E402
from ls2fm import pose, tracks as TR  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--kp", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_time.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    scene = S.match_scene(31, n_views=a.views, n_kp=a.kp, n_points=int(a.kp * 1.5), arc_deg=360.0, n_conflicts=50, miss=0.6)
    image_start, edges = TR.edges_from_n_views(scene["tables"])
    e = torch.as_tensor(edges).to(dev)
    poses = torch.as_tensor(scene["poses"]).to(dev)
    kp = torch.as_tensor(np.concatenate(scene["keypoints"])).to(dev)
    tracks = TR.build_tracks(image_start, e)
    tri = TR.triangulate_tracks(tracks, kp, poses, S.INTR)
    lengths = (tracks["track_start"][1:] - tracks["track_start"][:-1]).cpu().numpy()
    res = dict(views=a.views, keypoints_per_view=a.kp, edges=int(len(edges)), tracks=int(len(lengths)), observations=int(lengths.sum()),
               conflicts=tracks["n_conflicts"], track_length_mean=float(lengths.mean()), track_length_max=int(lengths.max()),
               successful=int(tri["success"].sum()))
    res["build_tracks"] = timed(lambda: TR.build_tracks(image_start, e), a.reps)
    res["triangulate_tracks"] = timed(lambda: TR.triangulate_tracks(tracks, kp, poses, S.INTR, validate=False), a.reps)
    res["batched"] = timed(lambda: TR.triangulate_tracks(TR.build_tracks(image_start, e), kp, poses, S.INTR, validate=False), a.reps)

    ts = tracks["track_start"].cpu().numpy()
    view, uv = tracks["obs_view"], tri["obs_uv"]
    chunks = []
    for t0 in range(0, len(lengths), 1000):
        t1 = min(t0 + 1000, len(lengths))
        s, en = int(ts[t0]), int(ts[t1])
        chunks.append(dict(track_start=(tracks["track_start"][t0:t1 + 1] - s).contiguous(), obs_view=view[s:en].contiguous(), uv=uv[s:en].contiguous()))

    def per_1000():
        for c in chunks:
            TR.triangulate_tracks(c, None, poses, S.INTR, obs_uv=c["uv"], validate=False)
    res["per_1000"] = timed(per_1000, a.reps)

    # before: host union-find (timed with the host clock) + one two-view DLT call per view pair over that pair's matches
    t0 = time.perf_counter()
    R.track_labels(image_start, edges)
    res["host_union_find_ms"] = (time.perf_counter() - t0) * 1e3
    Kmat = torch.as_tensor(S.K).to(dev)
    pairs = []
    for v, t in enumerate(scene["tables"]):
        for j in range(v + 1, a.views):
            idx = np.asarray(t["indxes"][j - 1]).reshape(-1, 2).astype(np.int64)[np.asarray(t["mask"][j - 1]).astype(bool)]
            if len(idx):
                pairs.append((Kmat @ poses[v], Kmat @ poses[j], kp[int(image_start[v]) + torch.as_tensor(idx[:, 0]).to(dev)],
                              kp[int(image_start[j]) + torch.as_tensor(idx[:, 1]).to(dev)]))

    def per_pair():
        for P0, P1, a0, a1 in pairs:
            pose.triangulate(P0, P1, a0, a1)
    res["per_pair_triangulate"] = timed(per_pair, max(3, a.reps // 2))
    res["pairs"] = len(pairs)
    res["before_ms"] = res["host_union_find_ms"] + res["per_pair_triangulate"]["median_ms"]
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
