"""Feature tracks and multi-view triangulation on the device: the step between ls2fm.match.two_view_tables and
ls2fm.stage.TradBALoop that the reference keeps in Python bookkeeping -- Point3DSet.add_point3d one point at a time and
Camera.idx2d_to_3d filled pair by pair from cv2.triangulatePoints (pipelines/Registration_Trad.py:183-215,
Initialization_Trad.py:97), every point from exactly two views and whichever pair arrives first claiming a key point.

`edges_from_n_views` turns the tables' inlier matches into the edges of the match graph (host), `build_tracks` labels its connected
components with ls2fm_track_labels (csrc/tracks.hip) and keeps the components with at most one key point per image,
`triangulate_tracks` runs ls2fm_triangulate_tracks -- hypotheses over the pairs of a track's first 64 observations, exact integer
scoring over all of them, a local optimisation on the inliers' normal matrix -- and `to_tracked_views` makes the result a
`TrackedViews`, the input of `TradBALoop`.  `visible_points` counts, per view, the triangulated points a candidate view would see.
Every rule is stated in include/ls2fm.h; tests/tracks_restate.py repeats them in numpy.

There is no CPU path for the two device calls: CPU tensors, a missing device or a missing library raise.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

HYP_OBS = 64                # LS2FM_TRACK_HYP_OBS
MAX_OBS = 4096              # LS2FM_TRACK_MAX_OBS
_EDGE_STATUS = {1: "an edge names a node outside [0, n_nodes)", 2: "both ends of an edge lie in one image"}
_TRACK_STATUS = {1: f"track_start does not rise inside [0, n_obs] or a track has more than {MAX_OBS} observations",
                 2: "an obs_view outside [0, n_views)"}


_device = functools.partial(_lib.require_device_tensors, "ls2fm.tracks")


def edges_from_n_views(n_views):
    """The match graph of the `n_views.npy` tables (ls2fm.match.two_view_tables / assemble_n_views; pure host function): for every
    pair v < j the rows of view v's `indxes` entry for j that its `mask` keeps.  -> (image_start int32 numpy [V + 1], edges int32
    numpy [E, 2] of node ids image_start[view] + key point).  The edges of a pair are read from the lower view's entry; the higher
    view's copy must hold the same rows with the columns swapped and the same mask, or the table is refused."""
    counts = [len(t["kypts"]) for t in n_views]
    image_start = np.zeros(len(n_views) + 1, dtype=np.int64)
    image_start[1:] = np.cumsum(counts)
    if image_start[-1] >= 1 << 31:
        raise ValueError(f"ls2fm.tracks.edges_from_n_views: {image_start[-1]} key points, 2^31 or more")
    edges = []
    for v, t in enumerate(n_views):
        if len(t["indxes"]) != len(n_views) - 1 or len(t["mask"]) != len(n_views) - 1:
            raise ValueError(f"ls2fm.tracks.edges_from_n_views: view {v} has {len(t['indxes'])} entries for {len(n_views) - 1} other views")
    for v, t in enumerate(n_views):
        for j in range(v + 1, len(n_views)):
            idx = np.asarray(t["indxes"][j - 1])              # the other views in increasing index, v itself left out
            mask = np.asarray(t["mask"][j - 1]).reshape(-1).astype(bool)
            if idx.size == 0:
                if np.asarray(n_views[j]["indxes"][v]).size:
                    raise ValueError(f"ls2fm.tracks.edges_from_n_views: the two copies of pair ({v}, {j}) disagree")
                continue
            idx = idx.reshape(-1, 2).astype(np.int64)
            if len(mask) != len(idx):
                raise ValueError(f"ls2fm.tracks.edges_from_n_views: pair ({v}, {j}) has a mask of {len(mask)} for {len(idx)} matches")
            # the higher view's copy of the pair: the same rows, columns swapped (its entry for v is at index v, since v < j)
            twin = np.asarray(n_views[j]["indxes"][v])
            twin_mask = np.asarray(n_views[j]["mask"][v]).reshape(-1).astype(bool)
            if twin.size != idx.size or not np.array_equal(twin.reshape(-1, 2).astype(np.int64)[:, ::-1], idx) \
                    or not np.array_equal(twin_mask, mask):
                raise ValueError(f"ls2fm.tracks.edges_from_n_views: the two copies of pair ({v}, {j}) disagree")
            idx = idx[mask]
            if len(idx) and (idx[:, 0].max() >= counts[v] or idx[:, 1].max() >= counts[j]):
                raise ValueError(f"ls2fm.tracks.edges_from_n_views: pair ({v}, {j}) names a key point its view does not have")
            edges.append(np.stack([image_start[v] + idx[:, 0], image_start[j] + idx[:, 1]], axis=1))
    edges = np.concatenate(edges) if edges else np.zeros((0, 2), dtype=np.int64)
    return image_start.astype(np.int32), edges.astype(np.int32).reshape(-1, 2)


def _image_start(image_start):
    h = np.asarray(image_start.cpu() if torch.is_tensor(image_start) else image_start).reshape(-1).astype(np.int64)
    if h.size < 2 or h[0] != 0 or (np.diff(h) < 0).any():
        raise ValueError("ls2fm.tracks: image_start must rise from 0, one entry more than there are images")
    if h[-1] >= 1 << 31:
        raise ValueError(f"ls2fm.tracks: {h[-1]} key points, 2^31 or more")
    return h


def track_labels(image_start, edges, return_status=False):
    """labels int32 [n_nodes] on the edges' device: the smallest node id of each node's connected component (ls2fm_track_labels).
    image_start: [V + 1] (host or device; read on the host), edges: int [E, 2] on the device.  A bad edge (outside [0, n_nodes), or
    inside one image) is found on the device and raises ValueError after the call; return_status=True returns (labels, status
    int32 [1] on the device) instead and reads nothing back."""
    h = _image_start(image_start)
    edges = torch.as_tensor(edges)
    _device(edges)
    if edges.numel() and (edges.dim() != 2 or edges.shape[1] != 2):
        raise ValueError(f"ls2fm.tracks: edges must be [E, 2], got shape {tuple(edges.shape)}")
    e = edges.reshape(-1, 2)
    if e.dtype != torch.int32:
        # an id that int32 cannot hold must not wrap into range: it becomes -1, which the device check reports
        e = e.long()
        e = torch.where((e < 0) | (e >= 1 << 31), torch.full_like(e, -1), e).to(torch.int32)
    e = e.contiguous()
    if e.shape[0] >= 1 << 31:
        raise ValueError(f"ls2fm.tracks: {e.shape[0]} edges, 2^31 or more")
    dev = e.device
    n_nodes = int(h[-1])
    with torch.cuda.device(dev):
        start = torch.as_tensor(h, dtype=torch.int32).to(dev)
        labels = torch.empty(n_nodes, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(_lib.load().ls2fm_track_labels(ptr(start), len(h) - 1, n_nodes, ptr(e), e.shape[0], ptr(labels), ptr(status), stream_ptr()),
              "ls2fm_track_labels")
    if return_status:
        return labels, status
    _lib.raise_status(status, "ls2fm.tracks.track_labels", _EDGE_STATUS)
    return labels


def build_tracks(image_start, edges):
    """The track table of a match graph.  image_start [V + 1]; edges int [E, 2] node pairs on the device, in any order.
    -> dict(track_start int32 [T + 1], obs_node int32 [n_obs], obs_view int32 [n_obs], n_conflicts int, labels int32 [n_nodes],
    image_start int32 [V + 1]; all tensors on the device).  A track is a connected component of >= 2 key points with at most one
    per image; a component with two key points of one image is a conflict and is dropped whole (the OpenMVG / hloc rule; COLMAP's
    correspondence graph keeps such components and lets the triangulator split them).  Tracks in rising label (their smallest
    node), observations inside a track in rising node id, so in rising view.  The labels are one device call; the table is a
    stable sort and segment offsets on the device, with one host read for the sizes."""
    labels = track_labels(image_start, edges)
    dev = labels.device
    with torch.cuda.device(dev):
        start = torch.as_tensor(_image_start(image_start), dtype=torch.int64).to(dev)
        n_nodes = labels.numel()
        node = torch.arange(n_nodes, device=dev)
        view = torch.bucketize(node, start[1:], right=True)
        # labels are node ids and a node's label is <= the node: sorting by label (stable) keeps every component's nodes in rising id
        lab, order = torch.sort(labels.long(), stable=True)
        size = torch.zeros(n_nodes, dtype=torch.int64, device=dev).index_add_(0, lab, torch.ones_like(lab))
        v_sorted = view[order]
        same = (lab[1:] == lab[:-1]) & (v_sorted[1:] == v_sorted[:-1])         # neighbours of one component in one image
        clash = torch.zeros(n_nodes, dtype=torch.int64, device=dev).index_add_(0, lab[1:], same.long())
        keep_comp = (size >= 2) & (clash == 0)
        keep = keep_comp[lab]
        obs_node = order[keep]
        obs_view = v_sorted[keep]
        sizes = size[keep_comp]
        track_start = torch.zeros(sizes.numel() + 1, dtype=torch.int64, device=dev)
        track_start[1:] = torch.cumsum(sizes, 0)
        n_conflicts = int(((size >= 2) & (clash > 0)).sum())
    return dict(track_start=track_start.to(torch.int32), obs_node=obs_node.to(torch.int32), obs_view=obs_view.to(torch.int32),
                n_conflicts=n_conflicts, labels=labels, image_start=start.to(torch.int32))


def _observations(tracks, keypoints):
    """obs_uv fp64 [n_obs, 2] from per-view key points (list of [n_v, 2] -- or [n_v, 4] as ls2fm.features.extract returns them, of which
    x, y are read -- or one [n_nodes, 2] tensor in node order)"""
    dev = tracks["obs_node"].device
    def xy(k):
        k = torch.as_tensor(k)
        if k.dim() != 2 or k.shape[1] < 2:
            raise ValueError(f"ls2fm.tracks: key points must be [n, 2] (or [n, 4] = x, y, scale, orientation), got {tuple(k.shape)}")
        return k[:, :2].to(device=dev, dtype=torch.float64)

    kp = torch.cat([xy(k) for k in keypoints]) if isinstance(keypoints, (list, tuple)) else xy(keypoints)
    n_nodes = int(tracks["image_start"][-1]) if "image_start" in tracks else kp.shape[0]
    if kp.shape[0] != n_nodes:
        raise ValueError(f"ls2fm.tracks: {kp.shape[0]} key points for {n_nodes} nodes")
    return kp[tracks["obs_node"].long()].contiguous()


def triangulate_tracks(tracks, keypoints, poses, intrinsics, max_error_px=4.0, min_tri_angle_deg=1.5, obs_uv=None, validate=True):
    """One robust N-view triangulation per track (ls2fm_triangulate_tracks; the rules are in include/ls2fm.h).  tracks: the dict
    of build_tracks (track_start, obs_view, obs_node); keypoints: list over views of [n_v, 2] pixels, or [n_nodes, 2] (or None with
    obs_uv [n_obs, 2] given); poses [V, 3, 4] world-to-camera; intrinsics as ls2fm.pose takes them ((fx, fy, cx, cy) [V, 4] / [4] or
    K).  max_error_px is COLMAP's filter_max_reproj_error, min_tri_angle_deg its filter_min_tri_angle.
    -> dict(X fp64 [T, 3] (zero without success), inliers bool [n_obs], num_inliers int32 [T], success bool [T], tri_angle fp64 [T]
    (radians), mean_error_px fp64 [T], best_pair int32 [T], status int32 [1]).
    The device call reads nothing back and can be captured into a graph; validate=True (ignored while a stream is capturing) reads
    the call's status word afterwards and raises ValueError for a malformed table."""
    from .pose import _intrinsics
    if not (np.isfinite(max_error_px) and max_error_px > 0):
        raise ValueError(f"ls2fm.tracks.triangulate_tracks: max_error_px {max_error_px} must be positive and finite")
    if not 0.0 <= min_tri_angle_deg <= 90.0:
        raise ValueError(f"ls2fm.tracks.triangulate_tracks: min_tri_angle_deg {min_tri_angle_deg} outside [0, 90]")
    ts, view = tracks["track_start"], tracks["obs_view"]
    _device(ts, view)
    dev = ts.device
    p = torch.as_tensor(poses)
    _device(p)
    if p.dim() != 3 or tuple(p.shape[1:]) != (3, 4):
        raise ValueError(f"ls2fm.tracks.triangulate_tracks: poses must be [V, 3, 4], got {tuple(p.shape)}")
    p = p.to(device=dev, dtype=torch.float64).contiguous()
    V = p.shape[0]
    intr = _intrinsics(intrinsics, V, dev)
    uv = _observations(tracks, keypoints) if obs_uv is None else torch.as_tensor(obs_uv).to(device=dev, dtype=torch.float64).reshape(-1, 2).contiguous()
    ts = ts.to(torch.int32).contiguous()
    view = view.to(torch.int32).contiguous()
    T, n_obs = ts.numel() - 1, view.numel()
    if T < 0 or uv.shape[0] != n_obs:
        raise ValueError(f"ls2fm.tracks.triangulate_tracks: {uv.shape[0]} pixel rows for {n_obs} observations of {T} tracks")
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.ls2fm_triangulate_tracks_workspace_bytes(T, V), "ls2fm_triangulate_tracks_workspace_bytes", dev)
        X = torch.empty(T, 3, dtype=torch.float64, device=dev)
        inl = torch.empty(n_obs, dtype=torch.uint8, device=dev)
        num, succ, best = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
        ang, err = (torch.empty(T, dtype=torch.float64, device=dev) for _ in range(2))
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.ls2fm_triangulate_tracks(ptr(p), ptr(intr), V, ptr(ts), T, ptr(view), ptr(uv), n_obs, float(max_error_px),
                                           float(min_tri_angle_deg), ptr(X), ptr(inl), ptr(num), ptr(succ), ptr(ang), ptr(err), ptr(best),
                                           ptr(status), ptr(ws), stream_ptr()), "ls2fm_triangulate_tracks")
        if validate and not torch.cuda.is_current_stream_capturing():
            _lib.raise_status(status, "ls2fm.tracks.triangulate_tracks", _TRACK_STATUS)
    return dict(X=X, inliers=inl.view(torch.bool), num_inliers=num, success=succ.bool(), tri_angle=ang, mean_error_px=err,
                best_pair=best, status=status, obs_uv=uv)


def _kept(tracks, tri):
    """(bool [n_obs]: the inlier observations of successful tracks, long [n_obs]: the track of every observation)"""
    ts = tracks["track_start"].long()
    n_obs = tracks["obs_view"].numel()
    track_of = torch.bucketize(torch.arange(n_obs, device=ts.device), ts[1:], right=True)
    if n_obs == 0:
        return torch.zeros(0, dtype=torch.bool, device=ts.device), track_of
    return tri["inliers"] & tri["success"][track_of], track_of


def to_tracked_views(tracks, tri, keypoints, poses, intrinsic, images=None, H=None, W=None):
    """ls2fm.stage.TrackedViews of the successful tracks' inlier observations: per view the key points that observe a triangulated
    point and that point's index, the points renumbered 0 .. M - 1 in track order (xyzs fp32 [M, 3]) -- directly a `TradBALoop`
    input.  poses [V, 3, 4] (or se(3) [V, 6]), intrinsic K [3, 3]; images [V, H*W, 3] or None (the classical loop does not read
    them: an empty placeholder is stored); H, W: the image size.  The tensors follow the tracks' device (CPU tables give a CPU
    container for the torch path of the loop)."""
    from .stage import TrackedViews
    if H is None or W is None:
        raise ValueError("ls2fm.tracks.to_tracked_views: H and W are needed")
    dev = tracks["obs_view"].device
    keep, track_of = _kept(tracks, tri)
    new_id = torch.cumsum(tri["success"].long(), 0) - 1                           # successful tracks in order
    xyzs = tri["X"][tri["success"]].float()
    uv = tri["obs_uv"] if "obs_uv" in tri else _observations(tracks, keypoints)
    view = tracks["obs_view"].long()
    V = torch.as_tensor(poses).shape[0]
    kps, ids = [], []
    for v in range(V):
        sel = keep & (view == v)
        kps.append(uv[sel].float())
        ids.append(new_id[track_of[sel]])
    if any(k.shape[0] == 0 for k in kps):
        raise ValueError("ls2fm.tracks.to_tracked_views: a view observes no triangulated point; drop it before building the container")
    if images is None:
        images = torch.zeros(V, 0, 3, device=dev)
    return TrackedViews(torch.as_tensor(poses).to(dev), torch.as_tensor(intrinsic).to(dev).float(), images, kps, ids, xyzs, H, W)


def visible_points(tracks, tri, registered):
    """What a next-best-view rule reads: int64 [V], per view the number of its key points that lie in a successful track with an
    inlier in a registered view; 0 for the registered views themselves.  registered: bool [V] or a list of view indices.  One
    scatter over the observations."""
    view = tracks["obs_view"].long()
    dev = view.device
    V = int(tracks["image_start"].numel() - 1) if "image_start" in tracks else int(view.max()) + 1
    reg = torch.as_tensor(registered, device=dev)
    if reg.dtype != torch.bool:
        reg = torch.zeros(V, dtype=torch.bool, device=dev).index_fill_(0, reg.long().reshape(-1), True)
    if reg.numel() != V:
        raise ValueError(f"ls2fm.tracks.visible_points: {reg.numel()} flags for {V} views")
    keep, track_of = _kept(tracks, tri)
    T = tracks["track_start"].numel() - 1
    seen = torch.zeros(T, dtype=torch.int64, device=dev).index_add_(0, track_of, (keep & reg[view]).long()) > 0
    counted = seen[track_of] & tri["success"][track_of] & ~reg[view]
    return torch.zeros(V, dtype=torch.int64, device=dev).index_add_(0, view, counted.long())
