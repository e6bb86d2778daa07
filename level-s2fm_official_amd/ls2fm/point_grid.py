"""The point grid: exact nearest neighbours of a cloud over a uniform grid (ls2fm_point_grid_*, csrc/point_grid.hip) -- PointGrid
with query (the nearest), knn (the k nearest) and c_args (the grid as the C entry points take it), the same rule as plain torch ops
(nearest_neighbors_bruteforce) and the argument checks its users share (ls2fm.metrics, whose prefix the messages keep and which
re-exports all of it, ls2fm.cloud, ls2fm.cloud_mesh).

The distance rule (include/ls2fm.h): dx = q.x - r.x, dy, dz likewise, d2 = (dx dx + dy dy) + dz dz, every operation one rounded
fp32 operation; a reference qualifies when d2 <= max_d2 and d2 < +inf; the smallest d2 wins, among equal d2 the lowest index.  The
result is a pure function of the two clouds: no grid, batch or visiting order shows in it, and tests/metrics_restate.py holds it bit
for bit.  There is no CPU path for the grid: CPU tensors, a missing device or a missing library raise.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

# The automatic cell size (auto_cell_size): "surface" sizes the cells for points on a surface, "volume" for points filling the box.
# Chosen by tools/time_metrics.py on 2 M x 2 M points of a sphere surface (profiles/metrics_time.json).
AUTO_CELL_RULE = "surface"
KNN_MAX_K = 32                            # the largest list capacity ls2fm_point_grid_knn instantiates
require_device = functools.partial(_lib.require_device_tensors, "ls2fm.metrics", phrase=": the point grid runs on MI355X only",
                                   more=" -- nearest_neighbors_bruteforce is the explicit torch form")


def points3(x, name):
    x = torch.as_tensor(x)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"ls2fm.metrics: {name} must be [n, 3], got shape {tuple(x.shape)}")
    return x


def squared_cutoff(max_dist):
    """max_d2 = float32(max_dist) * float32(max_dist) as a numpy float32; +inf for None"""
    if max_dist is None:
        return np.float32(np.inf)
    m = np.float32(max_dist)
    if not m >= 0:
        raise ValueError(f"ls2fm.metrics: max_dist {max_dist} must be >= 0 (None: no cut-off)")
    with np.errstate(over="ignore"):
        return np.float32(m * m)


def knn_k(k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError(f"ls2fm.metrics: k {k} must be an integer in [1, {KNN_MAX_K}]")
    return int(k)


def cell_dims(extent32, inv_h):
    """cells per axis that hold every reference: floor((max - origin) * inv_h) + 1 in the device's fp32 arithmetic (float64 [3])"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor((extent32 * inv_h).astype(np.float32)).astype(np.float64) + 1.0


def auto_cell_size(lo, hi, n, max_cells=2 ** 25, rule=None):
    """The automatic cell size of a cloud of n points inside the box [lo, hi] (host numbers).  Over the axes of non-zero extent e:
      "surface"  three axes: sqrt(2 (ex ey + ey ez + ez ex) / n), about one point per cell that a surface through the box crosses;
                 two axes: sqrt(e1 e2 / n); one axis: e1 / n
      "volume"   (product of e / n) ^ (1 / axes): one point per cell of the box
    a cloud without extent gets 1.  The size is then grown by 5 % at a time until the grid has at most max_cells cells, so it is
    always positive and finite."""
    rule = AUTO_CELL_RULE if rule is None else rule
    if rule not in ("surface", "volume"):
        raise ValueError(f"ls2fm.metrics.auto_cell_size: rule {rule!r} is neither 'surface' nor 'volume'")
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    extent32 = (hi32 - lo32).astype(np.float32)
    e = [float(v) for v in extent32 if v > 0]
    n = max(int(n), 1)
    if not e:
        h = 1.0
    elif rule == "volume" or len(e) < 3:
        h = (math.prod(e) / n) ** (1.0 / len(e))
    else:
        h = math.sqrt(2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]) / n)
    h = max(h, max(e, default=1.0) * 2.0 ** -20, float(np.finfo(np.float32).tiny) * 2.0 ** 24)
    while True:
        h32 = np.float32(h)
        if np.isfinite(h32) and h32 > 0 and float(np.prod(cell_dims(extent32, np.float32(1) / h32))) <= max_cells:
            return float(h32)
        h *= 1.05


class PointGrid:
    """A uniform grid over the reference cloud `ref` (float32 [N, 3] on the device, finite) for exact nearest-neighbour queries.
    origin is the per-axis minimum; `cell_size` is honoured exactly (ValueError if the grid would have more than `max_cells`
    cells), None takes auto_cell_size.  Building reads the bounding box on the host once; cell_start int32 [cells + 1], sorted_xyz
    float32 [N, 3] and sorted_index int32 [N] (views of one [N, 4] array) are the grid."""

    def __init__(self, ref, cell_size=None, max_cells=2 ** 25):
        ref = points3(ref, "ref")
        require_device(ref)
        lib = _lib.load()
        self.ref = _lib.cf(ref)
        self.n = int(self.ref.shape[0])
        self.device = dev = self.ref.device
        if self.n >= 1 << 31:
            raise ValueError(f"ls2fm.metrics.PointGrid: {self.n} points, 2^31 or more")
        if self.n:
            box = torch.stack([self.ref.amin(dim=0), self.ref.amax(dim=0)]).cpu().numpy()          # the one host read
            if not np.isfinite(box).all():
                raise ValueError("ls2fm.metrics.PointGrid: the reference cloud holds a NaN or infinite coordinate")
        else:
            box = np.zeros((2, 3), np.float32)
        lo, hi = box[0].astype(np.float32), box[1].astype(np.float32)
        if cell_size is None:
            h = np.float32(auto_cell_size(lo, hi, self.n, max_cells))
        else:
            h = np.float32(cell_size)
            if not (np.isfinite(h) and h > 0):
                raise ValueError(f"ls2fm.metrics.PointGrid: cell_size {cell_size} must be positive and finite")
        with np.errstate(over="ignore"):
            inv_h = np.float32(1) / h
        if not (np.isfinite(inv_h) and inv_h > 0):
            raise ValueError(f"ls2fm.metrics.PointGrid: cell_size {cell_size} has no finite fp32 reciprocal")
        dims = cell_dims((hi - lo).astype(np.float32), inv_h)
        cells = float(np.prod(dims))
        if not np.isfinite(cells) or cells > max_cells or cells >= 2 ** 31 - 1:
            raise ValueError(f"ls2fm.metrics.PointGrid: cell_size {float(h)} gives {dims.astype(np.int64).tolist()} cells, "
                             f"more than max_cells = {max_cells}")
        self.origin, self.cell_size, self.inv_cell_size = lo, float(h), float(inv_h)
        self.box_max = hi
        self.dim = tuple(int(d) for d in dims)
        self.n_cells = int(cells)
        self._origin = (ctypes.c_float * 3)(*[float(v) for v in lo])
        self._dim = (ctypes.c_int32 * 3)(*self.dim)
        with torch.cuda.device(dev):
            self.cell_start = torch.empty(self.n_cells + 1, dtype=torch.int32, device=dev)
            self.sorted = torch.empty(self.n, 4, dtype=torch.float32, device=dev)
            ws = _lib.workspace(lib.ls2fm_point_grid_workspace_bytes(self.n, self.n_cells), "ls2fm_point_grid_workspace_bytes", dev)
            check(lib.ls2fm_point_grid_build(ptr(self.ref), self.n, self._origin, self.cell_size, self.inv_cell_size, self._dim,
                                             ptr(self.cell_start), ptr(self.sorted), ptr(ws), stream_ptr()), "ls2fm_point_grid_build")
        self.sorted_xyz = self.sorted[:, :3]
        self.sorted_index = self.sorted.view(torch.int32)[:, 3]

    def c_args(self, n_first=False):
        """the grid in the C argument order (_lib._GRID); n_first: n ahead of sorted, as ls2fm_cloud_implicit and its _plan take it"""
        head = (ptr(self.sorted), ptr(self.cell_start), self.n)
        return (head[2:] + head[:2] if n_first else head) + (self._origin, self.cell_size, self.inv_cell_size, self._dim)

    def cell_order(self, q):
        """a permutation that walks the queries cell by cell (any order gives the same results: this one is for the caches)"""
        o = torch.as_tensor(self.origin, device=q.device)
        c = ((torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0) - o) * self.inv_cell_size).floor()
        c = torch.minimum(c.clamp_(min=0), torch.tensor([d - 1 for d in self.dim], dtype=torch.float32, device=q.device)).long()
        return torch.argsort((c[:, 2] * self.dim[1] + c[:, 1]) * self.dim[0] + c[:, 0])

    def _queries(self, q, who):
        q = points3(q, "q")
        require_device(q)
        if q.device != self.device:
            raise ValueError(f"ls2fm.metrics.PointGrid.{who}: queries on {q.device}, the grid on {self.device}")
        return _lib.cf(q)

    def _walk(self, symbol, q, sort, options, results):
        """One launch of symbol(q, M, *c_args(), *options, *results, stream), the shape of both query entry points; with `sort` (and no
        stream capturing) in the order of the queries' cells, the results put back.  results: (trailing shape, dtype) of each [M, ...]"""
        m = int(q.shape[0])
        with torch.cuda.device(self.device):
            perm = self.cell_order(q) if sort and m > 1 and self.n and not torch.cuda.is_current_stream_capturing() else None
            q, out = q if perm is None else q[perm], [torch.empty((m,) + shape, dtype=dtype, device=self.device) for shape, dtype in results]
            check(getattr(_lib.load(), symbol)(ptr(q), m, *self.c_args(), *options, *(ptr(x) for x in out), stream_ptr()), symbol)
            return tuple(out if perm is None else [torch.empty_like(x).index_copy_(0, perm, x) for x in out])

    def query(self, q, max_dist=None, sort=None):
        """(idx int32 [M], d2 float32 [M]) of the queries `q` (float32 [M, 3] on the grid's device): the index into `ref` of each
        query's nearest reference by the distance rule and its fp32 squared distance; -1 and +inf where no reference lies within
        `max_dist` (d2 <= float32(max_dist)^2; None: no cut-off) and for a NaN or infinite query.  Reads nothing back, so it can
        be captured into a graph.  The queries are walked in the order of their cells and the results put back (measured faster by the
        same tool; a torch sort, so not while a stream captures); sort=False walks them as given.  No result depends on it."""
        q = self._queries(q, "query")
        return self._walk("ls2fm_point_grid_query", q, sort is None or sort, (float(squared_cutoff(max_dist)),),
                          (((), torch.int32), ((), torch.float32)))

    def knn(self, q, k, max_dist=None, skip_own=False, sort=None):
        """(idx int32 [M, k], d2 float32 [M, k], count int32 [M]) of the queries `q`: each query's qualifying references ordered by
        (d2, index), the first k of them (1 <= k <= KNN_MAX_K; the K-NEIGHBOUR RULE of include/ls2fm.h), -1 / +inf in the slots
        without one and the number of filled slots.  skip_own: query t ignores reference t -- `q` must be the grid's own cloud
        in its order (M == N is checked, the rest is the caller's promise); a duplicate at another index stays a neighbour.
        One launch (ls2fm_point_grid_knn), nothing read back; the cell-order walk, its put-back and `sort` are `query`'s."""
        q, k, max_d2 = self._queries(q, "knn"), knn_k(k), float(squared_cutoff(max_dist))
        if skip_own and q.shape[0] != self.n:
            raise ValueError(f"ls2fm.metrics.PointGrid.knn: skip_own needs the grid's own cloud as queries, got {q.shape[0]} queries for {self.n} points")
        # skip_own identifies a query by its position: those are walked as given
        return self._walk("ls2fm_point_grid_knn", q, (sort is None or sort) and not skip_own, (k, max_d2, 1 if skip_own else 0),
                          (((k,), torch.int32), ((k,), torch.float32), ((), torch.int32)))


def nearest_neighbors(q, ref, max_dist=None, cell_size=None):
    """PointGrid(ref, cell_size).query(q, max_dist) in one call: (idx int32 [M], d2 float32 [M])"""
    q, ref = points3(q, "q"), points3(ref, "ref")
    require_device(q, ref)
    return PointGrid(ref, cell_size=cell_size).query(q, max_dist)


def nearest_neighbors_bruteforce(q, ref, max_dist=None, chunk=None):
    """The distance rule as plain torch ops, on whatever device the clouds are on: all M x N distances, `chunk` queries at a time
    (default: 2^24 distances per chunk).  The column differences, the three products and the two sums are separate torch ops in
    the stated order, so each rounds once; the minimum is taken first and the lowest index among the entries that equal it second
    (torch.argmin does not promise the first).  -> (idx int32 [M], d2 float32 [M]).  The timing baseline of the grid and the CPU
    route of the host tests; nothing in the library falls back to it."""
    q, ref = points3(q, "q").float(), points3(ref, "ref").float()
    dev = q.device
    ref = ref.to(dev)
    m, n = int(q.shape[0]), int(ref.shape[0])
    max_d2 = float(squared_cutoff(max_dist))
    idx = torch.full((m,), -1, dtype=torch.int32, device=dev)
    d2_out = torch.full((m,), float("inf"), dtype=torch.float32, device=dev)
    if m == 0 or n == 0:
        return idx, d2_out
    chunk = max(1, (1 << 24) // n) if chunk is None else max(1, int(chunk))
    rx, ry, rz = ref[:, 0][None, :], ref[:, 1][None, :], ref[:, 2][None, :]
    index = torch.arange(n, device=dev)[None, :]
    big = torch.iinfo(torch.int64).max
    for s in range(0, m, chunk):
        c = q[s:s + chunk]
        dx, dy, dz = c[:, 0:1] - rx, c[:, 1:2] - ry, c[:, 2:3] - rz
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = (d2 <= max_d2) & (d2 < float("inf"))
        d2 = torch.where(ok, d2, torch.full_like(d2, float("inf")))
        mn = d2.amin(dim=1)
        first = torch.where((d2 == mn[:, None]) & ok, index, torch.full_like(index, big)).amin(dim=1)
        idx[s:s + chunk] = torch.where(mn < float("inf"), first, torch.full_like(first, -1)).to(torch.int32)
        d2_out[s:s + chunk] = mn
    return idx, d2_out
