"""Plane-sweep multi-view stereo on the device: from posed photographs to depth maps, and through ls2fm.fusion to a surface.

  to_grey, select_sources, depth_range_from_points, depth_planes, relative_poses   the inputs of the sweep, as torch ops
  plane_sweep     per reference view the depth, score and plane of every pixel (ls2fm_mvs_sweep, csrc/mvs_sweep.hip): normalised
                  cross-correlation of a (2 w + 1)^2 window against S source views over D fronto-parallel planes
  filter_depths   the geometric-consistency filter of a set of depth maps (ls2fm_mvs_filter): a pixel stays when enough source
                  views hold a depth that projects back onto it
  plane_score, patch_match_step   PatchMatch stereo with slanted planes (ls2fm_mvs_plane_score, ls2fm_mvs_patchmatch_step,
                  csrc/mvs_patchmatch.hip): the NCC of a per-pixel plane (depth, normal), and one red-black half-sweep of
                  propagation and random refinement, in place on the state (depth, normal, score)
  patch_match     a coarse plane_sweep (or a caller's state) refined by `iterations` red-black sweeps -> depth, normal, score
  normals_to_world   camera-frame normal maps into the poses' world frame, elementwise
  fuse_depths     the depth (and normal) maps of all views as one deduplicated, oriented, coloured cloud -> FusedCloud
                  (ls2fm_mvs_fuse_mark, ls2fm_mvs_fuse_emit, csrc/mvs_fuse.hip; COLMAP's stereo_fusion): a pixel gives a point
                  unless a lower view holds a consistent partner of it, and the point is the mean over its consistent partners
  dense_reconstruct   plane_sweep or patch_match -> filter_depths -> fusion.volume_for -> fusion.integrate -> fusion.extract: the
                  classical dense baseline row of the neural-surface tables (COLMAP's patch_match_stereo and stereo_fusion); its
                  mesh goes into ls2fm.mesh_colors.photo_colors and ls2fm.metrics.evaluate_mesh as it stands.  With
                  surface="poisson" or "mls": filter_depths -> fuse_depths -> ls2fm.cloud_mesh.mesh_from_cloud instead of the volume
  plane_sweep_torch, filter_depths_torch, plane_score_torch, patch_match_step_torch, fuse_depths_torch   the same rules as separate
                  torch ops, on CPU tensors as well: the checks of the kernels and the timing baselines (tools/time_mvs.py,
                  tools/time_patchmatch.py, tools/time_fuse.py); nothing in the library falls back to them

THE SWEEP RULE, THE CONSISTENCY RULE, THE PLANE SCORE, THE PATCHMATCH STEP and THE FUSION RULE are stated in include/ls2fm.h and
restated in numpy in tests/mvs_restate.py, tests/patchmatch_restate.py and tests/fuse_restate.py; the kernels, the torch forms and
the restatements agree bit for bit.  Conventions are the rasteriser's (ls2fm.raster.rasterize): poses world ->
camera [V, 3, 4], intr [3, 3] or [V, 3, 3], pixel (px, py) has its centre at px + 0.5, depth is camera z.  All views of a call
share one image size.  Each kernel call is one launch without host read or atomics: it can be captured, a rerun repeats its bits,
and the chunking of the reference views does not show in them.

Deviations of plane_sweep from COLMAP's dense stage, on purpose: the planes are fronto-parallel to the reference (no per-pixel
normals) and every pixel tries every plane (no propagation) -- patch_match lifts both.  Deviations of both: the score of a plane
is the mean NCC over the valid sources, not the best K of them or a per-pixel view selection; the window's taps weigh the same (no
bilateral weights); the cost holds no geometric-consistency term (filter_depths runs afterwards); one scale and one image size per
call; grey images only; no gradients.  Deviations of fuse_depths from COLMAP's stereo_fusion: a mean over the contributors, not a
median; the partners of a pixel come from its view's source list alone, no traversal beyond one hop; the nearest pixel of a
partner, not an interpolated one; no min_num_pixels inside the rule (min_support thresholds afterwards); near-duplicates remain
where consistency is not mutual.  fuse_depths makes one host read, the row count.

There is no CPU path for the kernels: CPU tensors, a missing device or a missing library raise, as in ls2fm.fusion.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import torch

from . import _lib, _posed, fusion
from ._lib import check, ptr, stream_ptr

TILE = 16                   # LS2FM_MVS_TILE
MAX_HALF_WIDTH = 5          # LS2FM_MVS_MAX_HALF_WIDTH
MAX_SOURCES = 64            # LS2FM_MVS_MAX_SOURCES
MAX_PLANES = 65536          # LS2FM_MVS_MAX_PLANES
PM_TILE_H, PM_TILE_W = 16, 32   # LS2FM_MVS_PM_TILE_H, LS2FM_MVS_PM_TILE_W
PM_DRAWS = 9                # LS2FM_MVS_PM_DRAWS
MIX_A, MIX_B, MIX_SALT = 0x21F0AAAD, 0x735A2D97, 0x9E3779B9    # LS2FM_MVS_MIX_A, LS2FM_MVS_MIX_B, LS2FM_MVS_MIX_SALT
FUSE_MAX_CHANNELS = 4       # LS2FM_MVS_FUSE_MAX_CHANNELS
FUSE_TILE_W, FUSE_TILE_H = 32, 8    # LS2FM_MVS_FUSE_TILE_W, LS2FM_MVS_FUSE_TILE_H
NEIGHBOURS = ((0, -1), (-1, 0), (1, 0), (0, 1), (0, -3), (-3, 0), (3, 0), (0, 3))     # (dx, dy), THE PATCHMATCH STEP's order
_device = functools.partial(_lib.require_device_tensors, "ls2fm.mvs", phrase=": multi-view stereo runs on MI355X only")


@dataclasses.dataclass
class MvsOptions:
    """The settings of dense_reconstruct; plane_sweep and filter_depths take the same names as keywords."""
    half_width: int = 3             # w: the window has (2 w + 1)^2 taps
    near: float = 1e-3
    min_var: float = 1e-6           # a window whose summed squared deviation is below it carries no texture
    min_sources: int = 1
    n_sources: int = 4              # select_sources
    min_angle: float = 3.0          # degrees
    max_angle: float = 45.0
    n_planes: int = 128             # depth_planes
    inverse_depth: bool = True
    margin: float = 0.05            # depth_range_from_points
    max_reproj: float = 1.0         # pixels
    rel_depth: float = 0.01
    min_consistent: int = 2
    max_workspace_bytes: int = 2 ** 28
    iterations: int = 5             # patch_match (dense_reconstruct with stereo="patchmatch")
    seed: int = 0
    depth_perturb: float = 0.02     # relative; halves with every iteration
    normal_perturb: float = 0.5
    max_slope: float = 1.0
    tap_step: int = 1
    patchmatch_planes: int = 32     # the planes of the initial sweep when dense_reconstruct forms them
    max_normal_angle: float = 60.0  # degrees: fuse_depths (dense_reconstruct with surface="poisson" or "mls")
    min_support: int = 1

    def patchmatch(self):
        return dict(self.sweep(), iterations=self.iterations, seed=self.seed, depth_perturb=self.depth_perturb,
                    normal_perturb=self.normal_perturb, max_slope=self.max_slope, tap_step=self.tap_step)

    def sweep(self):
        return dict(half_width=self.half_width, near=self.near, min_var=self.min_var, min_sources=self.min_sources,
                    max_workspace_bytes=self.max_workspace_bytes)

    def filter(self):
        return dict(near=self.near, max_reproj=self.max_reproj, rel_depth=self.rel_depth, min_consistent=self.min_consistent)

    def fuse(self):
        return dict(near=self.near, max_reproj=self.max_reproj, rel_depth=self.rel_depth, max_normal_angle=self.max_normal_angle,
                    min_support=self.min_support, max_workspace_bytes=self.max_workspace_bytes)


# --------------------------------------------------------------------------------------------------------- inputs, as torch ops
def to_grey(images):
    """images [V, H, W, 3] (or [H, W, 3]) -> float32 [V, H, W]: (0.299 r + 0.587 g) + 0.114 b; [V, H, W] passes through"""
    images = torch.as_tensor(images)
    if images.dim() == 3 and images.shape[-1] != 3:
        return _lib.cf(images.detach())
    if images.dim() == 3:
        images = images[None]
    if images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"ls2fm.mvs.to_grey: images must be [V, H, W, 3] or [V, H, W], got {tuple(images.shape)}")
    c = images.detach().float()
    return ((0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]).contiguous()


def _compose(pa, pb):
    """P_a o P_b^-1 of fp64 [..., 3, 4] arrays as elementwise fp64 operations in a stated order (no matrix product: the result
    does not depend on the device's GEMM):  R_ij = (Ra_i0 Rb_j0 + Ra_i1 Rb_j1) + Ra_i2 Rb_j2;
    t_i = ta_i - ((R_i0 tb_0 + R_i1 tb_1) + R_i2 tb_2)"""
    Ra, ta, Rb, tb = pa[..., :3], pa[..., 3], pb[..., :3], pb[..., 3]
    p = Ra[..., :, None, :] * Rb[..., None, :, :]
    R = (p[..., 0] + p[..., 1]) + p[..., 2]
    q = R * tb[..., None, :]
    t = ta - ((q[..., 0] + q[..., 1]) + q[..., 2])
    return torch.cat([R, t[..., None]], dim=-1)


def relative_poses(pose, refs, sources, back=False):
    """P_rs = P_s o P_r^-1 per (reference, source) -> float32 [R, S, 3, 4], formed in fp64 with elementwise torch ops on the pose's
    device and rounded once; with back=True P_sr = P_r o P_s^-1.  pose [V, 3, 4]; refs int [R]; sources int [R, S], whose entries
    outside [0, V) give an entry that no rule reads."""
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).double()
    refs = torch.as_tensor(refs, device=P.device).long().reshape(-1)
    sources = torch.as_tensor(sources, device=P.device).long().reshape(refs.shape[0], -1)
    V = P.shape[0]
    Pr = P[refs.clamp(0, V - 1)][:, None]
    Ps = P[sources.clamp(0, V - 1)]
    return (_compose(Pr, Ps) if back else _compose(Ps, Pr)).float().contiguous()


def depth_planes(near, far, D, inverse=True):
    """The plane depths of the sweep -> float32 [R, D]: D planes from near to far, uniform in inverse depth (the default, uniform
    in disparity) or in depth, formed in fp64 and rounded once.  near and far: floats or [R] tensors; D = 1 gives near."""
    near, far = torch.as_tensor(near), torch.as_tensor(far)
    dev = near.device if near.is_cuda else far.device
    near, far = near.double().to(dev).reshape(-1), far.double().to(dev).reshape(-1)
    D = int(D)
    if D < 1:
        raise ValueError(f"ls2fm.mvs.depth_planes: D {D} must be at least 1")
    t = torch.arange(D, dtype=torch.float64, device=dev) / max(D - 1, 1)
    if inverse:
        d = 1.0 / (1.0 / near[:, None] + t * (1.0 / far[:, None] - 1.0 / near[:, None]))
    else:
        d = near[:, None] + t * (far[:, None] - near[:, None])
    return d.float().contiguous()


def depth_range_from_points(points, pose, margin=0.05):
    """Per view the range of camera z of the points in front of it -> (near, far) float32 [V] each: the minimum times 1 - margin
    and the maximum times 1 + margin, as torch ops; a view with no point in front of it gets NaN.  points: [N, 3], or an
    ls2fm.mapper.Reconstruction (its valid tracks' X)."""
    if hasattr(points, "X") and hasattr(points, "track_valid"):
        points = points.X[points.track_valid]
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).double()
    X = torch.as_tensor(points).detach().reshape(-1, 3).double().to(P.device)
    cz = ((P[:, None, 2, 0] * X[None, :, 0] + P[:, None, 2, 1] * X[None, :, 1]) + P[:, None, 2, 2] * X[None, :, 2]) + P[:, None, 2, 3]
    front = torch.isfinite(cz) & (cz > 0)
    inf = torch.full_like(cz, math.inf)
    lo = torch.where(front, cz, inf).amin(dim=1) if X.shape[0] else inf[:, 0]
    hi = torch.where(front, cz, -inf).amax(dim=1) if X.shape[0] else -inf[:, 0]
    nan = torch.full_like(lo, math.nan)
    some = front.any(dim=1)
    return (torch.where(some, lo * (1.0 - margin), nan).float(), torch.where(some, hi * (1.0 + margin), nan).float())


def select_sources(pose, n, min_angle=3.0, max_angle=45.0, centre=None):
    """Per view its n source views -> int32 [V, n], -1 where fewer qualify; torch ops, no host read.  The other views are ranked
    by the angle at the scene centre between the two viewing rays (camera centre to scene centre), the smallest first, inside
    the band [min_angle, max_angle] (degrees); equal angles go to the longer baseline, then to the lower index.  centre: three
    floats, by default the point nearest to all optical axes in least squares."""
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).double()
    V, n = int(P.shape[0]), int(n)
    R, t = P[:, :, :3], P[:, :, 3]
    C = -(R.transpose(1, 2) @ t[:, :, None])[:, :, 0]
    if centre is None:
        z = R[:, 2]
        M = torch.eye(3, dtype=torch.float64, device=P.device)[None] - z[:, :, None] * z[:, None, :]
        A, b = M.sum(dim=0), (M @ C[:, :, None]).sum(dim=0)
        c = (torch.linalg.inv_ex(A).inverse @ b)[:, 0]                 # inv_ex: no status read back
    else:
        c = torch.as_tensor(centre, dtype=torch.float64, device=P.device).reshape(3)
    ray = c[None] - C
    ray = ray / ray.norm(dim=1, keepdim=True)
    angle = torch.rad2deg(torch.acos((ray @ ray.T).clamp(-1.0, 1.0)))
    baseline = (C[:, None] - C[None]).norm(dim=2)
    ok = (angle >= float(min_angle)) & (angle <= float(max_angle)) & ~torch.eye(V, dtype=torch.bool, device=P.device)
    key = torch.where(ok, angle, torch.full_like(angle, math.inf))
    first = torch.argsort(-baseline, dim=1, stable=True)
    order = torch.gather(first, 1, torch.argsort(torch.gather(key, 1, first), dim=1, stable=True))
    picked = torch.where(torch.gather(ok, 1, order), order, torch.full_like(order, -1))
    out = torch.full((V, n), -1, dtype=torch.int64, device=P.device)
    out[:, :min(n, V)] = picked[:, :n]
    return out.to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _check_sweep(half_width, min_var, min_sources, S, D, who):
    half_width, min_var, min_sources = int(half_width), float(min_var), int(min_sources)
    if not 1 <= half_width <= MAX_HALF_WIDTH:
        raise ValueError(f"{who}: half_width {half_width} must be in [1, {MAX_HALF_WIDTH}]")
    if not 0.0 <= min_var < math.inf:
        raise ValueError(f"{who}: min_var {min_var} must be finite and not negative")
    if not 1 <= S <= MAX_SOURCES or not 1 <= D <= MAX_PLANES:
        raise ValueError(f"{who}: {S} sources per reference (1 to {MAX_SOURCES}) and {D} planes (1 to {MAX_PLANES})")
    if not 1 <= min_sources <= S:
        raise ValueError(f"{who}: min_sources {min_sources} must be in [1, {S}]")
    return half_width, min_var, min_sources


def _check_filter(max_reproj, rel_depth, min_consistent, S, who):
    max_reproj, rel_depth, min_consistent = float(max_reproj), float(rel_depth), int(min_consistent)
    if not (0.0 <= max_reproj < math.inf and 0.0 <= rel_depth < math.inf) or min_consistent < 0:
        raise ValueError(f"{who}: max_reproj {max_reproj} and rel_depth {rel_depth} must be finite and not negative, min_consistent "
                         f"{min_consistent} not negative")
    if not 1 <= S <= MAX_SOURCES:
        raise ValueError(f"{who}: {S} sources per view (1 to {MAX_SOURCES})")
    return max_reproj, rel_depth, min_consistent


def _index_arrays(refs, sources, depths, V, dev, who):
    refs = torch.arange(V, device=dev) if refs is None else torch.as_tensor(refs, device=dev).reshape(-1)
    R = int(refs.shape[0])
    sources = torch.as_tensor(sources, device=dev)
    if sources.dim() != 2 or sources.shape[0] != R:
        raise ValueError(f"{who}: sources must be [{R}, S], one row per reference, got {tuple(sources.shape)}")
    if depths is not None:
        depths = torch.as_tensor(depths, device=dev)
        if depths.dim() == 1:
            depths = depths[None].expand(R, -1)
        if depths.dim() != 2 or depths.shape[0] != R:
            raise ValueError(f"{who}: depths must be [D] or [{R}, D], got {tuple(depths.shape)}")
        depths = depths.detach().float().contiguous()
    return refs.to(torch.int32).contiguous(), sources.to(torch.int32).contiguous(), depths


def _grey(images, n, who):
    images = torch.as_tensor(images)
    if images.dim() != 3 or images.shape[0] != n:
        raise ValueError(f"{who}: images must be grey float [{n}, H, W] (see to_grey), got {tuple(images.shape)}")
    return _lib.cf(images.detach())


def _check_tap_step(tap_step, who):
    tap_step = int(tap_step)
    if tap_step not in (1, 2):
        raise ValueError(f"{who}: tap_step {tap_step} must be 1 or 2")
    return tap_step


class _Checked:
    """the checked inputs of one set of references, as the kernels (_Inputs) and the torch forms (_TorchScene) take them"""

    def gather(self, img, poses, sources, refs, depths, half_width, tap_step, min_var, min_sources, who):
        self.V, self.dev = int(poses.shape[0]), poses.device
        self.img = _grey(img, self.V, who)
        self.refs, self.sources, self.depths = _index_arrays(refs, sources, depths, self.V, self.dev, who)
        self.R, self.S, self.H, self.W = int(self.refs.shape[0]), int(self.sources.shape[1]), int(self.img.shape[1]), int(self.img.shape[2])
        self.D = 1 if depths is None else int(self.depths.shape[1])
        self.w, self.min_var, self.min_sources = _check_sweep(half_width, min_var, min_sources, self.S, self.D, who)
        self.t = _check_tap_step(tap_step, who)
        self.rel = relative_poses(poses, self.refs, self.sources)


def _device_views(maps, pose, intr, who):
    """-> the maps as given, the poses [V, 3, 4] and k4 [V, 4] of a call that runs on the device"""
    maps = torch.as_tensor(maps)
    _device(maps, torch.as_tensor(pose), torch.as_tensor(intr))
    return (maps,) + _posed.views(pose, intr, who)


class _Inputs(_Checked):
    """what plane_sweep, plane_score, patch_match_step and patch_match share: the checked inputs of one set of references"""

    def __init__(self, images, pose, intr, sources, refs, half_width, tap_step, near, min_var, min_sources, who, depths=None):
        images, poses, self.k4 = _device_views(images, pose, intr, who)
        self.gather(images, poses, sources, refs, depths, half_width, tap_step, min_var, min_sources, who)
        self.near = _posed.near_plane(near, who)
        if self.img.device != self.dev:
            raise ValueError(f"{who}: the poses on {self.dev}, the images on {self.img.device}")

    def head(self, s, e, depths=None):
        """the arguments every entry point begins with, for the references s .. e: the sweep has its planes before the poses and
        no tap step"""
        planes, taps = ((), (self.t,)) if depths is None else ((ptr(depths[s:e]), int(depths.shape[1])), ())
        return (ptr(self.img), self.V, self.H, self.W, ptr(self.refs[s:e]), e - s, ptr(self.sources[s:e]), self.S, *planes,
                ptr(self.rel[s:e]), ptr(self.k4), self.w, *taps, self.near, self.min_var, self.min_sources)

    def sweep(self, depths, budget):
        """ls2fm_mvs_sweep over the checked planes depths [R, D] -> depth, score, plane"""
        depth = torch.empty((self.R, self.H, self.W), dtype=torch.float32, device=self.dev)
        score = torch.empty((self.R, self.H, self.W), dtype=torch.float32, device=self.dev)
        plane = torch.empty((self.R, self.H, self.W), dtype=torch.int32, device=self.dev)
        lib = _lib.load()
        with torch.cuda.device(self.dev):
            for s, e in _posed.chunks(self.R, 12, self.H, self.W, budget):
                check(lib.ls2fm_mvs_sweep(*self.head(s, e, depths), ptr(depth[s:e]), ptr(score[s:e]), ptr(plane[s:e]), stream_ptr()),
                      "ls2fm_mvs_sweep")
        return depth, score, plane

    def score(self, depth, normal, score, budget):
        lib = _lib.load()
        with torch.cuda.device(self.dev):
            for s, e in _posed.chunks(self.R, 20, self.H, self.W, budget):
                check(lib.ls2fm_mvs_plane_score(*self.head(s, e), ptr(depth[s:e]), ptr(normal[s:e]), ptr(score[s:e]), stream_ptr()),
                      "ls2fm_mvs_plane_score")

    def step(self, depth, normal, score, colour, iteration, seed, rho_d, rho_n, sigma, d_min, d_max, budget):
        lib = _lib.load()
        with torch.cuda.device(self.dev):
            for s, e in _posed.chunks(self.R, 20, self.H, self.W, budget):
                check(lib.ls2fm_mvs_patchmatch_step(*self.head(s, e), colour, iteration, int(seed) & 0xFFFFFFFF, rho_d, rho_n, sigma,
                                                    ptr(d_min[s:e]), ptr(d_max[s:e]), ptr(depth[s:e]), ptr(normal[s:e]), ptr(score[s:e]),
                                                    stream_ptr()), "ls2fm_mvs_patchmatch_step")


@torch.no_grad()
def plane_sweep(images, pose, intr, sources, depths, refs=None, half_width=3, near=1e-3, min_var=1e-6, min_sources=1,
                max_workspace_bytes=2 ** 28):
    """THE SWEEP RULE of include/ls2fm.h -> (depth float32 [R, H, W], score float32 [R, H, W], plane int32 [R, H, W]); an
    invalid pixel has NaN, NaN and -1.
      images     grey float32 [V, H, W] (to_grey)
      pose, intr [V, 3, 4] world-to-camera and [3, 3] or [V, 3, 3], as ls2fm.raster.rasterize
      refs       int [R], the reference views; default every view
      sources    int [R, S], per reference its source views; -1 skips (select_sources)
      depths     float [R, D] or [D], the plane depths (depth_planes)
    The references go in chunks whose outputs (12 bytes per pixel) stay within max_workspace_bytes, one launch per chunk; the
    chunking does not show in the bits.  No host read."""
    a = _Inputs(images, pose, intr, sources, refs, half_width, 1, near, min_var, min_sources, "ls2fm.mvs.plane_sweep", depths)
    return a.sweep(a.depths, max_workspace_bytes)


@torch.no_grad()
def filter_depths(depth, pose, intr, sources, near=1e-3, max_reproj=1.0, rel_depth=0.01, min_consistent=2):
    """THE CONSISTENCY RULE of include/ls2fm.h -> (filtered float32 [V, H, W], count uint8 [V, H, W]): count is the number of
    source views whose depth map agrees with the pixel's depth (it projects back within max_reproj pixels and rel_depth d); filtered
    is the depth where count >= min_consistent and NaN elsewhere -- what ls2fm.fusion.integrate skips.
      depth      float32 [V, H, W], one map per view (plane_sweep with refs=None); pixels that are not finite and positive count 0
      sources    int [V, S]; -1 skips
    One launch, no host read."""
    who = "ls2fm.mvs.filter_depths"
    depth, poses, k4 = _device_views(depth, pose, intr, who)
    V, dev = int(poses.shape[0]), poses.device
    d = _grey(depth, V, who)
    refs, sources, _ = _index_arrays(None, sources, None, V, dev, who)
    S, H, W = int(sources.shape[1]), int(d.shape[1]), int(d.shape[2])
    max_reproj, rel_depth, min_consistent = _check_filter(max_reproj, rel_depth, min_consistent, S, who)
    near = _posed.near_plane(near, who)
    if d.device != dev:
        raise ValueError(f"{who}: the poses on {dev}, the depth maps on {d.device}")
    rel, back = relative_poses(poses, refs, sources), relative_poses(poses, refs, sources, back=True)
    count = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    out = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().ls2fm_mvs_filter(ptr(d), V, H, W, ptr(sources), S, ptr(rel), ptr(back), ptr(k4), near, max_reproj, rel_depth,
                                           min_consistent, ptr(count), ptr(out), stream_ptr()), "ls2fm_mvs_filter")
    return out, count


# ------------------------------------------------------------------------------------------------------------------------ fusion
@dataclasses.dataclass
class FusedCloud:
    """What fuse_depths returns: M rows in (view, py, px) order of their owners."""
    points: torch.Tensor            # float32 [M, 3], world
    normals: torch.Tensor           # float32 [M, 3], world, of unit length, toward the cameras; None without normal maps
    colors: torch.Tensor            # float32 [M, C]; None without images
    support: torch.Tensor           # uint8 [M]: 1 + the consistent partners folded into the row
    view: torch.Tensor              # int64 [M]: the owner's view
    pixel: torch.Tensor             # int64 [M]: (view H + py) W + px of the owner
    centers: torch.Tensor           # float32 [M, 3]: the owner's camera centre (estimate_normals' `toward`)


def cam_to_world(pose):
    """P^-1 per view -> float32 [V, 3, 4]: formed in fp64 with elementwise torch ops in relative_poses' order (the identity
    composed with P^-1) on the pose's device and rounded once; its last column is the camera centre."""
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).double()
    eye = torch.eye(3, 4, dtype=torch.float64, device=P.device).expand(P.shape)
    return _compose(eye, P).float().contiguous()


def _check_fuse(max_normal_angle, min_support, max_reproj, rel_depth, S, who):
    """-> max_reproj, rel_depth, cos2 (fp64; the float argument of the call, or the float32 tensor of the torch form, rounds it
    once), min_support"""
    max_reproj, rel_depth, _ = _check_filter(max_reproj, rel_depth, 0, S, who)
    angle, min_support = float(max_normal_angle), int(min_support)
    if not 0.0 <= angle <= 90.0:
        raise ValueError(f"{who}: max_normal_angle {angle} must be in [0, 90] degrees")
    if min_support < 1:
        raise ValueError(f"{who}: min_support {min_support} must be at least 1 (the pixel itself)")
    return max_reproj, rel_depth, math.cos(math.radians(angle)) ** 2, min_support


def _fuse_maps(normal, images, V, H, W, dev, who):
    """the optional maps as contiguous float32 [V, H, W, 3] and [V, H, W, C] on dev, or None"""
    if normal is not None:
        normal = torch.as_tensor(normal)
        if tuple(normal.shape) != (V, H, W, 3):
            raise ValueError(f"{who}: normal must be [{V}, {H}, {W}, 3], got {tuple(normal.shape)}")
        normal = _lib.cf(normal.detach())
    if images is not None:
        images = torch.as_tensor(images)
        if images.dim() == 3:
            images = images[..., None]
        if images.dim() != 4 or tuple(images.shape[:3]) != (V, H, W) or not 1 <= images.shape[3] <= FUSE_MAX_CHANNELS:
            raise ValueError(f"{who}: images must be [{V}, {H}, {W}] or [{V}, {H}, {W}, C] with C in 1 .. {FUSE_MAX_CHANNELS}, got "
                             f"{tuple(images.shape)}")
        images = _lib.cf(images.detach())
    for name, t in (("normal", normal), ("images", images)):
        if t is not None and t.device != dev:
            raise ValueError(f"{who}: the poses on {dev}, {name} on {t.device}")
    return normal, images


def _no_cloud(normal, colour, dev):
    """the FusedCloud of no views"""
    rows = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    return FusedCloud(rows(0, 3), None if normal is None else rows(0, 3), None if colour is None else rows(0, int(colour.shape[3])),
                      rows(0, dtype=torch.uint8), rows(0, dtype=torch.int64), rows(0, dtype=torch.int64), rows(0, 3))


def _fused_cloud(points, normals, colours, support, pixel, to_world, H, W, min_support):
    """the rows as a FusedCloud, those with support >= min_support (torch ops)"""
    if min_support > 1:
        keep = support >= min_support
        points, support, pixel = points[keep], support[keep], pixel[keep]
        normals = None if normals is None else normals[keep]
        colours = None if colours is None else colours[keep]
    view = torch.div(pixel, H * W, rounding_mode="floor")
    return FusedCloud(points, normals, colours, support, view, pixel, to_world[:, :, 3][view])


@torch.no_grad()
def fuse_depths(depth, pose, intr, sources, normal=None, images=None, near=1e-3, max_reproj=1.0, rel_depth=0.01, max_normal_angle=60.0,
                min_support=1, max_workspace_bytes=2 ** 28):
    """THE FUSION RULE of include/ls2fm.h -> FusedCloud: the depth (and normal) maps of all views as one deduplicated, oriented,
    coloured cloud in the poses' world frame.  A pixel with a depth gives a point unless a lower view holds a consistent partner of
    it; the point, normal and colour are the means over the pixel and its consistent partners.
      depth      float32 [V, H, W], filter_depths' output: pixels that are not finite and positive give nothing
      sources    int [V, S]; -1 skips; the partners of a pixel come from its view's row alone
      normal     float [V, H, W, 3] in each camera's frame (patch_match's), any length; a partner whose normal is further than
                 max_normal_angle degrees from the pixel's is not consistent.  None: no normal test, FusedCloud.normals is None
      images     float [V, H, W, C] or [V, H, W], C in 1 .. 4: the colours to average.  None: FusedCloud.colors is None
      min_support   rows with a lower support are dropped afterwards, with torch ops
    The views go in chunks whose workspace (the row index and its prefix sum, 24 bytes per pixel) stays within max_workspace_bytes:
    ls2fm_mvs_fuse_mark per chunk, the row count (the one host read), then torch's prefix sum and ls2fm_mvs_fuse_emit per chunk;
    the chunking does not show in the bits."""
    who = "ls2fm.mvs.fuse_depths"
    depth, poses, k4 = _device_views(depth, pose, intr, who)
    V, dev = int(poses.shape[0]), poses.device
    d = _grey(depth, V, who)
    refs, sources, _ = _index_arrays(None, sources, None, V, dev, who)
    S, H, W = int(sources.shape[1]), int(d.shape[1]), int(d.shape[2])
    max_reproj, rel_depth, cos2, min_support = _check_fuse(max_normal_angle, min_support, max_reproj, rel_depth, S, who)
    near = _posed.near_plane(near, who)
    if d.device != dev:
        raise ValueError(f"{who}: the poses on {dev}, the depth maps on {d.device}")
    for name, t in (("normal", normal), ("images", images)):
        if t is not None:
            _device(torch.as_tensor(t))
    normal, colour = _fuse_maps(normal, images, V, H, W, dev, who)
    C = 0 if colour is None else int(colour.shape[3])
    if V == 0:
        return _no_cloud(normal, colour, dev)
    rel, back = relative_poses(poses, refs, sources), relative_poses(poses, refs, sources, back=True)
    to_world = cam_to_world(poses)
    support = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    shared = (ptr(sources), S, ptr(rel), ptr(back), ptr(k4))
    chunks = _posed.chunks(V, 24, H, W, max_workspace_bytes)
    with torch.cuda.device(dev):
        for s, e in chunks:
            check(lib.ls2fm_mvs_fuse_mark(ptr(d), ptr(normal), V, H, W, *shared, near, max_reproj, rel_depth, cos2, s, e, ptr(support),
                                          stream_ptr()), "ls2fm_mvs_fuse_mark")
        per_view = (support > 0).reshape(V, -1).sum(dim=1)
        before = per_view.cumsum(dim=0) - per_view                      # int64 [V]: the rows of the views before each
        M = int(per_view.sum()) if V else 0                             # the one host read
        points = torch.empty((M, 3), dtype=torch.float32, device=dev)
        normals = None if normal is None else torch.empty((M, 3), dtype=torch.float32, device=dev)
        colours = None if colour is None else torch.empty((M, C), dtype=torch.float32, device=dev)
        pixel = torch.empty((M,), dtype=torch.int64, device=dev)
        for s, e in chunks if M else ():
            gives = support[s:e].reshape(-1).clamp(max=1)
            row = gives.cumsum(dim=0, dtype=torch.int64)                # made exclusive and global in place
            row -= gives
            row += before[s]
            check(lib.ls2fm_mvs_fuse_emit(ptr(d), ptr(normal), ptr(colour), C, V, H, W, *shared, ptr(to_world), near, max_reproj,
                                          rel_depth, cos2, s, e, ptr(support), ptr(row), M, ptr(points), ptr(normals), ptr(colours),
                                          ptr(pixel), stream_ptr()), "ls2fm_mvs_fuse_emit")
            del gives, row
    rows = support.reshape(-1)[pixel]
    return _fused_cloud(points, normals, colours, rows, pixel, to_world, H, W, min_support)


# -------------------------------------------------------------------------------------------------------------------- PatchMatch
def _check_step(colour, iteration, depth_perturb, normal_perturb, max_slope, who):
    """-> colour, iteration, rho_d, rho_n, sigma: the perturbations on the schedule rho 2^-iteration, formed in fp64 (the float
    argument of the call, or the float32 tensor of the torch form, rounds them once)"""
    colour, iteration = int(colour), int(iteration)
    if colour not in (0, 1) or iteration < 0:
        raise ValueError(f"{who}: colour {colour} must be 0 or 1, iteration {iteration} not negative")
    rho = [float(depth_perturb), float(normal_perturb), float(max_slope)]
    if not all(0.0 <= v < math.inf for v in rho):
        raise ValueError(f"{who}: depth_perturb {rho[0]}, normal_perturb {rho[1]} and max_slope {rho[2]} must be finite and not negative")
    return colour, iteration, rho[0] * 2.0 ** -iteration, rho[1] * 2.0 ** -iteration, rho[2]


def _state(depth, normal, score, R, H, W, dev, who, in_place):
    """the state's arrays as float32 [R, H, W], [R, H, W, 3], [R, H, W] on dev; what is updated in place must be so already"""
    out = []
    for name, t, shape in (("depth", depth, (R, H, W)), ("normal", normal, (R, H, W, 3)), ("score", score, (R, H, W))):
        if t is None:
            out.append(None)
            continue
        t = torch.as_tensor(t)
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)}, got {tuple(t.shape)}")
        if in_place and not (t.dtype == torch.float32 and t.is_contiguous() and t.device == dev):
            raise ValueError(f"{who}: {name} is updated in place: it must be a contiguous float32 tensor on {dev}")
        out.append(t if in_place else _lib.cf(t.detach().to(dev)))
    return out


def _range(d_min, d_max, R, dev, who):
    out = []
    for name, t in (("d_min", d_min), ("d_max", d_max)):
        t = torch.as_tensor(t, device=dev).detach().float().reshape(-1)
        if t.shape[0] == 1:
            t = t.expand(R)
        if t.shape[0] != R:
            raise ValueError(f"{who}: {name} must be a float or [{R}], got {tuple(t.shape)}")
        out.append(t.contiguous())
    return out


@torch.no_grad()
def plane_score(images, pose, intr, sources, depth, normal, refs=None, half_width=3, tap_step=1, near=1e-3, min_var=1e-6, min_sources=1,
                max_workspace_bytes=2 ** 28):
    """THE PLANE SCORE of include/ls2fm.h at every pixel of a state -> score float32 [R, H, W], NaN where the pixel, the
    hypothesis or too many sources are invalid.
      depth      float [R, H, W]: camera z at the pixel centre
      normal     float [R, H, W, 3]: the plane's normal in the reference camera's frame (any length); it must face the camera
      tap_step   1, or 2 for every other tap of the window in both axes
    The other arguments are plane_sweep's.  One launch per chunk of references (20 bytes per pixel within max_workspace_bytes); no
    host read."""
    who = "ls2fm.mvs.plane_score"
    a = _Inputs(images, pose, intr, sources, refs, half_width, tap_step, near, min_var, min_sources, who)
    depth, normal, _ = _state(depth, normal, None, a.R, a.H, a.W, a.dev, who, False)
    score = torch.empty((a.R, a.H, a.W), dtype=torch.float32, device=a.dev)
    a.score(depth, normal, score, max_workspace_bytes)
    return score


@torch.no_grad()
def patch_match_step(images, pose, intr, sources, depth, normal, score, colour, iteration, d_min, d_max, refs=None, seed=0,
                     depth_perturb=0.02, normal_perturb=0.5, max_slope=1.0, half_width=3, tap_step=1, near=1e-3, min_var=1e-6,
                     min_sources=1, max_workspace_bytes=2 ** 28):
    """THE PATCHMATCH STEP of include/ls2fm.h: one half-sweep over the pixels with (px + py) & 1 == colour, in place on the state
    depth [R, H, W], normal [R, H, W, 3], score [R, H, W] (contiguous float32 device tensors; score as plane_score leaves it)
    -> the same three tensors.  Each such pixel tries the planes of eight neighbours of the other colour, a perturbed depth, a
    perturbed normal, both, and a fresh hypothesis between d_min and d_max (floats or [R]) with a slope up to max_slope, and keeps
    what scores strictly higher.  depth_perturb and normal_perturb are the values of iteration 0: the step halves them `iteration`
    times.  The draws depend on (seed, view, iteration, pixel) alone.  One launch per chunk of references; no host read."""
    who = "ls2fm.mvs.patch_match_step"
    a = _Inputs(images, pose, intr, sources, refs, half_width, tap_step, near, min_var, min_sources, who)
    colour, iteration, rho_d, rho_n, sigma = _check_step(colour, iteration, depth_perturb, normal_perturb, max_slope, who)
    depth, normal, score = _state(depth, normal, score, a.R, a.H, a.W, a.dev, who, True)
    d_min, d_max = _range(d_min, d_max, a.R, a.dev, who)
    a.step(depth, normal, score, colour, iteration, seed, rho_d, rho_n, sigma, d_min, d_max, max_workspace_bytes)
    return depth, normal, score


@torch.no_grad()
def patch_match(images, pose, intr, sources, depths, refs=None, iterations=5, init=None, seed=0, depth_perturb=0.02, normal_perturb=0.5,
                max_slope=1.0, tap_step=1, half_width=3, near=1e-3, min_var=1e-6, min_sources=1, max_workspace_bytes=2 ** 28):
    """PatchMatch stereo -> (depth float32 [R, H, W], normal float32 [R, H, W, 3] in each reference camera's frame, score float32
    [R, H, W]); depth and normal are NaN where the final score is.
      depths     float [R, D] or [D]: the planes of the initial sweep (a coarse D, 16 to 32, is the intended use); the ends of each
                 row are the range d_min, d_max of the fresh hypotheses
      init       None: plane_sweep over `depths`, its depth with the normal (0, 0, -1); or a caller's (depth, normal)
      iterations each runs colour 0, then colour 1, with depth_perturb and normal_perturb halved from one to the next
    plane_score turns the initial state into scores; then 2 `iterations` launches of patch_match_step per chunk of references, chunked
    as plane_sweep chunks them.  No host read; a rerun repeats the bits."""
    who = "ls2fm.mvs.patch_match"
    a = _Inputs(images, pose, intr, sources, refs, half_width, tap_step, near, min_var, min_sources, who)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"{who}: iterations {iterations} must not be negative")
    _check_step(0, 0, depth_perturb, normal_perturb, max_slope, who)
    _, _, depths = _index_arrays(a.refs, a.sources, depths, a.V, a.dev, who)
    d_min, d_max = depths[:, 0].contiguous(), depths[:, -1].contiguous()
    if init is None:
        # the inputs are checked already; what the sweep adds is its plane count, refused in plane_sweep's name as before
        _check_sweep(a.w, a.min_var, a.min_sources, a.S, int(depths.shape[1]), "ls2fm.mvs.plane_sweep")
        depth = a.sweep(depths, max_workspace_bytes)[0]
        normal = torch.zeros((a.R, a.H, a.W, 3), dtype=torch.float32, device=a.dev)
        normal[..., 2] = -1.0
    else:
        depth, normal, _ = _state(init[0], init[1], None, a.R, a.H, a.W, a.dev, who, False)
        depth, normal = depth.clone(), normal.clone()
    score = torch.empty((a.R, a.H, a.W), dtype=torch.float32, device=a.dev)
    a.score(depth, normal, score, max_workspace_bytes)
    for it in range(iterations):
        _, _, rho_d, rho_n, sigma = _check_step(0, it, depth_perturb, normal_perturb, max_slope, who)
        for colour in (0, 1):
            a.step(depth, normal, score, colour, it, seed, rho_d, rho_n, sigma, d_min, d_max, max_workspace_bytes)
    dead = torch.isnan(score)
    depth.masked_fill_(dead, math.nan)
    normal.masked_fill_(dead[..., None], math.nan)
    return depth, normal, score


def normals_to_world(normal, pose, refs=None):
    """Camera-frame normal maps [R, H, W, 3] of the views refs (default: every view, R = V) -> the same in the world frame of
    pose [V, 3, 4]: n_w = R^T n_c as elementwise torch ops, (R_0j n_0 + R_1j n_1) + R_2j n_2 -- no GEMM, so the device's matrix
    product does not show in the bits.  Any device."""
    normal = torch.as_tensor(normal).detach().float()
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).float().to(normal.device)
    if normal.dim() != 4 or normal.shape[-1] != 3:
        raise ValueError(f"ls2fm.mvs.normals_to_world: normal must be [R, H, W, 3], got {tuple(normal.shape)}")
    refs = torch.arange(P.shape[0], device=normal.device) if refs is None else torch.as_tensor(refs, device=normal.device).long().reshape(-1)
    if refs.shape[0] != normal.shape[0]:
        raise ValueError(f"ls2fm.mvs.normals_to_world: {normal.shape[0]} normal maps for {refs.shape[0]} references")
    Rm = P[refs.clamp(0, P.shape[0] - 1), :, :3][:, None, None]                    # [R, 1, 1, 3, 3]
    n = normal[..., :, None]                                                       # [R, H, W, 3, 1]
    return (Rm[..., 0, :] * n[..., 0, :] + Rm[..., 1, :] * n[..., 1, :]) + Rm[..., 2, :] * n[..., 2, :]


# -------------------------------------------------------------------------------------------------------------- the torch forms
def _torch_views(maps, pose, intr):
    """-> the maps as float32, P [V, 3, 4] and K [V, 3, 3] on the maps' device"""
    maps = torch.as_tensor(maps).detach().float()
    P = torch.as_tensor(pose).detach().reshape(-1, 3, 4).float().to(maps.device)
    K = torch.as_tensor(intr).detach().reshape(-1, 3, 3).float().to(maps.device).expand(P.shape[0], 3, 3)
    return maps, P, K


def _scalar(v, dev):
    """a 0-dim float32 tensor on dev: a division by a Python scalar would be a multiplication by its reciprocal"""
    return torch.tensor(float(v), dtype=torch.float32, device=dev)


def _taps(Z, w):
    """the (2 w + 1)^2 shifted views of Z [H, W] in row-major window order; a tap outside the image reads NaN"""
    H, W = Z.shape
    pad = torch.full((H + 2 * w, W + 2 * w), math.nan, dtype=Z.dtype, device=Z.device)
    pad[w:w + H, w:w + W] = Z
    return [pad[i:i + H, j:j + W] for i in range(2 * w + 1) for j in range(2 * w + 1)]


def _tap_sum(taps):
    total = torch.zeros_like(taps[0])
    for t in taps:
        total = total + t
    return total


def _sqrt_rn(t):
    """the correctly rounded fp32 square root: torch.sqrt of a float32 tensor is not correctly rounded on every backend (the CPU's
    vectorised one is not); the fp64 root rounded to fp32 is, since 53 >= 2 * 24 + 2 bits leave no double rounding"""
    return torch.sqrt(t.double()).float()


def _lift(K, H, W, dev):
    """xn [1, W] and yn [H, 1] of every pixel centre"""
    xn = ((torch.arange(W, device=dev).float() + 0.5) - K[0, 2]) / K[0, 0]
    yn = ((torch.arange(H, device=dev).float() + 0.5) - K[1, 2]) / K[1, 1]
    return xn[None, :], yn[:, None]


class _TorchScene(_Checked):
    """the inputs of plane_sweep_torch, plane_score_torch and patch_match_step_torch, and per reference what no plane changes"""

    def __init__(self, images, pose, intr, sources, refs, half_width, tap_step, near, min_var, min_sources, who, depths=None):
        img, P, self.K = _torch_views(images, pose, intr)
        self.gather(img, P, sources, refs, depths, half_width, tap_step, min_var, min_sources, who)
        self.refs, self.sources = self.refs.tolist(), self.sources.tolist()
        self.scalar = functools.partial(_scalar, dev=self.dev)
        side = range(0, 2 * self.w + 1, self.t)
        self.offsets = [(j - self.w, i - self.w) for i in side for j in side]
        self.picked = [i * (2 * self.w + 1) + j for i in side for j in side]
        self.n, self.near, self.min_var = self.scalar(len(self.offsets)), self.scalar(_posed.near_plane(near, who)), self.scalar(self.min_var)
        self.cache = {}

    def reference(self, r):
        """step 1 of THE SWEEP RULE over the window's picked taps `a`, and the lift xn [W], yn [H]; None for a view outside [0, V)"""
        rv = self.refs[r]
        if not 0 <= rv < self.V:
            return None
        if r not in self.cache:
            nan = torch.full((self.H, self.W), math.nan, dtype=torch.float32, device=self.dev)
            img = torch.where(torch.isfinite(self.img[rv]), self.img[rv], nan)
            every = _taps(img, self.w)
            a = [every[i] for i in self.picked]
            sa = _tap_sum(a)
            ma = sa / self.n
            va = torch.zeros_like(sa)
            for t in a:
                va = va + (t - ma) * (t - ma)
            xn, yn = _lift(self.K[rv], self.H, self.W, self.dev)
            self.cache[r] = dict(rv=rv, img=img, a=a, ma=ma, va=va, pixel_ok=~torch.isnan(sa) & ~(va < self.min_var), xn=xn[0], yn=yn[:, 0])
        return self.cache[r]

    def sample(self, r, s, sv, X, Y, Z):
        """steps 2 and 3 of THE SWEEP RULE at the camera points (X, Y, Z) of reference r: NaN where not valid"""
        H, W = self.H, self.W
        _, u, v, usable, _, _, _ = _posed.project_torch(self.rel[r, s], self.K[sv], X, Y, Z, self.near, H, W)
        fx, fy = u - 0.5, v - 0.5
        x0, y0 = fx.floor(), fy.floor()
        tx, ty = fx - x0, fy - y0
        ok = usable & (x0 >= 0) & (x0 <= W - 2) & (y0 >= 0) & (y0 <= H - 2)
        zero = torch.zeros_like(x0)
        at = torch.where(ok, y0, zero).long() * W + torch.where(ok, x0, zero).long()
        src, last = self.img[sv].reshape(-1), H * W - 1
        b00, b10 = src[at], src[(at + 1).clamp(max=last)]
        b01, b11 = src[(at + W).clamp(max=last)], src[(at + W + 1).clamp(max=last)]
        r0 = b00 + tx * (b10 - b00)
        r1 = b01 + tx * (b11 - b01)
        b = r0 + ty * (r1 - r0)
        return torch.where(ok & torch.isfinite(b), b, torch.full_like(b, math.nan))

    def correlate(self, total, count, da, b, va, ok):
        """step 4 of THE SWEEP RULE and a source's share of step 5: the NCC of the samples b against the a_i - ma `da` -- both in tap
        order; da a list that the sweep forms once, or a generator that subtracts per tap -- joins (total, count) where it is valid"""
        sb = _tap_sum(b)
        mb = sb / self.n
        vb, cov = torch.zeros_like(sb), torch.zeros_like(sb)
        for dai, bi in zip(da, b):
            db = bi - mb
            vb = vb + db * db
            cov = cov + dai * db
        valid = ok & ~torch.isnan(sb) & ~(vb < self.min_var)
        ncc = cov / _sqrt_rn(va * vb)
        return torch.where(valid, total + ncc, total), count + valid

    def score(self, r, py, px, d, n):
        """THE PLANE SCORE of (d [N], n [N, 3]) at the pixels (px, py) (int64 [N]) of reference r -> float32 [N]"""
        nan = torch.full(py.shape, math.nan, dtype=torch.float32, device=self.dev)
        ref = self.reference(r)
        if ref is None:
            return nan
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        gp = (nx * ref["xn"][px] + ny * ref["yn"][py]) + nz
        ok = ref["pixel_ok"][py, px] & torch.isfinite(d) & (d > 0) & torch.isfinite(nx) & torch.isfinite(ny) & torch.isfinite(nz) & (gp < 0)
        h = gp * d
        a, pts = [], []
        for dx, dy in self.offsets:
            qx, qy = (px + dx).clamp(0, self.W - 1), (py + dy).clamp(0, self.H - 1)
            xq, yq = ref["xn"][qx], ref["yn"][qy]
            gq = (nx * xq + ny * yq) + nz
            dq = h / gq
            a.append(ref["img"][qy, qx])
            pts.append((xq * dq, yq * dq, dq, (gq < 0) & torch.isfinite(dq)))
        ma, va = ref["ma"][py, px], ref["va"][py, px]
        total, count = torch.zeros_like(nan), torch.zeros(py.shape, dtype=torch.int64, device=self.dev)
        for s, sv in enumerate(self.sources[r]):
            if not 0 <= sv < self.V:
                continue
            b = [torch.where(tap_ok, self.sample(r, s, sv, X, Y, Z), nan) for X, Y, Z, tap_ok in pts]
            total, count = self.correlate(total, count, (ai - ma for ai in a), b, va, ok)
        return torch.where(ok & (count >= self.min_sources), total / count.float(), nan)


@torch.no_grad()
def plane_sweep_torch(images, pose, intr, sources, depths, refs=None, half_width=3, near=1e-3, min_var=1e-6, min_sources=1):
    """THE SWEEP RULE as plain torch ops on the images' device (a CPU works), vectorised over the pixels of one reference, the
    references, planes, sources and taps in loops: the same operations in the same order, each a separate op, so each rounds
    once.  A non-finite or invalid sample is a NaN, and a window's sum is NaN exactly when one of its taps is.  Reads `refs` and
    `sources` on the host.  -> (depth, score, plane) as plane_sweep."""
    sc = _TorchScene(images, pose, intr, sources, refs, half_width, 1, near, min_var, min_sources, "ls2fm.mvs.plane_sweep_torch", depths)
    R, D, H, W, dev, depths = sc.R, sc.D, sc.H, sc.W, sc.dev, sc.depths
    nan = torch.full((H, W), math.nan, dtype=torch.float32, device=dev)
    out_d, out_s = nan.repeat(R, 1, 1), nan.repeat(R, 1, 1)
    out_k = torch.full((R, H, W), -1, dtype=torch.int32, device=dev)
    for r in range(R):
        ref = sc.reference(r)
        if ref is None:
            continue
        # 1. the reference window: a_i - ma once for all planes and sources
        da = [t - ref["ma"] for t in ref["a"]]
        xn, yn = ref["xn"][None, :], ref["yn"][:, None]
        best, before, after, previous = nan, nan, nan, nan
        best_k = torch.full((H, W), -1, dtype=torch.int64, device=dev)
        for k in range(D):
            d = depths[r, k]
            total, count = torch.zeros_like(nan), torch.zeros((H, W), dtype=torch.int64, device=dev)
            # 2. warp: every pixel of the reference is a tap
            X, Y, Z = (xn * d).expand(H, W).reshape(-1), (yn * d).expand(H, W).reshape(-1), d.expand(H * W)
            for s, sv in enumerate(sc.sources[r]):
                if not 0 <= sv < sc.V:
                    continue
                # 3. sample, 4. NCC
                bt = _taps(sc.sample(r, s, sv, X, Y, Z).reshape(H, W), sc.w)
                total, count = sc.correlate(total, count, da, bt, ref["va"], ref["pixel_ok"])
            # 5. aggregate, 6. select
            score = torch.where(count >= sc.min_sources, total / count.float(), nan)
            better = ~torch.isnan(score) & ((best_k < 0) | (score > best))
            follows = ~better & (best_k + 1 == k)
            before = torch.where(better, previous, before)
            after = torch.where(better, nan, torch.where(follows, score, after))
            best = torch.where(better, score, best)
            best_k = torch.where(better, torch.full_like(best_k, k), best_k)
            previous = score
        # 7. refine
        dr = depths[r]
        d0, dn, dp = dr[best_k.clamp(0, D - 1)], dr[(best_k + 1).clamp(0, D - 1)], dr[(best_k - 1).clamp(0, D - 1)]
        den = (before - 2.0 * best) + after
        off = (0.5 * (before - after)) / den
        step = torch.where(off >= 0, dn - d0, d0 - dp)
        refined = torch.where((best_k > 0) & (best_k < D - 1) & (den < 0), d0 + off * step, d0)
        out_d[r] = torch.where(best_k >= 0, refined, nan)
        out_s[r] = best
        out_k[r] = best_k.to(torch.int32)
        sc.cache.clear()                                               # a reference comes once: its taps need not outlive it
    return out_d, out_s, out_k


@torch.no_grad()
def filter_depths_torch(depth, pose, intr, sources, near=1e-3, max_reproj=1.0, rel_depth=0.01, min_consistent=2):
    """THE CONSISTENCY RULE as plain torch ops on the depth maps' device (a CPU works), vectorised over the pixels of one view.
    Reads `sources` on the host.  -> (filtered, count) as filter_depths."""
    who = "ls2fm.mvs.filter_depths_torch"
    depth, P, K = _torch_views(depth, pose, intr)
    V, dev = int(P.shape[0]), depth.device
    depth = _grey(depth, V, who)
    refs, sources, _ = _index_arrays(None, sources, None, V, dev, who)
    S, H, W = int(sources.shape[1]), int(depth.shape[1]), int(depth.shape[2])
    max_reproj, rel_depth, min_consistent = _check_filter(max_reproj, rel_depth, min_consistent, S, who)
    rel, back = relative_poses(P, refs, sources), relative_poses(P, refs, sources, back=True)
    scalar = functools.partial(_scalar, dev=dev)
    near, max_reproj, rel_depth = scalar(_posed.near_plane(near, who)), scalar(max_reproj), scalar(rel_depth)
    reproj2 = max_reproj * max_reproj
    count = torch.zeros((V, H * W), dtype=torch.int64, device=dev)
    centre = lambda n: torch.arange(n, device=dev).float() + 0.5
    uc, vc = centre(W)[None, :].expand(H, W).reshape(-1), centre(H)[:, None].expand(H, W).reshape(-1)
    for r, srcs in enumerate(sources.tolist()):
        d = depth[r].reshape(-1)
        has = torch.isfinite(d) & (d > 0)
        X, Y = ((uc - K[r, 0, 2]) / K[r, 0, 0]) * d, ((vc - K[r, 1, 2]) / K[r, 1, 1]) * d
        dz = rel_depth * d
        for s, sv in enumerate(srcs):
            if not 0 <= sv < V:
                continue
            _, _, _, _, ok, sx, sy = _posed.project_torch(rel[r, s], K[sv], X, Y, d, near, H, W)
            ds = depth[sv].reshape(-1)[sy * W + sx]
            ok = has & ok & torch.isfinite(ds) & (ds > 0)
            Xs = (((sx.float() + 0.5) - K[sv, 0, 2]) / K[sv, 0, 0]) * ds
            Ys = (((sy.float() + 0.5) - K[sv, 1, 2]) / K[sv, 1, 1]) * ds
            c, u, v, usable, _, _, _ = _posed.project_torch(back[r, s], K[r], Xs, Ys, ds, near, H, W)
            du, dv = u - uc, v - vc
            e = du * du + dv * dv
            count[r] += ok & usable & (e <= reproj2) & ((c[2] - d).abs() <= dz)
    flat = depth.reshape(V, -1)
    out = torch.where(count >= min_consistent, flat, torch.full_like(flat, math.nan))
    return out.reshape(V, H, W), count.to(torch.uint8).reshape(V, H, W)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


@torch.no_grad()
def fuse_depths_torch(depth, pose, intr, sources, normal=None, images=None, near=1e-3, max_reproj=1.0, rel_depth=0.01,
                      max_normal_angle=60.0, min_support=1):
    """THE FUSION RULE as plain torch ops on the depth maps' device (a CPU works), vectorised over the pixels of one view: the walk
    in float32, the sums in float64, each operation a separate op.  Reads `sources` and the owners on the host.  -> FusedCloud as
    fuse_depths."""
    who = "ls2fm.mvs.fuse_depths_torch"
    depth, P, K = _torch_views(depth, pose, intr)
    V, dev = int(P.shape[0]), depth.device
    depth = _grey(depth, V, who)
    refs, sources, _ = _index_arrays(None, sources, None, V, dev, who)
    S, H, W = int(sources.shape[1]), int(depth.shape[1]), int(depth.shape[2])
    max_reproj, rel_depth, cos2, min_support = _check_fuse(max_normal_angle, min_support, max_reproj, rel_depth, S, who)
    normal, colour = _fuse_maps(normal, images, V, H, W, dev, who)
    if V == 0:
        return _no_cloud(normal, colour, dev)
    rel, back = relative_poses(P, refs, sources), relative_poses(P, refs, sources, back=True)
    to_world = cam_to_world(P)
    M64 = to_world.double()
    scalar = functools.partial(_scalar, dev=dev)
    near, max_reproj, rel_depth, cos2 = scalar(_posed.near_plane(near, who)), scalar(max_reproj), scalar(rel_depth), scalar(cos2)
    reproj2 = max_reproj * max_reproj
    centre = lambda n: torch.arange(n, device=dev).float() + 0.5
    uc, vc = centre(W)[None, :].expand(H, W).reshape(-1), centre(H)[:, None].expand(H, W).reshape(-1)
    flat = depth.reshape(V, -1)
    nflat = None if normal is None else normal.reshape(V, H * W, 3)
    cflat = None if colour is None else colour.reshape(V, H * W, -1)

    def world(v, X, Y, d):
        m, X, Y, d = M64[v], X.double(), Y.double(), d.double()
        return [((m[i, 0] * X + m[i, 1] * Y) + m[i, 2] * d) + m[i, 3] for i in range(3)]

    def unit(v, n):
        m, n = M64[v], n.double()
        g = [(m[i, 0] * n[:, 0] + m[i, 1] * n[:, 1]) + m[i, 2] * n[:, 2] for i in range(3)]
        length = torch.sqrt(_dot3(g, g))
        return [gi / length for gi in g]

    rows = dict(points=[], normals=[], colours=[], support=[], pixel=[])
    for r, srcs in enumerate(sources.tolist()):
        d = flat[r]
        has = torch.isfinite(d) & (d > 0)
        X, Y = ((uc - K[r, 0, 2]) / K[r, 0, 0]) * d, ((vc - K[r, 1, 2]) / K[r, 1, 1]) * d
        dz = rel_depth * d
        count, lower = torch.zeros(H * W, dtype=torch.int64, device=dev), torch.zeros(H * W, dtype=torch.bool, device=dev)
        point = [torch.zeros(H * W, dtype=torch.float64, device=dev) + w for w in world(r, X, Y, d)]
        if nflat is not None:
            nr = [nflat[r][:, j] for j in range(3)]
            rr = _dot3(nr, nr)
            nsum = [torch.zeros(H * W, dtype=torch.float64, device=dev) + g for g in unit(r, nflat[r])]
        if cflat is not None:
            csum = torch.zeros_like(cflat[r], dtype=torch.float64) + cflat[r].double()
        for s, sv in enumerate(srcs):
            if not 0 <= sv < V or sv == r:
                continue
            _, _, _, _, ok, sx, sy = _posed.project_torch(rel[r, s], K[sv], X, Y, d, near, H, W)
            at = sy * W + sx
            ds = flat[sv][at]
            ok = has & ok & torch.isfinite(ds) & (ds > 0)
            Xs = (((sx.float() + 0.5) - K[sv, 0, 2]) / K[sv, 0, 0]) * ds
            Ys = (((sy.float() + 0.5) - K[sv, 1, 2]) / K[sv, 1, 1]) * ds
            c, u, v, usable, _, _, _ = _posed.project_torch(back[r, s], K[r], Xs, Ys, ds, near, H, W)
            du, dv = u - uc, v - vc
            e = du * du + dv * dv
            good = ok & usable & (e <= reproj2) & ((c[2] - d).abs() <= dz)
            if nflat is not None:
                ns, B = nflat[sv][at], back[r, s]
                turned = [(B[i, 0] * ns[:, 0] + B[i, 1] * ns[:, 1]) + B[i, 2] * ns[:, 2] for i in range(3)]
                a = _dot3(nr, turned)
                good = good & (a > 0) & (a * a >= cos2 * (rr * _dot3(turned, turned)))
            count += good
            lower |= good & (sv < r)
            for i, w in enumerate(world(sv, Xs, Ys, ds)):
                point[i] = torch.where(good, point[i] + w, point[i])
            if nflat is not None:
                for i, g in enumerate(unit(sv, nflat[sv][at])):
                    nsum[i] = torch.where(good, nsum[i] + g, nsum[i])
            if cflat is not None:
                csum = torch.where(good[:, None], csum + cflat[sv][at].double(), csum)
        owner = has & ~lower
        n = (1 + count[owner]).double()
        rows["support"].append((1 + count[owner]).to(torch.uint8))
        rows["points"].append(torch.stack([p[owner] / n for p in point], dim=1).float())
        if nflat is not None:
            t = [g[owner] for g in nsum]
            length = torch.sqrt(_dot3(t, t))
            rows["normals"].append(torch.stack([ti / length for ti in t], dim=1).float())
        if cflat is not None:
            rows["colours"].append((csum[owner] / n[:, None]).float())
        rows["pixel"].append(r * H * W + torch.nonzero(owner)[:, 0])
    cat = lambda name, shape, dtype: (torch.cat(rows[name]) if rows[name] else torch.zeros(0, dtype=dtype, device=dev)).reshape(shape)
    return _fused_cloud(cat("points", (-1, 3), torch.float32), None if nflat is None else cat("normals", (-1, 3), torch.float32),
                        None if cflat is None else cat("colours", (-1, cflat.shape[2]), torch.float32),
                        cat("support", (-1,), torch.uint8), cat("pixel", (-1,), torch.int64), to_world, H, W, min_support)


def _mix(x):
    """mix of THE DRAWS on int64 tensors that hold 32-bit values: both constants are below 2^31, so no product leaves 63 bits"""
    m = 0xFFFFFFFF
    x = x & m
    x = x ^ (x >> 16)
    x = (x * MIX_A) & m
    x = x ^ (x >> 15)
    x = (x * MIX_B) & m
    return x ^ (x >> 15)


def _draws(seed, view, iteration, pixel):
    """u_0 .. u_8 float32 of the pixels `pixel` (int64, py W + px) of view `view`"""
    h = _mix(torch.full_like(pixel[:1], (int(seed) + MIX_SALT) & 0xFFFFFFFF))
    h = _mix(_mix(h + int(view)) + int(iteration))
    key = _mix(h + pixel)
    return [(_mix(key + j) >> 8).float() * 2.0 ** -24 for j in range(PM_DRAWS)]


def _normalise(x, y, z):
    root = _sqrt_rn((x * x + y * y) + z * z)
    return torch.stack([x / root, y / root, z / root], dim=1)


@torch.no_grad()
def plane_score_torch(images, pose, intr, sources, depth, normal, refs=None, half_width=3, tap_step=1, near=1e-3, min_var=1e-6,
                      min_sources=1):
    """THE PLANE SCORE as plain torch ops on the images' device (a CPU works), vectorised over the pixels of one reference, the
    references, sources and taps in loops: the same operations in the same order, each a separate op.  Reads `refs` and `sources`
    on the host.  -> score as plane_score."""
    who = "ls2fm.mvs.plane_score_torch"
    sc = _TorchScene(images, pose, intr, sources, refs, half_width, tap_step, near, min_var, min_sources, who)
    depth, normal, _ = _state(depth, normal, None, sc.R, sc.H, sc.W, sc.dev, who, False)
    yy, xx = torch.meshgrid(torch.arange(sc.H, device=sc.dev), torch.arange(sc.W, device=sc.dev), indexing="ij")
    py, px = yy.reshape(-1), xx.reshape(-1)
    return torch.stack([sc.score(r, py, px, depth[r].reshape(-1), normal[r].reshape(-1, 3)).reshape(sc.H, sc.W) for r in range(sc.R)])


@torch.no_grad()
def patch_match_step_torch(images, pose, intr, sources, depth, normal, score, colour, iteration, d_min, d_max, refs=None, seed=0,
                           depth_perturb=0.02, normal_perturb=0.5, max_slope=1.0, half_width=3, tap_step=1, near=1e-3, min_var=1e-6,
                           min_sources=1):
    """THE PATCHMATCH STEP as plain torch ops on the images' device (a CPU works), the hash in int64 ops masked to 32 bits; in place
    on contiguous float32 tensors like patch_match_step.  Every candidate is scored at every pixel of the colour and masked.  Reads
    `refs` and `sources` on the host.  -> (depth, normal, score)."""
    who = "ls2fm.mvs.patch_match_step_torch"
    sc = _TorchScene(images, pose, intr, sources, refs, half_width, tap_step, near, min_var, min_sources, who)
    colour, iteration, rho_d, rho_n, sigma = _check_step(colour, iteration, depth_perturb, normal_perturb, max_slope, who)
    rho_d, rho_n, sigma = sc.scalar(rho_d), sc.scalar(rho_n), sc.scalar(sigma)
    depth, normal, score = _state(depth, normal, score, sc.R, sc.H, sc.W, sc.dev, who, True)
    d_min, d_max = _range(d_min, d_max, sc.R, sc.dev, who)
    H, W, w = sc.H, sc.W, sc.w
    yy, xx = torch.meshgrid(torch.arange(w, H - w, device=sc.dev), torch.arange(w, W - w, device=sc.dev), indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    mine = ((xx + yy) & 1) == colour
    py, px = yy[mine], xx[mine]
    if py.numel() == 0:
        return depth, normal, score
    one = sc.scalar(1.0)
    for r in range(sc.R):
        ref = sc.reference(r)
        if ref is None:
            continue
        best = [depth[r][py, px], normal[r][py, px], score[r][py, px]]
        u = _draws(seed, ref["rv"], iteration, py * W + px)
        xp, yp = ref["xn"][px], ref["yn"][py]

        def consider(cd, cn, active):
            s = sc.score(r, py, px, cd, cn)
            better = active & ~torch.isnan(s) & (torch.isnan(best[2]) | (s > best[2]))
            best[0] = torch.where(better, cd, best[0])
            best[1] = torch.where(better[:, None], cn, best[1])
            best[2] = torch.where(better, s, best[2])

        for dx, dy in NEIGHBOURS:
            mx, my = px + dx, py + dy
            inside = (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
            mx, my = mx.clamp(0, W - 1), my.clamp(0, H - 1)
            dm, nm = depth[r][my, mx], normal[r][my, mx]
            gm = (nm[:, 0] * ref["xn"][mx] + nm[:, 1] * ref["yn"][my]) + nm[:, 2]
            g = (nm[:, 0] * xp + nm[:, 1] * yp) + nm[:, 2]
            consider((gm * dm) / g, nm, inside & torch.isfinite(dm) & (dm > 0))
        have = ~torch.isnan(best[2])
        deeper = lambda j: best[0] * (one + rho_d * (2.0 * u[j] - 1.0))
        turned = lambda j: _normalise(best[1][:, 0] + rho_n * (2.0 * u[j] - 1.0), best[1][:, 1] + rho_n * (2.0 * u[j + 1] - 1.0), best[1][:, 2])
        consider(deeper(0), best[1], have)
        consider(best[0], turned(1), have)
        consider(deeper(3), turned(4), have)
        lo, hi = one / d_min[r], one / d_max[r]
        fresh = _normalise(sigma * (2.0 * u[7] - 1.0), sigma * (2.0 * u[8] - 1.0), torch.full_like(u[7], -1.0))
        consider(one / (lo + u[6] * (hi - lo)), fresh, torch.ones_like(have))
        depth[r][py, px], normal[r][py, px], score[r][py, px] = best
    return depth, normal, score


# ------------------------------------------------------------------------------------------------------------------ end to end
@torch.no_grad()
def dense_reconstruct(images, pose, intr, bounds, voxel, sources=None, depths=None, points=None, options=None, trunc=None,
                      min_weight=1.0, return_depth=False, stereo="sweep", surface="tsdf"):
    """Photographs to a surface: plane_sweep (stereo="sweep", the default) or patch_match (stereo="patchmatch") over every view ->
    filter_depths -> ls2fm.fusion.volume_for(bounds, voxel, trunc) -> fusion.integrate -> fusion.extract -> ls2fm.mesh.Mesh, in the
    poses' world frame.  With surface="poisson" or "mls" the depth maps go through the cloud instead of the volume: filter_depths ->
    fuse_depths -> ls2fm.cloud_mesh.mesh_from_cloud(method=surface, voxel=voxel, bounds=bounds), with patch_match's normals, or for
    the sweep, which has none, with normals estimated toward each point's camera; trunc and min_weight are the volume's and unused;
    with return_depth the FusedCloud is appended to the result.
      images     [V, H, W, 3] colour (to_grey) or grey [V, H, W]
      sources    int [V, S]; default select_sources(pose, options.n_sources, options.min_angle, options.max_angle)
      depths     float [V, D]; default depth_planes over depth_range_from_points of `points` (an [N, 3] cloud or an
                 ls2fm.mapper.Reconstruction), or of the eight corners of `bounds` when there are none; options.n_planes of them
                 for the sweep, options.patchmatch_planes for patch_match's initial sweep
      options    MvsOptions
    Host reads: those of fusion.extract.  With return_depth: (Mesh, filtered depth [V, H, W], count uint8 [V, H, W]), and with
    stereo="patchmatch" a fourth entry, the world normals [V, H, W, 3] (normals_to_world), NaN where the filter dropped the pixel."""
    opt = MvsOptions() if options is None else options
    if stereo not in ("sweep", "patchmatch"):
        raise ValueError(f"ls2fm.mvs.dense_reconstruct: stereo {stereo!r} must be 'sweep' or 'patchmatch'")
    if surface not in ("tsdf", "poisson", "mls"):
        raise ValueError(f"ls2fm.mvs.dense_reconstruct: surface {surface!r} must be 'tsdf', 'poisson' or 'mls'")
    images = torch.as_tensor(images)
    _device(images, torch.as_tensor(pose), torch.as_tensor(intr))
    grey = to_grey(images)
    if sources is None:
        sources = select_sources(pose, opt.n_sources, opt.min_angle, opt.max_angle)
    if depths is None:
        if points is None:
            lo, hi = ([float(v) for v in b] for b in bounds)
            points = torch.tensor([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=torch.float64)
        near, far = depth_range_from_points(points, pose, opt.margin)
        depths = depth_planes(near, far, opt.n_planes if stereo == "sweep" else opt.patchmatch_planes, opt.inverse_depth)
    if stereo == "sweep":
        depth, _, _ = plane_sweep(grey, pose, intr, sources, depths, **opt.sweep())
    else:
        depth, normal, _ = patch_match(grey, pose, intr, sources, depths, **opt.patchmatch())
    filtered, count = filter_depths(depth, pose, intr, sources, **opt.filter())
    fused = ()
    if surface == "tsdf":
        volume = fusion.volume_for(bounds, voxel, trunc, grey.device)
        fusion.integrate(volume, filtered, pose, intr, near=opt.near)
        out = fusion.extract(volume, min_weight)
    else:
        from . import cloud_mesh
        cloud = fuse_depths(filtered, pose, intr, sources, normal=None if stereo == "sweep" else normal,
                            images=images if images.dim() == 4 else grey, **opt.fuse())
        out = cloud_mesh.mesh_from_cloud(cloud.points, normals=cloud.normals, toward=cloud.centers, voxel=voxel, method=surface,
                                         bounds=bounds)
        fused = (cloud,)
    if not return_depth:
        return out
    if stereo == "sweep":
        return (out, filtered, count) + fused
    world = normals_to_world(normal, pose)
    return (out, filtered, count, world.masked_fill(torch.isnan(filtered)[..., None], math.nan)) + fused
