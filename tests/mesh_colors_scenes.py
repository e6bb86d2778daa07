"""Deterministic scenes for the vertex-colour tests (numpy only).

sphere_scene(): where THE VERTEX COLOUR RULE is judged by its properties (tests/test_mesh_colors_host.py), so that the GPU tests
can be exact comparisons against the restatement.  A marching-cubes sphere of radius r = 0.5 (tests/mc_restate.py on a 24^3
lattice of |x| - 0.5 over [-1, 1]^3: cells of 0.087), six cameras on the axes at distance D = 2.5 looking at the centre, one
constant colour per view.  The chosen values, by the tan(theta) / f_px reasoning of DESIGN 3.19:
  f_px = 160, images 96 x 96, principal point (48, 48): the silhouette has radius f r / sqrt(D^2 - r^2) = 32.7 px, inside the image.
  depth_tol = 0.02.  The relative depth change across one pixel on a surface inclined by theta is tan(theta) / f_px, and a vertex
    lies at most 0.71 px from its pixel's centre, where the depth map was taken.  Judged as seen: cos >= 0.5, theta <= 60 deg,
    with the facets of a 0.087 cell on a 0.5 sphere turning the surface by up to ~5 deg more: tan(65 deg) / 160 * 0.71 = 0.0095,
    half the tolerance.  Judged as hidden: cos <= -0.2 on the far side; the ray through such a vertex met the near side a chord
    2 r 0.2 = 0.2 earlier, 0.08 of the depth, and the near side there (cos = 0.2, theta = 78 deg) changes by
    tan(78 deg) / 160 * 0.71 = 0.021 across the pixel: the gap left, 0.059, is three times the tolerance.
  The band -0.2 < cos < 0.5 (the limb, where one pixel spans the tolerance) is left unjudged: 0.35 of the sphere's area.

edge_scene(H, W, C): the edge cases of the rule for the bit-for-bit GPU tests, in an H x W image of C channels (see there)."""
import functools

import numpy as np

import mc_restate
import mesh_colors_restate as MR
import raster_restate as R
from raster_scenes import IDENTITY, intrinsics, look_at, unproject

F32 = np.float32

SPHERE_F, SPHERE_HW, SPHERE_TOL, SPHERE_D = 160.0, 96, 0.02, 2.5
SPHERE_COLORS = np.array([[0.9, 0.1, 0.2], [0.1, 0.8, 0.3], [0.2, 0.3, 0.95], [0.85, 0.8, 0.1], [0.1, 0.75, 0.8], [0.7, 0.15, 0.9]], F32)


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """dict(verts, faces, normals (the sphere's own, unit), poses [6, 3, 4], eyes [6, 3], intr, H, W, images [6, H, W, 3], near,
    depth_tol, depth float32 [6, H, W] (the restatement's rasterisation)); callers do not write into it"""
    n = 24
    ax = np.linspace(-1.0, 1.0, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (np.sqrt(X * X + Y * Y + Z * Z) - 0.5).astype(F32)
    sp = 2.0 / (n - 1)
    verts, faces = mc_restate.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-1.0, -1.0, -1.0))
    eyes = np.array([[SPHERE_D, 0, 0], [-SPHERE_D, 0, 0], [0, SPHERE_D, 0], [0, -SPHERE_D, 0], [0, 0, SPHERE_D], [0, 0, -SPHERE_D]], np.float64)
    poses = np.stack([look_at(e, (0, 0, 0), up=(0.0, 0.0, 1.0) if e[1] != 0 else (0.0, 1.0, 0.0)) for e in eyes])
    K = intrinsics(SPHERE_F, SPHERE_HW / 2, SPHERE_HW / 2)
    H = W = SPHERE_HW
    images = np.broadcast_to(SPHERE_COLORS[:, None, None, :], (6, H, W, 3)).astype(F32).copy()
    normals = (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(F32)
    depth = R.rasterize(verts, faces, poses, K, H, W, 1e-3)["depth"]
    return dict(verts=verts, faces=faces, normals=normals, poses=poses, eyes=eyes, intr=K, H=H, W=W, images=images, near=1e-3,
                depth_tol=SPHERE_TOL, depth=depth)


def sphere_cosines(sc, view):
    """cos of the angle between each vertex's normal and the direction from the vertex to the camera (float64 [V])"""
    to_cam = sc["eyes"][view][None, :] - sc["verts"].astype(np.float64)
    to_cam /= np.linalg.norm(to_cam, axis=1, keepdims=True)
    return (sc["normals"].astype(np.float64) * to_cam).sum(axis=1)


@functools.lru_cache(maxsize=None)
def sphere_single_views():
    """the restatement's answer for each of the six views alone, without normals (every weight 1)"""
    sc = sphere_scene()
    return [MR.vertex_colors(sc["verts"], sc["poses"][i:i + 1], sc["intr"], sc["images"][i:i + 1], sc["depth"][i:i + 1],
                             near=sc["near"], depth_tol=sc["depth_tol"]) for i in range(6)]


# ------------------------------------------------------------------------------------------------------------------ edge cases
EDGE_TOL = 0.25          # exact in fp32: a front quad at depth 1 puts the threshold d + depth_tol d at exactly 1.25
EDGE_NEAR = 0.5
EDGE_NAMES = ["u_zero", "u_width", "pixel_centre", "last_column", "last_row", "last_corner", "first_corner", "behind_near",
              "nan_vertex", "nan_pixel", "facing_away", "at_threshold", "past_threshold", "occluded", "masked"]


@functools.lru_cache(maxsize=None)
def edge_scene(H, W, C, n_verts=257, n_views=3):
    """Under the identity pose of view 0 with fx = fy = 8, cx = cy = 0, a point (u, v) of the plane z = 2 is (u / 4, v / 4, 2):
    exact in fp32 for u, v on the 1 / 8 grid.  The mesh: a background quad over the plane z = 2, 16 pixels larger than the image on every side (no view has a corner of it behind its
    near plane: such a face is not drawn), and a
    front quad at z = 1 over the pixels [W // 2, W - 2] x [H // 2, H - 2].  The coloured points are NOT the mesh's vertices (the kernel takes the
    two apart): the first len(EDGE_NAMES) are the named cases below, the rest a lattice of plane points, some pulled in front of
    the plane, some pushed behind it.  Views 1 and 2 look at the plane from further back, slightly turned.
    -> dict(points float32 [n_verts, 3], normals float32 [n_verts, 3], mesh_verts, faces, poses, intr, images [N, H, W, C],
    masks uint8 [N, H, W], depth float32 [N, H, W] (the restatement's), near, depth_tol, index: name -> row of points)"""
    K = intrinsics(8.0, 0.0, 0.0)
    on_plane = lambda u, v, z=2.0: unproject(u, v, z, K)
    mesh_verts, faces = [], []
    big = [on_plane(-16.0, -16.0), on_plane(W + 16.0, -16.0), on_plane(W + 16.0, H + 16.0), on_plane(-16.0, H + 16.0)]
    mesh_verts += big
    faces += [[0, 1, 2], [0, 2, 3]]
    fx0, fx1, fy0, fy1 = W // 2, W - 1, H // 2, H - 1          # front quad: whole pixels, so the pixels it covers are known
    mesh_verts += [on_plane(fx0, fy0, 1.0), on_plane(fx1, fy0, 1.0), on_plane(fx1, fy1, 1.0), on_plane(fx0, fy1, 1.0)]
    faces += [[4, 5, 6], [4, 6, 7]]
    mid_u, mid_v = (fx0 + fx1) / 2.0 + 0.125, (fy0 + fy1) / 2.0 + 0.125            # inside the front quad, off the pixel centres
    cu, cv = float(min(2, W - 1)) + 0.5, float(min(1, H - 1)) + 0.5                # a pixel centre outside the front quad
    named = dict(
        u_zero=on_plane(0.0, 1.25), u_width=on_plane(float(W), 1.25), pixel_centre=on_plane(cu, cv),
        last_column=on_plane(W - 0.25, 1.375), last_row=on_plane(1.375, H - 0.25), last_corner=on_plane(W - 0.125, H - 0.125),
        first_corner=on_plane(0.125, 0.25), behind_near=[0.01, 0.01, EDGE_NEAR / 2], nan_vertex=[np.nan, 0.25, 2.0],
        nan_pixel=on_plane(W - 1.5 + 0.25, 0.75), facing_away=on_plane(1.625, 2.25),
        at_threshold=on_plane(mid_u, mid_v, 1.25), past_threshold=on_plane(mid_u, mid_v, float(np.nextafter(F32(1.25), F32(2)))),
        occluded=on_plane(mid_u - 0.25, mid_v, 1.5), masked=on_plane(cu + 1.25, cv + 0.25))
    points = [named[k] for k in EDGE_NAMES]
    i = 0
    while len(points) < n_verts:
        u, v = (i * 0.625) % (W + 2.0) - 1.0, ((i * 7) % (8 * H + 16)) / 8.0 - 1.0
        z = 2.0 if i % 5 else (1.75 if i % 10 else 2.5)
        points.append(on_plane(u, v, z))
        i += 1
    points = np.array(points[:n_verts], F32).reshape(-1, 3)
    rng = np.random.default_rng(7)
    normals = np.tile(np.array([0.0, 0.0, -1.0], F32), (len(points), 1))
    tilt = np.arange(len(points)) % 3 == 1
    normals[tilt] += rng.uniform(-0.8, 0.8, (int(tilt.sum()), 3)).astype(F32)
    index = {k: j for j, k in enumerate(EDGE_NAMES) if j < n_verts}
    if "facing_away" in index:
        normals[index["facing_away"]] = [0.0, 0.0, 1.0]
    mx, my = W / 8.0, H / 8.0                                                      # the middle of the image's part of the plane
    poses = np.stack([IDENTITY, look_at((mx + 0.4, my + 0.2, -1.0), (mx, my, 2.0)), look_at((mx - 0.7, my + 0.3, -0.5), (mx + 0.2, my, 2.0))])[:n_views]
    # views 1 and 2 are centred: their principal point is the image's middle
    Ks = np.stack([K, intrinsics(8.0, W / 2.0, H / 2.0), intrinsics(6.0, W / 2.0, H / 2.0)])[:n_views]
    N = len(poses)
    images = rng.uniform(0.0, 1.0, (N, H, W, C)).astype(F32)
    masks = np.ones((N, H, W), np.uint8)
    if N:
        images[0, 0, W - 2, C - 1] = np.nan                                     # a tap of nan_pixel in view 0
        masks[0, int(cv), int(cu + 1.25)] = 0                                   # exactly `masked`'s pixel in view 0
        masks[N - 1, H // 2:, : W // 2] = 0
    depth = R.rasterize(mesh_verts, faces, poses, Ks, H, W, EDGE_NEAR)["depth"] if N else np.zeros((0, H, W), F32)
    return dict(points=points, normals=normals, mesh_verts=np.array(mesh_verts, F32), faces=np.array(faces, np.int32), poses=poses,
                intr=Ks, images=images, masks=masks, depth=depth, near=EDGE_NEAR, depth_tol=EDGE_TOL, index=index)
