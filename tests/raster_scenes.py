"""Deterministic scenes for the rasteriser tests (numpy only; at most 3 views, a few thousand faces, images of 47 x 61, 48 x 64 and
1 x 1), each built to break one way a rasteriser goes wrong.  scenes() -> name -> dict(verts float32 [n, 3], faces int32 [F, 3],
poses float32 [N, 3, 4], intr float32 [3, 3], H, W, near).  expected(name) is the restatement's answer (tests/raster_restate.py)
with its per-pixel counts, computed once and shared; callers do not write into it.  tests/test_raster_host.py asserts, per scene,
the condition under which a wrong kernel fails it."""
import functools
import os
import re

import numpy as np

import raster_restate as R

F32 = np.float32
NAMES = ["sphere", "quad_centres", "ties", "rejects", "sizes", "one_pixel"]
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)


def lane_pixels():
    """LS2FM_RASTER_LANE_PIXELS of include/ls2fm.h"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ls2fm.h")).read()
    return int(re.search(r"#define\s+LS2FM_RASTER_LANE_PIXELS\s+(\d+)", header).group(1))


def intrinsics(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], F32)


K64 = intrinsics(64.0, 32.0, 24.0)                 # 48 x 64; powers of two, so pixel centres are exact (unproject)
K61 = intrinsics(57.0, 30.5, 23.5)                 # 47 x 61


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """world-to-camera [R | t] float32 [3, 4]: the camera at eye, its z axis toward target"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    return np.concatenate([Rm, -(Rm @ eye)[:, None]], axis=1).astype(F32)


def unproject(u, v, z, K):
    """the camera-frame point that the identity pose projects to (u, v) at depth z (float64)"""
    return [(u - float(K[0, 2])) / float(K[0, 0]) * z, (v - float(K[1, 2])) / float(K[1, 1]) * z, z]


def uv_sphere(stacks=12, slices=24, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """a closed UV sphere: verts float32 [2 + (stacks - 1) slices, 3], faces int32 [2 slices (stacks - 1), 3], outward winding"""
    verts = [[0.0, 0.0, radius]]
    for i in range(1, stacks):
        t = np.pi * i / stacks
        for j in range(slices):
            p = 2 * np.pi * j / slices
            verts.append([radius * np.sin(t) * np.cos(p), radius * np.sin(t) * np.sin(p), radius * np.cos(t)])
    verts.append([0.0, 0.0, -radius])
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    faces = []
    for j in range(slices):
        faces.append([0, ring(1, j), ring(1, j + 1)])
    for i in range(1, stacks - 1):
        for j in range(slices):
            faces.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            faces.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    last = len(verts) - 1
    for j in range(slices):
        faces.append([last, ring(stacks - 1, j + 1), ring(stacks - 1, j)])
    return (np.array(verts) + np.asarray(centre)).astype(F32), np.array(faces, np.int32)


def _scene(verts, faces, poses, intr, H, W, near=1e-3):
    return dict(verts=np.asarray(verts, F32).reshape(-1, 3), faces=np.asarray(faces, np.int32).reshape(-1, 3),
                poses=np.asarray(poses, F32).reshape(-1, 3, 4), intr=np.asarray(intr, F32), H=H, W=W, near=near)


def _sphere():
    """closed 12 x 24 sphere from three views: in front, oblique, and from inside (faces behind and across the near plane)"""
    v, f = uv_sphere()
    poses = [look_at((0.0, 0.0, -3.2), (0, 0, 0)), look_at((2.2, 1.1, -2.0), (0.1, 0, 0)), look_at((0.3, 0.1, 0.0), (0.3, 0.2, 1.0))]
    return _scene(v, f, poses, intrinsics(60.0, 32.0, 24.0), 48, 64)


def quad(x0, y0, x1, y1, z, K, diagonal, wind_first, wind_second):
    """two triangles over the pixel-space rectangle [x0, x1] x [y0, y1] at depth z: split along diagonal 0 (corner 0 - corner 2)
    or 1 (corner 1 - corner 3); wind_* reverse the vertex order of either triangle.  -> (4 verts, 2 faces)"""
    corners = [unproject(x0, y0, z, K), unproject(x1, y0, z, K), unproject(x1, y1, z, K), unproject(x0, y1, z, K)]
    tris = [[0, 1, 2], [0, 2, 3]] if diagonal == 0 else [[0, 1, 3], [1, 2, 3]]
    if wind_first:
        tris[0] = tris[0][::-1]
    if wind_second:
        tris[1] = tris[1][::-1]
    return corners, tris


QUAD_VARIANTS = [(0, False, False), (0, True, True), (0, False, True), (1, False, False), (1, True, False), (1, True, True)]


def _add(verts, faces, v, f):
    base = len(verts)
    verts += list(v)
    faces += [[base + i for i in t] for t in f]


def _quad_centres():
    """a 3 x 2 arrangement of 8 x 8 quads whose corners lie exactly on pixel centres of the plane z = 2, sharing their edges, in all
    the windings and diagonals of QUAD_VARIANTS: every pixel centre on a shared edge or corner must go to exactly one face"""
    verts, faces = [], []
    for i, (d, a, b) in enumerate(QUAD_VARIANTS):
        x0, y0 = 8.5 + 8 * (i % 3), 8.5 + 8 * (i // 3)
        _add(verts, faces, *quad(x0, y0, x0 + 8, y0 + 8, 2.0, K64, d, a, b))
    return _scene(verts, faces, [IDENTITY], K64, 48, 64)


def _ties():
    """the plane z = 2 of quad_centres' camera: a face and its duplicate (the lowest index wins), the duplicate again with its vertices
    rotated, two coplanar overlapping faces listed with the higher index first in memory order of their vertices, and two
    interpenetrating triangles that cross inside the image (per-pixel depth decides); a second view looks at them obliquely"""
    verts, faces = [], []
    tri = [unproject(4.5, 4.5, 2.0, K64), unproject(28.5, 6.5, 2.0, K64), unproject(10.5, 20.5, 2.0, K64)]
    _add(verts, faces, tri, [[0, 1, 2], [0, 1, 2], [1, 2, 0], [2, 1, 0]])
    a = [unproject(30.5, 4.5, 2.0, K64), unproject(60.5, 4.5, 2.0, K64), unproject(30.5, 30.5, 2.0, K64)]
    b = [unproject(40.5, 2.5, 2.0, K64), unproject(62.5, 20.5, 2.0, K64), unproject(34.5, 28.5, 2.0, K64)]
    _add(verts, faces, a, [[0, 1, 2]])
    _add(verts, faces, b, [[0, 1, 2]])
    p = [unproject(6.0, 26.0, 1.5, K64), unproject(40.0, 28.0, 2.5, K64), unproject(20.0, 45.0, 2.0, K64)]
    q = [unproject(8.0, 44.0, 2.4, K64), unproject(36.0, 24.0, 1.6, K64), unproject(38.0, 46.0, 2.0, K64)]
    _add(verts, faces, p, [[0, 1, 2]])
    _add(verts, faces, q, [[0, 1, 2]])
    return _scene(verts, faces, [IDENTITY, look_at((1.0, 0.4, -0.5), (0.0, 0.0, 2.0))], K64, 48, 64)


REJECT_NEAR = 0.5


def _rejects():
    """near = 0.5 under the identity pose (so camera z is the vertex's own z, exactly), 47 x 61.  One triangle per way a face is
    not drawn, and the drawn neighbours of each: see the comments.  A second view turns the camera so that other faces fall behind."""
    K = K61
    verts, faces = [], []
    tri = lambda u, v, z, s=6.0: [unproject(u, v, z, K), unproject(u + s, v + 0.5, z, K), unproject(u + 1.0, v + s, z, K)]
    below = float(np.nextafter(F32(REJECT_NEAR), F32(0)))
    t = tri(5.2, 5.3, 1.0)
    t[0] = unproject(5.2, 5.3, REJECT_NEAR, K)                     # c_z exactly near: usable, drawn
    _add(verts, faces, t, [[0, 1, 2]])
    t = tri(15.2, 5.3, 1.0)
    t[0] = unproject(15.2, 5.3, below, K)                          # one ulp below near: not drawn
    _add(verts, faces, t, [[0, 1, 2]])
    _add(verts, faces, tri(25.2, 5.3, -1.0), [[0, 1, 2]])          # wholly behind the camera
    t = tri(35.2, 5.3, 1.0)
    t[2] = [0.1, 0.1, -0.2]                                        # one vertex behind the camera
    _add(verts, faces, t, [[0, 1, 2]])
    t = tri(45.2, 5.3, 1.0)
    t[1] = [0.0, 0.0, 0.0]                                         # c_z = 0: u, v are NaN or infinite
    _add(verts, faces, t, [[0, 1, 2]])
    for bad in ([np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, np.inf], [0.0, 0.0, -np.inf], [np.nan] * 3, [3e38, 0.0, 1.0]):
        t = tri(5.2, 15.3, 1.0)
        t[1] = bad                                                 # NaN and infinite coordinates
        _add(verts, faces, t, [[0, 1, 2]])
    t = tri(15.2, 15.3, 1.0)
    t[1] = unproject(70000.0, 15.0, 1.0, K)                        # |u| > 65536
    _add(verts, faces, t, [[0, 1, 2]])
    t = tri(15.2, 15.3, 1.0)
    t[2] = unproject(15.0, -70000.0, 1.0, K)                       # |v| > 65536
    _add(verts, faces, t, [[0, 1, 2]])
    t = tri(25.2, 15.3, 1.2)
    t[1] = unproject(60000.0, 15.0, 1.2, K)                        # |u| < 65536: drawn, and clipped by the image
    _add(verts, faces, t, [[0, 1, 2]])
    n = len(verts)
    _add(verts, faces, tri(35.2, 15.3, 1.0), [[0, 1, 2]])
    faces += [[n, n + 1, -1], [n, 100000, n + 2], [2 ** 31 - 1, n, n + 1], [-2 ** 31, n, n + 1]]      # indices out of range
    faces += [[n, n, n + 1], [n + 2, n + 2, n + 2]]                # zero area: repeated vertices
    line = [unproject(40.0, 20.0, 1.0, K), unproject(44.0, 22.0, 1.0, K), unproject(48.0, 24.0, 1.0, K)]
    _add(verts, faces, line, [[0, 1, 2]])                          # zero area: collinear after the snap
    _add(verts, faces, [unproject(5.0, 24.6, 1.0, K), unproject(30.0, 24.9, 1.0, K), unproject(18.0, 24.7, 1.0, K)], [[0, 1, 2]])      # a sliver between rows of centres
    _add(verts, faces, [unproject(50.6, 26.0, 1.0, K), unproject(50.9, 44.0, 1.0, K), unproject(50.7, 35.0, 1.0, K)], [[0, 1, 2]])     # and between columns
    _add(verts, faces, [unproject(33.6, 30.6, 1.0, K), unproject(33.9, 30.7, 1.0, K), unproject(33.7, 30.9, 1.0, K)], [[0, 1, 2]])     # inside one pixel, off its centre
    _add(verts, faces, [unproject(5.0, 30.7, 1.0, K), unproject(15.0, 40.7, 1.0, K), unproject(15.0, 40.8, 1.0, K)], [[0, 1, 2]])       # a diagonal sliver: its box holds centres, it covers none
    for u, v in ((-3.0, 30.0), (58.0, 30.0), (20.0, -3.0), (20.0, 44.0)):                   # partly off the left, right, top, bottom
        _add(verts, faces, tri(u, v, 1.1), [[0, 1, 2]])
    for u, v in ((-20.0, 30.0), (70.0, 30.0), (20.0, -20.0), (20.0, 60.0), (-9.0, -9.0), (61.2, 47.2)):      # wholly off each side
        _add(verts, faces, tri(u, v, 1.1), [[0, 1, 2]])
    poses = [IDENTITY, look_at((0.4, 0.0, 0.2), (0.0, 0.1, 1.5))]
    return _scene(verts, faces, poses, K, 47, 61, near=REJECT_NEAR)


def _sizes():
    """47 x 61.  Triangles whose boxes are k = 1 .. 48 pixels wide and 1 .. 4 high (1 .. 192 pixels: the small / large budget is
    straddled whatever it is, and k = 16 is a box of exactly 16), a third of them behind and the rest in front of one triangle that
    covers the whole image at z = 3, and 6 boxes of 1 .. 47 rows that are one pixel wide."""
    K = K61
    verts, faces = [], []
    for k in range(1, 49):
        h = 1 + k % 4
        y = (k * 7) % 40 + 0.25
        z = (4.0 if k % 3 == 0 else 2.0) + 0.01 * k
        _add(verts, faces, [unproject(2.25, y, z, K), unproject(2.25 + k, y + 0.3 * h, z, K), unproject(2.25 + 0.6 * k, y + h, z, K)], [[0, 1, 2]])
    for i, rows in enumerate((1, 2, 16, 17, 33, 47)):
        x = 52.25 + i
        _add(verts, faces, [unproject(x, -0.25 + (47 - rows), 1.5, K), unproject(x + 0.7, 46.75 - 0.5 * rows, 1.5, K), unproject(x + 0.5, 46.75, 1.5, K)], [[0, 1, 2]])
    _add(verts, faces, [unproject(-200.0, -100.0, 3.0, K), unproject(400.0, -100.0, 3.0, K), unproject(-200.0, 500.0, 3.0, K)], [[0, 1, 2]])
    return _scene(verts, faces, [IDENTITY], K, 47, 61)


def _one_pixel():
    """a 1 x 1 image: one face over the pixel centre, a nearer one beside it"""
    K = intrinsics(1.0, 0.5, 0.5)
    verts, faces = [], []
    _add(verts, faces, [unproject(-1.0, -1.0, 2.0, K), unproject(3.0, -1.0, 2.0, K), unproject(-1.0, 3.0, 2.0, K)], [[0, 1, 2]])
    _add(verts, faces, [unproject(0.6, 0.6, 1.0, K), unproject(3.0, 0.6, 1.0, K), unproject(0.6, 3.0, 1.0, K)], [[0, 1, 2]])
    return _scene(verts, faces, [IDENTITY], K, 1, 1)


@functools.lru_cache(maxsize=None)
def scenes():
    return dict(sphere=_sphere(), quad_centres=_quad_centres(), ties=_ties(), rejects=_rejects(), sizes=_sizes(), one_pixel=_one_pixel())


@functools.lru_cache(maxsize=None)
def expected(name):
    sc = scenes()[name]
    return R.rasterize(sc["verts"], sc["faces"], sc["poses"], sc["intr"], sc["H"], sc["W"], sc["near"], return_counts=True)


# ------------------------------------------------------------------------------------------------------------- votes / clean_mesh
def votes_scene():
    """vertices under the identity pose of a 47 x 61 image with u exactly 0, exactly the width, v exactly 0 and exactly the height
    (fx = fy = 64, cx = cy = 0 and z = 2: exact), one ulp inside each, behind the camera, at c_z = near and below, NaN, beyond 65536,
    and a lattice over and around the image; a second, oblique view; masks: a disc and a checkerboard"""
    K = intrinsics(64.0, 0.0, 0.0)
    H, W, near = 47, 61, 0.5
    pts = []
    dn = lambda x: float(np.nextafter(F32(x), F32(-np.inf)))
    for u in (0.0, dn(0.0), -1e-3, 61.0, dn(61.0), 60.5, 1e-30):
        pts.append(unproject(u, 10.25, 2.0, K))
    for v in (0.0, dn(0.0), 47.0, dn(47.0), 46.5):
        pts.append(unproject(10.25, v, 2.0, K))
    pts += [unproject(61.0, 47.0, 2.0, K), unproject(0.0, 0.0, 2.0, K)]
    pts += [[0.1, 0.1, -1.0], [0.1, 0.1, 0.0], [0.1, 0.1, near], [0.1, 0.1, float(np.nextafter(F32(near), F32(0)))],
            [np.nan, 0.0, 1.0], [0.0, 0.0, np.inf], [0.0, np.inf, 1.0], unproject(70000.0, 5.0, 1.0, K), unproject(5.0, -70000.0, 1.0, K)]
    g = np.stack(np.meshgrid(np.linspace(-6.0, 67.0, 41), np.linspace(-5.0, 52.0, 37), indexing="ij"), axis=-1).reshape(-1, 2)
    pts += [unproject(u, v, 1.0 + 0.03 * (i % 50), K) for i, (u, v) in enumerate(g)]
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.stack([((xx - 30) ** 2 + (yy - 22) ** 2 < 18 ** 2), ((xx // 3 + yy // 2) % 2 == 0)]).astype(np.uint8)
    masks[1] *= 7                                                                  # any non-zero byte counts
    return dict(verts=np.array(pts, F32), poses=np.stack([IDENTITY, look_at((0.3, 0.1, -0.4), (0.4, 0.3, 1.5))]), intr=K,
                masks=masks, near=near)


CLEAN_OUTER_FACES = 528
CLEAN_FLOATER_FACES = 80


@functools.lru_cache(maxsize=None)
def clean_scene():
    """an outer 12 x 24 sphere of radius 1 (faces 0 .. 527), a floater beside it (outside the outer sphere's silhouette in every
    view) and a closed inner sphere of radius 0.5 that no camera sees; three views around, 48 x 64.  The masks are the outer sphere's
    own silhouette, rasterised by the restatement."""
    vo, fo = uv_sphere()
    vf, ff = uv_sphere(6, 8, 0.1, (0.0, 1.35, 0.0))
    vi, fi = uv_sphere(6, 12, 0.5)
    verts = np.concatenate([vo, vf, vi])
    faces = np.concatenate([fo, ff + len(vo), fi + len(vo) + len(vf)]).astype(np.int32)
    assert len(fo) == CLEAN_OUTER_FACES and len(ff) == CLEAN_FLOATER_FACES
    poses = np.stack([look_at((0.0, 0.0, -3.4), (0, 0.2, 0)), look_at((3.0, 0.3, -1.6), (0, 0.2, 0)), look_at((-2.4, -0.4, -2.4), (0, 0.2, 0))])
    K = intrinsics(60.0, 32.0, 24.0)
    masks = (R.rasterize(vo, fo, poses, K, 48, 64)["face_id"] >= 0).astype(np.uint8)
    return dict(verts=verts, faces=faces, poses=poses, intr=K, masks=masks, H=48, W=64)
