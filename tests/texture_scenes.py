"""Deterministic scenes for the texture tests (numpy only).

sphere_scene(): where the point of a texture atlas is judged (tests/test_texture_host.py) and where photo_texture is held to the
restatement bit for bit (tests/test_hip_texture.py).  A coarse icosphere of 320 faces and 162 vertices on the sphere of radius 0.5
(edges of 0.14 .. 0.16), six cameras on the axes at distance 2.5 (f_px = 160, 96 x 96: mesh_colors_scenes' geometry), and photographs
rendered analytically, ray against sphere, from the pattern
    c_ch(X) = 0.5 + 0.45 sin(2 pi / PATTERN_WAVELENGTH  X . d_ch)
with PATTERN_WAVELENGTH = 0.25: 1.6 .. 1.8 vertex spacings per wavelength (below the two a wave needs), 20 pixels of 0.0125, and 5
texels of 0.05 at the pitch-8 charts (L = 3) SPHERE_TEXEL puts every face in.  The face centres lie 0.008 inside the sphere, a
parallax of 0.2 rad of phase at 45 degrees; power = 2 weighs the head-on views.

small meshes and edge_mesh(): the shapes of the bit-for-bit kernel tests (see there)."""
import functools

import numpy as np

import mesh_colors_restate as MR
import raster_restate as R
import texture_restate as TR
from raster_scenes import intrinsics, look_at

F32 = np.float32

PATTERN_WAVELENGTH = 0.25
PATTERN_DIRS = np.array([[1.0, 0.3, 0.2], [-0.2, 1.0, 0.4], [0.3, -0.4, 1.0]]) / np.linalg.norm([[1.0, 0.3, 0.2], [-0.2, 1.0, 0.4], [0.3, -0.4, 1.0]], axis=1, keepdims=True)
SPHERE_R, SPHERE_D, SPHERE_F, SPHERE_HW, SPHERE_TOL, SPHERE_POWER = 0.5, 2.5, 160.0, 96, 0.02, 2
SPHERE_TEXEL = 0.056          # the longest leg of the icosphere is 0.1625 < 3 * 0.056: every face in the class of pitch 8
SPHERE_FILL = (0.25, 0.5, 0.75)


def icosphere(subdivisions=2, radius=SPHERE_R):
    """verts float32 [V, 3] on the sphere, faces int32 [F, 3] wound so that (b - a) x (c - a) points outward"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = out
    return (np.asarray(v) * radius).astype(F32), np.asarray(f, np.int32)


def pattern(X):
    """c(X) float64 [..., 3]"""
    X = np.asarray(X, np.float64)
    return 0.5 + 0.45 * np.sin(2.0 * np.pi / PATTERN_WAVELENGTH * (X @ PATTERN_DIRS.T))


def sphere_photo(pose, K, H, W, background=0.0):
    """the sphere's photograph, analytically: per pixel centre the ray against the sphere, the pattern at the hit (float32 [H, W, 3])"""
    P = np.asarray(pose, np.float64)
    Rm, t = P[:, :3], P[:, 3]
    eye = -Rm.T @ t
    v, u = np.mgrid[0:H, 0:W] + 0.5
    d = np.stack([(u - float(K[0, 2])) / float(K[0, 0]), (v - float(K[1, 2])) / float(K[1, 1]), np.ones_like(u)], axis=-1) @ Rm
    a, b, c = (d * d).sum(-1), 2.0 * (d @ eye), eye @ eye - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    hit = disc > 0
    s = (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a)
    img = np.full((H, W, 3), background, np.float64)
    img[hit] = pattern(eye + s[hit][:, None] * d[hit])
    return img.astype(F32)


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """dict(verts, faces, poses [6, 3, 4], intr, H, W, images [6, H, W, 3], near, depth_tol, power, depth float32 [6, H, W] (the
    restatement's rasterisation of the coarse mesh), texel, gutter); callers do not write into it"""
    verts, faces = icosphere(2)
    D = SPHERE_D
    eyes = np.array([[D, 0, 0], [-D, 0, 0], [0, D, 0], [0, -D, 0], [0, 0, D], [0, 0, -D]], np.float64)
    poses = np.stack([look_at(e, (0, 0, 0), up=(0.0, 0.0, 1.0) if e[1] != 0 else (0.0, 1.0, 0.0)) for e in eyes])
    K = intrinsics(SPHERE_F, SPHERE_HW / 2, SPHERE_HW / 2)
    H = W = SPHERE_HW
    images = np.stack([sphere_photo(p, K, H, W) for p in poses])
    depth = R.rasterize(verts, faces, poses, K, H, W, 1e-3)["depth"]
    return dict(verts=verts, faces=faces, poses=poses, intr=K, H=H, W=W, images=images, near=1e-3, depth_tol=SPHERE_TOL,
                power=SPHERE_POWER, depth=depth, texel=SPHERE_TEXEL, gutter=1)


@functools.lru_cache(maxsize=None)
def sphere_atlas():
    """the restatement's atlas of the sphere scene: dict(rot, cls, order, table, size, uv, face, point, normal)"""
    sc = sphere_scene()
    rot, cls = TR.classify(sc["verts"], sc["faces"], sc["texel"], sc["gutter"])
    order, table = TR.pack(cls, sc["gutter"])
    S = TR.smallest_size(table)
    out = TR.texels(sc["verts"], sc["faces"], order, rot, table, sc["gutter"], S)
    return dict(rot=rot, cls=cls, order=order, table=table, size=S, **out)


@functools.lru_cache(maxsize=None)
def sphere_texture():
    """the restatement's photo texture of the sphere scene: the texels' points through mesh_colors_restate, weights by the chart
    normals -> dict(texture float32 [S, S, 3], count int32 [S, S])"""
    sc, at = sphere_scene(), sphere_atlas()
    S = at["size"]
    got = MR.vertex_colors(at["point"].reshape(-1, 3), sc["poses"], sc["intr"], sc["images"], sc["depth"], normals=at["normal"].reshape(-1, 3),
                           near=sc["near"], depth_tol=sc["depth_tol"], power=sc["power"], fill=SPHERE_FILL)
    return dict(texture=got["colors"].reshape(S, S, 3), count=got["count"].reshape(S, S))


@functools.lru_cache(maxsize=None)
def sphere_vertex_colors():
    """the restatement's vertex colours of the same mesh under the same rule, weights by the sphere's own normals"""
    sc = sphere_scene()
    return MR.vertex_colors(sc["verts"], sc["poses"], sc["intr"], sc["images"], sc["depth"], normals=sc["verts"], near=sc["near"],
                            depth_tol=sc["depth_tol"], power=sc["power"], fill=SPHERE_FILL)["colors"]


def face_samples(n=6):
    """barycentric sample points of a face, corners and edges included: float32 [(n + 1)(n + 2) / 2, 3]"""
    return np.array([[i / n, j / n, (n - i - j) / n] for i in range(n + 1) for j in range(n + 1 - i)], F32)


# ------------------------------------------------------------------------------------------------------------------ kernel shapes
def small_mesh(n_faces):
    """1, 2 or 3 faces of different sizes over 5 vertices (float32 verts, int32 faces)"""
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 2.0, 0.5], [1.5, 1.75, -0.25], [-0.125, 0.5, 3.0]], F32)
    faces = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4]], np.int32)[:n_faces]
    return verts, faces


def edge_mesh():
    """37 faces of at least three classes at texel = 0.25, gutter 1 (legs from 0.3 to 40), with the rule's edge cases among them:
    face 3 has zero area (a repeated vertex), face 5 a NaN vertex, face 7 an index out of range, face 9 an isosceles tie between its
    two longest edges, face 11 is equilateral in exact coordinates (a three-way tie)"""
    rng = np.random.default_rng(11)
    verts, faces = [], []
    for i in range(37):
        scale = [0.3, 1.0, 2.5, 6.0, 40.0][i % 5]
        base = rng.uniform(-2, 2, 3)
        tri = base + scale * rng.uniform(0.2, 1.0, (3, 3)) * rng.choice([-1.0, 1.0], (3, 3))
        faces.append([len(verts) + k for k in range(3)])
        verts += list(tri)
    verts = np.array(verts, F32)
    faces = np.array(faces, np.int32)
    faces[3, 2] = faces[3, 1]
    verts[faces[5, 1], 0] = np.nan
    faces[7, 0] = len(verts) + 5
    verts[faces[9]] = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]          # right isosceles, then turned: the two legs tie, the hypotenuse wins
    verts[faces[9]] = verts[faces[9]][[1, 2, 0]]
    verts[faces[11]] = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]         # all three edges 2: rotation 0
    return verts, faces
