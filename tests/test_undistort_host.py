"""CPU: THE DISTORTION RULE and THE UNDISTORTION RULE of include/ls2fm.h judged by their properties on the numpy restatement
(tests/undistort_restate.py), so that the GPU tests (tests/test_hip_undistort.py) can be exact comparisons against that restatement;
the torch forms of ls2fm.undistort on CPU tensors against it bit for bit; that the edge scenes meet their edges; the output camera;
COLMAP's models and cameras.txt; refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import undistort_restate as UR
import undistort_scenes as US

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def U():
    from ls2fm import undistort
    return undistort


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def same(got, ref, what):
    """bit for bit; a NaN matches a NaN"""
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    r = np.asarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, f"{what}: {g.dtype} {g.shape} != {r.dtype} {r.shape}"
    view = {1: np.uint8, 4: np.int32, 8: np.int64}[g.dtype.itemsize]
    bad = g.view(view) != r.view(view)
    if g.dtype.kind == "f":
        bad &= ~(np.isnan(g) & np.isnan(r))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ, the first at {tuple(np.argwhere(bad)[0])}"


def full_size_cameras(U):
    """the four cameras of the issue: f = 1000 on 1600 x 1200 (barrel with tangential terms, pincushion with k3, rational with
    k4 = 0.5) and one of 47 x 33"""
    tang = [1e-3, -5e-4]
    return [(U.camera_from_colmap("OPENCV", [1000, 1000, 800, 600, -0.25, 0.08, *tang]), 1200, 1600),
            (U.camera_from_colmap("FULL_OPENCV", [1000, 990, 800, 600, 0.1, 0.02, *tang, 0.01, 0, 0, 0]), 1200, 1600),
            (U.camera_from_colmap("FULL_OPENCV", [1000, 1000, 800, 600, 0.2, 0.05, *tang, 0.01, 0.5, 0.02, 0.001]), 1200, 1600),
            (U.camera_from_colmap("OPENCV", [40, 41, 23.5, 16.25, -0.2, 0.05, 2e-3, -1e-3]), 33, 47)]


def test_the_header_s_constants_are_the_python_copies(U):
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()

    def const(name):
        return int(re.search(rf"#define\s+LS2FM_{name}\s+(\d+)", header).group(1))
    for name in ("CAMERA_PARAMS", "CAMERA_MAX_ITERS", "CAMERA_DISTORT", "CAMERA_UNDISTORT", "CAMERA_POINTS_THREADS", "UNDISTORT_BILINEAR",
                 "UNDISTORT_NEAREST", "UNDISTORT_TILE_W", "UNDISTORT_TILE_H"):
        assert const(name) == getattr(U, name), name
    assert U.UNDISTORT_TILE_W * U.UNDISTORT_TILE_H == 256
    assert (UR.PARAMS, UR.MAX_ITERS, UR.DISTORT, UR.UNDISTORT, UR.BILINEAR, UR.NEAREST) == \
        (U.CAMERA_PARAMS, U.CAMERA_MAX_ITERS, U.CAMERA_DISTORT, U.CAMERA_UNDISTORT, U.UNDISTORT_BILINEAR, U.UNDISTORT_NEAREST)
    assert (US.TILE_W, US.TILE_H) == (U.UNDISTORT_TILE_W, U.UNDISTORT_TILE_H)
    # the sizes of the bit-for-bit tests: inside one tile, a whole tile, one pixel past each edge of it
    for side, tile in ((0, US.TILE_H), (1, US.TILE_W)):
        outs = {out[side] for _, out in US.SIZES}
        assert any(s < tile for s in outs) and tile in outs and tile + 1 in outs
    assert all(src != out for src, out in US.SIZES)


@pytest.mark.parametrize("name,Hs,Ws,f", [("barrel", 33, 47, 40.0), ("rational", 65, 97, 60.0)])
def test_distortion_and_its_newton_inverse_undo_each_other(name, Hs, Ws, f):
    """every pixel centre, both orders, iters = 10: below 1e-9 px (a condition on the scene: the restatement meets it with orders
    to spare, the largest figure is printed)"""
    cam = US.camera(name, Hs, Ws, f)[None]
    k = np.array([[f * 1.25, f * 0.75, Ws / 2.0 + 1.0, Hs / 2.0 - 0.5]])
    p = US.grid_points(Hs, Ws)
    vs = US.one_view(len(p))
    # photograph -> pinhole -> photograph
    und, res = UR.camera_points(p, vs, cam, k, UR.UNDISTORT, 10)
    back, zero = UR.camera_points(und, vs, cam, k, UR.DISTORT)
    # pinhole (the camera's own) -> photograph -> pinhole
    dist, _ = UR.camera_points(p, vs, cam, cam[:, :4], UR.DISTORT)
    again, res2 = UR.camera_points(dist, vs, cam, cam[:, :4], UR.UNDISTORT, 10)
    worst = [np.sqrt(res.max()), np.abs(back - p).max(), np.sqrt(res2.max()), np.abs(again - p).max()]
    print(f"{name} {Hs} x {Ws}: residual and round trip {worst}")
    assert max(worst) < 1e-9 and (zero == 0).all()
    # the start is the answer without distortion, and the residual then is what the distortion moves
    start, r0 = UR.camera_points(p, vs, cam, cam[:, :4], UR.UNDISTORT, 0)
    assert np.abs(start - p).max() < 1e-12 and r0.max() > 1.0


def test_the_jacobian_is_the_derivative_of_the_rule():
    cam = US.camera("rational", 65, 97, 60.0)[None]
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-0.7, 0.7, 500), rng.uniform(-0.5, 0.5, 500)
    _, _, shared = UR.distort(cam, x, y)
    a, b, c, d = UR.jacobian(cam, shared, x, y)
    h = 1e-6
    xp, yp, _ = UR.distort(cam, x + h, y)
    xm, ym, _ = UR.distort(cam, x - h, y)
    assert np.abs((xp - xm) / (2 * h) - a).max() < 1e-8 and np.abs((yp - ym) / (2 * h) - c).max() < 1e-8
    xp, yp, _ = UR.distort(cam, x, y + h)
    xm, ym, _ = UR.distort(cam, x, y - h)
    assert np.abs((xp - xm) / (2 * h) - b).max() < 1e-8 and np.abs((yp - ym) / (2 * h) - d).max() < 1e-8


def test_the_output_camera_keeps_only_valid_pixels_or_every_pixel(U):
    for cam, Hs, Ws in full_size_cameras(U):
        c = cam.numpy()
        # blank_pixels = 0: every output pixel sees the photograph
        k, H, W = U.undistorted_intrinsics(cam, Hs, Ws, blank_pixels=0.0)
        assert k[0] == cam[0] and k[1] == cam[1] and H >= 1 and W >= 1
        u, v = UR.source_coordinates(c[None].astype(F32), k.numpy()[None].astype(F32), H, W)
        ok = (u >= 0) & (u < Ws) & (v >= 0) & (v < Hs)
        assert ok.all(), f"{int((~ok).sum())} invalid pixels of {H} x {W}"
        # blank_pixels = 1: every border pixel of the photograph lands within half a pixel of the output rectangle
        k, H, W = U.undistorted_intrinsics(cam, Hs, Ws, blank_pixels=1.0)
        ys, xs = np.arange(Hs) + 0.5, np.arange(Ws) + 0.5
        border = np.concatenate([np.stack([np.full(Hs, 0.5), ys], 1), np.stack([np.full(Hs, Ws - 0.5), ys], 1),
                                 np.stack([xs, np.full(Ws, 0.5)], 1), np.stack([xs, np.full(Ws, Hs - 0.5)], 1)])
        p, res = UR.camera_points(border, US.one_view(len(border)), c[None], k.numpy()[None], UR.UNDISTORT, 10)
        assert res.max() < 1e-18
        outside = max(-p.min(), (p[:, 0] - W).max(), (p[:, 1] - H).max(), 0.0)
        print(f"{Hs} x {Ws}: blank 1 -> {H} x {W}, the border at most {outside:.3f} px outside")
        assert outside <= 0.5
    # between the two the size is monotone, and the clip holds
    cam, Hs, Ws = full_size_cameras(U)[3]
    sizes = [U.undistorted_intrinsics(cam, Hs, Ws, blank_pixels=b)[1:] for b in (0.0, 0.5, 1.0)]
    assert sizes[0][0] <= sizes[1][0] <= sizes[2][0] and sizes[0][1] <= sizes[1][1] <= sizes[2][1] and sizes[0] != sizes[2]
    assert U.undistorted_intrinsics(cam, Hs, Ws, 1.0, max_scale=1.0)[1:] == (Hs, Ws)


def test_undistortion_reproduces_a_sinusoid_within_the_bilinear_bound():
    """P(X, Y) = 0.5 + 0.5 sin(a X) sin(a Y), a = 2 pi / 16 output pixels, synthesised on the photograph's grid through the
    restatement's inverse, then undistorted: it must miss P by at most 2 (1/8) a^2 J^2, J the largest source-pixel step per output
    pixel (the largest singular value of d(u, v)/d(X, Y) over the output pixels, from the rule's Jacobian).
    Derivation: bilinear interpolation of g on a unit grid errs by at most (1/8)(max |g_uu| + max |g_vv|).  With g(u, v) = P(X(u, v),
    Y(u, v)) and |P_XX| + |P_YY| <= a^2 |sin sin| <= a^2, the leading term is (1/8) a^2 / s^2, s the smallest singular value (output
    pixels per source pixel is 1 / s at worst); the bound's factor 2 J^2 covers it, the cross terms and the map's curvature when
    s^2 J^2 >= 0.75, which is asserted of the scene -- a condition computed from the Jacobian, not from the result."""
    Hs, Ws = 65, 97
    cam = US.camera("barrel", Hs, Ws, 1.5 * Ws)[None]
    H, W = 60, 90
    k = np.array([[1.4 * Ws, 1.45 * Ws, W / 2.0 - 0.4, H / 2.0 + 0.3]])
    p = US.grid_points(Hs, Ws)
    at, res = UR.camera_points(p, US.one_view(len(p)), cam, k, UR.UNDISTORT, 10)
    assert res.max() < 1e-18
    photo = US.wave(at[:, 0], at[:, 1]).reshape(1, Hs, Ws, 1).astype(F32)
    out, valid = UR.undistort_images(photo, cam.astype(F32), k.astype(F32), H, W)
    assert valid.mean() > 0.9
    q = US.grid_points(H, W)
    x, y = (q[:, 0] - k[0, 2]) / k[0, 0], (q[:, 1] - k[0, 3]) / k[0, 1]
    _, _, shared = UR.distort(cam, x, y)
    a, b, c, d = UR.jacobian(cam, shared, x, y)
    J = np.stack([np.stack([cam[0, 0] * a / k[0, 0], cam[0, 0] * b / k[0, 1]], -1), np.stack([cam[0, 1] * c / k[0, 0], cam[0, 1] * d / k[0, 1]], -1)], -2)
    sv = np.linalg.svd(J[valid.reshape(-1) > 0], compute_uv=False)
    J_max, s_min = sv.max(), sv.min()
    assert s_min ** 2 * J_max ** 2 >= 0.75, (s_min, J_max)
    bound = 2.0 * (1.0 / 8.0) * (2.0 * np.pi / US.WAVELENGTH) ** 2 * J_max ** 2
    err = np.abs(out[0, :, :, 0].astype(F64) - US.wave(q[:, 0], q[:, 1]).reshape(H, W))[valid[0] > 0].max()
    print(f"sinusoid: error {err:.4f}, bound {bound:.4f}, J {J_max:.3f}, smallest singular value {s_min:.3f}")
    assert err <= bound


def test_a_camera_without_distortion_returns_the_input_s_bits(U):
    """power-of-two fx, dyadic cx, the same out_intr, the same size: u = px + 0.5 exactly, tx = ty = 0"""
    rng = np.random.default_rng(3)
    img = rng.standard_normal((2, 9, 33, 3)).astype(F32)
    img[0, 4, 7, 1] = 3.0e38                    # finite: a tap of weight 0 on an inf or a NaN would be a NaN by the rule
    cam = np.zeros((2, 12), F32)
    cam[0, :4] = [32.0, 16.0, 16.5, 4.25]
    cam[1, :4] = [64.0, 64.0, 15.75, 5.0]
    for mode in (UR.BILINEAR, UR.NEAREST):
        out, valid = UR.undistort_images(img, cam, cam[:, :4], 9, 33, mode)
        same(out, img, f"mode {mode}")
        assert valid.all()
    out, valid = U.undistort_images(t(img), t(cam), None, 9, 33)
    same(out, img, "torch form")


def test_the_edge_scene_meets_its_edges():
    sc = US.edge_scene()
    u, v = UR.source_coordinates(sc["cam"], sc["out_intr"], 8, 8)
    out, valid = UR.undistort_images(sc["images"], sc["cam"], sc["out_intr"], 8, 8, UR.BILINEAR, [-1.0, -2.0])
    img = sc["images"]
    assert u[0, 2, 2] == 0 and v[0, 2, 2] == 0 and valid[0, 2, 2] == 1            # u exactly 0: valid, x0 = -1, both taps clamped to 0
    assert np.isnan(out[0, 2, 2, 0]) and out[0, 2, 2, 1] == img[0, 0, 0, 1]       # the NaN at (0, 0) stays; the other channel is the pixel
    assert 0 < u[1, 2, 2] < 1e-44 and valid[1, 2, 2] == 1                         # one ulp inside
    assert u[2, 0, 2] < 0 and not valid[2, :, 2].any() and valid[2, :6, 3].all()   # one ulp outside
    assert u[3, 0, 2] == 8 and not valid[3, :, 2:].any() and valid[3, :6, 1].all()  # u exactly Ws
    assert u[4, 2, 2] == F32(US.BELOW_8) and v[4, 2, 2] == F32(US.BELOW_8) and valid[4, 2, 2] == 1   # one ulp inside Ws: x0 = Ws - 1
    assert out[4, 2, 2, 1] == img[4, 7, 7, 1]
    assert v[5, 2, 0] == 8 and not valid[5, 2:, :].any() and valid[5, 1, :6].all()
    assert not valid[6, 2, :].any() and valid[6, 3, :6].all()
    assert not np.isfinite(u[US.EDGE_DEN0, 2, 6]) and valid[US.EDGE_DEN0, 2, 6] == 0 and valid[US.EDGE_DEN0, 2, 5] == 1
    assert not valid[US.EDGE_NAN].any() and not valid[US.EDGE_INF].any()
    assert valid[US.EDGE_PLAIN].all() and valid[:US.EDGE_DEN0].any(axis=(1, 2)).all()
    assert (out[~valid.astype(bool)] == np.array([-1.0, -2.0], F32)).all()
    finite = np.isfinite(out[US.EDGE_PLAIN])
    assert (~finite).any() and finite.any()                                        # the NaN and the inf pixel are tapped
    near, _ = UR.undistort_images(sc["images"], sc["cam"], sc["out_intr"], 8, 8, UR.NEAREST, np.nan)
    assert near[4, 2, 2, 1] == img[4, 7, 7, 1] and near[0, 2, 2, 1] == img[0, 0, 0, 1] and np.isnan(near[3, 0, 2]).all()


def test_the_points_scene_meets_its_edges():
    sc = US.points_scene()
    vs = sc["view_start"]
    assert np.diff(vs).tolist() == US.POINT_COUNTS and {0, 1, 63, 64, 65, 257} <= set(US.POINT_COUNTS)
    for iters in (0, 1, 10):
        out, res = UR.camera_points(sc["uv"], vs, sc["cam"], sc["out_intr"], UR.UNDISTORT, iters)
        k = sc["out_intr"]
        same(out[vs[2]], k[2, 2:4], "the principal point goes to the output's")
        assert res[vs[2]] == 0
        assert np.isnan(out[vs[3] + 5, 0]) and np.isnan(res[vs[3] + 5]) and np.isfinite(out[vs[3] + 4]).all()
        f = vs[US.FOLD_VIEW]                    # det = 0 at the start: no step is taken, whatever iters
        same(out[f], np.array([k[6, 0] * 1.0 + k[6, 2], k[6, 1] * 0.0 + k[6, 3]]), "the fold")
        assert res[f] == (8.0 * 3.0) ** 2
        assert not np.isfinite(res[vs[US.INF_VIEW]:]).any()        # no step is taken: the start stays, the residual tells
    moved, _ = UR.camera_points(sc["uv"], vs, sc["cam"], sc["out_intr"], UR.UNDISTORT, 1)
    assert (moved[f + 1] != UR.camera_points(sc["uv"], vs, sc["cam"], sc["out_intr"], UR.UNDISTORT, 0)[0][f + 1]).any()
    ten, res = UR.camera_points(sc["uv"], vs, sc["cam"], sc["out_intr"], UR.UNDISTORT, 10)
    assert res[:vs[6]][np.isfinite(res[:vs[6]])].max() < 1e-18


@pytest.mark.parametrize("src,out", US.SIZES)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_the_torch_form_of_the_images_on_the_cpu_leaves_the_restatement_s_bits(U, src, out, C):
    sc = US.image_scene(*src, *out, C)
    for mode, name in ((UR.BILINEAR, "bilinear"), (UR.NEAREST, "nearest")):
        want, valid = UR.undistort_images(sc["images"], sc["cam"], sc["out_intr"], *out, mode, np.nan)
        got, gv = U.undistort_images(t(sc["images"]), t(sc["cam"]), t(sc["out_intr"]), *out, mode=name)
        same(got, want, f"{name} out")
        same(gv, valid, f"{name} valid")
        assert 0 < valid.mean() < 1 and valid.min(axis=(1, 2)).max() == 0


def test_the_torch_forms_on_the_edge_scenes_leave_the_restatement_s_bits(U):
    sc = US.edge_scene()
    for mode, name in ((UR.BILINEAR, "bilinear"), (UR.NEAREST, "nearest")):
        for fill in (np.nan, [0.25, -3.0]):
            want, valid = UR.undistort_images(sc["images"], sc["cam"], sc["out_intr"], 8, 8, mode, fill)
            got, gv = U.undistort_images(t(sc["images"]), t(sc["cam"]), t(sc["out_intr"]), 8, 8, mode=name, fill=fill)
            same(got, want, f"{name} out")
            same(gv, valid, f"{name} valid")
    grey, _ = U.undistort_images(t(sc["images"][..., 0]), t(sc["cam"]), t(sc["out_intr"]), 8, 8)
    same(grey, UR.undistort_images(sc["images"][..., :1], sc["cam"], sc["out_intr"], 8, 8)[0][..., 0], "grey")
    pt = US.points_scene()
    for iters in (0, 1, 10, 32):
        want, res = UR.camera_points(pt["uv"], pt["view_start"], pt["cam"], pt["out_intr"], UR.UNDISTORT, iters)
        got, gr = U.undistort_points(t(pt["uv"]), t(pt["cam"]), t(pt["view_start"]), t(pt["out_intr"]), iters=iters)
        same(got, want, f"undistort {iters}")
        same(gr, res, f"residual {iters}")
    want, res = UR.camera_points(pt["uv"], pt["view_start"], pt["cam"], pt["out_intr"], UR.DISTORT)
    got, gr = U.distort_points(t(pt["uv"]), t(pt["cam"]), t(pt["view_start"]), t(pt["out_intr"]))
    same(got, want, "distort")
    same(gr, res, "distort's residual")
    # out_intr = None is the camera's own pinhole; rows outside every view are NaN
    own, _ = U.undistort_points(t(pt["uv"]), t(pt["cam"]), t(pt["view_start"]))
    same(own, UR.camera_points(pt["uv"], pt["view_start"], pt["cam"], pt["cam"][:, :4], UR.UNDISTORT, 10)[0], "own pinhole")
    short = pt["view_start"].copy()
    short[-1] -= 2
    cut, cr = U.undistort_points(t(pt["uv"]), t(pt["cam"]), t(short), t(pt["out_intr"]))
    assert torch.isnan(cut[-2:]).all() and torch.isnan(cr[-2:]).all()
    same(cut[:-2], UR.camera_points(pt["uv"], pt["view_start"], pt["cam"], pt["out_intr"], UR.UNDISTORT, 10)[0][:-2], "short table")


def test_undistort_keypoints_moves_positions_only(U):
    pt = US.points_scene()
    V, cap = 3, 70
    rng = np.random.default_rng(4)
    kp = rng.random((V * cap, 4)).astype(F32) * [47, 33, 4, 6.28]
    kp = kp.astype(F32)
    counts = np.array([65, 0, 70], np.int32)
    cam = pt["cam"][1:4]
    got = U.undistort_keypoints(t(kp), t(counts), t(cam), t(pt["out_intr"][1:4]))
    want, _ = UR.camera_points(kp[:, :2].astype(F64), np.arange(V + 1) * cap, cam, pt["out_intr"][1:4], UR.UNDISTORT, 10)
    live = (np.arange(cap)[None, :] < counts[:, None]).reshape(-1)
    same(got[:, 2:], kp[:, 2:], "scale and orientation")
    same(got[~live, :2], kp[~live, :2], "rows past counts")
    same(got[live, :2], want[live].astype(F32), "positions")
    assert got.dtype == torch.float32 and (got.numpy()[live, :2] != kp[live, :2]).any()


def test_undistort_views_uses_one_size_and_each_view_s_centre(U):
    rng = np.random.default_rng(6)
    photos = rng.random((2, 33, 47, 3), dtype=F32)
    cams = np.stack([US.camera("barrel", 33, 47, 40.0), US.camera("pincushion", 33, 47, 44.0)])
    each = [U.undistorted_intrinsics(t(c), 33, 47) for c in cams]
    out, intr, valid = U.undistort_views(t(photos), t(cams))
    H, W = min(e[1] for e in each), min(e[2] for e in each)
    assert tuple(out.shape) == (2, H, W, 3) and tuple(intr.shape) == (2, 3, 3) and intr.dtype == torch.float32 and bool(valid.all())
    k4 = np.stack([e[0].numpy() for e in each]).astype(F32)
    same(intr[:, [0, 1, 0, 1], [0, 1, 2, 2]], k4, "intr")
    assert (intr[:, 2, 2] == 1).all() and intr[:, 0, 1].abs().max() == 0
    same(out, UR.undistort_images(photos, cams.astype(F32), k4, H, W)[0], "images")
    one, k1, _ = U.undistort_views(t(photos[0, :, :, 0])[None], t(cams[0]), blank_pixels=1.0, mode="nearest", fill=0.0)
    k, H1, W1 = U.undistorted_intrinsics(t(cams[0]), 33, 47, blank_pixels=1.0)
    assert tuple(one.shape) == (1, H1, W1) and (H1, W1) != each[0][1:]
    same(k1[0, [0, 1, 0, 1], [0, 1, 2, 2]], k.numpy().astype(F32), "intr at blank_pixels = 1")
    same(one, UR.undistort_images(photos[:1, :, :, :1], cams[:1].astype(F32), k.numpy()[None].astype(F32), H1, W1, UR.NEAREST, 0.0)[0][..., 0],
         "nearest, grey, blank_pixels = 1")


def test_camera_from_colmap_on_each_name(U):
    z = [0.0] * 8
    cases = {"SIMPLE_PINHOLE": ([500, 320, 240], [500, 500, 320, 240] + z),
             "PINHOLE": ([500, 510, 320, 240], [500, 510, 320, 240] + z),
             "SIMPLE_RADIAL": ([500, 320, 240, -0.1], [500, 500, 320, 240, -0.1] + z[:7]),
             "RADIAL": ([500, 320, 240, -0.1, 0.02], [500, 500, 320, 240, -0.1, 0.02] + z[:6]),
             "OPENCV": ([500, 510, 320, 240, -0.1, 0.02, 1e-3, 2e-3], [500, 510, 320, 240, -0.1, 0.02, 1e-3, 2e-3] + z[:4]),
             "FULL_OPENCV": (list(range(1, 13)), list(range(1, 13)))}
    assert set(cases) == set(U.COLMAP_MODELS)
    for name, (params, want) in cases.items():
        cam = U.camera_from_colmap(name, params)
        assert cam.dtype == torch.float64 and cam.tolist() == [float(w) for w in want], name
        assert U.camera_from_colmap(name.lower(), params).tolist() == cam.tolist()
        with pytest.raises(ValueError, match=name):
            U.camera_from_colmap(name, params + [0.0])
    for name in ("OPENCV_FISHEYE", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"):
        with pytest.raises(ValueError, match=name):
            U.camera_from_colmap(name, [1.0] * 12)
    with pytest.raises(ValueError, match="WIDE_ANGLE"):
        U.camera_from_colmap("WIDE_ANGLE", [1.0])


def test_a_cameras_txt_is_read_back(U, tmp_path):
    path = tmp_path / "cameras.txt"
    path.write_text("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n# Number of cameras: 3\n"
                    "1 SIMPLE_RADIAL 1600 1200 1000.5 800 600 -0.125\n\n"
                    "7 OPENCV 6048 4032 3411.42 3410.02 3041.29 2014.07 0.21047 0.21102 -5.36231e-06 0.00051541\n"
                    "3 PINHOLE 640 480 525 525 319.5 239.5\n")
    cams = U.read_cameras_txt(str(path))
    assert sorted(cams) == [1, 3, 7]
    assert cams[1]["model"] == "SIMPLE_RADIAL" and (cams[1]["width"], cams[1]["height"]) == (1600, 1200)
    assert cams[1]["cam"].tolist() == [1000.5, 1000.5, 800.0, 600.0, -0.125] + [0.0] * 7
    assert cams[7]["cam"].tolist() == [3411.42, 3410.02, 3041.29, 2014.07, 0.21047, 0.21102, -5.36231e-06, 0.00051541, 0.0, 0.0, 0.0, 0.0]
    assert cams[3]["cam"][:4].tolist() == [525.0, 525.0, 319.5, 239.5] and (cams[7]["width"], cams[7]["height"]) == (6048, 4032)
    for bad in ("1 PINHOLE 640 480 525 525 319.5\n", "2 OPENCV_FISHEYE 640 480 1 1 1 1 0 0 0 0\n", "1 PINHOLE 640\n",
                "1 PINHOLE 640 480 1 1 1 1\n1 PINHOLE 640 480 1 1 1 1\n"):
        path.write_text(bad)
        with pytest.raises(ValueError, match="cameras.txt"):
            U.read_cameras_txt(str(path))


def test_refusals(U):
    from ls2fm import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    some, fill = P(4096), (ctypes.c_float * 4)(0, 0, 0, 0)        # refused calls touch no array

    def images(im=some, V=2, Hs=8, Ws=8, C=3, cam=some, k=some, H=8, W=8, mode=0, fl=fill, out=some, valid=P(0)):
        return lib.ls2fm_undistort_images(im, V, Hs, Ws, C, cam, k, H, W, mode, fl, out, valid, P(0))
    for kw in (dict(im=P(0)), dict(cam=P(0)), dict(k=P(0)), dict(out=P(0)), dict(fl=None), dict(V=-1), dict(Hs=0), dict(Ws=32769), dict(H=0),
               dict(H=32769), dict(W=0), dict(W=32769), dict(Hs=32769), dict(C=0), dict(C=5), dict(mode=2), dict(mode=-1),
               dict(V=1024, H=32768, W=32768), dict(V=1024, Hs=32768, Ws=32768), dict(V=2 ** 21, H=8192, W=32)):
        assert images(**kw) == -1, kw
    assert images(V=0, im=P(0), cam=P(0), k=P(0), out=P(0), fl=None) == 0

    def points(uv=some, n=10, vs=some, V=2, cam=some, k=some, direction=1, iters=10, out=some, res=P(0)):
        return lib.ls2fm_camera_points(uv, n, vs, V, cam, k, direction, iters, out, res, P(0))
    for kw in (dict(uv=P(0)), dict(vs=P(0)), dict(cam=P(0)), dict(k=P(0)), dict(out=P(0)), dict(n=-1), dict(n=2 ** 31), dict(V=0), dict(V=-1),
               dict(direction=2), dict(direction=-1), dict(iters=-1), dict(iters=33)):
        assert points(**kw) == -1, kw
    assert points(n=0, uv=P(0), vs=P(0), cam=P(0), k=P(0), out=P(0), V=0) == 0
    # the Python forms
    img, cam = torch.zeros(2, 8, 8, 3), torch.zeros(2, 12)
    for call in (lambda: U.undistort_images(torch.zeros(2, 8, 8, 5), cam, None, 8, 8),
                 lambda: U.undistort_images(torch.zeros(8, 8), cam, None, 8, 8),
                 lambda: U.undistort_images(img, cam, None, 8, 8, mode="bicubic"),
                 lambda: U.undistort_images(img, cam, None, 0, 8),
                 lambda: U.undistort_images(img, cam, None, 8, 32769),
                 lambda: U.undistort_images(img, torch.zeros(3, 12), None, 8, 8),
                 lambda: U.undistort_images(img, torch.zeros(2, 8), None, 8, 8),
                 lambda: U.undistort_images(img, cam, torch.zeros(3, 4), 8, 8),
                 lambda: U.undistort_images(img, cam, torch.zeros(2, 5), 8, 8),
                 lambda: U.undistort_images(img, cam, None, 8, 8, fill=[0.0, 1.0]),
                 lambda: U.undistort_points(torch.zeros(5, 3), cam[0]),
                 lambda: U.undistort_points(torch.zeros(5, 2), cam),
                 lambda: U.undistort_points(torch.zeros(5, 2), cam, view_start=[0, 5]),
                 lambda: U.undistort_points(torch.zeros(5, 2), cam[0], iters=33),
                 lambda: U.undistort_points(torch.zeros(5, 2), cam[0], iters=-1),
                 lambda: U.undistort_keypoints(torch.zeros(10, 3), torch.zeros(2, dtype=torch.int32), cam),
                 lambda: U.undistort_keypoints(torch.zeros(11, 4), torch.zeros(2, dtype=torch.int32), cam),
                 lambda: U.undistorted_intrinsics(cam[0], 0, 8),
                 lambda: U.undistorted_intrinsics(cam[0], 8, 8, blank_pixels=1.5),
                 lambda: U.undistorted_intrinsics(cam[0], 8, 8, min_scale=0.0),
                 lambda: U.undistort_views(img, torch.zeros(3, 12))):
        with pytest.raises(ValueError, match=r"ls2fm\.undistort"):
            call()
