"""GPU: ls2fm_undistort_images and ls2fm_camera_points (csrc/undistort.hip) through ls2fm.undistort: every output pixel, every valid
byte, every point and residual by their bits against the numpy restatement (tests/undistort_restate.py); the torch forms on the
device, views and rows in several calls, a rerun and a replay from a captured graph; the chain into ls2fm.mvs.plane_sweep.  The
rules themselves, and that the edge scenes meet their edges, are judged on the restatement (tests/test_undistort_host.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import undistort_restate as UR
import undistort_scenes as US

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64
MODES = ((UR.BILINEAR, "bilinear"), (UR.NEAREST, "nearest"))


@pytest.fixture(scope="module")
def U():
    from ls2fm import undistort
    return undistort


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same(got, ref, what):
    """bit for bit; a NaN matches a NaN (its sign and payload are the one thing IEEE 754 leaves to the implementation)"""
    g, r = host(got), host(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, f"{what}: {g.dtype} {g.shape} != {r.dtype} {r.shape}"
    view = {1: np.uint8, 4: np.int32, 8: np.int64}[g.dtype.itemsize]
    bad = g.view(view) != r.view(view)
    if g.dtype.kind == "f":
        bad &= ~(np.isnan(g) & np.isnan(r))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ, the first at {tuple(np.argwhere(bad)[0])}"


@functools.lru_cache(maxsize=None)
def restated_images(src, out, C, mode):
    sc = US.image_scene(*src, *out, C)
    return UR.undistort_images(sc["images"], sc["cam"], sc["out_intr"], *out, mode, np.nan)


@functools.lru_cache(maxsize=None)
def restated_points(direction, iters):
    pt = US.points_scene()
    return UR.camera_points(pt["uv"], pt["view_start"], pt["cam"], pt["out_intr"], direction, iters)


def raw_images(lib, images, cam, k4, H, W, mode, fill, out, valid):
    V, Hs, Ws, C = images.shape
    from ls2fm import _lib
    return lib.ls2fm_undistort_images(_lib.ptr(images), V, Hs, Ws, C, _lib.ptr(cam), _lib.ptr(k4), H, W, mode, (ctypes.c_float * C)(*fill),
                                      _lib.ptr(out), _lib.ptr(valid), _lib.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------- images
@pytest.mark.parametrize("src,out", US.SIZES)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_images_leave_the_bits_of_the_restatement(U, src, out, C):
    """three views with three cameras -- identity, barrel with tangential terms, rational -- in one call, both modes"""
    sc = US.image_scene(*src, *out, C)
    for mode, name in MODES:
        want, valid = restated_images(src, out, C, mode)
        got, gv = U.undistort_images(dev(sc["images"]), dev(sc["cam"]), dev(sc["out_intr"]), *out, mode=name)
        torch.cuda.synchronize()
        same(got, want, f"{name} out")
        same(gv, valid, f"{name} valid")
        assert got.dtype == torch.float32 and gv.dtype == torch.uint8


def test_the_hand_placed_edges_both_fills_and_valid_null(U):
    from ls2fm import _lib
    lib = _lib.load()
    sc = US.edge_scene()
    images, cam, k4 = dev(sc["images"]), dev(sc["cam"]), dev(sc["out_intr"])
    V = images.shape[0]
    for mode, name in MODES:
        for fill in (np.nan, [0.25, -3.0]):
            want, valid = UR.undistort_images(sc["images"], sc["cam"], sc["out_intr"], 8, 8, mode, fill)
            got, gv = U.undistort_images(images, cam, k4, 8, 8, mode=name, fill=fill)
            torch.cuda.synchronize()
            same(got, want, f"{name} out, fill {fill}")
            same(gv, valid, f"{name} valid, fill {fill}")
        # valid = NULL: the same pixels, nothing else written
        out = torch.full((V, 8, 8, 2), 7.0, device=DEV)
        assert raw_images(lib, images, cam, k4, 8, 8, mode, [0.25, -3.0], out, None) == 0
        torch.cuda.synchronize()
        same(out, want, f"{name} out without valid")
    # the NaN camera word spoils its own view only: with a sound word there, every other view keeps its bits
    sound = sc["cam"].copy()
    sound[US.EDGE_NAN, 5] = 0.0
    other, ov = U.undistort_images(images, dev(sound), k4, 8, 8)
    first, fv = U.undistort_images(images, cam, k4, 8, 8)
    keep = [v for v in range(V) if v != US.EDGE_NAN]
    same(other[keep], first[keep], "the other views")
    same(ov[keep], fv[keep], "the other views' valid")
    assert bool(ov[US.EDGE_NAN].any()) and not bool(fv[US.EDGE_NAN].any())
    grey, _ = U.undistort_images(images[..., 0], cam, k4, 8, 8)
    same(grey, first[..., 0], "grey")


def test_views_in_two_calls_a_rerun_a_replay_and_the_torch_form(U):
    from ls2fm import _lib
    lib = _lib.load()
    src, out, C = (33, 31), (15, 17), 3
    sc = US.image_scene(*src, *out, C)
    images, cam, k4 = dev(sc["images"]), dev(sc["cam"]), dev(sc["out_intr"])
    for mode, name in MODES:
        want, valid = restated_images(src, out, C, mode)
        parts = [U.undistort_images(images[s:e], cam[s:e], k4[s:e], *out, mode=name) for s, e in ((0, 1), (1, 3))]
        same(torch.cat([p[0] for p in parts]), want, f"{name}: two calls")
        same(torch.cat([p[1] for p in parts]), valid, f"{name}: two calls, valid")
        same(U.undistort_images(images, cam, k4, *out, mode=name)[0], want, f"{name}: rerun")
        form, fv = U._undistort_images_torch(images, cam, k4, *out, mode, [float("nan")] * C)
        same(form, want, f"{name}: the torch form on the device")
        same(fv, valid, f"{name}: the torch form's valid")
    want, valid = restated_images(src, out, C, UR.BILINEAR)
    res, ok = torch.zeros((3, *out, C), device=DEV), torch.zeros((3, *out), dtype=torch.uint8, device=DEV)

    def run():
        assert raw_images(lib, images, cam, k4, *out, UR.BILINEAR, [float("nan")] * C, res, ok) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                       # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        res.fill_(7)
        ok.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        same(res, want, "out, replay")
        same(ok, valid, "valid, replay")


# ---------------------------------------------------------------------------------------------------------------------- points
@pytest.mark.parametrize("iters", [0, 1, 10, 32])
def test_points_leave_the_bits_of_the_restatement(U, iters):
    """views of 0, 1, 63, 64, 65 and 257 points in one call; the principal point, a start whose det is exactly 0, a NaN point, an
    infinite camera word"""
    pt = US.points_scene()
    args = (dev(pt["uv"]), dev(pt["cam"]), dev(pt["view_start"]), dev(pt["out_intr"]))
    want, res = restated_points(UR.UNDISTORT, iters)
    got, gr = U.undistort_points(*args, iters=iters)
    torch.cuda.synchronize()
    same(got, want, "undistorted")
    same(gr, res, "residual")
    if iters == 0:
        want, res = restated_points(UR.DISTORT, 0)
        got, gr = U.distort_points(*args)
        same(got, want, "distorted")
        same(gr, res, "distort's residual")


def test_points_in_chunks_a_rerun_a_replay_and_the_torch_form(U):
    from ls2fm import _lib
    lib, p = _lib.load(), _lib.ptr
    pt = US.points_scene()
    uv, cam, vs, k4 = dev(pt["uv"]), dev(pt["cam"]), dev(pt["view_start"]), dev(pt["out_intr"])
    n, V = uv.shape[0], cam.shape[0]
    for direction in (UR.UNDISTORT, UR.DISTORT):
        want, res = restated_points(direction, 10 if direction == UR.UNDISTORT else 0)
        iters = 10 if direction == UR.UNDISTORT else 0
        form, fr = U._camera_points_torch(uv, vs, cam, k4, direction, iters)
        same(form, want, f"direction {direction}: the torch form on the device")
        same(fr, res, f"direction {direction}: the torch form's residual")
        # rows in two calls: the views 0 .. 3 with their table, then the rest with the table moved to the chunk's first row
        cut = int(pt["view_start"][4])
        out, rs = torch.zeros((n, 2), dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
        tail = (vs[4:] - cut).contiguous()
        assert lib.ls2fm_camera_points(p(uv), cut, p(vs[:5].contiguous()), 4, p(cam), p(k4), direction, iters, p(out), p(rs), _lib.stream_ptr()) == 0
        assert lib.ls2fm_camera_points(p(uv[cut:]), n - cut, p(tail), V - 4, p(cam[4:]), p(k4[4:]), direction, iters, p(out[cut:]), p(rs[cut:]),
                                       _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        same(out, want, f"direction {direction}: two calls")
        same(rs, res, f"direction {direction}: two calls, residual")
    want, res = restated_points(UR.UNDISTORT, 10)
    same(U.undistort_points(uv, cam, vs, k4)[0], want, "rerun")
    out, rs = torch.zeros((n, 2), dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)

    def run():
        assert lib.ls2fm_camera_points(p(uv), n, p(vs), V, p(cam), p(k4), UR.UNDISTORT, 10, p(out), p(rs), _lib.stream_ptr()) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        out.fill_(7)
        rs.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        same(out, want, "points, replay")
        same(rs, res, "residual, replay")
    # a table that ends before the last rows leaves them alone; residual = NULL
    out.fill_(7)
    short = vs.clone()
    short[-1] -= 2
    assert lib.ls2fm_camera_points(p(uv), n, p(short), V, p(cam), p(k4), UR.UNDISTORT, 10, p(out), None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    same(out[:-2], want[:-2], "short table")
    assert (host(out[-2:]) == 7).all()


def test_undistort_keypoints_moves_positions_only(U):
    pt = US.points_scene()
    V, cap = 3, 70
    rng = np.random.default_rng(4)
    kp = (rng.random((V * cap, 4)) * [47, 33, 4, 6.28]).astype(F32)
    counts = np.array([65, 0, 70], np.int32)
    cam, k = pt["cam"][1:4], pt["out_intr"][1:4]
    got = U.undistort_keypoints(dev(kp), dev(counts), dev(cam), dev(k))
    want, _ = UR.camera_points(kp[:, :2].astype(F64), np.arange(V + 1) * cap, cam, k, UR.UNDISTORT, 10)
    live = (np.arange(cap)[None, :] < counts[:, None]).reshape(-1)
    got = host(got)
    same(got[:, 2:], kp[:, 2:], "scale and orientation")
    same(got[~live, :2], kp[~live, :2], "rows past counts")
    same(got[live, :2], want[live].astype(F32), "positions")


# ---------------------------------------------------------------------------------------------------------------------- the chain
def test_undistort_views_feeds_the_plane_sweep(U):
    """the sphere scene's photographs re-imaged through a barrel lens on the host, undistorted on the device, swept: the bits of the
    sweep over the restatement's undistorted images.  Only the new code is under test: both sweeps are the same existing call."""
    import mvs_scenes
    from ls2fm import mvs
    sc = mvs_scenes.sphere_scene(hw=32)
    photos, cam = US.reimaged_sphere(32)
    images, intr, valid = U.undistort_views(dev(photos), dev(cam))
    torch.cuda.synchronize()
    H, W = images.shape[1:]
    K = host(intr)
    k4 = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)
    want, ok = UR.undistort_images(photos[..., None], np.tile(cam.astype(F32), (5, 1)), k4, H, W)
    same(images, want[..., 0], "undistorted photographs")
    same(valid, ok, "valid")
    assert ok.all() and np.isfinite(want).mean() > 0.3 and (H, W) != (32, 32)
    kw = dict(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])
    poses, sources, depths = dev(sc["poses"]), dev(sc["sources"]), dev(sc["depths"])
    got = mvs.plane_sweep(images, poses, intr, sources, depths, **kw)
    ref = mvs.plane_sweep(dev(want[..., 0]), poses, dev(K), sources, depths, **kw)
    torch.cuda.synchronize()
    for g, r, name in zip(got, ref, ("depth", "score", "plane")):
        same(g, r, name)
    assert np.isfinite(host(got[0])).mean() > 0.1
    k, Hn, Wn = U.undistorted_intrinsics(torch.from_numpy(cam), 32, 32)
    assert (Hn, Wn) == (H, W)
