"""GPU: ls2fm_mvs_fuse_mark and ls2fm_mvs_fuse_emit (csrc/mvs_fuse.hip) through ls2fm.mvs.fuse_depths: every pixel's support and every
row's point, normal, colour and pixel by their bits against the numpy restatement (tests/fuse_restate.py); the torch form, the view
ranges, a rerun and a replay; dense_reconstruct through the cloud.  The rule itself, and that the edge scene meets its edges, are
judged on the restatement (tests/test_fuse_host.py)."""
import functools

import numpy as np
import pytest
import torch

import fuse_restate as FR
import fuse_scenes as FS
import mvs_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


@pytest.fixture(scope="module")
def MV():
    from ls2fm import mvs
    return mvs


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
def restated(H, W, S_, C, nan_pose, normals, colours):
    sc = FS.edge_scene(H, W, S_, C, nan_pose)
    return FR.fuse(sc["depth"], sc["poses"], sc["intr"], sc["sources"], normal=sc["normal"] if normals else None,
                   colour=sc["colour"] if colours else None, **FS.fuse_kw(sc))


def check(got, want, sc, what=""):
    """a FusedCloud against the restatement's dict: the support of every pixel, every row"""
    torch.cuda.synchronize()
    same(got.pixel, want["pixel"], f"pixel {what}")
    sup = np.zeros(want["support"].size, np.uint8)
    sup[host(got.pixel)] = host(got.support)
    same(sup.reshape(want["support"].shape), want["support"], f"support {what}")
    for name, g in (("points", got.points), ("normals", got.normals), ("colours", got.colors)):
        if want[name] is None:
            assert g is None, f"{name} {what}"
        else:
            same(g, want[name], f"{name} {what}")
    same(got.view, want["pixel"] // (sc["H"] * sc["W"]), f"view {what}")
    same(got.centers, FR.cam_to_world(sc["poses"])[:, :, 3][host(got.view)], f"centers {what}")


def on_device(fn, sc, normals=True, colours=True, **kw):
    return fn(dev(sc["depth"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"]), normal=dev(sc["normal"]) if normals else None,
              images=dev(sc["colour"]) if colours else None, **FS.fuse_kw(sc), **kw)


# S, C, nan_pose, normals, colours: every S and C of the lists, with and without normals and colours, with the NaN pose; each with
# every image size of fuse_scenes.EDGE_SIZES -- one pixel, the sizes around 16 and 32, a whole 32 x 8 tile, one pixel past each of its edges
COMBOS = [(5, 3, False, True, True), (2, 1, True, True, False), (1, 4, False, False, True), (5, 4, True, False, False),
          (2, 3, False, True, True)]


@pytest.mark.parametrize("H,W", FS.EDGE_SIZES)
@pytest.mark.parametrize("S_,C,nan_pose,normals,colours", COMBOS)
def test_bits_of_the_restatement(MV, H, W, S_, C, nan_pose, normals, colours):
    sc = FS.edge_scene(H, W, S_, C, nan_pose)
    want = restated(H, W, S_, C, nan_pose, normals, colours)
    got = on_device(MV.fuse_depths, sc, normals, colours)
    check(got, want, sc)
    assert got.support.dtype == torch.uint8 and got.pixel.dtype == torch.int64 and len(want["pixel"]) > 0
    if H > 1:
        assert (want["support"] == 0).any() and (want["support"] >= 2).any()


def test_the_torch_form_on_the_device_gives_the_kernel_s_bits(MV):
    args = (17, 33, 5, 3, False, True, True)
    sc = FS.edge_scene(*args[:5])
    got = on_device(MV.fuse_depths_torch, sc)
    check(got, restated(*args), sc, "torch form")
    kernel = on_device(MV.fuse_depths, sc)
    for name in ("points", "normals", "colors", "support", "view", "pixel", "centers"):
        same(getattr(got, name), getattr(kernel, name), f"{name}, torch form against the kernels")


def raw_arguments(MV, sc):
    """what the two entry points take, formed as fuse_depths forms it"""
    from ls2fm import _posed
    poses, k4 = _posed.views(dev(sc["poses"]), dev(sc["intr"]), "test")
    V = poses.shape[0]
    src = dev(sc["sources"]).int().contiguous()
    every = torch.arange(V, device=DEV)
    return dict(d=dev(sc["depth"]), n=dev(sc["normal"]), c=dev(sc["colour"]), src=src, rel=MV.relative_poses(poses, every, src),
                back=MV.relative_poses(poses, every, src, back=True), k4=k4, c2w=MV.cam_to_world(poses), V=V, H=sc["H"], W=sc["W"],
                S=src.shape[1], C=sc["colour"].shape[3], cos2=float(FR.cos2_of(sc["max_normal_angle"])))


def test_view_ranges_a_rerun_and_a_replay(MV):
    from ls2fm import _lib
    lib, p = _lib.load(), _lib.ptr
    args = (17, 33, 5, 3, False, True, True)
    sc = FS.edge_scene(*args[:5])
    want = restated(*args)
    H, W = sc["H"], sc["W"]
    check(on_device(MV.fuse_depths, sc), want, sc, "one call")
    check(on_device(MV.fuse_depths, sc, max_workspace_bytes=1), want, sc, "one view per chunk")
    check(on_device(MV.fuse_depths, sc, max_workspace_bytes=2 * 24 * H * W), want, sc, "two views per chunk")
    check(on_device(MV.fuse_depths, sc), want, sc, "rerun")
    some = on_device(MV.fuse_depths, sc, min_support=2)
    keep = want["support"].reshape(-1)[want["pixel"]] >= 2
    same(some.pixel, want["pixel"][keep], "pixel, min_support 2")
    same(some.points, want["points"][keep], "points, min_support 2")

    # both launches replayed from one captured graph; `row` is prepared outside the capture, from the support of an eager call
    a = raw_arguments(MV, sc)
    V, M = a["V"], len(want["pixel"])
    support = torch.zeros((V, H, W), dtype=torch.uint8, device=DEV)
    points, normals = torch.zeros((M, 3), device=DEV), torch.zeros((M, 3), device=DEV)
    colours, pixel = torch.zeros((M, a["C"]), device=DEV), torch.zeros((M,), dtype=torch.int64, device=DEV)
    shared = (p(a["src"]), a["S"], p(a["rel"]), p(a["back"]), p(a["k4"]))
    tail = (sc["near"], sc["max_reproj"], sc["rel_depth"], a["cos2"], 0, V)
    row = dev(np.cumsum(want["support"].reshape(-1) > 0) - (want["support"].reshape(-1) > 0)).contiguous()
    assert row.dtype == torch.int64

    def run():
        s = _lib.stream_ptr()
        assert lib.ls2fm_mvs_fuse_mark(p(a["d"]), p(a["n"]), V, H, W, *shared, *tail, p(support), s) == 0
        assert lib.ls2fm_mvs_fuse_emit(p(a["d"]), p(a["n"]), p(a["c"]), a["C"], V, H, W, *shared, p(a["c2w"]), *tail, p(support), p(row), M,
                                       p(points), p(normals), p(colours), p(pixel), s) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                       # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        for t in (support, points, normals, colours, pixel):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        same(support, want["support"], "support, replay")
        same(pixel, want["pixel"], "pixel, replay")
        same(points, want["points"], "points, replay")
        same(normals, want["normals"], "normals, replay")
        same(colours, want["colours"], "colours, replay")


def test_dense_reconstruct_through_the_cloud_equals_the_restated_route(MV):
    """the sphere scene at 32 x 32 end to end with PatchMatch and Poisson: the fused cloud by its bits against the restatement on the
    filtered maps, the mesh against mesh_from_cloud on the restated cloud; surface="tsdf" is the call without the keyword"""
    from ls2fm import cloud_mesh
    sc = S.sphere_scene(hw=32)
    opt = MV.MvsOptions(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"],
                        max_reproj=sc["max_reproj"], rel_depth=sc["rel_depth"], min_consistent=sc["min_consistent"], iterations=2)
    depths = np.broadcast_to(np.linspace(1.9, 2.6, 16).astype(F32), (5, 16)).copy()
    views = (dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]))
    kw = dict(sources=dev(sc["sources"]), depths=dev(depths), options=opt)
    out, filtered, count, world, cloud = MV.dense_reconstruct(*views, sc["bounds"], sc["voxel"], return_depth=True, stereo="patchmatch",
                                                              surface="poisson", **kw)
    torch.cuda.synchronize()
    depth, normal, _ = MV.patch_match(*views, dev(sc["sources"]), dev(depths), **opt.patchmatch())
    again, _ = MV.filter_depths(depth, views[1], views[2], dev(sc["sources"]), **opt.filter())
    same(filtered, again, "filtered")
    want = FR.fuse(host(filtered), sc["poses"], sc["intr"], sc["sources"], normal=host(normal), colour=sc["images"][..., None], near=sc["near"],
                   max_reproj=sc["max_reproj"], rel_depth=sc["rel_depth"], max_normal_angle=opt.max_normal_angle)
    assert len(want["pixel"]) > 100 and 2 * len(want["pixel"]) < np.isfinite(host(filtered)).sum()
    check(cloud, want, sc, "dense_reconstruct's cloud")
    mesh = cloud_mesh.mesh_from_cloud(dev(want["points"]), normals=dev(want["normals"]), voxel=sc["voxel"], method="poisson",
                                      bounds=sc["bounds"])
    assert mesh.faces.shape[0] > 100
    same(out.vertices, mesh.vertices, "vertices")
    same(out.faces, mesh.faces, "faces")
    # the sweep has no normals: they are estimated toward each point's camera; the local surface runs as well
    mls = MV.dense_reconstruct(*views, sc["bounds"], sc["voxel"], return_depth=True, surface="mls", **kw)
    assert len(mls) == 4 and mls[3].normals is None and mls[3].points.shape[0] > 0 and bool(torch.isfinite(mls[0].vertices).all())
    # the default is the path of before
    plain = MV.dense_reconstruct(*views, sc["bounds"], sc["voxel"], **kw)
    tsdf = MV.dense_reconstruct(*views, sc["bounds"], sc["voxel"], surface="tsdf", **kw)
    assert plain.faces.shape[0] > 0
    same(tsdf.vertices, plain.vertices, "tsdf vertices")
    same(tsdf.faces, plain.faces, "tsdf faces")


def test_refusals_and_empty_calls(MV):
    from ls2fm import _lib
    lib, p, s = _lib.load(), _lib.ptr, _lib.stream_ptr()
    sc = FS.edge_scene(15, 17)
    a = raw_arguments(MV, sc)
    want = restated(15, 17, 5, 3, False, True, True)
    M = len(want["pixel"])
    support = dev(want["support"])
    row = dev(np.cumsum(want["support"].reshape(-1) > 0) - (want["support"].reshape(-1) > 0))
    points, normals = torch.zeros((M, 3), device=DEV), torch.zeros((M, 3), device=DEV)
    colours, pixel = torch.zeros((M, 3), device=DEV), torch.zeros((M,), dtype=torch.int64, device=DEV)
    inf, nan = float("inf"), float("nan")

    def mark(d=a["d"], n=a["n"], V=6, H=15, W=17, sr=a["src"], S_=5, rl=a["rel"], bk=a["back"], k=a["k4"], near=0.5, max_reproj=1.0,
             rel_depth=0.25, cos2=0.5, begin=0, end=6, sup=support):
        return lib.ls2fm_mvs_fuse_mark(p(d), p(n), V, H, W, p(sr), S_, p(rl), p(bk), p(k), near, max_reproj, rel_depth, cos2, begin, end, p(sup), s)

    def emit(d=a["d"], n=a["n"], c=a["c"], C=3, V=6, H=15, W=17, sr=a["src"], S_=5, rl=a["rel"], bk=a["back"], k=a["k4"], w=a["c2w"], near=0.5,
             max_reproj=1.0, rel_depth=0.25, cos2=0.5, begin=0, end=6, sup=support, rw=row, rows=M, pt=points, nm=normals, cl=colours, px=pixel):
        return lib.ls2fm_mvs_fuse_emit(p(d), p(n), p(c), C, V, H, W, p(sr), S_, p(rl), p(bk), p(k), p(w), near, max_reproj, rel_depth, cos2,
                                       begin, end, p(sup), p(rw), rows, p(pt), p(nm), p(cl), p(px), s)
    shared = (dict(d=None), dict(sr=None), dict(rl=None), dict(bk=None), dict(k=None), dict(sup=None), dict(V=-1), dict(H=0), dict(W=32769),
              dict(S_=0), dict(S_=65), dict(near=0.0), dict(near=nan), dict(max_reproj=-1.0), dict(max_reproj=nan), dict(rel_depth=inf),
              dict(cos2=-0.5), dict(cos2=1.5), dict(cos2=nan), dict(begin=-1), dict(end=7), dict(begin=4, end=3))
    assert mark() == 0 and emit() == 0
    for kw in shared:
        assert mark(**kw) == -1, kw
    for kw in shared + (dict(w=None), dict(rw=None), dict(pt=None), dict(px=None), dict(C=0), dict(C=5), dict(c=None), dict(cl=None),
                        dict(nm=None), dict(n=None), dict(rows=-1)):
        assert emit(**kw) == -1, kw
    # without normals or colours both sides are NULL; no views, an empty range and no rows return at once
    assert emit(n=None, nm=None) == 0 and emit(c=None, cl=None, C=0) == 0
    assert mark(V=0, begin=0, end=0, d=None, sup=None) == 0 and mark(begin=3, end=3, d=None, sup=None) == 0
    assert emit(V=0, begin=0, end=0, d=None, sup=None, rw=None, pt=None, px=None) == 0 and emit(begin=6, end=6, d=None) == 0
    assert emit(rows=0, pt=None, px=None) == 0
    # a row outside [0, n_rows) is not written
    pixel.fill_(-7)
    assert emit(rows=M - 5) == 0
    torch.cuda.synchronize()
    same(pixel[:M - 5], want["pixel"][:M - 5], "rows below n_rows")
    assert (host(pixel[M - 5:]) == -7).all()
    # depth maps without a depth: no rows, no launch of emit; no views
    blank = dict(sc, depth=np.full_like(sc["depth"], np.nan))
    none = on_device(MV.fuse_depths, blank)
    assert none.points.shape == (0, 3) and none.normals.shape == (0, 3) and none.colors.shape == (0, 3) and none.pixel.shape == (0,)
    empty = MV.fuse_depths(torch.zeros(0, 15, 17, device=DEV), torch.zeros(0, 3, 4, device=DEV), dev(sc["intr"]),
                           torch.zeros(0, 5, dtype=torch.int32, device=DEV))
    assert empty.points.shape == (0, 3) and empty.centers.shape == (0, 3) and empty.normals is None
    # CPU tensors and bad arguments
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs"):
        MV.fuse_depths(dev(sc["depth"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"]), normal=torch.from_numpy(sc["normal"]))
    with pytest.raises(ValueError):
        on_device(MV.fuse_depths, sc, min_support=0)
    with pytest.raises(ValueError):
        MV.fuse_depths(dev(sc["depth"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"]), **dict(FS.fuse_kw(sc), max_normal_angle=120.0))
