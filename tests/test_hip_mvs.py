"""GPU: ls2fm_mvs_sweep and ls2fm_mvs_filter (csrc/mvs_sweep.hip) through ls2fm.mvs: every pixel's plane exactly, and score, depth and
the filter's outputs by their bits, against the numpy restatement (tests/mvs_restate.py); dense_reconstruct on top of them.  The
rules themselves, and that the scenes meet their edges, are judged on the restatement (tests/test_mvs_host.py)."""
import functools

import numpy as np
import pytest
import torch

import fusion_restate as FR
import mvs_restate as MR
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


def sweep_kw(sc):
    return dict(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"])


@functools.lru_cache(maxsize=None)
def restated(scene, *args):
    sc = getattr(S, scene)(*args)
    return MR.sweep(sc["images"], sc["poses"], sc["intr"], sc["sources"], sc["depths"], refs=sc.get("refs"), **sweep_kw(sc))


def on_device(MV, sc, rows=slice(None), **kw):
    refs = sc.get("refs")
    return MV.plane_sweep(dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"][rows]), dev(sc["depths"][rows]),
                          refs=None if refs is None else dev(refs[rows]), **sweep_kw(sc), **kw)


def check(got, ref, what=""):
    torch.cuda.synchronize()
    same(got[2], ref[2], f"plane {what}")
    same(got[1], ref[1], f"score {what}")
    same(got[0], ref[0], f"depth {what}")


# H, W, w, S, R, D, nan_pose, patches: an image smaller than a tile and its halo, one pixel past a tile in each axis, whole tiles;
# every w from 1 to 5 (each instantiation of the kernel; w = 4 is the first with three halo pixels per lane) with every image size,
# S, R, D and nan_pose varied across them
CASES = [(15, 16, 1, 1, 1, 1, False, False), (15, 16, 2, 3, 2, 2, False, False), (15, 16, 5, 5, 3, 17, False, False),
         (17, 33, 1, 5, 3, 17, False, True), (17, 33, 2, 3, 3, 3, True, False), (17, 33, 5, 1, 3, 17, False, False),
         (17, 33, 1, 5, 3, 17, True, False), (32, 48, 1, 5, 1, 2, False, False), (32, 48, 2, 3, 3, 17, False, True),
         (32, 48, 5, 5, 2, 3, True, False),
         (15, 16, 3, 3, 3, 3, True, False), (15, 16, 4, 5, 2, 17, False, False), (17, 33, 3, 5, 3, 17, False, False),
         (17, 33, 4, 1, 1, 2, False, False), (32, 48, 3, 5, 2, 17, True, False), (32, 48, 4, 3, 3, 3, False, False)]


@pytest.mark.parametrize("H,W,w,S_,R,D,nan_pose,patches", CASES)
def test_bits_of_the_restatement(MV, H, W, w, S_, R, D, nan_pose, patches):
    args = (H, W, w, S_, R, D, nan_pose, patches)
    ref = restated("grid_scene", *args)
    check(on_device(MV, S.grid_scene(*args)), ref)
    if S_ > 1:
        assert (ref[2] >= 0).any() and (ref[2] < 0).any()


def test_the_den_and_the_exact_scenes(MV):
    sc = S.den_scene()
    ref = restated("den_scene")
    y, x = sc["pixel"]
    assert ref[2][0, y, x] == 1 and ref[0][0, y, x] == 1.0
    check(on_device(MV, sc), ref, "den == 0")
    for last in (False, True):
        sc = S.exact_scene(last)
        got = on_device(MV, sc)
        check(got, restated("exact_scene", last), "exact")
        inner = host(got[2])[0] >= 0
        assert inner.sum() == (sc["H"] - 4) * (sc["W"] - 4) and (host(got[1])[0][inner] == 1.0).all() and (host(got[0])[0][inner] == 4.0).all()


def test_the_torch_form_on_the_device_gives_the_kernel_s_bits(MV):
    args = (17, 33, 2, 5, 3, 17, False, False)
    sc = S.grid_scene(*args)
    got = MV.plane_sweep_torch(dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"]), dev(sc["depths"]), refs=dev(sc["refs"]),
                               **sweep_kw(sc))
    check(got, restated("grid_scene", *args), "torch form")
    fs = S.filter_scene(17, 33)
    kw = dict(near=fs["near"], max_reproj=fs["max_reproj"], rel_depth=fs["rel_depth"], min_consistent=2)
    f, c = MV.filter_depths_torch(dev(fs["depth"]), dev(fs["poses"]), dev(fs["intr"]), dev(fs["sources"]), **kw)
    rf, rc = MR.filter_depths(fs["depth"], fs["poses"], fs["intr"], fs["sources"], **kw)
    same(c, rc, "count, torch form")
    same(f, rf, "filtered, torch form")


def test_references_in_chunks_a_rerun_and_a_replay(MV):
    args = (17, 33, 2, 5, 3, 17, False, False)
    sc = S.grid_scene(*args)
    ref = restated("grid_scene", *args)
    check(on_device(MV, sc), ref, "one call")
    check(on_device(MV, sc, max_workspace_bytes=1), ref, "one reference per chunk")
    for r in range(3):
        part = on_device(MV, sc, slice(r, r + 1))
        check(part, tuple(t[r:r + 1] for t in ref), f"reference {r} alone")
    check(on_device(MV, sc), ref, "rerun")
    inputs = [dev(sc[k]) for k in ("images", "poses", "intr", "sources", "depths", "refs")]
    run = lambda: MV.plane_sweep(*inputs[:5], refs=inputs[5], **sweep_kw(sc))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                       # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        for t in out:
            t.fill_(7)
        graph.replay()
        check(out, ref, "replay")


FILTER_CASES = [(15, 16, 1, False, 1), (15, 16, 5, False, 0), (17, 33, 5, False, 2), (17, 33, 3, True, 2), (17, 33, 5, False, 6),
                (32, 48, 3, False, 1), (32, 48, 5, True, 3)]


@pytest.mark.parametrize("H,W,S_,nan_pose,min_consistent", FILTER_CASES)
def test_filter_bits_of_the_restatement(MV, H, W, S_, nan_pose, min_consistent):
    sc = S.filter_scene(H, W, S_, nan_pose)
    kw = dict(near=sc["near"], max_reproj=sc["max_reproj"], rel_depth=sc["rel_depth"], min_consistent=min_consistent)
    rf, rc = MR.filter_depths(sc["depth"], sc["poses"], sc["intr"], sc["sources"], **kw)
    args = (dev(sc["depth"]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["sources"]))
    f, c = MV.filter_depths(*args, **kw)
    torch.cuda.synchronize()
    assert c.dtype == torch.uint8
    same(c, rc, "count")
    same(f, rf, "filtered")
    if min_consistent == 0:
        same(f, sc["depth"], "min_consistent 0 keeps every pixel")
    if min_consistent > S_:
        assert np.isnan(host(f)).all()
    if (H, W, S_) == (17, 33, 5) and min_consistent == 2:
        f2, c2 = MV.filter_depths(*args, **kw)                      # a rerun and a replay
        same(c2, rc, "count, rerun")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            MV.filter_depths(*args, **kw)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            f3, c3 = MV.filter_depths(*args, **kw)
        f3.fill_(7)
        c3.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        same(c3, rc, "count, replay")
        same(f3, rf, "filtered, replay")


def test_dense_reconstruct_equals_the_restated_route(MV):
    """the sphere scene end to end: the filtered depth maps by their bits, then the mesh against fusion_restate (and through it
    mc_restate) on the restated depth maps"""
    sc = S.sphere_scene()
    opt = MV.MvsOptions(half_width=sc["half_width"], near=sc["near"], min_var=sc["min_var"], min_sources=sc["min_sources"],
                        max_reproj=sc["max_reproj"], rel_depth=sc["rel_depth"], min_consistent=sc["min_consistent"])
    out, filtered, count = MV.dense_reconstruct(dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), sc["bounds"], sc["voxel"],
                                                sources=dev(sc["sources"]), depths=dev(sc["depths"]), options=opt, return_depth=True)
    torch.cuda.synchronize()
    depth = restated("sphere_scene")[0]
    rf, rc = MR.filter_depths(depth, sc["poses"], sc["intr"], sc["sources"], near=sc["near"], max_reproj=sc["max_reproj"],
                              rel_depth=sc["rel_depth"], min_consistent=sc["min_consistent"])
    same(count, rc, "count")
    same(filtered, rf, "filtered")
    lo, hi = sc["bounds"]
    shape = tuple(max(2, int(np.ceil((h - l) / sc["voxel"])) + 1) for l, h in zip(lo, hi))
    state = FR.fuse(shape, lo, sc["voxel"], 3.0 * sc["voxel"], rf, sc["poses"], sc["intr"], near=sc["near"])
    v, f = FR.extract(state[0], state[1], lo, sc["voxel"])
    assert len(f) > 300
    same(out.vertices, v, "vertices")
    same(out.faces, f, "faces")
    # the surface is the sphere's: every vertex within two voxels of it
    r = np.linalg.norm(host(out.vertices).astype(np.float64), axis=1)
    assert (np.abs(r - S.SPHERE_R) <= 2 * sc["voxel"]).all()
    # the defaults run: sources by select_sources, planes from the bounds
    auto = MV.dense_reconstruct(dev(sc["images"]), dev(sc["poses"]), dev(sc["intr"]), sc["bounds"], sc["voxel"],
                                options=MV.MvsOptions(half_width=2, n_planes=32, min_var=sc["min_var"]))
    assert auto.faces.shape[0] > 100 and bool(torch.isfinite(auto.vertices).all())


def test_refusals_and_empty_calls(MV):
    from ls2fm import _lib, _posed
    lib = _lib.load()
    sc = S.grid_scene(15, 16)
    img, src, dep, refs = dev(sc["images"]), dev(sc["sources"]).int(), dev(sc["depths"]), dev(sc["refs"]).int()
    poses, k4 = _posed.views(dev(sc["poses"]), dev(sc["intr"]), "test")
    rel = MV.relative_poses(poses, refs, src)
    back = MV.relative_poses(poses, refs, src, back=True)
    depth, score = torch.zeros(3, 15, 16, device=DEV), torch.zeros(3, 15, 16, device=DEV)
    plane = torch.zeros(3, 15, 16, dtype=torch.int32, device=DEV)
    p, s = _lib.ptr, _lib.stream_ptr()
    inf, nan = float("inf"), float("nan")

    def sweep(im=img, V=6, H=15, W=16, rf=refs, R=3, sr=src, S_=5, dp=dep, D=17, rl=rel, k=k4, w=1, near=0.5, min_var=0.01, min_sources=2,
              od=depth, os_=score, op=plane):
        return lib.ls2fm_mvs_sweep(p(im), V, H, W, p(rf), R, p(sr), S_, p(dp), D, p(rl), p(k), w, near, min_var, min_sources, p(od), p(os_),
                                   p(op), s)
    assert sweep() == 0
    for kw in (dict(im=None), dict(rf=None), dict(sr=None), dict(dp=None), dict(rl=None), dict(k=None), dict(od=None), dict(os_=None),
               dict(op=None), dict(V=-1), dict(V=0), dict(H=0), dict(W=32769), dict(R=-1), dict(S_=0), dict(S_=65), dict(D=0), dict(D=65537),
               dict(w=0), dict(w=6), dict(near=0.0), dict(near=nan), dict(near=inf), dict(min_var=-1.0), dict(min_var=nan), dict(min_var=inf),
               dict(min_sources=0), dict(min_sources=6)):
        assert sweep(**kw) == -1, kw
    assert sweep(R=0, rf=None, od=None, os_=None, op=None) == 0

    fd = dev(S.filter_scene(15, 16)["depth"])
    fsrc = dev(S.filter_scene(15, 16)["sources"]).int()
    every = torch.arange(6, device=DEV)
    frel, fback = MV.relative_poses(poses, every, fsrc), MV.relative_poses(poses, every, fsrc, back=True)
    count = torch.zeros(6, 15, 16, dtype=torch.uint8, device=DEV)
    out = torch.zeros(6, 15, 16, device=DEV)

    def filt(d=fd, V=6, H=15, W=16, sr=fsrc, S_=5, rl=frel, bk=fback, k=k4, near=0.5, max_reproj=1.0, rel_depth=0.25, min_consistent=2,
             c=count, o=out):
        return lib.ls2fm_mvs_filter(p(d), V, H, W, p(sr), S_, p(rl), p(bk), p(k), near, max_reproj, rel_depth, min_consistent, p(c), p(o), s)
    assert filt() == 0
    for kw in (dict(d=None), dict(sr=None), dict(rl=None), dict(bk=None), dict(k=None), dict(c=None), dict(o=None), dict(V=-1), dict(H=0),
               dict(W=32769), dict(S_=0), dict(S_=65), dict(near=0.0), dict(near=nan), dict(max_reproj=-1.0), dict(max_reproj=nan),
               dict(max_reproj=inf), dict(rel_depth=-1.0), dict(rel_depth=nan), dict(min_consistent=-1)):
        assert filt(**kw) == -1, kw
    assert filt(V=0, d=None, c=None, o=None) == 0
    torch.cuda.synchronize()
    del back
    # a reference outside [0, V) has no valid pixel; a source outside [0, V) is skipped like -1
    got = MV.plane_sweep(img, dev(sc["poses"]), dev(sc["intr"]), src[:2], dep[:2], refs=torch.tensor([0, 6], device=DEV), **sweep_kw(sc))
    torch.cuda.synchronize()
    assert (host(got[2])[1] == -1).all() and np.isnan(host(got[0])[1]).all() and (host(got[2])[0] >= 0).any()
    far = src.clone()
    far[far < 0] = 6
    check(MV.plane_sweep(img, dev(sc["poses"]), dev(sc["intr"]), far, dep, refs=refs, **sweep_kw(sc)), restated("grid_scene", 15, 16))
    # CPU tensors and bad arguments
    with pytest.raises(RuntimeError, match=r"ls2fm\.mvs"):
        MV.plane_sweep(img.cpu(), dev(sc["poses"]), dev(sc["intr"]), src, dep, refs=refs)
    with pytest.raises(ValueError):
        MV.plane_sweep(img, dev(sc["poses"]), dev(sc["intr"]), src, dep, refs=refs, half_width=6)
    with pytest.raises(ValueError):
        MV.filter_depths(fd, dev(sc["poses"]), dev(sc["intr"]), fsrc, min_consistent=-1)
