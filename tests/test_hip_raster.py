"""GPU: ls2fm.raster -- the rasteriser (csrc/rasterize.hip) against the numpy restatement (tests/raster_restate.py) on the scenes of
tests/raster_scenes.py, and mask_votes and clean_mesh on top of it.

The rasterisation rule makes the images a pure function of the inputs, so face_id is compared exactly and depth and the
barycentrics by their BITS, on every pixel of every view of every scene, no pixel excluded; tests/test_raster_host.py asserts that
the scenes hold the cases a wrong kernel fails."""
import ctypes

import numpy as np
import pytest
import torch

import raster_restate as R
import raster_scenes as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def RS():
    from ls2fm import raster
    return raster


def dev(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def run(RS, sc, views=slice(None), **kw):
    return RS.rasterize(dev(sc["verts"]), dev(sc["faces"]), dev(sc["poses"][views]), dev(sc["intr"]), sc["H"], sc["W"], near=sc["near"], **kw)


def bits(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def mismatch(out, exp, views=slice(None)):
    """'' when face_id, the bits of depth and (where returned) of the barycentrics and the hits equal the restatement's"""
    torch.cuda.synchronize()
    fid = out.face_id.cpu().numpy()
    if fid.dtype != np.int32 or not np.array_equal(fid, exp["face_id"][views]):
        return f"face_id differs on {int((fid != exp['face_id'][views]).sum())} pixels"
    if not np.array_equal(bits(out.depth), exp["depth"][views].view(np.uint32)):
        return f"depth bits differ on {int((bits(out.depth) != exp['depth'][views].view(np.uint32)).sum())} pixels"
    if out.bary is not None and not np.array_equal(bits(out.bary), exp["bary"][views].view(np.uint32)):
        return f"bary bits differ on {int((bits(out.bary) != exp['bary'][views].view(np.uint32)).any(axis=-1).sum())} pixels"
    return ""


@pytest.mark.parametrize("name", S.NAMES)
def test_rasteriser_equals_restatement_on_every_pixel(RS, name):
    sc, exp = S.scenes()[name], S.expected(name)
    out = run(RS, sc, bary=True, hits=True)
    assert out.face_id.shape == (len(sc["poses"]), sc["H"], sc["W"]) and out.bary.shape == out.face_id.shape + (3,)
    assert mismatch(out, exp) == "", name
    hits = out.face_hits.cpu().numpy()
    assert hits.dtype == np.int32 and np.array_equal(hits, exp["face_hits"])
    fid = out.face_id.cpu().numpy()
    assert np.array_equal(hits, np.bincount(fid[fid >= 0], minlength=len(sc["faces"])))
    plain = run(RS, sc)
    assert plain.bary is None and plain.face_hits is None and mismatch(plain, exp) == ""


def test_marching_cubes_mesh_of_many_tiny_faces(RS):
    """ls2fm.mesh.marching_cubes of a 32^3 sphere-plus-box volume, 2 views at 96 x 128: thousands of faces of a few pixels each"""
    from ls2fm import mesh
    g = torch.linspace(-1.0, 1.0, 32, device=DEV)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    sphere = (x * x + y * y + z * z).sqrt() - 0.55
    q = torch.stack([(x - 0.45).abs() - 0.3, (y + 0.1).abs() - 0.25, (z - 0.2).abs() - 0.35], dim=-1)
    box = q.clamp(min=0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0)
    verts, faces = mesh.marching_cubes(torch.minimum(sphere, box), 0.0, spacing=(2 / 31,) * 3, origin=(-1.0,) * 3)
    assert 2000 < faces.shape[0] < 20000
    poses = np.stack([S.look_at((0.4, 0.5, -2.6), (0.1, 0, 0)), S.look_at((2.0, -0.8, 1.4), (0.1, 0, 0.1))])
    K = S.intrinsics(120.0, 64.0, 48.0)
    exp = R.rasterize(verts.cpu().numpy(), faces.cpu().numpy(), poses, K, 96, 128)
    out = RS.rasterize(verts, faces, dev(poses), dev(K), 96, 128, bary=True, hits=True)
    assert mismatch(out, exp) == ""
    assert np.array_equal(out.face_hits.cpu().numpy(), exp["face_hits"]) and (exp["face_id"] >= 0).sum() > 3000
    assert np.median(exp["face_hits"][exp["face_hits"] > 0]) <= 8


def test_views_chunks_reruns_do_not_show(RS):
    sc, exp = S.scenes()["sphere"], S.expected("sphere")
    whole = run(RS, sc, bary=True, hits=True)
    assert mismatch(whole, exp) == ""
    hits = torch.zeros_like(whole.face_hits)
    for n in range(3):                                             # one call over 3 views equals three calls
        one = run(RS, sc, views=slice(n, n + 1), bary=True, hits=True)
        assert mismatch(one, exp, slice(n, n + 1)) == ""
        hits += one.face_hits
    assert torch.equal(hits, whole.face_hits)
    chunked = run(RS, sc, bary=True, hits=True, max_workspace_bytes=1)          # one view per chunk
    again = run(RS, sc, bary=True, hits=True)                                   # a second run
    per_view = RS.rasterize(dev(sc["verts"]), dev(sc["faces"]), dev(sc["poses"]), dev(np.stack([sc["intr"]] * 3)), sc["H"], sc["W"],
                            near=sc["near"], bary=True, hits=True)             # intrinsics given per view
    for other in (chunked, again, per_view):
        assert torch.equal(other.face_id, whole.face_id) and torch.equal(other.depth.view(torch.int32), whole.depth.view(torch.int32))
        assert torch.equal(other.bary.view(torch.int32), whole.bary.view(torch.int32)) and torch.equal(other.face_hits, whole.face_hits)
    single = RS.rasterize(dev(sc["verts"]), dev(sc["faces"]), dev(sc["poses"][1]), dev(sc["intr"]), sc["H"], sc["W"])      # pose [3, 4]
    assert single.face_id.shape == (1, 48, 64) and torch.equal(single.face_id[0], whole.face_id[1])


def test_more_views_than_the_grid_has_rows(RS):
    """the kernels take the view from blockIdx.y, at most 65535 of them, and loop over the rest: 65605 views of the 1 x 1 scene, the
    first 65538 looking at it and the others past it"""
    sc = S.scenes()["one_pixel"]
    n, looking = 65535 + 70, 65535 + 3
    poses = np.repeat(sc["poses"], n, axis=0)
    poses[looking:, 0, 3] = 50.0
    v, f, p, k = dev(sc["verts"]), dev(sc["faces"]), dev(poses), dev(sc["intr"])
    out = RS.rasterize(v, f, p, k, 1, 1, bary=True, hits=True)
    fid = out.face_id.cpu().numpy().reshape(-1)
    assert (fid[:looking] == 0).all() and (fid[looking:] == -1).all() and out.face_hits.tolist() == [looking, 0]
    depth = bits(out.depth).reshape(-1)
    assert (depth[:looking] == np.float32(2).view(np.uint32)).all() and (depth[looking:] == R.INF_BITS).all()
    tail = RS.rasterize(v, f, p[65530:], k, 1, 1, bary=True)
    assert torch.equal(tail.face_id, out.face_id[65530:]) and torch.equal(tail.bary.view(torch.int32), out.bary[65530:].view(torch.int32))
    m = torch.ones(n, 1, 1, dtype=torch.uint8, device=DEV)
    seen, inside = RS.mask_votes(v, p, k, m)
    want = R.mask_votes(sc["verts"], poses[looking - 2:looking + 2], sc["intr"], np.ones((4, 1, 1), np.uint8))
    few = RS.mask_votes(v, p[looking - 2:looking + 2], k, m[:4])
    assert np.array_equal(few[0].cpu().numpy(), want[0]) and torch.equal(seen, inside) and int(seen.max()) <= looking


def test_captured_call_replays_to_the_eager_result(RS):
    sc, exp = S.scenes()["ties"], S.expected("ties")
    v, f, p, k = dev(sc["verts"]), dev(sc["faces"]), dev(sc["poses"]), dev(sc["intr"])
    call = lambda: RS.rasterize(v, f, p, k, sc["H"], sc["W"], near=sc["near"], bary=True, hits=True)
    eager = call()
    assert mismatch(eager, exp) == ""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                     # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(2):
        out.face_id.fill_(-7)
        out.depth.fill_(-1.0)
        out.bary.fill_(-1.0)
        graph.replay()
        assert mismatch(out, exp) == ""
        assert torch.equal(out.face_hits, eager.face_hits)         # zeroed inside the graph, so a replay does not add to the last


def test_no_views_and_no_faces(RS):
    sc = S.scenes()["ties"]
    none = RS.rasterize(dev(sc["verts"]), dev(sc["faces"]), torch.zeros(0, 3, 4, device=DEV), dev(sc["intr"]), 48, 64, bary=True, hits=True)
    assert none.face_id.shape == (0, 48, 64) and none.bary.shape == (0, 48, 64, 3) and int(none.face_hits.sum()) == 0
    empty = RS.rasterize(dev(sc["verts"]), torch.zeros(0, 3, dtype=torch.int32, device=DEV), dev(sc["poses"]), dev(sc["intr"]), 48, 64,
                         bary=True, hits=True)
    torch.cuda.synchronize()
    assert bool((empty.face_id == -1).all()) and bool(torch.isposinf(empty.depth).all()) and bool((empty.bary == 0).all())
    assert empty.face_hits.numel() == 0
    bare = RS.rasterize(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV), dev(sc["poses"]), dev(sc["intr"]), 1, 1)
    assert bare.face_id.tolist() == [[[-1]], [[-1]]]


def test_refusals_return_their_code_and_enqueue_nothing(RS):
    from ls2fm import _lib
    lib = _lib.load()
    sc = S.scenes()["ties"]
    v, f, p = dev(sc["verts"]), dev(sc["faces"]), dev(sc["poses"])
    k = dev(R.intr4(sc["intr"], 2))
    H, W, N = 48, 64, 2
    fid = torch.full((N, H, W), -5, dtype=torch.int32, device=DEV)
    dep = torch.full((N, H, W), -5.0, device=DEV)
    ws = torch.zeros(N * H * W, dtype=torch.int64, device=DEV)
    ptr, null = _lib.ptr, ctypes.c_void_p(0)
    INVALID, WORKSPACE = -1, -4
    assert lib.ls2fm_rasterize_workspace_bytes(N, H, W) == 8 * N * H * W and lib.ls2fm_rasterize_workspace_bytes(0, H, W) == 0

    def call(verts=ptr(v), n_verts=v.shape[0], faces=ptr(f), n_faces=f.shape[0], poses=ptr(p), intr=ptr(k), n_views=N, height=H, width=W,
             near=1e-3, face_id=ptr(fid), depth=ptr(dep), workspace=ptr(ws)):
        return lib.ls2fm_rasterize(verts, n_verts, faces, n_faces, poses, intr, n_views, height, width, near, face_id, depth, null, null,
                                   workspace, _lib.stream_ptr())

    for kw in (dict(verts=null), dict(faces=null), dict(poses=null), dict(intr=null), dict(face_id=null), dict(depth=null),
               dict(n_verts=-1), dict(n_faces=-1), dict(n_views=-1), dict(n_faces=1 << 31), dict(height=0), dict(width=0),
               dict(height=32769), dict(width=32769), dict(near=0.0), dict(near=-1.0), dict(near=float("inf")), dict(near=float("nan"))):
        assert call(**kw) == INVALID, kw
    assert call(workspace=null) == WORKSPACE
    assert call(workspace=ctypes.c_void_p(ws.data_ptr() + 4)) == INVALID
    for bad in ((-1, H, W), (N, 0, W), (N, H, 0), (N, 32769, W), (N, H, 32769), (1 << 20, 32768, 32768)):
        assert lib.ls2fm_rasterize_workspace_bytes(*bad) == INVALID, bad
    assert call(n_views=0) == 0 and call(n_views=0, poses=null, workspace=null) == 0          # returns at once
    se, ins = torch.full((v.shape[0],), -5, dtype=torch.int32, device=DEV), torch.full((v.shape[0],), -5, dtype=torch.int32, device=DEV)
    m = torch.ones(N, H, W, dtype=torch.uint8, device=DEV)

    def votes(verts=ptr(v), n_verts=v.shape[0], poses=ptr(p), intr=ptr(k), n_views=N, height=H, width=W, near=1e-3, masks=ptr(m),
              seen=ptr(se), inside=ptr(ins)):
        return lib.ls2fm_mesh_mask_votes(verts, n_verts, poses, intr, n_views, height, width, near, masks, seen, inside, _lib.stream_ptr())

    for kw in (dict(verts=null), dict(poses=null), dict(intr=null), dict(masks=null), dict(seen=null), dict(inside=null), dict(n_verts=-1),
               dict(n_views=-1), dict(height=0), dict(width=32769), dict(near=0.0), dict(near=float("nan"))):
        assert votes(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert bool((fid == -5).all()) and bool((dep == -5.0).all()) and bool((ws == 0).all())      # nothing was enqueued
    assert bool((se == -5).all()) and bool((ins == -5).all())
    assert call() == 0 and votes() == 0
    torch.cuda.synchronize()
    assert bool((fid >= -1).all()) and bool((se >= 0).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RS.rasterize(v.cpu(), f, p, dev(sc["intr"]), H, W)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RS.mask_votes(v, p.cpu(), dev(sc["intr"]), m)
    with pytest.raises(ValueError, match="near"):
        RS.rasterize(v, f, p, dev(sc["intr"]), H, W, near=0.0)
    with pytest.raises(ValueError, match="image size"):
        RS.rasterize(v, f, p, dev(sc["intr"]), 0, W)


def test_mask_votes_equal_the_restatement_and_the_torch_form(RS):
    vs = S.votes_scene()
    want = R.mask_votes(vs["verts"], vs["poses"], vs["intr"], vs["masks"], vs["near"])
    for masks in (dev(vs["masks"]), dev(vs["masks"] != 0)):                    # uint8 and bool
        seen, inside = RS.mask_votes(dev(vs["verts"]), dev(vs["poses"]), dev(vs["intr"]), masks, near=vs["near"])
        torch.cuda.synchronize()
        assert seen.dtype == torch.int32 and np.array_equal(seen.cpu().numpy(), want[0]) and np.array_equal(inside.cpu().numpy(), want[1])
    ts, ti = RS.mask_votes_torch(dev(vs["verts"]), dev(vs["poses"]), dev(vs["intr"]), dev(vs["masks"]), near=vs["near"])
    assert torch.equal(ts, seen) and torch.equal(ti, inside)
    none = RS.mask_votes(dev(vs["verts"]), torch.zeros(0, 3, 4, device=DEV), dev(vs["intr"]), torch.zeros(0, 47, 61, dtype=torch.uint8, device=DEV))
    assert int(none[0].abs().sum()) == 0 and int(none[1].abs().sum()) == 0


@pytest.fixture(scope="module")
def clean():
    cs = S.clean_scene()
    return cs, {k: dev(cs[k]) for k in ("verts", "faces", "poses", "intr", "masks")}


def test_clean_scene_masks_are_the_rasterisers_own_silhouette(RS, clean):
    cs, d = clean
    outer = RS.rasterize(d["verts"][:266], d["faces"][:S.CLEAN_OUTER_FACES], d["poses"], d["intr"], 48, 64)
    assert torch.equal((outer.face_id >= 0).to(torch.uint8), d["masks"])


@pytest.mark.parametrize("kw", [dict(), dict(dilate=2), dict(max_outside=1), dict(visibility=False), dict(masks=None), dict(min_seen=3, min_pixels=4)],
                         ids=["default", "dilate", "max_outside", "no_visibility", "no_masks", "min_seen_min_pixels"])
def test_clean_mesh_equals_the_restatements_selection(RS, clean, kw):
    cs, d = clean
    args = dict(masks=d["masks"], H=48, W=64)
    args.update(kw)
    rkw = {("dilate_px" if k == "dilate" else k): v for k, v in kw.items()}
    rargs = dict(masks=cs["masks"], H=48, W=64)
    rargs.update(rkw)
    keep, v, f = R.clean_mesh(cs["verts"], cs["faces"], cs["poses"], cs["intr"], **rargs)
    out, kept = RS.clean_mesh(d["verts"], d["faces"], d["poses"], d["intr"], **args)
    torch.cuda.synchronize()
    assert kept.dtype == torch.bool and np.array_equal(kept.cpu().numpy(), keep)
    assert out.faces.dtype == torch.int32 and np.array_equal(out.vertices.cpu().numpy(), v) and np.array_equal(out.faces.cpu().numpy(), f)
    if not kw:                                                     # the outer sphere's front-visible faces only
        assert 50 < int(kept.sum()) and not bool(kept[S.CLEAN_OUTER_FACES:].any())
        hits = RS.rasterize(d["verts"], d["faces"], d["poses"], d["intr"], 48, 64, hits=True).face_hits
        assert bool((hits[kept] >= 1).all())


def test_clean_mesh_keep_largest_drops_the_floater(RS, clean):
    from ls2fm import mesh
    cs, d = clean
    out, kept = RS.clean_mesh(d["verts"], d["faces"], d["poses"], d["intr"], H=48, W=64, keep_largest=True)
    loose, kept_loose = RS.clean_mesh(d["verts"], d["faces"], d["poses"], d["intr"], H=48, W=64)
    assert torch.equal(kept, kept_loose) and bool(kept[S.CLEAN_OUTER_FACES:S.CLEAN_OUTER_FACES + S.CLEAN_FLOATER_FACES].any())
    want = mesh.largest_component(loose.vertices, loose.faces)
    assert torch.equal(out.vertices, want.vertices) and torch.equal(out.faces, want.faces)
    assert 250 < out.faces.shape[0] <= int(kept[:S.CLEAN_OUTER_FACES].sum()) < loose.faces.shape[0]
    with pytest.raises(ValueError, match="image size"):
        RS.clean_mesh(d["verts"], d["faces"], d["poses"], d["intr"])
