"""GPU: ls2fm_mesh_vertex_colors / _finish (csrc/mesh_colors.hip) through ls2fm.mesh_colors, by their bits against the numpy
restatement (tests/mesh_colors_restate.py): counts, every entry of the sums and every colour.  The rule itself is judged on the
restatement (tests/test_mesh_colors_host.py)."""
import numpy as np
import pytest
import torch

import mesh_colors_restate as MR
import mesh_colors_scenes as S
from ls2fm import _posed, mesh_colors

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def bits(a):
    a = host(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, ref, what):
    """bit for bit; a NaN matches a NaN (its sign and payload are the one thing IEEE 754 leaves to the implementation: the
    x86 host and the device propagate different ones from the same NaN pixel)"""
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, f"{what}: shape {g.shape} != {r.shape}"
    bad = g != r
    if host(ref).dtype.kind == "f":
        bad &= ~(np.isnan(host(got)) & np.isnan(host(ref)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ, the first at {tuple(np.argwhere(bad)[0])}"


def device_state(sc, V, views, with_normals, power, with_masks=True, state=None):
    """accumulate the views `views` of an edge scene's first V points on the device -> (sums, count)"""
    pts = dev(sc["points"][:V])
    pose4 = _posed.views(dev(sc["poses"][views]), dev(sc["intr"][views]), "test")
    img = dev(sc["images"][views])
    C = img.shape[3]
    if state is None:
        state = (torch.zeros(V, C + 1, dtype=torch.float64, device=DEV), torch.zeros(V, dtype=torch.int32, device=DEV))
    mesh_colors.accumulate_views(state, pts, pose4, img, dev(sc["depth"][views]), dev(sc["masks"][views]) if with_masks else None,
                                 dev(sc["normals"][:V]) if with_normals else None, sc["near"], sc["depth_tol"], power)
    return state


def restated(sc, V, views, with_normals, power, with_masks=True, **kw):
    return MR.vertex_colors(sc["points"][:V], sc["poses"][views], sc["intr"][views], sc["images"][views], sc["depth"][views],
                            masks=sc["masks"][views] if with_masks else None, normals=sc["normals"][:V] if with_normals else None,
                            near=sc["near"], depth_tol=sc["depth_tol"], power=power, **kw)


# H, W, C, V, N, normals, power: V = 0, 1, 63, 64, 65 and one past the workgroup's 256; N = 0, 1, 3; 5 x 7 to 33 x 17
CASES = [(5, 7, 1, 0, 3, True, 1), (5, 7, 1, 1, 1, False, 0), (5, 7, 3, 63, 3, True, 8), (17, 33, 3, 64, 3, True, 1),
         (17, 33, 4, 65, 1, True, 0), (33, 17, 4, 257, 3, True, 8), (33, 17, 1, 257, 3, False, 1), (17, 33, 3, 257, 0, True, 1),
         (5, 7, 4, 257, 3, True, 1), (17, 33, 3, 257, 3, True, 1)]


@pytest.mark.parametrize("H,W,C,V,N,with_normals,power", CASES)
def test_bits_of_the_restatement(H, W, C, V, N, with_normals, power):
    sc = S.edge_scene(H, W, C)
    views = slice(0, N)
    fallback = np.random.default_rng(V + N).uniform(0, 1, (V, C)).astype(np.float32) if V % 2 else None
    ref = restated(sc, V, views, with_normals, power, fill=(0.25, 0.5, 0.75), fallback=fallback)
    state = device_state(sc, V, views, with_normals, power)
    colors = mesh_colors.finish_colors(state, C, fill=(0.25, 0.5, 0.75), fallback=dev(fallback))
    torch.cuda.synchronize()
    same(state[1], ref["count"], "count")
    same(state[0], ref["sums"], "sums")
    same(colors, ref["colors"], "colors")
    if V == 257 and N == 3:
        assert (ref["count"] == 0).any() and (ref["count"] == 3).any() and np.isnan(ref["sums"]).any(), "the scene's cases are live"


def test_without_masks_and_split_over_views():
    sc = S.edge_scene(17, 33, 3)
    V = 257
    whole = restated(sc, V, slice(0, 3), True, 2, with_masks=False)
    one = device_state(sc, V, slice(0, 3), True, 2, with_masks=False)
    same(one[0], whole["sums"], "sums, one call")
    same(one[1], whole["count"], "count, one call")
    split = device_state(sc, V, slice(0, 2), True, 2, with_masks=False)
    split = device_state(sc, V, slice(2, 3), True, 2, with_masks=False, state=split)
    same(split[0], one[0], "sums, views 0..1 then 2")
    same(split[1], one[1], "count, views 0..1 then 2")


def test_photo_colors_rasterises_chunks_reruns_and_replays():
    """the public call on the sphere scene: its own rasterisation (two chunks of views), the state carried across them, the
    finish; a rerun and a captured replay give the eager bits"""
    sc = S.sphere_scene()
    ref = MR.vertex_colors(sc["verts"], sc["poses"], sc["intr"], sc["images"], sc["depth"], normals=sc["normals"], near=sc["near"],
                           depth_tol=sc["depth_tol"], power=2, fill=0.5)
    args = [dev(sc[k]) for k in ("verts", "faces", "poses", "intr", "images")]
    nrm = dev(sc["normals"])
    call = lambda chunk: mesh_colors.photo_colors(*args, normals=nrm, near=sc["near"], depth_tol=sc["depth_tol"], power=2, fill=0.5,
                                                  view_chunk=chunk)
    eager = call(4)
    same(eager.count, ref["count"], "count")
    same(eager.weight, ref["sums"][:, 3], "weight")
    same(eager.colors, ref["colors"], "colors")
    again, whole = call(4), call(None)
    for a in (again, whole):
        assert torch.equal(a.count, eager.count) and torch.equal(bits_t(a.colors), bits_t(eager.colors)) and torch.equal(a.weight, eager.weight)
    given = mesh_colors.photo_colors(*args, normals=nrm, near=sc["near"], depth_tol=sc["depth_tol"], power=2, fill=0.5, depth=dev(sc["depth"]))
    assert torch.equal(given.count, eager.count) and torch.equal(bits_t(given.colors), bits_t(eager.colors))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(4)                                                    # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(4)
    for _ in range(2):
        out.colors.fill_(-1.0)
        out.count.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.count, eager.count) and torch.equal(bits_t(out.colors), bits_t(eager.colors))
        assert torch.equal(out.weight, eager.weight)


def bits_t(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def test_kernel_against_the_torch_form_on_the_device():
    sc = S.edge_scene(33, 17, 4)
    V = 257
    state = device_state(sc, V, slice(0, 3), True, 3)
    got = mesh_colors.finish_colors(state, 4, fill=0.5)
    ref = mesh_colors.photo_colors_torch(dev(sc["points"][:V]), dev(sc["poses"]), dev(sc["intr"]), dev(sc["images"]), dev(sc["depth"]),
                                         masks=dev(sc["masks"]), normals=dev(sc["normals"][:V]), near=sc["near"], depth_tol=sc["depth_tol"],
                                         power=3, fill=0.5)
    assert torch.equal(state[1], ref.count)
    ok = torch.isclose(got, ref.colors, rtol=1e-6, atol=1e-7, equal_nan=True)
    assert bool(ok.all())


def test_refusals_and_empty_calls():
    from ls2fm import _lib
    lib = _lib.load()
    sc = S.edge_scene(5, 7, 3)
    V = 8
    pts, img, depth = dev(sc["points"][:V]), dev(sc["images"]), dev(sc["depth"])
    poses, k4 = _posed.views(dev(sc["poses"]), dev(sc["intr"]), "test")
    sums = torch.zeros(V, 4, dtype=torch.float64, device=DEV)
    count = torch.zeros(V, dtype=torch.int32, device=DEV)
    p, s = _lib.ptr, _lib.stream_ptr()

    def call(verts=pts, n_verts=V, n_views=3, H=5, W=7, C=3, images=img, d=depth, near=0.5, tol=0.25, power=1, sm=sums, ct=count):
        return lib.ls2fm_mesh_vertex_colors(p(verts), p(None), n_verts, p(poses), p(k4), n_views, H, W, C, p(images), p(d), p(None), near,
                                            tol, power, p(sm), p(ct), s)
    assert call() == 0
    for kw in (dict(verts=None), dict(images=None), dict(d=None), dict(sm=None), dict(ct=None), dict(n_verts=-1), dict(n_views=-1),
               dict(H=0), dict(W=32769), dict(C=0), dict(C=5), dict(power=-1), dict(power=9), dict(tol=-1e-3), dict(tol=float("inf")),
               dict(tol=float("nan")), dict(near=0.0), dict(near=float("nan"))):
        assert call(**kw) == -1, kw
    assert call(n_verts=0, verts=None, sm=None, ct=None) == 0 and call(n_views=0, images=None, d=None) == 0
    color = torch.empty(V, 3, device=DEV)
    fill = (3 * _lib.c_float)(0.1, 0.2, 0.3)
    fin = lambda sm=sums, ct=count, n=V, C=3, fb=None, fl=fill, out=color: lib.ls2fm_mesh_vertex_colors_finish(p(sm), p(ct), n, C, p(fb), fl, p(out), s)
    assert fin() == 0
    for kw in (dict(sm=None), dict(ct=None), dict(out=None), dict(n=-1), dict(C=0), dict(C=5), dict(fl=None)):
        assert fin(**kw) == -1, kw
    assert fin(n=0, sm=None, ct=None, out=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        mesh_colors.photo_colors(pts, dev(sc["faces"]), dev(sc["poses"]), dev(sc["intr"]), img[..., :0])
