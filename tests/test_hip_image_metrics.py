"""GPU: ls2fm.image_metrics (ls2fm_image_compare, csrc/image_metrics.hip) against the numpy restatement
(tests/image_metrics_restate.py) on the scenes of tests/image_metrics_scenes.py.
  map     every window of every scene equals the restatement by its bits
  counts  exact
  sums    sse and ssim_sum equal the stated tile-and-lane order bit for bit, and numpy's own order within
          (count + 16) 2^-53 sum |term|
and: views are isolated, the map is optional, reruns and graph replays repeat the bits, the exact properties, the derived
scores, the refusals (nothing enqueued, outputs untouched), the conv2d form, and ls2fm.image.evaluate_views."""
import ctypes
import math

import numpy as np
import pytest
import torch

import image_metrics_restate as R
import image_metrics_scenes as S
from ls2fm import _lib, image
from ls2fm import image_metrics as IM

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = IM.TILE
SCENES = S.scenes(T)
IDS = [s.name for s in SCENES]
_REF = {}


def ref_of(sc):
    """the restatement of a scene in both orders, computed once and never changed"""
    if sc.name not in _REF:
        _REF[sc.name] = (S.reference(sc, T), S.reference(sc, T, ordered=False))
    return _REF[sc.name]


def scene(name):
    return next(s for s in SCENES if s.name.startswith(name))


def run(sc, full=True, views=slice(None), a=None, b=None):
    a = sc.a if a is None else a
    b = sc.b if b is None else b
    mask = None if sc.mask is None else torch.from_numpy(sc.mask[views]).to(DEV)
    return IM.compare_images(torch.from_numpy(a[views]).to(DEV), torch.from_numpy(b[views]).to(DEV), mask=mask, data_range=sc.data_range,
                             window=sc.taps, k1=sc.k1, k2=sc.k2, full=full)


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return t.view(np.uint64) if t.dtype == np.float64 else t


def same_numbers(x, y):
    """the four per-view numbers of two ImageScores agree bit for bit (NaN payloads aside)"""
    for k in ("sse", "ssim_sum", "count", "ssim_count"):
        u, v = getattr(x, k).cpu().numpy(), getattr(y, k).cpu().numpy()
        assert np.array_equal(u, v, equal_nan=True) and np.array_equal(np.signbit(u.astype(np.float64)), np.signbit(v.astype(np.float64))), k


@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_every_pixel_of_every_scene(sc):
    ordered, plain = ref_of(sc)
    got = run(sc)
    smap = got.ssim_map.cpu().numpy()
    assert smap.shape == ordered["ssim_map"].shape and smap.dtype == np.float64
    fin = np.isfinite(ordered["ssim_map"])
    assert np.array_equal(np.isnan(smap), np.isnan(ordered["ssim_map"]))
    assert np.array_equal(bits(smap)[fin], bits(ordered["ssim_map"])[fin])
    assert np.array_equal(got.count.cpu().numpy(), ordered["count"]) and np.array_equal(got.ssim_count.cpu().numpy(), ordered["ssim_count"])
    for key, n_key, abs_key in (("sse", "count", "sse_abs"), ("ssim_sum", "ssim_count", "ssim_abs")):
        dev = getattr(got, key).cpu().numpy()
        print(f"{sc.name} {key}: device {dev}, stated order {ordered[key]}, numpy {plain[key]}")
        assert np.array_equal(np.isnan(dev), np.isnan(ordered[key]))
        ok = ~np.isnan(dev)
        assert np.array_equal(bits(dev)[ok], bits(ordered[key])[ok]), key
        ok &= np.isfinite(plain[key])
        assert (np.abs(dev - plain[key])[ok] <= R.sum_bound(ordered[n_key], ordered[abs_key])[ok]).all(), key


@pytest.mark.parametrize("name", ["three_views_nonfinite", "three_views_empty_mask"])
def test_views_are_isolated(name):
    sc = scene(name)
    batch = run(sc)
    for v in range(3):
        one = run(sc, views=slice(v, v + 1))
        for k in ("sse", "ssim_sum", "count", "ssim_count", "ssim_map"):
            u, w = getattr(batch, k)[v].cpu().numpy(), getattr(one, k)[0].cpu().numpy()
            assert np.array_equal(u, w, equal_nan=True), (k, v)
    # view 1 replaced by finite content: no bit of its neighbours changes
    a, b = sc.a.copy(), sc.b.copy()
    a[1], b[1] = sc.a[0], sc.b[2]
    clean = run(sc, a=a, b=b)
    for k in ("sse", "ssim_sum", "count", "ssim_count", "ssim_map"):
        for v in (0, 2):
            assert torch.equal(getattr(batch, k)[v], getattr(clean, k)[v]), (k, v)
    if name == "three_views_nonfinite":
        assert torch.isnan(batch.ssim_sum[1]) and not torch.isfinite(batch.sse[1]) and torch.isfinite(batch.ssim_sum[[0, 2]]).all()
        assert torch.isfinite(clean.ssim_sum).all() and torch.isfinite(clean.sse).all()


@pytest.mark.parametrize("name", ["short_of_two_tiles", "wide_c3", "three_views_nonfinite"])
def test_the_map_is_optional_and_a_rerun_repeats_the_bits(name):
    sc = scene(name)
    with_map, without = run(sc, full=True), run(sc, full=False)
    assert without.ssim_map is None
    same_numbers(with_map, without)
    again = run(sc, full=True)
    same_numbers(with_map, again)
    assert np.array_equal(with_map.ssim_map.cpu().numpy(), again.ssim_map.cpu().numpy(), equal_nan=True)


def test_graph_replay_after_the_inputs_are_overwritten_in_place():
    first, second = scene("noisy_c3_uniform_random_mask"), scene("range_255_c3")          # both 40 x 52 x 3
    assert first.a.shape == second.a.shape
    a, b = torch.from_numpy(first.a).to(DEV), torch.from_numpy(first.b).to(DEV)
    mask = torch.from_numpy(first.mask).to(DEV)
    kw = dict(window=second.taps, data_range=second.data_range, full=True)
    IM.compare_images(a, b, mask=mask, **kw)                                             # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            cap = IM.compare_images(a, b, mask=mask, **kw)
    torch.cuda.current_stream().wait_stream(s)
    a.copy_(torch.from_numpy(second.a))
    b.copy_(torch.from_numpy(second.b))
    mask.fill_(1)
    g.replay()
    torch.cuda.synchronize()
    eager = IM.compare_images(torch.from_numpy(second.a).to(DEV), torch.from_numpy(second.b).to(DEV), **kw)
    same_numbers(cap, eager)
    for k in ("ssim_map", "mse", "psnr", "ssim"):
        assert torch.equal(getattr(cap, k), getattr(eager, k)), k
    ordered, _ = ref_of(second)
    assert np.array_equal(bits(cap.ssim_map), bits(ordered["ssim_map"])) and np.array_equal(bits(cap.ssim_sum), bits(ordered["ssim_sum"]))


def test_identical_images_and_an_empty_mask():
    for sc in (scene("identical_c3"), scene("wide_c1"), scene("range_255_c3")):
        got = run(sc, b=sc.a)
        assert (got.ssim_map == 1.0).all() and (got.sse == 0.0).all()
        assert torch.equal(got.ssim_sum, got.ssim_count.double()) and (got.ssim == 1.0).all()
        assert torch.isinf(got.psnr).all() and (got.psnr > 0).all()
    sc = scene("three_views_empty_mask")
    got = run(sc)
    assert got.count[1] == 0 and got.ssim_count[1] == 0 and got.sse[1] == 0.0 and got.ssim_sum[1] == 0.0
    assert not torch.signbit(got.sse[1]) and not torch.signbit(got.ssim_sum[1])
    for k in ("mse", "psnr", "ssim"):
        v = getattr(got, k)
        assert torch.isnan(v[1]) and torch.isfinite(v[[0, 2]]).all(), k
    p, s = got.mean()
    assert torch.equal(p, (got.psnr[0] + got.psnr[2]) / 2.0) and torch.equal(s, (got.ssim[0] + got.ssim[2]) / 2.0)


@pytest.mark.parametrize("name", ["noisy_c3_uniform", "range_255_c3", "ramp_c1", "three_views_empty_mask"])
def test_derived_scores(name):
    """mse, psnr and ssim are torch expressions of the four numbers; psnr against numpy's 10 log10 within 4 ulp of the result
    plus (10 / ln 10) x the relative bound on sse (a derived bound: |d psnr| = (10 / ln 10) |d sse| / sse)."""
    sc = scene(name)
    ordered, plain = ref_of(sc)
    got = run(sc)
    sse, count = torch.from_numpy(ordered["sse"]).to(DEV), torch.from_numpy(ordered["count"]).to(DEV)
    ssum, scount = torch.from_numpy(ordered["ssim_sum"]).to(DEV), torch.from_numpy(ordered["ssim_count"]).to(DEV)
    mse = sse / count.double()
    want = dict(mse=mse, psnr=10.0 * torch.log10(sc.data_range ** 2 / mse), ssim=ssum / scount.double())
    for k, v in want.items():
        assert np.array_equal(getattr(got, k).cpu().numpy(), v.cpu().numpy(), equal_nan=True), k
    has = ordered["count"] > 0
    with np.errstate(all="ignore"):
        ref = 10.0 * np.log10(sc.data_range ** 2 / (plain["sse"] / ordered["count"]))
        rel = R.sum_bound(ordered["count"], ordered["sse_abs"]) / plain["sse"]
    err = np.abs(got.psnr.cpu().numpy() - ref)[has]
    bound = (4 * np.spacing(np.abs(ref)) + (10.0 / math.log(10.0)) * rel)[has]
    print(f"{name}: psnr {got.psnr.cpu().numpy()}, numpy {ref}, |difference| {err}, bound {bound}")
    assert (err <= bound).all()


def test_refusals_enqueue_nothing_and_leave_the_outputs_untouched():
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -4
    sc = scene("noisy_c3_uniform")
    N, H, W, C = sc.a.shape
    n = 11
    a, b = torch.from_numpy(sc.a).to(DEV), torch.from_numpy(sc.b).to(DEV)
    taps = R.gaussian_taps()
    sums = torch.full((2, N), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((2, N), -7, dtype=torch.int64, device=DEV)
    smap = torch.full((N, H - n + 1, W - n + 1, C), -7.0, dtype=torch.float64, device=DEV)
    need = lib.ls2fm_image_compare_workspace_bytes(N, H, W, C, n)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    base = dict(a=a, b=b, n=N, h=H, w=W, c=C, taps=taps, n_taps=n, c1=1e-4, c2=9e-4, sse=sums[0], count=counts[0], ssum=sums[1],
                scount=counts[1], ws=ws, ws_bytes=need)

    def call(**kw):
        k = dict(base, **kw)
        tp = k["taps"].ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if k["taps"] is not None else ctypes.POINTER(ctypes.c_double)()
        return lib.ls2fm_image_compare(_lib.ptr(k["a"]), _lib.ptr(k["b"]), _lib.ptr(None), k["n"], k["h"], k["w"], k["c"], tp, k["n_taps"],
                                       k["c1"], k["c2"], _lib.ptr(k["sse"]), _lib.ptr(k["count"]), _lib.ptr(k["ssum"]), _lib.ptr(k["scount"]),
                                       _lib.ptr(smap), _lib.ptr(k["ws"]), k["ws_bytes"], _lib.stream_ptr())

    for name in ("a", "b", "sse", "count", "ssum", "scount"):
        assert call(**{name: None}) == INVALID, name
    assert call(taps=None) == INVALID
    for kw in (dict(n=0), dict(c=0), dict(c=5), dict(n_taps=10), dict(n_taps=0), dict(n_taps=35), dict(h=10), dict(w=10), dict(c1=-1.0),
               dict(c2=float("nan")), dict(c1=float("inf")), dict(h=32768, w=32768, c=2)):
        assert call(**kw) == INVALID, kw
    assert call(ws=None) == WORKSPACE and call(ws_bytes=need - 1) == WORKSPACE
    assert lib.ls2fm_image_compare_workspace_bytes(N, H, W, C, 12) == INVALID and lib.ls2fm_image_compare_workspace_bytes(0, H, W, C, n) == INVALID
    torch.cuda.synchronize()
    assert (sums == -7.0).all() and (counts == -7).all() and (smap == -7.0).all() and (ws == 0).all()
    assert call() == 0                                                              # the same arguments, unrefused, do write
    torch.cuda.synchronize()
    assert (sums != -7.0).all() and (counts == H * W * C).logical_or(counts == (H - n + 1) * (W - n + 1) * C).all() and (smap != -7.0).all()
    # the python wrapper refuses in words
    with pytest.raises(ValueError):
        IM.compare_images(a, b, window=np.ones(4) / 4)
    with pytest.raises(ValueError):
        IM.compare_images(a[:, :5], b[:, :5])


@pytest.mark.parametrize("name", ["noisy_c3_uniform", "ramp_c1", "range_255_c3", "past_tile_x_c4", "wide_c1"])
def test_conv2d_form_agrees_with_the_kernel(name):
    sc = scene(name)
    got = run(sc)
    mask = None if sc.mask is None else torch.from_numpy(sc.mask).to(DEV)
    conv = IM._compare_torch(torch.from_numpy(sc.a).to(DEV), torch.from_numpy(sc.b).to(DEV), mask=mask, data_range=sc.data_range,
                             window=sc.taps, k1=sc.k1, k2=sc.k2, full=True)
    gap = float((conv.ssim_map - got.ssim_map).abs().max())
    print(f"{name}: |conv2d form - kernel| = {gap:.3e} (bound {S.CONV_BOUND:.3e})")
    assert gap <= S.CONV_BOUND
    assert torch.equal(conv.count, got.count) and torch.equal(conv.ssim_count, got.ssim_count)
    ordered, _ = ref_of(sc)
    assert (np.abs(conv.sse.cpu().numpy() - ordered["sse"]) <= R.sum_bound(ordered["count"], ordered["sse_abs"])).all()


def test_evaluate_views_equals_render_then_compare():
    from test_hip_render_image import _scene, _view
    opt, sdf, rad, ren = _scene("ETH3D", True, 32, levels=8, log2=14)
    H, W = 24, 32
    poses, intr = _view(opt, H, W, V=2)
    gen = torch.Generator().manual_seed(11)
    images = torch.rand(2, H, W, 3, generator=gen).to(DEV)
    masks = (torch.rand(2, H, W, generator=gen) < 0.8).to(DEV)
    scores, render = image.evaluate_views(ren, opt, sdf, rad, poses, intr, images, masks=masks, H=H, W=W, return_render=True, full=True)
    rgb = image.render_image(ren, opt, sdf, rad, poses, intr, H=H, W=W).rgb
    assert torch.equal(render.rgb, rgb)
    want = IM.compare_images(rgb, images.reshape(2, H * W, 3), mask=masks, H=H, W=W, full=True)
    same_numbers(scores, want)
    for k in ("ssim_map", "mse", "psnr", "ssim"):
        assert torch.equal(getattr(scores, k), getattr(want, k)), k
    assert scores.ssim_map.shape == (2, H - 10, W - 10, 3) and torch.isfinite(scores.psnr).all()
    alone = image.evaluate_views(ren, opt, sdf, rad, poses, intr, images, H=H, W=W)
    assert alone.ssim_map is None and (alone.count == H * W * 3).all()
