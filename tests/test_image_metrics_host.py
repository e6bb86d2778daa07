"""CPU: the image-comparison restatement (tests/image_metrics_restate.py) against an independent scipy route, its exact
properties, the scenes (tests/image_metrics_scenes.py) hold the cases a wrong kernel fails, the CPU paths of
ls2fm.image_metrics against the restatement, and the C ABI's refusals (the library loads without a GPU; every refusal returns
before anything is enqueued)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import image_metrics_restate as R
import image_metrics_scenes as S
from conftest import ROOT
from ls2fm import _lib
from ls2fm import image_metrics as IM

T = IM.TILE
SCENES = S.scenes(T)
IDS = [s.name for s in SCENES]

SCIPY_BOUND, CONV_BOUND = S.SCIPY_BOUND, S.CONV_BOUND


def _torch_kw(sc, dev="cpu"):
    return dict(mask=None if sc.mask is None else torch.from_numpy(sc.mask).to(dev), data_range=sc.data_range, window=sc.taps,
                k1=sc.k1, k2=sc.k2, full=True)


def test_tile_and_limits_are_the_headers():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    assert int(re.search(r"#define\s+LS2FM_IMAGE_TILE\s+(\d+)", header).group(1)) == IM.TILE
    assert int(re.search(r"#define\s+LS2FM_IMAGE_MAX_TAPS\s+(\d+)", header).group(1)) == IM.MAX_TAPS == 33
    assert np.array_equal(IM.gaussian_window(), R.gaussian_taps()) and np.array_equal(IM.uniform_window(), R.uniform_taps())
    assert IM.gaussian_window().dtype == np.float64 and len(IM.gaussian_window()) == 11 and len(IM.uniform_window()) == 7
    assert abs(IM.gaussian_window().sum() - 1.0) < 1e-15


def test_restatement_agrees_with_the_scipy_route():
    """scipy.ndimage.gaussian_filter(sigma 1.5, truncate 3.5) has radius 5 = the 11-tap window; cropped to the valid region its
    zero padding never enters.  Its own order of summation differs: agreement to rounding."""
    ndi = pytest.importorskip("scipy.ndimage")
    worst, used = 0.0, 0
    for sc in SCENES:
        if len(sc.taps) != 11 or not sc.finite:
            continue
        x, y = sc.a.astype(np.float64), sc.b.astype(np.float64)

        def f(v):
            return ndi.gaussian_filter(v, sigma=(0, 1.5, 1.5, 0), truncate=3.5, mode="constant")[:, 5:v.shape[1] - 5, 5:v.shape[2] - 5]

        mx, my, xx, yy, xy = f(x), f(y), f(x * x), f(y * y), f(x * y)
        vx, vy, cxy = xx - mx * mx, yy - my * my, xy - mx * my
        s = ((2 * mx * my + sc.c1) * (2 * cxy + sc.c2)) / ((mx * mx + my * my + sc.c1) * (vx + vy + sc.c2))
        gap = float(np.abs(s - S.reference(sc, T)["ssim_map"]).max())
        print(f"{sc.name}: |restatement - scipy| = {gap:.3e}")
        worst, used = max(worst, gap), used + 1
    assert used >= 8
    assert worst <= SCIPY_BOUND, worst


def test_identical_images_give_exactly_one_and_swapping_changes_no_bit():
    for sc in SCENES:
        same = R.compare(sc.a, sc.a, sc.taps, sc.c1, sc.c2, mask=sc.mask, T=T)
        fin = np.isfinite(same["ssim_map"])
        assert (same["ssim_map"][fin] == 1.0).all() and fin.any(), sc.name
        if sc.finite:
            assert fin.all() and (same["sse"] == 0.0).all() and np.array_equal(same["ssim_sum"], same["ssim_count"].astype(np.float64))
        fwd, rev = S.reference(sc, T), R.compare(sc.b, sc.a, sc.taps, sc.c1, sc.c2, mask=sc.mask, T=T)
        for k in ("sse", "ssim_sum", "ssim_map"):
            assert np.array_equal(fwd[k].view(np.uint64), rev[k].view(np.uint64)) or not sc.finite, (sc.name, k)
            assert np.array_equal(fwd[k], rev[k], equal_nan=True), (sc.name, k)


def test_scenes_hold_the_cases_a_wrong_kernel_fails():
    # moments kept in fp32 lose the variance on the ramp: such a kernel is off by far more than any tolerance here
    a, b = S.ramp()
    g = R.gaussian_taps()
    m64, m32 = R.ssim_map(a, b, g, 1e-4, 9e-4), R.ssim_map(a, b, g, 1e-4, 9e-4, dtype=np.float32)
    assert np.abs(m64 - m32.astype(np.float64)).max() > 1e-5
    assert any(sc.name.startswith("ramp") and np.array_equal(sc.a, a) for sc in SCENES)
    # every size class, for the tile the library reports
    present = set()
    for sc in SCENES:
        present |= S.size_class(sc.a.shape[1], sc.a.shape[2], len(sc.taps), T)
    assert present == S.SIZE_CLASSES, S.SIZE_CLASSES - present
    assert {sc.a.shape[3] for sc in SCENES} >= {1, 3, 4}
    assert {len(sc.taps) for sc in SCENES} >= {1, 7, 11, 33}
    assert any(sc.data_range == 255.0 and np.array_equal(sc.a, np.rint(sc.a)) for sc in SCENES)
    assert any(not sc.finite and sc.a.shape[0] == 3 for sc in SCENES)
    assert any(sc.mask is not None and sc.a.shape[0] == 3 and not sc.mask[1].any() and sc.mask[0].any() for sc in SCENES)
    # a mask edge on a tile boundary: on up to column T - 1, off from column T
    assert any(sc.mask is not None and sc.mask[0, 0, T - 1] and not sc.mask[0, 0, T] for sc in SCENES)
    # constants: zero variance, the map is the luminance term alone
    sc = next(s for s in SCENES if s.name.startswith("constants"))
    want = (2 * 0.25 * 0.75 + sc.c1) / (0.25 ** 2 + 0.75 ** 2 + sc.c1)
    assert np.abs(S.reference(sc, T)["ssim_map"] - want).max() < 1e-12
    # the stated order is a different order: it agrees with np.sum within the bound and, somewhere, not by its bits
    differs = False
    for sc in SCENES:
        o, p = S.reference(sc, T), S.reference(sc, T, ordered=False)
        assert np.array_equal(o["count"], p["count"]) and np.array_equal(o["ssim_count"], p["ssim_count"])
        if sc.finite:
            assert (np.abs(o["sse"] - p["sse"]) <= R.sum_bound(o["count"], o["sse_abs"])).all(), sc.name
            assert (np.abs(o["ssim_sum"] - p["ssim_sum"]) <= R.sum_bound(o["ssim_count"], o["ssim_abs"])).all(), sc.name
            differs |= not np.array_equal(o["ssim_sum"], p["ssim_sum"]) or not np.array_equal(o["sse"], p["sse"])
    assert differs


@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_cpu_path_agrees_with_the_restatement(sc):
    ref = S.reference(sc, T)
    got = IM.compare_images(torch.from_numpy(sc.a), torch.from_numpy(sc.b), **_torch_kw(sc))
    assert got.ssim_map.dtype == torch.float64 and got.sse.dtype == torch.float64 and got.count.dtype == torch.int64
    assert np.array_equal(got.ssim_map.numpy(), ref["ssim_map"], equal_nan=True)               # 4 x the measured gap of 0
    assert np.array_equal(got.count.numpy(), ref["count"]) and np.array_equal(got.ssim_count.numpy(), ref["ssim_count"])
    for view in range(sc.a.shape[0]):
        if not (np.isfinite(sc.a[view]).all() and np.isfinite(sc.b[view]).all()):
            assert np.isnan(got.ssim_sum[view].item())
            continue
        assert abs(got.sse[view].item() - ref["sse"][view]) <= R.sum_bound(ref["count"], ref["sse_abs"])[view]
        assert abs(got.ssim_sum[view].item() - ref["ssim_sum"][view]) <= R.sum_bound(ref["ssim_count"], ref["ssim_abs"])[view]
    conv = IM._compare_torch(torch.from_numpy(sc.a), torch.from_numpy(sc.b), **_torch_kw(sc))
    fin = np.isfinite(ref["ssim_map"])
    gap = float(np.abs(conv.ssim_map.numpy() - ref["ssim_map"])[fin].max())
    print(f"{sc.name}: |conv2d form - restatement| = {gap:.3e}")
    assert gap <= CONV_BOUND and np.array_equal(np.isfinite(conv.ssim_map.numpy()), fin)


def test_scores_shapes_and_the_table_row():
    sc = next(s for s in SCENES if s.name.startswith("three_views_empty"))
    a, b, m = torch.from_numpy(sc.a), torch.from_numpy(sc.b), torch.from_numpy(sc.mask)
    N, H, W, C = a.shape
    got = IM.compare_images(a, b, mask=m)
    flat = IM.compare_images(a.reshape(N, H * W, C), b.reshape(N, H * W, C), mask=m.reshape(N, H * W), H=H, W=W)
    assert torch.equal(got.sse, flat.sse) and torch.equal(got.ssim_sum, flat.ssim_sum)
    assert got.count[1] == 0 and got.ssim_count[1] == 0 and torch.isnan(got.psnr[1]) and torch.isnan(got.ssim[1])
    p, s = got.mean()
    assert torch.allclose(p, (got.psnr[0] + got.psnr[2]) / 2) and torch.allclose(s, (got.ssim[0] + got.ssim[2]) / 2)
    def same_bits(u, v):
        return np.array_equal(u.numpy(), v.numpy(), equal_nan=True)

    assert same_bits(got.psnr, 10.0 * torch.log10(1.0 / got.mse)) and same_bits(IM.psnr(a, b, mask=m), got.psnr)
    assert same_bits(IM.ssim(a, b, mask=m), got.ssim)
    one = IM.compare_images(a[0], b[0], mask=m[0])                                         # [H, W, C]
    assert torch.equal(one.sse, got.sse[:1])
    grey = IM.compare_images(a[..., 0], b[..., 0])                                         # [N, H, W]
    assert grey.count.tolist() == [H * W] * 3
    u8 = IM.compare_images((a * 255).round().to(torch.uint8), (b * 255).round().to(torch.uint8))
    assert u8.data_range == 255.0
    same = IM.compare_images(a, a)
    assert (same.ssim == 1.0).all() and torch.isinf(same.psnr).all() and (same.psnr > 0).all()
    for bad in (dict(window=np.ones(4) / 4), dict(window=np.ones(35) / 35), dict(window=np.ones(61) / 61), dict(k1=float("nan"))):
        with pytest.raises(ValueError):
            IM.compare_images(a, b, **bad)
    with pytest.raises(ValueError):
        IM.compare_images(a, b[:, :-1])


def test_c_abi_refusals_come_before_anything_is_enqueued():
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -4                                                            # LS2FM_ERR_INVALID_ARGUMENT, LS2FM_ERR_WORKSPACE
    assert lib.ls2fm_image_compare_workspace_bytes(0, 0, 0, 0, 0) == INVALID              # the size query refuses the same way
    fake = ctypes.c_void_p(1 << 20)                                                        # never dereferenced by a refused call
    null = ctypes.c_void_p(0)
    taps = R.gaussian_taps()
    base = dict(a=fake, b=fake, mask=null, n=2, h=40, w=52, c=3, taps=taps, c1=1e-4, c2=9e-4, sse=fake, count=fake, ssum=fake,
                scount=fake, smap=null, ws=fake, ws_bytes=None)

    def call(**kw):
        k = dict(base, **kw)
        t = k["taps"]
        tp = t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if t is not None else ctypes.POINTER(ctypes.c_double)()
        n_taps = k.get("n_taps", len(t) if t is not None else 11)
        need = lib.ls2fm_image_compare_workspace_bytes(k["n"], k["h"], k["w"], k["c"], n_taps)
        ws_bytes = k["ws_bytes"] if k["ws_bytes"] is not None else max(need, 0)
        return lib.ls2fm_image_compare(k["a"], k["b"], k["mask"], k["n"], k["h"], k["w"], k["c"], tp, n_taps, k["c1"], k["c2"], k["sse"],
                                       k["count"], k["ssum"], k["scount"], k["smap"], k["ws"], ws_bytes, null)

    for name in ("a", "b", "sse", "count", "ssum", "scount"):
        assert call(**{name: null}) == INVALID, name
    assert call(taps=None) == INVALID
    for kw in (dict(n=0), dict(c=0), dict(c=5), dict(n_taps=10), dict(n_taps=0), dict(n_taps=35, taps=np.ones(35) / 35),
               dict(h=10), dict(w=10), dict(c1=-1.0), dict(c2=float("nan")), dict(c1=float("inf")), dict(h=32768, w=32768, c=2)):
        assert call(**kw) == INVALID, kw
    assert lib.ls2fm_image_compare_workspace_bytes(1, 32768, 32768, 2, 11) == INVALID
    assert lib.ls2fm_image_compare_workspace_bytes(1, 40, 52, 3, 12) == INVALID
    assert lib.ls2fm_image_compare_workspace_bytes(1, 10, 52, 3, 11) == INVALID
    need = lib.ls2fm_image_compare_workspace_bytes(2, 40, 52, 3, 11)
    assert need >= 2 * 3 * 4 * (2 * 8 + 2 * 8)                                             # a row and two counts per view and tile
    assert call(ws=null) == WORKSPACE and call(ws_bytes=need - 1) == WORKSPACE
