"""SIFT extraction, host side (no GPU): the C ABI's symbols and refusals, the numpy restatement (tests/sift_restate.py) on cases
with known answers, the input conditions the GPU tests rest on (float32 and float64 restatement agree on which keypoints exist;
scene C carries enough true matches), and the restatement's own float32-vs-float64 gaps, which are the GPU tests' yardstick."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_restate as MR  # noqa: E402
import sift_restate as R  # noqa: E402
import sift_scenes as SC  # noqa: E402

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


@functools.lru_cache(maxsize=None)
def _both(name):
    img = {"A": SC.scene_a, "B": SC.scene_b}[name]()
    return R.extract(img, np.float32), R.extract(img, np.float64)


def _opts(**kw):
    from ls2fm.features import SiftOptions
    return SiftOptions(**kw).c_struct()


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_workspace_query():
    from ls2fm import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ls2fm.h")).read()
    for name in ("ls2fm_sift_workspace_bytes", "ls2fm_sift_extract"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name + "(" in header
    o = _opts()
    h, ch = _i32([1200])
    w, cw = _i32([1600])
    one = lib.ls2fm_sift_workspace_bytes(ch, cw, 1, ctypes.byref(o))
    levels = 6 * 2400 * 3200 * 4
    assert levels < one < 4 * levels                              # the levels, the DoG planes, the further octaves; no more
    h49, ch49 = _i32([1200] * 49)
    w49, cw49 = _i32([1600] * 49)
    many = lib.ls2fm_sift_workspace_bytes(ch49, cw49, 49, ctypes.byref(o))
    assert one <= many <= 2 << 30                                 # bounded by the chunk, not by the call
    tight = _opts(max_workspace_bytes=1)
    assert lib.ls2fm_sift_workspace_bytes(ch49, cw49, 49, ctypes.byref(tight)) == one      # one view per chunk


def test_refusals_enqueue_nothing():
    from ls2fm import _lib
    lib = _lib.load()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)
    off = np.zeros(1, dtype=np.int64)
    c_off = off.ctypes.data_as(ctypes.c_void_p)

    def query(h, w, **kw):
        o = _opts(**kw)
        a, ca = _i32([h])
        b, cb = _i32([w])
        return lib.ls2fm_sift_workspace_bytes(ca, cb, 1, ctypes.byref(o))

    assert query(15, 40) == INVALID and query(40, 15) == INVALID and query(16, 16) > 0
    assert query(9000, 64) == UNSUPPORTED
    assert query(64, 64, first_octave=1) == INVALID and query(64, 64, first_octave=-2) == INVALID
    assert query(64, 64, octave_resolution=4) == UNSUPPORTED and query(64, 64, num_octaves=5) == UNSUPPORTED
    assert query(64, 64, max_num_orientations=3) == UNSUPPORTED and query(64, 64, max_num_features=0) == INVALID
    assert query(64, 64, peak_threshold=float("nan")) == INVALID and query(64, 64, edge_threshold=0.0) == INVALID
    o = _opts()
    a, ca = _i32([64])
    assert lib.ls2fm_sift_workspace_bytes(null, ca, 1, ctypes.byref(o)) == INVALID
    assert lib.ls2fm_sift_workspace_bytes(ca, ca, 0, ctypes.byref(o)) == INVALID
    assert lib.ls2fm_sift_workspace_bytes(ca, ca, 1, None) == INVALID

    def call(pix=fake, offs=c_off, h=ca, kp=fake, desc=fake, cnt=fake, ws=fake, opts=o):
        return lib.ls2fm_sift_extract(pix, offs, h, ca, 1, ctypes.byref(opts), kp, desc, cnt, ws, null)

    for k in ("pix", "offs", "h", "kp", "desc", "cnt"):
        assert call(**{k: null}) == INVALID, k
    assert call(ws=null) == WORKSPACE and call(ws=ctypes.c_void_p((1 << 20) + 16)) == WORKSPACE
    small, c_small = _i32([15])
    assert call(h=c_small) == INVALID
    with pytest.raises(ValueError):
        _opts(normalization="l3")


def test_levels_of_an_impulse_have_the_stated_sigma():
    """the base is the impulse itself (first_octave 0; its nominal blur of 0.5 is a convention, so the impulse measures the blur
    APPLIED): level l carries sqrt(sigma_l^2 - 0.25), the next octave's first level twice its own in the finer pixels"""
    img = np.zeros((129, 129), dtype=np.float32)
    img[64, 64] = 1.0
    octs = R.scale_space(img, first_octave=0, num_octaves=2, dtype=np.float64)
    yy, xx = np.mgrid[0:129, 0:129].astype(np.float64)
    for l, want in enumerate(R.level_sigmas()):
        L = octs[0][l]
        assert abs(L.sum() - 1.0) < 1e-9
        var = (L * (xx - 64) ** 2).sum()
        assert abs(np.sqrt(var) - np.sqrt(want ** 2 - 0.25)) < 0.02 * want, (l, np.sqrt(var), want)       # the taps stop at 4 sigma
    assert octs[1].shape == (6, 64, 64)
    assert np.array_equal(octs[1][0], octs[0][R.S][0::2, 0::2][:64, :64])
    assert abs(R.level_sigmas()[R.S] - 2.0 * R.level_sigmas()[0]) < 1e-12


def test_isolated_blob_is_found_at_its_centre_and_scale():
    sigma, cy, cx = 4.0, 40.0, 52.0
    yy, xx = np.mgrid[0:80, 0:104].astype(np.float64)
    img = (0.2 + 0.6 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))).astype(np.float32)
    out = R.extract(img, np.float64)
    kp = out["keypoints"]
    near = np.hypot(kp[:, 0] - (cx + 0.5), kp[:, 1] - (cy + 0.5)) < 0.25
    assert near.any(), kp
    # a Gaussian blob of sigma s answers the scale-normalised Laplacian most strongly at scale s (DoG: within a level's ratio)
    ratio = kp[near, 2] / sigma
    assert ((ratio > 2 ** (-1 / 3)) & (ratio < 2 ** (1 / 3))).any(), kp[near]


def test_constant_image_gives_no_keypoint():
    out = R.extract(SC.scene_d(), np.float32)
    assert out["keypoints"].shape == (0, 4) and out["descriptors"].shape == (0, 128)


def test_descriptor_bin_permutation():
    p = R.UBC_FROM_VLFEAT
    assert sorted(p.tolist()) == list(range(128))
    assert p[0] == 0 and p[1] == 7 and p[7] == 1 and p[8] == 8 and p[9] == 15        # cell kept, orientation bins reversed
    assert np.array_equal(p[p], np.arange(128))                                       # an involution


@pytest.mark.parametrize("name", ["A", "B"])
def test_input_condition_float32_and_float64_find_the_same_keypoints(name):
    a, b = _both(name)
    g = R.gaps(a, b)
    print(f"[sift] scene {name}: {g['n_a']} / {g['n_b']} rows (fp32 / fp64), {g['paired']} paired, unpaired share {g['unpaired']:.4f}")
    assert min(g["n_a"], g["n_b"]) >= 40
    assert g["unpaired"] <= 0.01
    assert len({tuple(k) for k in b["keys"].tolist()}) == len(b["keys"])              # the key is unique
    assert b["keys"].tolist() == sorted(b["keys"].tolist())                           # and the rows come in its order


def test_scene_c_carries_enough_true_matches():
    first, second, M = SC.scene_c()
    e0, e1 = R.extract(first, np.float64), R.extract(second, np.float64)
    m = MR.match_pair(e0["descriptors"], e1["descriptors"])["matches"]
    p = e0["keypoints"][m[:, 0], :2] @ M[:2, :2].T + M[:2, 2]
    err = np.linalg.norm(p - e1["keypoints"][m[:, 1], :2], axis=1)
    print(f"[sift] scene C: {len(e0['keys'])} / {len(e1['keys'])} rows, {len(m)} matches, {(err < 4.0).sum()} within 4 px")
    assert (err < 4.0).sum() >= 50


@pytest.mark.parametrize("name", ["A", "B"])
def test_gap_recording(name):
    """the restatement's float32-vs-float64 gaps: the GPU tests hold the device to 4x these against the float64 restatement"""
    g = R.gaps(*_both(name))
    print(f"[sift] scene {name} fp32-vs-fp64 gaps: levels (worst per octave) {[f'{max(o):.2e}' for o in g['level']]}, x {g['x']:.2e}, "
          f"y {g['y']:.2e}, scale {g['scale']:.2e}, orientation {g['orientation']:.2e} rad, descriptor {g['descriptor']} counts")
    assert all(0 < v < 1e-5 for o in g["level"] for v in o)
    assert g["x"] < 0.05 and g["y"] < 0.05 and g["scale"] < 0.05 and g["orientation"] < 0.05 and g["descriptor"] <= 8
