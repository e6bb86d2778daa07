"""SIFT extraction, host side (no GPU): the C ABI's symbols and refusals, the numpy restatement (tests/sift_restate.py) on cases
with known answers, the input conditions the GPU tests rest on (float32 and float64 restatement agree on which keypoints exist;
scene C carries enough true matches), and the restatement's own float32-vs-float64 gaps, which are the GPU tests' yardstick.
The second half pins what tests/test_hip_sift.py's option, short-view, cap, deep-octave and quarter-turn tests rest on: the row
counts of every scene and option they run, that each option changes the rows, that float32 and float64 leave no row unpaired
(0.0, so the GPU tests' 0.02 is a cap and not a measurement), B's twin rows, and the quarter-turn calibration."""
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


# ---- conditions of the option, short-view, cap, deep-octave and quarter-turn tests of tests/test_hip_sift.py ----

ALL_SCENES = dict(A=SC.scene_a, B=SC.scene_b, E=SC.scene_e, **{n: functools.partial(SC.small, n) for n in SC.SMALL})


@functools.lru_cache(maxsize=None)
def _pair(name, items=()):
    img = ALL_SCENES[name]()
    return R.extract(img, np.float32, **dict(items)), R.extract(img, np.float64, **dict(items))


def _per_octave(keys):
    return tuple(int((keys[:, 0] == k).sum()) for k in range(4))


def _key_set(e):
    return {tuple(k) for k in e["keys"].tolist()}


# (scene, options, rows of the float64 restatement); the defaults give A 51 and B 290
OPTION_ROWS = [("A", dict(num_octaves=1), 32), ("A", dict(num_octaves=2), 49), ("B", dict(num_octaves=3), 287),
               ("A", dict(peak_threshold=0.0), 54), ("A", dict(peak_threshold=0.02), 30), ("A", dict(edge_threshold=3.0), 36),
               ("A", dict(max_num_orientations=1), 46), ("A", dict(first_octave=0, num_octaves=2), 19)]


@pytest.mark.parametrize("name,options,rows", OPTION_ROWS, ids=[f"{n}-" + "-".join(f"{k}={v}" for k, v in o.items()) for n, o, _ in OPTION_ROWS])
def test_every_option_changes_the_restated_rows(name, options, rows):
    """an option the device ignored could not pass the GPU test of the same case: the restated row set differs from the default's"""
    default = _pair(name)[1]
    a, b = _pair(name, tuple(sorted(options.items())))
    g = R.gaps(a, b)
    print(f"[sift] scene {name} {options}: {len(b['keys'])} rows, per octave {_per_octave(b['keys'])} (default {len(default['keys'])}), "
          f"fp32-vs-fp64 unpaired share {g['unpaired']:.4f}")
    assert len(b["keys"]) == rows and g["unpaired"] == 0.0
    assert _key_set(b) != _key_set(default)
    if options == dict(num_octaves=3):                 # drops B's three rows of octave index 3 and nothing else
        assert _per_octave(default["keys"])[3] == 3 and np.array_equal(b["keys"], default["keys"][default["keys"][:, 0] < 3])
    if options == dict(max_num_orientations=1):
        assert (b["keys"][:, 4] == 0).all() and (default["keys"][:, 4] == 1).sum() == len(default["keys"]) - rows
    if "first_octave" not in options:
        assert len(default["keys"]) == {"A": 51, "B": 290}[name]


@pytest.mark.parametrize("first_octave", [-1, 0])
@pytest.mark.parametrize("name", sorted(SC.SMALL))
def test_small_scenes_have_the_recorded_octaves_and_rows(name, first_octave):
    h, w, _ = SC.SMALL[name]
    a, b = _pair(name, (("first_octave", first_octave),))
    up = 2 if first_octave == -1 else 1
    sides, hh, ww = [], h * up, w * up
    while min(hh, ww) >= R.MIN_SIDE and len(sides) < 4:
        sides.append((6, hh, ww))
        hh, ww = hh // 2, ww // 2
    g = R.gaps(a, b)
    print(f"[sift] scene {name} first_octave {first_octave}: octaves {[l.shape[1:] for l in b['levels']]}, {len(b['keys'])} rows, per octave "
          f"{_per_octave(b['keys'])}, fp32-vs-fp64 unpaired share {g['unpaired']:.4f}")
    assert [l.shape for l in b["levels"]] == sides
    assert len(sides) == {("S33", -1): 4, ("S33", 0): 3}.get((name, first_octave), 3 if first_octave == -1 else 2)
    assert len(b["keys"]) == SC.SMALL_ROWS[name][first_octave] and g["unpaired"] == 0.0
    if name == "S33":
        assert min(b["levels"][-1].shape[1:]) == R.MIN_SIDE             # the last octave is exactly as small as an octave may be


def _straddling_caps(keys, scales):
    """caps whose last kept row has orientation index 0 while the next row in scale order is the same candidate's index 1"""
    n = len(keys)
    order = np.lexsort((np.arange(n), -np.asarray(scales, dtype=np.float64)))
    return [c for c in range(1, n) if keys[order[c - 1], 4] == 0 and keys[order[c], 4] == 1 and order[c] == order[c - 1] + 1]


def test_scene_b_has_twin_rows_and_a_cap_that_parts_them():
    a, b = _pair("B")
    n = len(b["keys"])
    assert n == 290 and (b["keys"][:, 4] == 1).sum() == 36
    caps = _straddling_caps(b["keys"], b["keypoints"][:, 2])
    print(f"[sift] scene B: {n} rows, 36 of orientation index 1, caps that part twins {caps[:8]} ... ({len(caps)})")
    assert len([c for c in caps if c >= 10]) >= 1
    cap = [c for c in caps if c >= 10][0]
    for c in (1, cap, cap + 1, n - 1, n, n + 1):
        ca, cb = R.cap_rows(a, c), R.cap_rows(b, c)
        assert len(cb["keys"]) == min(c, n) and R.gaps(ca, cb)["unpaired"] == 0.0, c
    cut = R.cap_rows(b, cap)["keys"]
    twin = R.cap_rows(b, cap + 1)["keys"]
    lost = _key_set(dict(keys=twin)) - _key_set(dict(keys=cut))
    assert len(lost) == 1 and next(iter(lost))[4] == 1 and next(iter(lost))[:4] + (0,) in _key_set(dict(keys=cut))
    again = R.extract(SC.scene_b(), np.float64, max_num_features=cap)       # cap_rows is extract's own last step
    assert np.array_equal(again["keys"], cut) and np.array_equal(again["keypoints"], R.cap_rows(b, cap)["keypoints"])
    # the batch case of the GPU tests: A, B and S33 under half of the smallest view's count, and under 7
    counts = [len(_pair(v)[1]["keys"]) for v in ("A", "B", "S33")]
    assert counts == [51, 290, 44]
    for v in ("A", "B", "S33"):
        for c in (min(counts) // 2, 7):
            assert R.gaps(R.cap_rows(_pair(v)[0], c), R.cap_rows(_pair(v)[1], c))["unpaired"] == 0.0, (v, c)


def test_scene_e_fills_the_deep_octaves():
    a, b = _pair("E")
    g = R.gaps(a, b)
    rows = _per_octave(b["keys"])
    print(f"[sift] scene E: octaves {[l.shape[1:] for l in b['levels']]}, rows per octave {rows}, fp32-vs-fp64 unpaired share {g['unpaired']:.4f}")
    assert [l.shape[1:] for l in b["levels"]] == [(260, 354), (130, 177), (65, 88), (32, 44)]
    assert rows == SC.ROWS_E and rows[2] >= 30 and rows[3] >= 10 and g["unpaired"] == 0.0


QUARTER_TURN = dict(first_octave=0, num_octaves=1, max_num_orientations=1)
# the float64 calibration on scene B: 61 of 65 rows pair; the four that do not are rows whose histogram has a second peak
QUARTER_TURN_SHARE = 61 / 65


def test_quarter_turn_calibration():
    """first_octave 0 (no up-sampling, whose repeated last row is not symmetric), one octave (no every-second-pixel step) and one
    orientation: every stated rule then commutes with np.rot90 except the order of the row and column blurs (a rounding matter)
    and the first-peak-in-bin-order rule.  Float64 shows the rules do commute: all rows pair except those with a second peak,
    and the pairs differ by 1e-12.  That figure is the float64 rounding of the blur order; float32 coordinates near 100 px are
    7.6e-6 apart, so it cannot serve a float32 device as a bar.  The GPU test therefore takes the share from here and, by the
    rule of every other bar of that file, 4x the differences the float32 restatement reaches on the same check, recorded below."""
    img = SC.scene_b()
    turned = np.ascontiguousarray(np.rot90(img))
    found = {}
    for dtype in (np.float64, np.float32):
        a, b = R.extract(img, dtype, **QUARTER_TURN), R.extract(turned, dtype, **QUARTER_TURN)
        c = R.quarter_turn_check(a["keypoints"], a["descriptors"], b["keypoints"], b["descriptors"], img.shape[1])
        print(f"[sift] quarter turn, {dtype.__name__} restatement: {len(a['keys'])} / {len(b['keys'])} rows, share paired {c['share']:.4f}; x {c['x']:.2e}, "
              f"y {c['y']:.2e}, scale {c['scale']:.2e}, orientation {c['orientation']:.2e}, descriptor {c['descriptor']}")
        found[dtype] = (a, c)
    a, c = found[np.float64]
    assert len(a["keys"]) == 65 and c["share"] == QUARTER_TURN_SHARE
    two_peaks = {tuple(k[:4]) for k in R.extract(img, np.float64, first_octave=0, num_octaves=1)["keys"].tolist() if k[4] == 1}
    unpaired = {tuple(k[:4]) for i, k in enumerate(a["keys"].tolist()) if i not in set(c["paired"].tolist())}
    assert len(unpaired) == 4 and unpaired <= two_peaks                       # only the bin-order rule parts a row from its turned self
    assert max(c["x"], c["y"], c["scale"], c["orientation"]) < 1e-10 and c["descriptor"] == 0
    c32 = found[np.float32][1]
    assert c32["share"] == QUARTER_TURN_SHARE
    assert max(c32["x"], c32["y"], c32["scale"], c32["orientation"]) < 1e-3 and c32["descriptor"] <= 1
