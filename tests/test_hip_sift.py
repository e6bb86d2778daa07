"""ls2fm.features on the device against the numpy restatement (tests/sift_restate.py).  Every tolerance is 4x the restatement's
own float32-vs-float64 gap on the same scene and options (the multiple the BA tests use), measured when the test runs and
printed; the reference is the float64 restatement.  Scenes are procedural (tests/sift_scenes.py).  The row counts, the twin
rows and the quarter-turn calibration these tests rest on are pinned without a device in tests/test_sift_host.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_restate as R  # noqa: E402
import sift_scenes as SC  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = dict(A=SC.scene_a, B=SC.scene_b, E=SC.scene_e, **{n: functools.partial(SC.small, n) for n in SC.SMALL})
QUANTITIES = ("x", "y", "scale", "orientation", "descriptor")


@functools.lru_cache(maxsize=None)
def _restated(name, items=()):
    """(float32 extraction, float64 extraction, their gaps) of a scene under the given options, computed once; a cap is applied
    to the cached uncapped extraction (R.cap_rows is R.extract's own last step)"""
    options = dict(items)
    if "max_num_features" in options:
        cap = options.pop("max_num_features")
        a, b, _ = _restated(name, tuple(sorted(options.items())))
        a, b = R.cap_rows(a, cap), R.cap_rows(b, cap)
    else:
        img = SCENES[name]()
        a, b = R.extract(img, np.float32, **options), R.extract(img, np.float64, **options)
    return a, b, R.gaps(a, b)


@functools.lru_cache(maxsize=None)
def _family_gap(first_octave):
    """the largest float32-vs-float64 gap per quantity over the small scenes and scene A at one first_octave: the yardstick of
    the small scenes, whose own one to ten rows are too few for a maximum over them to measure anything"""
    gaps = [_restated(n, (("first_octave", first_octave),))[2] for n in sorted(SC.SMALL) + ["A"]]
    return {k: max(g[k] for g in gaps) for k in QUANTITIES}


def _device(name, **options):
    from ls2fm.features import SiftOptions, extract
    kp, desc, keys = extract([SCENES[name]()], SiftOptions(**options), return_keys=True)[0]
    return dict(keypoints=kp.cpu().numpy(), descriptors=desc.cpu().numpy(), keys=keys.cpu().numpy())


def _check_against_restatement(name, what, floor=10, gap=None, rows=None, got=None, **options):
    """floor: the fewest paired rows that make the comparison mean something; gap: another yardstick than the scene's own;
    rows: a predicate on keys that restricts both sides (the bars then hold on those rows alone); got: a device result at hand"""
    _, ref, own = _restated(name, tuple(sorted(options.items())))
    gap = gap or own
    got = got or _device(name, **options)
    if rows is not None:
        got, ref = ({k: v[rows(e["keys"])] for k, v in e.items() if k != "levels"} for e in (got, ref))
    assert got["keys"].tolist() == sorted(got["keys"].tolist()), f"{what}: rows out of the stated order"
    ia, ib = R.pair_rows(got["keys"], ref["keys"])
    n = max(len(got["keys"]), len(ref["keys"]), 1)
    unpaired = max(len(got["keys"]) - len(ia), len(ref["keys"]) - len(ib)) / n
    ka, kb = got["keypoints"][ia].astype(np.float64), ref["keypoints"][ib]
    dth = np.abs(ka[:, 3] - kb[:, 3])
    dth = np.minimum(dth, R.TWO_PI - dth)
    reached = dict(x=np.abs(ka[:, 0] - kb[:, 0]).max(), y=np.abs(ka[:, 1] - kb[:, 1]).max(), scale=np.abs(ka[:, 2] - kb[:, 2]).max(),
                   orientation=dth.max())
    ddesc = int(np.abs(got["descriptors"][ia].astype(np.int64) - ref["descriptors"][ib].astype(np.int64)).max())
    print(f"[sift] {what}: {len(got['keys'])} device rows / {len(ref['keys'])} restated, unpaired {unpaired:.4f}; reached (bar = 4 x gap): "
          + ", ".join(f"{k} {v:.2e} ({4 * gap[k]:.2e})" for k, v in reached.items()) + f", descriptor {ddesc} ({4 * gap['descriptor'] + 1})")
    assert len(ia) >= floor                               # not vacuous (scene A without the up-sampling has 19 rows)
    assert unpaired <= 0.02, f"{what}: {unpaired:.4f} of the rows unpaired"
    for k, v in reached.items():
        assert v <= 4 * gap[k], f"{what}: {k} off by {v:.3e}, bar {4 * gap[k]:.3e}"
    assert ddesc <= 4 * gap["descriptor"] + 1, f"{what}: descriptor off by {ddesc}"
    return got, dict(reached, descriptor=ddesc)


@pytest.mark.parametrize("name", ["A", "B"])
def test_1_levels(name):
    from ls2fm.features import gaussian_levels
    _, ref, gap = _restated(name)
    got = gaussian_levels(SCENES[name]())
    assert len(got) == len(ref["levels"])
    for k, (g, r) in enumerate(zip(got, ref["levels"])):
        assert tuple(g.shape) == r.shape, (k, tuple(g.shape), r.shape)
        g = g.cpu().numpy().astype(np.float64)
        for l in range(R.N_LEVELS):
            err = np.abs(g[l] - r[l]).max()
            bar = max(4 * gap["level"][k][l], float(np.spacing(np.float32(np.abs(r[l]).max()))))
            print(f"[sift] scene {name} octave {k} level {l}: {err:.2e} (bar {bar:.2e})")
            assert err <= bar, (name, k, l, err, bar)


@pytest.mark.parametrize("name", ["A", "B"])
def test_2_keypoints_and_descriptors(name):
    _check_against_restatement(name, f"scene {name}")


def test_3_cap_keeps_the_largest_scales_in_order():
    from ls2fm.features import SiftOptions, extract
    full = _device("B")
    n = len(full["keys"])
    half = n // 2
    order = np.lexsort((np.arange(n), -full["keypoints"][:, 2].astype(np.float64)))
    keep = np.sort(order[:half])
    kp, desc, keys = extract([SC.scene_b()], SiftOptions(max_num_features=half), return_keys=True)[0]
    assert kp.shape[0] == half
    assert np.array_equal(keys.cpu().numpy(), full["keys"][keep])
    assert np.array_equal(kp.cpu().numpy(), full["keypoints"][keep]) and np.array_equal(desc.cpu().numpy(), full["descriptors"][keep])


def _straddling_caps(keys, scales):
    """caps whose last kept row has orientation index 0 while the next row in scale order is the same candidate's index 1"""
    n = len(keys)
    order = np.lexsort((np.arange(n), -np.asarray(scales, dtype=np.float64)))
    return [c for c in range(1, n) if keys[order[c - 1], 4] == 0 and keys[order[c], 4] == 1 and order[c] == order[c - 1] + 1]


def test_3_cap_at_its_edges_and_between_twin_rows():
    """caps 1, n - 1, n, n + 1, one that keeps the first of a candidate's two orientations and drops the second, and one more:
    against the device's own uncapped rows under the stated rule, and against the capped restatement (the floor is the cap
    itself, up to 10)"""
    from ls2fm.features import SiftOptions, extract
    full = _device("B")
    n = len(full["keys"])
    scales = full["keypoints"][:, 2].astype(np.float64)
    order = np.lexsort((np.arange(n), -scales))
    between = [c for c in _straddling_caps(full["keys"], scales) if c >= 10]
    assert between, "scene B has no cap that parts twin rows"
    for cap in (1, between[0], between[0] + 1, n - 1, n, n + 1):
        keep = np.sort(order[:cap])
        kp, desc, keys = extract([SC.scene_b()], SiftOptions(max_num_features=cap), return_keys=True)[0]
        got = dict(keypoints=kp.cpu().numpy(), descriptors=desc.cpu().numpy(), keys=keys.cpu().numpy())
        assert kp.shape[0] == min(cap, n)
        for k in ("keys", "keypoints", "descriptors"):
            assert np.array_equal(got[k], full[k][keep]), (cap, k)
        if cap == between[0]:
            assert got["keys"][:, 4].tolist().count(1) == full["keys"][np.sort(order[:cap + 1])][:, 4].tolist().count(1) - 1
        _check_against_restatement("B", f"scene B cap {cap}", floor=min(cap, 10), got=got, max_num_features=cap)


@pytest.mark.parametrize("cap", ["half_of_the_smallest", 7])
def test_3_cap_in_a_batch_keeps_the_views_apart(cap):
    """with a small max_num_features the output stride of a view is small too: view * max_features + row on the device and
    i * max_num_features in the slicing are all that keep the views apart"""
    from ls2fm.features import SiftOptions, extract
    images = [SC.scene_a(), SC.scene_b(), SC.small("S33")]
    uncapped = [int(k.shape[0]) for k, _ in extract(images)]
    assert uncapped == [len(_restated(v)[1]["keys"]) for v in ("A", "B", "S33")]
    cap = min(uncapped) // 2 if cap == "half_of_the_smallest" else cap
    opt = SiftOptions(max_num_features=cap)
    single = [extract([i], opt)[0] for i in images]
    runs = dict(batch=extract(images, opt), library_chunks=extract(images, SiftOptions(max_num_features=cap, max_workspace_bytes=1)),
                call_chunks=extract(images, SiftOptions(max_num_features=cap, chunk_views=2)))
    print(f"[sift] cap {cap} in a batch of views with {uncapped} rows: {[int(k.shape[0]) for k, _ in runs['batch']]} rows")
    for what, got in runs.items():
        assert [int(k.shape[0]) for k, _ in got] == [min(cap, n) for n in uncapped], what
        for v, ((k, d), (ks, ds)) in enumerate(zip(got, single)):
            assert k.shape == ks.shape and torch.equal(k, ks) and torch.equal(d, ds), f"{what}: view {v} differs from its single call"


def test_3_batch_rerun_and_chunking_return_the_same_bits():
    from ls2fm.features import SiftOptions, extract
    c0, c1, _ = SC.scene_c()
    images = [SC.scene_a(), SC.scene_b(), SC.scene_d(), c0, c1]
    single = [extract([i])[0] for i in images]
    runs = dict(batch=extract(images), rerun=extract(images), library_chunks=extract(images, SiftOptions(max_workspace_bytes=1)),
                call_chunks=extract(images, SiftOptions(chunk_views=2)))
    assert [int(k.shape[0]) for k, _ in single][2] == 0 and min(int(k.shape[0]) for k, _ in single[:2] + single[3:]) >= 40
    for what, got in runs.items():
        assert len(got) == len(images)
        for v, ((k, d), (ks, ds)) in enumerate(zip(got, single)):
            assert k.shape == ks.shape and torch.equal(k, ks) and torch.equal(d, ds), f"{what}: view {v} differs from its single call"


def test_4_constant_image_and_small_image():
    from ls2fm.features import extract
    kp, desc = extract([SC.scene_d()])[0]
    assert tuple(kp.shape) == (0, 4) and tuple(desc.shape) == (0, 128)
    with pytest.raises(RuntimeError, match="invalid argument|status -1"):
        extract([np.full((15, 40), 0.5, dtype=np.float32)])
    # uint8 and RGB inputs follow the stated conversions
    grey = SC.scene_a()
    rgb = np.stack([grey, grey, grey], axis=-1)
    k_rgb, _ = extract([rgb])[0]
    want = R.to_grey(rgb)
    k_ref, _ = extract([want])[0]
    assert torch.equal(k_rgb, k_ref)
    u8 = np.round(grey * 255).astype(np.uint8)
    assert torch.equal(extract([u8])[0][0], extract([R.to_grey(u8)])[0][0])


OPTION_CASES = [("A", dict(first_octave=0)), ("A", dict(upright=True)), ("A", dict(normalization="l2")), ("A", dict(num_octaves=1)),
                ("A", dict(num_octaves=2)), ("B", dict(num_octaves=3)), ("A", dict(peak_threshold=0.0)), ("A", dict(peak_threshold=0.02)),
                ("A", dict(edge_threshold=3.0)), ("A", dict(max_num_orientations=1)), ("A", dict(first_octave=0, num_octaves=2))]
OPTION_IDS = ["first_octave_0", "upright", "l2", "num_octaves_1", "num_octaves_2", "B_num_octaves_3", "peak_0", "peak_0.02", "edge_3",
              "one_orientation", "first_octave_0_num_octaves_2"]


@pytest.mark.parametrize("name,options", OPTION_CASES, ids=OPTION_IDS)
def test_4_options_agree_with_the_restatement(name, options):
    """tests/test_sift_host.py shows that each of these options changes the restated rows, so a device that ignored one fails"""
    got, _ = _check_against_restatement(name, f"scene {name} {options}", **options)
    if options == dict(num_octaves=3):                    # B's three rows of octave index 3 go, and nothing else changes
        full = _device("B")
        keep = full["keys"][:, 0] < 3
        assert int((~keep).sum()) == 3
        for k in ("keys", "keypoints", "descriptors"):
            assert np.array_equal(got[k], full[k][keep]), k
    if options == dict(max_num_orientations=1):
        assert (got["keys"][:, 4] == 0).all()


def test_5_end_to_end_on_the_pair():
    from ls2fm import pose
    from ls2fm.features import extract, n_views_from_images
    from ls2fm.match import match_descriptors
    c0, c1, M = SC.scene_c()
    (k0, d0), (k1, d1) = extract([c0, c1])
    matches = match_descriptors([d0, d1])[0]
    uv0 = k0[matches[:, 0], :2].double()
    uv1 = k1[matches[:, 1], :2].double()
    out = pose.homography([uv0], [uv1], seed=0)
    inl = out["inliers"].cpu().numpy()
    H = out["H"].cpu().numpy()[0]
    print(f"[sift] scene C: {k0.shape[0]} / {k1.shape[0]} rows, {matches.shape[0]} matches, {int(inl.sum())} homography inliers")
    assert int(inl.sum()) >= 50
    corners = np.array([[0.0, 0.0, 1.0], [320.0, 0.0, 1.0], [0.0, 240.0, 1.0], [320.0, 240.0, 1.0]])
    got = corners @ H.T
    got = got[:, :2] / got[:, 2:]
    want = (corners @ M.T)[:, :2]
    err = np.linalg.norm(got - want, axis=1)
    print(f"[sift] scene C: corner errors {np.round(err, 3)} px")
    assert err.max() <= 4.0
    tables = n_views_from_images([c0, c1], intrinsic=None, seed=0)
    assert len(tables) == 2 and np.array_equal(tables[0]["kypts"], k0[:, :2].cpu().numpy().astype(np.float64))
    assert np.array_equal(tables[0]["indxes"][0], matches.cpu().numpy().astype(np.uint32))
    assert np.array_equal(tables[1]["indxes"][0], matches.cpu().numpy().astype(np.uint32)[:, [1, 0]])
    from ls2fm.match import two_view_tables
    again = two_view_tables([k0[:, :2].cpu().numpy().astype(np.float64), k1[:, :2].cpu().numpy().astype(np.float64)], [d0, d1], None, seed=0)
    assert np.array_equal(tables[0]["mask"][0], again[0]["mask"][0]) and np.array_equal(tables[1]["mask"][0], again[0]["mask"][0])
    assert tables[0]["mask"][0].sum() >= 50


def _octave_shapes(name, first_octave):
    h, w, _ = SC.SMALL[name]
    up = 2 if first_octave == -1 else 1
    shapes, h, w = [], h * up, w * up
    while min(h, w) >= R.MIN_SIDE and len(shapes) < 4:
        shapes.append((R.N_LEVELS, h, w))
        h, w = h // 2, w // 2
    return shapes


@pytest.mark.parametrize("first_octave", [-1, 0])
@pytest.mark.parametrize("name", sorted(SC.SMALL))
def test_6_short_views_alone(name, first_octave):
    """views of two and three octaves (16 x 16 is the smallest legal size).  Levels: the number and shapes of the octaves and the
    bar of test_1_levels (a maximum over a plane, so the scene's own gap).  Keypoints and descriptors: the yardstick per quantity
    is the largest gap over the small scenes and scene A at the same first_octave, since one to ten rows measure nothing; the
    floor is the restated row count pinned in tests/test_sift_host.py, so every restated row must be found."""
    from ls2fm.features import SiftOptions, gaussian_levels
    _, ref, gap = _restated(name, (("first_octave", first_octave),))
    got = gaussian_levels(SCENES[name](), SiftOptions(first_octave=first_octave))
    assert [tuple(g.shape) for g in got] == _octave_shapes(name, first_octave) == [r.shape for r in ref["levels"]]
    worst = (0.0, 0.0)
    for k, (g, r) in enumerate(zip(got, ref["levels"])):
        g = g.cpu().numpy().astype(np.float64)
        for l in range(R.N_LEVELS):
            err = np.abs(g[l] - r[l]).max()
            bar = max(4 * gap["level"][k][l], float(np.spacing(np.float32(np.abs(r[l]).max()))))
            worst = max(worst, (err / bar, err))
            assert err <= bar, (name, k, l, err, bar)
    print(f"[sift] scene {name} first_octave {first_octave}: octaves {[tuple(g.shape[1:]) for g in got]}, worst level error {worst[1]:.2e} "
          f"({worst[0]:.2f} of its bar)")
    assert len(ref["keys"]) == SC.SMALL_ROWS[name][first_octave]
    _check_against_restatement(name, f"scene {name} first_octave {first_octave}", floor=SC.SMALL_ROWS[name][first_octave],
                               gap=_family_gap(first_octave), first_octave=first_octave)


@pytest.mark.parametrize("options", [dict(), dict(first_octave=0), dict(chunk_views=2), dict(max_workspace_bytes=1)],
                         ids=["default", "first_octave_0", "call_chunks", "library_chunks"])
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_6_short_views_in_mixed_batches(order, options):
    """a view of three octaves in launches sized by a view of four, before and after it: every view has the bits of its single call"""
    from ls2fm.features import SiftOptions, extract
    names = ["S23", "B", "S31", "A", "S16"]
    names = names[::-1] if order == "reverse" else names
    images = [SCENES[n]() for n in names]
    opt = SiftOptions(**options)
    single_opt = SiftOptions(first_octave=opt.first_octave)
    single = [extract([i], single_opt)[0] for i in images]
    got = extract(images, opt)
    rows = [int(k.shape[0]) for k, _ in got]
    print(f"[sift] batch {names} {options}: {rows} rows")
    assert rows == [len(_restated(n, (("first_octave", opt.first_octave),))[1]["keys"]) for n in names]
    assert len(got) == len(images)
    for v, ((k, d), (ks, ds)) in enumerate(zip(got, single)):
        assert k.shape == ks.shape and torch.equal(k, ks) and torch.equal(d, ds), f"view {v} ({names[v]}) differs from its single call"


def test_7_deep_octaves_with_odd_sides():
    """scene E: 260 x 354 -> 130 x 177 -> 65 x 88 -> 32 x 44 with 41 and 12 restated rows in octave indices 2 and 3.  The whole
    scene under the usual bars, then the rows of octave index >= 2 alone under 4x the restatement's gap on those same rows, all
    53 of them found, so that an error of the pixel step, the offset or the every-second-pixel step cannot hide under octave 0's
    maximum"""
    a, b, _ = _restated("E")
    got, _ = _check_against_restatement("E", "scene E")
    for k in range(4):                                               # printed, not held: twelve rows are no yardstick
        g, r = ({q: v[e["keys"][:, 0] == k] for q, v in e.items() if q != "levels"} for e in (got, b))
        d = R.gaps(dict(g, levels=[]), dict(r, levels=[]))
        print(f"[sift] scene E octave index {k}: {d['n_a']} device rows / {d['n_b']} restated, unpaired {d['unpaired']:.4f}; reached "
              + ", ".join(f"{q} {d[q]:.2e}" for q in QUANTITIES[:4]) + f", descriptor {d['descriptor']}")
        assert d["n_b"] == SC.ROWS_E[k]
    deep = lambda keys: keys[:, 0] >= 2                              # noqa: E731
    part = [{q: v[deep(e["keys"])] for q, v in e.items() if q != "levels"} for e in (a, b)]
    _check_against_restatement("E", "scene E octave index >= 2", floor=SC.ROWS_E[2] + SC.ROWS_E[3],
                               gap=R.gaps(dict(part[0], levels=[]), dict(part[1], levels=[])), rows=deep, got=got)


def test_8_quarter_turn():
    """an image against np.rot90 of itself under first_octave 0, one octave and one orientation, where every stated rule commutes
    with the turn except the rounding order of the two blurs and the first-peak-in-bin-order rule (R.quarter_turn derives the
    mapping from np.rot90's definition, not from an implementation).  The float64 restatement pairs 61 of 65 rows -- the other
    four have a second peak -- and its pairs differ by 1e-12 (tests/test_sift_host.py): the rules commute.  The device must pair
    that share less 0.02.  Its pairs are held to 4x the differences the FLOAT32 restatement reaches on the same check, + 1 on
    descriptor bytes: 4x the float64 figure is far below the spacing of float32 coordinates (7.6e-6 at 100 px) and no float32
    output could meet it."""
    from ls2fm.features import SiftOptions, extract
    opts = dict(first_octave=0, num_octaves=1, max_num_orientations=1)
    img = SC.scene_b()
    turned = np.ascontiguousarray(np.rot90(img))
    cal = {}
    for dtype in (np.float64, np.float32):
        a, b = R.extract(img, dtype, **opts), R.extract(turned, dtype, **opts)
        cal[dtype] = R.quarter_turn_check(a["keypoints"], a["descriptors"], b["keypoints"], b["descriptors"], img.shape[1])
    (k0, d0), (k1, d1) = extract([img, turned], SiftOptions(**opts))
    c = R.quarter_turn_check(k0.cpu().numpy(), d0.cpu().numpy(), k1.cpu().numpy(), d1.cpu().numpy(), img.shape[1])
    bar = {q: 4 * cal[np.float32][q] for q in QUANTITIES[:4]}
    print(f"[sift] quarter turn of scene B: {k0.shape[0]} / {k1.shape[0]} device rows, share paired {c['share']:.4f} (float64 restatement "
          f"{cal[np.float64]['share']:.4f}); reached (bar = 4 x float32 restatement): " + ", ".join(f"{q} {c[q]:.2e} ({bar[q]:.2e})" for q in bar)
          + f", descriptor {c['descriptor']} ({4 * cal[np.float32]['descriptor'] + 1}); float64 restatement reaches "
          + ", ".join(f"{q} {cal[np.float64][q]:.1e}" for q in bar))
    assert min(k0.shape[0], k1.shape[0]) >= 60
    assert c["share"] >= cal[np.float64]["share"] - 0.02
    for q in bar:
        assert c[q] <= bar[q], f"quarter turn: {q} off by {c[q]:.3e}, bar {bar[q]:.3e}"
    assert c["descriptor"] <= 4 * cal[np.float32]["descriptor"] + 1


def test_9_input_forms_return_the_same_bits():
    from ls2fm.features import extract
    img = SC.scene_a()
    want_k, want_d = extract([img])[0]
    wide = torch.zeros((img.shape[0], img.shape[1] + 5), dtype=torch.float32, device="cuda")
    wide[:, 3:-2] = torch.from_numpy(img).cuda()
    sliced = wide[:, 3:-2]
    fortran = np.asfortranarray(img)
    assert not sliced.is_contiguous() and not fortran.flags["C_CONTIGUOUS"]
    forms = dict(device_tensor=torch.from_numpy(img).cuda(), float64=img.astype(np.float64), fortran_order=fortran, sliced_device_tensor=sliced,
                 every_second_column=np.repeat(img, 2, axis=1)[:, ::2])
    assert want_k.shape[0] >= 40
    for what, form in forms.items():
        k, d = extract([form])[0]
        assert torch.equal(k, want_k) and torch.equal(d, want_d), what
