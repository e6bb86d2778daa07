"""ls2fm.features on the device against the numpy restatement (tests/sift_restate.py).  Every tolerance is 4x the restatement's
own float32-vs-float64 gap on the same scene and options (the multiple the BA tests use), measured when the test runs and
printed; the reference is the float64 restatement.  Scenes are procedural (tests/sift_scenes.py)."""
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

SCENES = {"A": SC.scene_a, "B": SC.scene_b}


@functools.lru_cache(maxsize=None)
def _restated(name, items=()):
    """(float32 extraction, float64 extraction, their gaps) of a scene under the given options, computed once"""
    img = SCENES[name]()
    a, b = R.extract(img, np.float32, **dict(items)), R.extract(img, np.float64, **dict(items))
    return a, b, R.gaps(a, b)


def _device(name, **options):
    from ls2fm.features import SiftOptions, extract
    kp, desc, keys = extract([SCENES[name]()], SiftOptions(**options), return_keys=True)[0]
    return dict(keypoints=kp.cpu().numpy(), descriptors=desc.cpu().numpy(), keys=keys.cpu().numpy())


def _check_against_restatement(name, what, **options):
    _, ref, gap = _restated(name, tuple(sorted(options.items())))
    got = _device(name, **options)
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
    assert len(ia) >= 10                                  # not vacuous (scene A without the up-sampling has 19 rows)
    assert unpaired <= 0.02, f"{what}: {unpaired:.4f} of the rows unpaired"
    for k, v in reached.items():
        assert v <= 4 * gap[k], f"{what}: {k} off by {v:.3e}, bar {4 * gap[k]:.3e}"
    assert ddesc <= 4 * gap["descriptor"] + 1, f"{what}: descriptor off by {ddesc}"


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


@pytest.mark.parametrize("options", [dict(first_octave=0), dict(upright=True), dict(normalization="l2")], ids=["first_octave_0", "upright", "l2"])
def test_4_options_agree_with_the_restatement(options):
    _check_against_restatement("A", f"scene A {options}", **options)


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
