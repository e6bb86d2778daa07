"""GPU: every output bit of ls2fm_sphere_trace (wave, wide and narrow kernel; near, far, track, t_end history, track_sdf, trips),
ls2fm_trace_image, ls2fm_sdf_eval in its five launch choices, ls2fm_sdf_eval_prepared and ls2fm_sdf_volume against what the library
of the commit before csrc/trace_loop.h produced on an MI355X (tests/golden/trace_parent.json, recorded by
tests/golden/make_golden_trace_parent.py, whose case builders this file runs).  The build is -ffp-contract=off and every sum is
fixed-order, so there is no tolerance: only a moved operation changes a bit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_golden_trace_parent", os.path.join(GOLDEN, "make_golden_trace_parent.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "trace_parent.json")) as f:
        return json.load(f)


def same(golden, prefix, out):
    want = {k[len(prefix) + 1:]: v for k, v in golden["entries"].items() if k.startswith(prefix + "/")}
    assert sorted(want) == sorted(out), prefix
    for k, v in out.items():
        got = R.encode(v, R.case_size(prefix))
        assert got["shape"] == want[k]["shape"] and got["dtype"] == want[k]["dtype"], (prefix, k)
        assert got == want[k], (prefix, k)


@pytest.mark.parametrize("name, n, it", R.TRACE_CASES)
def test_sphere_trace_bits_unchanged(golden, name, n, it):
    key = R.trace_key(name, n, it)
    out = R.run_trace(name, n, it)
    assert int(out["trips"].item()) == golden["trace_trips"][key]
    same(golden, key, out)
    assert set(out) == {"near", "far", "track", "t_end", "track_sdf", "trips"}


def test_trace_fixture_shows_the_loops_quirks(golden):
    """the recording itself: somewhere an end crossed, a start end converged before iters_max, a finished start end kept moving on
    its stale value and the background branch was selected; the image views got different trip counts, and K = 0 occurs"""
    props = golden["trace_properties"]
    assert set(props) == {R.trace_key(f, n, "default") for f in R.FIELDS for n in R.RAY_COUNTS}
    for p in ("crossed", "converged_before_iters_max", "moved_on_stale_value", "background_selected"):
        assert any(v[p] for v in props.values()), p
    two = golden["image_trips"]["two_views_7x5"]
    assert two[0] != two[1] and golden["image_trips"]["two_views_7x5_all_converged"] == [0, 0]
    assert len(golden["image_trips"]["one_view_1x1"]) == 1


@pytest.mark.parametrize("which", R.IMAGE_CASES)
def test_trace_image_bits_unchanged(golden, which):
    out = R.run_image(which)
    assert out["trips"].cpu().tolist() == golden["image_trips"][which]
    same(golden, f"image/{which}", out)


@pytest.mark.parametrize("which", R.POINT_CASES)
def test_point_evaluator_bits_unchanged(golden, which):
    same(golden, f"points/{which}", R.run_points(which))


def test_launch_choices_agree_in_the_recording(golden):
    """the recorded sdf column is the same in all five launch choices and in the prepared call, features and normals in theirs"""
    e = golden["entries"]
    for name in R.FIELDS:
        sdf = [e[f"points/{w}/{name}/sdf"] for w in R.POINT_CASES if w != "volume"]
        assert all(s == sdf[0] for s in sdf), name
        assert e[f"points/sdf_feat_wide/{name}/feat"] == e[f"points/thread_per_point/{name}/feat"]
        assert e[f"points/sdf_feat_normal_wide/{name}/normal"] == e[f"points/thread_per_point_normal/{name}/normal"]
