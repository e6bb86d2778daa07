"""Host: THE VERTEX COLOUR RULE judged by its properties on the numpy restatement (tests/mesh_colors_restate.py), the CPU torch
form of ls2fm.mesh_colors.photo_colors held to that restatement, and the PLY writer's colour element."""
import numpy as np
import pytest
import torch

import mesh_colors_restate as MR
import mesh_colors_scenes as S
from ls2fm import mesh, mesh_colors

EPS = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the rule, by its properties
def test_sphere_scene_is_a_closed_sphere_inside_every_image():
    sc = S.sphere_scene()
    r = np.linalg.norm(sc["verts"], axis=1)
    assert len(sc["verts"]) > 400 and float(np.abs(r - 0.5).max()) < 0.01
    assert (np.isfinite(sc["depth"]).sum(axis=(1, 2)) > 2000).all(), "every view sees the sphere"
    for d in sc["depth"]:
        assert not np.isfinite(d[0]).any() and not np.isfinite(d[:, 0]).any(), "the silhouette stays inside the image"


@pytest.mark.parametrize("view", range(6))
def test_one_view_colours_what_it_sees_and_nothing_else(view):
    sc, one = S.sphere_scene(), S.sphere_single_views()[view]
    count, colors = one["count"], one["colors"]
    cos = S.sphere_cosines(sc, view)
    seen = count > 0
    assert seen.any()
    # 1. every vertex some view counts for gets exactly that view's constant: bilinear taps of a constant image, weight 1
    assert (colors[seen] == S.SPHERE_COLORS[view]).all()
    assert (colors[~seen] == np.float32(0.5)).all()
    # 2. the far side is hidden by the near side
    assert (count[cos <= -0.2] == 0).all(), f"{int((count[cos <= -0.2] != 0).sum())} far-side vertices were coloured"
    # 3. what faces the camera is seen (the whole sphere projects into the image)
    assert (count[cos >= 0.5] == 1).all(), f"{int((count[cos >= 0.5] != 1).sum())} facing vertices were missed"
    band = (cos > -0.2) & (cos < 0.5)
    assert (cos <= -0.2).sum() > 100 and (cos >= 0.5).sum() > 100
    assert band.mean() < 0.45, f"the unjudged band holds {band.mean():.2f} of the vertices"


@pytest.mark.parametrize("with_normals,power", [(False, 1), (True, 1), (True, 4)])
def test_six_views_blend_within_the_contributing_constants(with_normals, power):
    sc, singles = S.sphere_scene(), S.sphere_single_views()
    out = MR.vertex_colors(sc["verts"], sc["poses"], sc["intr"], sc["images"], sc["depth"], near=sc["near"], depth_tol=sc["depth_tol"],
                           normals=sc["normals"] if with_normals else None, power=power)
    contrib = np.stack([s["count"] > 0 for s in singles], axis=1)                 # [V, 6], without normals
    if not with_normals:
        assert (out["count"] == contrib.sum(axis=1)).all()
        assert (out["count"] > 0).all(), "six axis cameras see the whole sphere"
    else:
        assert (out["count"] <= contrib.sum(axis=1)).all(), "a normal can only take views away"
        assert (out["count"] > 0).mean() > 0.95
    lo = np.where(contrib[:, :, None], S.SPHERE_COLORS[None], np.inf).min(axis=1)
    hi = np.where(contrib[:, :, None], S.SPHERE_COLORS[None], -np.inf).max(axis=1)
    got = out["colors"].astype(np.float64)
    seen = out["count"] > 0
    slack = 4 * 2.0 ** -24           # the fp32 cast of a convex combination formed in fp64
    assert (got[seen] >= lo[seen] - slack).all() and (got[seen] <= hi[seen] + slack).all()
    several = out["count"] > 1
    assert several.sum() > 50, "the scene must blend somewhere"
    if with_normals:
        # the weight of a view is cos^power: at a vertex two views see, the colour leans toward the view it faces
        w = out["sums"][:, 3]
        assert (w[seen] > 0).all() and (w[seen] <= out["count"][seen] + 1e-9).all()


# ------------------------------------------------------------------------------------------------ the CPU torch form
def _held_to_restatement(sc, points, C_normals, power, sel=slice(None)):
    normals = sc["normals"] if C_normals else None
    ref = MR.vertex_colors(points, sc["poses"][sel], sc["intr"] if sc["intr"].ndim == 2 else sc["intr"][sel], sc["images"][sel],
                           sc["depth"][sel], masks=sc["masks"][sel] if "masks" in sc else None, normals=normals, near=sc["near"],
                           depth_tol=sc["depth_tol"], power=power, return_terms=True)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    intr = sc["intr"] if sc["intr"].ndim == 2 else sc["intr"][sel]
    kw = dict(masks=t(sc["masks"][sel]) if "masks" in sc else None, normals=t(normals), near=sc["near"], depth_tol=sc["depth_tol"],
              power=power)
    got = mesh_colors.photo_colors(t(points), t(sc["faces"]), t(sc["poses"][sel]), t(intr), t(sc["images"][sel]), depth=t(sc["depth"][sel]),
                                   **kw)
    C = ref["sums"].shape[1] - 1
    state = (torch.zeros(len(points), C + 1, dtype=torch.float64), torch.zeros(len(points), dtype=torch.int32))
    again = mesh_colors.photo_colors_torch(t(points), t(sc["poses"][sel]), t(intr), t(sc["images"][sel]), t(sc["depth"][sel]), state=state, **kw)
    assert got.colors.dtype == torch.float32 and got.weight.dtype == torch.float64 and got.count.dtype == torch.int32
    assert torch.equal(again.count, got.count) and torch.equal(again.colors, got.colors) or torch.isnan(got.colors).any()
    assert np.array_equal(got.count.numpy(), ref["count"]), "counts are exact"
    assert np.array_equal(got.weight.numpy(), state[0][:, C].numpy(), equal_nan=True)
    # sums and colours to (count + 16) 2^-53 sum |term|; a NaN must be a NaN in both
    bound = (ref["count"][:, None] + 16) * EPS * ref["terms"]
    with np.errstate(invalid="ignore"):
        err = np.abs(state[0].numpy() - ref["sums"])
        ok = (err <= bound) | (np.isnan(state[0].numpy()) & np.isnan(ref["sums"]))
    assert ok.all(), f"{int((~ok).sum())} sums outside the bound, the worst by {np.nanmax(err - bound):.3e}"
    seen = ref["count"] > 0
    with np.errstate(invalid="ignore"):
        ce = np.abs(got.colors.numpy().astype(np.float64) - ref["colors"].astype(np.float64))
        cok = (ce <= bound[:, :C]) | (np.isnan(got.colors.numpy()) & np.isnan(ref["colors"]))
    assert cok[seen].all(), f"{int((~cok[seen]).sum())} colours outside the bound, the worst by {np.nanmax((ce - bound[:, :C])[seen]):.3e}"
    assert np.array_equal(got.colors.numpy()[~seen], ref["colors"][~seen]), "the fill is exact"
    return ref


def test_cpu_form_on_the_sphere():
    sc = S.sphere_scene()
    ref = _held_to_restatement(sc, sc["verts"], True, 2)
    assert (ref["count"] > 1).sum() > 50


@pytest.mark.parametrize("H,W,C,with_normals,power", [(17, 33, 3, True, 1), (5, 7, 1, False, 0), (33, 17, 4, True, 8)])
def test_cpu_form_on_the_edge_cases(H, W, C, with_normals, power):
    sc = S.edge_scene(H, W, C)
    ref = _held_to_restatement(sc, sc["points"], with_normals, power)
    idx, count = sc["index"], ref["count"]
    # the edge cases are what their names say, in the restatement itself (view 0 alone)
    one = MR.vertex_colors(sc["points"], sc["poses"][:1], sc["intr"][:1], sc["images"][:1], sc["depth"][:1], masks=sc["masks"][:1],
                           normals=sc["normals"] if with_normals else None, near=sc["near"], depth_tol=sc["depth_tol"], power=power)
    c0 = one["count"]
    assert c0[idx["u_zero"]] == 1 and c0[idx["u_width"]] == 0 and c0[idx["pixel_centre"]] == 1
    assert c0[idx["last_column"]] == 1 and c0[idx["last_row"]] == 1 and c0[idx["last_corner"]] == 1 and c0[idx["first_corner"]] == 1
    assert count[idx["behind_near"]] == 0 and count[idx["nan_vertex"]] == 0
    assert c0[idx["nan_pixel"]] == 1 and np.isnan(one["sums"][idx["nan_pixel"], C - 1]), "a NaN pixel stays in the vertex that sampled it"
    assert c0[idx["at_threshold"]] == 1 and c0[idx["past_threshold"]] == 0 and c0[idx["occluded"]] == 0
    assert c0[idx["masked"]] == 0 and count[idx["masked"]] >= 0
    if with_normals:
        assert count[idx["facing_away"]] == 0
    assert 0 < (count > 0).sum() and (count == 0).sum() > 2 and (count == len(sc["poses"])).any()


def test_cpu_form_needs_the_depth_maps_and_checks_its_arguments():
    sc = S.edge_scene(5, 7, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (t(sc["points"]), t(sc["faces"]), t(sc["poses"]), t(sc["intr"]), t(sc["images"]))
    with pytest.raises(RuntimeError, match="depth"):
        mesh_colors.photo_colors(*args)
    with pytest.raises(ValueError, match="depth_tol"):
        mesh_colors.photo_colors(*args, depth=t(sc["depth"]), depth_tol=-1.0)
    with pytest.raises(ValueError, match="depth_tol"):
        mesh_colors.photo_colors(*args, depth=t(sc["depth"]), depth_tol=float("nan"))
    with pytest.raises(ValueError, match="power"):
        mesh_colors.photo_colors(*args, depth=t(sc["depth"]), power=9)


def test_split_over_views_equals_one_call_in_the_restatement():
    sc = S.edge_scene(17, 33, 3)
    whole = MR.vertex_colors(sc["points"], sc["poses"], sc["intr"], sc["images"], sc["depth"], masks=sc["masks"], normals=sc["normals"],
                             near=sc["near"], depth_tol=sc["depth_tol"])
    state = MR.new_state(len(sc["points"]), 3)
    for sel in (slice(0, 2), slice(2, 3)):
        MR.accumulate(state, sc["points"], sc["poses"][sel], sc["intr"][sel], sc["images"][sel], sc["depth"][sel], sc["masks"][sel],
                      sc["normals"], sc["near"], sc["depth_tol"])
    assert np.array_equal(state[0], whole["sums"], equal_nan=True) and np.array_equal(state[1], whole["count"])


# ------------------------------------------------------------------------------------------------ PLY
def _legacy_binary(v, f):
    """the bytes write_ply wrote before it knew colours"""
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    rows = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    rows["n"], rows["idx"] = 3, f
    return head + v.astype("<f4").tobytes() + rows.tobytes()


def _legacy_ascii(v, f):
    head = ("ply\nformat ascii 1.0\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    body = "".join("%.9g %.9g %.9g\n" % tuple(float(t) for t in row) for row in v.astype(np.float64))
    body += "".join("3 %d %d %d\n" % tuple(int(t) for t in row) for row in f)
    return (head + body).encode("ascii")


def _tiny_mesh():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], np.int32)
    return v, f


def test_ply_without_colours_is_byte_identical(tmp_path):
    v, f = _tiny_mesh()
    mesh.write_ply(tmp_path / "b.ply", v, f)
    mesh.write_ply(tmp_path / "b2.ply", v, f, colors=None)
    mesh.write_ply(tmp_path / "a.ply", v, f, encoding="ascii", colors=None)
    assert (tmp_path / "b.ply").read_bytes() == _legacy_binary(v, f) == (tmp_path / "b2.ply").read_bytes()
    assert (tmp_path / "a.ply").read_bytes() == _legacy_ascii(v, f)
    assert mesh.ply_header(7, 4) == mesh.ply_header(7, 4, colors=None) == _legacy_binary(v, f)[:len(mesh.ply_header(7, 4))]
    rv, rf, rc = mesh.read_ply_colors(tmp_path / "b.ply")
    assert rc is None and np.array_equal(rv, v) and np.array_equal(rf, f)
    assert mesh.read_ply_colors(tmp_path / "a.ply")[2] is None


@pytest.mark.parametrize("encoding", ["binary", "ascii"])
@pytest.mark.parametrize("channels", [3, 4])
def test_ply_colours_round_trip_as_rounded_bytes(tmp_path, encoding, channels):
    v, f = _tiny_mesh()
    c = np.array([[0.0, 1.0, 0.5], [0.5 / 255, 1.5 / 255, 2.5 / 255], [-0.3, 1.7, 0.2], [1 / 3, 2 / 3, 0.999], [0.25, 0.75, 0.1],
                  [np.nan, 0.2, 0.4], [254.5 / 255, 0.1, 0.9]], np.float32)
    if channels == 4:
        c = np.concatenate([c, np.linspace(0, 1, 7, dtype=np.float32)[:, None]], axis=1)
    want = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0, 1) * 255).astype(np.uint8)
    # halves go to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (the float32 values k + 0.5 over 255 are not exact; the rule is np.rint's)
    assert want[0].tolist()[:3] == [0, 255, 128] and want[2].tolist()[:3] == [0, 255, 51]
    path = tmp_path / "c.ply"
    mesh.write_ply(path, torch.from_numpy(v), torch.from_numpy(f), encoding=encoding, colors=torch.from_numpy(c))
    head = path.read_bytes().split(b"end_header\n")[0].decode()
    assert "property uchar red\nproperty uchar green\nproperty uchar blue\n" in head
    assert ("property uchar alpha\n" in head) == (channels == 4)
    assert head.index("property float z") < head.index("property uchar red") < head.index("element face")
    rv, rf, rc = mesh.read_ply_colors(path)
    assert rc.dtype == np.uint8 and np.array_equal(rc, want) and np.array_equal(rv, v) and np.array_equal(rf, f)
    gv, gf = (mesh.read_ply if encoding == "binary" else mesh.read_ply_ascii)(path)
    assert np.array_equal(gv, v) and np.array_equal(gf, f), "read_ply on a coloured file still returns the geometry"
    if encoding == "binary":
        assert len(path.read_bytes()) == len(mesh.ply_header(7, 4, channels)) + 7 * (12 + channels) + 4 * 13
    mesh.write_ply(tmp_path / "u.ply", v, f, encoding=encoding, colors=want)
    assert (tmp_path / "u.ply").read_bytes() == path.read_bytes(), "uint8 colours are written as they are"


def test_ply_colour_shapes_that_raise(tmp_path):
    v, f = _tiny_mesh()
    for bad in (np.zeros((7, 2)), np.zeros((7, 5)), np.zeros((6, 3)), np.zeros(21), np.zeros((7, 3, 1))):
        with pytest.raises(ValueError):
            mesh.write_ply(tmp_path / "x.ply", v, f, colors=bad)
    with pytest.raises(ValueError):
        mesh.ply_header(7, 4, colors=2)
    mesh.write_ply(tmp_path / "a.ply", v, f, encoding="ascii")
    with pytest.raises(ValueError):
        mesh.read_ply(tmp_path / "a.ply")


def test_resolve_colors_argument():
    v, f = _tiny_mesh()
    assert mesh_colors.resolve_colors(None, v, f, None, None, "t") is None
    got = mesh_colors.resolve_colors(lambda a, b: np.full((len(a), 3), 0.25), v, f, None, None, "t")
    assert got.shape == (7, 3)
    with pytest.raises(ValueError):
        mesh_colors.resolve_colors("field", v, f, None, None, "t")
    with pytest.raises(ValueError):
        mesh_colors.resolve_colors("photos", v, f, None, None, "t")
