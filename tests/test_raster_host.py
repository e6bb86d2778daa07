"""CPU: the numpy restatement of the rasterisation rule (tests/raster_restate.py) held to properties that do not depend on it,
and the scenes of tests/raster_scenes.py held to the cases a wrong kernel fails: tests/test_hip_raster.py compares the device
against the restatement on these scenes, bit for bit, so both have to be worth comparing against."""
import numpy as np
import pytest

import raster_restate as R
import raster_scenes as S

F32 = np.float32


def raster(sc, **kw):
    return R.rasterize(sc["verts"], sc["faces"], sc["poses"], sc["intr"], sc["H"], sc["W"], sc["near"], return_counts=True, **kw)


# -------------------------------------------------------------------------------------------------------------------- properties
def test_closed_sphere_is_hit_an_even_number_of_times_and_has_no_hole():
    sc, e = S.scenes()["sphere"], S.expected("sphere")
    whole = e["drawn"].all(axis=1)
    assert whole.tolist() == [True, True, False]                  # the third camera is inside: faces behind and across its near plane
    for n in np.nonzero(whole)[0]:
        c = e["counts"][n]
        assert c.max() == 2 and ((c % 2) == 0).all() and (c > 0).sum() > 500
        cov = c > 0                                               # the silhouette of a sphere is convex: every row and column is one run
        for line in list(cov) + list(cov.T):
            at = np.nonzero(line)[0]
            assert len(at) == 0 or len(at) == at[-1] - at[0] + 1
    inside = e["counts"][2]
    assert 0 < e["drawn"][2].sum() < len(sc["faces"]) and inside.max() == 1 and (inside > 0).sum() > 1000


@pytest.mark.parametrize("variant", S.QUAD_VARIANTS)
def test_quad_on_pixel_centres_covers_each_pixel_once(variant):
    """a 16 x 16 quad with its corners exactly on pixel centres: the tie rule gives every centre on its outline and on its diagonal to
    exactly one triangle, and keeps exactly 16 x 16 of the 17 x 17 centres it touches"""
    v, f = S.quad(8.5, 8.5, 24.5, 24.5, 2.0, S.K64, *variant)
    e = R.rasterize(v, f, [S.IDENTITY], S.K64, 48, 64, return_counts=True)
    c = e["counts"][0]
    assert c.max() == 1 and c.sum() == 256 and e["on_edge"].sum() >= 16
    ys, xs = np.nonzero(c)
    assert xs.max() - xs.min() == 15 and ys.max() - ys.min() == 15
    assert sorted(e["face_hits"].tolist()) == [120, 136]          # the diagonal's 16 centres go to one of the two


def test_two_quads_sharing_an_edge_on_pixel_centres_tile_without_gap_or_overlap():
    e = S.expected("quad_centres")
    c = e["counts"][0]
    assert c.max() == 1 and c.sum() == 6 * 64
    ys, xs = np.nonzero(c)
    assert (xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) == (24, 16)


def test_fronto_parallel_plane_has_the_depth_bits_of_two():
    e = S.expected("quad_centres")
    hit = e["face_id"][0] >= 0
    assert hit.sum() == 384 and (e["depth"][0][hit].view(np.uint32) == F32(2).view(np.uint32)).all()
    assert np.isposinf(e["depth"][0][~hit]).all() and (e["bary"][0][~hit] == 0).all()
    b = e["bary"][0][hit].astype(np.float64)
    assert np.abs(b.sum(axis=1) - 1).max() < 3e-7 and b.min() >= 0


def test_barycentrics_interpolate_the_vertices_camera_depth():
    sc, e = S.scenes()["ties"], S.expected("ties")
    for n in range(2):
        z = R.project(sc["verts"], sc["poses"][n], R.intr4(sc["intr"], 2)[n], sc["near"])[0].astype(np.float64)
        hit = e["face_id"][n] >= 0
        corner = z[sc["faces"][e["face_id"][n][hit]]]
        interp = (e["bary"][n][hit].astype(np.float64) * corner).sum(axis=1)          # beta_i z_i = w_i / num, so the sum is |A| / num
        assert np.abs(interp / e["depth"][n][hit] - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------- the cases the scenes must hold
def test_scenes_hold_a_pixel_centre_on_a_shared_edge():
    for name in ("sphere", "quad_centres"):
        e = S.expected(name)
        assert e["on_edge"].sum() > 0
    e = S.expected("quad_centres")
    assert (e["on_edge"] & (e["counts"] == 1)).sum() > 100        # on an edge, and still taken exactly once


def test_scenes_hold_pixels_where_two_faces_tie_in_depth_bits():
    sc, e = S.scenes()["ties"], S.expected("ties")
    assert e["ties"][0].sum() > 100
    first = e["face_id"][0][e["ties"][0]]
    assert set(first.tolist()) == {0, 4}                          # the duplicated face and the coplanar pair: the lowest index of each
    assert not np.isin(e["face_id"][0], [1, 2, 3, 5])[e["ties"][0]].any() and not np.isin(e["face_id"][0], [1, 2, 3]).any()
    both = (e["face_id"][0] == 6).any() and (e["face_id"][0] == 7).any()          # the interpenetrating pair: each wins somewhere
    assert both and sc["faces"].shape[0] == 8


def test_rejects_drop_a_face_by_each_usable_clause_and_keep_their_neighbours():
    sc, e = S.scenes()["rejects"], S.expected("rejects")
    z, u, v, usable = R.project(sc["verts"], sc["poses"][0], R.intr4(sc["intr"], 2)[0], sc["near"])
    faces, n = sc["faces"].astype(np.int64), len(sc["verts"])
    in_range = ((faces >= 0) & (faces < n)).all(axis=1)
    assert (~in_range).sum() == 4 and not e["drawn"][0][~in_range].any()
    fv = np.where(in_range[:, None], faces, 0)
    with np.errstate(all="ignore"):
        clauses = dict(not_finite=~np.isfinite(z), below_near=np.isfinite(z) & (z < F32(sc["near"])), behind=z < 0,
                       u_beyond=np.isfinite(z) & (z >= F32(sc["near"])) & ~(np.abs(u) <= 65536) & (np.abs(v) <= 65536),
                       v_beyond=np.isfinite(z) & (z >= F32(sc["near"])) & (np.abs(u) <= 65536) & ~(np.abs(v) <= 65536),
                       u_overflows=np.isfinite(z) & (z >= F32(sc["near"])) & np.isinf(u), nan_z=np.isnan(z))
    for name, bad in clauses.items():
        dropped = in_range & bad[fv].any(axis=1)
        assert dropped.any() and not e["drawn"][0][dropped].any(), name
    at_near = usable & (z == F32(sc["near"]))
    just_below = z == np.nextafter(F32(sc["near"]), F32(0))
    assert e["drawn"][0][in_range & at_near[fv].any(axis=1)].any() and just_below.any() and not usable[just_below].any()
    assert e["face_hits"][0] > 0 and e["face_hits"][1] == 0       # the face at exactly near is drawn and seen; its neighbour is not
    # zero area (repeated vertices, collinear after the snap) and slivers that hold no pixel centre
    _, UV, A, _ = R.setup(sc["verts"], faces, sc["poses"][0], R.intr4(sc["intr"], 2)[0], sc["near"])
    ok = in_range & usable[fv].all(axis=1)
    assert (ok & (A == 0)).sum() >= 3
    won = np.bincount(e["face_id"][0][e["face_id"][0] >= 0], minlength=len(faces))
    sliver = e["drawn"][0] & (e["box_pixels"][0] > 0) & (won == 0)
    assert sliver.sum() >= 1 and (e["drawn"][0] & (e["box_pixels"][0] == 0)).sum() >= 6       # boxes without a centre, faces off the image
    assert e["drawn"][1].sum() > 0 and (e["drawn"][1] != e["drawn"][0]).any()


def test_rejects_clip_a_box_on_each_image_side():
    sc, e = S.scenes()["rejects"], S.expected("rejects")
    _, UV, A, _ = R.setup(sc["verts"], sc["faces"], sc["poses"][0], R.intr4(sc["intr"], 2)[0], sc["near"])
    H, W = sc["H"], sc["W"]
    sides = dict(left=0, right=0, top=0, bottom=0)
    for f in np.nonzero(e["drawn"][0] & (e["box_pixels"][0] > 0))[0]:
        sides["left"] += UV[f, :, 0].min() < 128 - 256
        sides["right"] += UV[f, :, 0].max() > 256 * W + 128
        sides["top"] += UV[f, :, 1].min() < 128 - 256
        sides["bottom"] += UV[f, :, 1].max() > 256 * H + 128
    assert all(v >= 1 for v in sides.values()), sides
    assert (e["face_id"][0][:, 0] >= 0).any() and (e["face_id"][0][:, -1] >= 0).any()
    assert (e["face_id"][0][0] >= 0).any() and (e["face_id"][0][-1] >= 0).any()


def test_sizes_straddle_the_lane_budget_and_every_box_side():
    sc, e = S.scenes()["sizes"], S.expected("sizes")
    budget = S.lane_pixels()
    px = e["box_pixels"][0]
    assert (px[px > 0] <= budget).sum() >= 5 and (px > budget).sum() >= 5 and (px == budget).any() and (px == budget + 1).any()
    _, UV, _, _ = R.setup(sc["verts"], sc["faces"], sc["poses"][0], R.intr4(sc["intr"], 1)[0], sc["near"])
    widths = {R.box(UV[f], sc["H"], sc["W"])[1] - R.box(UV[f], sc["H"], sc["W"])[0] + 1 for f in range(48)}
    assert widths == set(range(1, 49))
    heights = {R.box(UV[f], sc["H"], sc["W"])[3] - R.box(UV[f], sc["H"], sc["W"])[2] + 1 for f in range(48, 54)}
    assert heights == {1, 2, 16, 17, 33, 47}
    cover = len(sc["faces"]) - 1
    assert px[cover] == sc["H"] * sc["W"] and (e["counts"][0] >= 1).all()              # one face over the whole image
    won = set(np.unique(e["face_id"][0]).tolist())
    front = [f for f in range(48) if (f + 1) % 3 != 0]
    behind = [f for f in range(48) if (f + 1) % 3 == 0]
    assert cover in won and any(f in won for f in front) and not any(f in won for f in behind)
    assert e["face_hits"][behind].sum() == 0 and e["box_pixels"][0][behind].min() > 0


def test_one_pixel_image():
    e = S.expected("one_pixel")
    assert e["face_id"].tolist() == [[[0]]] and e["depth"].view(np.uint32).tolist() == [[[int(F32(2).view(np.uint32))]]]


def test_key_order_is_depth_then_face_index():
    """positive floats order like their bit patterns, so the 64-bit minimum is the nearest depth, then the lowest index"""
    z = np.array([1e-30, 0.5, np.nextafter(F32(2), F32(0)), 2.0, np.nextafter(F32(2), F32(3)), 3.4e38], F32)
    bits = z.view(np.uint32).astype(np.uint64)
    assert (np.diff(bits.astype(np.int64)) > 0).all()
    keys = (bits[:, None] << np.uint64(32)) | np.arange(3, dtype=np.uint64)[None, :]
    flat = [int(k) for k in keys.reshape(-1)]
    assert flat == sorted(set(flat)) and flat[-1] < int(R.EMPTY)


# ------------------------------------------------------------------------------------------------------ votes and the selection
def test_votes_scene_holds_the_image_borders_and_the_unusable():
    vs = S.votes_scene()
    seen, inside = R.mask_votes(vs["verts"], vs["poses"], vs["intr"], vs["masks"], vs["near"])
    z, u, v, usable = R.project(vs["verts"], vs["poses"][0], R.intr4(vs["intr"], 2)[0], vs["near"])
    one = R.mask_votes(vs["verts"], vs["poses"][:1], vs["intr"], vs["masks"][:1], vs["near"])[0]
    for value, axis, want in ((0.0, u, 1), (61.0, u, 0), (0.0, v, 1), (47.0, v, 0)):
        at = usable & (axis == F32(value)) & (u <= 61) & (v <= 47) & (u >= 0) & (v >= 0)
        at &= (u < 61) if axis is v else (v < 47)
        assert at.any() and (one[at] == want).all(), (value, want)
    assert (u == np.nextafter(F32(61), F32(0))).any() and (z < 0).any() and np.isnan(u).any() and (np.abs(u) > 65536).any()
    assert one[z < 0].sum() == 0 and one[~usable].sum() == 0
    assert (inside <= seen).all() and set(np.unique(seen).tolist()) == {0, 1, 2} and (inside == 2).any() and ((seen == 2) & (inside == 0)).any()


def test_the_library_s_torch_projection_is_the_restatement_s():
    """ls2fm._posed.project_torch, the one torch statement of the projection under the three *_torch forms, against R.project on
    the votes scene (the image borders and every unusable clause), view by view: the flags equal, camera z, u and v equal as
    bits (NaN by its pattern); then mask_votes_torch on CPU tensors against R.mask_votes"""
    import torch
    from ls2fm import _posed, raster
    vs = S.votes_scene()
    (H, W), n = vs["masks"].shape[1:], len(vs["poses"])
    bits = lambda a: np.asarray(a, F32).view(np.uint32)
    v = torch.from_numpy(vs["verts"])
    P = torch.from_numpy(np.asarray(vs["poses"], F32))
    K = torch.from_numpy(np.asarray(vs["intr"], F32)).reshape(-1, 3, 3).expand(n, 3, 3)
    for i in range(n):
        z, u, w, usable = R.project(vs["verts"], vs["poses"][i], R.intr4(vs["intr"], n)[i], vs["near"])
        with np.errstate(all="ignore"):
            in_image = usable & (u >= 0) & (u < W) & (w >= 0) & (w < H)
        assert usable.any() and (~usable).any() and in_image.any() and (usable & ~in_image).any()
        c, tu, tw, t_usable, ok, px, py = _posed.project_torch(P[i], K[i], v[:, 0], v[:, 1], v[:, 2], vs["near"], H, W)
        assert np.array_equal(t_usable.numpy(), usable) and np.array_equal(ok.numpy(), in_image)
        for got, want in ((c[2], z), (tu, u), (tw, w)):
            assert np.array_equal(bits(got.numpy()), bits(want))
        with np.errstate(all="ignore"):
            assert np.array_equal(px.numpy(), np.where(in_image, np.floor(u), 0).astype(np.int64))
            assert np.array_equal(py.numpy(), np.where(in_image, np.floor(w), 0).astype(np.int64))
    seen, inside = raster.mask_votes_torch(v, P, torch.from_numpy(np.asarray(vs["intr"], F32)), torch.from_numpy(vs["masks"]), vs["near"])
    want = R.mask_votes(vs["verts"], vs["poses"], vs["intr"], vs["masks"], vs["near"])
    assert np.array_equal(seen.numpy(), want[0]) and np.array_equal(inside.numpy(), want[1])


def test_dilation_is_a_max_pool():
    import torch
    m = (np.random.default_rng(2).uniform(size=(2, 13, 17)) < 0.08).astype(np.uint8)
    for d in (0, 1, 3):
        ref = torch.nn.functional.max_pool2d(torch.from_numpy(m)[:, None].float(), kernel_size=2 * d + 1, stride=1, padding=d)[:, 0] > 0
        assert np.array_equal(R.dilate(m, d), ref.numpy())


def test_clean_scene_keeps_the_outer_spheres_front_only():
    cs = S.clean_scene()
    keep, v, f = R.clean_mesh(cs["verts"], cs["faces"], cs["poses"], cs["intr"], cs["masks"])
    outer = S.CLEAN_OUTER_FACES
    assert 50 < keep.sum() and not keep[outer:].any()             # neither the floater nor the inner sphere
    hits = R.rasterize(cs["verts"], cs["faces"], cs["poses"], cs["intr"], 48, 64)["face_hits"]
    assert (hits[keep] >= 1).all() and hits[outer + S.CLEAN_FLOATER_FACES:].sum() == 0 and hits[outer:outer + S.CLEAN_FLOATER_FACES].sum() > 0      # the floater is seen, the inner sphere never
    assert f.max() == len(v) - 1 and len(f) == keep.sum() and len(np.unique(f)) == len(v)
    assert np.array_equal(v[f], cs["verts"][cs["faces"][keep]])
    no_vis = R.clean_mesh(cs["verts"], cs["faces"], cs["poses"], cs["intr"], cs["masks"], visibility=False)[0]
    assert no_vis[outer + S.CLEAN_FLOATER_FACES:].any() and not no_vis[outer:outer + S.CLEAN_FLOATER_FACES].any() and (keep <= no_vis).all()
    wide = R.clean_mesh(cs["verts"], cs["faces"], cs["poses"], cs["intr"], cs["masks"], dilate_px=2)[0]
    lax = R.clean_mesh(cs["verts"], cs["faces"], cs["poses"], cs["intr"], cs["masks"], max_outside=1)[0]
    assert (keep <= wide).all() and wide.sum() > keep.sum() and (keep <= lax).all() and lax.sum() > keep.sum()
    unmasked = R.clean_mesh(cs["verts"], cs["faces"], cs["poses"], cs["intr"], None, H=48, W=64)[0]
    assert unmasked[outer:outer + S.CLEAN_FLOATER_FACES].any() and not unmasked[outer + S.CLEAN_FLOATER_FACES:].any()
