"""CPU: ls2fm.cloud_mesh's torch form (_implicit_torch, the route of CPU tensors) against the numpy restatement
(tests/cloud_mesh_restate.py) by the bits of value and support on every lattice point of every scene of tests/cloud_mesh_scenes.py;
the properties of the rule itself, measured on the restatement; the refusals of the module and of the C entry point; the new
symbols; and cloud.depths_to_cloud against the rasteriser's projection."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cloud_mesh_restate as CR
import cloud_mesh_scenes as S
import cloud_scenes as CS
from ls2fm import _lib, _posed, cloud, cloud_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ls2fm_cloud_implicit", "ls2fm_cloud_implicit_plan")


def torch_form(sc, k=S.K, min_neighbors=S.MIN_NEIGHBORS):
    v, s = cloud_mesh._implicit_torch(torch.as_tensor(sc["points"]), torch.as_tensor(sc["normals"]), sc["shape"], sc["origin"], sc["voxel"],
                                      sc["radius"], k, min_neighbors, chunk=5000)
    return v.numpy(), s.numpy()


# ------------------------------------------------------------------------------------------------- the torch form, by bits
@pytest.mark.parametrize("name", S.NAMES)
def test_implicit_torch_equals_restatement_on_every_lattice_point(name):
    sc = S.scene(name)
    value, support = torch_form(sc)
    exp = S.expected(name)
    assert value.shape == sc["shape"] and CR.same_bits(value, exp[0]) and CR.same_bits(support, exp[1])
    if name in ("duplicates", "few"):                                                  # another capacity, another threshold
        for k, least in ((9, 1), (32, 32)):
            got, exp = torch_form(sc, k, least), S.expected(name, k, least)
            assert CR.same_bits(got[0], exp[0]) and CR.same_bits(got[1], exp[1])


def test_the_public_route_of_cpu_tensors_and_its_filter():
    """implicit_from_cloud on CPU tensors: default bounds (the box grown by the radius), the lattice of fusion.volume_for, and
    points with a non-finite coordinate or normal dropped first"""
    sc = S.scene("duplicates")
    p, n = torch.as_tensor(sc["points"]), torch.as_tensor(sc["normals"])
    vol = cloud_mesh.implicit_from_cloud(p, n, sc["voxel"])
    lo, hi = sc["points"].min(axis=0).astype(np.float64) - 3 * sc["voxel"], sc["points"].max(axis=0).astype(np.float64) + 3 * sc["voxel"]
    shape = tuple(max(2, int(np.ceil((h - l) / sc["voxel"])) + 1) for l, h in zip(lo, hi))
    assert vol.shape == shape and vol.origin == tuple(lo) and vol.radius == 3 * sc["voxel"] and vol.voxel == sc["voxel"]
    exp = CR.implicit(sc["points"], sc["normals"], shape, lo, sc["voxel"], 3 * sc["voxel"], 16, 3)
    assert CR.same_bits(vol.value.numpy(), exp[0]) and CR.same_bits(vol.support.numpy(), exp[1])
    bad_p, bad_n = torch.cat([p, p[:3]]), torch.cat([n, n[:3]])
    bad_p[-1, 1], bad_n[-2, 0], bad_n[-3, 2] = float("inf"), float("nan"), float("-inf")
    again = cloud_mesh.implicit_from_cloud(bad_p, bad_n, sc["voxel"], bounds=(lo, hi))
    assert CR.same_bits(again.value.numpy(), exp[0]) and CR.same_bits(again.support.numpy(), exp[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_mesh.extract(vol)                                                       # marching cubes has no CPU path


# ------------------------------------------------------------------------------------------------------ the rule's properties
def test_the_plane_reproduces_the_signed_distance():
    """Every s_j is X.z - c exactly (dyadic heights, normal (0, 0, 1)), so num = sum w_j s and den = sum w_j differ from s den
    and den only by the roundings of their n - 1 adds and n products: num / den is within (n + 2) 2^-53 of s, relative, in fp64
    before the final rounding.  Exact equality does not follow: the two sums round separately."""
    sc = S.scene("plane")
    X = CR.lattice_points(sc["shape"], sc["origin"], sc["voxel"])
    num, den, n = CR.sums(sc["points"], sc["normals"], X, CS.prefix(S.lists("plane"), S.K), sc["radius"])
    ok = (n >= S.MIN_NEIGHBORS) & (den > 0)
    s = X[:, 2].astype(np.float64) - S.PLANE_HEIGHT
    assert ok.sum() > 3000 and (s[ok] != 0).all()
    err = np.abs(num[ok] / den[ok] - s[ok]) / np.abs(s[ok])
    print(f"plane: worst relative error {err.max():.3e} over {ok.sum()} defined lattice points")
    assert (err <= (n[ok] + 2) * 2.0 ** -53).all()
    value = S.expected("plane")[0].reshape(-1)
    assert np.array_equal(value[ok], s[ok].astype(np.float32)) and np.isnan(value[~ok]).all()


@pytest.mark.parametrize("name", S.SURFACES)
def test_every_zero_crossing_lies_within_half_a_voxel_of_the_surface(name):
    """The restatement at the scenes' lattices, radius 3 voxels, k = 16: the distance from the true surface of every zero crossing
    between two defined lattice neighbours.  Measured here (worst, mean, in voxels): sphere 0.031, 0.025; cube 0.449 (at its
    edges), 0.015; plane 0, 0; sheets 0, 0 (each sheet keeps its surface, exactly 1.000 voxel from the midplane); hemisphere 0.445
    (below its rim, against the full sphere), 0.078.  The cap of 0.5 voxel is a condition on the rule."""
    sc = S.scene(name)
    c = CR.crossings(S.expected(name)[0], sc["origin"], sc["voxel"])
    d = sc["distance"](c) / sc["voxel"]
    print(f"{name}: {len(c)} crossings, worst {d.max():.4f} voxel, mean {d.mean():.4f}")
    assert len(c) >= 500 and d.max() <= 0.5
    if name == "sheets":
        assert np.array_equal(np.abs(c[:, 2] - S.SHEET_MID), np.full(len(c), sc["voxel"]))


def test_the_spheres_crossing_count_does_not_depend_on_k():
    """No lattice point lies within SPHERE_MARGIN = 0.06 voxel of the sphere, and the rule's crossings stay nearer to it than that
    at k = 8, 16 and 32 (measured: 0.017, 0.031, 0.057): the sign at every lattice point is the true one, the count one number."""
    sc = S.scene("sphere")
    X = CR.lattice_points(sc["shape"], sc["origin"], sc["voxel"]).astype(np.float64)
    assert (sc["distance"](X) / sc["voxel"]).min() >= S.SPHERE_MARGIN
    counts = []
    for k in (8, 16, 32):
        c = CR.crossings(S.expected("sphere", k)[0], sc["origin"], sc["voxel"])
        assert (sc["distance"](c) / sc["voxel"]).max() < S.SPHERE_MARGIN
        counts.append(len(c))
    assert counts[0] == counts[1] == counts[2] == 1248


def test_the_small_scenes_hold_what_they_name():
    value, support = S.expected("few")
    assert np.isnan(value).all() and (support > 0).sum() > 100
    assert np.isfinite(S.expected("few", S.K, 1)[0]).sum() == (support > 0).sum()
    value, support = S.expected("empty")
    assert np.isnan(value).all() and (support == 0).all()
    idx = S.lists("duplicates")[0]
    assert ((idx[:, :2] >= 600).any(axis=1) & (S.lists("duplicates")[1][:, 0] == S.lists("duplicates")[1][:, 1])).any()   # twins tie on d2


# ---------------------------------------------------------------------------------------------------------- depths_to_cloud
def test_depths_to_cloud_inverts_the_projection():
    """its points pushed through _posed.project_torch land within 1e-3 px of (px + 0.5, py + 0.5) and their c_z equals the depth
    to fp32 rounding: within 16 ulp of the largest term of the camera-z sum, |R row| |X| + |t|"""
    rng = np.random.default_rng(7)
    V, H, W = 3, 11, 14
    depth = torch.as_tensor(rng.uniform(1.5, 4.0, (V, H, W)).astype(np.float32))
    depth[0, 0, 0], depth[0, 1, 2], depth[1, 3, 3], depth[2, 4, 5], depth[2, 10, 13] = float("nan"), float("inf"), 0.0, -1.0, 9.0
    poses = []
    for v in range(V):
        w = rng.normal(size=3) * 0.4
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
        poses.append(np.concatenate([R, rng.normal(size=(3, 1))], axis=1))
    pose = torch.as_tensor(np.array(poses, np.float32))
    intr = torch.tensor([[20.0, 0.0, 7.3], [0.0, 19.0, 5.1], [0.0, 0.0, 1.0]])
    for stride in (1, 3):
        pts, centers = cloud.depths_to_cloud(depth, pose, intr, stride=stride, max_depth=8.0)
        sub = depth[:, ::stride, ::stride]
        ok = torch.isfinite(sub) & (sub > 0) & (sub <= 8.0)
        assert pts.dtype == centers.dtype == torch.float32 and pts.shape == centers.shape == (int(ok.sum()), 3)
        assert int(ok.sum()) == ok.numel() - (5 if stride == 1 else 2)               # stride 3 meets the NaN and the zero only
        at = 0
        for v in range(V):
            py, px = torch.nonzero(ok[v], as_tuple=True)
            m = len(py)
            X = pts[at:at + m]
            c, u, w_, usable, inside, _, _ = _posed.project_torch(pose[v], intr, X[:, 0], X[:, 1], X[:, 2], 1e-3, H, W)
            assert bool(inside.all())
            assert float((u - (px * stride + 0.5)).abs().max()) < 1e-3 and float((w_ - (py * stride + 0.5)).abs().max()) < 1e-3
            scale = pose[v, 2, :3].abs() @ X.abs().T + pose[v, 2, 3].abs()
            assert bool(((c[2] - sub[v][py, px]).abs() <= 16 * 2.0 ** -24 * scale).all())
            centre = -(pose[v, :, :3].double().T @ pose[v, :, 3].double())
            assert torch.equal(centers[at:at + m], centre.float()[None].expand(m, 3))
            at += m
        assert at == len(pts)
    one, _ = cloud.depths_to_cloud(depth[0], pose[0], intr)
    assert torch.equal(one, cloud.depths_to_cloud(depth[:1], pose[:1], intr[None])[0])
    with pytest.raises(ValueError, match="stride"):
        cloud.depths_to_cloud(depth, pose, intr, stride=0)
    with pytest.raises(ValueError, match="poses"):
        cloud.depths_to_cloud(depth, pose[:2], intr)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_module():
    sc = S.scene("few")
    p, n = torch.as_tensor(sc["points"]), torch.as_tensor(sc["normals"])
    for kw, match in ((dict(voxel=0.0), "voxel"), (dict(voxel=float("inf")), "voxel"), (dict(voxel=0.1, radius=0.0), "radius"),
                      (dict(voxel=0.1, radius=float("inf")), "radius"), (dict(voxel=0.1, radius=float("nan")), "max_dist"),
                      (dict(voxel=0.1, k=0), "k "), (dict(voxel=0.1, k=33), "k "), (dict(voxel=0.1, min_neighbors=0), "min_neighbors"),
                      (dict(voxel=0.1, min_neighbors=2.5), "min_neighbors"), (dict(voxel=1e-6), "lattice"),
                      (dict(voxel=0.1, bounds=((0, 0, 0), (1, float("nan"), 1))), "bounds")):
        with pytest.raises(ValueError, match=match):
            cloud_mesh.implicit_from_cloud(p, n, **kw)
    with pytest.raises(ValueError, match="normals"):
        cloud_mesh.implicit_from_cloud(p, n[:1], 0.1)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        cloud_mesh.implicit_from_cloud(p[:, :2], n, 0.1)
    with pytest.raises(ValueError, match="give bounds"):
        cloud_mesh.implicit_from_cloud(p[:0], n[:0], 0.1)
    with pytest.raises(ValueError, match="toward is required"):
        cloud_mesh.mesh_from_cloud(p, voxel=0.1)
    with pytest.raises(ValueError, match="voxel"):
        cloud_mesh.mesh_from_cloud(p, n)


def test_symbols_and_the_library_refusals():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    lib = _lib.load()
    declared = set(re.findall(r"\b(ls2fm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    abi = int(re.search(r"#define\s+LS2FM_ABI_VERSION\s+(\d+)", header).group(1))
    assert abi == 13 and lib.ls2fm_abi_version() == _lib.ABI_VERSION == abi
    assert "THE IMPLICIT RULE" in header
    macro = lambda name: int(re.search(rf"#define\s+LS2FM_CLOUD_IMPLICIT_{name}\s+(\d+)", header).group(1))      # noqa: E731
    assert tuple(tuple(macro(f"BRICK{b}_{a}") for a in "XYZ") for b in (0, 1)) == cloud_mesh.BRICKS
    assert cloud_mesh.DEFAULT_PLAN == dict(brick=macro("BRICK"), empty_test=bool(macro("EMPTY_TEST")))
    # refused before anything is enqueued: no device is needed to see it (NULL arrays and sizes only)
    origin, dim = (ctypes.c_float * 3)(0.0, 0.0, 0.0), (ctypes.c_int32 * 3)(2, 2, 2)
    nan3 = (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
    good = dict(n=5, origin=origin, h=1.0, inv_h=1.0, dim=dim, shape=(4, 4, 4), lat=origin, voxel=0.5, k=8, max_d2=1.0, least=3)

    def call(plan=None, **kw):
        a = dict(good, **kw)
        head = (None, None, a["n"], None, None, a["origin"], a["h"], a["inv_h"], a["dim"], *a["shape"], a["lat"], a["voxel"], a["k"],
                a["max_d2"], a["least"])
        if plan is None:
            return lib.ls2fm_cloud_implicit(*head, None, None, None)
        return lib.ls2fm_cloud_implicit_plan(*head, *plan, None, None, None)

    for kw in (dict(), dict(n=-1), dict(n=2 ** 31), dict(shape=(0, 4, 4)), dict(shape=(4, -1, 4)), dict(shape=(2048, 1024, 1024)),
               dict(shape=(2 ** 24 + 1, 1, 1)), dict(voxel=0.0), dict(voxel=float("inf")), dict(voxel=float("nan")), dict(lat=nan3),
               dict(lat=None), dict(k=0), dict(k=33), dict(max_d2=0.0), dict(max_d2=float("inf")), dict(max_d2=float("nan")),
               dict(max_d2=-1.0), dict(least=0), dict(h=0.0), dict(origin=nan3), dict(dim=(ctypes.c_int32 * 3)(2, 0, 2)), dict(n=0)):
        assert call(**kw) == -1, kw                                                   # the first and the last: NULL arrays
    for plan in ((2, 0), (-1, 1), (0, 2)):
        assert call(plan) == -1, plan
