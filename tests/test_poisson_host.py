"""CPU: ls2fm.cloud_mesh's torch form of THE POISSON RULE (_poisson_torch, the route of CPU tensors) against the numpy restatement
(tests/poisson_restate.py) by the bits of chi and of the density on every lattice point of every scene of tests/poisson_scenes.py;
the properties of the rule itself, measured on the restatement, among them the crossings against numpy.linalg.solve on the
assembled fp64 matrix; the refusals of the module and of every C entry point; the new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cloud_mesh_restate as CR
import poisson_restate as PR
import poisson_scenes as S
from ls2fm import _lib, cloud_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ls2fm_poisson_workspace_bytes", "ls2fm_poisson_solve", "ls2fm_poisson_solve_plan", "ls2fm_poisson_splat",
       "ls2fm_poisson_sweep_colour", "ls2fm_poisson_restrict", "ls2fm_poisson_prolong")


# ------------------------------------------------------------------------------------------------- the torch form, by bits
@pytest.mark.parametrize("name", S.NAMES)
def test_poisson_torch_equals_restatement_on_every_lattice_point(name):
    sc = S.scene(name)
    value, density = cloud_mesh._poisson_torch(torch.as_tensor(sc["points"]), torch.as_tensor(sc["normals"]), *S.lattice_of(sc))
    exp = S.expected(name)
    assert tuple(value.shape) == sc["shape"] and CR.same_bits(value.numpy(), exp[0]) and CR.same_bits(density.numpy(), exp[1])
    assert np.isfinite(exp[0]).all()
    if name in ("crowded", "last_cell"):                                              # a V-cycle, another screen, fewer cycles
        got = cloud_mesh._poisson_torch(torch.as_tensor(sc["points"]), torch.as_tensor(sc["normals"]), *S.lattice_of(sc), 0.25, 2, 1)
        exp = S.expected(name, 0.25, 2, 1)
        assert CR.same_bits(got[0].numpy(), exp[0]) and CR.same_bits(got[1].numpy(), exp[1])


def test_the_stages_of_the_torch_form_by_bits():
    """each stage on a lattice with even and odd sides, at s = 1 and s = 1 / 16"""
    rng = np.random.default_rng(4)
    shape = (9, 6, 8)
    chi, b = rng.normal(size=shape).astype(np.float32), rng.normal(size=shape).astype(np.float32)
    W = np.maximum(rng.normal(size=shape), 0).astype(np.float32)
    t = torch.as_tensor
    for s in (1.0, 1.0 / 16.0):
        for colour in (0, 1):
            assert CR.same_bits(cloud_mesh._sweep_colour_torch(t(chi), t(b), t(W), s, 4.0, colour).numpy(), PR.sweep_colour(chi, b, W, s, 4.0, colour))
        assert CR.same_bits(cloud_mesh._residual_torch(t(chi), t(b), t(W), s, 0.25).numpy(), PR.residual(chi, b, W, s, 0.25))
    assert CR.same_bits(cloud_mesh._restrict_torch(t(chi)).numpy(), PR.restrict(chi))
    e = rng.normal(size=(5, 3, 4)).astype(np.float32)
    assert CR.same_bits(cloud_mesh._prolong_torch(t(e), shape).numpy(), PR.prolong(e, shape))
    assert cloud_mesh.poisson_levels((32, 32, 35)) == PR.level_shapes((32, 32, 35)) == [(32, 32, 35), (16, 16, 18), (8, 8, 9), (4, 4, 5), (2, 2, 3)]
    assert PR.level_shapes((4, 4, 4)) == [(4, 4, 4)] and PR.level_shapes((3, 9, 9)) == [(3, 9, 9)] and len(PR.level_shapes((5, 4, 4))) == 2


def test_the_transfers_are_transposes_up_to_the_halving():
    """R = P^T / 8 away from rounding: <R r, e> = <r, P e> / 8 on dyadic data, exactly, at even and odd sides"""
    rng = np.random.default_rng(6)
    for shape in ((8, 7, 6), (5, 4, 9), (2, 2, 3)):
        coarse = tuple((n + 1) // 2 for n in shape)
        r = rng.integers(-64, 65, shape).astype(np.float32)
        e = rng.integers(-64, 65, coarse).astype(np.float32)
        lhs = (PR.restrict(r).astype(np.float64) * e).sum()
        rhs = (r.astype(np.float64) * PR.prolong(e, shape)).sum() / 8.0
        assert lhs == rhs, shape


def test_the_public_route_of_cpu_tensors_and_its_filter():
    sc = S.scene("crowded")
    p, n = torch.as_tensor(sc["points"]), torch.as_tensor(sc["normals"])
    lo, hi = sc["origin"], tuple(o + (s - 1) * sc["voxel"] for o, s in zip(sc["origin"], sc["shape"]))
    kept = cloud_mesh._oriented(p, n, "test")
    exp = PR.solve(kept[0].numpy(), kept[1].numpy(), *S.lattice_of(sc), 4.0, 2, 2)
    vol = cloud_mesh.poisson_from_cloud(p, n, sc["voxel"], cycles=2, bounds=(lo, hi))
    assert vol.shape == sc["shape"] and vol.origin == sc["origin"] and vol.voxel == sc["voxel"] and vol.screen == 4.0
    assert CR.same_bits(vol.value.numpy(), exp[0]) and CR.same_bits(vol.support.numpy(), exp[1])
    bad_p, bad_n = torch.cat([p, p[:4]]), torch.cat([n * 0.3, n[:4]])
    bad_p[-1, 1], bad_n[-2, 0], bad_n[-3], bad_n[-4, 2] = float("inf"), float("nan"), 0.0, float("-inf")
    scaled = cloud_mesh._oriented(p, n * 0.3, "test")
    again = cloud_mesh.poisson_from_cloud(bad_p, bad_n, sc["voxel"], cycles=2, bounds=(lo, hi))
    exp = PR.solve(scaled[0].numpy(), scaled[1].numpy(), *S.lattice_of(sc), 4.0, 2, 2)
    assert CR.same_bits(again.value.numpy(), exp[0]) and CR.same_bits(again.support.numpy(), exp[1])
    b, W = PR.system(scaled[0].numpy(), scaled[1].numpy(), *S.lattice_of(sc))
    figure = cloud_mesh.poisson_residual(again, bad_p, bad_n)
    assert 0 < figure < 1 and abs(figure - PR.relative_residual(exp[0], b, W, 4.0)) <= 1e-6 * figure
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_mesh.extract(vol)                                                       # marching cubes has no CPU path


# ------------------------------------------------------------------------------------------------------ the rule's properties
def _magnitudes(chi, b, W, V, screen):
    """per lattice point, the sum of the absolute terms of r_i (m_r) and of b_i (m_b): each fp32 rounding in them is at most
    2^-24 of it"""
    absN = PR.neighbour_sum(np.abs(chi))[0].astype(np.float64)
    deg = PR.neighbour_sum(chi)[1].astype(np.float64)
    m_r = np.abs(b).astype(np.float64) + deg * np.abs(chi) + absN + screen * W.astype(np.float64) * np.abs(chi)
    m_b = np.zeros(chi.shape)
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        g = 0.5 * (np.abs(V[a][tuple(lo)]).astype(np.float64) + np.abs(V[a][tuple(hi)]))
        m_b[tuple(lo)] += g
        m_b[tuple(hi)] += g
    return m_r, m_b


@pytest.mark.parametrize("name", ["sphere", "capped", "plane", "crowded"])
def test_the_weighted_sum_of_chi_vanishes_to_rounding(name):
    """Summing the equations, every edge target enters two of them with opposite signs and every neighbour term cancels:
    sum b = 0 and screen sum W chi = sum b - sum r, for ANY chi, up to the fp32 roundings inside b_i and r_i.

    The identity, held to its rounding error.  r_i is 12 rounded operations (5 adds of N, deg chi, the difference, s ., a W, . chi,
    the sum, b - .), b_i is 5 (three differences, two adds; the edge targets themselves enter both of their equations with the
    same bits and cancel).  Each rounding is at most 2^-24 of m_i, the sum of the absolute terms of its expression, and they are
    independent and of either sign, so the fp64 sum over the lattice has a standard deviation of at most 2^-24 sqrt(k sum m_i^2 /
    3), k roundings per point.  The test allows 6 of them.  (Measured: the two sides differ by 3e-4 of 0.17 on the sphere; the
    bound is about 1e-3 there.  A flipped sign of the screening term would show as twice the left side.)

    The property, held to what the issue allows the cycles: a shift of chi by a constant d moves sum W chi by d sum W, so
    |sum W chi| / sum W |chi| is the offset of the zero level at the samples in units of the typical |chi| there, and |chi| at a
    sample is what chi gains over the fraction of a voxel between the sample and the zero level.  The issue holds 8 cycles to
    0.02 voxel from the exact zero level; an offset of 1e-3 of that scale is a twentieth of it.  Bound: 1e-3."""
    V, W, b = S.system(name)
    chi = S.expected(name)[0]
    r = PR.residual(chi, b, W, 1.0, S.SCREEN).astype(np.float64)
    m_r, m_b = _magnitudes(chi, b, W, V, S.SCREEN)
    sigma_b = 2.0 ** -24 * np.sqrt(5 * (m_b ** 2).sum() / 3)
    sigma_r = 2.0 ** -24 * np.sqrt(12 * (m_r ** 2).sum() / 3)
    sum_b, lhs = b.astype(np.float64).sum(), S.SCREEN * (W.astype(np.float64) * chi).sum()
    weighted, scale = (W.astype(np.float64) * chi).sum(), (W.astype(np.float64) * np.abs(chi)).sum()
    print(f"{name}: sum b {sum_b:.3e} (6 sigma {6 * sigma_b:.3e}); screen sum W chi {lhs:.6e}, sum b - sum r {sum_b - r.sum():.6e}, "
          f"apart {abs(lhs - (sum_b - r.sum())):.3e} (6 sigma {6 * np.hypot(sigma_b, sigma_r):.3e}); |sum W chi| / sum W |chi| {abs(weighted) / scale:.3e}")
    assert abs(sum_b) <= 6 * sigma_b
    assert abs(lhs - (sum_b - r.sum())) <= 6 * np.hypot(sigma_b, sigma_r)
    assert abs(lhs) > 20 * np.hypot(sigma_b, sigma_r)                                  # the identity is held far below what it relates
    assert abs(weighted) <= 1e-3 * scale


def test_the_spheres_crossings_lie_within_half_a_voxel():
    """measured: worst 0.120 voxel, the figure of the issue's prototype (0.08 - 0.13)"""
    sc = S.scene("sphere")
    c = CR.crossings(S.expected("sphere")[0], sc["origin"], sc["voxel"])
    d = sc["distance"](c) / sc["voxel"]
    print(f"sphere: {len(c)} crossings, worst {d.max():.4f} voxel, mean {d.mean():.4f}")
    assert len(c) >= 1000 and d.max() <= 0.5


def rim_edges(value):
    """The number of lattice edges where a zero level extracted cube by cube ends: edges with a sign change between two defined
    ends of which not all four surrounding lattice cubes exist with eight defined corners.  Marching cubes emits faces in exactly
    those cubes, and the vertex on an edge is interior to the mesh when all four around it do; an edge on the boundary of the box
    has fewer than four cubes and counts.  A field whose count is 0 has a closed zero level."""
    v = np.asarray(value, np.float64)
    defined = np.isfinite(v)
    cube = np.ones(tuple(n - 1 for n in v.shape), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cube &= defined[dx:v.shape[0] - 1 + dx, dy:v.shape[1] - 1 + dy, dz:v.shape[2] - 1 + dz]
    count = 0
    for a in range(3):
        others = [x for x in range(3) if x != a]
        padded = np.pad(cube, [(0, 0) if x == a else (1, 1) for x in range(3)], constant_values=False)
        around = np.ones(tuple(v.shape[x] - (1 if x == a else 0) for x in range(3)), bool)       # one entry per edge along a
        for d0 in (0, 1):
            for d1 in (0, 1):
                idx = [slice(None)] * 3
                idx[others[0]], idx[others[1]] = slice(d0, d0 + v.shape[others[0]]), slice(d1, d1 + v.shape[others[1]])
                around &= padded[tuple(idx)]
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        p, q = v[tuple(lo)], v[tuple(hi)]
        with np.errstate(invalid="ignore"):
            crossing = np.isfinite(p) & np.isfinite(q) & ((p < 0) != (q < 0))
        count += int((crossing & ~around).sum())
    return count


def test_the_capped_sphere_closes_and_the_local_surface_does_not():
    """No sign change of chi lies on an edge that lacks one of its four lattice cubes (rim_edges; it would on the boundary of the
    box, the only place a field defined everywhere can have one), so its zero level is closed, and its crossings over the hole
    stay within 1 voxel of the sphere (measured: worst 0.386).  THE IMPLICIT RULE on the same cloud is undefined over the hole:
    its zero level ends in a rim there.  rim_edges is itself checked on a plane that leaves the box."""
    sc = S.scene("capped")
    chi = S.expected("capped")[0]
    assert np.isfinite(chi).all() and rim_edges(chi) == 0
    assert rim_edges(S.expected("plane")[0]) > 50                                      # a surface that leaves the box is not closed
    shell = np.ones(chi.shape, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert (chi[shell] > 0).all() and (chi < 0).sum() > 1000
    c = CR.crossings(chi, sc["origin"], sc["voxel"])
    d = sc["distance"](c) / sc["voxel"]
    over_hole = (c[:, 2] - S.SPHERE_CENTRE[2]) / S.SPHERE_RADIUS > S.CAP
    print(f"capped: {len(c)} crossings, {over_hole.sum()} over the hole, worst {d.max():.4f} voxel, over the hole {d[over_hole].max():.4f}")
    assert over_hole.sum() > 50 and d.max() <= 1.0
    local = CR.implicit(sc["points"], sc["normals"], *S.lattice_of(sc), 3 * sc["voxel"], 16, 3)[0]
    assert np.isnan(local).any() and rim_edges(local) > 20


def test_eight_cycles_against_the_solved_matrix():
    """12 x 13 x 16: the crossings after 8 default cycles against those of numpy.linalg.solve on the assembled fp64 matrix of the
    same equations (the same fp32 b and W): the same lattice edges cross, and each crossing lies within 0.02 voxel of its
    counterpart (measured: see the print; the issue's prototype had 0.005 at 32^3)."""
    sc = S.small((12, 13, 16), strays=0)
    b, W = PR.system(sc["points"], sc["normals"], *S.lattice_of(sc))
    chi = PR.solve_lattice(b, W, S.SCREEN, S.CYCLES, S.GAMMA)
    A, rhs = PR.assemble(b, W, S.SCREEN)
    exact = np.linalg.solve(A, rhs).reshape(b.shape)
    assert np.abs(A @ exact.reshape(-1) - rhs).max() <= 1e-12 * np.abs(rhs).max()
    got, ref = CR.crossings(chi, sc["origin"], sc["voxel"]), CR.crossings(exact, sc["origin"], sc["voxel"])
    assert len(got) > 150 and len(ref) > 150
    apart = np.linalg.norm(got[:, None] - ref[None], axis=2) / sc["voxel"]           # each crossing and its nearest counterpart, both ways
    d = np.maximum(apart.min(axis=1).max(), apart.min(axis=0).max()).reshape(1)
    print(f"12 x 13 x 16: {len(got)} crossings, worst {d.max():.5f} voxel from the solved matrix's, max |chi - exact| "
          f"{np.abs(chi - exact).max():.3e} of {np.abs(exact).max():.3e}")
    assert d.max() <= 0.02
    assert sc["distance"](ref).max() / sc["voxel"] <= 0.5


def test_residual_contraction_per_cycle_is_recorded():
    """max |r| after a cycle over max |r| before it, per scene (DESIGN 3.26 keeps the table).  Not bounded at gamma = 2: on the
    scenes with little data the residual reaches its fp32 floor within the 8 cycles and the ratio there is noise ('two': 0.75)."""
    for gamma in (2, 1):
        for name in ("sphere", "capped", "hemisphere", "plane", "crowded", "two"):
            _, W, b = S.system(name)
            history = []
            PR.solve_lattice(b, W, S.SCREEN, 5, gamma, history)
            h = np.array(history)
            print(f"gamma {gamma} {name}: " + " ".join(f"{x:.3f}" for x in h[1:] / h[:-1]))
            assert h[-1] < h[0]


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_module():
    sc = S.scene("two")
    p, n = torch.as_tensor(sc["points"]), torch.as_tensor(sc["normals"])
    for kw, match in ((dict(voxel=0.0), "voxel"), (dict(voxel=float("inf")), "voxel"), (dict(voxel=0.1, screen=0.0), "screen"),
                      (dict(voxel=0.1, screen=float("inf")), "screen"), (dict(voxel=0.1, screen=float("nan")), "screen"),
                      (dict(voxel=0.1, screen=1e-60), "screen"), (dict(voxel=0.1, cycles=-1), "cycles"), (dict(voxel=0.1, cycles=2.5), "cycles"),
                      (dict(voxel=0.1, gamma=0), "gamma"), (dict(voxel=0.1, gamma=3), "gamma"), (dict(voxel=1e-6), "lattice"),
                      (dict(voxel=0.1, bounds=((0, 0, 0), (1, float("nan"), 1))), "bounds")):
        with pytest.raises(ValueError, match=match):
            cloud_mesh.poisson_from_cloud(p, n, **kw)
    with pytest.raises(ValueError, match="normals"):
        cloud_mesh.poisson_from_cloud(p, n[:1], 0.1)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        cloud_mesh.poisson_from_cloud(p[:, :2], n, 0.1)
    with pytest.raises(ValueError, match="give bounds"):
        cloud_mesh.poisson_from_cloud(p, n * 0.0, 0.1)
    with pytest.raises(ValueError, match="method"):
        cloud_mesh.mesh_from_cloud(p, n, voxel=0.1, method="ball-pivoting")
    for kw in (dict(radius=0.3), dict(k=8), dict(min_neighbors=2)):                    # the local surface's options
        with pytest.raises(ValueError, match="takes screen, cycles, gamma and bounds"):
            cloud_mesh.mesh_from_cloud(p, n, voxel=0.1, method="poisson", **kw)
    with pytest.raises(ValueError, match="trim"):
        cloud_mesh.mesh_from_cloud(p, n, voxel=0.1, method="poisson", trim=-1.0)
    with pytest.raises(ValueError, match="Poisson lattice"):
        cloud_mesh._poisson_torch(p, n, (1, 4, 4), (0, 0, 0), 0.1)


def test_symbols_and_the_library_refusals():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    lib = _lib.load()
    declared = set(re.findall(r"\b(ls2fm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    abi = int(re.search(r"#define\s+LS2FM_ABI_VERSION\s+(\d+)", header).group(1))
    assert abi == 13 and lib.ls2fm_abi_version() == _lib.ABI_VERSION == abi
    assert "THE POISSON RULE" in header
    macro = lambda name: int(re.search(rf"#define\s+LS2FM_POISSON_{name}\s+(\d+)", header).group(1))      # noqa: E731
    assert tuple(macro(f"BRICK_{a}") for a in "XYZ") == cloud_mesh.POISSON_BRICK and macro("TAIL_POINTS") == cloud_mesh.POISSON_TAIL_POINTS
    # the workspace: 32 bytes a lattice point (or the coarse levels, if they need more) and b of level 0, in 256-byte pieces
    assert lib.ls2fm_poisson_workspace_bytes(16, 16, 16) == 4096 * 32 + 4096 * 4
    assert lib.ls2fm_poisson_workspace_bytes(2, 2, 2) == 256 + 256
    for shape in ((1, 4, 4), (4, 0, 4), (2 ** 24 + 1, 2, 2), (2048, 1024, 1024), (2 ** 16, 2 ** 16, 2)):
        assert lib.ls2fm_poisson_workspace_bytes(*shape) == -1, shape
    # refused before anything is enqueued: no device is needed to see it (NULL arrays and sizes only, so nothing could ever launch)
    origin, nan3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0), (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
    fake = None
    good = dict(n=5, shape=(4, 4, 5), origin=origin, voxel=0.5, screen=4.0, cycles=1, gamma=2, ws=fake, size=1 << 20, value=fake)

    def solve(tail=None, **kw):
        a = dict(good, **kw)
        head = (fake, fake, a["n"], *a["shape"], a["origin"], a["voxel"], a["screen"], a["cycles"], a["gamma"])
        rest = (a["value"], fake, a["ws"], a["size"], None)
        return lib.ls2fm_poisson_solve(*head, *rest) if tail is None else lib.ls2fm_poisson_solve_plan(*head, tail, *rest)

    bad = (dict(n=-1), dict(n=2 ** 31), dict(shape=(1, 4, 4)), dict(shape=(4, 4, 0)), dict(shape=(2 ** 24 + 1, 2, 2)), dict(shape=(2048, 1024, 1024)),
           dict(voxel=0.0), dict(voxel=float("inf")), dict(voxel=float("nan")), dict(origin=nan3), dict(origin=None), dict(cycles=-1),
           dict(gamma=0), dict(gamma=3), dict(screen=0.0), dict(screen=-1.0), dict(screen=float("inf")), dict(screen=float("nan")),
           dict(size=4 * 4 * 5 * 36 - 1), dict(n=0), dict())
    for kw in bad:
        assert solve(**kw) == -1 and solve(0, **kw) == -1 and solve(4096, **kw) == -1, kw
    for tail in (-1, 1, 4095, 8192):
        assert solve(tail) == -1, tail
    splat = lambda **kw: (lambda a: lib.ls2fm_poisson_splat(fake, fake, a["n"], *a["shape"], a["origin"], a["voxel"], None, a["value"], fake, a["ws"],   # noqa: E731
                                                            a["size"], None))(dict(good, **kw))
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(shape=(1, 4, 4)), dict(voxel=0.0), dict(origin=nan3), dict(size=80 * 32 - 1), dict(n=0),
               dict()):
        assert splat(**kw) == -1, kw
    for args in ((None, fake, fake, 4, 4, 4, 1.0, 4.0, 0), (fake, None, fake, 4, 4, 4, 1.0, 4.0, 0), (fake, fake, fake, 1, 4, 4, 1.0, 4.0, 0),
                 (fake, fake, fake, 4, 4, 4, 0.0, 4.0, 0), (fake, fake, fake, 4, 4, 4, 2.0, 4.0, 0), (fake, fake, fake, 4, 4, 4, 1.0, 0.0, 0),
                 (fake, fake, fake, 4, 4, 4, 1.0, float("nan"), 1), (fake, fake, fake, 4, 4, 4, 1.0, 4.0, 2)):
        assert lib.ls2fm_poisson_sweep_colour(*args, None) == -1, args
    for args in ((None, fake, fake, 4, 4, 4, 1.0, 4.0, fake), (fake, fake, None, 4, 4, 4, 1.0, 4.0, fake), (fake, None, fake, 4, 4, 4, 1.0, 4.0, fake),
                 (fake, fake, fake, 4, 1, 4, 1.0, 4.0, fake), (fake, fake, fake, 4, 4, 4, 0.0, 4.0, fake), (fake, fake, fake, 4, 4, 4, 1.0, -4.0, fake),
                 (fake, fake, fake, 4, 4, 4, 1.0, 4.0, None)):
        assert lib.ls2fm_poisson_restrict(*args, None) == -1, args
    for args in ((None, 4, 4, 4, fake), (fake, 4, 4, 4, None), (fake, 4, 4, 1, fake)):
        assert lib.ls2fm_poisson_prolong(*args, None) == -1, args
