"""ls2fm_marching_cubes_* (csrc/marching_cubes.hip) on the device: bit-identical to the numpy restatement (tests/mc_restate.py),
deterministic, watertight and outward-oriented at scale, and behind extract_mesh(backend="device") on a real field sweep."""
import math

import numpy as np
import pytest
import torch

import mc_restate as R
from ls2fm import mesh
from ls2fm.models.SDF import SDF
from ls2fm.options import make_options
from ls2fm.utils import util

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grid(shape, centre=None):
    axes = [torch.arange(n, dtype=torch.float64) for n in shape]
    c = [(n - 1) / 2 for n in shape] if centre is None else centre
    x, y, z = torch.meshgrid(*axes, indexing="ij")
    return x - c[0], y - c[1], z - c[2]


def _sphere(shape, r, centre=None):
    x, y, z = _grid(shape, centre)
    return ((x * x + y * y + z * z).sqrt() - r).float()


def _torus(shape, big, small):
    x, y, z = _grid(shape)
    return (((x * x + y * y).sqrt() - big) ** 2 + z * z).sqrt().sub(small).float()


def _checkerboard(shape):
    i, j, k = torch.meshgrid(*[torch.arange(n) for n in shape], indexing="ij")
    return ((i + j + k) % 2 * 2 - 1).float()


def _cases():
    gen = torch.Generator().manual_seed(11)
    return {
        "sphere_33": (_sphere((33, 33, 33), 12.4), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
        "torus_40x48x56": (_torus((40, 48, 56), 14.0, 5.5), 0.0, (0.05, 0.04, 0.03), (-1.0, -0.5, 0.25)),
        "noise_24": (torch.randn(24, 24, 24, generator=gen), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
        "exact_level": (torch.randint(-1, 2, (13, 11, 17), generator=gen).float(), 0.0, (0.5, 0.25, 2.0), (1.0, 2.0, 3.0)),
        "exact_level_0.5": (torch.randint(0, 3, (9, 10, 8), generator=gen).float() * 0.5, 0.5, (1.0, 1.0, 1.0),
                            (0.0, 0.0, 0.0)),
        "level_nonzero": (_sphere((30, 31, 29), 0.0), 9.3, (0.1, 0.1, 0.1), (-1.5, -1.5, -1.5)),
        "checkerboard": (_checkerboard((12, 9, 10)), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
        "cube_2x2x2": (torch.tensor([[[-1.0, 2.0], [0.5, -3.0]], [[4.0, -0.25], [1.0, 2.0]]]), 0.0, (1.0, 1.0, 1.0),
                       (0.0, 0.0, 0.0)),
        "all_above": (torch.ones(5, 6, 7), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
        "all_below": (-torch.ones(4, 4, 9), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    }


@pytest.mark.parametrize("name", list(_cases()))
def test_device_mesh_equals_the_restatement_bit_for_bit(name):
    vol, level, sp, og = _cases()[name]
    verts, faces = mesh.marching_cubes(vol.to(DEV), level, sp, og)
    want_v, want_f = R.marching_cubes(vol.numpy(), level, sp, og)
    assert verts.device.type == "cuda" and faces.device.type == "cuda"
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32
    assert tuple(verts.shape) == want_v.shape and tuple(faces.shape) == want_f.shape
    assert np.array_equal(faces.cpu().numpy(), want_f)
    assert np.array_equal(verts.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
    if name.startswith("all_"):
        assert verts.shape == (0, 3) and faces.shape == (0, 3)
    else:
        assert len(want_f) > 0


def test_non_contiguous_volume_and_repeat_calls_are_identical():
    vol = _torus((40, 48, 56), 14.0, 5.5).to(DEV)
    v1, f1 = mesh.marching_cubes(vol, 0.25)
    v2, f2 = mesh.marching_cubes(vol, 0.25)
    assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(f1, f2)
    t = vol.permute(2, 1, 0).contiguous().permute(2, 1, 0)                      # same values, not contiguous
    assert not t.is_contiguous()
    v3, f3 = mesh.marching_cubes(t, 0.25)
    assert torch.equal(v1.view(torch.int32), v3.view(torch.int32)) and torch.equal(f1, f3)


def _closed_and_oriented(verts, faces):
    """on the device: every directed edge once, and its reverse present (a closed, consistently oriented surface)"""
    f = faces.long()
    d = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = verts.shape[0] + 1
    key, _ = torch.sort(d[:, 0] * n + d[:, 1])
    assert bool((key[1:] != key[:-1]).all()), "a directed edge repeats"
    rev = d[:, 1] * n + d[:, 0]
    at = torch.searchsorted(key, rev).clamp(max=key.numel() - 1)
    assert bool((key[at] == rev).all()), "an edge without its opposite"
    assert int(torch.unique(f).numel()) == verts.shape[0]


def _signed_volume(verts, faces):
    p = verts.double()[faces.long()]
    return float((p[:, 0] * torch.cross(p[:, 1], p[:, 2], dim=1)).sum() / 6)


def test_sphere_256_is_watertight_and_outward():
    r = 100.0
    vol = _sphere((256, 256, 256), r).to(DEV)
    verts, faces = mesh.marching_cubes(vol)
    assert faces.shape[0] > 100000
    _closed_and_oriented(verts, faces)
    assert abs(_signed_volume(verts, faces) / (4 / 3 * math.pi * r ** 3) - 1) < 0.005
    r = 50.0
    vol = _sphere((128, 128, 128), r, centre=(63.3, 64.1, 62.7)).to(DEV)
    verts, faces = mesh.marching_cubes(vol)
    _closed_and_oriented(verts, faces)
    assert abs(_signed_volume(verts, faces) / (4 / 3 * math.pi * r ** 3) - 1) < 0.005


def _dtu_field(seed=0):
    torch.manual_seed(seed)
    opt = make_options("DTU", device=DEV)
    return opt, SDF(opt).to(DEV)


def test_extract_mesh_device_backend_on_a_dtu_field(tmp_path):
    opt, sdf = _dtu_field()
    N, size = 512, 2.0
    path = str(tmp_path / "surface.ply")
    vol = util.extract_mesh(sdf, volume_size=size, N=N, filepath=path, backend="device")
    assert vol.shape == (N, N, N)
    assert torch.equal(vol, util.sdf_volume(sdf, size, N))                             # the return value is the sweep's volume
    _, _, origin, sizes = util._lattice(size, N, None, None)
    verts, faces = mesh.marching_cubes(vol, 0.0, [s / N for s in sizes], origin)
    assert faces.shape[0] > 10000
    v, f = mesh.read_ply(path)
    assert np.array_equal(v.view(np.uint32), verts.cpu().numpy().view(np.uint32))
    assert np.array_equal(f, faces.cpu().numpy())
    _closed_and_oriented(verts, faces)


def test_vertices_lie_on_the_zero_set_of_the_field():
    """regular lattice, true step as spacing: every vertex within a quarter step of the field's zero set"""
    opt, sdf = _dtu_field(1)
    N, size = 160, 2.0
    vol = util.sdf_volume(sdf, size, N, reference_indexing=False)
    step, col_origin, _, _ = util._lattice(size, N, None, None)
    verts, faces = mesh.marching_cubes(vol, 0.0, step, col_origin)
    assert faces.shape[0] > 1000
    with torch.no_grad():
        s = sdf.infer_sdf(verts).view(-1)
    assert float(s.abs().max()) <= 0.25 * step[0]


def test_same_vertex_set_as_skimage_on_a_smooth_sphere():
    measure = pytest.importorskip("skimage.measure")
    vol = _sphere((64, 64, 64), 20.3, centre=(31.6, 32.2, 31.9))
    verts, _ = mesh.marching_cubes(vol.to(DEV))
    sv, _, _, _ = measure.marching_cubes(vol.numpy(), level=0.0)
    a = np.unique(np.round(verts.cpu().numpy().astype(np.float64), 4), axis=0)
    b = np.unique(np.round(sv.astype(np.float64), 4), axis=0)
    assert a.shape == b.shape and np.allclose(a, b, atol=2e-4)
