"""ls2fm_mesh_* (csrc/mesh_components.hip) and the device path of get_surface_high_res_mesh on the GPU: labels, areas and the
extracted component against the numpy restatement (tests/mesh_restate.py), the tie rule, surface sampling, and the whole
high-resolution mesh export on an analytic field and on the sphere-initialised DTU field."""
import math
import sys

import numpy as np
import pytest
import torch

import mc_restate as R
import mesh_restate as M
from ls2fm import mesh
from ls2fm.models.SDF import SDF
from ls2fm.options import make_options
from ls2fm.utils import plots

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grid(shape):
    return torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device=DEV) for n in shape], indexing="ij")


def _sphere(g, r, c):
    return ((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2).sqrt() - r


def _three_spheres_and_torus():
    g = _grid((64, 56, 72))
    x, y, z = g
    torus = (((x - 44.3) ** 2 + (y - 28.1) ** 2).sqrt() - 9.0) ** 2 + (z - 50.2) ** 2
    vol = torch.minimum(torch.minimum(_sphere(g, 12.3, (16.2, 17.1, 18.4)), _sphere(g, 7.4, (46.1, 40.3, 15.2))),
                        torch.minimum(_sphere(g, 3.3, (14.7, 44.6, 52.3)), torus.sqrt() - 3.1))
    return mesh.marching_cubes(vol.float())


_THREE = ((14.2, (18.3, 19.1, 20.2)), (9.1, (42.4, 41.2, 40.3)), (5.3, (45.6, 14.1, 44.7)))


def _three_spheres():
    g = _grid((60, 60, 60))
    (r0, c0), (r1, c1), (r2, c2) = _THREE
    vol = torch.minimum(torch.minimum(_sphere(g, r0, c0), _sphere(g, r1, c1)), _sphere(g, r2, c2))
    return mesh.marching_cubes(vol.float())


def _soup(seed, n_verts, n_faces, used):
    gen = torch.Generator().manual_seed(seed)
    f = torch.randint(0, used, (n_faces, 3), generator=gen, dtype=torch.int32)
    v = torch.randn(n_verts, 3, generator=gen)
    return v.to(DEV), f.to(DEV)


def _cases():
    return {
        "three_spheres_torus": _three_spheres_and_torus,
        "soup_sparse": lambda: _soup(1, 5000, 1500, 4500),          # many small components, unused vertices
        "soup_tiny": lambda: _soup(2, 40, 7, 30),
        "soup_dense": lambda: _soup(3, 20000, 9000, 20000),
    }


@pytest.mark.parametrize("name", list(_cases()))
def test_labels_equal_the_restatement(name):
    verts, faces = _cases()[name]()
    f = faces.cpu().numpy()
    labels = mesh.connected_components(faces, verts.shape[0])
    assert labels.dtype == torch.int32 and labels.shape == (verts.shape[0],)
    want = M.components(f, verts.shape[0])
    assert np.array_equal(labels.cpu().numpy(), want)
    assert torch.equal(labels, mesh.connected_components(faces, verts.shape[0]))
    if name == "three_spheres_torus":
        assert len(np.unique(want)) == 4
    if name.startswith("soup"):
        assert (want == np.arange(len(want))).sum() > 1       # unused vertices are their own component


def test_labels_on_the_512_sphere():
    g = _grid((512, 512, 512))
    vol = _sphere(g, 200.0, (255.3, 256.1, 255.7)).float()
    del g
    verts, faces = mesh.marching_cubes(vol)
    del vol
    assert faces.shape[0] > 900000
    labels = mesh.connected_components(faces, verts.shape[0])
    assert np.array_equal(labels.cpu().numpy(), M.components(faces.cpu().numpy(), verts.shape[0]))
    assert int(labels.max()) == 0
    lv, lf = mesh.largest_component(verts, faces)
    assert torch.equal(lv, verts) and torch.equal(lf, faces)


def test_no_faces_and_bad_indices():
    v = torch.zeros(5, 3, device=DEV)
    f = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    assert torch.equal(mesh.connected_components(f, 5), torch.arange(5, dtype=torch.int32, device=DEV))
    ev, ef = mesh.largest_component(v, f)
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        mesh.connected_components(torch.tensor([[0, 1, 5]], dtype=torch.int32, device=DEV), 5)
    with pytest.raises(ValueError, match="outside"):
        mesh.largest_component(v, torch.tensor([[0, -1, 2]], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("name", list(_cases()))
def test_areas_match_float64_and_repeat_bit_for_bit(name):
    verts, faces = _cases()[name]()
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    a1 = mesh.component_areas(verts, faces)
    a2 = mesh.component_areas(verts, faces)
    assert a1.dtype == torch.float64 and torch.equal(a1.view(torch.int64), a2.view(torch.int64))
    want = M.component_areas(v, f, M.components(f, len(v)))
    total = M.face_areas(v, f).sum()
    assert np.abs(a1.cpu().numpy() - want).max() <= 1e-12 * total


@pytest.mark.parametrize("name", list(_cases()))
def test_largest_component_equals_the_restatement(name):
    verts, faces = _cases()[name]()
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    labels = M.components(f, len(v))
    want_v, want_f = M.extract(v, f, labels, M.largest_label(v, f, labels))
    got_v, got_f = mesh.largest_component(verts, faces)
    assert torch.equal(got_v, torch.from_numpy(want_v).to(DEV))
    assert torch.equal(got_f, torch.from_numpy(want_f).to(DEV))
    again = mesh.largest_component(verts, faces)
    assert torch.equal(again.vertices, got_v) and torch.equal(again.faces, got_f)


def test_tie_goes_to_the_component_holding_face_0():
    g = _grid((40, 40, 40))
    verts, faces = mesh.marching_cubes(_sphere(g, 13.2, (19.3, 20.1, 19.7)).float())
    n_v, n_f = verts.shape[0], faces.shape[0]
    perm = torch.randperm(n_f, generator=torch.Generator().manual_seed(4)).to(DEV)
    second = faces[perm] + n_v                         # same coordinates, other indices, shuffled, listed first
    both_v = torch.cat([verts, verts])
    both_f = torch.cat([second, faces]).contiguous()
    labels = mesh.connected_components(both_f, 2 * n_v)
    assert set(labels.unique().tolist()) == {0, n_v}
    areas = mesh.component_areas(both_v, both_f)
    assert areas[0].item() > 0 and torch.equal(areas[0:1].view(torch.int64), areas[n_v:n_v + 1].view(torch.int64))
    kept_v, kept_f = mesh.largest_component(both_v, both_f)
    assert torch.equal(kept_v, verts) and torch.equal(kept_f, faces[perm])     # face 0 belongs to the second copy


def test_sample_surface_from_uniforms_matches_the_restatement():
    verts, faces = _three_spheres_and_torus()
    n = 200000
    gen = torch.Generator().manual_seed(7)
    u0, u1, u2 = (torch.rand(n, dtype=torch.float64, generator=gen) for _ in range(3))
    pts, face = mesh._sample_surface_from_uniforms(verts, faces, u0.to(DEV), u1.to(DEV), u2.to(DEV))
    want_p, want_face, cum = M.sample_surface(verts.cpu().numpy(), faces.cpu().numpy(), u0.numpy(), u1.numpy(), u2.numpy())
    face = face.cpu().numpy()
    pick = u0.numpy() * cum[-1]
    differ = face != want_face
    if differ.any():                                   # only picks within 1e-12 relative of a cumulative boundary
        near = np.abs(cum[np.minimum(want_face[differ], len(cum) - 1)] - pick[differ]) <= 1e-12 * cum[-1]
        near |= np.abs(cum[np.maximum(want_face[differ] - 1, 0)] - pick[differ]) <= 1e-12 * cum[-1]
        assert near.all()
    same = ~differ
    assert same.sum() > n - 10
    assert pts.dtype == torch.float32
    assert np.abs(pts.cpu().numpy()[same].astype(np.float64) - want_p[same]).max() <= 1e-6 * max(1.0, np.abs(want_p).max())


def test_sample_surface_shares_follow_the_areas():
    verts, faces = _three_spheres()
    labels = mesh.connected_components(faces, verts.shape[0])
    areas = mesh.component_areas(verts, faces)
    roots = torch.nonzero(areas).view(-1)
    assert roots.numel() == 3
    n = 300000
    gen = torch.Generator(device=DEV).manual_seed(3)
    pts = mesh.sample_surface(verts, faces, n, generator=gen)
    gen2 = torch.Generator(device=DEV).manual_seed(3)
    assert torch.equal(pts, mesh.sample_surface(verts, faces, n, generator=gen2))
    # the component of each point: the nearest sphere centre (the spheres lie far apart); its label: that of the nearest vertex
    centres = torch.tensor([c for _, c in _THREE], dtype=torch.float64, device=DEV)
    which = torch.cdist(pts.double(), centres).argmin(dim=1)
    vert_label = labels[torch.cdist(centres, verts.double()).argmin(dim=1)]
    assert sorted(vert_label.tolist()) == sorted(roots.tolist())
    share = areas[vert_label] / areas.sum()
    for k, p in enumerate(share.tolist()):
        got = float((which == k).double().mean())
        sigma = math.sqrt(p * (1 - p) / n)
        assert abs(got - p) <= 3 * sigma, (k, got, p, (got - p) / sigma)


def _closed_and_outward(verts, faces):
    f = faces.cpu().numpy()
    d = R.directed_edges(f)
    key = d[:, 0] * (len(verts) + 1) + d[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge repeats"
    rev = d[:, 1] * (len(verts) + 1) + d[:, 0]
    assert np.isin(rev, key).all(), "an edge without its opposite"
    assert R.euler_characteristic(verts.cpu().numpy(), f) == 2
    p = verts.double()[faces.long()]
    assert float((p[:, 0] * torch.cross(p[:, 1], p[:, 2], dim=1)).sum()) > 0      # outward: positive signed volume


def _sphere_with_floater(pts):
    big = pts.norm(dim=1) - 0.3
    small = (pts - torch.tensor([0.5, 0.5, 0.5], device=pts.device)).norm(dim=1) - 0.05
    return torch.minimum(big, small)[:, None]


def test_high_res_mesh_on_an_analytic_field_drops_the_floater(tmp_path):
    path = str(tmp_path / "mesh.ply")
    torch.manual_seed(0)
    out = plots.get_surface_high_res_mesh(_sphere_with_floater, resolution=128, grid_boundary=[-0.6, 0.6],
                                          take_components=True, path=path, backend="device")
    assert isinstance(out, mesh.Mesh) and out.vertices.is_cuda and out.faces.dtype == torch.int32
    v, f = mesh.read_ply_ascii(path)
    assert np.array_equal(v.view(np.uint32), out.vertices.cpu().numpy().view(np.uint32))
    assert np.array_equal(f, out.faces.cpu().numpy())
    step = (0.6 + 0.1) * 2 / 127                       # the fitted box's shortest side over resolution - 1
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(r - 0.3).max() <= step
    assert np.linalg.norm(v - np.array([0.5, 0.5, 0.5]), axis=1).min() > 0.2
    _closed_and_outward(out.vertices, out.faces)


def test_high_res_mesh_without_components_keeps_the_sampling_frame(tmp_path):
    torch.manual_seed(0)
    out = plots.get_surface_high_res_mesh(lambda p: p.norm(dim=1, keepdim=True) - 0.3, resolution=64,
                                          grid_boundary=[-0.6, 0.6], take_components=False, path=None, backend="device")
    _closed_and_outward(out.vertices, out.faces)
    with pytest.raises(ValueError, match="no crossing"):
        plots.get_surface_high_res_mesh(lambda p: p.norm(dim=1, keepdim=True) + 1.0, resolution=64,
                                        grid_boundary=[-0.6, 0.6], backend="device")


def _dtu_field():
    torch.manual_seed(0)
    opt = make_options("DTU", device=DEV)
    return SDF(opt).to(DEV)


def test_high_res_mesh_on_the_dtu_field_equals_the_restatement(tmp_path):
    sdf = _dtu_field()
    torch.manual_seed(5)
    result, info = plots._high_res_device(sdf.infer_sdf, 128, [-0.6, 0.6], 0.0, True)
    vol = info["volume"].cpu().numpy()
    sp = info["spacing"]
    want_v, want_f = R.marching_cubes(vol, 0.0, (sp, sp, sp))
    verts = torch.from_numpy(want_v).to(DEV) @ info["vecs"] + info["first"]
    assert torch.equal(result.faces.cpu(), torch.from_numpy(want_f))
    assert torch.equal(result.vertices.view(torch.int32), verts.view(torch.int32))
    # the public call, same seed: the same mesh in the file
    path = str(tmp_path / "dtu.ply")
    torch.manual_seed(5)
    out = plots.get_surface_high_res_mesh(sdf.infer_sdf, resolution=128, grid_boundary=[-0.6, 0.6], level=0.,
                                          take_components=True, path=path, backend="device")
    v, f = mesh.read_ply_ascii(path)
    assert np.array_equal(v.view(np.uint32), result.vertices.cpu().numpy().view(np.uint32))
    assert np.array_equal(f, want_f) and torch.equal(out.faces, result.faces)
    _closed_and_outward(out.vertices, out.faces)


def test_high_res_mesh_at_the_pipelines_resolution(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "trimesh", None)
    sdf = _dtu_field()
    path = str(tmp_path / "dtu512.ply")
    out = plots.get_surface_high_res_mesh(sdf.infer_sdf, resolution=512, grid_boundary=[-0.6, 0.6], level=0.,
                                          take_components=True, path=path)            # backend="auto" without trimesh
    assert out.faces.shape[0] > 500000
    v, f = mesh.read_ply_ascii(path)
    assert v.shape[0] == out.vertices.shape[0] and np.array_equal(f, out.faces.cpu().numpy())
    _closed_and_outward(out.vertices, out.faces)


def test_auto_picks_the_device_path_without_trimesh(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "trimesh", None)
    path = str(tmp_path / "auto.ply")
    torch.manual_seed(0)
    out = plots.get_surface_high_res_mesh(_sphere_with_floater, resolution=48, grid_boundary=[-0.6, 0.6], path=path)
    assert isinstance(out, mesh.Mesh)
    assert open(path, "rb").read().startswith(b"ply\nformat ascii 1.0\n")
