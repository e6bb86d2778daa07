"""CPU: THE CLUSTERING RULE of include/ls2fm.h judged by its properties on the numpy restatement (tests/simplify_restate.py), so that
the GPU tests (tests/test_hip_simplify.py) can be exact comparisons against that restatement; the C refusals, which fire before any
device work; the bisection of ls2fm.simplify.simplify_to_faces and the torch form on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import simplify_restate as R
import simplify_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE_N, SPHERE_R = 64, 20.0
SPHERE_CELLS = (2.5, 4.0, 7.0)
BOX = ((40, 36, 44), (11.3, 9.6, 13.2))


def test_header_binding_and_library_agree_on_the_new_symbols():
    from ls2fm import _lib, simplify  # noqa: F401
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    declared = set(re.findall(r"\b(ls2fm_mesh_simplify_[a-z_]+)\s*\(", header))
    assert declared == {"ls2fm_mesh_simplify_" + n for n in ("workspace_bytes", "keys", "mark", "index", "place", "emit")}
    lib = _lib.load()
    for name in declared:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.ls2fm_abi_version() == 13 == int(re.search(r"#define\s+LS2FM_ABI_VERSION\s+(\d+)", header).group(1))
    assert int(re.search(r"#define\s+LS2FM_SIMPLIFY_SUMS\s+(\d+)", header).group(1)) == R.N_SUMS == simplify.N_SUMS
    assert simplify.DEFAULT_REG == 2.0 ** -2 and simplify.KEY_BITS == R.KEY_BITS


def test_every_c_refusal_fires_before_device_work():
    """host buffers stand in for device arrays: a call that is refused never looks at them, and nothing here needs a GPU"""
    from ls2fm import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    INVALID, WORKSPACE = -1, -4
    assert lib.ls2fm_mesh_simplify_workspace_bytes(-1, 0) == INVALID and lib.ls2fm_mesh_simplify_workspace_bytes(0, -1) == INVALID
    assert lib.ls2fm_mesh_simplify_workspace_bytes(1 << 31, 0) == INVALID                       # sizes at the limits
    assert lib.ls2fm_mesh_simplify_workspace_bytes((1 << 31) - 1, 0) > 0
    assert lib.ls2fm_mesh_simplify_workspace_bytes(8, 715827883) == INVALID                     # 3 F = 2^31 + 1
    assert lib.ls2fm_mesh_simplify_workspace_bytes(8, 715827882) > 0                            # 3 F = 2^31 - 2
    need = lib.ls2fm_mesh_simplify_workspace_bytes(8, 4)
    assert need >= 2 * 8 * 4

    def keys(verts=p, n_verts=8, faces=p, n_faces=4, cell=1.0, vert_key=p, counts=p):
        return lib.ls2fm_mesh_simplify_keys(verts, n_verts, faces, n_faces, cell, vert_key, None, counts, None)
    for bad in (dict(verts=None), dict(faces=None), dict(vert_key=None), dict(counts=None), dict(n_verts=-1), dict(n_verts=1 << 31),
                dict(n_faces=-1), dict(n_faces=715827883), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")),
                dict(cell=float("inf")), dict(n_verts=0)):
        assert keys(**bad) == INVALID, bad

    def mark(sorted_key=p, n_verts=8, faces=p, n_faces=4, corner_head=p, head_used=p, ws=p, ws_bytes=need):
        return lib.ls2fm_mesh_simplify_mark(sorted_key, p, n_verts, faces, n_faces, p, corner_head, head_used, ws, ws_bytes, None)

    def index(head_rank=p, n_verts=8, n_faces=4, vertex_map=p, face_index=p, ws=p, ws_bytes=need):
        return lib.ls2fm_mesh_simplify_index(p, head_rank, n_verts, p, n_faces, p, vertex_map, face_index, ws, ws_bytes, None)
    for call, bads in ((mark, (dict(sorted_key=None), dict(faces=None), dict(corner_head=None), dict(head_used=None), dict(n_verts=-1),
                              dict(n_faces=715827883))),
                       (index, (dict(head_rank=None), dict(vertex_map=None), dict(face_index=None), dict(n_verts=1 << 31), dict(n_faces=-1)))):
        for bad in bads:
            assert call(**bad) == INVALID, (call.__name__, bad)
        assert call(ws=None) == WORKSPACE and call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE

    def place(verts=p, colors=None, channels=0, cell=1.0, placement=0, reg=0.25, sorted_key=p, n_out=2, stages=3, sums=p, out_verts=p,
              out_colors=None, ws=p, ws_bytes=need):
        return lib.ls2fm_mesh_simplify_place(verts, colors, channels, 8, p, 4, cell, placement, reg, sorted_key, p, p, p, n_out, stages,
                                             sums, p, out_verts, out_colors, ws, ws_bytes, None)
    for bad in (dict(verts=None), dict(sorted_key=None), dict(sums=None), dict(out_verts=None), dict(cell=0.0), dict(cell=-2.0),
                dict(cell=float("nan")), dict(cell=float("inf")), dict(colors=p, channels=0, out_colors=p),
                dict(colors=p, channels=5, out_colors=p), dict(colors=None, channels=3), dict(colors=p, channels=3, out_colors=None),
                dict(placement=2), dict(placement=-1), dict(reg=-1.0), dict(reg=float("nan")), dict(reg=float("inf")), dict(n_out=-1),
                dict(n_out=9), dict(stages=0), dict(stages=4)):
        assert place(**bad) == INVALID, bad
    assert place(ws=None) == WORKSPACE and place(ws_bytes=need - 1) == WORKSPACE

    def emit(face_index=p, keep=p, n_faces=4, n_kept=2, out_faces=p):
        return lib.ls2fm_mesh_simplify_emit(face_index, keep, p, n_faces, n_kept, out_faces, None)
    for bad in (dict(face_index=None), dict(keep=None), dict(out_faces=None), dict(n_faces=-1), dict(n_kept=-1), dict(n_kept=5),
                dict(n_faces=715827883)):
        assert emit(**bad) == INVALID, bad
    assert not any(buf.raw)                                                                    # nothing was written either


def test_python_refusals():
    from ls2fm import simplify
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for fn in (lambda: simplify.simplify(v, f, 1.0), lambda: simplify.count_faces(v, f, 1.0), lambda: simplify.simplify_to_faces(v, f, 10)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="cell"):
            simplify.simplify(v, f, bad)
    with pytest.raises(ValueError, match="placement"):
        simplify.simplify(v, f, 1.0, placement="median")
    with pytest.raises(ValueError, match="reg"):
        simplify.simplify(v, f, 1.0, reg=-1.0)
    with pytest.raises(ValueError, match="21 bits"):
        simplify._simplify_torch(torch.tensor([[3.0e6, 0.0, 0.0]]), f[:0], 1.0)


@pytest.fixture(scope="module")
def sphere_runs():
    v, f, c = S.sphere_mesh(SPHERE_N, SPHERE_R)
    return {(cell, pl): R.simplify(v, f, cell, placement=pl) for cell in SPHERE_CELLS for pl in ("quadric", "mean")}, c


def test_sphere_counts_fall_and_the_output_is_well_formed(sphere_runs):
    runs, _ = sphere_runs
    counts = [runs[(cell, "quadric")]["n_surviving"] for cell in SPHERE_CELLS]
    assert counts[0] > counts[1] > counts[2] > 0
    for (cell, pl), r in runs.items():
        f = r["faces"]
        assert len(f) and np.array_equal(np.unique(f), np.arange(len(r["vertices"])))          # every output vertex is used
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert np.array_equal(r["faces"], runs[(cell, "mean")]["faces"]) and r["n_bad"] == 0
        assert np.isfinite(r["vertices"]).all()


def test_quadric_placement_beats_the_mean_on_the_sphere(sphere_runs):
    """the orderings are the assertions; the restatement's figures are printed (DESIGN 3.21 records them)"""
    runs, c = sphere_runs
    v, f, _ = S.sphere_mesh(SPHERE_N, SPHERE_R)
    true_volume = 4.0 / 3.0 * np.pi * SPHERE_R ** 3
    for cell in SPHERE_CELLS:
        radial, volume = {}, {}
        for pl in ("quadric", "mean"):
            r = runs[(cell, pl)]
            radial[pl] = float(np.abs(np.linalg.norm(r["vertices"].astype(np.float64) - c, axis=1) - SPHERE_R).max())
            volume[pl] = abs(abs(S.signed_volume(r["vertices"], r["faces"])) - true_volume)
        print(f"sphere r {SPHERE_R} cell {cell}: {runs[(cell, 'quadric')]['n_surviving']} faces of {len(f)}; worst radial error quadric "
              f"{radial['quadric']:.4f} mean {radial['mean']:.4f}; volume error quadric {volume['quadric']:.1f} mean {volume['mean']:.1f}")
        assert radial["quadric"] < radial["mean"]
        assert volume["quadric"] < volume["mean"]


@pytest.mark.parametrize("cell", [2.5, 4.0])
def test_quadric_placement_beats_the_mean_on_the_box(cell):
    v, f, c, h = S.box_mesh(*BOX)
    worst = {pl: float(S.box_distance(R.simplify(v, f, cell, placement=pl)["vertices"], c, h).max()) for pl in ("quadric", "mean")}
    print(f"box half {BOX[1]} cell {cell}: worst distance to the surface quadric {worst['quadric']:.4f} mean {worst['mean']:.4f}")
    assert worst["quadric"] < worst["mean"]


def test_a_cell_larger_than_the_mesh_leaves_nothing():
    v, f, _ = S.sphere_mesh(24, 8.3)
    r = R.simplify(v, f, 64.0)
    assert len(r["vertices"]) == 0 and len(r["faces"]) == 0 and (r["vertex_map"] == -1).all() and r["n_surviving"] == 0


def test_a_cell_that_holds_one_vertex_gives_the_mesh_back():
    v, f, _ = S.sphere_mesh(24, 8.3)
    cell = 2.0 ** -12
    r = R.simplify(v, f, cell, placement="mean")
    assert len(np.unique(r["key"])) == len(v)                                                  # every vertex alone in its cell
    order = np.argsort(r["key"], kind="stable")
    assert np.array_equal(r["vertices"].view(np.uint32), v[order].view(np.uint32))
    assert np.array_equal(r["vertex_map"][order], np.arange(len(v)))
    assert np.array_equal(r["faces"], r["vertex_map"][f])                                      # marching cubes repeats no triangle
    doubled = np.concatenate([f, f[:5][:, [1, 2, 0]], f[:3][:, [0, 2, 1]]])                    # rotated copies go, opposite ones stay
    r2 = R.simplify(v, doubled, cell, placement="mean")
    assert np.array_equal(r2["faces"], r["vertex_map"][np.concatenate([f, f[:3][:, [0, 2, 1]]])])


def test_the_gpu_scenes_meet_the_edges_they_are_there_for():
    sc = S.gpu_scenes()
    r = R.simplify(**{k: sc["soup_c3"][k] for k in ("verts", "faces", "cell", "colors")})
    assert set(np.unique(r["face_class"])) == {0, 1, 2} and (~r["valid"]).sum() == 3
    assert r["n_surviving"] > len(r["faces"])                                                  # duplicates were removed
    assert (r["vertex_map"][~r["valid"]] == -1).all() and (r["vertex_map"][r["valid"]] == -1).any()
    assert (sc["soup_c3"]["verts"][np.isfinite(sc["soup_c3"]["verts"]).all(axis=1)] < 0).any()
    seg = R.simplify(sc["segments"]["verts"], sc["segments"]["faces"], sc["segments"]["cell"])
    corners = seg["n_terms"][:, 0]
    assert set(S.SEGMENT_LENGTHS) <= set(corners.tolist()) and set(S.SEGMENT_LENGTHS) <= set(seg["count"].tolist()) | {1}
    sheet = R.simplify(sc["sheet"]["verts"], sc["sheet"]["faces"], sc["sheet"]["cell"])
    assert len(sheet["vertices"]) > 2048 * S.CELLS_PER_WORKGROUP
    dy = sc["sphere_dyadic_2"]
    on_face = (np.mod(dy["verts"].astype(np.float64), dy["cell"]) == 0).any(axis=1)
    assert on_face.mean() > 0.3                                                                # vertices exactly on cell faces
    ex = R.simplify(sc["extreme_cells"]["verts"], sc["extreme_cells"]["faces"], sc["extreme_cells"]["cell"])
    assert ex["valid"].all() and ex["n_bad"] == 0 and ex["key"][0] == 2 ** 63 - 1 and ex["key"][3] == 0        # no key is a sentinel
    assert len(ex["vertices"]) == 5 and len(ex["faces"]) == 3 and (ex["vertex_map"] >= 0).all()
    for name in ("no_faces", "one_cell", "empty"):
        r = R.simplify(sc[name]["verts"], sc[name]["faces"], sc[name]["cell"])
        assert len(r["vertices"]) == 0 and len(r["faces"]) == 0
    assert {len(sc[k]["verts"]) for k in sc if k.startswith("sized")} == {S.THREADS - 1, S.THREADS, S.THREADS + 1}


def test_the_bisection_meets_its_target_and_repeats():
    from ls2fm import simplify
    v, f, _ = S.sphere_mesh(24, 8.3)
    diagonal = float(np.sqrt(((v.max(axis=0).astype(np.float64) - v.min(axis=0)) ** 2).sum()))
    tried = []

    def count(cell):
        key, _, bad = R.vertex_keys(v, cell)
        tried.append(cell)
        return int((R.face_classes(key, f) == R.FACE_SURVIVES).sum()), int(bad.sum())
    target = 400
    cell = simplify._bisect_cell(count, diagonal, target)
    first = list(tried)
    assert len(first) == simplify.BISECTION_STEPS + 1 and cell in first
    r = R.simplify(v, f, cell)
    assert 0 < len(r["faces"]) <= r["n_surviving"] <= target
    assert all(count(c)[0] > target for c in first if c < cell)                                # the smallest cell tried that fits
    del tried[:]
    assert simplify._bisect_cell(count, diagonal, target) == cell and tried == first           # deterministic
    with pytest.raises(ValueError, match="survive"):
        simplify._bisect_cell(lambda c: (10, 0), diagonal, 5)


@pytest.mark.parametrize("name", ["sphere_2.5", "soup_c3", "segments", "one_face", "no_faces"])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_the_torch_form_on_the_cpu_follows_the_restatement(name, placement):
    """ls2fm.simplify._simplify_torch on CPU tensors: keys, faces and vertex_map exactly; the sums within the summation bound (index_add_
    has no stated order); the vertices to 1e-5 of the cell"""
    from ls2fm import simplify
    sc = S.gpu_scenes()[name]
    want = R.simplify(sc["verts"], sc["faces"], sc["cell"], sc["colors"], placement=placement)
    colors = None if sc["colors"] is None else torch.from_numpy(sc["colors"])
    got, sums, count = simplify._simplify_torch(torch.from_numpy(sc["verts"]), torch.from_numpy(sc["faces"]), sc["cell"], colors,
                                                placement=placement, return_sums=True)
    assert np.array_equal(got.faces.numpy(), want["faces"]) and np.array_equal(got.vertex_map.numpy(), want["vertex_map"])
    assert np.array_equal(count.numpy(), want["count"])
    bound = (want["n_terms"] + 16) * 2.0 ** -53 * want["abs_sums"]
    assert (np.abs(sums.numpy() - want["sums"]) <= bound).all()
    assert np.abs(got.vertices.numpy().astype(np.float64) - want["vertices"]).max(initial=0.0) <= 1e-5 * sc["cell"]
    if colors is not None:
        assert np.abs(got.colors.numpy() - want["colors"]).max(initial=0.0) <= 1e-6
