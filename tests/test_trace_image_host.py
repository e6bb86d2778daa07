"""CPU: the C ABI of the image tracing (ls2fm_trace_image / ls2fm_trace_image_workspace_bytes) -- header, binding and library
agree, the workspace does not depend on the image or the number of views, and the refusals return their codes before any
device work."""
import ctypes
import os
import re

import pytest

from ls2fm import _lib
from ls2fm.hashgrid import build_grid_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ls2fm_trace_image_workspace_bytes", "ls2fm_trace_image")


def _descs(levels=16, log2=19, bg_sdf=0):
    f = _lib.FieldDesc()
    for d in range(3):
        f.bound_min[d], f.bound_max[d] = -1.0, 1.0
    f.rescale, f.scale_mlp, f.inside, f.bg_sdf, f.bg_rad = 1.0, 1.0, 1, bg_sdf, 2.0
    f.n_samples, f.dual_field = 128, 1
    g = build_grid_desc(levels, 2, log2, 16, 1.447269237440378)
    return f, g


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    lib = _lib.load()
    for name in SYMS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    # the binding's argument count matches the header's declaration
    decl = re.search(r"int ls2fm_trace_image\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib._SIGNATURES["ls2fm_trace_image"][1]) == 20


def test_workspace_does_not_depend_on_the_image_or_the_views():
    lib = _lib.load()
    sizes = set()
    for levels, log2 in ((16, 19), (8, 14), (12, 22)):
        f, g = _descs(levels, log2)
        ws = lib.ls2fm_trace_image_workspace_bytes(ctypes.byref(f), ctypes.byref(g))
        assert 0 < ws <= 8 << 20, ws           # the packed weights and one chunk of the normal query: a few MB
        sizes.add(ws)
    # the query takes no image size and no view count: one value serves 16 x 16 and 1200 x 1600, one view and sixty
    assert len(sizes) == 1


def _call(lib, f, g, params=True, poses=True, kinv=True, outs=True, V=1, H=16, W=16, iters=10, ws=True, grad=True):
    p = _lib.Params()
    p.sdf_table = p.sdf_mlp[0].weight_v = p.sdf_mlp[1].weight_v = 0x1000
    k = (ctypes.c_float * 9)(*([1.0] * 9))
    fake = ctypes.c_void_p(0x1000)              # never dereferenced: every refusal comes first
    nul = ctypes.c_void_p(0)
    return lib.ls2fm_trace_image(ctypes.byref(f), ctypes.byref(g), ctypes.byref(p) if params else None, fake if poses else nul, V,
                                 k if kinv else None, H, W, 5e-5, iters, 1e-3, fake if outs else nul, fake, fake, fake,
                                 fake if grad else nul, nul, fake, fake if ws else nul, nul)


@pytest.mark.parametrize("case", ["depth", "poses", "params", "kinv", "views", "height", "width", "iters"])
def test_argument_refusals(case):
    lib = _lib.load()
    f, g = _descs()
    kw = {"depth": dict(outs=False), "poses": dict(poses=False), "params": dict(params=False), "kinv": dict(kinv=False),
          "views": dict(V=0), "height": dict(H=0), "width": dict(W=-3), "iters": dict(iters=-1)}[case]
    assert _call(lib, f, g, **kw) == -1          # LS2FM_ERR_INVALID_ARGUMENT


def test_unsupported_and_workspace_refusals():
    lib = _lib.load()
    f, g = _descs(bg_sdf=1)
    assert _call(lib, f, g) == -2                # LS2FM_ERR_UNSUPPORTED: bg_sdf (the normal query has no sphere min)
    assert lib.ls2fm_trace_image_workspace_bytes(ctypes.byref(f), ctypes.byref(g)) == -2
    f, g = _descs()
    assert _call(lib, f, g, ws=False) == -4      # LS2FM_ERR_WORKSPACE
    assert _call(lib, f, g, ws=False, grad=False) == -4
    assert lib.ls2fm_trace_image_workspace_bytes(None, ctypes.byref(g)) == -1
    assert lib.ls2fm_trace_image_workspace_bytes(ctypes.byref(f), None) == -1
