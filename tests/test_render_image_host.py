"""CPU: the C ABI of the image render (ls2fm_render_image / ls2fm_render_image_workspace_bytes) -- header, binding and library
agree, the workspace does not depend on the image, and the refusals return their codes before any device work."""
import ctypes
import os
import re

import pytest

from ls2fm import _lib
from ls2fm.hashgrid import build_grid_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ls2fm_render_image_workspace_bytes", "ls2fm_render_image")


def _descs(dual=True, n_samples=128, levels=16, log2=19):
    f = _lib.FieldDesc()
    for d in range(3):
        f.bound_min[d], f.bound_max[d] = -1.0, 1.0
    f.rescale, f.scale_mlp, f.inside, f.bg_sdf, f.bg_rad = 1.0, 1.0, 1, 0, 2.0
    f.n_samples, f.dual_field = n_samples, 1 if dual else 0
    g = build_grid_desc(levels, 2, log2, 16, 1.447269237440378)
    return f, g


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "ls2fm.h")).read()
    lib = _lib.load()
    for name in SYMS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_workspace_does_not_depend_on_the_image():
    lib = _lib.load()
    for dual in (True, False):
        for n in (48, 128, 320):
            f, g = _descs(dual, n)
            ws = lib.ls2fm_render_image_workspace_bytes(ctypes.byref(f), ctypes.byref(g), ctypes.byref(g) if dual else None)
            assert 0 < ws < 1 << 30, (dual, n, ws)
    # the size query takes no image size: the one value serves 16 x 16 and 1200 x 1600, one view and sixty
    f, g = _descs()
    a = lib.ls2fm_render_image_workspace_bytes(ctypes.byref(f), ctypes.byref(g), ctypes.byref(g))
    b = lib.ls2fm_render_image_workspace_bytes(ctypes.byref(f), ctypes.byref(g), ctypes.byref(g))
    assert a == b
    # smaller than the training workspace of one 8192-ray slice of the sliced path
    assert a < lib.ls2fm_render_workspace_bytes(ctypes.byref(f), ctypes.byref(g), 8192)


def _call(lib, f, g1, g2, params=True, poses=True, kinv=True, outs=True, V=1, H=16, W=16, ws=True):
    p = _lib.Params()
    k = (ctypes.c_float * 9)(*([1.0] * 9))
    fake = ctypes.c_void_p(0x1000)              # never dereferenced: every refusal comes first
    nul = ctypes.c_void_p(0)
    return lib.ls2fm_render_image(ctypes.byref(f), ctypes.byref(g1), ctypes.byref(g2) if g2 is not None else None,
                                  ctypes.byref(p) if params else None, fake if poses else nul, V, k if kinv else None, H, W,
                                  fake if outs else nul, fake, fake, nul, fake if ws else nul, nul)


@pytest.mark.parametrize("case", ["outputs", "poses", "params", "views", "height", "width"])
def test_argument_refusals(case):
    lib = _lib.load()
    f, g = _descs()
    kw = {"outputs": dict(outs=False), "poses": dict(poses=False), "params": dict(params=False), "views": dict(V=0),
          "height": dict(H=0), "width": dict(W=-3)}[case]
    assert _call(lib, f, g, g, **kw) == -1          # LS2FM_ERR_INVALID_ARGUMENT


def test_unsupported_and_workspace_refusals():
    lib = _lib.load()
    f, g = _descs()
    f.bg_sdf = 1
    assert _call(lib, f, g, g) == -2                # LS2FM_ERR_UNSUPPORTED: bg_sdf
    assert lib.ls2fm_render_image_workspace_bytes(ctypes.byref(f), ctypes.byref(g), ctypes.byref(g)) == -2
    f.bg_sdf = 0
    _, g_other = _descs(levels=12)
    assert _call(lib, f, g, g_other) == -2          # dual grids of different geometry
    f, g = _descs(n_samples=640)
    assert _call(lib, f, g, g) == -2                # more samples than the shading kernels serve
    f, g = _descs()
    assert _call(lib, f, g, g, ws=False) == -4      # LS2FM_ERR_WORKSPACE
    assert lib.ls2fm_render_image_workspace_bytes(None, ctypes.byref(g), None) == -1
