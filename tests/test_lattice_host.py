"""CPU: ls2fm/lattice.py, the dense lattice under ls2fm.fusion and ls2fm.cloud_mesh -- its shaping rule against literal shapes, its
torch form of the lattice points against the numpy restatement (tests/fusion_restate.lattice, which tests/cloud_mesh_restate.py
uses too) by their bits, and its default bounds against a box computed by hand.  The restatement itself is held, element by
element, to the scalar expression fl32(fl32((float) i * voxel) + origin)."""
import numpy as np
import pytest
import torch

import cloud_mesh_restate as CR
import fusion_restate as FR
from ls2fm import lattice

F32 = np.float32
# (shape, origin, voxel): dyadic; not dyadic with a side of 1 and one of 65; large coordinates; a single point; an empty lattice
FRAMES = (((3, 4, 5), (0.0, 0.0, 0.0), 0.25), ((7, 1, 65), (-0.35, 0.2, 1e-3), 0.1), ((65, 2, 3), (1e3, -7.77, 0.3333), 0.0123),
          ((1, 1, 1), (0.1, 0.2, 0.3), 3.0), ((0, 3, 4), (0.0, 1.0, 2.0), 0.5))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("shape, origin, voxel", FRAMES)
def test_the_restatement_is_the_scalar_expression_and_the_torch_form_has_its_bits(shape, origin, voxel):
    X = FR.lattice(shape, origin, voxel)
    assert CR.lattice_points is FR.lattice and X.dtype == F32 and X.shape == (int(np.prod(shape)), 3)
    index = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), axis=-1).reshape(-1, 3)       # axis 2 fastest
    want = np.array([[F32(F32(F32(i) * F32(voxel)) + F32(o)) for i, o in zip(row, origin)] for row in index], F32).reshape(-1, 3)
    assert np.array_equal(bits(X), bits(want))
    got = torch.stack(lattice.points(shape, origin, voxel, "cpu"), dim=1)
    assert got.dtype == torch.float32 and np.array_equal(bits(got.numpy()), bits(X))


def test_the_shaping_rule():
    """the expected shapes are those ls2fm.fusion.volume_for and ls2fm.cloud_mesh._lattice gave, in agreement, before the rule
    moved here: a multiple of the voxel, a non-multiple, a non-dyadic box with high == low on an axis, a point, a general box"""
    cases = ((((0, 0, 0), (1, 2, 3)), 0.25, (5, 9, 13)), (((0, 0, 0), (1, 2, 3)), 0.3, (5, 8, 11)),
             (((-0.35, 0.2, 1e-3), (0.65, 0.2, 0.5)), 0.1, (11, 2, 6)), (((1, 1, 1), (1, 1, 1)), 0.5, (2, 2, 2)),
             (((-1, -2, -3), (1.5, 0.25, -2.9)), 0.07, (37, 34, 3)))
    for bounds, voxel, shape in cases:
        assert lattice.shape_for(bounds, voxel, "refused") == (shape, tuple(float(v) for v in bounds[0]))
    for bounds, voxel in ((cases[0][0], 0.0), (cases[0][0], float("inf")), (cases[0][0], float("nan")), (((0, 0, 0), (1, float("nan"), 1)), 0.1),
                          (((0, 0, 0), (1, float("inf"), 1)), 0.1), (((0, 0), (1, 1)), 0.1)):
        with pytest.raises(ValueError, match="^who: 0.0 and 1.0 with"):
            lattice.shape_for(bounds, voxel, "who: {lo[0]} and {hi[0]} with {voxel}")


def test_the_default_bounds():
    x = torch.tensor([[0.5, -2.0, 3.0], [1.5, 4.0, -1.0], [-0.25, 0.0, 0.0]])
    assert lattice.grown_box(x, 0.5) == ([-0.75, -2.5, -1.5], [2.0, 4.5, 3.5])
    assert lattice.grown_box(x[:1], 0.0) == ([0.5, -2.0, 3.0], [0.5, -2.0, 3.0])
