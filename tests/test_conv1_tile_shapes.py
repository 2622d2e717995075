"""The inputs of tests/test_gpu_conv1_tile.py are decisive before a GPU sees them: under the fp64 reference alone (tests/conv1_reference.py)
the operands of the reference check leave at most AMBIGUOUS_CAP of the windows ambiguous at every shape, and the 1/64-grid operands of the
generation-against-generation check hold windows whose positive maximum is tied — where the first-maximum rule decides the code."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1_reference as cr  # noqa: E402
import conv1_tile_cases as tc  # noqa: E402


@pytest.mark.parametrize("shape", tc.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_reference_operands_are_decisive(shape):
    amb, _ = cr.Reference(*tc.reference_operands(*shape)).shares()
    print('%s ambiguous %.4f' % (shape, amb))
    assert amb <= cr.AMBIGUOUS_CAP


@pytest.mark.parametrize("shape", tc.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_grid_operands_hold_tied_positive_maxima(shape):
    share = tc.tied_positive_share(*tc.grid_operands(*shape))
    print('%s tied positive maxima %.4f' % (shape, share))
    assert share > 0.0
