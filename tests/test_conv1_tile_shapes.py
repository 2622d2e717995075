"""The inputs of tests/test_gpu_conv1_tile.py are decisive before a GPU sees them: under the fp64 reference alone (tests/conv1_reference.py)
the operands of the reference check leave at most AMBIGUOUS_CAP of the windows ambiguous at every shape, and the 1/64-grid operands of the
bit-for-bit check hold windows whose positive maximum is tied — where the first-maximum rule decides the code — and make every forward sum
exact in fp32, so tc.exact_forward is the device's result.  The committed slab words of the first generation
(tests/golden/conv1_pool_first_generation.npz) are complete and a valid gradient of those operands: a mis-recorded fixture fails here."""
import os
import sys

import numpy as np
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


@pytest.mark.parametrize("shape", tc.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_grid_operands_make_the_forward_exact(shape):
    """z = sum x w + b, computed in fp64, is an fp32 number, and so is every partial sum in any order: all terms are multiples of 2^-12 and
    the sum of their magnitudes stays below 2^5, i.e. within 17 of the 24 bits."""
    x, w, b = tc.grid_operands(*shape)
    for t in (x, w, b):
        assert np.array_equal(t * 64, np.round(t * 64))
    ref = cr.Reference(x, w, b)
    assert np.array_equal(ref.z, ref.z.astype(np.float32).astype(np.float64))
    bound = float(np.abs(x).max()) * float(np.abs(w).sum(0).max()) + float(np.abs(b).max())
    print('%s max|x| sum|w| + max|b| = %.4f' % (shape, bound))
    assert bound <= 17.5 and bound * 2 ** 12 < 2 ** 24
    pooled, codes = tc.exact_forward(shape)
    p = ref.pool()
    assert np.array_equal(pooled, cr.bf16_bits(p['pooled'])) and np.array_equal(codes, p['code']) and not (codes & 8).any()


@pytest.mark.parametrize("ppb", sorted(tc.PPBS))
def test_first_generation_fixture_is_a_valid_gradient(ppb):
    fx = np.load(tc.FIXTURE)
    assert sorted(fx.files) == sorted(tc.fixture_key(q, s, k) for q, shapes in tc.PPBS.items() for s in shapes
                                      for k in ('slab_codes', 'slab_recompute'))
    for shape in tc.PPBS[ppb]:
        Nb, W, H = shape
        npix = Nb * (W // 2) * (H // 2)
        ref = cr.Reference(*tc.grid_operands(*shape))
        bw = ref.backward_with(cr.make_dp((Nb, W // 2, H // 2, 64), 4), tc.exact_forward(shape)[1])
        for k in ('slab_codes', 'slab_recompute'):
            words = fx[tc.fixture_key(ppb, shape, k)]
            assert words.dtype == np.int32 and words.shape == (cr.ceil_div(npix, ppb), 640)
            slab = words.view(np.float32)
            assert not np.isnan(slab).any()
            worst = ref.check_backward(bw, *cr.slab_sums(slab), ppb, False)
            print('%s ppb %d %s %s' % (shape, ppb, k, worst))
            assert all(v <= 1.0 for v in worst.values()), (shape, ppb, k, worst)
