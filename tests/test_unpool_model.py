"""CPU: the flat-row index algebra of conv_k3's unpool write-out (tests/unpool_model.py restates it) against the window layout of
tests/pool_codes_model.py, for both windows, on the shapes tests/test_gpu_unpool_dgrad.py runs — every (m, a, b) -> full-resolution row,
across image boundaries — and the routing decision against the model's codes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pool_codes_model import pool_codes, unpack_codes, windows  # noqa: E402
from unpool_model import full_row, unpool  # noqa: E402

SHAPES = [(1, 64, 4), (2, 128, 4), (2, 64, 8), (3, 32, 8)]          # pooled (Nb, W, H)


@pytest.mark.parametrize("kw,kh", [(1, 2), (2, 2)])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_window_element_lands_on_its_full_resolution_row(shape, kw, kh):
    Nb, W, H = shape
    rows = np.arange(Nb * W * kw * H * kh, dtype=np.float64).reshape(Nb, W * kw, H * kh, 1)        # a tensor that holds its own row numbers
    want = windows(rows, kw, kh).reshape(Nb * W * H, kw * kh).astype(np.int64)                   # [window m][cnt = a * kh + b]
    m = np.arange(Nb * W * H)
    for a in range(kw):
        for b in range(kh):
            got = full_row(m, a, b, H, kw, kh)
            assert np.array_equal(got, want[:, a * kh + b]), (shape, kw, kh, a, b)
    assert np.array_equal(np.sort(want.flatten()), np.arange(want.size))                         # a bijection onto the full-resolution rows


@pytest.mark.parametrize("relu_mask", [False, True])
@pytest.mark.parametrize("kw,kh", [(1, 2), (2, 2)])
@pytest.mark.parametrize("shape", SHAPES[:1] + SHAPES[3:])
def test_routing_equals_the_pool_backward_on_the_stored_tensor(shape, kw, kh, relu_mask):
    """unpool(...) from the codes of x against the max-pool backward written out on x itself (first maximum in scan order; relu_mask: > 0)."""
    Nb, W, H = shape
    C = 16
    rng = np.random.RandomState(Nb * 100 + W + kw)
    x = rng.randint(-2, 3, size=(Nb, W * kw, H * kh, C)).astype(np.float32) * 0.5      # coarse: ties and non-positive windows are common
    g = rng.randint(1, 0x7f80, size=(Nb * W * H, C)).astype(np.uint16)                 # non-zero bit patterns of finite bf16 values
    words, code = pool_codes(x, kw, kh)
    assert np.array_equal(unpack_codes(words, C), code.reshape(-1, C))
    win = windows(x, kw, kh).reshape(Nb * W * H, kw * kh, C)
    first = np.argmax(win, axis=1)                                                     # numpy: the FIRST maximum
    keep = np.arange(kw * kh).reshape(1, -1, 1) == first[:, None, :]
    if relu_mask:
        keep &= (win.max(axis=1) > 0)[:, None, :]
    dwin = np.where(keep, g[:, None, :], np.uint16(0))                                 # [window][cnt][C]
    rows = windows(np.arange(Nb * W * kw * H * kh, dtype=np.float64).reshape(Nb, W * kw, H * kh, 1), kw, kh).reshape(-1).astype(np.int64)
    want = np.empty((Nb * W * kw * H * kh, C), dtype=np.uint16)
    want[rows] = dwin.reshape(-1, C)
    got = unpool(g, words, Nb, W, H, kw, kh, relu_mask)
    assert np.array_equal(got, want)
    assert (got != 0).any() and (got == 0).any()
