"""The numpy model of the max-pool routing codes (tests/pool_codes_model.py) against a direct statement of what they mean: numpy's argmax
(the FIRST maximum) over the window in scan order, and the sign of the maximum.  Every ordering of four values in the four positions of a
2 x 2 window (4^4 windows per value set), and every pair for the 1 x 2 window; the value sets hold the ties that matter: equal positive
values, -0.0 against 0.0 (equal: the first wins, and neither is > 0) and windows without a positive element."""
import itertools

import numpy as np
import pytest

from pool_codes_model import pool_codes, unpack_codes, windows

VALUE_SETS = [(-1.0, -0.0, 0.0, 0.5), (-0.5, 0.0, 0.5, 1.0), (0.25, 0.25, 0.5, -2.0), (-3.0, -1.0, -0.0, -0.0)]


def _direct(win):
    """win [..., cnt, C] -> codes [..., C]: argmax-first | (max > 0) << 2."""
    return (np.argmax(win, axis=-2).astype(np.uint32) | ((np.max(win, axis=-2) > 0).astype(np.uint32) << 2))


@pytest.mark.parametrize("values", VALUE_SETS)
@pytest.mark.parametrize("kw,kh", [(2, 2), (1, 2)])
def test_codes_are_first_argmax_and_sign(values, kw, kh):
    cnt = kw * kh
    combos = np.array(list(itertools.product(values, repeat=cnt)), dtype=np.float32)        # [4^cnt, cnt]
    n = len(combos)
    assert n == 4 ** cnt
    # one window per (w block, channel): N = 1, W = kw * n / 8 windows along W, H = kh, C = 8 — window i, channel c holds combo (8 i + c) % n
    # rolled by c, so that the eight nibbles of a word differ
    nw = n // 8 if n >= 8 else 1
    x = np.zeros((1, kw * nw, kh, 8), dtype=np.float32)
    want = np.zeros((nw, 8), dtype=np.uint32)
    for i in range(nw):
        for c in range(8):
            combo = combos[(8 * i + c * 3) % n]
            for a in range(kw):
                for b in range(kh):
                    x[0, kw * i + a, b, c] = combo[a * kh + b]
            want[i, c] = int(np.argmax(combo)) | (4 if combo.max() > 0 else 0)
    words, code = pool_codes(x, kw, kh)
    assert words.dtype == np.uint32 and words.shape == (nw, 1)
    assert np.array_equal(code.reshape(nw, 8), want)
    assert np.array_equal(unpack_codes(words, 8), want)
    assert np.array_equal(_direct(windows(x, kw, kh)).reshape(nw, 8), want)
    # every combination was placed: (8 i + 3 c) mod n reaches all residues for n a power of two >= 8
    if n >= 8:
        assert len({(8 * i + c * 3) % n for i in range(nw) for c in range(8)}) == n


def test_all_orderings_against_direct():
    """All 4^4 windows of every value set at once, C = 16 (two words per window), against the direct form."""
    for values in VALUE_SETS:
        combos = np.array(list(itertools.product(values, repeat=4)), dtype=np.float32)      # [256, 4]
        rng = np.random.RandomState(7)
        perm = np.stack([rng.permutation(256) for _ in range(16)], axis=1)                  # channel c sees the windows in its own order
        w5 = combos[perm].transpose(0, 2, 1).reshape(2, 64, 2, 4, 16)                       # 2 x 64 x 2 = 256 windows [n, w, h, element, c]
        x = w5.reshape(2, 64, 2, 2, 2, 16).transpose(0, 1, 3, 2, 4, 5).reshape(2, 128, 4, 16)
        assert np.array_equal(windows(x, 2, 2), w5)
        words, code = pool_codes(x, 2, 2)
        assert words.shape == (256, 2)
        assert np.array_equal(code, _direct(w5))
        assert np.array_equal(unpack_codes(words, 16).reshape(code.shape), code)
        for c in range(16):                                                                 # every ordering occurs in every channel
            assert len(set(map(tuple, w5[..., c].reshape(256, 4)))) == len(set(map(tuple, combos)))


def test_negative_zero_ties_with_zero():
    x = np.array([-0.0, 0.0, 0.0, -0.0], dtype=np.float32).reshape(1, 2, 2, 1).repeat(8, axis=3)
    words, code = pool_codes(x, 2, 2)
    assert int(words[0, 0]) == 0 and not code.any()          # first element wins, nothing is > 0
    words, code = pool_codes(x, 1, 2)
    assert not words.any()
