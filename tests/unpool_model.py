"""The index map of conv_k3's unpool write-out in numpy (plain module, no GPU): which full-resolution row receives window element (a, b) of
pooled pixel m, as the kernel computes it from flat row numbers — shared by tests/test_unpool_model.py (CPU) and tests/test_gpu_unpool_dgrad.py.

Pooled tensor [Nb, W, H, C] as rows m = (n * W + w) * H + h; full-resolution tensor [Nb, W * kw, H * kh, C] as rows of C channels."""
import numpy as np


def full_row(m, a, b, H, kw, kh):
    """Row of the full-resolution tensor for element (a, b) of the window of pooled row m (arrays broadcast).  H: POOLED feature rows."""
    m = np.asarray(m, dtype=np.int64)
    if (kw, kh) == (1, 2):
        return 2 * m + b
    assert (kw, kh) == (2, 2)
    col, h = m // H, m % H                       # col counts the columns of the whole batch: image n = col // W, w = col % W
    return (2 * col + a) * (2 * H) + 2 * h + b


def unpool(g, words, Nb, W, H, kw, kh, relu_mask):
    """g: the pooled gradient as uint16 bit patterns [Nb * W * H, C]; words: uint32 [Nb * W * H, C / 8] -> the full-resolution gradient's bit
    patterns [Nb * W * kw * H * kh, C], every row written exactly once: element cnt = a * kh + b of a window receives g's bits where the
    channel's code names it (and, relu_mask, its ReLU bit is set), else +0."""
    M, C = g.shape
    assert M == Nb * W * H and words.shape == (M, C // 8)
    code = (words.astype(np.uint32).reshape(M, C // 8, 1) >> (4 * np.arange(8, dtype=np.uint32))).reshape(M, C) & 7
    out = np.full((M * kw * kh, C), 0xffff, dtype=np.uint16)
    hits = np.zeros(M * kw * kh, dtype=np.int64)
    m = np.arange(M)
    for a in range(kw):
        for b in range(kh):
            keep = (code & 3) == a * kh + b
            if relu_mask:
                keep &= (code & 4) != 0
            rows = full_row(m, a, b, H, kw, kh)
            out[rows] = np.where(keep, g, np.uint16(0))
            np.add.at(hits, rows, 1)
    assert (hits == 1).all(), "the map does not cover every full-resolution row exactly once"
    return out
