"""The max-pool routing codes in numpy: what the training forward kernels write (conv1.hip's conv1_pool_pack / common.h's pool_code_word / conv_ws's ws_code_word) and
what maxpool_bwd_codes and the batch-norm backward passes read.  Shared by tests/test_pool_codes_model.py (CPU) and
tests/test_gpu_pool_codes.py.  Plain module, no GPU.

One uint32 per (pooled pixel, 8-channel group), channel c of the group at bits 4c .. 4c + 2: bits 0-1 the index of the window's FIRST maximum
in TF scan order (a * kh + b: a over W, b over H), bit 2 maximum > 0.  Layout [windows][C / 8], windows in (n, w / kw, h / kh) order."""
import numpy as np


def windows(x, kw, kh):
    """x [N, W, H, C] -> [N, W / kw, H / kh, kw * kh, C]: the elements of every window in scan order."""
    N, W, H, C = x.shape
    return x.reshape(N, W // kw, kw, H // kh, kh, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, W // kw, H // kh, kw * kh, C)


def pool_codes(x, kw, kh):
    """x: float array [N, W, H, C] holding the bf16 values the storing forward pass writes -> (codes uint32 [windows, C / 8], the 3-bit codes
    [N, W / kw, H / kh, C]).  pool_code_word restated: scan, replace on strictly greater."""
    win = windows(np.asarray(x, dtype=np.float32), kw, kh)
    best, bv = np.zeros(win[..., 0, :].shape, dtype=np.uint32), win[..., 0, :].copy()
    for e in range(1, kw * kh):
        gt = win[..., e, :] > bv
        best[gt], bv[gt] = e, win[..., e, :][gt]
    code = best | ((bv > 0).astype(np.uint32) << 2)
    C = code.shape[-1]
    words = (code.reshape(-1, C // 8, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(-1, dtype=np.uint32)
    return words, code


def unpack_codes(words, C):
    """uint32 [windows, C / 8] -> the 3-bit codes [windows, C]."""
    w = np.asarray(words).astype(np.uint32).reshape(-1, C // 8, 1)
    return ((w >> (4 * np.arange(8, dtype=np.uint32))) & 7).reshape(-1, C)
