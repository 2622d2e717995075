"""-m gpu: ops.conv3x3_dgrad_unpool — a data gradient with the backward pass of the max-pool in front in conv_k3's write-out — bit for bit
against the unfused pair ops.conv3x3(dy, wd) -> ops.maxpool_bwd_codes(codes, ., kw, kh, relu_mask), both unchanged code that
tests/test_gpu_pool_codes.py checks against CPU references.

The shapes are the smallest at which each instance and index path runs: one 256-pixel tile per image, two (interior and edge tiles), image
boundaries between tiles; tile D, tile A and a second channel tile; one and two 64-channel chunks of the contraction; both windows at both H.
At these sizes the plain ops.conv3x3 of the pair runs another kernel family than conv_k3 (the tap-reuse kernels start at 4096 pixels), whose
fp32 sums are added in another order: the operands are therefore multiples of 1/2 (|dy| <= 2) and 1/8 (|w| <= 1/2), so every partial sum of the
at most 1152 products is a multiple of 1/16 below 2^11 — exact in fp32 in any order — and the bf16 rounding is the only rounding there is.  One case at a product shape, where both sides run the same conv_k3 instance,
uses normally distributed operands.

No tolerances: every comparison is on the bit patterns, and out_full starts as NaN so that an unwritten byte shows."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from test_gpu_memory_bound_kernels import _assert_bits_equal  # noqa: E402
from unpool_model import unpool  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from lstm_ctc_ocr_amd._native import NativeError  # noqa: E402

BF = torch.bfloat16
SHAPES = [(1, 64, 4), (2, 128, 4), (2, 64, 8), (3, 32, 8)]          # pooled (Nb, W, H)
WINDOWS = [(1, 2), (2, 2)]


def _nan(shape, dev):
    return torch.full(shape, float('nan'), dtype=BF, device=dev)


def _exact_operands(Nb, W, H, Ci, Co, seed, dev):
    g = torch.Generator().manual_seed(seed)
    dy = (torch.randint(-4, 5, (Nb, W, H, Ci), generator=g).float() * 0.5).to(BF).to(dev)
    wd = (torch.randint(-4, 5, (Co, 3, 3, Ci), generator=g).float() * 0.125).to(BF).to(dev)
    return dy, wd


def _code_sets(M, Co, kw, kh, seed):
    """name -> uint32 words [M, Co / 8]: random valid codes; all zero; every channel on the LAST window element with the ReLU bit clear."""
    rng = np.random.RandomState(seed)
    code = rng.randint(0, kw * kh, size=(M, Co // 8, 8)).astype(np.uint32) | (rng.randint(0, 2, size=(M, Co // 8, 8)).astype(np.uint32) << 2)
    shifts = 4 * np.arange(8, dtype=np.uint32)
    last = np.full((M, Co // 8, 8), kw * kh - 1, dtype=np.uint32)
    return {"random": (code << shifts).sum(-1, dtype=np.uint32), "zero": np.zeros((M, Co // 8), dtype=np.uint32),
            "last, relu clear": (last << shifts).sum(-1, dtype=np.uint32)}


def _codes_dev(words, dev):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)


def _compare(what, dy, wd, codes, kw, kh, dev, pooled=None):
    Nb, W, H, _ = dy.shape
    Co = wd.shape[0]
    if pooled is None:
        pooled = ops.conv3x3(dy, wd, out=_nan((Nb, W, H, Co), dev))
    for relu_mask in (0, 1):
        want = ops.maxpool_bwd_codes(codes, pooled, kw, kh, relu_mask, out=_nan((Nb, W * kw, H * kh, Co), dev))
        got = ops.conv3x3_dgrad_unpool(dy, wd, codes, kw, kh, relu_mask, out=_nan((Nb, W * kw, H * kh, Co), dev))
        _assert_bits_equal("%s relu_mask=%d" % (what, relu_mask), got, want)
    return pooled


@pytest.mark.parametrize("Co", [64, 128, 192])
@pytest.mark.parametrize("Ci", [64, 128])
@pytest.mark.parametrize("kw,kh", WINDOWS)
@pytest.mark.parametrize("shape", SHAPES)
def test_unpool_dgrad_equals_dgrad_then_maxpool_bwd_codes(dev, shape, kw, kh, Ci, Co):
    Nb, W, H = shape
    assert ops.conv3x3_unpool_supported(Nb, W, H, Ci, Co, kw, kh)
    dy, wd = _exact_operands(Nb, W, H, Ci, Co, 1000 * W + 10 * H + Ci + Co, dev)
    pooled = None
    for name, words in sorted(_code_sets(Nb * W * H, Co, kw, kh, W + Co).items()):
        pooled = _compare("%s %dx%d Ci=%d Co=%d codes: %s" % (shape, kw, kh, Ci, Co, name), dy, wd, _codes_dev(words, dev), kw, kh, dev, pooled)
    p = pooled.float().cpu()
    assert bool(torch.isfinite(p).all()) and float((p != 0).float().mean()) > 0.9       # the gradient that is routed is not a tensor of zeros
    # ... and, once per case, the numpy model of the index map on the random codes (tests/test_unpool_model.py checks the model on the CPU)
    words = _code_sets(Nb * W * H, Co, kw, kh, W + Co)["random"]
    got = ops.conv3x3_dgrad_unpool(dy, wd, _codes_dev(words, dev), kw, kh, 1, out=_nan((Nb, W * kw, H * kh, Co), dev))
    bits = pooled.cpu().view(torch.int16).numpy().view(np.uint16).reshape(Nb * W * H, Co)
    assert np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16).reshape(-1, Co), unpool(bits, words, Nb, W, H, kw, kh, True))


# full-resolution forward shapes (N, W, H, Cin, Cout) whose fused pool writes codes and whose pooled shape the unpool instances take
FORWARD_CANDIDATES = [(8, 128, 8, 128, 256), (8, 128, 16, 128, 256), (16, 128, 8, 128, 256)]


@pytest.mark.parametrize("kw,kh", WINDOWS)
def test_unpool_dgrad_with_the_codes_of_a_forward_pass(dev, kw, kh):
    """Codes as a training forward pass leaves them (small-integer inputs: many exact ties and all-non-positive windows)."""
    for N, W, H, Cf, Co in FORWARD_CANDIDATES:
        if ops.conv3x3_pool_codes_supported(N, W, H, Cf, Co, kw, kh) and ops.conv3x3_unpool_supported(N, W // kw, H // kh, 64, Co, kw, kh):
            break
    else:
        pytest.fail("no candidate shape has both the codes write-out and the unpool write-out for a %d x %d pool" % (kw, kh))
    g = torch.Generator().manual_seed(N + W + kw)
    x = (torch.randint(-2, 3, (N, W, H, Cf), generator=g).float() * 0.5).to(BF).to(dev)
    w = (torch.randint(-1, 2, (Co, 3, 3, Cf), generator=g).float() * 0.125).to(BF).to(dev)
    b = (torch.randint(-2, 3, (Co,), generator=g).float() * 0.25).to(dev)
    Wp, Hp = W // kw, H // kh
    codes = torch.full((N * Wp * Hp, Co // 8), -1, dtype=torch.int32, device=dev)
    ops.conv3x3_relu_pool_codes(x, w, None, _nan((N, Wp, Hp, Co), dev), codes, b, kw, kh)
    c = codes.cpu().numpy().view(np.uint32)
    idx = (c[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & 3
    assert ((c & 0x88888888) == 0).all() and (idx < kw * kh).all() and len(np.unique(idx)) == kw * kh
    assert 0.05 < ((c & 0x44444444) != 0x44444444).mean()                               # windows without a positive element exist
    dy, wd = _exact_operands(N, Wp, Hp, 64, Co, 77, dev)
    _compare("forward codes %s %dx%d" % ((N, W, H, Cf, Co), kw, kh), dy, wd, codes, kw, kh, dev)


PRODUCT_CANDIDATES = [(64, 64, 8, 256, 128), (64, 64, 4, 512, 256), (32, 128, 8, 256, 128)]


@pytest.mark.parametrize("kw,kh", WINDOWS)
def test_unpool_dgrad_at_a_product_shape_with_normal_operands(dev, kw, kh):
    """Where the plain data gradient itself runs an aligned-width conv_k3 kernel (the condition under which the engine uses the unpool form)
    both sides run the same instance up to the write-out: arbitrary operands, the same bits."""
    for Nb, W, H, Ci, Co in PRODUCT_CANDIDATES:
        if (ops.conv3x3_kernel_choice(Nb, W, H, Ci, Co, bias=False, relu=False) in ("conv_k3/A", "conv_k3/D")
                and ops.conv3x3_unpool_supported(Nb, W, H, Ci, Co, kw, kh)):
            break
    else:
        pytest.fail("no candidate data gradient is planned on an aligned-width conv_k3 kernel")
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(Nb, W, H, Ci, generator=g).to(BF).to(dev)
    wd = (torch.randn(Co, 3, 3, Ci, generator=g) * 0.05).to(BF).to(dev)
    words = _code_sets(Nb * W * H, Co, kw, kh, 3)["random"]
    _compare("product %s %dx%d" % ((Nb, W, H, Ci, Co), kw, kh), dy, wd, _codes_dev(words, dev), kw, kh, dev)


@pytest.mark.parametrize("shape", [(2, 80, 4, 64, 64), (8, 128, 2, 64, 64), (2, 128, 4, 64, 72)])
def test_shapes_without_an_instance_are_refused_and_launch_nothing(dev, shape):
    Nb, W, H, Ci, Co = shape
    for kw, kh in WINDOWS:
        assert not ops.conv3x3_unpool_supported(Nb, W, H, Ci, Co, kw, kh)
        dy = torch.zeros((Nb, W, H, Ci), dtype=BF, device=dev)
        wd = torch.zeros((Co, 3, 3, Ci), dtype=BF, device=dev)
        codes = torch.zeros((Nb * W * H, Co // 8), dtype=torch.int32, device=dev)
        out = _nan((Nb, W * kw, H * kh, Co), dev)
        with pytest.raises(NativeError, match="invalid value"):
            ops.conv3x3_dgrad_unpool(dy, wd, codes, kw, kh, 0, out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.float()).all())
