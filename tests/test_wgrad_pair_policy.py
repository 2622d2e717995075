"""When may two layers' 3x3 weight-gradient slab kernels share a launch — the host-only query ocr_conv3x3_wgrad_pair_supported (the policy
the paired launch itself asks: wgrad9.hip wgrad9_pair_ok), pinned without a GPU.  With no device visible the library counts the MI355X's
256 CUs, so "at most half the CUs" is 128 workgroups here."""
import ctypes
import os

import pytest

from lstm_ctc_ocr_amd import _native as nat
from lstm_ctc_ocr_amd import ops

pytestmark = pytest.mark.skipif(not os.path.exists(nat.LIB_PATH), reason="libocrhip.so not built")

CONV2, CONV3_1, CONV3_2 = (64, 128, 16, 64, 128), (64, 64, 8, 128, 256), (64, 64, 8, 256, 256)      # the 64 x 256 batch's layers
INVALID = 2         # OCR_ERR_INVALID


def _grid(shape):
    kernel, S = ops.conv3x3_wgrad_kernel_choice(*shape)
    return kernel, S * (shape[3] // 64) * (shape[4] // 64)


def test_headline_pair_is_supported():
    assert _grid(CONV2) == ('wgrad9', 128) and _grid(CONV3_1) == ('wgrad9p<8>', 256)
    assert ops.conv3x3_wgrad_pair_supported(CONV2, CONV3_1)
    # ... at every width of the variable-width workload (W = 80 .. 320 images: conv2 at 40 .. 160 columns), with each kind of partner
    for W in (40, 44, 80, 120, 160):
        assert ops.conv3x3_wgrad_pair_supported((64, W, 16, 64, 128), (64, W // 2, 8, 128, 256)), W
    assert ops.conv3x3_wgrad_pair_supported(CONV2, CONV2)                                   # wgrad9 + wgrad9
    assert ops.conv3x3_wgrad_pair_supported(CONV2, (64, 64, 4, 256, 512))                   # + wgrad9p<4>
    assert ops.conv3x3_wgrad_pair_supported(CONV2, (64, 80, 4, 256, 512))                   # + its zero-row instance
    assert ops.conv3x3_wgrad_pair_supported(CONV2, (64, 20, 8, 128, 256))                   # + wgrad9p<8>/zero-row


def test_refused_when_the_first_grid_exceeds_half_the_cus():
    full = (64, 128, 16, 128, 128)                  # H = 16: wgrad9_kernel, 4 tiles x 64 splits = 256 workgroups
    assert _grid(full) == ('wgrad9', 256)
    assert not ops.conv3x3_wgrad_pair_supported(full, CONV3_1)
    assert ops.conv3x3_wgrad_pair_supported((64, 128, 16, 64, 64), full)          # 64 workgroups in front: room for any second job


def test_refused_when_a_shape_is_no_slab_shape():
    no_slab = (64, 128, 16, 32, 128)                # Cin % 64 != 0: gemm_tn2 / gemm_tn
    assert ops.conv3x3_wgrad_workspace_bytes(*no_slab) == 0
    assert not ops.conv3x3_wgrad_pair_supported(no_slab, CONV3_1)
    assert not ops.conv3x3_wgrad_pair_supported(CONV2, no_slab)
    assert not ops.conv3x3_wgrad_pair_supported(CONV2, (1, 8, 16, 64, 128))       # fewer than 512 pixels


def test_refused_without_an_instance_for_the_two_kernels():
    """The paired instances have wgrad9_kernel's body in front.  A plane-layout kernel in front has none, however small its grid — with an
    H = 2 layer (always wgrad9_kernel) behind it as with anything else; the other way round the pair exists."""
    h2, plane = (64, 64, 2, 64, 64), (4, 32, 4, 64, 64)
    assert _grid(h2)[0] == 'wgrad9' and _grid(plane) == ('wgrad9p<4>', 1)
    assert not ops.conv3x3_wgrad_pair_supported(plane, h2)
    assert not ops.conv3x3_wgrad_pair_supported(plane, plane)
    assert not ops.conv3x3_wgrad_pair_supported(CONV3_1, CONV2)
    assert ops.conv3x3_wgrad_pair_supported(h2, plane)


def test_wgrad_engine_without_slab_kernels_has_no_pairs():
    try:
        nat.call("ocr_set_wgrad_engine", 1)
        assert not ops.conv3x3_wgrad_pair_supported(CONV2, CONV3_1)
    finally:
        nat.call("ocr_set_wgrad_engine", int(os.environ.get("OCR_WGRAD_ENGINE") or 2))
    assert ops.conv3x3_wgrad_pair_supported(CONV2, CONV3_1)


def test_argument_validation():
    lib = nat.lib()
    arr = lambda s: (ctypes.c_int * 5)(*s)          # noqa: E731
    assert lib.ocr_conv3x3_wgrad_pair_supported(None, arr(CONV3_1)) == -INVALID
    assert lib.ocr_conv3x3_wgrad_pair_supported(arr(CONV2), None) == -INVALID
    assert lib.ocr_conv3x3_wgrad_pair_supported(arr((0, 128, 16, 64, 128)), arr(CONV3_1)) == -INVALID
    assert lib.ocr_conv3x3_wgrad_pair_supported(arr(CONV2), arr((64, 64, 8, 124, 256))) == -INVALID       # channels % 8
    with pytest.raises(nat.NativeError):
        ops.conv3x3_wgrad_pair_supported(CONV2, (64, 64, -8, 128, 256))
    # the launch validates before it touches anything: null operands, null job slots and bad shapes are OCR_ERR_INVALID (no GPU needed)
    job, nblk = (ctypes.c_ubyte * 64)(), ctypes.c_int(0)
    jp, np_ = ctypes.cast(job, ctypes.c_void_p), ctypes.byref(nblk)
    a, b = arr(CONV2), arr(CONV3_1)
    assert lib.ocr_conv3x3_wgrad_pair_defer_bf16(None, None, None, None, a, None, 0, None, None, None, None, b, None, 0, jp, jp, np_, np_, None) == INVALID
    assert lib.ocr_conv3x3_wgrad_pair_defer_bf16(64, 64, 64, None, a, 64, 1 << 30, 64, 64, 64, None, b, 64, 1 << 30, None, jp, np_, np_, None) == INVALID
    assert lib.ocr_conv3x3_wgrad_pair_defer_bf16(64, 64, 64, None, None, 64, 1 << 30, 64, 64, 64, None, b, 64, 1 << 30, jp, jp, np_, np_, None) == INVALID
    # ... and so are a pair the policy refuses and a workspace smaller than ocr_conv3x3_wgrad_workspace_size: nothing is launched
    assert lib.ocr_conv3x3_wgrad_pair_defer_bf16(64, 64, 64, None, b, 64, 1 << 30, 64, 64, 64, None, a, 64, 1 << 30, jp, jp, np_, np_, None) == INVALID
    assert lib.ocr_conv3x3_wgrad_pair_defer_bf16(64, 64, 64, None, a, 64, 16, 64, 64, 64, None, b, 64, 1 << 30, jp, jp, np_, np_, None) == INVALID
