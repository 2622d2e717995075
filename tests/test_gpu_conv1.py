"""-m gpu: the first layer's kernels (csrc/conv1.hip: conv1_fwd, conv1_wgrad, conv1_pool_fwd with and without routing codes, conv1_pool_bwd
in its atomics and slab forms, with saved codes and with recomputed windows) against the fp64 reference of tests/conv1_reference.py, on
rendered captchas under the trained taps — where one window in five holds a positive maximum shared by several elements and the first-
maximum rule decides where the gradient goes — beside the uniform random regime, perturbed taps and constant images.  The bounds, their
derivation and what "ambiguous" means are in that module's docstring; tests/test_conv1_reference.py pins the checker without a GPU.

c = 10 / (1 - 10 u), u = 2^-24 (nine fmas from zero and the bias add).  k = ppb / 32 + 3 + 3 [+ blocks for atomics]: 14 for the slab form at
the default 256 pooled pixels per block (7 at OCR_CONV1_PPB=32, 38 at 1024), 14 + ceil(npix / 256) for the atomics form (294 at V0[:28]),
38 + ceil(npix / 1024) for conv1_wgrad (108 at V0[:7]).  Every asserted limit is 1.

Shares per regime (ambiguous windows / positive-maximum ties among the unambiguous ones; a property of the reference, measured on the CPU):
    captcha    C1 2.2 % / 11.9 %    V0[:28] 1.4 % / 20.7 %    crop (3, 30, 12) 2.2 % / 2.5 %
    perturbed  C1 2.8 % / 11.6 %    V0[:28] 1.6 % / 20.6 %    crop (3, 30, 12) 2.1 % / 2.4 %
    random     (3, 30, 12) 0.8 % / 0.3 %        zeros  0 % / 28.1 %        ones  (3, 30, 12) 0 % / 38.3 %

Worst |device - reference| / bound.  NOT YET MEASURED ON AN MI355X: no device could be had while this file was written, so the figures
below are those of the numpy fp32 model of the kernels (tests/test_conv1_reference.py), which performs the same fp32 operations in the
same order; the first run on the device has to replace them.
    conv1_fwd            y 1.000 with and without the ReLU (a value next to a rounding midpoint: the half ulp itself, as it should be)
    conv1_wgrad          dw 0.048  db 0.001                     (worst at (2, 6, 2); C1: dw 0.0016 db 0.0009)
    pool_fwd, codes      pooled 0.999  exact 0  codes 0  choice 0.96  relu_bit 0
    pool_bwd atomics     dw 0.10  db 0.001                      (worst at (2, 6, 2); C1: dw 0.034)
    pool_bwd slab        dw 0.12  db 0.0006                     (worst at (2, 6, 2); C1: dw 0.034)
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1_reference as cr  # noqa: E402

from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                          # poisoned rows behind every output
POISON = {BF: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC00001), I32: (torch.int32, -1)}       # NaNs; all code bits set
ERR_INVALID = 2


def _np(t):
    return (t.float() if t.dtype == BF else t).cpu().numpy()


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _bf(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(BF)


class Guarded:
    """rows x cols of poison with GUARD more rows behind them; .t is the view a kernel gets, intact() whether the rows behind it (or, with
    whole=True, all of it) still hold the poison."""

    def __init__(self, dev, rows, cols, dtype, shape=None):
        self.as_int, self.pattern = POISON[dtype]
        self.buf = torch.empty((rows + GUARD, cols), dtype=dtype, device=dev)
        self.buf.view(self.as_int).fill_(self.pattern)
        self.rows = rows
        self.t = self.buf[:rows] if shape is None else self.buf[:rows].view(shape)

    def intact(self, whole=False):
        torch.cuda.synchronize()
        return bool((self.buf[0 if whole else self.rows:].view(self.as_int) == self.pattern).all())


def _ppb():
    """Pooled pixels per block of the slab form as the library reads it: OCR_CONV1_PPB if it is a multiple of 32 in [32, 1024], else 256."""
    try:
        v = int(os.environ.get('OCR_CONV1_PPB', '256'))
    except ValueError:
        v = 0
    return v if 32 <= v <= 1024 and v % 32 == 0 else 256


def _assert(name, what, worst):
    print('%-18s %-22s %s' % (name, what, '  '.join('%s %.3g' % kv for kv in sorted(worst.items()))), flush=True)
    assert all(v <= 1.0 for v in worst.values()), (name, what, worst)


def _full_resolution(dev, name, ref, x, w, b, wgrad=True):
    Nb, W, H = x.shape
    Co = ref.Co
    xd, wd, bd = _dev(dev, x, w, b)
    for relu in (True, False):
        y = Guarded(dev, Nb * W * H, Co, BF, (Nb, W, H, Co))
        ops.conv1_fwd(xd, wd, bd, relu=relu, out=y.t)
        assert y.intact()
        _assert(name, 'conv1_fwd relu=%d' % relu, dict(y=ref.check_full(_np(y.t), relu)))
    if wgrad:
        dz = cr.make_dp((Nb, W, H, Co), 5)
        dw = torch.zeros((9, Co), device=dev); db = torch.zeros(Co, device=dev)
        ops.conv1_wgrad(xd, _bf(dev, dz), dw, db)
        _assert(name, 'conv1_wgrad', ref.check_wgrad(dz, _np(dw), _np(db)))


@pytest.mark.parametrize("name", [n for n in cr.CASES if not n.endswith('-V0')] + list(cr.FULL_ONLY))
def test_conv1_fwd_and_wgrad(dev, name):
    """conv1_fwd with and without the ReLU, every element against its own bound; conv1_wgrad against a given bf16 dz.  captcha-V0x7 has 71680
    pixels: the grid-stride loop of conv1_fwd (65536 pixels per sweep) makes a second pass, conv1_wgrad runs 70 blocks."""
    x, w, b = cr.case_operands(name)
    _full_resolution(dev, name, cr.Reference(x, w, b), x, w, b)


@pytest.mark.parametrize("name", list(cr.CASES))
def test_conv1_pool_kernels(dev, name):
    """The fused pair: the pooled map (plain launch and training launch alike), the routing codes, and the four backward launches (atomics /
    slab, saved codes / recomputed windows) against the reference that takes the device's code in ambiguous windows only."""
    x, w, b = cr.case_operands(name)
    ref = cr.Reference(x, w, b)
    amb, tie = ref.shares()
    assert amb <= cr.AMBIGUOUS_CAP and (tie >= cr.TIE_FLOOR or name not in cr.BATCH_CASES)
    Nb, W, H = x.shape
    Wo, Ho, Co = W // 2, H // 2, 64
    npix = Nb * Wo * Ho
    xd, wd, bd = _dev(dev, x, w, b)
    # forward, plain
    p = Guarded(dev, npix, Co, BF, (Nb, Wo, Ho, Co))
    ops.conv1_pool_fwd(xd, wd, bd, out=p.t)
    assert p.intact()
    _assert(name, 'pool_fwd', ref.check_pooled(_np(p.t)))
    # forward, training: codes, and the two fills touch exactly their words
    p2 = Guarded(dev, npix, Co, BF, (Nb, Wo, Ho, Co))
    codes = Guarded(dev, npix, 8, I32)
    junk = torch.full((4096 + 8,), 7.0, device=dev)
    ones = torch.zeros(4096 + 64, dtype=I32, device=dev)
    ops.conv1_pool_fwd(xd, wd, bd, out=p2.t, zero=junk[4:4100], codes=codes.t, ones=ones[8:4104])
    assert p2.intact() and codes.intact() and torch.equal(p2.t, p.t)
    assert float(junk[4:4100].abs().max()) == 0.0 and bool((junk[:4] == 7.0).all()) and bool((junk[4100:] == 7.0).all())
    assert bool((ones[8:4104] == -1).all()) and bool((ones[:8] == 0).all()) and bool((ones[4104:] == 0).all())
    cn = codes.t.cpu().numpy()
    _assert(name, 'pool_fwd codes', ref.check_pooled(_np(p2.t), cn))
    # backward
    dp = cr.make_dp((Nb, Wo, Ho, Co), 4)
    dpd = _bf(dev, dp)
    ppb = _ppb()
    rows = ops.conv1_pool_bwd_slab_rows(Nb, W, H)
    assert rows == cr.ceil_div(npix, ppb)
    print('slab: ppb=%d rows=%d' % (ppb, rows))
    bw = ref.backward(dp, cn)
    slabs = []
    for cd, tag in ((codes.t, 'codes'), (None, 'recompute')):
        dw = torch.zeros((9, Co), device=dev); db = torch.zeros(Co, device=dev)
        ops.conv1_pool_bwd(xd, wd, bd, dpd, dw, db, codes=cd)
        _assert(name, 'pool_bwd atomics ' + tag, ref.check_backward(bw, _np(dw), _np(db), cr.ATOMICS_PPB, True))
        slab = Guarded(dev, rows, 640, F32)                                    # NaN in every word before the call
        ops.conv1_pool_bwd_slab(xd, wd, bd, dpd, slab.t, codes=cd)
        assert slab.intact()
        dws, dbs = cr.slab_sums(_np(slab.t))
        _assert(name, 'pool_bwd slab ' + tag, ref.check_backward(bw, dws, dbs, ppb, False))
        slabs.append(slab.t)
    assert torch.equal(slabs[0], slabs[1])                                     # the same terms in the same order


@pytest.mark.parametrize("Co", [8, 128])
def test_other_filter_counts(dev, Co):
    """Cout the engine never passes: one channel group per thread row (8) and sixteen (128), on (3, 30, 12)."""
    x, w, b = cr.random_operands(3, 30, 12, Co=Co, seed=7)
    ref = cr.Reference(x, w, b)
    name = 'random-3x30x12-Co%d' % Co
    _full_resolution(dev, name, ref, x, w, b, wgrad=False)
    xd, wd, bd = _dev(dev, x, w, b)
    p = Guarded(dev, 3 * 15 * 6, Co, BF, (3, 15, 6, Co))
    ops.conv1_pool_fwd(xd, wd, bd, out=p.t)
    assert p.intact()
    _assert(name, 'pool_fwd', ref.check_pooled(_np(p.t)))


def test_refused_calls_leave_the_outputs_alone(dev):
    """What the entry points refuse: the error comes back and no output word is written.  Every buffer is large enough for the shape the
    call names, so a call that was wrongly accepted would show in the poison and not as a fault."""
    lib = nat.lib()
    Nb, W, H = 3, 30, 12
    st = nat.stream()
    x = torch.rand((Nb, W + 1, H + 1), device=dev)
    w = torch.rand((9, 128), device=dev); b = torch.rand(128, device=dev)
    big = Nb * (W + 1) * (H + 1)
    y = Guarded(dev, big, 128, BF)
    codes = Guarded(dev, big, 16, I32)
    fill = Guarded(dev, 64, 4, F32)
    dw = Guarded(dev, 9, 128, F32); db = Guarded(dev, 1, 128, F32); slab = Guarded(dev, 16, 640, F32)
    dz = torch.zeros((big, 128), dtype=BF, device=dev)
    good_codes = torch.zeros((big, 16), dtype=I32, device=dev)
    X, Wt, B, Y, C, DZ = x.data_ptr(), w.data_ptr(), b.data_ptr(), y.t.data_ptr(), codes.t.data_ptr(), dz.data_ptr()
    Z, DW, DB, SL, GC = fill.t.data_ptr(), dw.t.data_ptr(), db.t.data_ptr(), slab.t.data_ptr(), good_codes.data_ptr()
    refused = {
        'fwd Cout=24': lib.ocr_conv1_fwd(X, Wt, B, Y, Nb, W, H, 24, 1, st),
        'fwd Cout=12': lib.ocr_conv1_fwd(X, Wt, B, Y, Nb, W, H, 12, 1, st),
        'pool Cout=24': lib.ocr_conv1_pool_fwd(X, Wt, B, Y, Nb, W, H, 24, st),
        'pool odd W': lib.ocr_conv1_pool_fwd(X, Wt, B, Y, Nb, W + 1, H, 64, st),
        'pool odd H': lib.ocr_conv1_pool_fwd(X, Wt, B, Y, Nb, W, H + 1, 64, st),
        'train odd W': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W + 1, H, 64, C, None, 0, None, 0, st),
        'codes Cout=8': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W, H, 8, C, None, 0, None, 0, st),
        'codes Cout=128': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W, H, 128, C, None, 0, None, 0, st),
        'zero % 4': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W, H, 64, C, Z, 6, None, 0, st),
        'zero misaligned': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W, H, 64, C, Z + 4, 8, None, 0, st),
        'zero NULL': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W, H, 64, C, None, 8, None, 0, st),
        'ones % 4': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W, H, 64, C, None, 0, Z, 6, st),
        'ones misaligned': lib.ocr_conv1_pool_fwd_train(X, Wt, B, Y, Nb, W, H, 64, C, None, 0, Z + 8, 8, st),
        'wgrad Cout=128': lib.ocr_conv1_wgrad(X, DZ, DW, DB, Nb, W, H, 128, st),
        'wgrad Cout=8': lib.ocr_conv1_wgrad(X, DZ, DW, DB, Nb, W, H, 8, st),
        'bwd Cout=128': lib.ocr_conv1_pool_bwd(X, Wt, B, DZ, DW, DB, Nb, W, H, 128, st),
        'bwd odd W': lib.ocr_conv1_pool_bwd(X, Wt, B, DZ, DW, DB, Nb, W + 1, H, 64, st),
        'bwd odd H': lib.ocr_conv1_pool_bwd(X, Wt, B, DZ, DW, DB, Nb, W, H + 1, 64, st),
        'bwd codes Cout=8': lib.ocr_conv1_pool_bwd_codes(X, Wt, B, DZ, DW, DB, Nb, W, H, 8, GC, st),
        'bwd codes NULL': lib.ocr_conv1_pool_bwd_codes(X, Wt, B, DZ, DW, DB, Nb, W, H, 64, None, st),
        'slab Cout=128': lib.ocr_conv1_pool_bwd_slab(X, Wt, B, DZ, Nb, W, H, 128, None, SL, st),
        'slab odd H': lib.ocr_conv1_pool_bwd_slab(X, Wt, B, DZ, Nb, W, H + 1, 64, GC, SL, st),
        'slab misaligned': lib.ocr_conv1_pool_bwd_slab(X, Wt, B, DZ, Nb, W, H, 64, None, SL + 4, st),
    }
    assert all(rc == ERR_INVALID for rc in refused.values()), refused
    assert ops.conv1_pool_bwd_slab_rows(Nb, W + 1, H) == 0 and ops.conv1_pool_bwd_slab_rows(Nb, W, H + 1) == 0
    for g in (y, codes, fill, dw, db, slab):
        assert g.intact(whole=True)
    with pytest.raises(nat.NativeError):                                       # and the wrappers raise
        ops.conv1_fwd(x[:, :W, :H].contiguous(), w[:, :24].contiguous(), b[:24].contiguous())


@pytest.mark.parametrize("ppb", [32, 1024])
def test_slab_form_at_other_block_sizes(dev, ppb):
    """OCR_CONV1_PPB is read once per process: the pool test on (3, 30, 12) and on batch C1 in an interpreter of its own per value, under a
    time limit.  The child asserts rows = ceil(npix / ppb) and the slab bound with k = ppb / 32 + 6."""
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-s', '-k',
                          'test_conv1_pool_kernels and (captcha-3x30x12 or captcha-C1)'],
                         env=dict(os.environ, OCR_CONV1_PPB=str(ppb)), capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    assert '2 passed' in out.stdout and 'skipped' not in out.stdout, out.stdout[-1000:]
    for npix in (3 * 15 * 6, 8 * 44 * 16):
        assert 'slab: ppb=%d rows=%d' % (ppb, cr.ceil_div(npix, ppb)) in out.stdout
