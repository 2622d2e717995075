"""-m gpu: the tile generation of the fused conv1 + pool kernels (csrc/conv1.hip: a block stages the input rows of its run of pooled
pixels in LDS once; codes in packed 16-bit integer arithmetic; the backward routes by select-and-multiply) at the shapes of
tests/conv1_tile_cases.py.

(a) Bit for bit against the first generation of these kernels (per-lane patch loads, float-compare codes; removed from the library, readable
    at commit 29b4ab6), on 1/64-grid operands (frequent ties).  Its slab words were recorded from it and are committed as
    tests/golden/conv1_pool_first_generation.npz; its pooled map and routing codes equalled tc.exact_forward when they were recorded — on
    these operands every forward sum is exact in fp32, so the fp64 model IS the device result.  OCR_CONV1_PPB is read once per process, so
    the other block sizes run in a child interpreter.
(b) Against the fp64 reference of tests/conv1_reference.py, with its bounds (c = 10 / (1 - 10 u) forward; k = ppb / 32 + 6 slab backward),
    guarded outputs and the two fills.
tests/test_conv1_tile_shapes.py shows without a GPU that the operands are decisive and exact, and that the fixture is a valid gradient."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1_reference as cr  # noqa: E402
import conv1_tile_cases as tc  # noqa: E402

from lstm_ctc_ocr_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
POISON = {BF: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC00001), I32: (torch.int32, -1)}
_ID = lambda s: '%dx%dx%d' % s


def _child(path, shapes, **env):
    """The launches of tc.run_train_launches on the product library in an interpreter of its own -> the arrays it saved, by shape."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'conv1_tile_cases.py'), str(path)] + ['%d,%d,%d' % s for s in shapes],
                         env=dict({k: v for k, v in os.environ.items() if k != 'OCR_NATIVE_LIB'}, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and 'TILE_CASES_OK' in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
    d = np.load(str(path))
    return {s: {k: d['%dx%dx%d/%s' % (s + (k,))] for k in ('pooled', 'codes', 'slab_codes', 'slab_recompute')} for s in shapes}


def _assert_same(first, ppb, tile, shapes):
    """tile[shape] = what tc.run_train_launches returned; first = the fixture."""
    for s in shapes:
        pooled, codes = tc.exact_forward(s)
        got = tile[s]
        assert np.array_equal(got['pooled'].view(np.uint16).reshape(pooled.shape), pooled), (s, 'pooled')
        assert np.array_equal(cr.unpack_codes(got['codes'], codes.shape), codes), (s, 'codes')
        for k in ('slab_codes', 'slab_recompute'):
            a, b = first[tc.fixture_key(ppb, s, k)], got[k]
            assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (s, k, int((a != b).sum()))
        assert np.array_equal(got['slab_codes'], got['slab_recompute'])


def test_bit_equal_to_first_generation(dev):
    assert _ppb() == 256            # the fixture's entries for all of tc.SHAPES are those of the default block size
    tile = {s: tc.run_train_launches(dev, s) for s in tc.SHAPES}
    _assert_same(np.load(tc.FIXTURE), 256, tile, tc.SHAPES)


@pytest.mark.parametrize("ppb", [32, 1024])
def test_bit_equal_at_other_block_sizes(dev, tmp_path, ppb):
    shapes = (tc.PPB_SHAPE,)
    tile = _child(tmp_path / 'tile.npz', shapes, OCR_CONV1_PPB=str(ppb))
    npix = tc.PPB_SHAPE[0] * (tc.PPB_SHAPE[1] // 2) * (tc.PPB_SHAPE[2] // 2)
    assert tile[tc.PPB_SHAPE]['slab_codes'].shape == (cr.ceil_div(npix, ppb), 640)
    _assert_same(np.load(tc.FIXTURE), ppb, tile, shapes)


# ------------------------------------------------------------------------------------------------ (b) the fp64 reference
class Guarded:
    """rows x cols of poison with GUARD more rows behind them; .t is the view a kernel gets, intact() whether the rows behind still hold it."""

    def __init__(self, dev, rows, cols, dtype, shape=None):
        self.as_int, self.pattern = POISON[dtype]
        self.buf = torch.empty((rows + GUARD, cols), dtype=dtype, device=dev)
        self.buf.view(self.as_int).fill_(self.pattern)
        self.rows = rows
        self.t = self.buf[:rows] if shape is None else self.buf[:rows].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[self.rows:].view(self.as_int) == self.pattern).all())


def _np(t):
    return (t.float() if t.dtype == BF else t).cpu().numpy()


def _assert(shape, what, worst):
    print('%-12s %-24s %s' % (_ID(shape), what, '  '.join('%s %.3g' % kv for kv in sorted(worst.items()))), flush=True)
    assert all(v <= 1.0 for v in worst.values()), (shape, what, worst)


def _ppb():
    try:
        v = int(os.environ.get('OCR_CONV1_PPB', '256'))
    except ValueError:
        v = 0
    return v if 32 <= v <= 1024 and v % 32 == 0 else 256


@pytest.mark.parametrize("shape", tc.SHAPES, ids=_ID)
def test_against_fp64_reference(dev, shape):
    Nb, W, H = shape
    x, w, b = tc.reference_operands(Nb, W, H)
    ref = cr.Reference(x, w, b)
    assert ref.shares()[0] <= cr.AMBIGUOUS_CAP
    Wo, Ho, Co = W // 2, H // 2, 64
    npix = Nb * Wo * Ho
    xd, wd, bd = (torch.from_numpy(a).to(dev) for a in (x, w, b))
    # inference forward
    p = Guarded(dev, npix, Co, BF, (Nb, Wo, Ho, Co))
    ops.conv1_pool_fwd(xd, wd, bd, out=p.t)
    assert p.intact()
    _assert(shape, 'pool_fwd', ref.check_pooled(_np(p.t)))
    # training forward: the codes, and the two fills touch exactly their words
    p2 = Guarded(dev, npix, Co, BF, (Nb, Wo, Ho, Co))
    codes = Guarded(dev, npix, 8, I32)
    junk = torch.full((4096 + 8,), 7.0, device=dev)
    ones = torch.zeros(4096 + 64, dtype=I32, device=dev)
    ops.conv1_pool_fwd(xd, wd, bd, out=p2.t, zero=junk[4:4100], codes=codes.t, ones=ones[8:4104])
    assert p2.intact() and codes.intact() and torch.equal(p2.t, p.t)
    assert float(junk[4:4100].abs().max()) == 0.0 and bool((junk[:4] == 7.0).all()) and bool((junk[4100:] == 7.0).all())
    assert bool((ones[8:4104] == -1).all()) and bool((ones[:8] == 0).all()) and bool((ones[4104:] == 0).all())
    cn = codes.t.cpu().numpy()
    _assert(shape, 'pool_fwd codes', ref.check_pooled(_np(p2.t), cn))
    # slab backward, from the saved codes and from recomputed windows
    dp = cr.make_dp((Nb, Wo, Ho, Co), 4)
    dpd = torch.from_numpy(dp).to(dev).to(BF)
    ppb = _ppb()
    rows = ops.conv1_pool_bwd_slab_rows(Nb, W, H)
    assert rows == cr.ceil_div(npix, ppb)
    bw = ref.backward(dp, cn)
    slabs = []
    for cd, tag in ((codes.t, 'codes'), (None, 'recompute')):
        slab = Guarded(dev, rows, 640, F32)                                     # NaN in every word before the call
        ops.conv1_pool_bwd_slab(xd, wd, bd, dpd, slab.t, codes=cd)
        assert slab.intact() and not bool(torch.isnan(slab.t).any())
        dws, dbs = cr.slab_sums(_np(slab.t))
        _assert(shape, 'pool_bwd slab ' + tag, ref.check_backward(bw, dws, dbs, ppb, False))
        slabs.append(slab.t)
    assert torch.equal(slabs[0], slabs[1])
