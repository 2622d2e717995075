"""CPU: the checker of tests/conv1_reference.py pinned without a GPU.  A numpy fp32 model of the conv1 kernels (the same fp32 operations in
the same order: nine fmas from zero, the bias add, ReLU, RNE to bf16; first maximum of the rounded values, W outer; per-thread fma chains,
the shuffle tree, the four-wave sum, atomics or slab rows) passes every check; eight deliberately wrong models each fail one.  Also the
claims the GPU test rests on: at most 5 % ambiguous windows in every case it runs, at least 5 % positive-maximum ties on rendered captchas.

An fma is modelled as fl32(fl64(acc + x w)): the product is exact in fp64 and the double rounding costs at most 2^-29 of a step's u."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1_reference as cr  # noqa: E402

F32, F64 = np.float32, np.float64
MUTANTS = ('last_max', 'unrounded_argmax', 'h_outer', 'relu_ge', 'no_pad_high_w', 'truncate', 'drop_partial_block', 'no_relu_mask')
SCAN_H_OUTER = (0, 2, 1, 3)        # e = 2 (w offset) + (h offset) visited with the h offset outermost


def fma(acc, x, w):
    return (acc.astype(F64) + x.astype(F64) * w.astype(F64)).astype(F32)


class Model:
    """fp32 model of the kernels; `wrong` names one mutation (MUTANTS) or None."""

    def __init__(self, x, w, b, wrong=None):
        self.x, self.w, self.b, self.wrong = x, w.reshape(9, -1), b, wrong
        self.Nb, self.W, self.H = x.shape
        self.Co = self.w.shape[1]
        self.xp = np.zeros((self.Nb, self.W + 2, self.H + 2), F32)
        self.xp[:, 1:-1, 1:-1] = x
        if wrong == 'no_pad_high_w':                      # reads the last row again where the zero border belongs
            self.xp[:, -1, :] = self.xp[:, -2, :]

    def conv1_fwd(self, relu=True, rounded=True):
        o = np.zeros((self.Nb, self.W, self.H, self.Co), F32)
        for t in range(9):
            i, j = divmod(t, 3)
            o = fma(o, self.xp[:, i:i + self.W, j:j + self.H, None], self.w[t])
        o = o + self.b
        if relu:
            o = np.maximum(o, F32(0))
        return cr.f32_to_bf16(o, truncate=self.wrong == 'truncate') if rounded else o

    def conv1_pool_fwd(self):
        """-> pooled bf16 (as fp32) [Nb, W/2, H/2, Co], code words uint32 [npix, Co / 8]"""
        o = cr.windows(self.conv1_fwd(rounded=False))
        r = cr.windows(self.conv1_fwd())
        pooled = r.max(3)
        key = o if self.wrong == 'unrounded_argmax' else r
        if self.wrong == 'last_max':
            best = 3 - key[:, :, :, ::-1].argmax(3)
        elif self.wrong == 'h_outer':
            best = np.asarray(SCAN_H_OUTER)[key[:, :, :, SCAN_H_OUTER].argmax(3)]
        else:
            best = key.argmax(3)
        bit = (pooled >= 0) if self.wrong == 'relu_ge' else (pooled > 0)
        code = (best.astype(np.uint32) | (bit.astype(np.uint32) << 2)).reshape(-1, self.Co // 8, 8)
        words = (code << (4 * np.arange(8, dtype=np.uint32))).sum(2, dtype=np.uint32)
        return pooled, words

    def _chains(self, patch, g, ppb, atomics):
        """patch fp32 [npix, 9, Co] (the tap values per pixel and channel), g fp32 [npix, Co] in pixel order -> the device's sums: a block
        owns ppb consecutive pixels, lane pl runs an fma chain over every 32nd of them; then _tree."""
        npix = g.shape[0]
        nblk = cr.ceil_div(npix, ppb)
        if self.wrong == 'drop_partial_block' and npix % ppb:
            patch, g = patch[:npix - npix % ppb], g[:npix - npix % ppb]
        P = np.zeros((nblk * ppb, 9, self.Co), F32); P[:patch.shape[0]] = patch
        G = np.zeros((nblk * ppb, self.Co), F32); G[:g.shape[0]] = g
        P = P.reshape(nblk, ppb // 32, 32, 9, self.Co); G = G.reshape(nblk, ppb // 32, 32, self.Co)
        acc = np.zeros((nblk, 32, 10, self.Co), F32)
        for i in range(ppb // 32):
            acc[:, :, :9] = fma(acc[:, :, :9], P[:, i], G[:, i][:, :, None, :])
            acc[:, :, 9] = acc[:, :, 9] + G[:, i]
        return self._tree(acc, atomics)

    def _tree(self, acc, atomics):
        """acc fp32 [blocks, 32 lanes, 10, Co]: the eight lanes of a wave by xor-shuffles (pl = 8 wave + lane), the four waves in order, then
        the blocks in order (atomics) or one row per block (slab)."""
        nblk = acc.shape[0]
        acc = acc.reshape(nblk, 4, 8, 10, self.Co)
        for bit in (1, 2, 4):
            acc = acc + acc[:, :, np.arange(8) ^ bit]
        rows = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]
        if not atomics:
            return rows.reshape(nblk, 10 * self.Co)
        tot = np.zeros((10, self.Co), F32)
        for r in rows:
            tot = tot + r
        return tot[:9], tot[9]

    def conv1_wgrad(self, dz):
        P = np.stack([self.xp[:, i:i + self.W, j:j + self.H].reshape(-1) for i in range(3) for j in range(3)], 1)
        P = np.broadcast_to(P[:, :, None], P.shape + (self.Co,))
        return self._chains(P, np.asarray(dz, F32).reshape(-1, self.Co), cr.WGRAD_PPB, True)

    def conv1_pool_bwd(self, dp, words, ppb=cr.ATOMICS_PPB, atomics=True):
        Wo, Ho = self.W // 2, self.H // 2
        code = cr.unpack_codes(words, (self.Nb * Wo * Ho, self.Co))
        g = np.asarray(dp, F32).reshape(-1, self.Co)
        if self.wrong != 'no_relu_mask':
            g = np.where((code & 4) != 0, g, F32(0))
        best = code & 3
        P = np.zeros((g.shape[0], 9, self.Co), F32)
        for el in range(4):
            a, b = el >> 1, el & 1
            Pe = np.stack([self.xp[:, a + i:a + i + 2 * Wo:2, b + j:b + j + 2 * Ho:2].reshape(-1) for i in range(3) for j in range(3)], 1)
            P = np.where((best == el)[:, None, :], Pe[:, :, None], P)
        return self._chains(P, g, ppb, atomics)


def run_checks(ref, m, dp, dz=None, ppb=256):
    """Every check of the checker on one model -> {name: ratio}."""
    out = {}
    for relu in (True, False):
        out['fwd relu=%d' % relu] = ref.check_full(m.conv1_fwd(relu), relu)
    pooled, words = m.conv1_pool_fwd()
    out.update(('pool ' + k, v) for k, v in ref.check_pooled(pooled, words).items())
    bw = ref.backward(dp, words)
    dw, db = m.conv1_pool_bwd(dp, words)
    out.update(('bwd atomics ' + k, v) for k, v in ref.check_backward(bw, dw, db, 256, True).items())
    dw, db = cr.slab_sums(m.conv1_pool_bwd(dp, words, ppb, atomics=False))
    out.update(('bwd slab ' + k, v) for k, v in ref.check_backward(bw, dw, db, ppb, False).items())
    if dz is not None:
        dw, db = m.conv1_wgrad(dz)
        out.update(('wgrad ' + k, v) for k, v in ref.check_wgrad(dz, dw, db).items())
    return out


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        x, w, b = cr.case_operands(name)
        ref = cr.Reference(x, w, b)
        dp = cr.make_dp((x.shape[0], x.shape[1] // 2, x.shape[2] // 2, 64), 4)
        dz = cr.make_dp(x.shape + (64,), 5)
        _CACHE[name] = (x, w, b, ref, dp, dz)
    return _CACHE[name]


MODEL_CASES = [n for n in cr.CASES if not n.endswith('V0')]        # the small shapes in every regime, and batch C1


@pytest.mark.parametrize("name", MODEL_CASES)
def test_the_model_of_the_kernels_passes(name):
    x, w, b, ref, dp, dz = _case(name)
    worst = run_checks(ref, Model(x, w, b), dp, dz)
    print(name, ' '.join('%s %.3g' % kv for kv in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("ppb", [32, 1024])
def test_the_model_passes_at_other_block_sizes(ppb):
    x, w, b, ref, dp, _ = _case('captcha-3x30x12')
    m = Model(x, w, b)
    _, words = m.conv1_pool_fwd()
    slab = m.conv1_pool_bwd(dp, words, ppb, atomics=False)
    assert slab.shape == (cr.ceil_div(3 * 15 * 6, ppb), 640)
    dw, db = cr.slab_sums(slab)
    assert max(ref.check_backward(ref.backward(dp, words), dw, db, ppb, False).values()) <= 1.0


# where each wrong model has to show: (case, the checks of which at least one must exceed 1)
EXPECT = {
    'last_max': ('pool codes',),
    'unrounded_argmax': ('pool codes',),
    'h_outer': ('pool codes',),
    'relu_ge': ('pool codes',),
    'no_pad_high_w': ('fwd relu=1', 'fwd relu=0', 'pool pooled'),
    'truncate': ('fwd relu=1', 'fwd relu=0', 'pool pooled', 'pool exact'),
    'drop_partial_block': ('bwd atomics dw', 'bwd atomics db', 'bwd slab dw', 'bwd slab db'),
    'no_relu_mask': ('bwd atomics db', 'bwd slab db'),
}


@pytest.mark.parametrize("name", ['captcha-C1', 'captcha-3x30x12'])
@pytest.mark.parametrize("wrong", MUTANTS)
def test_a_wrong_model_fails(wrong, name):
    """On rendered captchas: whole batch C1 and the crop.  Two of the wrong models cannot show on C1 and run on the all-ones image instead:
    C1 has 2816 = 11 * 256 pooled pixels, no partial block; and its images end in zero columns (the batch is padded to a common width), so
    what stands beyond the high-W edge is multiplied by nothing there."""
    if wrong in ('drop_partial_block', 'no_pad_high_w') and name == 'captcha-C1':
        name = 'ones-3x30x12'
    x, w, b, ref, dp, dz = _case(name)
    worst = run_checks(ref, Model(x, w, b, wrong), dp, dz if wrong in ('drop_partial_block', 'no_pad_high_w') else None)
    failed = [k for k, v in worst.items() if not v <= 1.0]
    assert failed and any(k in EXPECT[wrong] for k in failed), (wrong, worst)
    if wrong in ('drop_partial_block', 'no_pad_high_w'):
        assert not worst['wgrad dw'] <= 1.0


def test_the_wrong_tie_rules_pass_on_the_uniform_regime_windows_they_were_tested_on():
    """Why the captchas are needed: on the uniform random regime the tie mutants differ from the kernel in almost no window."""
    x, w, b, ref, dp, _ = _case('random-3x30x12')
    _, good = Model(x, w, b).conv1_pool_fwd()
    for wrong in ('last_max', 'h_outer'):
        _, words = Model(x, w, b, wrong).conv1_pool_fwd()
        p = ref.pool()
        moved = (cr.unpack_codes(words, p['code'].shape) != cr.unpack_codes(good, p['code'].shape)) & (p['pooled'] > 0)
        assert moved.mean() < 0.005
    x, w, b, ref, dp, _ = _case('captcha-C1')
    _, good = Model(x, w, b).conv1_pool_fwd()
    _, words = Model(x, w, b, 'last_max').conv1_pool_fwd()
    p = ref.pool()
    moved = (cr.unpack_codes(words, p['code'].shape) != cr.unpack_codes(good, p['code'].shape)) & (p['pooled'] > 0)
    assert moved.mean() > 0.05


@pytest.mark.parametrize("name", list(cr.CASES))
def test_ambiguity_cap_and_tie_floor(name):
    """Every case of the GPU test: at most 5 % ambiguous windows; whole rendered batches: at least 5 % of the unambiguous windows hold a
    positive maximum shared by two or more elements.  Measured: C1 2.2 % / 11.9 %, V0[:28] 1.4 % / 20.7 %, perturbed taps 2.8 % / 11.6 % and
    1.6 % / 20.6 %, uniform random (3, 30, 12) 0.8 % / 0.3 %, constant images 0 % ambiguous."""
    x, w, b = cr.case_operands(name)
    amb, tie = (_CACHE[name][3] if name in _CACHE else cr.Reference(x, w, b)).shares()
    print('%s: ambiguous %.4f, positive ties %.4f' % (name, amb, tie))
    assert amb <= cr.AMBIGUOUS_CAP
    if name in cr.BATCH_CASES:
        assert tie >= cr.TIE_FLOOR


def test_bf16_helpers():
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0, 0.0, 2.0 ** -130, 255.5], F64)       # 1 + 2^-8 (midpoint -> even), 1 + 3 * 2^-8 (-> up)
    assert np.array_equal(cr.bf16_rne(v), [1.0, 1.0, 1.015625, -3.0, 0.0, 2.0 ** -130, 256.0])
    assert np.array_equal(cr.bf16_ulp(np.array([1.0, 1.99, 2.0, 0.0, -0.75])), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -8])
    a = np.random.RandomState(0).uniform(-4, 4, 10000).astype(F32)
    assert np.array_equal(cr.f32_to_bf16(a).astype(F64), cr.bf16_rne(a.astype(F64)))
    words = np.array([[0x76543210] + [0] * 7], np.uint32)
    assert cr.unpack_codes(words, (1, 64))[0, :8].tolist() == list(range(8))
