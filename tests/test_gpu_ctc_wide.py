"""-m gpu: the wide-alphabet CTC loss (ctc_long.hip: ctc_wide_rows_kernel + ctc_wide_samples_kernel, ops.ctc_loss_wide) against the float64 oracle
on the cases of tests/ctc_wide_cases.py, on small-alphabet cases of tests/ctc_long_cases.py, its refusals, and the engine's choice of it.
Bounds and their derivation: ctc_wide_cases.py (ctc_long_cases.py for its own cases).

Measured on an MI355X (worst over the cases and the four forms; the tests print every figure before they assert):

                                   float32 floor     bound (8 x)     device
    cost, absolute                 8.96e-4           7.17e-3         7.04e-4 (L255; saturated 1.25e-4)
    gradient entry, absolute       1.113e-3          8.90e-3         1.112e-3 (L255; saturated 2.39e-4)
    bf16 gradient of the training form, |dev - ref / 64| / (8.90e-3 / 64 + half a bf16 ulp of ref / 64): 0.26 (L255; 0.17 to 0.19 elsewhere)
    small alphabets (ctc_long_cases.py: handover, stride, repeats, C200_blank_last): cost 1.37e-4, gradient 2.63e-4 (repeats), its floor
    engine, wide path against parent path (C = 4096, N = 2, W = 64, L = 9 and 4): costs equal; logits' gradient differs by at most 9.5e-7 at |dy| <= 0.375
    engine, C = 4096 with a 200-character label at T = 207: costs 1688.3 and 1575.5, at most 3.8e-4 from the float64 oracle
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_wide_cases as wc  # noqa: E402
import lstm_replay as lr  # noqa: E402

lc = wc.lc
pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float('nan')
SCALE = 1.0 / 64


def _device_inputs(k, dev):
    a = torch.from_numpy(k.acts).to(dev)
    fl, ll, il = (torch.from_numpy(v).to(dev) for v in (k.flat, k.ll, k.il))
    return a, fl, ll, il


def _nan_workspace(k, dev):
    from lstm_ctc_ocr_amd import ops
    n = ops.ctc_wide_workspace_bytes(k.C, k.mll, k.T, k.N)
    assert n == wc.workspace_bytes(k.C, k.mll, k.T, k.N)
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)          # 0xFFFFFFFF: a NaN in every float


def _check(k, mod, tag, costs, grads=None, gb=None):
    """Costs, f32 [T][N][C] gradient and bf16 [N][T][C] scaled gradient of case k of module mod (its reference, its bounds) against the oracle;
    prints the measured figures first."""
    ref_c, ref_g = mod.reference(k)
    bad = k.infeasible()
    c = costs.cpu().numpy().astype(np.float64)
    ec = float(np.abs(c - ref_c).max())
    msg = '%s %s: cost error %.3e (bound %.3e)' % (k.name, tag, ec, mod.COST_BOUND)
    eg = ratio = None
    past = np.arange(k.T)[:, None] >= np.minimum(k.il, k.T)[None, :]          # [T][N]: frames past Tn
    if grads is not None:
        g = grads.cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all(), '%s %s: f32 gradient elements left unwritten' % (k.name, tag)
        eg = float(np.abs(g - ref_g).max())
        msg += '; gradient error %.3e (bound %.3e)' % (eg, mod.GRAD_BOUND)
        assert not g[:, bad].any() and not g[past].any(), (k.name, tag)
    if gb is not None:
        got = gb.float().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), '%s %s: bf16 gradient elements left unwritten' % (k.name, tag)
        want = SCALE * np.transpose(ref_g, (1, 0, 2))
        ratio = float((np.abs(got - want) / (SCALE * mod.GRAD_BOUND + lr.half_ulp_bf16(want))).max())
        msg += '; bf16 gradient worst |dev - ref| / bound %.3f' % ratio
        assert not got[bad].any() and not got[past.T].any(), (k.name, tag)
    print(msg)
    assert np.isfinite(c).all() and np.all(c[bad] == 0), msg
    assert ec <= mod.COST_BOUND, msg
    assert eg is None or eg <= mod.GRAD_BOUND, msg
    assert ratio is None or ratio <= 1.0, msg


def _four_forms(k, mod, dev):
    from lstm_ctc_ocr_amd import ops
    assert ops.ctc_wide_supported(k.C, k.T, k.mll)
    a, fl, ll, il = _device_inputs(k, dev)
    nan_costs = lambda: torch.full((k.N,), NAN, device=dev)
    nan_bf = lambda: torch.full((k.N, k.T, k.C), NAN, dtype=BF, device=dev)

    costs, none = ops.ctc_loss_wide(a, fl, ll, il, k.mll, k.blank, want_grad=False, workspace=_nan_workspace(k, dev), costs=nan_costs())
    torch.cuda.synchronize()
    assert none is None
    _check(k, mod, 'score only', costs)

    costs, grads = ops.ctc_loss_wide(a, fl, ll, il, k.mll, k.blank, workspace=_nan_workspace(k, dev), costs=nan_costs(), grads=torch.full_like(a, NAN))
    torch.cuda.synchronize()
    _check(k, mod, 'f32 gradient', costs, grads)

    gb = nan_bf()
    costs, _ = ops.ctc_loss_wide(a, fl, ll, il, k.mll, k.blank, want_grad=False, grad_ntc_bf16=gb, scale=SCALE, workspace=_nan_workspace(k, dev),
                                 costs=nan_costs())
    torch.cuda.synchronize()
    _check(k, mod, 'bf16 training form', costs, gb=gb)

    gb = nan_bf()
    costs, grads = ops.ctc_loss_wide(a, fl, ll, il, k.mll, k.blank, grad_ntc_bf16=gb, scale=SCALE, workspace=_nan_workspace(k, dev), costs=nan_costs(),
                                     grads=torch.full_like(a, NAN))
    torch.cuda.synchronize()
    _check(k, mod, 'both gradients', costs, grads, gb)


@pytest.mark.parametrize('name', [k.name for k in wc.cases()])
def test_wide_kernels_against_oracle(dev, name):
    _four_forms(wc.case(name), wc, dev)


@pytest.mark.parametrize('name', ['handover', 'stride', 'repeats', 'C200_blank_last'])
def test_wide_kernels_on_small_alphabets(dev, name):
    """The wide entry is general in the class count: cases of the long kernel (C = 37, 11, 129, 200), with that module's bounds."""
    _four_forms(lc.case(name), lc, dev)


def test_refused_inputs(dev):
    """OCR_ERR_INVALID (2) and no launch: costs and gradients keep the value they were given."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    k = wc.case('past_long')
    a, fl, ll, il = _device_inputs(k, dev)
    need = ops.ctc_wide_workspace_bytes(k.C, k.mll, k.T, k.N)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    costs = torch.full((k.N,), 7.0, device=dev)
    grads = torch.full_like(a, 7.0)
    gb = torch.full((k.N, k.T, k.C), 7.0, dtype=BF, device=dev)
    p = nat.ptr
    good = dict(acts=p(a), labels=p(fl), ll=p(ll), il=p(il), costs=p(costs), ws=p(ws), C=k.C, mll=k.mll, blank=k.blank, ws_bytes=need)

    def status(**kw):
        v = dict(good, **kw)
        return nat.lib().ocr_ctc_loss_wide(v['acts'], p(grads), p(gb), SCALE, v['labels'], v['ll'], v['il'], v['C'], k.N, k.T, v['mll'], v['blank'],
                                           v['costs'], v['ws'], v['ws_bytes'], nat.stream())
    assert status(C=16385) == 2
    assert status(mll=0) == 2
    assert status(mll=256) == 2
    assert status(ws_bytes=need - 1) == 2
    for operand in ('acts', 'labels', 'll', 'il', 'costs', 'ws'):
        assert status(**{operand: None}) == 2, operand
    assert status(blank=-1) == 2
    assert status(blank=k.C) == 2
    torch.cuda.synchronize()
    assert bool((costs == 7.0).all()) and bool((grads == 7.0).all()) and bool((gb == 7.0).all())
    assert not ops.ctc_wide_supported(16385, k.T, k.mll) and not ops.ctc_wide_supported(k.C, k.T, 256) and not ops.ctc_wide_supported(k.C, k.T, 0)
    sz = ctypes.c_size_t(0)
    assert nat.lib().ocr_ctc_wide_workspace_size(k.C, 256, k.T, k.N, ctypes.byref(sz)) == 2
    with pytest.raises(nat.NativeError):
        ops.ctc_loss_wide(a, fl, ll, il, 256)
    assert status() == 0                      # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    _check(k, wc, 'after the refusals', costs, grads, gb)


def _no_adjacent_repeats(rng, L, lo, hi):
    out = []
    while len(out) < L:
        v = int(rng.randint(lo, hi))
        if not out or v != out[-1]:
            out.append(v)
    return out


ENGINE_CLASSES = 4096


def _engine_batch(W, lens, seed):
    rng = np.random.RandomState(seed)
    N = len(lens)
    x = rng.rand(N, W, 32).astype(np.float32)
    sl = np.full(N, W // 4 - 1, np.int32)
    labels = np.array([v for L in lens for v in _no_adjacent_repeats(rng, L, 1, ENGINE_CLASSES - 1)], np.int32)
    return x, sl, labels, np.array(lens, np.int32)


def test_engine_wide_path_against_parent_path(dev):
    from lstm_ctc_ocr_amd import dist as ocr_dist
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    N, W = 2, 64
    assert Engine(get_network('LSTM_train'), device='cuda:0', seed=3).ctc_path(N, W) == 'fast'          # the default configuration
    x, sl, labels, ll = _engine_batch(W, [9, 4], 43)
    old = cfg.NCLASSES
    cfg.NCLASSES = ENGINE_CLASSES
    try:
        def run(**kw):
            eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3, max_label_len=40, **kw)
            sp = eng.plan(N, W)
            eng._bind(sp, x, sl, labels, ll)
            eng._run(sp, 'fb')
            torch.cuda.synchronize()
            return (eng.ctc_path(N, W), sp.costs.cpu().numpy().astype(np.float64), eng.ops[-1].dy(sp).float().cpu().numpy().astype(np.float64), sp,
                    eng)
        path_w, cost_w, dy_w, sp, eng = run()
        path_g, cost_g, dy_g, _, _ = run(ctc_wide=False)
        assert (path_w, path_g) == ('wide', 'general')
        assert (sp.T, sp.C) == (W // 4 - 1, ENGINE_CLASSES)
        scale = ocr_dist.loss_scale(N, 1)
        assert scale == 1.0 / N
        print('engine: costs wide %s general %s; worst cost difference %.3e; worst dy difference %.3e (largest |dy| %.3e)'
              % (cost_w, cost_g, np.abs(cost_w - cost_g).max(), np.abs(dy_w - dy_g).max(), np.abs(dy_g).max()))
        assert np.all(cost_w > 0) and np.isfinite(cost_w).all()
        assert np.abs(cost_w - cost_g).max() <= 2 * wc.COST_BOUND
        assert dy_w.size == N * sp.T * sp.C and dy_w.shape == dy_g.shape and np.abs(dy_g).max() > 0      # [N][T][C], held as [N * T, C]
        tol = 2 * scale * wc.GRAD_BOUND + 2 * lr.half_ulp_bf16(np.maximum(np.abs(dy_w), np.abs(dy_g)))
        assert np.all(np.abs(dy_w - dy_g) <= tol)
        eng.setup_optimizer('Adam', 1e-4)
        loss = eng.train_step(x, labels, ll, sl)
        assert np.isfinite(loss)
    finally:
        cfg.NCLASSES = old
    assert Engine(get_network('LSTM_train'), device='cuda:0', seed=3).ctc_path(N, W) == 'fast'


def test_engine_trains_a_wide_alphabet_with_a_200_character_label(dev):
    """C = 4096 with max_label_len = 200: no CTC form covered the shape before (the general kernel stops at 127 characters, the long kernel near
    2040 classes)."""
    from lstm_ctc_ocr_amd import ops
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    N, W = 2, 832
    T = W // 4 - 1
    assert T >= 201
    x, sl, labels, ll = _engine_batch(W, [200, 37], 47)
    old = cfg.NCLASSES
    cfg.NCLASSES = ENGINE_CLASSES
    try:
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3, max_label_len=200)
        assert eng.ctc_path(N, W) == 'wide'
        assert not ops.ctc_long_supported(ENGINE_CLASSES, T, 200) and not ops.ctc_train_supported(ENGINE_CLASSES, T, 200)
        logits = eng.forward(x, sl).float().cpu().numpy()
        assert logits.shape == (T, N, ENGINE_CLASSES)
        sp = eng.plan(N, W)
        eng._bind(sp, x, sl, labels, ll)
        eng._run(sp, 'fb')
        torch.cuda.synchronize()
        costs = sp.costs.cpu().numpy().astype(np.float64)
        ref_c, _ = wc.octc.ctc_loss_numpy(logits, labels, ll, sl, 0)
        print('engine, C = %d, L = 200, T = %d: costs %s, oracle %s, worst difference %.3e (bound %.3e)'
              % (ENGINE_CLASSES, T, costs, ref_c, np.abs(costs - ref_c).max(), wc.COST_BOUND))
        assert np.all(ref_c > 0) and np.abs(costs - ref_c).max() <= wc.COST_BOUND
        eng.setup_optimizer('Adam', 1e-4)
        loss = eng.train_step(x, labels, ll, sl)
        assert np.isfinite(loss)
    finally:
        cfg.NCLASSES = old
