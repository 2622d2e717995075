"""-m gpu: the long-label CTC kernel (ctc_long.hip: ctc_long_kernel, ops.ctc_loss_long) against the float64 oracle on the cases of
tests/ctc_long_cases.py, its refusals, and the engine's choice of it.  Bounds and their derivation: ctc_long_cases.py.

Measured on an MI355X (worst over the 15 cases and the four forms; the test prints every figure before it asserts):

                                   float32 floor     bound (8 x)     device
    cost, absolute                 9.97e-4           7.98e-3         7.53e-4 (line200; L255 7.41e-4)
    gradient entry, absolute       1.121e-3          8.97e-3         1.19e-3 (L255; line200 1.16e-3)
    bf16 gradient of the training form, |dev - ref / 64| / (8.97e-3 / 64 + half a bf16 ulp of ref / 64): 0.27 (L255)
    general kernel on the cases it accepts (L <= 127): the same figures as the long kernel to three digits (worst 4.69e-4, L127)
    engine, long path against parent path (N = 4, W = 256, L = 40): costs equal; logits' gradient differs by at most 3.8e-6 at |dy| <= 0.19
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_long_cases as lc  # noqa: E402
import lstm_replay as lr  # noqa: E402

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
    n = ops.ctc_long_workspace_bytes(k.C, k.mll, k.T, k.N)
    return torch.full((max(n, 4),), 0xFF, dtype=torch.uint8, device=dev), n          # 0xFFFFFFFF: a NaN in every float


def _check(k, tag, costs, grads=None, gb=None):
    """Costs, f32 [T][N][C] gradient and bf16 [N][T][C] scaled gradient of case k against the oracle; prints the measured figures first."""
    ref_c, ref_g = lc.reference(k)
    bad = k.infeasible()
    c = costs.cpu().numpy().astype(np.float64)
    ec = float(np.abs(c - ref_c).max())
    msg = '%s %s: cost error %.3e (bound %.3e)' % (k.name, tag, ec, lc.COST_BOUND)
    eg = ratio = None
    if grads is not None:
        g = grads.cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all(), '%s %s: f32 gradient elements left unwritten' % (k.name, tag)
        eg = float(np.abs(g - ref_g).max())
        msg += '; gradient error %.3e (bound %.3e)' % (eg, lc.GRAD_BOUND)
        assert not g[:, bad].any(), (k.name, tag)
    if gb is not None:
        got = gb.float().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), '%s %s: bf16 gradient elements left unwritten' % (k.name, tag)
        want = SCALE * np.transpose(ref_g, (1, 0, 2))
        ratio = float((np.abs(got - want) / (SCALE * lc.GRAD_BOUND + lr.half_ulp_bf16(want))).max())
        msg += '; bf16 gradient worst |dev - ref| / bound %.3f' % ratio
        assert not got[bad].any(), (k.name, tag)
    print(msg)
    assert np.isfinite(c).all() and np.all(c[bad] == 0), msg
    assert ec <= lc.COST_BOUND, msg
    assert eg is None or eg <= lc.GRAD_BOUND, msg
    assert ratio is None or ratio <= 1.0, msg


@pytest.mark.parametrize('name', [k.name for k in lc.cases()])
def test_long_kernel_against_oracle(dev, name):
    from lstm_ctc_ocr_amd import ops
    k = lc.case(name)
    assert ops.ctc_long_supported(k.C, k.T, k.mll)
    assert ops.ctc_long_placement(k.C, k.T, k.mll) == lc.placement(k.C, k.T, k.mll)
    a, fl, ll, il = _device_inputs(k, dev)
    nan_costs = lambda: torch.full((k.N,), NAN, device=dev)

    ws, nbytes = _nan_workspace(k, dev)
    assert (nbytes == 0) == (lc.placement(k.C, k.T, k.mll) == 'lds')
    costs, none = ops.ctc_loss_long(a, fl, ll, il, k.mll, k.blank, want_grad=False, workspace=ws, costs=nan_costs())
    torch.cuda.synchronize()
    assert none is None
    _check(k, 'score only', costs)

    ws, _ = _nan_workspace(k, dev)
    costs, grads = ops.ctc_loss_long(a, fl, ll, il, k.mll, k.blank, workspace=ws, costs=nan_costs(), grads=torch.full_like(a, NAN))
    torch.cuda.synchronize()
    _check(k, 'f32 gradient', costs, grads)

    ws, _ = _nan_workspace(k, dev)
    gb = torch.full((k.N, k.T, k.C), NAN, dtype=BF, device=dev)
    costs, _ = ops.ctc_loss_long(a, fl, ll, il, k.mll, k.blank, want_grad=False, grad_ntc_bf16=gb, scale=SCALE, workspace=ws, costs=nan_costs())
    torch.cuda.synchronize()
    _check(k, 'bf16 training form', costs, gb=gb)

    ws, _ = _nan_workspace(k, dev)
    gb = torch.full((k.N, k.T, k.C), NAN, dtype=BF, device=dev)
    costs, grads = ops.ctc_loss_long(a, fl, ll, il, k.mll, k.blank, grad_ntc_bf16=gb, scale=SCALE, workspace=ws, costs=nan_costs(),
                                     grads=torch.full_like(a, NAN))
    torch.cuda.synchronize()
    _check(k, 'both gradients', costs, grads, gb)

    if k.mll <= 127:            # the general kernel accepts the case: the same bounds hold for it
        costs, grads = ops.ctc_loss(a, fl, ll, il, k.mll, k.blank, costs=nan_costs(), grads=torch.full_like(a, NAN))
        torch.cuda.synchronize()
        _check(k, 'general kernel', costs, grads)


def test_refused_inputs(dev):
    """OCR_ERR_INVALID (2) and no launch: the costs keep the value they were given."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    k = lc.case('lds_past')
    a, fl, ll, il = _device_inputs(k, dev)
    need = ops.ctc_long_workspace_bytes(k.C, k.mll, k.T, k.N)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    costs = torch.full((k.N,), 7.0, device=dev)
    grads = torch.full_like(a, 7.0)
    p = nat.ptr

    def status(mll=k.mll, blank=k.blank, costs_ptr=p(costs), ws_bytes=need):
        return nat.lib().ocr_ctc_loss_long(p(a), p(grads), None, 1.0, p(fl), p(ll), p(il), k.C, k.N, k.T, mll, blank, costs_ptr, p(ws),
                                           ws_bytes, nat.stream())
    assert status(mll=256) == 2
    assert status(ws_bytes=need - 1) == 2
    assert status(blank=k.C) == 2
    assert status(blank=-1) == 2
    assert status(costs_ptr=None) == 2
    torch.cuda.synchronize()
    assert bool((costs == 7.0).all()) and bool((grads == 7.0).all())
    assert not ops.ctc_long_supported(k.C, k.T, 256) and not ops.ctc_long_supported(k.C, k.T, 0)
    sz = ctypes.c_size_t(0)
    assert nat.lib().ocr_ctc_long_workspace_size(k.C, 256, k.T, k.N, ctypes.byref(sz)) == 2
    with pytest.raises(nat.NativeError):
        ops.ctc_loss_long(a, fl, ll, il, 256)
    assert status() == 0                      # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    _check(k, 'after the refusals', costs, grads)


def test_unchanged_entry_points(dev):
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    assert not ops.ctc_train_supported(128, 64, 32)
    assert ops.ctc_long_supported(128, 64, 32)
    assert ops.ctc_train_supported(128, 64, 31)
    assert nat.lib().ocr_abi_version() == 1


def _no_adjacent_repeats(rng, L, lo, hi):
    out = []
    while len(out) < L:
        v = int(rng.randint(lo, hi))
        if not out or v != out[-1]:
            out.append(v)
    return out


def test_engine_long_path_against_parent_path(dev):
    from lstm_ctc_ocr_amd import dist as ocr_dist
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    N, W, L = 4, 256, 40
    rng = np.random.RandomState(41)
    x = rng.rand(N, W, 32).astype(np.float32)
    sl = np.full(N, W // 4 - 1, np.int32)
    labels = np.array([v for _ in range(N) for v in _no_adjacent_repeats(rng, L, 1, 63)], np.int32)
    ll = np.full(N, L, np.int32)

    def run(**kw):
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3, max_label_len=L, **kw)
        sp = eng.plan(N, W)
        eng._bind(sp, x, sl, labels, ll)
        eng._run(sp, 'fb')
        torch.cuda.synchronize()
        return eng.ctc_path(N, W), sp.costs.cpu().numpy().astype(np.float64), eng.ops[-1].dy(sp).float().cpu().numpy().astype(np.float64), sp
    path_l, cost_l, dy_l, sp = run(ctc_long=True)
    path_g, cost_g, dy_g, _ = run(ctc_long=False)
    assert (path_l, path_g) == ('long', 'general')
    scale = ocr_dist.loss_scale(N, 1)
    assert scale == 1.0 / N
    print('engine: costs long %s general %s; worst cost difference %.3e; worst dy difference %.3e (largest |dy| %.3e)'
          % (cost_l, cost_g, np.abs(cost_l - cost_g).max(), np.abs(dy_l - dy_g).max(), np.abs(dy_g).max()))
    assert np.all(cost_l > 0) and np.isfinite(cost_l).all()
    assert np.abs(cost_l - cost_g).max() <= 2 * lc.COST_BOUND
    assert dy_l.size == N * sp.T * sp.C and dy_l.shape == dy_g.shape and np.abs(dy_g).max() > 0      # [N][T][C], held as [N * T, C]
    tol = 2 * scale * lc.GRAD_BOUND + 2 * lr.half_ulp_bf16(np.maximum(np.abs(dy_l), np.abs(dy_g)))
    assert np.all(np.abs(dy_l - dy_g) <= tol)
    assert Engine(get_network('LSTM_train'), device='cuda:0', seed=3, max_label_len=31).ctc_path(N, W) == 'fast'
    with pytest.raises(ValueError, match='255'):
        Engine(get_network('LSTM_train'), device='cuda:0', seed=3, max_label_len=256)


def test_a_200_character_label_trains(dev):
    """A label the project could not score before: 200 characters at T = 420, C = 96."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    k = lc.case('line200')
    assert (k.T, k.C, int(k.ll.max())) == (420, 96, 200)
    a, fl, ll, il = _device_inputs(k, dev)
    gb = torch.full((k.N, k.T, k.C), NAN, dtype=BF, device=dev)
    costs, grads = ops.ctc_loss_long(a, fl, ll, il, k.mll, k.blank, grad_ntc_bf16=gb, scale=SCALE)
    torch.cuda.synchronize()
    _check(k, 'ops defaults', costs, grads, gb)
    with pytest.raises(nat.NativeError):
        ops.ctc_loss(a, fl, ll, il, k.mll, k.blank)


def test_warpctc_abi_takes_a_long_label(dev):
    """compute_ctc_loss refused a batch with a label over 127 characters; it now answers through the long form."""
    from lstm_ctc_ocr_amd import warpctc
    k = lc.case('L128')
    a = torch.from_numpy(k.acts).to(dev)
    costs, grads = warpctc.compute(a, k.flat, k.ll, np.minimum(k.il, k.T), blank_label=k.blank)
    torch.cuda.synchronize()
    _check(k, 'warp-ctc ABI', costs, grads)
