"""CTC (ctc.hip, ctc_common.h) where the product trains: on the TRAINED logits of the committed fixture, and on the boundary shapes of the fast kernel.

Trained logits (tests/golden/trained_expect.npz, all five batches; labels and lengths from captcha_batches.npz).  A trained network's
cost per sample is 9e-5 .. 6e-2 (median 3.5e-4) and its largest gradient entry 0.012 .. 0.06, so the bounds of the random-logit cases
(1e-4 absolute on a cost, 5e-4 on a gradient entry) would let a cost be wrong by a quarter of itself.  Reference: the float64 oracle
(oracle/ctc.py::ctc_loss_numpy).  Bounds: fp32 log-space arithmetic has a floor of its own — logy = act - lse rounds at 2^-24 |lse|, about
1.5e-6 per frame with lse near 25, and a cost sums T such terms — which is MEASURED on the reference side: the same recursion in numpy
float32 (ctc_recursion below) against the float64 oracle on these fixtures.  The bound is 8 x that floor: the fast kernel's recursion uses the
hardware v_exp_f32 / v_log_f32 forms, about 2^-21 relative against libm's 2^-24.

                                   float32 floor     bound (8 x)     device, measured on MI355X (worst of both engines / all forms)
    cost, absolute                 8.11e-6 (C2)      6.49e-5         7.89e-6 (V0; 7.12e-6 on C2)
    gradient entry, absolute       1.38e-6 (V1)      1.10e-5         1.30e-6 (C2, fast kernel)
    bf16 gradient of the training form: |dev - 0.25 ref| / (0.25 x 1.10e-5 + half a bf16 ulp of 0.25 ref) <= 1; measured 0.72 (C2)

test_float32_floor_is_what_the_bounds_quote (no GPU) recomputes the floor, so the constants cannot drift from the reference."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)
import make_trained_fixture as fx  # noqa: E402
import lstm_replay as lr  # noqa: E402

from oracle import ctc as octc  # noqa: E402

BF = torch.bfloat16
# worst |float32 recursion - float64 oracle| over the five batches, measured on the CPU (printed by the no-GPU test below):
COST_FLOOR = 8.111e-06    # C2: T = 63, the batch with the largest cost (6.4e-2)
GRAD_FLOOR = 1.379e-06    # V1
COST_BOUND = 8 * COST_FLOOR
GRAD_BOUND = 8 * GRAD_FLOOR


def _lse(rows, axis):
    m = rows.max(axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0).astype(rows.dtype)
    with np.errstate(divide='ignore'):
        return (m + np.log(np.exp(rows - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def ctc_recursion(act, flat_labels, label_lengths, input_lengths, blank, dtype):
    """The kernels' recursion (log-softmax denominators, alpha and beta in log space both including the frame's own logy, posteriors
    exp(alpha + beta - logy - logp)) with every operation in `dtype`."""
    act = np.asarray(act, dtype)
    T, N, C = act.shape
    costs = np.zeros(N, dtype); grad = np.zeros_like(act)
    NEG = dtype(-np.inf)
    off = 0
    for n in range(N):
        L = int(label_lengths[n]); Tn = min(int(input_lengths[n]), T)
        lab = [int(v) for v in flat_labels[off:off + L]]; off += L
        rep = sum(1 for i in range(1, L) if lab[i] == lab[i - 1])
        if L + rep > Tn or Tn <= 0:
            continue
        ext = np.full(2 * L + 1, blank); ext[1::2] = lab
        S = len(ext)
        skip = np.zeros(S, bool); skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        rows = act[:Tn, n]
        lse = _lse(rows, 1)
        logy = rows[:, ext] - lse[:, None]
        a = np.full((Tn, S), NEG, dtype); b = np.full((Tn, S), NEG, dtype)
        a[0, :2] = logy[0, :2]
        for t in range(1, Tn):
            p = a[t - 1]
            c = np.full((3, S), NEG, dtype)
            c[0] = p; c[1, 1:] = p[:-1]; c[2, 2:] = np.where(skip[2:], p[:-2], NEG)
            a[t] = _lse(c, 0) + logy[t]
        logp = _lse(a[Tn - 1, max(S - 2, 0):], 0)
        costs[n] = -logp
        b[Tn - 1, max(S - 2, 0):] = logy[Tn - 1, max(S - 2, 0):]
        for t in range(Tn - 2, -1, -1):
            p = b[t + 1]
            c = np.full((3, S), NEG, dtype)
            c[0] = p; c[1, :-1] = p[1:]; c[2, :-2] = np.where(skip[2:], p[2:], NEG)
            b[t] = _lse(c, 0) + logy[t]
        with np.errstate(invalid='ignore'):
            gamma = np.where(np.isfinite(a + b), np.exp(a + b - logy - logp), dtype(0)).astype(dtype)
        post = np.zeros((Tn, C), dtype)
        for s in range(S):
            post[:, ext[s]] += gamma[:, s]
        grad[:Tn, n] = np.exp(rows - lse[:, None]) - post
    return costs, grad


_CACHE = {}


def trained_batch(name):
    """-> logits [T, N, C] float32, flat labels, label lengths, input lengths, float64 oracle costs and gradients (cached)."""
    if name not in _CACHE:
        d, e = np.load(fx.BATCHES), np.load(fx.EXPECT)
        _, labels, ll, sl = fx.load_batch(d, name)
        acts = np.ascontiguousarray(e[name + '/logits'], np.float32)
        ref_c, ref_g = octc.ctc_loss_numpy(acts, labels, ll, sl, 0)
        _CACHE[name] = (acts, labels.astype(np.int32), ll.astype(np.int32), sl.astype(np.int32), ref_c, ref_g)
    return _CACHE[name]


def test_float32_floor_is_what_the_bounds_quote():
    worst_c = worst_g = 0.0
    for name in fx.NAMES:
        acts, labels, ll, sl, ref_c, ref_g = trained_batch(name)
        c64, g64 = ctc_recursion(acts, labels, ll, sl, 0, np.float64)
        assert np.abs(c64 - ref_c).max() < 1e-11 and np.abs(g64 - ref_g).max() < 1e-12      # the same recursion as the oracle's
        c32, g32 = ctc_recursion(acts, labels, ll, sl, 0, np.float32)
        ec, eg = float(np.abs(c32 - ref_c).max()), float(np.abs(g32 - ref_g).max())
        print('%s: T=%d N=%d float32 floor: cost %.3e, gradient entry %.3e; costs %.2e .. %.2e, largest gradient entry %.3g, logits %.1f .. %.1f'
              % (name, acts.shape[0], acts.shape[1], ec, eg, ref_c[ref_c > 0].min(), ref_c.max(), np.abs(ref_g).max(), acts.min(), acts.max()))
        worst_c, worst_g = max(worst_c, ec), max(worst_g, eg)
    print('float32 floor over the five batches: cost %.3e, gradient entry %.3e' % (worst_c, worst_g))
    # libm builds differ in the last bit: the quoted floor is the measured one within a factor of two, and never below it by more than that
    assert COST_FLOOR / 2 <= worst_c <= COST_FLOOR * 2, (worst_c, COST_FLOOR)
    assert GRAD_FLOOR / 2 <= worst_g <= GRAD_FLOOR * 2, (worst_g, GRAD_FLOOR)
    k = int(np.argmin(trained_batch('V0')[3]))
    assert trained_batch('V0')[4][k] == 0 and not trained_batch('V0')[5][:, k].any()          # V0's infeasible sample


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(fx.NAMES))
def test_trained_logits(dev, name):
    """Both engines with gradients, the score-only call and the training form; the measured figures are in the module docstring."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    acts, labels, ll, sl, ref_c, ref_g = trained_batch(name)
    T, N, C = acts.shape
    mll = int(ll.max())
    a = torch.from_numpy(acts).to(dev)
    fl, lld, sld = (torch.from_numpy(v).to(dev) for v in (labels, ll, sl))
    infeasible = ref_c == 0
    assert infeasible.sum() == (1 if name == 'V0' else 0)

    def check(tag, costs, grads=None):
        c = costs.cpu().numpy().astype(np.float64)
        ec = float(np.abs(c - ref_c).max())
        msg = '%s %s: cost error %.3e (bound %.3e, float32 floor %.3e)' % (name, tag, ec, COST_BOUND, COST_FLOOR)
        assert np.all(c[infeasible] == 0), (tag, c[infeasible])
        eg = None
        if grads is not None:
            g = grads.cpu().numpy().astype(np.float64)
            eg = float(np.abs(g - ref_g).max())
            msg += '; gradient error %.3e (bound %.3e, float32 floor %.3e)' % (eg, GRAD_BOUND, GRAD_FLOOR)
            assert not g[:, infeasible].any(), tag
        print(msg)
        assert ec <= COST_BOUND, msg
        assert eg is None or eg <= GRAD_BOUND, msg

    try:
        for engine in (0, 1):                 # the general one-wave kernel and the LDS-resident fast kernel
            nat.call("ocr_set_ctc_engine", engine)
            grads = torch.full_like(a, 7.0)
            costs, grads = ops.ctc_loss(a, fl, lld, sld, mll, 0, grads=grads)
            torch.cuda.synchronize()
            check('engine %d' % engine, costs, grads)
            costs2, _ = ops.ctc_loss(a, fl, lld, sld, mll, 0, want_grad=False)
            torch.cuda.synchronize()
            check('engine %d score only' % engine, costs2)
    finally:
        nat.call("ocr_set_ctc_engine", 1)
    assert ops.ctc_train_supported(C, T, mll)
    scale = 0.25
    gb = torch.full((N, T, C), 7.0, dtype=BF, device=dev)
    c3 = torch.empty(N, device=dev)
    ops.ctc_loss_train(a, gb, scale, fl, lld, sld, mll, c3, 0)
    torch.cuda.synchronize()
    check('train form', c3)
    want = scale * np.transpose(ref_g, (1, 0, 2))
    got = gb.float().cpu().numpy().astype(np.float64)
    # the fp32 gradient within its bound, scaled exactly (a power of two), then ONE rounding to bf16: half an ulp of the reference on top
    bound = scale * GRAD_BOUND + lr.half_ulp_bf16(want)
    ratio = np.abs(got - want) / bound
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print('%s train form: bf16 gradient worst |dev - ref| / bound %.3f at %s (ref %.3e)' % (name, ratio[k], k, want[k]))
    assert ratio[k] <= 1.0
    assert not got[infeasible].any()


# ------------------------------------------------------------------------------------------------ boundary shapes of the fast kernel
def _ctc_case():
    import test_gpu_kernels as tk
    return tk._ctc_case


def _repeats(labels):
    return sum(1 for i in range(1, len(labels)) if labels[i] == labels[i - 1])


@pytest.mark.gpu
def test_boundary_shapes(dev):
    from lstm_ctc_ocr_amd import ops
    case = _ctc_case()
    # L = 31: S = 63, the last slot count the 64-lane recursion covers; T = 64, C = 128: the last shape with the frames cached in registers
    assert ops.ctc_train_supported(128, 64, 31)
    case(dev, 64, 4, 128, [31, 31, 30, 1], [64, 63, 64, 5], 21)
    # L = 32: S = 65, refused by the fast kernel; the general kernel answers
    assert not ops.ctc_train_supported(128, 64, 32)
    case(dev, 64, 3, 128, [32, 31, 7], [64, 64, 40], 22)
    # T = 65, C = 129: one past `cached` on either side; C = 65: a partial second lane group
    case(dev, 65, 4, 128, [10, 31, 3, 12], [65, 64, 65, 30], 23)
    case(dev, 64, 4, 129, [10, 31, 3, 12], [64, 64, 33, 30], 24)
    case(dev, 65, 3, 129, [10, 20, 3], [65, 64, 20], 25)
    case(dev, 63, 5, 65, [10, 9, 3, 10, 1], [63, 40, 63, 21, 2], 26)
    # one repeated character: L + repeats == T is just feasible (a single alignment), L + repeats == T + 1 is not (cost 0, gradient 0)
    labels = [[5, 5, 7, 3], [5, 5, 7, 3], [2, 2, 2], [2, 2, 2], [4, 9]]
    in_lens = [5, 4, 5, 4, 12]
    assert [len(l) + _repeats(l) - t for l, t in zip(labels, in_lens)] == [0, 1, 0, 1, -10]
    case(dev, 12, 5, 16, None, in_lens, 27, labels=labels)
    ref_c, _ = octc.ctc_loss_c((np.random.RandomState(27).randn(12, 5, 16) * 2).astype(np.float32), np.array([v for l in labels for v in l], np.int32),
                               np.array([len(l) for l in labels], np.int32), np.array(in_lens, np.int32), 0)
    assert ref_c[1] == 0 and ref_c[3] == 0 and ref_c[0] > 0 and ref_c[2] > 0


@pytest.mark.gpu
def test_table_stride_larger_than_every_label(dev):
    """max_label_len = 20 for labels of at most 10: the table stride SMAX = 41 differs from every S (_ctc_case always passes the batch
    maximum).  Both engines, the score-only call and the training form, against the float64 oracle at _ctc_case's bounds."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    T, N, C, MLL = 63, 6, 64, 20
    rng = np.random.RandomState(31)
    acts = (rng.randn(T, N, C) * 2).astype(np.float32)
    labels = [rng.randint(1, C, size=l).tolist() for l in (10, 4, 7, 10, 1, 9)]
    flat = np.array([v for l in labels for v in l], np.int32)
    ll = np.array([len(l) for l in labels], np.int32)
    il = np.array([63, 40, 63, 21, 2, 63], np.int32)
    ref_c, ref_g = octc.ctc_loss_numpy(acts, flat, ll, il, 0)
    a = torch.from_numpy(acts).to(dev)
    fl, lld, ild = (torch.from_numpy(v).to(dev) for v in (flat, ll, il))
    try:
        for engine in (0, 1):
            nat.call("ocr_set_ctc_engine", engine)
            costs, grads = ops.ctc_loss(a, fl, lld, ild, MLL, 0)
            torch.cuda.synchronize()
            assert np.allclose(costs.cpu().numpy(), ref_c, rtol=1e-4, atol=1e-4), (engine, costs.cpu().numpy(), ref_c)
            assert np.abs(grads.cpu().numpy() - ref_g).max() < 5e-4, (engine, np.abs(grads.cpu().numpy() - ref_g).max())
            costs2, _ = ops.ctc_loss(a, fl, lld, ild, MLL, 0, want_grad=False)
            assert np.allclose(costs2.cpu().numpy(), ref_c, rtol=1e-4, atol=1e-4)
    finally:
        nat.call("ocr_set_ctc_engine", 1)
    assert ops.ctc_train_supported(C, T, MLL)
    gb = torch.full((N, T, C), 7.0, dtype=BF, device=dev)
    c3 = torch.empty(N, device=dev)
    ops.ctc_loss_train(a, gb, 0.25, fl, lld, ild, MLL, c3, 0)
    torch.cuda.synchronize()
    assert np.allclose(c3.cpu().numpy(), ref_c, rtol=1e-4, atol=1e-4)
    want = 0.25 * np.transpose(ref_g, (1, 0, 2))
    assert np.all(np.abs(gb.float().cpu().numpy() - want) <= 0.25 * 5e-4 + lr.half_ulp_bf16(want))
