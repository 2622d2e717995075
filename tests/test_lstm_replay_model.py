"""The step replay checker (tests/lstm_replay.py) pinned on the CPU: a float32 emulation of the BiLSTM recurrence as the kernels compute it
(bf16 h, fp32 cell, packed gate columns, ragged and clamped lengths, poisoned outputs) must come out at or below 1 in every value regime
the GPU tests use — the reference stays inside its own bounds — and each mutant of the emulation must come out above 1: the checker
catches what tests/test_gpu_lstm_replay.py is there to catch.  The emulation's activations are libm's float32 ones (correctly rounded to
~1 ulp), not the hardware's: the activation term of the bounds is derived in lstm_replay.py from the instruction accuracies."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_replay as lr  # noqa: E402

F = np.float32


def _mm(a, b):
    return (torch.from_numpy(np.ascontiguousarray(a, F)) @ torch.from_numpy(np.ascontiguousarray(b, F))).numpy()


def _sig(a):
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(a, F))).numpy()


def _tanh(a):
    return torch.tanh(torch.from_numpy(np.ascontiguousarray(a, F))).numpy()


def emulate_forward(x, Ws, bs, seq_len, U, forget_bias, mutant=None):
    N, T, D = x.shape
    lens = lr.clamped_lengths(seq_len, T)
    xp = np.stack([_mm(x.reshape(N * T, D), Ws[d][:D]) + bs[d].astype(F) for d in range(2)], 1).reshape(N, T, 2, 4, U)
    hout = np.full((N, T, 2, U), 7.0, F)                     # poison: every row is overwritten
    gates = np.zeros((2, N, T, 4, U), F); cell = np.zeros((2, N, T, U), F)
    fb = F(1.0 if mutant == 'ignore_forget_bias' else forget_bias)
    for d in range(2):
        Wh = Ws[d][D:]
        for s in range(T):
            hout[lens <= s, s, d] = 0.0
            idx = np.nonzero(lens > s)[0]
            if idx.size == 0:
                continue
            t = np.full(idx.size, s) if d == 0 else lens[idx] - 1 - s
            tp = t - 1 if d == 0 else t + 1
            z = xp[idx, t, d].copy()
            cp = np.zeros((idx.size, U), F)
            if s > 0:
                z += _mm(hout[idx, tp, d], Wh).reshape(-1, 4, U)
                cp = cell[d, idx, tp]
            gi, gj, gf, go = _sig(z[:, 0]), _tanh(z[:, 1]), _sig(z[:, 2] + fb), _sig(z[:, 3])
            c = gf * cp + gi * gj
            if mutant == 'bf16_cell':
                c = lr.bf16_round(c)
            h = go * _tanh(c)
            hout[idx, t, d] = lr.bf16_trunc(h) if mutant == 'truncated_h' else lr.bf16_round(h)
            cell[d, idx, t] = c
            gates[d, idx, t] = np.stack([gi, gf, gj, go] if mutant == 'swapped_gates' else [gi, gj, gf, go], 1)
    return dict(xproj=lr.pack_gate_columns(xp, U).reshape(N * T, 8 * U), hout=hout.reshape(N * T, 2 * U),
                gates=lr.pack_gate_columns(gates, U).reshape(2, N * T, 4 * U), cell=cell.reshape(2, N * T, U))


def emulate_backward(Ws, D, seq_len, N, T, U, dhout, gates, cell, mutant=None):
    """lstm_bwd_step_kernel, step by step: -> dz [R, 8U] (bf16 values, master columns), dc_state [2, N, U]."""
    lens = lr.clamped_lengths(seq_len, T)
    dhout = dhout.reshape(N, T, 2, U)
    gates = lr.unpack_gate_columns(gates.reshape(2, N, T, 4 * U), U)
    cell = cell.reshape(2, N, T, U)
    dz = np.full((N, T, 2, 4, U), 3.0, F)                    # poison
    dcs = np.zeros((2, N, U), F)
    for d in range(2):
        Wh = Ws[d][D:]
        for s in range(T - 1, -1, -1):
            if mutant != 'padding_dz_kept':
                dz[lens <= s, s, d] = 0.0
            idx = np.nonzero(lens > s)[0]
            if idx.size == 0:
                continue
            n = idx.size
            t = np.full(n, s) if d == 0 else lens[idx] - 1 - s
            has_next = lens[idx] > s + 1
            tn = np.where(has_next, t + 1 if d == 0 else t - 1, 0)            # the kernel's row: frame 0 when there is no next step
            dh = np.zeros((n, U), F)
            if s + 1 < T:
                dh = _mm(dz[idx, tn, d].reshape(n, 4 * U), Wh.T)
            if mutant != 'has_next_dropped':
                dh[~has_next] = 0.0
            dh = dh + dhout[idx, t, d]
            gi, gj, gf, go = (gates[d, idx, t, g] for g in range(4))
            c = cell[d, idx, t]
            cp = cell[d, idx, t - 1 if d == 0 else t + 1] if s > 0 else np.zeros((n, U), F)
            tc = _tanh(c)
            dc = dcs[d, idx] + dh * go * (F(1) - tc * tc)
            out = np.stack([dc * gj * gi * (F(1) - gi), dc * gi * (F(1) - gj * gj), dc * cp * gf * (F(1) - gf), dh * tc * go * (F(1) - go)], 1)
            dz[idx, t, d] = lr.bf16_round(out)
            dcs[d, idx] = dc * gf
    return dz.reshape(N * T, 8 * U), dcs


def _run(regime, N, T, D, U, lens_kind, forget_bias, fwd_mutant=None, bwd_mutant=None, fused=False):
    x, Ws, bs, dh = lr.make_case(regime, N, T, D, U)
    seq_len = lr.length_vector(lens_kind, N, T)
    st = emulate_forward(x, Ws, bs, seq_len, U, forget_bias, fwd_mutant)
    Wh = [w[D:] for w in Ws]
    if fused:
        fwd = lr.forward_check(Wh, seq_len, N, T, U, st['hout'], st['gates'], st['cell'], forget_bias, x=x, Wx=[w[:D] for w in Ws], b=bs)
    else:
        fwd = lr.forward_check(Wh, seq_len, N, T, U, st['hout'], st['gates'], st['cell'], forget_bias, xproj=st['xproj'])
    dz, dcs = emulate_backward(Ws, D, seq_len, N, T, U, dh, st['gates'], st['cell'], bwd_mutant)
    bwd = lr.backward_check(Wh, seq_len, N, T, U, dh, st['gates'], st['cell'], dz, dc_state=dcs)
    return fwd, bwd


SHAPE = dict(small=(8, 21, 64, 32), trained=(8, 21, 512, 256), saturating=(8, 21, 512, 256))


@pytest.mark.parametrize('regime', lr.REGIMES)
@pytest.mark.parametrize('lens_kind', ['full', 'random', 'edges'])
@pytest.mark.parametrize('forget_bias', [1.0, 0.0, 2.5])
def test_clean_emulation_stays_inside_the_bounds(regime, lens_kind, forget_bias):
    fwd, bwd = _run(regime, *SHAPE[regime], lens_kind, forget_bias, fused=(forget_bias == 2.5))
    print(regime, lens_kind, forget_bias, lr.report(fwd), lr.report(bwd), 'saturated %.3f max |z| %.1f' % (fwd['sat_fraction'], fwd['max_abs_z']))
    for k in ('gates', 'cell', 'h', 'pad_h'):
        assert fwd[k].ratio <= 1.0, fwd[k]
    for k in ('dz', 'pad_dz', 'dc_state'):
        assert bwd[k].ratio <= 1.0, bwd[k]
    assert fwd['h'].count == 2 * SHAPE[regime][3] * int(lr.clamped_lengths(lr.length_vector(lens_kind, *SHAPE[regime][:2]), SHAPE[regime][1]).sum())
    if regime == 'saturating':              # the regime is what it says: from the replay itself
        assert fwd['sat_fraction'] >= 0.25 and 20.0 <= fwd['max_abs_z'] <= 60.0, (fwd['sat_fraction'], fwd['max_abs_z'])
    else:
        assert fwd['sat_fraction'] < 0.25


@pytest.mark.parametrize('regime', lr.REGIMES)
@pytest.mark.parametrize('mutant,tensor', [('truncated_h', 'h'), ('bf16_cell', 'cell'), ('ignore_forget_bias', 'gates'), ('swapped_gates', 'gates')])
def test_forward_mutants_leave_the_bounds(regime, mutant, tensor):
    fwd, _ = _run(regime, *SHAPE[regime], 'random', 0.0, fwd_mutant=mutant)
    print(regime, mutant, lr.report(fwd))
    assert fwd[tensor].ratio > 1.0, fwd[tensor]


@pytest.mark.parametrize('regime', lr.REGIMES)
@pytest.mark.parametrize('mutant,tensor', [('has_next_dropped', 'dz'), ('padding_dz_kept', 'pad_dz')])
def test_backward_mutants_leave_the_bounds(regime, mutant, tensor):
    _, bwd = _run(regime, *SHAPE[regime], 'random', 1.0, bwd_mutant=mutant)
    print(regime, mutant, lr.report(bwd))
    assert bwd[tensor].ratio > 1.0, bwd[tensor]


def test_half_ulp_and_layout_helpers():
    assert lr.half_ulp_bf16(0.75) == 2.0 ** -9 and lr.half_ulp_bf16(1.0) == 2.0 ** -8 and lr.half_ulp_bf16(-0.3) == 2.0 ** -10
    v = np.array([1.00390625 + 2.0 ** -9, 1.0 + 2.0 ** -8, -0.7], F)          # a tie goes to the even neighbour
    assert lr.bf16_round(v).tolist()[1] == 1.0 and abs(lr.bf16_trunc(v)[2]) <= 0.7
    assert np.all(np.abs(lr.bf16_round(v).astype(np.float64) - v) <= lr.half_ulp_bf16(v))
    U = 32
    p = lr.packed_columns(U)
    assert p[2, 17] == 64 + 32 + 1 and sorted(p.ravel().tolist()) == list(range(4 * U))
    a = np.arange(4 * U, dtype=F).reshape(4, U)
    assert np.array_equal(lr.unpack_gate_columns(lr.pack_gate_columns(a, U), U), a)
    assert lr.bit_zero(np.array([0.0, -0.0, 1.0], F)).tolist() == [True, False, False]
    h = np.arange(2 * 3 * 2 * 8, dtype=F).reshape(2 * 3, 2 * 8) + 1
    hp = lr.hprev_reference(h, [3, 2], 2, 3, 8).reshape(2, 2, 3, 8)
    hh = h.reshape(2, 3, 2, 8)
    assert np.array_equal(hp[0, 0, 1], hh[0, 0, 0]) and not hp[0, 0, 0].any() and np.array_equal(hp[1, 0, 0], hh[0, 1, 1]) and not hp[1, 0, 2].any()
    assert not hp[:, 1, 2].any() and np.array_equal(hp[1, 1, 0], hh[1, 1, 1]) and not hp[1, 1, 1].any()
