"""The BiLSTM kernels (lstm.hip, lstm_seq.hip) step by step against a float64 replay of each step from the device's own state of the step
before (tests/lstm_replay.py: derivation of every bound; tests/test_lstm_replay_model.py: the checker pinned on the CPU).

Every family goes through the same checker: the per-step kernels (two directions and one; U = 32, 256, 512), the persistent kernels
(four waves and one, hand-off block prepared by the call or by the caller), the persistent forward with the input projection inside, and
— in an interpreter of their own, the knobs being read once per process — the counter protocol and forced 32-row tiles.  Compared per
element, none excluded: the saved gates and cells (fp32, what the whole backward pass reads), hout and dz (bf16: half an ulp of storage
rounding plus the fp32 terms — truncation does not fit), the per-step kernels' dc_state, bit-zero hout / dz rows past a sample's length
(over 7.0 / 3.0 poison), and lstm_hprev bit for bit.  Value regimes: small random, the committed trained BiLSTM, saturating (asserted from
the replay: a quarter of the sigma gates outside [1e-3, 1 - 1e-3], 20 <= max |z| <= 60); forget_bias 1.0, 0.0 and 2.5; lengths all T, random,
and one vector with 0, 1, T and T + 5 in it.  Only finite values go in (bf16 0xFFFF is the persistent kernels' "not yet written" mark).

Asserted: worst |device - replay| / bound <= 1 per tensor.  Measured on MI355X (worst ratio over all cases of this file):
    per-step kernels, 2 directions   gates 0.47   cell 0.042   h 0.995   dz 0.997   dc_state 0.021
    per-step kernels, 1 direction    gates 0.47   cell 0.047   h 0.996   dz 0.998   dc_state 0.022
    persistent, four waves           gates 0.50   cell 0.041   h 0.982   dz 0.984
    persistent, one wave             gates 0.48   cell 0.041   h 0.982   dz 0.984
    projection inside                gates 0.0012 cell 0.0008  h 0.73                (K = D + U: the summation term dominates the bound)
    counter protocol / 32-row tiles  gates 0.47   cell 0.040   h 0.982   dz 0.984              (both runs of the subprocess test alike)
h and dz sit at the half ulp itself, as they should: the fp32 terms are three to four orders of magnitude below it (truncation: 1.96).
The gates' worst case is step 0, where z is the projection alone and the bound is the activation term alone: the hardware
activations use half of what the instruction accuracies allow."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_replay as lr  # noqa: E402

from lstm_ctc_ocr_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.float().cpu().numpy()


def _operands(dev, x, Ws, bs, U, ndir):
    """The executor's operand preparation: packed transposed weights, packed bias, bf16 input rows, master-order bf16 weights (backward)."""
    N, T, D = x.shape
    wxT = torch.empty((ndir * 4 * U, D), dtype=BF, device=dev)
    whT = torch.empty((ndir, 4 * U, U), dtype=BF, device=dev)
    whb = torch.empty((ndir, D + U, 4 * U), dtype=BF, device=dev)
    for d in range(ndir):
        Wd = torch.from_numpy(Ws[d]).to(dev)
        ops.pack_transpose(Wd[:D], wxT[d * 4 * U:(d + 1) * 4 * U], lstm_units=U, R=D, Cc=4 * U, ldin=4 * U)
        ops.pack_transpose(Wd[D:], whT[d], lstm_units=U, R=U, Cc=4 * U, ldin=4 * U)
        ops.cast_bf16(Wd.contiguous(), whb[d])
    bias = torch.empty(ndir * 4 * U, device=dev)
    ops.lstm_pack_bias(torch.from_numpy(bs[0]).to(dev), torch.from_numpy(bs[1 % len(bs)]).to(dev), bias, U, ndir)
    xd = torch.from_numpy(x).to(dev).to(BF).reshape(N * T, D)
    return dict(wxT=wxT, whT=whT, whb=whb, bias=bias, xd=xd)


def _fresh(dev, R, U, ndir):
    hout = torch.full((R, ndir * U), 7.0, dtype=BF, device=dev)            # poison: the kernels overwrite every row
    gates = torch.zeros((ndir, R, 4 * U), device=dev)
    cell = torch.zeros((ndir, R, U), device=dev)
    return hout, gates, cell


def _sync_block(dev, N, U, prepared):
    return torch.full((ops.lstm_seq_sync_words(N, U),), -1 if prepared else 0, dtype=torch.int32, device=dev)


def _no_timeout(sync, prepared, what):
    torch.cuda.synchronize()
    # prepared: the error word reads -1 (untouched) or 1 (time-out); the counter protocol ignores the flag and zeroes the block itself
    assert int(sync[-1]) in ((-1, 0) if prepared else (0,)), "persistent LSTM %s: spin time-out" % what


def _assert_forward(tag, fwd, regime):
    print('%s forward: %s; saturated %.3f, max |z| %.1f' % (tag, lr.report(fwd), fwd['sat_fraction'], fwd['max_abs_z']))
    for k in ('gates', 'cell', 'h', 'pad_h'):
        assert fwd[k].ratio <= 1.0, (tag, fwd[k])
    if regime == 'saturating':               # from the replay, so that the regime cannot silently drift back to the easy one
        assert fwd['sat_fraction'] >= 0.25 and 20.0 <= fwd['max_abs_z'] <= 60.0, (tag, fwd['sat_fraction'], fwd['max_abs_z'])


def _assert_backward(tag, bwd):
    print('%s backward: %s' % (tag, lr.report(bwd)))
    for k in bwd:
        assert bwd[k].ratio <= 1.0, (tag, bwd[k])


def _check_hprev(dev, hout, sl, seq_len, N, T, U, ndir):
    hprev = torch.full((ndir, N * T, U), 5.0, dtype=BF, device=dev)
    ops.lstm_hprev(hout, sl, hprev, N, T, U, ndir)
    got = hprev.view(torch.int16).cpu().numpy()
    want = lr.hprev_reference(hout.view(torch.int16).cpu().numpy(), seq_len, N, T, U, ndir)
    assert np.array_equal(got, want), "lstm_hprev: not the bits of the row before"


# ------------------------------------------------------------------------------------------------ per-step kernels
STEP_CASES = [
    # N,  T,  D,    U,   lengths,  regime,       forget_bias, ndir
    (64, 63, 512, 256, 'edges', 'trained', 0.0, 2),
    (64, 63, 512, 256, 'random', 'saturating', 2.5, 1),
    (64, 79, 512, 256, 'full', 'small', 0.0, 2),
    (32, 21, 1024, 512, 'random', 'saturating', 0.0, 2),
    (32, 21, 1024, 512, 'edges', 'small', 1.0, 1),
    (64, 1, 512, 256, 'full', 'small', 1.0, 1),
    (1, 9, 512, 256, 'random', 'trained', 2.5, 2),
    (17, 12, 512, 256, 'full', 'saturating', 1.0, 2),
    (17, 12, 64, 32, 'edges', 'small', 2.5, 2),
    (100, 12, 64, 256, 'edges', 'small', 0.0, 1),
    (200, 4, 64, 256, 'random', 'small', 1.0, 2),
    (200, 4, 64, 32, 'full', 'small', 0.0, 1),
]


@pytest.mark.parametrize("N,T,D,U,lens_kind,regime,forget_bias,ndir", STEP_CASES)
def test_step_kernels_against_the_step_replay(dev, N, T, D, U, lens_kind, regime, forget_bias, ndir):
    x, Ws, bs, dh = lr.make_case(regime, N, T, D, U)
    Ws, bs = Ws[:ndir], bs[:ndir]
    dh = np.ascontiguousarray(dh[:, :, :ndir * U])
    seq_len = lr.length_vector(lens_kind, N, T)
    R = N * T
    op = _operands(dev, x, Ws, bs, U, ndir)
    xproj = ops.gemm_nt(op['xd'], op['wxT'], bias=op['bias'], out_f32=True)
    sl = torch.tensor(seq_len, dtype=torch.int32, device=dev)
    hout, gates, cell = _fresh(dev, R, U, ndir)
    for s in range(T):
        ops.lstm_fwd_step(xproj, op['whT'], sl, hout, gates, cell, N, T, U, s, forget_bias, ndir)
    torch.cuda.synchronize()
    Wh = [w[D:] for w in Ws]
    tag = 'step ndir=%d %s' % (ndir, (N, T, D, U, lens_kind, regime, forget_bias))
    _assert_forward(tag, lr.forward_check(Wh, seq_len, N, T, U, _np(hout), _np(gates), _np(cell), forget_bias, xproj=_np(xproj), ndir=ndir), regime)
    dz = torch.full((R, ndir * 4 * U), 3.0, dtype=BF, device=dev)       # poison
    dc = torch.zeros((ndir, N, U), device=dev)
    dhd = torch.from_numpy(dh).to(dev).to(BF).reshape(R, ndir * U)
    for s in range(T - 1, -1, -1):
        ops.lstm_bwd_step(op['whb'][:, D:], 4 * U, (D + U) * 4 * U, sl, dhd, gates, cell, dz, dc, N, T, U, s, ndir)
    torch.cuda.synchronize()
    _assert_backward(tag, lr.backward_check(Wh, seq_len, N, T, U, _np(dhd), _np(gates), _np(cell), _np(dz), dc_state=_np(dc), ndir=ndir))
    _check_hprev(dev, hout, sl, seq_len, N, T, U, ndir)


# ------------------------------------------------------------------------------------------------ persistent kernels
SEQ_CASES = [
    # N,  T,  D,    U,   lengths,  regime,       forget_bias, (ksplit, prepared) runs
    pytest.param(64, 63, 512, 256, 'random', 'small', 1.0, ((4, False), (1, True)), id='headline-small'),
    pytest.param(64, 63, 512, 256, 'edges', 'trained', 0.0, ((4, True), (1, False)), id='headline-trained'),
    pytest.param(64, 63, 512, 256, 'full', 'saturating', 2.5, ((4, False),), id='headline-saturating'),
    pytest.param(64, 79, 512, 256, 'random', 'trained', 2.5, ((4, False), (1, False)), id='longest-trained'),
    pytest.param(64, 79, 512, 256, 'edges', 'saturating', 0.0, ((4, True),), id='longest-saturating'),
    pytest.param(32, 21, 1024, 512, 'random', 'small', 2.5, ((4, True), (1, False)), id='configs4-small'),
    pytest.param(32, 21, 1024, 512, 'edges', 'saturating', 1.0, ((4, False), (1, True)), id='configs4-saturating'),
    pytest.param(64, 1, 512, 256, 'full', 'small', 0.0, ((4, False), (1, False)), id='one-step'),
    pytest.param(1, 9, 512, 256, 'full', 'trained', 1.0, ((4, False), (1, False)), id='one-sample'),
    pytest.param(17, 12, 512, 256, 'edges', 'saturating', 2.5, ((4, False), (1, True)), id='ragged-tile'),
    pytest.param(100, 12, 64, 256, 'random', 'small', 0.0, ((4, True), (1, False)), id='hundred'),
    pytest.param(200, 4, 64, 256, 'edges', 'small', 1.0, ((4, False), (1, False)), id='tiles32'),
]


@pytest.mark.parametrize("N,T,D,U,lens_kind,regime,forget_bias,runs", SEQ_CASES)
def test_persistent_kernels_against_the_step_replay(dev, N, T, D, U, lens_kind, regime, forget_bias, runs):
    assert ops.lstm_seq_supported(N, U)
    x, Ws, bs, dh = lr.make_case(regime, N, T, D, U)
    seq_len = lr.length_vector(lens_kind, N, T)
    R = N * T
    op = _operands(dev, x, Ws, bs, U, 2)
    xproj = ops.gemm_nt(op['xd'], op['wxT'], bias=op['bias'], out_f32=True)
    sl = torch.tensor(seq_len, dtype=torch.int32, device=dev)
    dhd = torch.from_numpy(dh).to(dev).to(BF).reshape(R, 2 * U)
    Wh = [w[D:] for w in Ws]
    for ksplit, prepared in runs:
        tag = 'seq ksplit=%d prepared=%d %s' % (ksplit, prepared, (N, T, D, U, lens_kind, regime, forget_bias))
        ops.set_lstm_ksplit(ksplit)
        try:
            hout, gates, cell = _fresh(dev, R, U, 2)
            sync = _sync_block(dev, N, U, prepared)
            ops.lstm_fwd_seq(xproj, op['whT'], sl, hout, gates, cell, N, T, U, sync, forget_bias, prepared=prepared)
            _no_timeout(sync, prepared, 'forward')
            dz = torch.full((R, 8 * U), 3.0, dtype=BF, device=dev)
            sync = _sync_block(dev, N, U, prepared)
            ops.lstm_bwd_seq(op['whb'][:, D:], 4 * U, (D + U) * 4 * U, sl, dhd, gates, cell, dz, N, T, U, sync, prepared=prepared)
            _no_timeout(sync, prepared, 'backward')
        finally:
            ops.set_lstm_ksplit(4)
        _assert_forward(tag, lr.forward_check(Wh, seq_len, N, T, U, _np(hout), _np(gates), _np(cell), forget_bias, xproj=_np(xproj)), regime)
        _assert_backward(tag, lr.backward_check(Wh, seq_len, N, T, U, _np(dhd), _np(gates), _np(cell), _np(dz)))
        _check_hprev(dev, hout, sl, seq_len, N, T, U, 2)
    if D in (512, 1024) and ops.lstm_fwd_seq_x_supported(N, U, D):
        # the projection inside the recurrent kernel: no projection tensor, z = x Wx + b + h Wh summed over K = D + U
        for prepared in (False, True):
            tag = 'seq_x prepared=%d %s' % (prepared, (N, T, D, U, lens_kind, regime, forget_bias))
            hout, gates, cell = _fresh(dev, R, U, 2)
            sync = _sync_block(dev, N, U, prepared)
            ops.lstm_fwd_seq_x(op['xd'], op['wxT'], op['bias'], op['whT'], sl, hout, gates, cell, N, T, U, sync, forget_bias, prepared=prepared)
            torch.cuda.synchronize()
            assert int(sync[-1]) == (-1 if prepared else 0), "persistent LSTM forward with the projection inside: spin time-out"
            _assert_forward(tag, lr.forward_check(Wh, seq_len, N, T, U, _np(hout), _np(gates), _np(cell), forget_bias,
                                                  x=x, Wx=[w[:D] for w in Ws], b=bs), regime)


def test_the_fused_projection_kernel_covers_the_product_shapes(dev):
    """So that the loop above cannot silently stop reaching lstm_fwd_seq_x: under the default protocol the headline, the longest plan and
    configs[4] are covered (the counter protocol does not have the kernel: OCR_LSTM_PROTO=0 runs skip this)."""
    if os.environ.get('OCR_LSTM_PROTO') == '0':
        return
    assert ops.lstm_fwd_seq_x_supported(64, 256, 512) and ops.lstm_fwd_seq_x_supported(32, 512, 1024)


@pytest.mark.parametrize("env", [dict(OCR_LSTM_PROTO='0'), dict(OCR_LSTM_ROWS='32')])
def test_persistent_kernels_other_protocol_and_tiles(dev, env):
    """The counter protocol and 32-row workgroups forced where 16 rows are the default, through the same replay (the knobs are read once per
    process: an interpreter of its own per run, one after the other, each under a time limit)."""
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-s', '-k',
                          'test_persistent_kernels_against_the_step_replay and (headline or ragged or tiles32 or configs4-saturating)'],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:]
    assert ' passed' in out.stdout and 'skipped' not in out.stdout, out.stdout[-1000:]
    worst = {}
    for name, ratio in re.findall(r'(\w+): ratio ([0-9.e+-]+|inf)', out.stdout):
        worst[name] = max(worst.get(name, 0.0), float(ratio))
    print(env, 'worst ratios', worst)
    assert {'gates', 'cell', 'h', 'dz', 'pad_h', 'pad_dz'} <= set(worst) and max(worst.values()) <= 1.0, worst
