"""-m gpu: the wide beam-search kernel (ctc_beam.hip, WIDE = true) against the float64 oracles, forced on the shapes the table kernel
covers and dispatched automatically beyond them; the refusals; and the engine decoding a 512-class model.

Label sequences are compared exactly (the inputs are conditioned for that: tests/beam_wide_cases.py), -neg_log_prob within
1e-3 * max(1, |score|) of the oracle as in test_ctc_beam_search_matches_tf_semantics_oracle.  Every output buffer is pre-filled with a
sentinel so that a sample the kernel did not write shows."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_wide_cases as bw  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from oracle import decode as odec  # noqa: E402

SENTINEL = -7


def workspace_bytes(C, N, T, K):
    sz = ctypes.c_size_t(0)
    nat.call("ocr_ctc_beam_workspace_size", C, N, T, K, ctypes.byref(sz))
    return sz.value


def decode(dev, acts, il, K, merge):
    """ocr_ctc_beam_decode into sentinel-filled buffers -> (out [N, T], lens, nlp) as numpy."""
    T, N, C = acts.shape
    a = torch.tensor(acts, device=dev)
    l = torch.tensor(il, device=dev)
    out = torch.full((N, T), SENTINEL, dtype=torch.int32, device=dev)
    lens = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
    nlp = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(workspace_bytes(C, N, T, K), dtype=torch.uint8, device=dev)
    nat.call("ocr_ctc_beam_decode", a.data_ptr(), l.data_ptr(), C, N, T, K, int(merge), 0, out.data_ptr(), lens.data_ptr(),
             nlp.data_ptr(), ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy(), nlp.cpu().numpy()


def check(got, ref, scores, tag):
    out, lens, nlp = got
    worst = 0.0
    for n in range(out.shape[0]):
        assert 0 <= lens[n] <= out.shape[1], (tag, n, lens[n])
        assert out[n, :lens[n]].tolist() == ref[n], (tag, n, out[n, :lens[n]].tolist(), ref[n])
        assert (out[n, lens[n]:] == 0).all(), (tag, n)
        worst = max(worst, abs(-float(nlp[n]) - scores[n]))
        assert abs(-nlp[n] - scores[n]) < 1e-3 * max(1.0, abs(scores[n])), (tag, n, -nlp[n], scores[n])
    print("%s: worst |-nlp - score| = %.3e" % (tag, worst))


_tf_cases = {}


def tf_case(T, N, C, beam):
    """The inputs of test_ctc_beam_search_matches_tf_semantics_oracle and beam_search_tf's answer, once per shape (merge_repeated only
    post-processes the top path, so one search serves both settings; the (63, 8, 64, 100) search is 9 s of Python, the decodes are ms)."""
    key = (T, N, C, beam)
    if key not in _tf_cases:
        rng = np.random.RandomState(T + C)
        acts = (rng.randn(T, N, C) * 3).astype(np.float32)
        acts[rng.rand(T, N) < 0.3, C - 1] += 5.0
        acts[rng.rand(T, N) < 0.3, 0] += 5.0
        il = rng.randint(max(1, T // 2), T + 1, N).astype(np.int32)
        seqs, scores = odec.beam_search_tf(acts, il, beam_width=beam, merge_repeated=False)
        _tf_cases[key] = (acts, il, {False: seqs, True: [bw.merge_repeats(s) for s in seqs]}, scores)
    return _tf_cases[key]


@pytest.mark.parametrize("T,N,C,beam", [(12, 6, 8, 100), (20, 5, 16, 4), (63, 8, 64, 100), (30, 3, 96, 25), (7, 4, 5, 2)])
def test_forced_wide_kernel_matches_the_oracle_and_the_table_kernel(dev, T, N, C, beam):
    """M = min(K + 1, C - 1) clamps to C - 1 on the first and third shape (every class is selected) and prunes on the other three."""
    acts, il, ref, scores = tf_case(T, N, C, beam)
    try:
        for merge in (True, False):
            ops.set_beam_engine(0)
            assert ops.ctc_beam_kernel_choice(C, beam) == "table"
            table = decode(dev, acts, il, beam, merge)
            ops.set_beam_engine(2)
            assert ops.ctc_beam_kernel_choice(C, beam) == "wide"
            wide = decode(dev, acts, il, beam, merge)
            check(wide, ref[merge], scores, "forced wide %r merge=%d" % ((T, N, C, beam), merge))
            assert (wide[1] == table[1]).all() and (wide[0] == table[0]).all()
    finally:
        ops.set_beam_engine(0)


@pytest.mark.parametrize("shape", sorted(bw.CASES))
def test_wide_alphabets_under_automatic_dispatch(dev, shape):
    """The default engine on every case (ocr_ctc_beam_kernel_choice confirms which kernel that is); the one case whose K lets the table
    kernel fit is run on the forced wide kernel as well."""
    T, N, C, K = shape
    acts, il, ref = bw.build_case(*shape)
    try:
        for mode, kernel in bw.CASES[shape][1]:
            ops.set_beam_engine(2 if mode == "forced" else 0)
            assert ops.ctc_beam_kernel_choice(C, K) == kernel
            if kernel == "wide":
                assert any(v >= 256 for s in ref[False][0] for v in s)
            for merge in (True, False):
                check(decode(dev, acts, il, K, merge), ref[merge][0], ref[merge][1], "%s %s %r merge=%d" % (mode, kernel, shape, merge))
    finally:
        ops.set_beam_engine(0)


def test_refusals_return_invalid_and_launch_nothing(dev):
    T, N = 6, 3
    lib = nat.lib()
    st = nat.stream()

    def attempt(C, K, ws_bytes=None, null=None):
        acts = torch.zeros((T, N, min(C, 64)), dtype=torch.float32, device=dev)      # never read: the call must refuse before launching
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        out = torch.full((N, T), SENTINEL, dtype=torch.int32, device=dev)
        lens = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
        nlp = torch.full((N,), -1.0, dtype=torch.float32, device=dev)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        p = dict(acts=acts.data_ptr(), il=il.data_ptr(), out=out.data_ptr(), lens=lens.data_ptr(), ws=ws.data_ptr())
        if null:
            p[null] = None
        rc = lib.ocr_ctc_beam_decode(p["acts"], p["il"], C, N, T, K, 1, 0, p["out"], p["lens"], nlp.data_ptr(), p["ws"],
                                     ws.numel() if ws_bytes is None else ws_bytes, st)
        torch.cuda.synchronize()
        assert rc == 2, (C, K, ws_bytes, null, rc)
        assert (out == SENTINEL).all() and (lens == SENTINEL).all() and (nlp == -1.0).all()

    sz = ctypes.c_size_t(0)
    assert lib.ocr_ctc_beam_workspace_size(16385, N, T, 128, ctypes.byref(sz)) == 2
    assert lib.ocr_ctc_beam_workspace_size(64, N, T, 129, ctypes.byref(sz)) == 2
    attempt(16385, 128)
    attempt(64, 129)
    for C, K in ((64, 100), (512, 100)):                       # one byte short, table and wide kernel
        attempt(C, K, ws_bytes=workspace_bytes(C, N, T, K) - 1)
        for null in ("acts", "il", "out", "lens", "ws"):
            attempt(C, K, null=null)


def test_engine_decodes_a_512_class_model(dev):
    """cfg.NCLASSES = 512: Engine.decode's default method used to raise NativeError (the table kernel does not fit).  The CTC loss
    already trains such a model (whichever of its paths the plan takes); decode must work before and after a step."""
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    old = cfg.NCLASSES
    cfg.NCLASSES = 512
    try:
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3)
        N, W = 2, 64
        rng = np.random.RandomState(11)
        x = rng.rand(N, W, 32).astype(np.float32)
        sl = np.full(N, W // 4 - 1, np.int32)
        ll = np.array([3, 4], np.int32)
        labels = rng.randint(1, 511, size=int(ll.sum())).astype(np.int32)
        assert ops.ctc_beam_kernel_choice(512, 100) == "wide"
        print('CTC path of the 512-class plan:', eng.ctc_path(N, W))

        def decode_both():
            got = eng.decode(x, sl, method='beam')
            logits = eng.forward(x, sl).float()
            assert tuple(logits.shape) == (W // 4 - 1, N, 512)
            out, lens, _ = ops.ctc_beam_decode(logits.contiguous(), torch.from_numpy(sl).to(dev), beam_width=100)
            out, lens = out.cpu().numpy(), lens.cpu().numpy()
            assert got == [[int(v) for v in out[i, :lens[i]] if v != 0] for i in range(N)]
            return got

        decode_both()
        eng.setup_optimizer('Adam', 1e-4)
        loss = eng.train_step(x, labels, ll, sl)
        assert np.isfinite(loss)
        decode_both()
    finally:
        cfg.NCLASSES = old
