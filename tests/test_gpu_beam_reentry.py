"""-m gpu: beam search on flat logits, where prefixes leave the beam and come back (tests/beam_reentry_cases.py), on the table kernel
and the forced wide kernel of ctc_beam.hip, against the float64 oracle; and the decoder's edges (empty and one-frame inputs, beams of
1 and 2, the pad value, no score output).

Label sequences are compared exactly (every case is perturbation-stable by the oracle), -neg_log_prob within 1e-3 * max(1, |score|).
Every output buffer is pre-filled with a sentinel so that a sample the kernel did not write shows."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_reentry_cases as br  # noqa: E402
import beam_wide_cases as bw  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

SENTINEL = -7
IDS = ["T%d-N%d-C%d-K%d-s%g-seed%d" % c for c in br.CASES]


def decode(dev, acts, il, K, merge, pad=0, want_nlp=True):
    """ocr_ctc_beam_decode into sentinel-filled buffers -> (out [N, T], lens, nlp) as numpy; nlp stays NaN with want_nlp=False."""
    T, N, C = acts.shape
    a = torch.tensor(acts, device=dev)
    l = torch.tensor(np.asarray(il, np.int32), device=dev)
    out = torch.full((N, T), SENTINEL, dtype=torch.int32, device=dev)
    lens = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
    nlp = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    sz = ctypes.c_size_t(0)
    nat.call("ocr_ctc_beam_workspace_size", C, N, T, K, ctypes.byref(sz))
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    nat.call("ocr_ctc_beam_decode", a.data_ptr(), l.data_ptr(), C, N, T, K, int(merge), pad, out.data_ptr(), lens.data_ptr(),
             nlp.data_ptr() if want_nlp else None, ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy(), nlp.cpu().numpy()


def check(got, ref, scores, tag, pad=0, nlp_written=True):
    out, lens, nlp = got
    worst = 0.0
    for n in range(out.shape[0]):
        assert 0 <= lens[n] <= out.shape[1], (tag, n, lens[n])
        assert out[n, :lens[n]].tolist() == ref[n], (tag, n, out[n, :lens[n]].tolist(), ref[n])
        assert (out[n, lens[n]:] == pad).all(), (tag, n)
        if nlp_written:
            worst = max(worst, abs(-float(nlp[n]) - scores[n]))
            assert abs(-nlp[n] - scores[n]) < 1e-3 * max(1.0, abs(scores[n])), (tag, n, -nlp[n], scores[n])
        else:
            assert math.isnan(nlp[n]), (tag, n)
    print("%s: worst |-nlp - score| = %.3e" % (tag, worst))


def both_kernels(dev, acts, il, K, ref, tag, default_kernel="table", **kw):
    """Table kernel and forced wide kernel, merge_repeated on and off: each against `ref` = {merge: (sequences, scores)}, and equal."""
    C = acts.shape[2]
    try:
        for merge in (True, False):
            ops.set_beam_engine(0)
            assert ops.ctc_beam_kernel_choice(C, K) == default_kernel
            table = decode(dev, acts, il, K, merge, **kw)
            ops.set_beam_engine(2)
            assert ops.ctc_beam_kernel_choice(C, K) == "wide"
            wide = decode(dev, acts, il, K, merge, **kw)
            for name, got in ((default_kernel, table), ("forced wide", wide)):
                check(got, ref[merge][0], ref[merge][1], "%s %s merge=%d" % (name, tag, merge), pad=kw.get("pad", 0),
                      nlp_written=kw.get("want_nlp", True))
            assert (wide[0] == table[0]).all() and (wide[1] == table[1]).all()
            assert np.array_equal(wide[2], table[2], equal_nan=True)
    finally:
        ops.set_beam_engine(0)


def oracle(acts, il, K):
    """{merge: (sequences, scores)} of beam_search_pruned, input lengths clamped to T as the kernel clamps them."""
    il = np.minimum(np.asarray(il), acts.shape[0])
    seqs, scores = bw.beam_search_pruned(acts, il, beam_width=K, merge_repeated=False)
    return {False: (seqs, scores), True: ([bw.merge_repeats(s) for s in seqs], scores)}


@pytest.mark.parametrize("case", br.CASES, ids=IDS)
def test_prefixes_that_reenter_the_beam(dev, case):
    """At least two samples of every case decode differently when a re-entering prefix gets a second trie node
    (test_beam_reentry_cases.py).  The 300-class case runs the table kernel by default (K = 8) and prunes classes on the wide one."""
    T, N, C, K, scale, seed = case
    acts, il, ref = br.build_case(case)
    both_kernels(dev, acts, il, K, ref, repr(case))


def flat(T, N, C, seed, scale=1.0):
    return (np.random.RandomState(seed).randn(T, N, C) * scale).astype(np.float32)


def test_input_lengths_zero_one_and_beyond_T(dev):
    """input_len = 0 decodes to nothing with probability 1 (length 0, the row all pad, nlp = 0), also between neighbours that decode
    something; input_len = 1 sees one frame; input_len > T clamps to T."""
    T, N, C, K = 9, 6, 6, 5
    acts = flat(T, N, C, 3)
    acts[0, 3, 2] += 4.0                                       # the one-frame sample decodes [2]
    il = [T, 0, 5, 1, T + 7, 0]
    ref = oracle(acts, il, K)
    for n in (1, 5):
        assert ref[False][0][n] == [] and ref[False][1][n] == 0.0
    assert ref[False][0][3] == [2]
    assert abs(ref[False][1][3] - float(torch.log_softmax(torch.tensor(acts[0, 3], dtype=torch.float64), 0)[2])) < 1e-12
    full = oracle(acts[:, 4:5], [T], K)
    assert ref[False][0][4] == full[False][0][0] and ref[False][1][4] == full[False][1][0]
    both_kernels(dev, acts, il, K, ref, "lengths %r" % (il,))
    ops.set_beam_engine(0)
    out, lens, nlp = decode(dev, acts, il, K, True)
    for n in (1, 5):
        assert lens[n] == 0 and (out[n] == 0).all() and nlp[n] == 0.0
    both_kernels(dev, acts[:, :2], [0, 0], K, oracle(acts[:, :2], [0, 0], K), "all lengths zero")


@pytest.mark.parametrize("T,N,C,K", [(12, 4, 7, 1), (10, 5, 2, 2), (10, 3, 2, 1)])
def test_beams_of_one_and_two(dev, T, N, C, K):
    """K = 1 keeps the single best of leaf and children each frame; at C = 2 there are only the blank and one label, so M = 1."""
    acts = flat(T, N, C, 10 * C + K)
    acts[::3, :, C - 1] += 1.5                                 # some blank frames, so that repeats of the one label separate
    il = [T] + list(range(T - N + 1, T))
    ref = oracle(acts, il, K)
    assert any(len(s) > 1 for s in ref[False][0])
    both_kernels(dev, acts, il, K, ref, "K=%d C=%d" % (K, C))


def test_beam_of_one_by_hand(dev):
    """Two frames, classes (a, blank), K = 1, p(a) = 0.6 then 0.3.  Frame 0: [a] 0.6 beats [] 0.4.  Frame 1: [a] stays with
    0.6 * (0.3 + 0.7) = 0.6; its child [a, a] needs a blank in between and has none (p_blank of [a] is 0)."""
    p = np.array([[0.6, 0.4], [0.3, 0.7]])
    acts = np.log(p).astype(np.float32).reshape(2, 1, 2)
    ref = {m: ([[0]], [math.log(0.6)]) for m in (True, False)}
    both_kernels(dev, acts, [2], 1, ref, "by hand")


def test_pad_value_and_no_score_output(dev):
    T, N, C, K = 11, 4, 6, 6
    acts = flat(T, N, C, 21)
    il = [T, 6, 0, 9]
    ref = oracle(acts, il, K)
    assert all(len(s) < T for s in ref[False][0])              # every row has a tail to pad
    both_kernels(dev, acts, il, K, ref, "pad -1", pad=-1)
    both_kernels(dev, acts, il, K, ref, "no nlp", want_nlp=False)
    both_kernels(dev, acts, il, K, ref, "pad -1, no nlp", pad=-1, want_nlp=False)
