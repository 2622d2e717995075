"""The pruning the wide beam-search kernel rests on, the committed cases of test_gpu_beam_wide.py and the host-only dispatch query:
everything here runs without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_wide_cases as bw  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from oracle import decode as odec  # noqa: E402

# (T, N, C, K): pruning bites (K + 1 < C - 1) on the first four, not on the last
PRUNE_SHAPES = [(12, 6, 40, 3), (15, 4, 64, 8), (20, 3, 50, 5), (8, 4, 300, 4), (10, 3, 24, 30)]
_full = {}


def _case(T, N, C, K):
    """Logits (peaky samples from the case builder, the last sample flat randn) and beam_search_tf's answer, computed once per shape."""
    key = (T, N, C, K)
    if key not in _full:
        acts, il = bw.make_logits(T, N, C, seed=T + C)
        acts[:, N - 1, :] = np.random.RandomState(C).randn(T, C).astype(np.float32)
        seqs, scores = odec.beam_search_tf(acts, il, beam_width=K, merge_repeated=False)
        acts.setflags(write=False)
        _full[key] = (acts, il, seqs, scores)
    return _full[key]


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("T,N,C,K", PRUNE_SHAPES)
def test_pruned_oracle_equals_the_full_one(T, N, C, K, merge):
    acts, il, seqs, scores = _case(T, N, C, K)
    want, want_scores = odec.beam_search_tf(acts, il, beam_width=K, merge_repeated=merge) if merge else (seqs, scores)
    got, got_scores = bw.beam_search_pruned(acts, il, beam_width=K, merge_repeated=merge)
    assert got == want
    assert max(abs(a - b) for a, b in zip(got_scores, want_scores)) < 1e-9


def test_a_wrong_pruning_is_seen():
    """Only the K - 1 likeliest classes, without the last label and the in-beam children: must disagree with the full search somewhere."""
    differs = 0
    for (T, N, C, K) in PRUNE_SHAPES:
        acts, il, seqs, scores = _case(T, N, C, K)
        top = lambda row, blank, K=K: bw.select_classes(row, blank, max(K - 1, 0))
        got, got_scores = bw.beam_search_pruned(acts, il, beam_width=K, merge_repeated=False, select=top, extras=False)
        differs += (got != seqs) or max(abs(a - b) for a, b in zip(got_scores, scores)) >= 1e-9
    assert differs >= 1


@pytest.mark.parametrize("shape", sorted(bw.SEEDS))
def test_committed_cases_meet_their_conditions(shape):
    T, N, C, K = shape
    acts, il, ref = bw.build_case(*shape)
    assert acts.dtype == np.float32 and acts.shape == (T, N, C) and il.min() >= 1 and il.max() == T
    ok, why = bw.conditions(acts, il, K, bw.is_wide_case(shape))
    assert ok, why
    assert ref[True][0] == [bw.merge_repeats(s) for s in ref[False][0]]


def test_kernel_choice_and_engine_setter():
    choice = nat.lib().ocr_ctc_beam_kernel_choice
    flip = bw.table_limit_classes(100)
    assert 64 < flip < 16384
    try:
        assert nat.lib().ocr_set_beam_engine(0) == 0
        assert choice(flip - 1, 100) == 1 and choice(flip, 100) == 2
        assert choice(64, 100) == 1
        assert choice(16384, 128) == 2
        assert choice(16385, 128) == 0 and choice(64, 129) == 0 and choice(1, 4) == 0
        assert ops.ctc_beam_kernel_choice(64, 100) == "table" and ops.ctc_beam_kernel_choice(4096, 100) == "wide"
        assert ops.ctc_beam_kernel_choice(16385, 128) is None
        for bad in (1, 3):
            assert nat.lib().ocr_set_beam_engine(bad) == 2
            with pytest.raises(nat.NativeError):
                ops.set_beam_engine(bad)
            assert choice(64, 100) == 1                     # a refused value changes nothing
        ops.set_beam_engine(2)
        assert choice(64, 100) == 2 and choice(16385, 128) == 0 and choice(64, 129) == 0
    finally:
        ops.set_beam_engine(0)


def test_workspace_size_accepts_a_wide_alphabet():
    """Before the wide kernel this returned OCR_STATUS_INVALID (2): 4096 classes at beam 100 need 2.4 MB of LDS in the table kernel."""
    sz = ctypes.c_size_t(0)
    assert nat.lib().ocr_ctc_beam_workspace_size(4096, 4, 16, 100, ctypes.byref(sz)) == 0
    pool = 16 * 100 + 2
    assert sz.value == ((4 * pool * 10 + 255) // 256) * 256         # the formula did not change: two ints and a short per node
    for C, K in ((16385, 128), (64, 129), (1, 4)):
        assert nat.lib().ocr_ctc_beam_workspace_size(C, 4, 16, K, ctypes.byref(sz)) == 2
