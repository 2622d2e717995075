"""The reference and the committed cases of test_gpu_beam_nbest.py, and what of the n-best entry can be checked on the host: everything here
runs without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_nbest_cases as bn  # noqa: E402
import beam_wide_cases as bw  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from oracle import decode as odec  # noqa: E402

# (T, N, C, K, top_paths): pruning bites (K + 1 < C - 1) on the first three; the beam holds fewer than top_paths prefixes on short samples
SMALL = [(10, 4, 24, 3, 3), (8, 3, 40, 6, 4), (6, 3, 300, 2, 2), (9, 4, 8, 30, 12), (7, 4, 5, 2, 2)]


@pytest.mark.parametrize("T,N,C,K,P", SMALL)
def test_the_reference_equals_beam_search_tf(T, N, C, K, P):
    acts, il = bw.make_logits(T, N, C, seed=T + C)
    acts[:, N - 1, :] = np.random.RandomState(C).randn(T, C).astype(np.float32)          # one flat sample: prefixes re-enter the beam
    for blank in bn.blanks(C):
        want, want_scores = bn.drop_impossible(*odec.beam_search_tf(acts, il, beam_width=K, merge_repeated=False, blank=blank, top_paths=max(P, 2)))
        want, want_scores = [s[:P] for s in want], [s[:P] for s in want_scores]
        got, got_scores = bn.beam_search_nbest(acts, il, beam_width=K, blank=blank, top_paths=P)
        assert got == want, blank
        assert all(len(a) == len(b) for a, b in zip(got_scores, want_scores))
        assert max(abs(a - b) for sa, sb in zip(got_scores, want_scores) for a, b in zip(sa, sb)) < 1e-9


def test_the_reference_reproduces_tensorflows_known_answer():
    """The vector pinned on beam_search_tf in test_oracle_ctc.py (TF's ctc_beam_search_decoder_test): beam 2, top_paths 2, blank 5."""
    logits, il = bn.tf_known_answer()
    seqs, scores = bn.beam_search_nbest(logits, il, beam_width=2, blank=5, top_paths=2)
    assert seqs[0] == bn.TF_KNOWN_PATHS and scores[0][0] > scores[0][1]
    assert odec.beam_search_tf(logits, il, beam_width=2, merge_repeated=False, top_paths=2)[0][0] == bn.TF_KNOWN_PATHS


def test_the_case_list_is_the_one_the_issue_names():
    F = bn.C_FLIP
    assert sorted(bn.CASES) == sorted([(12, 4, 8, 100, 5), (20, 4, 16, 4, 4), (16, 4, 40, 100, 8), (7, 4, 5, 2, 2), (10, 3, F, 100, 5),
                                       (10, 3, F - 1, 100, 5), (9, 3, 1000, 7, 5)])
    assert sorted(bn.SEEDS) == sorted((case, blank) for case in bn.CASES for blank in bn.blanks(case[2]))
    assert all(0 <= seed < 8 for seed in bn.SEEDS.values())
    assert ("forced", "wide") in bn.CASES[(9, 3, 1000, 7, 5)]


@pytest.mark.parametrize("case", sorted(bn.CASES))
def test_committed_cases_meet_their_conditions(case):
    T, N, C, K, n = case
    for blank in bn.blanks(C):
        acts, il, ref, scores = bn.build_case(case, blank)
        assert acts.dtype == np.float32 and acts.shape == (T, N, C) and il.min() >= 1 and il.max() == T
        ok, why, gap = bn.conditions(case, blank, acts, il)
        print("%r blank %d: smallest gap %.2e" % (case, blank, gap))
        assert ok, (blank, why)
        assert all(1 <= len(s) <= n and len(s) == len(sc) for s, sc in zip(ref[False], scores))
        assert any(len(s) == n for s in ref[False])
        assert all(np.isfinite(v) for sc in scores for v in sc)
        assert ref[True] == [[bw.merge_repeats(p) for p in s] for s in ref[False]]
        assert all(blank not in p for s in ref[False] for p in s)


def test_the_entry_is_declared_exported_and_bound():
    assert "ocr_ctc_beam_decode_nbest" in nat.declared_symbols()
    assert hasattr(nat.lib(), "ocr_ctc_beam_decode_nbest")
    from lstm_ctc_ocr_amd import ops
    assert callable(ops.ctc_beam_nbest)


def test_engine_refuses_bad_nbest_arguments_before_any_device_work():
    """The checks come first: no forward pass, no device (the engine object is not even built)."""
    from lstm_ctc_ocr_amd.engine import Engine
    for kw in (dict(k=0), dict(k=65, beam_width=100, candidates=70), dict(k=5, candidates=4), dict(k=5, candidates=101, beam_width=100),
               dict(k=5, beam_width=4)):
        with pytest.raises(ValueError):
            Engine.decode_nbest_beam(Engine.__new__(Engine), None, None, **kw)
