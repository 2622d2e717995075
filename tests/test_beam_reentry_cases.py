"""The pinned flat-logit cases of test_gpu_beam_reentry.py and the model of ctc_beam.hip's trie bookkeeping that chose them: everything
here runs without a GPU.  One node per prefix (canonical=True) is the oracle's dictionary search; a fresh node for every child that
enters the beam (canonical=False) is not, on every case - which is what lets the GPU test tell the two apart."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_reentry_cases as br  # noqa: E402
import beam_wide_cases as bw  # noqa: E402
from oracle import decode as odec  # noqa: E402

IDS = ["T%d-N%d-C%d-K%d-s%g-seed%d" % c for c in br.CASES]


def test_the_cases_cover_the_beam_widths_and_the_wide_alphabet():
    assert set(c[3] for c in br.CASES) >= {4, 8, 16, 32, 100}
    assert all(4 <= c[1] <= 6 for c in br.CASES)
    wide = [c for c in br.CASES if c[2] == 300 and c[3] == 8]
    assert len(wide) == 1 and min(wide[0][3] + 1, wide[0][2] - 1) == 9           # M = 9 < C - 1: the class selection prunes


@pytest.mark.parametrize("case", br.CASES, ids=IDS)
def test_committed_cases_meet_their_conditions(case):
    T, N, C, K, scale, seed = case
    acts, il, ref = br.build_case(case)
    assert acts.dtype == np.float32 and acts.shape == (T, N, C)
    assert il[0] == T and il.min() >= T // 2 and il.max() <= T and len(set(il.tolist())) > 1
    ok, why = bw.conditions(acts, il, K, False)
    assert ok, why
    assert ref[True][0] == [bw.merge_repeats(s) for s in ref[False][0]]
    assert len(br.model_mismatches(acts, il, K, ref[False])) >= br.MIN_MISMATCHES


@pytest.mark.parametrize("case", br.CASES, ids=IDS)
def test_one_node_per_prefix_is_the_oracle_and_a_fresh_node_per_child_is_not(case):
    T, N, C, K, scale, seed = case
    acts, il, ref = br.build_case(case)
    seqs, scores = ref[False]
    for restrict in ((False, True) if C > 64 else (False,)):                    # the wide kernel's class selection changes nothing
        seen = 0
        for n in range(N):
            path, score, twice = br.kernel_bookkeeping_model(acts[:il[n], n, :], K, canonical=True, restrict=restrict)
            assert path == seqs[n], (n, restrict, path, seqs[n])
            assert abs(score - scores[n]) < 1e-9, (n, restrict, score, scores[n])
            assert not twice, (n, restrict)
            path, score, twice = br.kernel_bookkeeping_model(acts[:il[n], n, :], K, canonical=False, restrict=restrict)
            seen += br.differs(path, score, seqs[n], scores[n])
        assert seen >= br.MIN_MISMATCHES, (restrict, seen)


@pytest.mark.parametrize("case", [c for c in br.CASES if c[2] <= 8], ids=[i for c, i in zip(br.CASES, IDS) if c[2] <= 8])
def test_pruned_oracle_equals_the_full_one_on_flat_logits(case):
    T, N, C, K, scale, seed = case
    acts, il, ref = br.build_case(case)
    for merge in (False, True):
        want, want_scores = odec.beam_search_tf(acts, il, beam_width=K, merge_repeated=merge)
        assert ref[merge][0] == want
        assert max(abs(a - b) for a, b in zip(ref[merge][1], want_scores)) < 1e-9
