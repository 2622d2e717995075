"""-m gpu: the beam search fused with a label automaton (ctc_beam.hip: ocr_ctc_beam_decode_lm, ops.ctc_beam_lm) against the float64 reference
of tests/beam_lm_cases.py with the blank at C - 1, 0 and C // 2: bit for bit against ocr_ctc_beam_decode_nbest under the zero automaton, against
brute force over all alignments plus the automaton's score at the exhaustive shapes, on pruned and on re-entering beams, under constraints
(a lexicon, a format, an automaton that accepts nothing), on malformed tables, at its edges and refusals; and Engine.decode_lm,
decode_nbest_beam_lm and decode_spans_lm on the committed trained weights and batches.

Label sequences, lengths and counts are compared exactly (the inputs are conditioned for that: beam_lm_cases.py), -neg_log_prob and lm_score
within 1e-3 * max(1, |score|) of the reference as in the other beam tests.  Every output buffer is pre-filled with a sentinel so that a slot
the kernel did not write shows.  The tests print every figure before they assert."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_cases as bl  # noqa: E402
import beam_nbest_cases as bn  # noqa: E402
import beam_wide_cases as bw  # noqa: E402
import test_gpu_beam_nbest as tn  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from lstm_ctc_ocr_amd.automaton import LabelAutomaton  # noqa: E402
from lstm_ctc_ocr_amd.rescoring import CharNGram, rerank  # noqa: E402

fx = tn.fx
tt = tn.tt
trained_engine = tn.trained_engine          # the module-scoped fixture of the n-best tests, instantiated for this module
SENTINEL = tn.SENTINEL
PAD = tn.PAD
NEG = bl.NEG
score_tol = tn.score_tol


def workspace_bytes(C, N, T, K):
    sz = ctypes.c_size_t(0)
    nat.call("ocr_ctc_beam_lm_workspace_size", C, N, T, K, ctypes.byref(sz))
    return sz.value


def fused(dev, acts, il, automaton, K, P, blank, pad=PAD):
    """ocr_ctc_beam_decode_lm into sentinel-filled buffers, the automaton a LabelAutomaton or raw (next, weight, final) tables that go to the
    entry as they are -> (paths [N, P, T], lens [N, P], nlp [N, P], lm [N, P], count [N]) as numpy."""
    T, N, C = acts.shape
    nxt, weight, final = (torch.tensor(np.ascontiguousarray(v), device=dev) for v in bl.tables(automaton))
    assert nxt.dtype == torch.int32 and weight.dtype == torch.float32 and final.dtype == torch.float32 and tuple(weight.shape) == (final.numel(), C)
    a = torch.tensor(np.array(acts), device=dev)
    l = torch.tensor(np.array(il), device=dev)
    paths = torch.full((N, P, T), SENTINEL, dtype=torch.int32, device=dev)
    lens = torch.full((N, P), SENTINEL, dtype=torch.int32, device=dev)
    nlp = torch.full((N, P), float("nan"), dtype=torch.float32, device=dev)
    lm = torch.full((N, P), float("nan"), dtype=torch.float32, device=dev)
    count = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.empty(workspace_bytes(C, N, T, K), dtype=torch.uint8, device=dev)
    nat.call("ocr_ctc_beam_decode_lm", a.data_ptr(), l.data_ptr(), C, N, T, K, P, blank, pad, nxt.data_ptr(), weight.data_ptr(), final.data_ptr(),
             final.numel(), paths.data_ptr(), lens.data_ptr(), nlp.data_ptr(), lm.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    return paths.cpu().numpy(), lens.cpu().numpy(), nlp.cpu().numpy(), lm.cpu().numpy(), count.cpu().numpy()


def check_layout(got, pad, tag):
    """What holds for every answer: counts in range (0 included), lengths in range below count, the padding, and pad / -1 / +inf / -inf at and
    beyond count."""
    paths, lens, nlp, lm, count = got
    N, P, T = paths.shape
    for n in range(N):
        assert 0 <= count[n] <= P, (tag, n, count[n])
        for r in range(P):
            if r < count[n]:
                assert 0 <= lens[n, r] <= T and np.isfinite(nlp[n, r]) and np.isfinite(lm[n, r]), (tag, n, r, lens[n, r], nlp[n, r], lm[n, r])
                assert (paths[n, r, lens[n, r]:] == pad).all(), (tag, n, r)
            else:
                assert lens[n, r] == -1 and nlp[n, r] == np.inf and lm[n, r] == -np.inf and (paths[n, r] == pad).all(), (
                    tag, n, r, lens[n, r], nlp[n, r], lm[n, r])


def strings_of(got, n):
    paths, lens, _, _, count = got
    return [paths[n, r, :lens[n, r]].tolist() for r in range(count[n])]


def check(got, ref, tag):
    """Against (sequences, scores, lm scores) of the reference."""
    seqs, scores, lms = ref
    paths, lens, nlp, lm, count = got
    check_layout(got, PAD, tag)
    worst = 0.0
    for n in range(paths.shape[0]):
        assert count[n] == len(seqs[n]), (tag, n, count[n], len(seqs[n]))
        assert strings_of(got, n) == seqs[n], (tag, n, strings_of(got, n), seqs[n])
        for r in range(count[n]):
            for mine, want in ((-float(nlp[n, r]), scores[n][r]), (float(lm[n, r]), lms[n][r])):
                worst = max(worst, abs(mine - want) / score_tol(want))
                assert abs(mine - want) < score_tol(want), (tag, n, r, mine, want)
    print("%s: worst |score - reference| / tolerance = %.3e" % (tag, worst))


# ---------------------------------------------------------------------------------------------- the zero automaton
@pytest.mark.parametrize("case", sorted(case for case in bn.CASES if bl.fits(case[2], case[3])))
def test_zero_automaton_is_the_nbest_entry_bit_for_bit(dev, case):
    """One state, weights 0, final 0: decoded, lengths, count and the bits of neg_log_prob are ocr_ctc_beam_decode_nbest(merge_repeated=0)'s on
    the table kernel, and lm_score is exactly 0."""
    T, N, C, K, n = case
    assert ops.ctc_beam_lm_supported(C, K, 1)
    ops.set_beam_engine(0)
    assert ops.ctc_beam_kernel_choice(C, K) == "table"
    for blank in bn.blanks(C):
        acts, il, ref, scores = bn.build_case(case, blank)
        want = tn.nbest(dev, acts, il, K, n, blank, False)
        got = fused(dev, acts, il, bl.zero_automaton(C), K, n, blank)
        check_layout(got, PAD, (case, blank))
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[4] == want[3]).all(), (case, blank)
        assert got[2].tobytes() == want[2].tobytes(), (case, blank)
        for i in range(N):
            assert (got[3][i, :got[4][i]] == 0.0).all(), (case, blank, i)
            assert strings_of(got, i) == ref[False][i], (case, blank, i)


def test_every_nbest_case_outside_the_fused_entrys_limit_is_refused():
    assert [case for case in sorted(bn.CASES) if not bl.fits(case[2], case[3])] == [(10, 3, bn.C_FLIP - 1, 100, 5), (10, 3, bn.C_FLIP, 100, 5)]
    assert not ops.ctc_beam_lm_supported(bn.C_FLIP - 1, 100, 1)


# ---------------------------------------------------------------------------------------------- exhaustive shapes
@pytest.mark.parametrize("kind", bl.EXHAUSTIVE_KINDS)
@pytest.mark.parametrize("case", bl.EXHAUSTIVE_CASES)
def test_exhaustive_shapes_against_brute_force(dev, case, kind):
    """The beam of 128 keeps every string the sample can emit and the automaton accepts: -neg_log_prob is the brute-force CTC log-probability
    plus automaton.score, -neg_log_prob - lm_score is minus ops.ctc_score's cost of the string, and the order is rescoring.rerank's."""
    T, N, C, K, n = case
    worst_total, worst_acoustic = 0.0, 0.0
    for blank in bl.blanks(C):
        acts, il, automaton, seqs, scores, lms = bl.build_case(case, kind, blank)
        got = fused(dev, acts, il, automaton, K, n, blank)
        tag = "%r %s blank=%d" % (case, kind, blank)
        check(got, (seqs, scores, lms), tag)
        paths, lens, nlp, lm, count = got
        a, l = torch.tensor(np.array(acts), device=dev), torch.tensor(np.array(il), device=dev)
        costs = ops.ctc_score(a, l, torch.tensor(paths, device=dev).contiguous(), torch.tensor(lens, device=dev), blank=blank, per_sample=True,
                              want_best=False)[0].cpu().numpy()
        for i in range(N):
            exact = bl.brute_force(acts[:il[i], i, :], blank)
            accepted = {s: lp for s, lp in exact.items() if automaton.accepts(s)}
            assert count[i] == len(accepted), (tag, i, count[i], len(accepted))
            for r, p in enumerate(strings_of(got, i)):
                want = accepted[tuple(p)] + automaton.score(p)
                worst_total = max(worst_total, abs(-float(nlp[i, r]) - want) / score_tol(want))
                assert abs(-float(nlp[i, r]) - want) < score_tol(want), (tag, i, r, -nlp[i, r], want)
                acoustic = -float(nlp[i, r]) - float(lm[i, r])
                worst_acoustic = max(worst_acoustic, abs(acoustic + float(costs[i, r])) / score_tol(costs[i, r]))
                assert abs(acoustic + float(costs[i, r])) < score_tol(costs[i, r]), (tag, i, r, acoustic, -costs[i, r])
            entries = [(list(s), lp) for s, lp in sorted(accepted.items())]
            assert [e[0] for e in rerank([entries], bl.ScoreLM(automaton), 1.0, 0.0)[0]] == strings_of(got, i), (tag, i)
            if kind != "pattern" and blank == 0:
                model = bl.fitted_ngram(2 if kind == "bigram" else 3, C)
                every = [(list(s), lp) for s, lp in sorted(exact.items())]
                assert [e[0] for e in rerank([every], model, bl.ALPHA, bl.BETA)[0]] == strings_of(got, i), (tag, i)
    print("%r %s: worst |-nlp - (brute force + score)| %.3e, |(-nlp - lm_score) + ctc_score cost| %.3e of the tolerance" % (
        case, kind, worst_total, worst_acoustic))


# ---------------------------------------------------------------------------------------------- pruned beams
@pytest.mark.parametrize("kind", bl.FAIR_KINDS)
@pytest.mark.parametrize("case", bl.FAIR_CASES)
def test_pruned_beams_against_the_reference(dev, case, kind):
    T, N, C, K, n = case
    for blank in bl.blanks(C):
        acts, il, automaton, seqs, scores, lms = bl.build_case(case, kind, blank)
        check(fused(dev, acts, il, automaton, K, n, blank), (seqs, scores, lms), "%r %s blank=%d" % (case, kind, blank))


def test_the_fused_best_string_is_not_the_acoustic_best(dev):
    """Where the reference says the automaton changes the answer, the fused entry returns the reference's string and the plain search another."""
    seen = 0
    for case, kind, blank, i in bl.fused_differs_from_acoustic()[:6]:
        T, N, C, K, n = case
        acts, il, automaton, seqs, _, _ = bl.build_case(case, kind, blank)
        plain = tn.nbest(dev, acts, il, K, 1, blank, False)
        got = fused(dev, acts, il, automaton, K, 1, blank)
        mine, theirs = strings_of(got, i)[:1], [plain[0][i, 0, :plain[1][i, 0]].tolist()]
        assert mine == seqs[i][:1] and mine != theirs, (case, kind, blank, i, mine, theirs, seqs[i][:1])
        seen += 1
    assert seen > 0


def test_a_prefix_that_leaves_the_beam_and_returns_keeps_its_state_and_weight(dev):
    """Flat logits, a beam of 8: by the reference a prefix drops out while an extension of it stays, and re-enters later on its old node."""
    T, N, C, K, n = bl.REENTRY_CASE
    for blank in bl.blanks(C):
        acts, il, automaton, seqs, scores, lms = bl.build_case(bl.REENTRY_CASE, bl.REENTRY_KIND, blank)
        check(fused(dev, acts, il, automaton, K, n, blank), (seqs, scores, lms), "re-entry blank=%d" % blank)


# ---------------------------------------------------------------------------------------------- constraints
def test_a_lexicon_automaton_returns_words_only(dev):
    case = bl.EXHAUSTIVE_CASES[0]
    T, N, C, K, n = case
    for blank in bl.blanks(C):
        acts, il = bl.build_case(case, "bigram", blank)[:2]
        classes = [k for k in range(C) if k != blank]
        rng = np.random.RandomState(7 + blank)
        words = sorted({tuple(int(v) for v in rng.choice(classes, rng.randint(1, T + 2))) for _ in range(12)})
        automaton = LabelAutomaton.from_lexicon([list(w) for w in words], C, blank=blank)
        got = fused(dev, acts, il, automaton, K, n, blank)
        check(got, bl.beam_search_lm(acts, il, automaton, beam_width=K, blank=blank, top_paths=n), "lexicon blank=%d" % blank)
        a, l = torch.tensor(np.array(acts), device=dev), torch.tensor(np.array(il), device=dev)
        dense = np.zeros((len(words), T + 1), np.int32)
        for k, w in enumerate(words):
            dense[k, :len(w)] = w
        costs = ops.ctc_score(a, l, torch.tensor(dense, device=dev), torch.tensor([len(w) for w in words], dtype=torch.int32, device=dev),
                              blank=blank, want_best=False)[0].cpu().numpy()
        for i in range(N):
            mine = strings_of(got, i)
            assert all(tuple(p) in words for p in mine), (blank, i, mine)
            assert len(mine) == int(np.isfinite(costs[i]).sum()) >= 1, (blank, i, mine, costs[i])       # every word the sample can emit, no other
            assert mine[0] == list(words[int(np.argmin(costs[i]))]), (blank, i, mine[0], costs[i])
            assert (got[3][i, :len(mine)] == 0.0).all()


def test_a_pattern_with_a_minimum_length_above_the_acoustic_best(dev):
    case, kind, blank = (12, 4, 8, 100, 5), "bigram", 0
    T, N, C, K, n = case
    acts, il = bl.build_case(case, kind, blank)[:2]
    plain, _, _ = bl.beam_search_lm(acts, il, bl.zero_automaton(C), beam_width=K, blank=blank, top_paths=1)
    min_len = max(len(s[0]) for s in plain) + 1
    assert min_len <= T
    automaton = LabelAutomaton.from_pattern([[k for k in range(C) if k != blank]] * T, min_len, C)
    ref = bl.beam_search_lm(acts, il, automaton, beam_width=K, blank=blank, top_paths=n)
    assert any(ref[0])
    got = fused(dev, acts, il, automaton, K, n, blank)
    check_layout(got, PAD, "pattern")
    for i in range(N):
        mine = strings_of(got, i)
        assert all(min_len <= len(p) <= T for p in mine), (i, mine)
        assert len(mine) == len(ref[0][i]) and set(map(tuple, mine)) == set(map(tuple, ref[0][i])), (i, mine, ref[0][i])
        assert mine[:1] == ref[0][i][:1], (i, mine, ref[0][i])
        for r in range(len(mine)):
            want = ref[1][i][ref[0][i].index(mine[r])]
            assert abs(-float(got[2][i, r]) - want) < score_tol(want), (i, r)


def test_an_automaton_that_accepts_nothing_returns_nothing(dev):
    case = (7, 4, 5, 2, 2)
    T, N, C, K, n = case
    acts, il = bl.build_case(case, "bigram", 0)[:2]
    none_ends = LabelAutomaton(np.zeros((1, C), np.int32), np.zeros((1, C), np.float32), np.full(1, NEG, np.float32))
    nothing_moves = LabelAutomaton(np.zeros((2, C), np.int32), np.full((2, C), NEG, np.float32), np.full(2, NEG, np.float32))
    for automaton in (none_ends, nothing_moves):
        for blank in bl.blanks(C):
            got = fused(dev, acts, il, automaton, K, n, blank)
            check_layout(got, PAD, "accepts nothing")
            assert (got[4] == 0).all()


# ---------------------------------------------------------------------------------------------- hostile tables
def test_malformed_tables_forbid_their_transitions_and_nothing_else(dev):
    """next = -1, num_states, 1 << 30 and INT_MIN under finite weights, NaN and +inf weights and end weights go to the entry as they are
    (LabelAutomaton refuses them): the kernel bounds-checks every next and reads a weight that is not finite as forbidden, so the result is the
    reference's with those transitions taken out.  The inputs are conditioned like every other case (beam_lm_cases.hostile_conditions)."""
    for case in bl.HOSTILE_CASES:
        T, N, C, K, n = case
        for blank in bl.blanks(C):
            acts, il, tabs, ref = bl.build_hostile_case(case, blank)
            with pytest.raises(ValueError):
                LabelAutomaton(*tabs, blank=blank)
            check(fused(dev, acts, il, tabs, K, n, blank), ref, "hostile %r blank=%d" % (case, blank))


# ---------------------------------------------------------------------------------------------- edges
def test_beams_shorter_than_top_paths_nan_frames_and_empty_inputs(dev):
    """C = 3: after one frame the beam holds the empty prefix and two labels, after none the empty prefix alone, whose lm_score is final[0].
    Frames beyond input_lengths are NaN: one read of them would poison the scores."""
    T, N, C, K, P = 4, 2, 3, 8, 5
    rng = np.random.RandomState(5)
    acts = np.full((T, N, C), np.nan, np.float32)
    acts[0, 0] = rng.randn(C) * 2
    il = np.array([1, 0], np.int32)
    row = acts[0, 0].astype(np.float64)
    logp = row - (row.max() + np.log(np.exp(row - row.max()).sum()))
    for blank in (2, 0, 1):
        automaton = LabelAutomaton((np.arange(2 * C, dtype=np.int32).reshape(2, C) % 2), rng.randn(2, C).astype(np.float32),
                                   np.array([-0.25, 0.5], np.float32))
        got = paths, lens, nlp, lm, count = fused(dev, acts, il, automaton, K, P, blank)
        check_layout(got, PAD, blank)
        assert count.tolist() == [3, 1], blank
        want = sorted([(-(logp[c] + automaton.score([] if c == blank else [c])), [] if c == blank else [c]) for c in range(C)])
        for r, (cost, seq) in enumerate(want):
            assert paths[0, r, :lens[0, r]].tolist() == seq, (blank, r)
            assert abs(nlp[0, r] - cost) < score_tol(cost), (blank, r, nlp[0, r], cost)
            assert abs(lm[0, r] - automaton.score(seq)) < score_tol(automaton.score(seq)), (blank, r)
        assert lens[1, 0] == 0 and nlp[1, 0] == 0.25 and lm[1, 0] == -0.25, blank


def test_refusals_return_invalid_and_write_nothing(dev):
    T, N = 6, 3
    lib = nat.lib()
    st = nat.stream()

    def attempt(C, K, P, blank, H=4, ws_bytes=None, null=None):
        acts = torch.zeros((T, N, C), dtype=torch.float32, device=dev)
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        rows = max(1, min(H, 8))
        nxt = torch.zeros((rows, C), dtype=torch.int32, device=dev)
        weight = torch.zeros((rows, C), dtype=torch.float32, device=dev)
        final = torch.zeros((rows,), dtype=torch.float32, device=dev)
        width = max(1, min(P, 160))
        out = torch.full((N, width, T), SENTINEL, dtype=torch.int32, device=dev)
        lens = torch.full((N, width), SENTINEL, dtype=torch.int32, device=dev)
        nlp = torch.full((N, width), -1.0, dtype=torch.float32, device=dev)
        lm = torch.full((N, width), -1.0, dtype=torch.float32, device=dev)
        count = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        p = dict(acts=acts.data_ptr(), il=il.data_ptr(), next=nxt.data_ptr(), weight=weight.data_ptr(), final=final.data_ptr(), out=out.data_ptr(),
                 lens=lens.data_ptr(), nlp=nlp.data_ptr(), lm=lm.data_ptr(), count=count.data_ptr(), ws=ws.data_ptr())
        if null:
            p[null] = None
        rc = lib.ocr_ctc_beam_decode_lm(p["acts"], p["il"], C, N, T, K, P, blank, 0, p["next"], p["weight"], p["final"], H, p["out"], p["lens"],
                                        p["nlp"], p["lm"], p["count"], p["ws"], ws.numel() if ws_bytes is None else ws_bytes, st)
        torch.cuda.synchronize()
        tag = (C, K, P, blank, H, ws_bytes, null, rc)
        assert rc == 2, tag
        assert (out == SENTINEL).all() and (lens == SENTINEL).all() and (nlp == -1.0).all() and (lm == -1.0).all() and (count == SENTINEL).all(), tag

    C, K = 64, 100
    assert workspace_bytes(C, N, T, K) < (1 << 20)
    attempt(C, K, 0, 0)
    attempt(C, K, K + 1, 0)
    attempt(C, 128, 129, 0)
    attempt(C, K, -1, 0)
    attempt(C, K, 5, -1)
    attempt(C, K, 5, C)
    attempt(C, K, 5, 0, H=0)
    attempt(C, K, 5, 0, H=-1)
    attempt(C, K, 5, 0, H=(1 << 20) + 1)
    attempt(C, K, 5, 0, ws_bytes=workspace_bytes(C, N, T, K) - 1)
    for null in ("acts", "il", "next", "weight", "final", "out", "lens", "nlp", "lm", "count", "ws"):
        attempt(C, K, 5, 0, null=null)
    attempt(C, 129, 5, 0)
    attempt(C, 0, 1, 0)
    attempt(1, K, 1, 0)
    attempt(bl.LM_LIMIT_AT_100, K, 5, 0)              # the first alphabet beyond the table kernel's LDS with the two extra arrays
    attempt(512, K, 5, 0)                             # the wide kernel's ground: out of scope


def test_the_size_and_support_queries(dev):
    T, N = 9, 5
    for C, K in ((5, 2), (40, 100), (bl.LM_LIMIT_AT_100 - 1, 100), (200, 128), (1000, 7)):
        assert ops.ctc_beam_lm_supported(C, K, 1) and ops.ctc_beam_lm_supported(C, K, 1 << 20)
        pool = T * K + 2
        need = (N * pool * (4 * 4 + 2) + 255) & ~255
        assert workspace_bytes(C, N, T, K) == need, (C, K)
        assert workspace_bytes(C, N, T, K) > tn.workspace_bytes(C, N, T, K)
    assert bl.LM_LIMIT_AT_100 == 257
    assert not ops.ctc_beam_lm_supported(bl.LM_LIMIT_AT_100, 100, 1) and ops.ctc_beam_kernel_choice(bl.LM_LIMIT_AT_100, 100) == "table"
    sz = ctypes.c_size_t(0)
    for args in ((bl.LM_LIMIT_AT_100, N, T, 100), (40, 0, T, 100), (40, N, 0, 100), (40, N, T, 129), (1, N, T, 10)):
        assert nat.lib().ocr_ctc_beam_lm_workspace_size(*args, ctypes.byref(sz)) == 2, args
    assert nat.lib().ocr_ctc_beam_lm_workspace_size(40, N, T, 100, None) == 2


def test_ops_wrapper(dev):
    """ops.ctc_beam_lm: shapes and dtypes, the cached device tables, a mismatched automaton, and a refusal is a NativeError."""
    case, kind, blank = (7, 4, 5, 2, 2), "trigram", 2
    T, N, C, K, n = case
    acts, il, automaton, seqs, scores, lms = bl.build_case(case, kind, blank)
    a, l = torch.tensor(np.array(acts), device=dev), torch.tensor(np.array(il), device=dev)
    paths, lens, nlp, lm, count = got = ops.ctc_beam_lm(a, l, automaton, n, beam_width=K, blank=blank, pad_value=PAD)
    assert paths.shape == (N, n, T) and paths.dtype == torch.int32 and lens.shape == (N, n) and lens.dtype == torch.int32
    assert nlp.shape == lm.shape == (N, n) and nlp.dtype == lm.dtype == torch.float32 and count.shape == (N,) and count.dtype == torch.int32
    check(tuple(v.cpu().numpy() for v in got), (seqs, scores, lms), "ops")
    first = automaton.device_arrays(a.device)
    assert all(x is y for x, y in zip(first, automaton.device_arrays(a.device)))
    assert first[0].dtype == torch.int32 and first[1].dtype == torch.float32 and first[0].is_contiguous()
    with pytest.raises(ValueError):
        ops.ctc_beam_lm(a, l, bl.zero_automaton(C + 1), n, beam_width=K, blank=blank)
    with pytest.raises(ValueError):                      # an automaton built for another blank
        ops.ctc_beam_lm(a, l, automaton, n, beam_width=K, blank=0)
    for kw in (dict(top_paths=K + 1, blank=blank), dict(top_paths=0, blank=blank), dict(top_paths=1, blank=C), dict(top_paths=1, blank=-1)):
        with pytest.raises(nat.NativeError):
            ops.ctc_beam_lm(a, l, automaton, beam_width=K, **kw)


# ---------------------------------------------------------------------------------------------- the engine on the trained fixture
def _truth(d, name):
    out, pos = [], 0
    for n in d[name + '/label_len']:
        out.append([int(v) for v in d[name + '/labels'][pos:pos + n]])
        pos += n
    return out


@pytest.mark.parametrize('name', list(tn.ac.TRAINED_BATCHES))
def test_engine_with_an_automaton_on_trained_logits(trained_engine, name):
    eng = trained_engine
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, name)
    N = x.shape[0]
    truth = _truth(d, name)
    C = int(eng.forward(x, sl).shape[2])
    # the zero automaton changes nothing
    zero = LabelAutomaton.zero(C)
    assert eng.decode_lm(x, sl, zero) == eng.decode(x, sl, method='prefix')
    assert eng.decode_spans_lm(x, sl, zero) == eng.decode_spans(x, sl, method='prefix')
    for kw in (dict(k=5), dict(k=5, rescore=False), dict(k=3, candidates=40)):
        assert eng.decode_nbest_beam_lm(x, sl, zero, **kw) == eng.decode_nbest_beam(x, sl, **kw), kw
    # a bigram fitted on the batch's labels
    bigram = LabelAutomaton.from_ngram(CharNGram(2, C).fit(truth), 0.7, 0.3)
    k = 5
    lists = eng.decode_nbest_beam_lm(x, sl, bigram, k=k)
    own = eng.decode_nbest_beam_lm(x, sl, bigram, k=k, rescore=False)
    assert len(lists) == len(own) == N
    assert [lst[0][0] for lst in own] == eng.decode_lm(x, sl, bigram)
    lexicon = sorted({tuple(e[0]) for lst in lists for e in lst})
    costs = eng.score(x, sl, [list(s) for s in lexicon])[0]
    col = {s: j for j, s in enumerate(lexicon)}
    worst_cost, worst_post = 0.0, 0.0
    for n in range(N):
        assert 1 <= len(lists[n]) <= k, (name, n)
        strings = [tuple(e[0]) for e in lists[n]]
        assert len(set(strings)) == len(strings) and all(0 not in s for s in strings), (name, n, strings)
        for lst in (lists[n], own[n]):
            assert all(lst[j][1] >= lst[j + 1][1] for j in range(len(lst) - 1)), (name, n)
            post = tn._logsumexp([e[2] for e in lst])
            worst_post = max(worst_post, abs(post))
            assert abs(post) <= 1e-5, (name, n, post)
        for labels_, log_prob, _ in lists[n]:
            want = -float(costs[n, col[tuple(labels_)]]) + bigram.score(labels_)
            worst_cost = max(worst_cost, abs(log_prob - want))
            assert abs(log_prob - want) <= tt.COST_BOUND, (name, n, labels_, log_prob, want)
    print('%s: |log_prob - (-Engine.score + automaton.score)| at most %.3e (bound %.3e); |logsumexp(log_post)| at most %.3e'
          % (name, worst_cost, tt.COST_BOUND, worst_post))
    # a lexicon of the true labels and distractors
    rng = np.random.RandomState(3)
    words = {tuple(t) for t in truth} | {tuple(int(v) for v in rng.randint(1, C, rng.randint(3, 9))) for _ in range(200)}
    lexicon_lm = LabelAutomaton.from_lexicon([list(w) for w in sorted(words)], C)
    assert () not in words
    decoded = eng.decode_lm(x, sl, lexicon_lm)
    logits = eng.forward(x, sl)
    count = ops.ctc_beam_lm(logits, eng.plan(x.shape[0], x.shape[1]).seq_len, lexicon_lm, 1, beam_width=100, blank=0)[4].cpu().numpy()
    for n in range(N):              # a string wherever the search returned one, and it is a word; [] only where count is 0 (no word left in the beam)
        assert (tuple(decoded[n]) in words) if count[n] == 1 else (count[n] == 0 and decoded[n] == []), (name, n, count[n], decoded[n])
    print('%s: %d of %d samples decode to a word of the lexicon, %d have none left in the beam' % (name, int((count == 1).sum()), N, int((count == 0).sum())))
    assert (count == 1).any(), name
    for lst in eng.decode_nbest_beam_lm(x, sl, lexicon_lm, k=k, candidates=20):
        assert all(tuple(e[0]) in words for e in lst), name
    strings, spans = eng.decode_spans_lm(x, sl, lexicon_lm)
    assert strings == decoded
    for n in range(N):
        assert [c for c, _, _, _ in spans[n]] == strings[n], (name, n)
