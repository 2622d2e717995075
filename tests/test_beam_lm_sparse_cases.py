"""The reference and the committed cases of test_gpu_beam_lm_sparse.py, rescoring.BackoffNGram, automaton.SparseLabelAutomaton and what of the
sparse fused beam-search entry can be checked on the host: everything here runs without a GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_cases as bl  # noqa: E402
import beam_lm_sparse_cases as bs  # noqa: E402
import beam_nbest_cases as bn  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd.automaton import LabelAutomaton, SparseLabelAutomaton  # noqa: E402
from lstm_ctc_ocr_amd.rescoring import BackoffNGram, CharNGram  # noqa: E402

NEG = bs.NEG


# ------------------------------------------------------------------------------------------------------------------ the pinned inputs
@pytest.mark.parametrize("entry", list(bs.all_entries()), ids=lambda e: "%s-%s-%s-%d" % (e[0], "x".join(map(str, e[1])), e[2], e[3]))
def test_every_pinned_seed_still_meets_its_conditions(entry):
    ok, why, gap = bs.entry_conditions(*entry, bs.SEEDS[entry])
    print("%r: smallest gap %.2e" % (entry, gap))
    assert ok, (entry, why)


@pytest.mark.parametrize("case", bs.DENSE_CASES)
def test_the_dense_equivalence_seeds_meet_beam_lm_cases_conditions(case):
    for kind in bs.DENSE_KINDS:
        for blank in bs.blanks(case[2]):
            acts, il = bl.make_inputs(case, bs.DENSE_SEEDS[(case, kind, blank)])
            ok, why, _ = bl.conditions(case, kind, blank, acts, il)
            assert ok, (case, kind, blank, why)
            assert min(bs.default_cutoff(case[3]), case[2] - 1) == case[2] - 1          # nothing is selected away


def test_the_seed_tables_hold_exactly_the_entries():
    assert set(bs.SEEDS) == set(bs.all_entries())
    assert set(bs.DENSE_SEEDS) == {(case, kind, blank) for case in bs.DENSE_CASES for kind in bs.DENSE_KINDS for blank in bs.blanks(case[2])}
    assert bs.FAIR_CASES == [(12, 4, 40, 8, 4), (16, 4, 300, 100, 5), (8, 2, 6625, 16, 4)]
    assert min(bs.default_cutoff(8), 39) == 9 < 39                                            # the selection prunes in the first
    assert not bl.fits(300, 100)                                                              # the second is beyond the dense entry


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", bs.EXHAUSTIVE_CASES)
@pytest.mark.parametrize("kind", bs.EXHAUSTIVE_KINDS)
def test_the_reference_equals_brute_force_plus_the_automatons_score(case, kind):
    T, N, C, K, n = case
    worst = 0.0
    for blank in bs.blanks(C):
        acts, il, automaton, cutoff, (seqs, scores, lms) = bs.build_case("exhaustive", case, kind, blank)
        for i in range(N):
            exact = bs.brute_force(acts[:il[i], i, :], blank)
            accepted = {s: lp for s, lp in exact.items() if automaton.accepts(s)}
            assert len(accepted) <= K
            assert sorted(tuple(p) for p in seqs[i]) == sorted(accepted), (blank, i)
            for p, total, lm in zip(seqs[i], scores[i], lms[i]):
                assert abs(lm - automaton.score(p)) < 1e-12
                worst = max(worst, abs(total - (accepted[tuple(p)] + automaton.score(p))))
    print("%r %s: worst |total - (brute force + score)| = %.2e" % (case, kind, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("case", sorted(c for c in bn.CASES if c[2] <= 1000))
def test_the_reference_with_the_zero_automaton_is_beam_search_nbest(case):
    """The default cutoff K + 1 is beam_search_nbest's own selection."""
    T, N, C, K, n = case
    for blank in bn.blanks(C):
        acts, il, ref, scores = bn.build_case(case, blank)
        seqs, got_scores, lms = bs.beam_search_sparse(acts, il, bs.zero_automaton(C, blank), beam_width=K, blank=blank, top_paths=n)
        assert seqs == ref[False], blank
        assert max(abs(a - b) for sa, sb in zip(got_scores, scores) for a, b in zip(sa, sb)) < 1e-9
        assert all(v == 0.0 for s in lms for v in s)


def test_the_reference_steps_like_the_class_on_well_formed_automata():
    for kind, C, blank in (("bigram", 8, 0), ("trigram", 8, 4), ("trigram", 40, 39)):
        automaton = bs.make_automaton(kind, C, blank)
        st = bs.Stepper(automaton.arrays())
        for s in range(automaton.num_states):
            for c in range(C):
                if c == blank:
                    continue
                mine, theirs = st.step(s, c), automaton.step(s, c)
                assert (mine is None) == (theirs is None)
                if mine is not None:
                    assert mine[0] == float(theirs[0]) and mine[1] == theirs[1]


def test_the_fused_best_string_is_not_the_acoustic_best_at_300_classes():
    found = bs.fused_differs_from_acoustic((16, 4, 300, 100, 5))
    print(found)
    assert found


def test_a_winning_path_takes_a_backoff_hop():
    seen = 0
    for case in bs.FAIR_CASES:
        for kind in bs.FAIR_KINDS:
            for blank in bs.blanks(case[2]):
                acts, il, automaton, cutoff, (seqs, _, _) = bs.build_case("fair", case, kind, blank)
                seen += sum(1 for s in seqs if s and max(bs.hops_along(automaton, s[0]) + [0]) >= 1)
    print("%d winning paths back off" % seen)
    assert seen > 0
    acts, il, automaton, cutoff, (seqs, _, _) = bs.build_case("fair", (8, 2, 6625, 16, 4), "bigram", 0)
    hops = [h for s in seqs for p in s for h in bs.hops_along(automaton, p)]
    # 200 strings over 6624 labels: a transition out of a seen context backs off, and lands in the empty context, which holds every label
    assert sum(h >= 1 for h in hops) >= len(hops) // 3


def test_the_cutoff_changes_the_answer():
    for blank in bs.blanks(bs.CUTOFF_CASE[2]):
        acts, il, automaton, cutoff, (seqs, _, _) = bs.build_case("cutoff", bs.CUTOFF_CASE, bs.CUTOFF_KIND, blank)
        T, N, C, K, n = bs.CUTOFF_CASE
        assert cutoff == 3
        assert seqs != bs.beam_search_sparse(acts, il, automaton, beam_width=K, blank=blank, top_paths=n)[0], blank


def test_the_hostile_arrays_are_refused_by_validate_and_change_the_answer():
    T, N, C, K, n = bs.HOSTILE_CASE
    for blank in bs.blanks(C):
        acts, il, arrays, cutoff, (seqs, _, _) = bs.build_case("hostile", bs.HOSTILE_CASE, "bigram", blank)
        with pytest.raises(ValueError):
            SparseLabelAutomaton(*arrays, C, blank=blank)
        good = bs.make_automaton("bigram", C, blank)
        assert seqs != bs.beam_search_sparse(acts, il, good, beam_width=K, blank=blank, top_paths=n)[0]
        st = bs.stepper(arrays)
        H = good.num_states
        Y1, Z1 = H + 3, H + 12
        cls = [k for k in range(C) if k != blank]
        assert all(st.step(Y1, c) is None for c in cls) and all(st.step(Z1, c) is None for c in cls)          # 9 hops; a cycle
        assert any(tr is not None and tr[2] == 8 for tr in (st.step(Y1 + 1, c) for c in cls))                 # 8 hops are taken
        assert all(st.step(H, c) == st.step(H + 2, c) for c in cls)                                           # inverted and beyond A: both empty


# ------------------------------------------------------------------------------------------------------------------ BackoffNGram
def _direct(lm, ctx, sym):
    """P(sym | ctx) written out from the counts, recursively."""
    lower = _direct(lm, ctx[1:], sym) if ctx else 1.0 / lm.num_classes
    n = sum(lm.counts.get(ctx, {}).values())
    if n == 0:
        return lower
    seen = lm.counts[ctx]
    return max(seen.get(sym, 0) - lm.discount, 0.0) / n + lm.discount * len(seen) / n * lower


@pytest.mark.parametrize("order", (1, 2, 3, 4))
def test_backoff_ngram_is_a_distribution_and_its_log_prob_is_the_recursion(order):
    C = 9
    rng = np.random.RandomState(order)
    strings = [list(1 + rng.randint(0, 5, rng.randint(1, 7))) for _ in range(30)]          # labels 6 .. 8 never occur
    lm = BackoffNGram(order, C).fit(strings)
    assert lm.END == CharNGram.END and lm.BEGIN == CharNGram.BEGIN
    for history in ([], [1], [1, 2], [3, 3, 3], [8], [7, 8, 6], [1, 8], strings[0]):
        total = sum(math.exp(lm.cond_log_prob(history, s)) for s in lm.vocab)
        assert abs(total - 1.0) < 1e-12, (history, total)
    for s in strings[:5] + [[8, 7], [1, 8, 1], []]:
        padded = [lm.BEGIN] * (order - 1) + s + [lm.END]
        want = sum(math.log(_direct(lm, tuple(padded[i - order + 1:i]), padded[i])) for i in range(order - 1, len(padded)))
        assert abs(lm.log_prob(s) - want) < 1e-12
    if order > 1:                                                                           # lower-order counts are marginals
        for ctx, seen in lm.counts.items():
            if len(ctx) < order - 1:
                for sym, cnt in seen.items():
                    assert cnt == sum(v.get(sym, 0) for h, v in lm.counts.items() if len(h) == order - 1 and h[order - 1 - len(ctx):] == ctx)
    with pytest.raises(ValueError):
        BackoffNGram(0, C)
    with pytest.raises(ValueError):
        BackoffNGram(2, C, discount=1.0)
    with pytest.raises(ValueError):
        lm.log_prob([0])


# ------------------------------------------------------------------------------------------------------------------ SparseLabelAutomaton
@pytest.mark.parametrize("order, C, blank", ((1, 6, 0), (2, 9, 0), (3, 9, 8), (3, 9, 4), (4, 7, 0)))
def test_from_backoff_ngram_scores_like_the_model(order, C, blank):
    rng = np.random.RandomState(10 * order + C)
    lm = BackoffNGram(order, C).fit([list(1 + rng.randint(0, C - 3, rng.randint(1, 8))) for _ in range(40)])       # the last two labels never occur
    alpha, beta = 0.7, 0.3
    automaton = SparseLabelAutomaton.from_backoff_ngram(lm, alpha, beta, blank=blank)
    classes = [k for k in range(C) if k != blank]
    assert automaton.num_states <= 2 + sum(len(v) for v in lm.counts.values())
    root = automaton.num_states - 1 if order == 1 else int(automaton.backoff[0]) if order == 2 else None
    if root is not None:
        assert automaton.arc_begin[root + 1] - automaton.arc_begin[root] == C - 1 and automaton.backoff[root] == -1
    worst, backed = 0.0, 0
    for _ in range(300):
        labels = [int(v) for v in 1 + rng.randint(0, C - 1, rng.randint(0, 9))]
        want = alpha * lm.log_prob(labels) + beta * len(labels)
        got = automaton.score([classes[v - 1] for v in labels])
        worst = max(worst, abs(got - want) / max(1.0, abs(want)))
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (labels, got, want)
        backed += any(C - 2 <= v for v in labels)
    assert backed > 0 or order == 1
    print("order %d: worst relative |score - (alpha log_prob + beta len)| = %.2e" % (order, worst))
    with pytest.raises(ValueError):
        SparseLabelAutomaton.from_backoff_ngram(BackoffNGram(10, 5), 1.0, 0.0)                 # 9 hops


def test_to_dense_scores_exactly_and_from_dense_round_trips():
    rng = np.random.RandomState(4)
    for kind, C, blank in (("trigram", 8, 4), ("bigram", 8, 0), ("trigram", 6, 5)):
        sparse = bs.make_automaton(kind, C, blank)
        dense = sparse.to_dense()
        assert isinstance(dense, LabelAutomaton) and dense.blank == blank and dense.num_states == sparse.num_states
        for _ in range(200):
            s = [int(c) for c in rng.randint(0, C, rng.randint(0, 8)) if c != blank]
            assert dense.score(s) == sparse.score(s), s
    for order, C, blank in ((2, 8, 0), (3, 8, 7), (2, 16, 8)):
        x = bl.ngram_automaton(order, C, blank)
        back = SparseLabelAutomaton.from_dense(x)
        assert back.num_arcs == x.num_states * (C - 1) and (back.backoff == -1).all()
        y = back.to_dense()
        m = np.isfinite(x.weight)
        m[:, blank] = False
        assert (x.weight[m] == y.weight[m]).all() and (x.next[m] == y.next[m]).all() and (x.final == y.final).all()
        assert not np.isfinite(y.weight[~m]).any()
    pattern = bl.pattern_automaton(6, 0, 5, 2)
    sp = SparseLabelAutomaton.from_dense(pattern)
    for _ in range(200):
        s = [int(c) for c in rng.randint(1, 6, rng.randint(0, 7))]
        assert sp.score(s) == pattern.score(s)
    big = SparseLabelAutomaton.from_lexicon([[1] * 9] * 1, 3)
    assert big.to_dense().accepts([1] * 9)
    huge = SparseLabelAutomaton.__new__(SparseLabelAutomaton)
    huge.num_states, huge.num_classes = LabelAutomaton.MAX_STATES + 1, 3
    with pytest.raises(ValueError):
        huge.to_dense()


def test_zero_accepts_everything_with_score_zero():
    for C, blank in ((5, 0), (5, 4), (300, 150)):
        z = SparseLabelAutomaton.zero(C, blank=blank)
        assert z.num_states == 1 and z.num_arcs == C - 1
        assert z.score([]) == 0.0 and z.score([k for k in range(C) if k != blank]) == 0.0 and not z.accepts([blank])


def test_from_lexicon_accepts_exactly_its_words():
    C = 6
    rng = np.random.RandomState(2)
    for blank in (0, 5, 3):
        classes = [k for k in range(C) if k != blank]
        words = {tuple(int(v) for v in rng.choice(classes, rng.randint(0, 5))) for _ in range(25)}
        automaton = SparseLabelAutomaton.from_lexicon([list(w) for w in words] * 2, C, blank=blank)
        for L in range(6):
            for s in np.ndindex(*([len(classes)] * L)):
                s = tuple(classes[i] for i in s)
                assert automaton.accepts(s) == (s in words), (blank, s)
                assert automaton.score(s) == (0.0 if s in words else NEG)
            if L == 3:
                break
        dense = LabelAutomaton.from_lexicon([list(w) for w in sorted(words)], C, blank=blank)
        assert automaton.num_states == dense.num_states
        with pytest.raises(ValueError):
            SparseLabelAutomaton.from_lexicon([[blank]], C, blank=blank)
        with pytest.raises(ValueError):
            SparseLabelAutomaton.from_lexicon([[C]], C, blank=blank)


def test_from_lexicon_builds_100000_words_over_6625_classes():
    rng = np.random.RandomState(1)
    words = [rng.randint(1, 6625, rng.randint(1, 9)).tolist() for _ in range(100000)]
    automaton = SparseLabelAutomaton.from_lexicon(words, 6625)
    assert automaton.num_arcs == automaton.num_states - 1 and 100000 < automaton.num_states <= 1 + sum(map(len, words))
    assert sum(a.nbytes for a in automaton.arrays()) < 32 * automaton.num_states            # the dense tables would take 53 KB per state
    assert all(automaton.accepts(w) for w in words[:300])
    assert not automaton.accepts(words[0] + [1, 1, 1, 1, 1, 1, 1, 1, 1]) and not automaton.accepts([])


def _good():
    return [a.copy() for a in bs.make_automaton("trigram", 8, 0).arrays()]


def test_validate_rejects_each_malformed_array():
    C = 8
    SparseLabelAutomaton(*_good(), C)
    BEGIN, LABEL, NEXT, WEIGHT, BACKOFF, BWEIGHT, FINAL = range(7)
    H, A = len(_good()[FINAL]), len(_good()[LABEL])

    def refused(change, num_classes=C, blank=0):
        arrays = _good()
        change(arrays)
        with pytest.raises(ValueError):
            SparseLabelAutomaton(*arrays, num_classes, blank=blank)

    def put(which, index, value):
        def change(arrays):
            arrays[which][index] = value
        return change

    def replace(which, value):
        def change(arrays):
            arrays[which] = value(arrays[which])
        return change

    for which in range(7):                                                              # dtypes and shapes
        refused(replace(which, lambda a: a.astype(np.float64)))
        refused(replace(which, lambda a: a[:-1].copy()))
        refused(replace(which, lambda a: a.reshape(1, -1)))
        refused(replace(which, lambda a: a.tolist()))
    refused(put(BEGIN, 0, 1))                                                           # arc_begin: not from 0, not to A, not monotone
    refused(put(BEGIN, H, A - 1))
    first = next(s for s in range(H) if _good()[BEGIN][s + 1] - _good()[BEGIN][s] >= 2)
    lo = int(_good()[BEGIN][first])
    refused(put(BEGIN, first + 1, lo - 1 if lo else A + 1))
    refused(lambda a: a[LABEL].__setitem__(slice(lo, lo + 2), a[LABEL][lo:lo + 2][::-1].copy()))      # unsorted
    refused(put(LABEL, lo + 1, int(_good()[LABEL][lo])))                                # duplicated
    refused(put(LABEL, lo, -1))                                                         # out of range
    refused(put(LABEL, int(_good()[BEGIN][first + 1]) - 1, C))
    refused(put(LABEL, lo, 0))                                                          # the blank
    for bad in (-1, H, 1 << 30, bs.INT_MIN):
        refused(put(NEXT, lo, bad))                                                     # a finite arc that leads outside
    for which, index in ((WEIGHT, lo), (BWEIGHT, 1), (FINAL, 2)):
        refused(put(which, index, np.nan))
        refused(put(which, index, np.inf))
    refused(put(BACKOFF, 1, -2))
    refused(put(BACKOFF, 1, H))
    refused(put(BACKOFF, 1, 1))                                                         # a cycle of one
    refused(lambda a: (a[BACKOFF].__setitem__(1, 2), a[BACKOFF].__setitem__(2, 1)))     # a cycle of two
    refused(lambda a: None, num_classes=1)
    refused(lambda a: None, blank=C)
    refused(lambda a: None, blank=-1)
    # a chain of 8 hops is accepted, one of 9 is not
    for length, ok in ((8, True), (9, False)):
        n = length + 1
        arrays = (np.array([0] * n + [2], np.int32), np.array([1, 2], np.int32), np.zeros(2, np.int32), np.zeros(2, np.float32),
                  np.array([i + 1 for i in range(n - 1)] + [-1], np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32))
        if ok:
            assert SparseLabelAutomaton(*arrays, 3).step(0, 1) is not None
        else:
            with pytest.raises(ValueError):
                SparseLabelAutomaton(*arrays, 3)
    # a forbidden arc's next is never followed and may hold anything; -inf is allowed everywhere
    arrays = _good()
    arrays[WEIGHT][lo], arrays[NEXT][lo], arrays[FINAL][0], arrays[BWEIGHT][1] = NEG, 99, NEG, NEG
    ok = SparseLabelAutomaton(*arrays, C)
    assert ok.step(first, int(arrays[LABEL][lo])) is None                               # forbidden: no back-off is tried
    assert SparseLabelAutomaton(np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                np.full(1, -1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.float32), 4).accepts([])      # no arcs at all


# ------------------------------------------------------------------------------------------------------------------ the entry, on the host
def test_the_entries_are_declared_exported_and_bound():
    for name in ("ocr_ctc_beam_lm_sparse_supported", "ocr_ctc_beam_lm_sparse_workspace_size", "ocr_ctc_beam_decode_lm_sparse"):
        assert name in nat.declared_symbols()
        assert hasattr(nat.lib(), name)
    from lstm_ctc_ocr_amd import ops
    assert callable(ops.ctc_beam_lm_sparse) and callable(ops.ctc_beam_lm_sparse_supported)


def test_the_support_query_is_host_arithmetic():
    from lstm_ctc_ocr_amd import ops
    sup = ops.ctc_beam_lm_sparse_supported
    for K in (1, 2, 7, 100, 128):
        for C in (1, 2, 5, 40, 257, 6625, 16384, 16385):
            for cutoff in (0, 1, 2, K, K + 1, K + 2):
                assert sup(C, K, cutoff, 1, 0) == bs.fits(C, K, cutoff, 1, 0), (C, K, cutoff)
    assert sup(6625, 100, 101, 774, 7613) and sup(16384, 128, 129, 1 << 24, 1 << 28) and sup(2, 1, 1, 1, 0)
    assert bs.lds_bytes(16384, 128, 129) <= 160 * 1024                                     # the LDS term never binds inside the other limits
    for C, K, cutoff, H, A in ((1, 100, 101, 1, 0), (16385, 100, 101, 1, 0), (40, 0, 1, 1, 0), (40, 129, 130, 1, 0), (40, 100, 0, 1, 0),
                               (40, 100, 102, 1, 0), (40, 100, -1, 1, 0), (40, 100, 101, 0, 0), (40, 100, 101, -1, 0),
                               (40, 100, 101, (1 << 24) + 1, 0), (40, 100, 101, 1, -1), (40, 100, 101, 1, (1 << 28) + 1)):
        assert not sup(C, K, cutoff, H, A), (C, K, cutoff, H, A)
        assert not bs.fits(C, K, cutoff, H, A)
    assert sup(40, 100, 1, 1, 0) and sup(40, 100, 101, 1, 0) and sup(40, 100, 101, 1 << 24, 1 << 28)      # both ends of every range


def test_engine_takes_a_sparse_automaton_and_still_refuses_everything_else():
    from lstm_ctc_ocr_amd.engine import Engine
    eng = Engine.__new__(Engine)
    for not_an_automaton in (None, [[1, 2]], BackoffNGram(2, 5), SparseLabelAutomaton.zero(5, blank=4)):          # (the engine's blank is 0)
        with pytest.raises(ValueError):
            eng.decode_lm(None, None, not_an_automaton)
        with pytest.raises(ValueError):
            eng.decode_spans_lm(None, None, not_an_automaton)
        with pytest.raises(ValueError):
            eng.decode_nbest_beam_lm(None, None, not_an_automaton)
    assert Engine._check_lm(SparseLabelAutomaton.zero(5)).num_classes == 5
    with pytest.raises(ValueError):
        eng.decode_nbest_beam_lm(None, None, SparseLabelAutomaton.zero(5), k=0)
