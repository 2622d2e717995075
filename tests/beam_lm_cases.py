"""Inputs and the float64 reference for the beam search fused with a label automaton (ctc_beam.hip, ocr_ctc_beam_decode_lm): shared by
test_beam_lm_cases.py (CPU) and test_gpu_beam_lm.py.

`beam_search_lm` is the dictionary algorithm of oracle/decode.py over ALL classes (no per-frame class selection: the fused entry runs the
table kernel only) with any class as the blank, the `top_paths` ranked prefixes of beam_nbest_cases.beam_search_nbest, and the automaton's
terms: a prefix P carries its state and W(P); extending P by c pays weight[state(P)][c] on top of the acoustic term (the repeat term
pnb + lp[c], which keeps P itself, pays nothing); a transition whose weight is not finite or whose next state lies outside [0, num_states)
is not taken; the beam is pruned by total = log p_beam + W, and the final ranking is by total + final[state], entries of -inf dropped.  It
reads the raw tables, so it also says what a malformed table means (the hostile-table test).  test_beam_lm_cases.py shows it equal to
beam_search_nbest under the zero automaton, and at the exhaustive shapes to brute force over all alignments plus automaton.score.

A case is (T, N, C, K, n) and is run with the blank at C - 1, 0 and C // 2; logits are beam_wide_cases.make_logits(T, N, C, seed) (the
re-entry case: beam_reentry_cases.make_flat_logits).  A seed is pinned only if the REFERENCE says the inputs make a fair test (no code under
test is consulted): for every sample the first n fused prefixes are the same under three N(0, 1e-4) perturbations of the logits, and
consecutive ranks 1 .. n + 1 are at least 1e-3 apart on total + final.  The exhaustive shapes also need a beam that never prunes, the
re-entry case a prefix that leaves the beam while an extension of it stays and returns later.  At most 8 seeds are tried per entry
(`find_seed`; `python tests/beam_lm_cases.py` prints them); test_beam_lm_cases.py checks that each pinned one still meets its conditions.

The n-gram automata are rescoring.CharNGram models fitted on a few random strings (so that they have strong preferences), compiled with
LabelAutomaton.from_ngram(lm, ALPHA, BETA, blank).  ALPHA and BETA were chosen so that by the reference alone the fused best string differs
from the acoustic best on some sample of some fair case (test_beam_lm_cases.py asserts it): the GPU test then cannot pass without the fusion.
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import beam_nbest_cases as bn  # noqa: E402
import beam_reentry_cases as br  # noqa: E402
import beam_wide_cases as bw  # noqa: E402
from lstm_ctc_ocr_amd.automaton import LabelAutomaton  # noqa: E402
from lstm_ctc_ocr_amd.rescoring import CharNGram  # noqa: E402

NEG = bw.NEG
_lse = bw._lse
MIN_GAP = bn.MIN_GAP
blanks = bn.blanks
ALPHA, BETA = 0.7, 0.3


def tables(automaton):
    """(next, weight, final) of a LabelAutomaton, or the tuple itself (raw tables, possibly malformed)."""
    return (automaton.next, automaton.weight, automaton.final) if isinstance(automaton, LabelAutomaton) else automaton


def step(tabs, s, c):
    """(weight, next state) of reading class c in state s; None where the transition is forbidden: a weight that is not finite or a next
    state outside the automaton."""
    nxt, weight, _ = tabs
    w, s2 = float(weight[s, c]), int(nxt[s, c])
    if not np.isfinite(w) or not 0 <= s2 < weight.shape[0]:
        return None
    return w, s2


def beam_search_lm(logits_tnc, seq_len, automaton, beam_width=100, blank=0, top_paths=1, trace=None):
    """Per sample the lists of the (at most) top_paths best prefixes, of total + final and of W + final, best first.  trace: a list that
    receives per sample (the set of prefixes in the beam after each frame, whether any frame pruned)."""
    T, N, C = logits_tnc.shape
    tabs = tables(automaton)
    final = tabs[2]
    results, scores, lms = [], [], []
    for n in range(N):
        x = np.asarray(logits_tnc[:seq_len[n], n, :], np.float64)
        m = x.max(axis=-1, keepdims=True)
        logp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
        beams = {(): (0.0, NEG)}
        info = {(): (0.0, 0)}                       # prefix -> (W, state): a function of the prefix alone
        frames, pruned = [], False
        for t in range(x.shape[0]):
            row = [float(v) for v in logp[t]]
            nxt = {}

            def add(prefix, pb, pnb):
                o = nxt.get(prefix)
                nxt[prefix] = (pb, pnb) if o is None else (_lse(o[0], pb), _lse(o[1], pnb))

            for prefix, (pb, pnb) in beams.items():
                tot = _lse(pb, pnb)
                add(prefix, tot + row[blank], NEG)
                last = prefix[-1] if prefix else -1
                W, s = info[prefix]
                for c in range(C):
                    if c == blank:
                        continue
                    if c == last:
                        add(prefix, NEG, pnb + row[c])
                    tr = step(tabs, s, c)
                    if tr is None:
                        continue
                    child = prefix + (c,)
                    if child not in info:
                        info[child] = (W + tr[0], tr[1])
                    add(child, NEG, (pb if c == last else tot) + row[c] + tr[0])
            live = [(p, v) for p, v in nxt.items() if _lse(*v) != NEG]
            pruned = pruned or len(live) > beam_width
            beams = dict(sorted(live, key=lambda kv: -_lse(*kv[1]))[:beam_width])
            frames.append(set(beams))
        ranked = []
        for p, v in beams.items():
            f = float(final[info[p][1]])
            if np.isfinite(f) and _lse(*v) != NEG:
                ranked.append((_lse(*v) + f, info[p][0] + f, p))
        ranked.sort(key=lambda e: -e[0])
        ranked = ranked[:top_paths]
        results.append([list(p) for _, _, p in ranked])
        scores.append([s for s, _, _ in ranked])
        lms.append([w for _, w, _ in ranked])
        if trace is not None:
            trace.append((frames, pruned))
    return results, scores, lms


def brute_force(logits_tc, blank):
    """{string: log-probability} over all C^T alignments of one sample's [T, C] logits (float64): the exact CTC probabilities."""
    x = np.asarray(logits_tc, np.float64)
    T, C = x.shape
    m = x.max(axis=-1, keepdims=True) if T else x
    logp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True))) if T else x
    out = {}
    for path in itertools.product(range(C), repeat=T):
        s, prev = [], -1
        for c in path:
            if c != prev and c != blank:
                s.append(c)
            prev = c
        lp = float(sum(logp[t, c] for t, c in enumerate(path)))
        key = tuple(s)
        out[key] = lp if key not in out else _lse(out[key], lp)
    return out


class ScoreLM:
    """rescoring.rerank's `lm` over any automaton: log_prob = automaton.score, to be used with alpha = 1, beta = 0."""

    def __init__(self, automaton):
        self.automaton = automaton

    def log_prob(self, labels):
        return self.automaton.score(labels)


# ------------------------------------------------------------------------------------------------------------------ automata
_automata = {}


def fitted_ngram(order, C, seed=0):
    """A CharNGram over C classes (its own convention: labels 1 .. C - 1) fitted on 3 * C random strings of 2 .. 8 labels drawn from a
    skewed distribution, so that it prefers some continuations strongly."""
    rng = np.random.RandomState(1000 * order + C + seed)
    p = rng.dirichlet(np.full(C - 1, 0.3))
    strings = [list(1 + rng.choice(C - 1, size=rng.randint(2, 9), p=p)) for _ in range(3 * C)]
    return CharNGram(order, C, add_k=0.1).fit(strings)


def ngram_automaton(order, C, blank):
    key = ("ngram", order, C, blank)
    if key not in _automata:
        _automata[key] = LabelAutomaton.from_ngram(fitted_ngram(order, C), ALPHA, BETA, blank=blank)
    return _automata[key]


def pattern_automaton(C, blank, length, min_len):
    """Even positions take the lower half of the non-blank classes, odd positions the upper half and the first class."""
    key = ("pattern", C, blank, length, min_len)
    if key not in _automata:
        cls = [k for k in range(C) if k != blank]
        half = len(cls) // 2
        allowed = [cls[:half] if i % 2 == 0 else cls[half:] + cls[:1] for i in range(length)]
        _automata[key] = LabelAutomaton.from_pattern(allowed, min_len, C, blank=blank)
    return _automata[key]


def zero_automaton(C, blank=0):
    return LabelAutomaton.zero(C, blank=blank)


def make_automaton(kind, C, blank, T):
    if kind == "bigram":
        return ngram_automaton(2, C, blank)
    if kind == "trigram":
        return ngram_automaton(3, C, blank)
    if kind == "pattern":
        return pattern_automaton(C, blank, T, 1)
    raise ValueError(kind)


def lm_lds_bytes(C, K):
    """ctc_beam.hip: the table kernel's LDS (beam_wide_cases.table_limit_classes spells it out) and two more [2][128] beam arrays."""
    b = ((C + 3) & ~3) * 4 + (K + K * C) * 4 + ((K * C + 1) & ~1) * 2 + 128 * 2 * 6 * 4 + 128 * 4
    return ((b + 15) & ~15) + 128 * 2 * 2 * 4


def fits(C, K):
    """Whether the fused entry covers C classes at beam width K: host arithmetic, what ocr_ctc_beam_lm_supported must answer."""
    return C >= 2 and 1 <= K <= 128 and lm_lds_bytes(C, K) <= 160 * 1024


LM_LIMIT_AT_100 = next(C for C in range(2, 1000) if not fits(C, 100))          # the first alphabet refused at beam 100


# ------------------------------------------------------------------------------------------------------------------ cases
FAIR_CASES = [(12, 4, 8, 100, 5), (16, 4, 40, 100, 8), (20, 4, 16, 4, 4), (7, 4, 5, 2, 2)]
FAIR_KINDS = ("bigram", "trigram")
EXHAUSTIVE_CASES = [(4, 2, 4, 128, 128), (3, 2, 6, 128, 128)]
EXHAUSTIVE_KINDS = ("bigram", "trigram", "pattern")
REENTRY_CASE = (24, 6, 6, 8, 4)              # beam_reentry_cases.make_flat_logits(T, N, C, REENTRY_SCALE, seed)
REENTRY_SCALE = 0.7
REENTRY_KIND = "bigram"


def make_inputs(case, seed):
    T, N, C, K, n = case
    if case == REENTRY_CASE:
        return br.make_flat_logits(T, N, C, REENTRY_SCALE, seed)
    return bw.make_logits(T, N, C, seed)


def reentries(frames):
    """The prefixes that are in the beam, leave it while one of their extensions stays, and are back later."""
    found = set()
    seen = set()
    for t, beam in enumerate(frames):
        for p in seen - beam:
            if p not in found and any(len(q) > len(p) and q[:len(p)] == p for q in beam) and any(p in later for later in frames[t + 1:]):
                found.add(p)
        seen |= beam
    return found


def conditions(case, kind, blank, acts, il):
    """(ok, what failed, smallest gap): the reference's own view of whether these inputs make a fair test."""
    T, N, C, K, n = case
    automaton = make_automaton(kind, C, blank, T)
    more = min(n + 1, K)
    trace = []
    base, sc, _ = beam_search_lm(acts, il, automaton, beam_width=K, blank=blank, top_paths=more, trace=trace)
    gap = min([a - b for s in sc for a, b in zip(s, s[1:])] + [np.inf])
    if gap < MIN_GAP:
        return False, "a gap of %.2e between consecutive ranks" % gap, gap
    if case in EXHAUSTIVE_CASES and any(pruned for _, pruned in trace):
        return False, "a frame holds more than %d prefixes" % K, gap
    if case == REENTRY_CASE and not any(reentries(frames) for frames, _ in trace):
        return False, "no prefix leaves the beam and returns", gap
    rng = np.random.RandomState(12345)
    for i in range(3):
        pert = acts.astype(np.float64) + rng.randn(*acts.shape) * 1e-4
        got, _, _ = beam_search_lm(pert, il, automaton, beam_width=K, blank=blank, top_paths=n)
        if got != [s[:n] for s in base]:
            return False, "the first %d prefixes change under perturbation %d" % (n, i), gap
    return True, "", gap


# ---- malformed tables: a bigram automaton with entries LabelAutomaton refuses, handed to the entry (and to the reference) as raw tables
HOSTILE_CASES = [(10, 4, 5, 16, 8), (10, 4, 8, 16, 8)]


def hostile_tables(C, blank):
    """(next, weight, final) of the bigram automaton with a next of -1, num_states, 1 << 30 and INT_MIN under finite weights, a NaN and a +inf
    weight, and a NaN and a +inf end weight."""
    good = ngram_automaton(2, C, blank)
    nxt, weight, final = good.next.copy(), good.weight.copy(), good.final.copy()
    cls = [k for k in range(C) if k != blank]
    nxt[0, cls[0]] = -1
    nxt[1, cls[1]] = weight.shape[0]
    nxt[2, cls[2]] = 1 << 30
    nxt[3, cls[0]] = np.iinfo(np.int32).min
    weight[3, cls[3]] = np.nan
    weight[0, cls[1]] = np.inf
    final[2] = np.nan
    final[3] = np.inf
    return nxt, weight, final


def hostile_conditions(case, blank, acts, il):
    """The fair-test conditions of `conditions` for the raw malformed tables, and that they change the answer of the well-formed automaton."""
    T, N, C, K, n = case
    tabs = hostile_tables(C, blank)
    base, sc, _ = beam_search_lm(acts, il, tabs, beam_width=K, blank=blank, top_paths=min(n + 1, K))
    gap = min([a - b for s in sc for a, b in zip(s, s[1:])] + [np.inf])
    if gap < MIN_GAP:
        return False, "a gap of %.2e between consecutive ranks" % gap, gap
    if [s[:n] for s in base] == beam_search_lm(acts, il, ngram_automaton(2, C, blank), beam_width=K, blank=blank, top_paths=n)[0]:
        return False, "the malformed entries change nothing", gap
    rng = np.random.RandomState(12345)
    for i in range(3):
        pert = acts.astype(np.float64) + rng.randn(*acts.shape) * 1e-4
        if beam_search_lm(pert, il, tabs, beam_width=K, blank=blank, top_paths=n)[0] != [s[:n] for s in base]:
            return False, "the first %d prefixes change under perturbation %d" % (n, i), gap
    return True, "", gap


def find_hostile_seed(case, blank, tries=8):
    for seed in range(tries):
        acts, il = bw.make_logits(case[0], case[1], case[2], seed)
        ok, _, gap = hostile_conditions(case, blank, acts, il)
        if ok:
            return seed, gap
    raise RuntimeError("no seed in %d tries meets the conditions for the malformed tables at %r, blank %d" % (tries, case, blank))


HOSTILE_SEEDS = {               # found with find_hostile_seed
    ((10, 4, 5, 16, 8), 4): 0,        # smallest gap 4.92e-03
    ((10, 4, 5, 16, 8), 0): 0,        # 3.45e-02
    ((10, 4, 5, 16, 8), 2): 0,        # 4.36e-02
    ((10, 4, 8, 16, 8), 7): 0,        # 2.01e-03
    ((10, 4, 8, 16, 8), 0): 0,        # 6.23e-03
    ((10, 4, 8, 16, 8), 4): 0,        # 4.16e-03
}


def build_hostile_case(case, blank):
    """(acts, input_lengths, raw tables, (sequences, scores, lm_scores) of the reference)."""
    key = ("hostile", case, blank)
    if key not in _cache:
        T, N, C, K, n = case
        acts, il = bw.make_logits(T, N, C, HOSTILE_SEEDS[(case, blank)])
        tabs = hostile_tables(C, blank)
        _cache[key] = (acts, il, tabs, beam_search_lm(acts, il, tabs, beam_width=K, blank=blank, top_paths=n))
    return _cache[key]


def find_seed(case, kind, blank, tries=8):
    for seed in range(tries):
        acts, il = make_inputs(case, seed)
        ok, _, gap = conditions(case, kind, blank, acts, il)
        if ok:
            return seed, gap
    raise RuntimeError("no seed in %d tries meets the conditions for %r %s, blank %d" % (tries, case, kind, blank))


def all_entries():
    for case in FAIR_CASES:
        for kind in FAIR_KINDS:
            for blank in blanks(case[2]):
                yield case, kind, blank
    for case in EXHAUSTIVE_CASES:
        for kind in EXHAUSTIVE_KINDS:
            for blank in blanks(case[2]):
                yield case, kind, blank
    for blank in blanks(REENTRY_CASE[2]):
        yield REENTRY_CASE, REENTRY_KIND, blank


# (case, kind, blank) -> seed, found with find_seed
SEEDS = {
    ((12, 4, 8, 100, 5), 'bigram', 7): 0,         # smallest gap 4.24e-03
    ((12, 4, 8, 100, 5), 'bigram', 0): 0,         # 9.30e-03
    ((12, 4, 8, 100, 5), 'bigram', 4): 0,         # 1.37e-02
    ((12, 4, 8, 100, 5), 'trigram', 7): 0,        # 2.24e-02
    ((12, 4, 8, 100, 5), 'trigram', 0): 0,        # 1.24e-02
    ((12, 4, 8, 100, 5), 'trigram', 4): 0,        # 2.54e-03
    ((16, 4, 40, 100, 8), 'bigram', 39): 0,       # 2.68e-03
    ((16, 4, 40, 100, 8), 'bigram', 0): 0,        # 1.86e-03
    ((16, 4, 40, 100, 8), 'bigram', 20): 3,       # 6.14e-03
    ((16, 4, 40, 100, 8), 'trigram', 39): 0,      # 6.28e-03
    ((16, 4, 40, 100, 8), 'trigram', 0): 0,       # 1.56e-02
    ((16, 4, 40, 100, 8), 'trigram', 20): 1,      # 3.10e-03
    ((20, 4, 16, 4, 4), 'bigram', 15): 0,         # 1.49e-02
    ((20, 4, 16, 4, 4), 'bigram', 0): 0,          # 2.01e-02
    ((20, 4, 16, 4, 4), 'bigram', 8): 0,          # 4.77e-02
    ((20, 4, 16, 4, 4), 'trigram', 15): 0,        # 4.85e-02
    ((20, 4, 16, 4, 4), 'trigram', 0): 0,         # 1.48e-01
    ((20, 4, 16, 4, 4), 'trigram', 8): 0,         # 1.98e-02
    ((7, 4, 5, 2, 2), 'bigram', 4): 0,            # 7.50e-01
    ((7, 4, 5, 2, 2), 'bigram', 0): 0,            # 5.56e-01
    ((7, 4, 5, 2, 2), 'bigram', 2): 0,            # 2.18e-02
    ((7, 4, 5, 2, 2), 'trigram', 4): 0,           # 1.03e-01
    ((7, 4, 5, 2, 2), 'trigram', 0): 0,           # 1.71e-01
    ((7, 4, 5, 2, 2), 'trigram', 2): 0,           # 2.48e-01
    ((4, 2, 4, 128, 128), 'bigram', 3): 0,        # 3.62e-03
    ((4, 2, 4, 128, 128), 'bigram', 0): 1,        # 3.28e-02
    ((4, 2, 4, 128, 128), 'bigram', 2): 3,        # 1.66e-03
    ((4, 2, 4, 128, 128), 'trigram', 3): 0,       # 3.58e-03
    ((4, 2, 4, 128, 128), 'trigram', 0): 0,       # 2.82e-03
    ((4, 2, 4, 128, 128), 'trigram', 2): 1,       # 2.49e-03
    ((4, 2, 4, 128, 128), 'pattern', 3): 0,       # 3.91e-02
    ((4, 2, 4, 128, 128), 'pattern', 0): 0,       # 1.03e-01
    ((4, 2, 4, 128, 128), 'pattern', 2): 0,       # 8.10e-02
    ((3, 2, 6, 128, 128), 'bigram', 5): 0,        # 5.99e-03
    ((3, 2, 6, 128, 128), 'bigram', 0): 0,        # 2.63e-03
    ((3, 2, 6, 128, 128), 'bigram', 3): 0,        # 5.85e-03
    ((3, 2, 6, 128, 128), 'trigram', 5): 1,       # 1.99e-03
    ((3, 2, 6, 128, 128), 'trigram', 0): 0,       # 3.16e-03
    ((3, 2, 6, 128, 128), 'trigram', 3): 2,       # 2.01e-03
    ((3, 2, 6, 128, 128), 'pattern', 5): 0,       # 3.63e-02
    ((3, 2, 6, 128, 128), 'pattern', 0): 0,       # 1.20e-02
    ((3, 2, 6, 128, 128), 'pattern', 3): 0,       # 9.77e-02
    ((24, 6, 6, 8, 4), 'bigram', 5): 1,           # 5.24e-03
    ((24, 6, 6, 8, 4), 'bigram', 0): 2,           # 7.30e-03
    ((24, 6, 6, 8, 4), 'bigram', 3): 6,           # 7.76e-03
}

_cache = {}


def build_case(case, kind, blank):
    """(acts, input_lengths, automaton, sequences[sample][rank], scores, lm_scores) - computed once per process and shared."""
    key = (case, kind, blank)
    if key not in _cache:
        T, N, C, K, n = case
        acts, il = make_inputs(case, SEEDS[key])
        automaton = make_automaton(kind, C, blank, T)
        seqs, scores, lms = beam_search_lm(acts, il, automaton, beam_width=K, blank=blank, top_paths=n)
        acts.setflags(write=False)
        il.setflags(write=False)
        _cache[key] = (acts, il, automaton, seqs, scores, lms)
    return _cache[key]


def fused_differs_from_acoustic():
    """The (case, kind, blank, sample) of the fair cases whose fused best string is not the acoustic best, by the reference alone."""
    out = []
    for case in FAIR_CASES:
        T, N, C, K, n = case
        for kind in FAIR_KINDS:
            for blank in blanks(C):
                acts, il, automaton, seqs, _, _ = build_case(case, kind, blank)
                plain, _, _ = beam_search_lm(acts, il, zero_automaton(C), beam_width=K, blank=blank, top_paths=1)
                out += [(case, kind, blank, i) for i in range(N) if seqs[i][:1] != plain[i][:1]]
    return out


if __name__ == "__main__":
    import time
    for case, kind, blank in all_entries():
        t0 = time.time()
        seed, gap = find_seed(case, kind, blank)
        print("    (%r, %r, %d): %d,        # smallest gap %.2e, %.1f s" % (case, kind, blank, seed, gap, time.time() - t0), flush=True)
    for case in HOSTILE_CASES:
        for blank in blanks(case[2]):
            seed, gap = find_hostile_seed(case, blank)
            print("    (%r, %d): %d,        # smallest gap %.2e" % (case, blank, seed, gap), flush=True)
