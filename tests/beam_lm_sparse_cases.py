"""Inputs and the float64 reference for the wide beam search fused with a sparse back-off automaton (ctc_beam.hip,
ocr_ctc_beam_decode_lm_sparse): shared by test_beam_lm_sparse_cases.py (CPU) and test_gpu_beam_lm_sparse.py.

`beam_search_sparse` is beam_lm_cases.beam_search_lm with two changes.  (1) The per-frame class selection, which with weights in the search
is part of the specification: a NEW child P + c is a candidate only for c in S, the M = min(cutoff, C - 1) non-blank classes of largest
log-probability (beam_wide_cases.select_classes: ties to the lowest class); a child that is in the beam takes its in-beam parent's mass
whatever its class, and the repeat term never asks.  (2) `step` walks the raw sparse arrays: bisection among the arcs of the state, a miss
retries in backoff[s] after paying backoff_weight[s], at most MAX_HOPS = 8 hops, the weights summed in float32 in hop order with the arc
weight last; arc ranges are clamped to [0, A], an inverted range is empty, a next state or back-off outside [0, H) and a weight that is
not finite forbid.  It never consults SparseLabelAutomaton.step, so it also says what malformed arrays mean (the hostile case).

A case is (T, N, C, K, n), run with the blank at C - 1, 0 and C // 2, logits beam_wide_cases.make_logits (re-entry: beam_reentry_cases'
flat logits).  A seed is pinned only if the REFERENCE says the inputs make a fair test: consecutive ranks 1 .. n + 1 are at least MIN_GAP
apart on total + final, and the first n prefixes are unchanged under three N(0, 1e-4) perturbations of the logits - the perturbed searches
select their own classes, which guards the selection boundary.  The exhaustive shapes need a beam that never prunes, the re-entry case a
prefix that leaves the beam and returns, the cutoff case an answer that differs from the default cutoff's, the hostile case one that
differs from the well-formed automaton's.  At most 8 seeds are tried per entry; `python tests/beam_lm_sparse_cases.py` prints them and
test_beam_lm_sparse_cases.py checks that each pinned one still meets its conditions.

The automata are rescoring.BackoffNGram models fitted on random strings from a skewed distribution (3 * C of them; 200 at C = 6625, so
that nearly every transition backs off), compiled with SparseLabelAutomaton.from_backoff_ngram(lm, ALPHA, BETA, blank).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import beam_lm_cases as bl  # noqa: E402
import beam_nbest_cases as bn  # noqa: E402
import beam_reentry_cases as br  # noqa: E402
import beam_wide_cases as bw  # noqa: E402
from lstm_ctc_ocr_amd.automaton import SparseLabelAutomaton  # noqa: E402
from lstm_ctc_ocr_amd.rescoring import BackoffNGram  # noqa: E402

NEG = bw.NEG
_lse = bw._lse
MIN_GAP = bn.MIN_GAP
blanks = bn.blanks
brute_force = bl.brute_force
ALPHA, BETA = bl.ALPHA, bl.BETA
MAX_HOPS = 8
INT_MIN = int(np.iinfo(np.int32).min)


# ------------------------------------------------------------------------------------------------------------------ step over raw arrays
class Stepper:
    """step over the seven raw arrays (arc_begin, arc_label, arc_next, arc_weight, backoff, backoff_weight, final), memoised."""

    def __init__(self, arrays):
        self.begin, self.label, self.next = (np.asarray(a).tolist() for a in arrays[:3])
        self.weight, self.backoff, self.backoff_weight = np.asarray(arrays[3], np.float32), np.asarray(arrays[4]).tolist(), np.asarray(arrays[5], np.float32)
        self.final = np.asarray(arrays[6], np.float32)
        self.H, self.A = len(self.backoff), len(self.label)
        self.memo = {}

    def step(self, s, c):
        """(weight, next state, hops) of reading class c in state s, or None where the transition is forbidden."""
        key = (s, c)
        if key not in self.memo:
            self.memo[key] = self._step(s, c)
        return self.memo[key]

    def _step(self, s, c):
        acc, hops = np.float32(0.0), 0
        while True:
            lo = min(max(self.begin[s], 0), self.A)
            end = min(max(self.begin[s + 1], 0), self.A)
            hi = max(end, lo)
            while lo < hi:
                mid = (lo + hi) >> 1
                if self.label[mid] < c:
                    lo = mid + 1
                else:
                    hi = mid
            if lo < end and self.label[lo] == c:
                aw = self.weight[lo]
                with np.errstate(all="ignore"):
                    w = np.float32(acc + aw)
                if not (np.isfinite(aw) and np.isfinite(w) and 0 <= self.next[lo] < self.H):
                    return None
                return float(w), self.next[lo], hops
            bo, bwt = self.backoff[s], self.backoff_weight[s]
            if hops == MAX_HOPS or not 0 <= bo < self.H or not np.isfinite(bwt):
                return None
            with np.errstate(all="ignore"):
                acc = np.float32(acc + bwt)
            s = bo
            hops += 1


_steppers = {}


def stepper(automaton):
    """The memoised Stepper of a SparseLabelAutomaton or of a tuple of raw arrays (kept alive with it)."""
    key = id(automaton)
    if key not in _steppers:
        _steppers[key] = (automaton, Stepper(automaton.arrays() if isinstance(automaton, SparseLabelAutomaton) else automaton))
    return _steppers[key][1]


def default_cutoff(K):
    return K + 1


def beam_search_sparse(logits_tnc, seq_len, automaton, beam_width=100, blank=0, top_paths=1, cutoff=None, trace=None):
    """Per sample the lists of the (at most) top_paths best prefixes, of total + final and of W + final, best first.  trace: a list that
    receives per sample (the set of prefixes in the beam after each frame, whether any frame pruned)."""
    T, N, C = logits_tnc.shape
    st = stepper(automaton)
    M = min(default_cutoff(beam_width) if cutoff is None else cutoff, C - 1)
    results, scores, lms = [], [], []
    for n in range(N):
        x = np.asarray(logits_tnc[:seq_len[n], n, :], np.float64)
        m = x.max(axis=-1, keepdims=True)
        logp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
        beams = {(): (0.0, NEG)}
        info = {(): (0.0, 0)}                       # prefix -> (W, state): a function of the prefix alone
        frames, pruned = [], False
        for t in range(x.shape[0]):
            row = logp[t]
            S = bw.select_classes(row, blank, M)
            lpb = float(row[blank])
            children = {}
            for prefix in beams:
                if prefix and prefix[:-1] in beams:
                    children.setdefault(prefix[:-1], []).append(prefix[-1])
            nxt = {}

            def add(prefix, pb, pnb):
                o = nxt.get(prefix)
                nxt[prefix] = (pb, pnb) if o is None else (_lse(o[0], pb), _lse(o[1], pnb))

            for prefix, (pb, pnb) in beams.items():
                tot = _lse(pb, pnb)
                add(prefix, tot + lpb, NEG)
                last = prefix[-1] if prefix else -1
                if last >= 0:
                    add(prefix, NEG, pnb + float(row[last]))          # the repeat term pays nothing and asks no selection
                W, s = info[prefix]
                for c in sorted(set(S) | set(children.get(prefix, ()))):      # new children from S; children in the beam whatever their class
                    tr = st.step(s, c)
                    if tr is None:
                        continue
                    child = prefix + (c,)
                    if child not in info:
                        info[child] = (W + tr[0], tr[1])
                    add(child, NEG, (pb if c == last else tot) + float(row[c]) + tr[0])
            live = [(p, v) for p, v in nxt.items() if _lse(*v) != NEG]
            pruned = pruned or len(live) > beam_width
            beams = dict(sorted(live, key=lambda kv: -_lse(*kv[1]))[:beam_width])
            frames.append(set(beams))
        ranked = []
        for p, v in beams.items():
            f = float(st.final[info[p][1]])
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


def hops_along(automaton, labels):
    """The back-off hops of each transition of `labels` from the start state (the string must be accepted)."""
    st, s, out = stepper(automaton), 0, []
    for c in labels:
        w, s, hops = st.step(s, c)
        out.append(hops)
    return out


# ------------------------------------------------------------------------------------------------------------------ automata
_models, _automata = {}, {}
STRINGS_AT_6625 = 200


def fitted_backoff(order, C):
    """A BackoffNGram over C classes fitted on 3 * C (C = 6625: 200) random strings of 2 .. 8 labels drawn from a skewed distribution."""
    key = (order, C)
    if key not in _models:
        rng = np.random.RandomState(1000 * order + C)
        p = rng.dirichlet(np.full(C - 1, 0.3))
        count = STRINGS_AT_6625 if C == 6625 else 3 * C
        strings = [list(1 + rng.choice(C - 1, size=rng.randint(2, 9), p=p)) for _ in range(count)]
        _models[key] = BackoffNGram(order, C).fit(strings)
    return _models[key]


def make_automaton(kind, C, blank):
    key = (kind, C, blank)
    if key not in _automata:
        order = {"bigram": 2, "trigram": 3}[kind]
        _automata[key] = SparseLabelAutomaton.from_backoff_ngram(fitted_backoff(order, C), ALPHA, BETA, blank=blank)
    return _automata[key]


def zero_automaton(C, blank=0):
    return SparseLabelAutomaton.zero(C, blank=blank)


def lds_bytes(C, K, cutoff):
    """ctc_beam.hip: the wide kernel's LDS with M = min(cutoff, C - 1) candidate classes, and two more [2][128] beam arrays."""
    M = min(cutoff, C - 1)
    b = ((C + 3) & ~3) * 4 + (K + K * M) * 4 + M * 4 + 128 * 2 * 6 * 4 + 128 * 4
    return ((b + 15) & ~15) + 128 * 2 * 2 * 4


def fits(C, K, cutoff, H, A):
    """What ocr_ctc_beam_lm_sparse_supported must answer: host arithmetic."""
    return (2 <= C <= 16384 and 1 <= K <= 128 and 1 <= cutoff <= K + 1 and 1 <= H <= (1 << 24) and 0 <= A <= (1 << 28)
            and lds_bytes(C, K, cutoff) <= 160 * 1024)


# ------------------------------------------------------------------------------------------------------------------ cases
FAIR_CASES = [(12, 4, 40, 8, 4), (16, 4, 300, 100, 5), (8, 2, 6625, 16, 4)]
FAIR_KINDS = ("bigram", "trigram")
CUTOFF_CASE, CUTOFF, CUTOFF_KIND = (12, 4, 40, 8, 4), 3, "bigram"
EXHAUSTIVE_CASES = bl.EXHAUSTIVE_CASES                       # (4, 2, 4, 128, 128), (3, 2, 6, 128, 128)
EXHAUSTIVE_KINDS = ("bigram", "trigram")
REENTRY_CASE, REENTRY_SCALE, REENTRY_KIND = bl.REENTRY_CASE, bl.REENTRY_SCALE, "bigram"
DENSE_CASES = [(12, 4, 8, 100, 5), (20, 4, 16, 100, 4)]      # M = C - 1: nothing is selected away, so the dense entry's search is the same
DENSE_KINDS = bl.FAIR_KINDS                                  # beam_lm_cases' dense add-k automata, through from_dense
HOSTILE_CASE = (10, 4, 8, 16, 8)


def make_inputs(case, seed):
    T, N, C, K, n = case
    if case == REENTRY_CASE:
        return br.make_flat_logits(T, N, C, REENTRY_SCALE, seed)
    return bw.make_logits(T, N, C, seed)


def _gap(scores):
    return min([a - b for s in scores for a, b in zip(s, s[1:])] + [np.inf])


def _stable(acts, il, automaton, K, blank, n, cutoff, base):
    rng = np.random.RandomState(12345)
    for i in range(3):
        pert = acts.astype(np.float64) + rng.randn(*acts.shape) * 1e-4
        got, _, _ = beam_search_sparse(pert, il, automaton, beam_width=K, blank=blank, top_paths=n, cutoff=cutoff)
        if got != [s[:n] for s in base]:
            return i
    return None


def conditions(case, automaton, blank, acts, il, cutoff=None, differs_from=None):
    """(ok, what failed, smallest gap): the reference's own view of whether these inputs make a fair test.  differs_from: (automaton, cutoff)
    of a search whose first n prefixes must not all be the same as this one's."""
    T, N, C, K, n = case
    trace = []
    base, sc, _ = beam_search_sparse(acts, il, automaton, beam_width=K, blank=blank, top_paths=min(n + 1, K), cutoff=cutoff, trace=trace)
    gap = _gap(sc)
    if gap < MIN_GAP:
        return False, "a gap of %.2e between consecutive ranks" % gap, gap
    if case in EXHAUSTIVE_CASES and any(pruned for _, pruned in trace):
        return False, "a frame holds more than %d prefixes" % K, gap
    if case == REENTRY_CASE and not any(bl.reentries(frames) for frames, _ in trace):
        return False, "no prefix leaves the beam and returns", gap
    if differs_from is not None:
        other = beam_search_sparse(acts, il, differs_from[0], beam_width=K, blank=blank, top_paths=n, cutoff=differs_from[1])[0]
        if other == [s[:n] for s in base]:
            return False, "the answer is that of the search it must differ from", gap
    bad = _stable(acts, il, automaton, K, blank, n, cutoff, base)
    if bad is not None:
        return False, "the first %d prefixes change under perturbation %d" % (n, bad), gap
    return True, "", gap


# ---- malformed arrays: a back-off bigram with everything SparseLabelAutomaton.validate refuses, handed over as raw arrays
def hostile_arrays(C, blank):
    """The seven arrays of the back-off bigram automaton with: extra states whose arc_begin is inverted, reaches beyond A (one clamps to a
    range of unsorted labels, one to nothing), a back-off chain of 9 hops, a back-off cycle; arcs whose next is -1, H, 1 << 30 and INT_MIN
    under finite weights; a NaN and a +inf arc weight; two swapped labels; a NaN final.  Arcs of the start state and of the empty context
    lead into the extra states."""
    good = make_automaton("bigram", C, blank)
    begin, label, nxt, weight, backoff, bweight, final = (a.copy() for a in good.arrays())
    H, A = good.num_states, good.num_arcs
    root = int(backoff[0])                                   # the empty context (the start state backs off to it)
    assert root > 0 and begin[root + 1] - begin[root] == C - 1
    # extra states: W inverted, U = [2, A + 7) clamped, X beyond A, Y1 .. Y9 a chain into the root, Z1 <-> Z2
    W, U, X, Y1, Z1, Z2 = H, H + 1, H + 2, H + 3, H + 12, H + 13
    H2 = H + 14
    begin = np.concatenate([begin, np.array([2, A + 7] + [A + 9] * 12, np.int32)])        # begin[H] = A is W's start
    backoff = np.concatenate([backoff, np.array([root, -1, root] + [Y1 + i + 1 for i in range(8)] + [root, Z2, Z1], np.int32)])
    bweight = np.concatenate([bweight, np.full(14, -0.125, np.float32)])
    final = np.concatenate([final, np.zeros(14, np.float32)])
    r0 = int(begin[root])
    for j, target in ((3, Y1 + 1), (4, Z1), (5, X), (6, U)):                                # the root's arcs for its 4th .. 7th class
        nxt[r0 + j] = target
    s0 = int(begin[0])
    assert begin[1] - s0 >= 2
    nxt[s0], nxt[s0 + 1] = W, Y1                                                             # the start state's first two arcs
    others = [i for s in range(1, H) if s != root for i in range(int(begin[s]), int(begin[s + 1]))]
    assert len(others) >= 8
    for i, bad in zip(others[:4], (-1, H2, 1 << 30, INT_MIN)):
        nxt[i] = bad
    weight[others[4]], weight[others[5]] = np.nan, np.inf
    swap = next(s for s in range(1, H) if s != root and begin[s + 1] - begin[s] >= 2 and int(begin[s]) > others[5])
    i = int(begin[swap])
    label[i], label[i + 1] = label[i + 1], label[i]
    final[2] = np.nan
    assert len(begin) == H2 + 1 and len(backoff) == H2
    return begin, label, nxt, weight, backoff, bweight, final


_hostile = {}


def hostile(C, blank):
    if (C, blank) not in _hostile:
        _hostile[(C, blank)] = hostile_arrays(C, blank)
    return _hostile[(C, blank)]


def all_entries():
    """(tag, case, kind, blank) of every pinned entry."""
    for case in FAIR_CASES:
        for kind in FAIR_KINDS:
            for blank in blanks(case[2]):
                yield "fair", case, kind, blank
    for blank in blanks(CUTOFF_CASE[2]):
        yield "cutoff", CUTOFF_CASE, CUTOFF_KIND, blank
    for case in EXHAUSTIVE_CASES:
        for kind in EXHAUSTIVE_KINDS:
            for blank in blanks(case[2]):
                yield "exhaustive", case, kind, blank
    for blank in blanks(REENTRY_CASE[2]):
        yield "reentry", REENTRY_CASE, REENTRY_KIND, blank
    for blank in blanks(HOSTILE_CASE[2]):
        yield "hostile", HOSTILE_CASE, "bigram", blank


def entry_setup(tag, case, kind, blank):
    """(automaton or raw arrays, cutoff, differs_from) of an entry."""
    C = case[2]
    if tag == "cutoff":
        return make_automaton(kind, C, blank), CUTOFF, (make_automaton(kind, C, blank), None)
    if tag == "hostile":
        return hostile(C, blank), None, (make_automaton(kind, C, blank), None)
    return make_automaton(kind, C, blank), None, None


def entry_conditions(tag, case, kind, blank, seed):
    acts, il = make_inputs(case, seed)
    automaton, cutoff, differs = entry_setup(tag, case, kind, blank)
    return conditions(case, automaton, blank, acts, il, cutoff=cutoff, differs_from=differs)


def find_seed(tag, case, kind, blank, tries=8):
    for seed in range(tries):
        ok, _, gap = entry_conditions(tag, case, kind, blank, seed)
        if ok:
            return seed, gap
    raise RuntimeError("no seed in %d tries meets the conditions for %s %r %s, blank %d" % (tries, tag, case, kind, blank))


# (tag, case, kind, blank) -> seed, found with find_seed
SEEDS = {
    ('fair', (12, 4, 40, 8, 4), 'bigram', 39): 0,        # smallest gap 2.15e-02
    ('fair', (12, 4, 40, 8, 4), 'bigram', 0): 0,        # smallest gap 2.29e-02
    ('fair', (12, 4, 40, 8, 4), 'bigram', 20): 0,        # smallest gap 2.09e-02
    ('fair', (12, 4, 40, 8, 4), 'trigram', 39): 0,        # smallest gap 5.55e-03
    ('fair', (12, 4, 40, 8, 4), 'trigram', 0): 0,        # smallest gap 5.76e-02
    ('fair', (12, 4, 40, 8, 4), 'trigram', 20): 0,        # smallest gap 6.05e-03
    ('fair', (16, 4, 300, 100, 5), 'bigram', 299): 0,        # smallest gap 3.56e-03
    ('fair', (16, 4, 300, 100, 5), 'bigram', 0): 0,        # smallest gap 1.23e-03
    ('fair', (16, 4, 300, 100, 5), 'bigram', 150): 0,        # smallest gap 1.04e-02
    ('fair', (16, 4, 300, 100, 5), 'trigram', 299): 0,        # smallest gap 1.52e-02
    ('fair', (16, 4, 300, 100, 5), 'trigram', 0): 0,        # smallest gap 1.94e-03
    ('fair', (16, 4, 300, 100, 5), 'trigram', 150): 0,        # smallest gap 1.89e-03
    ('fair', (8, 2, 6625, 16, 4), 'bigram', 6624): 0,        # smallest gap 9.50e-03
    ('fair', (8, 2, 6625, 16, 4), 'bigram', 0): 0,        # smallest gap 1.94e-02
    ('fair', (8, 2, 6625, 16, 4), 'bigram', 3312): 0,        # smallest gap 2.54e-02
    ('fair', (8, 2, 6625, 16, 4), 'trigram', 6624): 0,        # smallest gap 3.25e-02
    ('fair', (8, 2, 6625, 16, 4), 'trigram', 0): 0,        # smallest gap 5.48e-03
    ('fair', (8, 2, 6625, 16, 4), 'trigram', 3312): 0,        # smallest gap 7.81e-02
    ('cutoff', (12, 4, 40, 8, 4), 'bigram', 39): 0,        # smallest gap 2.15e-02
    ('cutoff', (12, 4, 40, 8, 4), 'bigram', 0): 0,        # smallest gap 2.21e-02
    ('cutoff', (12, 4, 40, 8, 4), 'bigram', 20): 0,        # smallest gap 2.09e-02
    ('exhaustive', (4, 2, 4, 128, 128), 'bigram', 3): 1,        # smallest gap 1.47e-03
    ('exhaustive', (4, 2, 4, 128, 128), 'bigram', 0): 0,        # smallest gap 1.06e-03
    ('exhaustive', (4, 2, 4, 128, 128), 'bigram', 2): 1,        # smallest gap 1.88e-02
    ('exhaustive', (4, 2, 4, 128, 128), 'trigram', 3): 0,        # smallest gap 1.62e-03
    ('exhaustive', (4, 2, 4, 128, 128), 'trigram', 0): 1,        # smallest gap 5.22e-03
    ('exhaustive', (4, 2, 4, 128, 128), 'trigram', 2): 0,        # smallest gap 6.02e-03
    ('exhaustive', (3, 2, 6, 128, 128), 'bigram', 5): 0,        # smallest gap 3.33e-03
    ('exhaustive', (3, 2, 6, 128, 128), 'bigram', 0): 1,        # smallest gap 1.15e-03
    ('exhaustive', (3, 2, 6, 128, 128), 'bigram', 3): 3,        # smallest gap 1.54e-03
    ('exhaustive', (3, 2, 6, 128, 128), 'trigram', 5): 0,        # smallest gap 6.78e-03
    ('exhaustive', (3, 2, 6, 128, 128), 'trigram', 0): 0,        # smallest gap 6.97e-03
    ('exhaustive', (3, 2, 6, 128, 128), 'trigram', 3): 1,        # smallest gap 1.04e-03
    ('reentry', (24, 6, 6, 8, 4), 'bigram', 5): 0,        # smallest gap 6.54e-03
    ('reentry', (24, 6, 6, 8, 4), 'bigram', 0): 3,        # smallest gap 9.88e-03
    ('reentry', (24, 6, 6, 8, 4), 'bigram', 3): 2,        # smallest gap 1.56e-03
    ('hostile', (10, 4, 8, 16, 8), 'bigram', 7): 0,        # smallest gap 1.22e-02
    ('hostile', (10, 4, 8, 16, 8), 'bigram', 0): 0,        # smallest gap 1.86e-02
    ('hostile', (10, 4, 8, 16, 8), 'bigram', 4): 0,        # smallest gap 2.92e-02
}

# the dense-equivalence inputs are pinned by beam_lm_cases' own reference and conditions (bl.find_seed): (case, kind, blank) -> seed
DENSE_SEEDS = {
    ((12, 4, 8, 100, 5), 'bigram', 7): 0,        # smallest gap 4.24e-03
    ((12, 4, 8, 100, 5), 'bigram', 0): 0,        # smallest gap 9.30e-03
    ((12, 4, 8, 100, 5), 'bigram', 4): 0,        # smallest gap 1.37e-02
    ((12, 4, 8, 100, 5), 'trigram', 7): 0,        # smallest gap 2.24e-02
    ((12, 4, 8, 100, 5), 'trigram', 0): 0,        # smallest gap 1.24e-02
    ((12, 4, 8, 100, 5), 'trigram', 4): 0,        # smallest gap 2.54e-03
    ((20, 4, 16, 100, 4), 'bigram', 15): 0,        # smallest gap 7.39e-03
    ((20, 4, 16, 100, 4), 'bigram', 0): 0,        # smallest gap 1.02e-02
    ((20, 4, 16, 100, 4), 'bigram', 8): 0,        # smallest gap 2.69e-02
    ((20, 4, 16, 100, 4), 'trigram', 15): 0,        # smallest gap 2.05e-03
    ((20, 4, 16, 100, 4), 'trigram', 0): 0,        # smallest gap 2.84e-03
    ((20, 4, 16, 100, 4), 'trigram', 8): 0,        # smallest gap 7.21e-03
}

_cache = {}


def build_case(tag, case, kind, blank):
    """(acts, input_lengths, automaton or raw arrays, cutoff, (sequences[sample][rank], scores, lm_scores)) - computed once per process."""
    key = (tag, case, kind, blank)
    if key not in _cache:
        T, N, C, K, n = case
        acts, il = make_inputs(case, SEEDS[key])
        automaton, cutoff, _ = entry_setup(tag, case, kind, blank)
        ref = beam_search_sparse(acts, il, automaton, beam_width=K, blank=blank, top_paths=n, cutoff=cutoff)
        acts.setflags(write=False)
        il.setflags(write=False)
        _cache[key] = (acts, il, automaton, cutoff, ref)
    return _cache[key]


def build_dense_case(case, kind, blank):
    """(acts, input_lengths, the dense LabelAutomaton of beam_lm_cases, its reference's (sequences, scores, lm_scores))."""
    key = ("dense", case, kind, blank)
    if key not in _cache:
        T, N, C, K, n = case
        acts, il = bl.make_inputs(case, DENSE_SEEDS[(case, kind, blank)])
        automaton = bl.make_automaton(kind, C, blank, T)
        _cache[key] = (acts, il, automaton, bl.beam_search_lm(acts, il, automaton, beam_width=K, blank=blank, top_paths=n))
    return _cache[key]


def fused_differs_from_acoustic(case):
    """The (kind, blank, sample) of a fair case whose fused best string is not the acoustic best, by the reference alone."""
    T, N, C, K, n = case
    out = []
    for kind in FAIR_KINDS:
        for blank in blanks(C):
            acts, il, automaton, cutoff, (seqs, _, _) = build_case("fair", case, kind, blank)
            plain = beam_search_sparse(acts, il, zero_automaton(C, blank), beam_width=K, blank=blank, top_paths=1)[0]
            out += [(kind, blank, i) for i in range(N) if seqs[i][:1] != plain[i][:1]]
    return out


if __name__ == "__main__":
    import time
    for tag, case, kind, blank in all_entries():
        t0 = time.time()
        seed, gap = find_seed(tag, case, kind, blank)
        print("    (%r, %r, %r, %d): %d,        # smallest gap %.2e, %.1f s" % (tag, case, kind, blank, seed, gap, time.time() - t0), flush=True)
    for case in DENSE_CASES:
        for kind in DENSE_KINDS:
            for blank in blanks(case[2]):
                seed, gap = bl.find_seed(case, kind, blank)
                print("    (%r, %r, %d): %d,        # smallest gap %.2e" % (case, kind, blank, seed, gap), flush=True)
