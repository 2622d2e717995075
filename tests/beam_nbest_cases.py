"""Inputs and the float64 reference for the n-best beam-search entry (ctc_beam.hip, ocr_ctc_beam_decode_nbest): shared by
test_beam_nbest_cases.py (CPU) and test_gpu_beam_nbest.py.

`beam_search_nbest` is `beam_wide_cases.beam_search_pruned` (the dictionary algorithm of oracle/decode.py with the per-frame class
selection that loses nothing: see that module) with two more arguments: `blank`, any class, and `top_paths`, the number of ranked
prefixes of the final beam to return.  Prefixes of probability zero are dropped: the dictionary algorithm can rank them when the beam is
not full, the kernels never keep them.  test_beam_nbest_cases.py shows it equal to oracle.decode.beam_search_tf(blank=, top_paths=) at
small shapes; the cases use it throughout because beam_search_tf takes about 15 s per search at C = 260, K = 100, T = 10.

A case is (T, N, C, K, n) and is run with the blank at C - 1, 0 and C // 2.  Its logits are beam_wide_cases.make_logits(T, N, C, seed),
and a seed is pinned only if the ORACLE says the inputs make a fair test (conditions on the inputs; no code under test is consulted).
For every sample:
  * the first n ranked prefixes, unmerged, are the same under three N(0, 1e-4) perturbations of the logits, so a float32 kernel and a
    float64 reference cannot legitimately disagree on them or on their order;
  * consecutive log-probabilities of ranks 1 .. n + 1 (as many as the beam holds) differ by at least 1e-3;
and for the case the wide kernel is forced on, some returned label is >= 256.  At most 8 seeds are tried per (case, blank)
(`find_seed`); the pinned ones are in SEEDS and test_beam_nbest_cases.py checks that each still meets the conditions.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_wide_cases as bw  # noqa: E402

NEG = bw.NEG
_lse = bw._lse
merge_repeats = bw.merge_repeats
C_FLIP = bw.C_FLIP
MIN_GAP = 1e-3


def beam_search_nbest(logits_tnc, seq_len, beam_width=100, blank=None, top_paths=1):
    """Per sample the lists of the (at most) top_paths best prefixes, unmerged, and of their log-probabilities, best first."""
    T, N, C = logits_tnc.shape
    blank = C - 1 if blank is None else blank
    M = min(beam_width + 1, C - 1)
    results, scores = [], []
    for n in range(N):
        x = np.asarray(logits_tnc[:seq_len[n], n, :], np.float64)
        m = x.max(axis=-1, keepdims=True)
        logp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
        beams = {(): (0.0, NEG)}
        for t in range(x.shape[0]):
            row = logp[t]
            S = bw.select_classes(row, blank, M)
            inS = set(S)
            lpS = [(c, float(row[c])) for c in S]
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
                more = set(children.get(prefix, ()))
                if last >= 0:
                    more.add(last)
                more -= inS
                cls = lpS + [(c, float(row[c])) for c in sorted(more)] if more else lpS
                for c, lp in cls:
                    if c == last:
                        add(prefix, NEG, pnb + lp)
                        add(prefix + (c,), NEG, pb + lp)
                    else:
                        add(prefix + (c,), NEG, tot + lp)
            beams = dict(sorted(nxt.items(), key=lambda kv: -_lse(*kv[1]))[:beam_width])
        ranked = sorted(((_lse(*v), p) for p, v in beams.items()), key=lambda sp: -sp[0])
        ranked = [(s, p) for s, p in ranked if s != NEG][:top_paths]
        results.append([list(p) for _, p in ranked])
        scores.append([s for s, _ in ranked])
    return results, scores


def drop_impossible(seqs, scores):
    """beam_search_tf's top_paths > 1 result without its -inf-scored entries."""
    keep = [[i for i, s in enumerate(sc) if s != NEG] for sc in scores]
    return [[sq[i] for i in k] for sq, k in zip(seqs, keep)], [[sc[i] for i in k] for sc, k in zip(scores, keep)]


# (T, N, C, K, n) -> the kernels test_gpu_beam_nbest.py runs the case on: ("auto", name) is the default engine, whose choice must be the
# kernel named; ("forced", "wide") sets the wide kernel.  Cases the table kernel covers by default run on both, which is where the two
# are compared with each other.
BOTH = (("auto", "table"), ("forced", "wide"))
CASES = {
    (12, 4, 8, 100, 5): BOTH,                     # the whole class set fits the beam
    (20, 4, 16, 4, 4): BOTH,                      # n = K
    (16, 4, 40, 100, 8): BOTH,                    # the product alphabet
    (7, 4, 5, 2, 2): BOTH,
    (10, 3, C_FLIP, 100, 5): (("auto", "wide"),),             # the two sides of the table / wide boundary
    (10, 3, C_FLIP - 1, 100, 5): BOTH,
    (9, 3, 1000, 7, 5): BOTH,                     # ragged C, labels >= 256 (the wide kernel forced)
}
HIGH_LABEL_CASES = {(9, 3, 1000, 7, 5)}


def blanks(C):
    return (C - 1, 0, C // 2)


# (case, blank) -> seed, found with find_seed (python tests/beam_nbest_cases.py prints them)
SEEDS = {
    ((12, 4, 8, 100, 5), 7): 0,                # smallest gap 1.11e-03
    ((12, 4, 8, 100, 5), 0): 1,                # 2.23e-02
    ((12, 4, 8, 100, 5), 4): 0,                # 9.63e-03
    ((20, 4, 16, 4, 4), 15): 0,                # 2.30e-02
    ((20, 4, 16, 4, 4), 0): 0,                 # 6.16e-03
    ((20, 4, 16, 4, 4), 8): 0,                 # 5.01e-03
    ((16, 4, 40, 100, 8), 39): 1,              # 9.51e-03
    ((16, 4, 40, 100, 8), 0): 3,               # 3.04e-03
    ((16, 4, 40, 100, 8), 20): 1,              # 4.30e-03
    ((7, 4, 5, 2, 2), 4): 0,                   # 7.18e-01
    ((7, 4, 5, 2, 2), 0): 0,                   # 4.08e-01
    ((7, 4, 5, 2, 2), 2): 0,                   # 7.67e-01
    ((10, 3, C_FLIP, 100, 5), C_FLIP - 1): 0,              # 4.23e-03
    ((10, 3, C_FLIP, 100, 5), 0): 0,                       # 4.23e-03
    ((10, 3, C_FLIP, 100, 5), C_FLIP // 2): 0,             # 4.23e-03
    ((10, 3, C_FLIP - 1, 100, 5), C_FLIP - 2): 0,          # 1.42e-02
    ((10, 3, C_FLIP - 1, 100, 5), 0): 0,                   # 1.08e-02
    ((10, 3, C_FLIP - 1, 100, 5), (C_FLIP - 1) // 2): 0,   # 1.08e-02
    ((9, 3, 1000, 7, 5), 999): 0,              # 7.15e-03
    ((9, 3, 1000, 7, 5), 0): 0,                # 7.15e-03
    ((9, 3, 1000, 7, 5), 500): 0,              # 7.15e-03
}


def conditions(case, blank, acts, il):
    """(ok, what failed, smallest gap): the oracle's own view of whether these inputs make a fair test."""
    T, N, C, K, n = case
    more = min(n + 1, K)
    base, sc = beam_search_nbest(acts, il, beam_width=K, blank=blank, top_paths=more)
    gap = min([a - b for s in sc for a, b in zip(s, s[1:])] + [np.inf])
    if gap < MIN_GAP:
        return False, "a gap of %.2e between consecutive ranks" % gap, gap
    if case in HIGH_LABEL_CASES and not any(v >= 256 for s in base for p in s[:n] for v in p):
        return False, "no returned label >= 256", gap
    rng = np.random.RandomState(12345)
    for i in range(3):
        pert = acts.astype(np.float64) + rng.randn(*acts.shape) * 1e-4
        got, _ = beam_search_nbest(pert, il, beam_width=K, blank=blank, top_paths=n)
        if got != [s[:n] for s in base]:
            return False, "the first %d prefixes change under perturbation %d" % (n, i), gap
    return True, "", gap


def find_seed(case, blank, tries=8):
    T, N, C, K, n = case
    for seed in range(tries):
        acts, il = bw.make_logits(T, N, C, seed)
        ok, _, gap = conditions(case, blank, acts, il)
        if ok:
            return seed, gap
    raise RuntimeError("no seed in %d tries meets the conditions for %r, blank %d" % (tries, case, blank))


TF_KNOWN_PATHS = [[1, 0], [0, 1, 0]]


def tf_known_answer():
    """TensorFlow's ctc_decoder_ops_test.py::testCTCDecoderBeamSearch as test_oracle_ctc.py pins it on the oracle: 6 classes (blank 5), 5 frames
    and a sixth beyond seq_len, beam_width 2, top_paths 2, merge_repeated False -> [1, 0] then [0, 1, 0].  (logits [6, 1, 6] float32, [5])"""
    prob = np.array([[0.30999, 0.309938, 0.0679938, 0.0673362, 0.0708352, 0.173908],
                     [0.215136, 0.439699, 0.0370931, 0.0393967, 0.0381581, 0.230517],
                     [0.199959, 0.489485, 0.0233221, 0.0251417, 0.0233289, 0.238763],
                     [0.279611, 0.452966, 0.0204795, 0.0209126, 0.0194803, 0.20655],
                     [0.51286, 0.288951, 0.0243026, 0.0220788, 0.0219297, 0.129878],
                     [0.155251, 0.164444, 0.173517, 0.176138, 0.169979, 0.160671]], np.float64)
    return (np.log(prob) + 2.0)[:, None, :].astype(np.float32), np.array([5], np.int32)


_cache = {}


def build_case(case, blank):
    """(acts, input_lengths, {merge_repeated: sequences[sample][rank]}, scores[sample][rank]) - computed once per process and shared."""
    key = (case, blank)
    if key not in _cache:
        T, N, C, K, n = case
        acts, il = bw.make_logits(T, N, C, SEEDS[key])
        seqs, scores = beam_search_nbest(acts, il, beam_width=K, blank=blank, top_paths=n)
        ref = {False: seqs, True: [[merge_repeats(p) for p in s] for s in seqs]}
        acts.setflags(write=False)
        il.setflags(write=False)
        _cache[key] = (acts, il, ref, scores)
    return _cache[key]


if __name__ == "__main__":
    import time
    for case in CASES:
        for blank in blanks(case[2]):
            t0 = time.time()
            seed, gap = find_seed(case, blank)
            print("    (%r, %d): %d,        # smallest gap %.2e, %.1f s" % (case, blank, seed, gap, time.time() - t0), flush=True)
