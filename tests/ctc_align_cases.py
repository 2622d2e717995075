"""Cases, float64 reference, float32 model, margins and bounds of CTC forced alignment (ctc_align.hip: ctc_align_kernel; ops.ctc_align).  A helper
module, not collected.

Reference: per (sample, candidate) the max-plus (Viterbi) recursion over ly = act - lse in float64 with the library's tie rules: of equal values
the smaller step wins (stay, then one slot, then two), and the path ends in the last slot unless the one before it is strictly better.  It gives
the path (a slot per frame), the spans (first and last frame of every character), the span scores and the path cost.  A candidate is infeasible
by tests/ctc_score_cases.py::candidate_ok; its slots hold -1 / -1 / -inf and its cost +inf, as do the slots at and beyond a feasible one's length.

Float32 model: the same code in numpy float32.  The recursion has no exp and no log, so given the lse table the device computed the model is the
kernel's arithmetic bit for bit (one subtraction rounded once per ly, float32 compares, one float32 add per step and per span frame).

margin(case, n, j): the lead in float64 of the best path over the best path that differs from it in any frame, from forward and backward max-plus
tables (the maximum of v + w over all (t, s) off the best path); +inf where no other path exists.  Where the margin exceeds 2 x PATH_BOUND a
float32 recursion must find the float64 path; the other pairs (at most a tenth of all, test_ctc_align_cases.py) are compared by score only.

Bounds, by the rule of tests/ctc_wide_cases.py: 8 x the float32 floor, i.e. the model with its own float32 lse table against the reference.  Span
scores are compared where the two paths agree.  Measured floor per case (tests/test_ctc_align_cases.py recomputes and prints it):

    case        T    N  C      K    max_label_len  feasible  close  path_cost floor  score floor   smallest margin
    lane31       72  2     40    5   31              10        2    6.494e-05        1.276e-05     3.244e-03
    lane32       72  2     40    5   32              10        1    1.247e-04        5.623e-06     5.348e-03
    lane63      140  2     40    4   63               8        3    2.645e-04        1.134e-04     8.726e-04
    lane64      140  2     40    4   64               8        1    1.486e-04        3.828e-05     7.926e-03
    lane127     264  2     40    3  127               6        2    4.352e-04        1.470e-04     5.976e-03
    lane128     264  2     40    3  128               6        2    5.600e-04        2.544e-06     3.622e-03
    L255        520  1     24    3  255               3        1    9.398e-04        1.035e-04     9.007e-04
    repeats       8  5      6    8    6              21        0    1.323e-06        5.271e-07     1.662e-01
    brute         5  3      4   40    3              87        4    1.075e-06        8.085e-07     6.108e-03
    brute_last    5  3      4   40    3              87        0    9.821e-07        3.314e-07     4.296e-02
    K3           10  3     12    3    4               9        1    2.436e-06        1.172e-06     7.519e-03
    K4           10  3     12    4    4              12        0    1.382e-06        1.054e-06     1.458e-01
    K5           10  3     12    5    4              15        0    2.721e-06        3.779e-07     2.035e-02
    K257         10  3     12  257    4             771       33    5.180e-06        2.219e-06     7.805e-03
    C37           6  2     37    5    3              10        1    2.344e-06        5.940e-07     1.550e-02
    C1024         6  2   1024    5    3              10        0    3.451e-06        2.461e-06     8.104e-02
    C1028         6  2   1028    5    3              10        1    4.765e-06        8.680e-07     1.355e-02
    C16384        6  2  16384    5    3              10        0    3.433e-06        1.166e-06     6.332e-02
    bad          10  3     12    9    3               6        0    2.900e-06        9.104e-07     5.144e-02
    saturated    10  3     12    8    4              24        0    1.102e-05        1.368e-06     9.505e-02
    flat         12  2      6    3    3               6        4    2.609e-07        9.747e-08     0 (4 pairs tie), else one path
    tight        31  3     40    3   31               6        0    1.310e-05        4.576e-06     8.531e-02
    planted      70  1     40    1   20               1        0    3.238e-07        8.498e-07     5.414e+00
    T1            1  2      6    3    2               4        0    3.777e-07        3.777e-07     one path each
    T64          64  2     12    3    5               6        1    3.107e-05        2.091e-05     1.569e-02
    T65          65  2     12    3    5               6        0    3.063e-05        3.828e-05     1.946e-02
    T128        128  2     12    3    5               6        0    8.575e-05        1.755e-05     5.263e-02
    T129        129  2     12    3    5               6        0    1.882e-04        3.036e-05     1.720e-02
    ends         10  2     12    2    3               4        0    2.580e-06        2.007e-06     2.854e-01
    short        20  4     12    4    9              11        0    5.716e-06        1.492e-06     4.097e-02

(feasible = pairs a sample can emit; close = those whose margin is at or below 2 x PATH_BOUND = 1.50e-2: 55 of 1179, 4.7 %)

                                   float32 floor          bound (8 x)
    path_cost, absolute            9.40e-4 (L255)         7.52e-3
    span score, absolute           1.47e-4 (lane127)      1.18e-3

The path cost's floor grows with T as the scorer's does: at T = 520 the running maximum reaches -2400, where a float32 has an ulp of 2.4e-4.  A
span score is a float32 sum over the span's frames: a few ulps of a value near 10 for the usual handful of frames, 1.5e-4 where one character of a
short candidate holds most of 264 frames (lane127: a sum near -800).  The device's own figures are in tests/test_gpu_ctc_align.py's docstring."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_score_cases as sc  # noqa: E402

lc = sc.lc
_lse = sc._lse
ScoreCase = sc.ScoreCase
candidate_ok = sc.candidate_ok

PATH_FLOOR = 9.40e-04     # L255: T = 520, path costs up to 2400
SCORE_FLOOR = 1.47e-04    # lane127: one character over most of 264 frames, a sum near -800
PATH_BOUND = 8 * PATH_FLOOR
SCORE_BOUND = 8 * SCORE_FLOOR

# ---------------------------------------------------------------- the library's host arithmetic, restated (ocr_ctc_align_supported / _workspace_size)
BLOCK_FRAMES = 64         # back-pointer words stay in LDS up to here; beyond, 64 words of 16 bits per (sample, candidate, frame) in the workspace
supported = sc.supported


def workspace_bytes(C, T, N, K, max_label_len):
    if N <= 0 or N > 65535 or not supported(C, T, max_label_len, K) or N * T > 0x7fffffff:
        return None
    bp = N * K * T * 128 if T > BLOCK_FRAMES else 0
    if bp > 1 << 40:
        return None
    return (N * T * 4 + 255) // 256 * 256 + (bp + 255) // 256 * 256


# ---------------------------------------------------------------- reference and float32 model
def extended(label, blank):
    """The extended label [b, l1, b, ..., lL, b] and, per slot, whether the step over the blank before it is allowed."""
    ext = np.full(2 * len(label) + 1, blank, np.int64)
    ext[1::2] = label
    skip = np.zeros(len(ext), bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return ext, skip


def viterbi(lyx, skip):
    """Best path through lyx [Tn, S] (log-probabilities of the extended label's slots, any float dtype): -> (path [Tn] of slots, end value)."""
    dtype = lyx.dtype.type
    NEG = dtype(-np.inf)
    Tn, S = lyx.shape
    v = np.full(S, NEG, dtype)
    v[:2] = lyx[0, :2]
    bp = np.zeros((Tn, S), np.int8)
    for t in range(1, Tn):
        x1 = np.full(S, NEG, dtype); x1[1:] = v[:-1]
        x2 = np.full(S, NEG, dtype); x2[2:] = np.where(skip[2:], v[:-2], NEG)
        best, step = v.copy(), np.zeros(S, np.int8)
        m = x1 > best                     # strictly greater: ties prefer staying, then one slot, then two
        best[m] = x1[m]; step[m] = 1
        m = x2 > best
        best[m] = x2[m]; step[m] = 2
        v = (best + lyx[t]).astype(dtype)
        bp[t] = step
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        s = S - 2
    end = v[s]
    path = np.empty(Tn, np.int64)
    for t in range(Tn - 1, -1, -1):
        path[t] = s
        if t > 0:
            s -= int(bp[t, s])
    return path, end


def spans_of(path, L):
    """start [L], end [L] of a path of slots (-1 for a character the path never visits: not a valid path)."""
    start, end = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    for j in range(L):
        f = np.nonzero(path == 2 * j + 1)[0]
        if len(f):
            start[j], end[j] = f[0], f[-1]
    return start, end


def path_of(start, end, L, Tn):
    """The slot per frame of a valid span set: the blank slots fill the frames between the characters."""
    path = np.empty(Tn, np.int64)
    path[:] = 2 * L
    pos = 0
    for j in range(L):
        path[pos:start[j]] = 2 * j
        path[start[j]:end[j] + 1] = 2 * j + 1
        pos = end[j] + 1
    path[pos:] = 2 * L
    return path


def span_scores(lyx, start, end):
    """Per character the sum of its slot's lyx over its frames, added in ascending t in lyx's dtype."""
    dtype = lyx.dtype.type
    out = np.empty(len(start), lyx.dtype)
    for j in range(len(start)):
        acc = dtype(0)
        for t in range(start[j], end[j] + 1):
            acc = dtype(acc + lyx[t, 2 * j + 1])
        out[j] = acc
    return out


def slot_logprobs(k, n, j, dtype, lse=None):
    """lyx [Tn, S] of (sample n, candidate j) in `dtype`: act - lse rounded once; lse [T, N] is computed in `dtype` unless given."""
    Tn = min(int(k.il[n]), k.T)
    label = k.lexicon[j][:int(k.lens[j])]
    ext, skip = extended(label, k.blank)
    rows = k.acts[:Tn, n].astype(dtype)
    col = _lse(rows, 1) if lse is None else np.asarray(lse)[:Tn, n].astype(dtype)
    return (rows[:, ext] - col[:, None]).astype(dtype), skip


def feasible(k, n, j):
    return candidate_ok(k.lexicon[j], int(k.lens[j]), k.mll, k.C, k.blank, min(int(k.il[n]), k.T))


class Aligned(object):
    """start, end [N, K, mll] int32; score [N, K, mll]; cost [N, K]; paths {(n, j): slots per frame} of the feasible pairs."""

    def __init__(self, k, dtype):
        self.start = np.full((k.N, k.K, k.mll), -1, np.int32)
        self.end = np.full((k.N, k.K, k.mll), -1, np.int32)
        self.score = np.full((k.N, k.K, k.mll), -np.inf, dtype)
        self.cost = np.full((k.N, k.K), np.inf, dtype)
        self.paths = {}


def align_model(k, dtype, lse=None):
    """The alignment of every (sample, candidate) of case k with the recursion in `dtype`; lse: the [T, N] table to take the row log-sum-exp
    from (the device's own, for the bit-for-bit comparison) instead of computing it."""
    out = Aligned(k, dtype)
    for n in range(k.N):
        for j in range(k.K):
            if not feasible(k, n, j):
                continue
            L = int(k.lens[j])
            lyx, skip = slot_logprobs(k, n, j, dtype, lse)
            path, end = viterbi(lyx, skip)
            st, en = spans_of(path, L)
            out.paths[(n, j)] = path
            out.start[n, j, :L], out.end[n, j, :L] = st, en
            out.score[n, j, :L] = span_scores(lyx, st, en)
            out.cost[n, j] = -end
    return out


def margin_of(lyx, skip, path):
    """The lead of `path`, the best one through lyx [Tn, S] (float64), over the best path that differs from it in any frame (+inf: there is
    none): the maximum of v + w over all (t, s) off the path, v and w the forward and backward max-plus tables."""
    Tn, S = lyx.shape
    NEG = -np.inf
    v = np.full((Tn, S), NEG)
    v[0, :2] = lyx[0, :2]
    for t in range(1, Tn):
        p = v[t - 1]
        x1 = np.full(S, NEG); x1[1:] = p[:-1]
        x2 = np.full(S, NEG); x2[2:] = np.where(skip[2:], p[:-2], NEG)
        v[t] = np.maximum(np.maximum(p, x1), x2) + lyx[t]
    w = np.full((Tn, S), NEG)             # the best continuation after (t, s), its own frame not counted
    w[Tn - 1, max(S - 2, 0):] = 0.0
    for t in range(Tn - 2, -1, -1):
        q = w[t + 1] + lyx[t + 1]
        y1 = np.full(S, NEG); y1[:-1] = q[1:]
        y2 = np.full(S, NEG); y2[:-2] = np.where(skip[2:], q[2:], NEG)
        w[t] = np.maximum(np.maximum(q, y1), y2)
    through = v + w
    best = through[0, path[0]]
    through[np.arange(Tn), path] = NEG
    other = through.max()
    return np.inf if other == NEG else float(best - other)


def margin(k, n, j):
    """margin_of for (sample n, candidate j) of a case, against the reference's path."""
    lyx, skip = slot_logprobs(k, n, j, np.float64)
    return margin_of(lyx, skip, reference(k).paths[(n, j)])


def align_rows(rows, label, blank, dtype, col=None):
    """One sample's logits rows [Tn, C] against one label in `dtype` (col: the rows' log-sum-exp, computed unless given)
    -> (path, start, end, span scores, path cost, lyx, skip)."""
    rows = np.asarray(rows).astype(dtype)
    ext, skip = extended(label, blank)
    col = _lse(rows, 1) if col is None else np.asarray(col).astype(dtype)
    lyx = (rows[:, ext] - col[:, None]).astype(dtype)
    path, end_value = viterbi(lyx, skip)
    st, en = spans_of(path, len(label))
    return path, st, en, span_scores(lyx, st, en), -end_value, lyx, skip


def valid_alignment(label, start, end, Tn):
    """Every character has at least one frame, the spans are ordered and disjoint, a blank frame separates equal neighbours, and all of it lies
    inside [0, Tn)."""
    L = len(label)
    if len(start) != L or len(end) != L:
        return False
    for j in range(L):
        if not (0 <= start[j] <= end[j] < Tn):
            return False
        if j + 1 < L:
            if not end[j] < start[j + 1]:
                return False
            if label[j] == label[j + 1] and not end[j] + 1 < start[j + 1]:
                return False
    return True


def left_packed(label):
    """The alignment the tie rules pick when every path ties: one frame per character from frame 0, one blank between equal neighbours."""
    start, t = [], 0
    for j, c in enumerate(label):
        if j and c == label[j - 1]:
            t += 1
        start.append(t)
        t += 1
    return np.array(start, np.int32), np.array(start, np.int32)


# ---------------------------------------------------------------- cases
FROM_SCORE = ('lane31', 'lane32', 'lane63', 'lane64', 'lane127', 'lane128', 'L255', 'repeats', 'brute', 'brute_last', 'K3', 'K4', 'K5', 'K257',
              'C37', 'C1024', 'C1028', 'C16384', 'bad', 'saturated')


class AlignCase(ScoreCase):
    """A ScoreCase whose logits `shape(acts, case)` rewrites before they are frozen (acts: a writable copy, rewritten in place)."""

    def __init__(self, name, seed, T, C, in_lens, lexicon, shape=None, **kw):
        ScoreCase.__init__(self, name, seed, T, C, in_lens, lexicon, **kw)
        acts = self.acts.copy()
        if shape is not None:
            shape(acts, self)
        acts.setflags(write=False)
        self.acts = acts


def planted_alignment(rng, L, T):
    """Spans of 1 to 6 frames and gaps of 0 to 4 blanks (before the first character, between characters, after the last), both extremes present,
    that fill T frames exactly -> (start [L], end [L])."""
    while True:
        spans = rng.randint(1, 7, L)
        gaps = rng.randint(0, 5, L)
        tail = T - int(spans.sum() + gaps.sum())
        if 0 <= tail <= 4 and {1, 6} <= set(spans.tolist()) and {0, 4} <= set(gaps.tolist()):
            break
    start = np.cumsum(gaps) + np.concatenate([[0], np.cumsum(spans)[:-1]])
    return start.astype(np.int32), (start + spans - 1).astype(np.int32)


PLANTED = {}            # name -> (sample, candidate, start, end)
TIGHT_PAIRS = ((0, 0), (1, 1), (2, 2))          # (sample, candidate) of 'tight' with L + repeats == Tn
ENDS = {}               # sample -> the slot from the end (1 or 2) its best path of 'ends' finishes in


def build_cases():
    c = [sc.case(name) for name in FROM_SCORE]
    AC = AlignCase

    # every logit of sample 0 equal; sample 1 constant per frame, different between frames: every alignment ties exactly
    def flat(acts, k):
        acts[:, 0, :] = 0.5
        acts[:, 1, :] = acts[:, 1, :1]
    c.append(AC('flat', 501, 12, 6, [12, 12], [[1, 2, 3], [1, 1], []], shape=flat, mll=3))
    # L + repeats == Tn: one alignment exists ([1,2,3] at Tn = 3, [1,1,2] at Tn = 4, 31 characters at Tn = 31)
    c.append(AC('tight', 502, 31, 40, [3, 4, 31], [[1, 2, 3], [1, 1, 2], 31], mll=31))

    # +8 along a chosen alignment of 20 characters in 70 frames (noise of spread 1 here: a boundary moved by a frame loses 8 +- 1.4)
    def planted(acts, k):
        rng = np.random.RandomState(k.seed + 1)
        acts[:] = (rng.randn(*acts.shape)).astype(np.float32)
        st, en = planted_alignment(rng, 20, 70)
        PLANTED[k.name] = (0, 0, st, en)
        path = path_of(st, en, 20, 70)
        ext = extended(k.lexicon[0], k.blank)[0]
        for t in range(70):
            acts[t, 0, ext[path[t]]] += 8.0
    c.append(AC('planted', 503, 70, 40, [70], [20], shape=planted, mll=20))
    # one frame: the empty string, one character, two characters (infeasible)
    c.append(AC('T1', 504, 1, 6, [1, 1], [[], [3], [3, 4]], mll=2))
    # the edges of a 64-frame back-trace block; the second sample one frame shorter (T65: one sample in LDS throughout, one through the workspace)
    for i, T in enumerate((64, 65, 128, 129)):
        c.append(AC('T%d' % T, 505 + i, T, 12, [T, T - 1], [5, 5, 2], mll=5))

    # the last frame decides the final slot: the last character raised there in sample 0 (the path ends in slot S - 2), the blank in sample 1
    def ends(acts, k):
        acts[-1, 0, k.lexicon[0][-1]] += 8.0
        acts[-1, 1, k.blank] += 8.0
        ENDS[0], ENDS[1] = 2, 1
    c.append(AC('ends', 510, 10, 12, [10, 10], [3, 1], shape=ends, mll=3))

    # input lengths of 0 and below T: the frames a sample does not own hold NaN and must never be read
    def short(acts, k):
        for n, tn in enumerate(k.il):
            acts[max(int(tn), 0):, n, :] = np.nan
    c.append(AC('short', 511, 20, 12, [20, 13, 0, 7], [4, [2, 2, 5], [], 9], shape=short, mll=9))
    return c


PER_SAMPLE_CASES = ('K5', 'K257', 'bad', 'T65')

_CASES = None
_REF = {}
_MARGIN = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def case(name):
    return [k for k in cases() if k.name == name][0]


def reference(k):
    """The float64 alignment of a case: computed once per process, shared and left unchanged by every test."""
    if k.name not in _REF:
        out = align_model(k, np.float64)
        for v in (out.start, out.end, out.score, out.cost):
            v.setflags(write=False)
        _REF[k.name] = out
    return _REF[k.name]


def margins(k):
    """{(n, j): margin} over the feasible pairs of a case, computed once."""
    if k.name not in _MARGIN:
        _MARGIN[k.name] = {p: margin(k, *p) for p in sorted(reference(k).paths)}
    return _MARGIN[k.name]


def floors(k):
    """(path_cost floor, span score floor, pairs whose float32 path is the float64 one) of a case: the float32 model with its own float32 lse table
    against the reference; span scores where the two paths agree."""
    ref, m32 = reference(k), align_model(k, np.float32)
    ep = es = 0.0
    same = 0
    for p in ref.paths:
        ep = max(ep, abs(float(m32.cost[p]) - float(ref.cost[p])))
        if np.array_equal(m32.paths[p], ref.paths[p]):
            same += 1
            L = int(k.lens[p[1]])
            if L:
                es = max(es, float(np.abs(m32.score[p][:L].astype(np.float64) - ref.score[p][:L]).max()))
    return ep, es, same


# case -> (path_cost floor, span score floor): what the docstring's table quotes and tests/test_ctc_align_cases.py recomputes
FLOORS = {
    'lane31': (6.494e-05, 1.276e-05),
    'lane32': (1.247e-04, 5.623e-06),
    'lane63': (2.645e-04, 1.134e-04),
    'lane64': (1.486e-04, 3.828e-05),
    'lane127': (4.352e-04, 1.470e-04),
    'lane128': (5.600e-04, 2.544e-06),
    'L255': (9.398e-04, 1.035e-04),
    'repeats': (1.323e-06, 5.271e-07),
    'brute': (1.075e-06, 8.085e-07),
    'brute_last': (9.821e-07, 3.314e-07),
    'K3': (2.436e-06, 1.172e-06),
    'K4': (1.382e-06, 1.054e-06),
    'K5': (2.721e-06, 3.779e-07),
    'K257': (5.180e-06, 2.219e-06),
    'C37': (2.344e-06, 5.940e-07),
    'C1024': (3.451e-06, 2.461e-06),
    'C1028': (4.765e-06, 8.680e-07),
    'C16384': (3.433e-06, 1.166e-06),
    'bad': (2.900e-06, 9.104e-07),
    'saturated': (1.102e-05, 1.368e-06),
    'flat': (2.609e-07, 9.747e-08),
    'tight': (1.310e-05, 4.576e-06),
    'planted': (3.238e-07, 8.498e-07),
    'T1': (3.777e-07, 3.777e-07),
    'T64': (3.107e-05, 2.091e-05),
    'T65': (3.063e-05, 3.828e-05),
    'T128': (8.575e-05, 1.755e-05),
    'T129': (1.882e-04, 3.036e-05),
    'ends': (2.580e-06, 2.007e-06),
    'short': (5.716e-06, 1.492e-06),
}


# ---------------------------------------------------------------- trained logits (tests/golden/trained_expect.npz)
# worst |float32 path cost - float64 path cost| of the true labels on the committed logits of C1 and V0 (tests/test_ctc_align_cases.py recomputes it)
TRAINED_PATH_FLOOR = 6.24e-06      # V0 (C1: 2.70e-6); the smallest margins there are 0.26 (C1) and 0.032 (V0)
TRAINED_PATH_BOUND = 8 * TRAINED_PATH_FLOOR
TRAINED_BATCHES = ('C1', 'V0')


def trained_truth(name):
    """-> logits [T, N, C] float32 of the committed fixture, the true label lists, input lengths."""
    acts, labels, ll, sl = lc.tt.trained_batch(name)[:4]
    truth, pos = [], 0
    for n in ll:
        truth.append([int(v) for v in labels[pos:pos + n]])
        pos += n
    return acts, truth, sl


def trained_floor(name):
    """(float32 floor of the path cost, smallest margin, samples the float32 path differs on) of the true labels on the committed logits."""
    acts, truth, sl = trained_truth(name)
    worst, lead, differ = 0.0, np.inf, 0
    for n, label in enumerate(truth):
        Tn = min(int(sl[n]), acts.shape[0])
        if len(label) + lc.repeats(label) > Tn:
            continue
        p64, _, _, _, c64, lyx, skip = align_rows(acts[:Tn, n], label, 0, np.float64)
        p32, _, _, _, c32, _, _ = align_rows(acts[:Tn, n], label, 0, np.float32)
        worst = max(worst, abs(float(c32) - float(c64)))
        lead = min(lead, margin_of(lyx, skip, p64))
        differ += int(not np.array_equal(p32, p64))
    return worst, lead, differ
