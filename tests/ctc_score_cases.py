"""Cases, float64 reference, float32 model and bounds of lexicon scoring under CTC (ctc_score.hip: ctc_score_rows_kernel, ctc_score_cands_kernel,
ctc_score_best_kernel; ops.ctc_score).  A helper module, not collected.

Reference: per (sample, candidate) the alpha half of oracle/ctc.py::ctc_loss_numpy written out in float64 (tests/test_ctc_score_cases.py checks it
against that function and against oracle.ctc.ctc_brute_force over all labellings), +inf where the candidate cannot be emitted: input length <= 0,
length + repeats above the input length, a declared length outside [0, max_label_len], or a label inside the length that is outside [0, C) or
equals the blank.  best = arg-min with the lowest index on ties (-1 when every cost is +inf), log_norm = np.logaddexp.reduce(-costs).

Bounds, by the rule of tests/ctc_wide_cases.py: the same recursion in numpy float32 against the reference gives the floor that float32 log-space
arithmetic has of its own on these inputs, and the bound is 8 x that floor (the recursion uses v_exp_f32 / v_log_f32, the row sums v_exp_f32:
about 2^-21 relative against libm's 2^-24).  Logits are random with spread 2, as in the wide cases.

Measured float32 floor per case (tests/test_ctc_score_cases.py recomputes and prints it):

    case        T    N  C      K    max_label_len  slots/lane  row path (threads per row, vector)  cost floor   log_norm floor   finite costs
    lane31       72  2     40    5   31            1           64, 8                               6.485e-05    8.959e-06        235.2 .. 405.3
    lane32       72  2     40    5   32            2           64, 8                               1.247e-04    5.540e-06        228.2 .. 378.8
    lane63      140  2     40    4   63            2           64, 8                               2.645e-04    8.125e-05        439.6 .. 793.1
    lane64      140  2     40    4   64            4           64, 8                               2.071e-04    1.815e-05        457.7 .. 745.6
    lane127     264  2     40    3  127            4           64, 8                               5.444e-04    5.444e-04        861.8 .. 1426.3
    lane128     264  2     40    3  128            8           64, 8                               5.600e-04    1.551e-04        868.8 .. 1429.0
    L255        520  1     24    3  255            8           64, 8                               6.659e-04    6.317e-04        1431.1 .. 2404.3
    repeats       8  5      6    8    6            1           64, 1                               1.323e-06    6.971e-07        1.4 .. 22.4
    brute         5  3      4   40    3            1           64, 4                               1.075e-06    1.411e-07        0.7 .. 13.5
    brute_last    5  3      4   40    3            1           64, 4                               9.821e-07    2.299e-07        0.4 .. 17.9
    K1           10  3     12    1    0            1           64, 4                               9.773e-07    9.773e-07        34.5 .. 41.6
    K3           10  3     12    3    4            1           64, 4                               2.934e-06    3.007e-06        13.3 .. 27.2
    K4           10  3     12    4    4            1           64, 4                               3.078e-06    2.583e-06        11.8 .. 27.5
    K5           10  3     12    5    4            1           64, 4                               3.814e-06    3.474e-06        17.9 .. 35.0
    K257         10  3     12  257    4            1           64, 4                               5.540e-06    1.197e-05        9.6 .. 44.9
    C37           6  2     37    5    3            1           64, 1                               1.806e-06    2.018e-06        14.0 .. 32.3
    C38           6  2     38    5    3            1           64, 1                               1.991e-06    9.525e-07        14.1 .. 23.6
    C40           6  2     40    5    3            1           64, 8                               4.057e-06    4.506e-07        15.0 .. 42.1
    C44           6  2     44    5    3            1           64, 4                               3.673e-06    6.379e-07        16.8 .. 43.1
    C1024         6  2   1024    5    3            1           64, 8                               4.716e-06    2.578e-06        27.6 .. 53.4
    C1028         6  2   1028    5    3            1           256, 4                              3.727e-06    1.835e-06        26.8 .. 45.0
    C4100         6  2   4100    5    3            1           512, 4                              3.952e-06    9.428e-07        33.4 .. 63.0
    C8200         6  2   8200    5    3            1           1024, 8                             8.987e-06    1.701e-06        32.9 .. 71.0
    C16384        6  2  16384    5    3            1           1024, 8                             4.727e-06    7.884e-07        40.0 .. 72.9
    bad          10  3     12    9    3            1           64, 4                               3.521e-06    2.723e-06        23.2 .. 26.2
    dups         12  3     12   12    4            1           64, 4                               5.524e-06    2.380e-06        1.4 .. 46.1
    saturated    10  3     12    8    4            1           64, 4                               1.593e-05    8.665e-07        20.9 .. 110.0

                                   float32 floor          bound (8 x)
    cost, absolute                 6.66e-4 (L255)         5.33e-3
    log_norm, absolute             6.32e-4 (L255)         5.06e-3

The floor grows with T: at T = 520 alpha runs to -2400, where a float32 has an ulp of 2.4e-4.  Outside the deliberate duplicates every sample's
best candidate leads the runner-up by more than 2 x COST_BOUND (2 x COST_BOUND = 1.07e-2; the smallest lead is 2.48e-2, brute_last), so the arg-min is well defined; the
CPU test asserts it.  The device's own figures are in tests/test_gpu_ctc_score.py's docstring."""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_long_cases as lc  # noqa: E402

octc = lc.octc
_lse = lc.tt._lse

COST_FLOOR = 6.66e-04     # L255: T = 520, costs up to 2404
NORM_FLOOR = 6.32e-04     # L255
COST_BOUND = 8 * COST_FLOOR
NORM_BOUND = 8 * NORM_FLOOR

# ---------------------------------------------------------------- the library's host arithmetic, restated (ocr_ctc_score_supported / _workspace_size)
MAX_C = 16384
MAX_LABEL = 255
MAX_K = 65536
ROW_ELEMENTS_PER_THREAD = 16


def supported(C, T, max_label_len, K):
    return 1 <= C <= MAX_C and T >= 1 and 0 <= max_label_len <= MAX_LABEL and 1 <= K <= MAX_K


def workspace_bytes(C, T, N):
    """One float per logit row (the log-sum-exp table), rounded up to 256 bytes; None where the shape is refused."""
    if N <= 0 or not supported(C, T, 0, 1) or N * T > 0x7fffffff:
        return None
    return (N * T * 4 + 255) // 256 * 256


def slots_per_lane(max_label_len):
    s = 2 * max_label_len + 1
    return 1 if s <= 64 else 2 if s <= 128 else 4 if s <= 256 else 8


def row_path(C):
    """(threads that hold one row, elements per load) of ctc_score_rows_kernel for 16-byte aligned logits: a wave per row up to 1024 classes."""
    return ([nt for nt in (64, 256, 512, 1024) if C <= nt * ROW_ELEMENTS_PER_THREAD][0], 8 if C % 8 == 0 else 4 if C % 4 == 0 else 1)


# ---------------------------------------------------------------- reference and float32 model
def candidate_ok(label, declared, mll, C, blank, Tn):
    """The feasibility rules: False means cost +inf."""
    if Tn <= 0 or declared < 0 or declared > mll:
        return False
    lab = label[:declared]
    if any(v < 0 or v >= C or v == blank for v in lab):
        return False
    return declared + lc.repeats(lab) <= Tn


def alpha_cost(logy, label, blank):
    """-log p(label) from log-probabilities logy [Tn, C], every operation in logy's dtype: the alpha half of ctc_loss_numpy, a row at a time."""
    dtype = logy.dtype.type
    NEG = dtype(-np.inf)
    ext = np.full(2 * len(label) + 1, blank, np.int64)
    ext[1::2] = label
    S = len(ext)
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ly = logy[:, ext]
    a = np.full(S, NEG, dtype)
    a[:2] = ly[0, :2]
    for t in range(1, len(logy)):
        c = np.full((3, S), NEG, dtype)
        c[0] = a; c[1, 1:] = a[:-1]; c[2, 2:] = np.where(skip[2:], a[:-2], NEG)
        a = _lse(c, 0) + ly[t]
    return -_lse(a[max(S - 2, 0):], 0)


def score_model(k, dtype):
    """costs [N, K] (+inf where a candidate cannot be emitted), best [N], best_cost [N], log_norm [N] of case k with the recursion in `dtype`."""
    costs = np.full((k.N, k.K), np.inf, dtype)
    for n in range(k.N):
        Tn = min(int(k.il[n]), k.T)
        if Tn <= 0:
            continue
        rows = k.acts[:Tn, n].astype(dtype)
        logy = rows - _lse(rows, 1)[:, None]
        for j in range(k.K):
            if candidate_ok(k.lexicon[j], int(k.lens[j]), k.mll, k.C, k.blank, Tn):
                costs[n, j] = alpha_cost(logy, k.lexicon[j][:int(k.lens[j])], k.blank)
    return (costs,) + summary(costs)


def summary(costs):
    """best (lowest index on ties, -1 when nothing is finite), best_cost, log_norm of a cost matrix, in its dtype."""
    any_ = np.isfinite(costs).any(axis=1)
    best = np.where(any_, np.argmin(costs, axis=1), -1).astype(np.int32)
    with np.errstate(divide='ignore'):
        norm = np.array([np.logaddexp.reduce(-row) for row in costs], costs.dtype)
    return best, costs.min(axis=1), norm


# ---------------------------------------------------------------- cases
class ScoreCase(object):
    """lexicon: candidates as label lists (an int draws that many random labels without adjacent repeats); lens: declared lengths where they
    differ from the lists'; boost = (sample, candidate): that sample's logits are raised along one alignment of the candidate."""

    def __init__(self, name, seed, T, C, in_lens, lexicon, mll=None, blank=0, lens=None, dups=(), boost=None, saturate=False):
        self.name, self.seed, self.T, self.C, self.blank, self.dups = name, seed, T, C, blank, tuple(dups)
        rng = np.random.RandomState(seed)
        self.N = len(in_lens)
        self.acts = (rng.randn(T, self.N, C) * 2.0).astype(np.float32)
        self.lexicon = [lc._draw(rng, l, C, blank) if isinstance(l, int) else list(l) for l in lexicon]
        for a, b in self.dups:
            self.lexicon[b] = list(self.lexicon[a])
        self.K = len(self.lexicon)
        self.lens = np.array([len(l) for l in self.lexicon] if lens is None else lens, np.int32)
        self.il = np.array(in_lens, np.int32)
        self.mll = int(max(len(l) for l in self.lexicon)) if mll is None else mll
        if boost is not None:
            n, j = boost
            Tn = min(int(self.il[n]), T)
            path = [v for c in self.lexicon[j] for v in (c, blank)]
            assert len(path) <= Tn
            path += [blank] * (Tn - len(path))
            for t, c in enumerate(path):
                self.acts[t, n, c] += 8.0
        if saturate:                         # one frame with +80 on a class, one with -80 on another
            self.acts[3, :, self.lexicon[0][0]] = 80.0
            self.acts[5, :, self.lexicon[1][0]] = -80.0
        self.acts.setflags(write=False)

    def packed(self):
        """int32 [K, max_label_len] labels and [K] declared lengths; words at and beyond a candidate's length alternate -1 and C + 7."""
        lab = np.empty((self.K, self.mll), np.int32)
        lab[:, 0::2] = -1
        lab[:, 1::2] = self.C + 7
        for j, l in enumerate(self.lexicon):
            n = min(len(l), self.mll, max(int(self.lens[j]), 0))
            lab[j, :n] = l[:n]
        return lab, self.lens.copy()

    def per_sample(self):
        """The same strings in a different order for every sample: labels [N, K, max_label_len], lengths [N, K], perm [N, K] with entry (n, j) the
        shared lexicon's index of sample n's candidate j."""
        lab, lens = self.packed()
        rng = np.random.RandomState(self.seed + 1000)
        perm = np.stack([rng.permutation(self.K) for _ in range(self.N)])
        return np.ascontiguousarray(lab[perm]), np.ascontiguousarray(lens[perm]), perm


def _distinct(rng, K, C, blank, max_len):
    """K distinct strings of 0 .. max_len labels."""
    seen, out = set(), []
    while len(out) < K:
        s = tuple(lc._draw(rng, int(rng.randint(0, max_len + 1)), C, blank, norep=False))
        if s not in seen:
            seen.add(s)
            out.append(list(s))
    return out


ROW_PATH_CLASSES = (37, 38, 40, 44, 1024, 1028, 4100, 8200, 16384)
GRID_K = (1, 3, 4, 5, 257)


def build_cases():
    SC = ScoreCase
    c = []
    # lane boundaries: the last label length of 1, 2 and 4 slots per lane and the first of 2, 4 and 8; the empty string and one character beside them
    c.append(SC('lane31', 301, 72, 40, [72, 70], [0, 1, 31, 31, 7], mll=31))
    c.append(SC('lane32', 302, 72, 40, [72, 66], [0, 1, 31, 32, 9], mll=32))
    c.append(SC('lane63', 303, 140, 40, [140, 130], [0, 1, 63, 20], mll=63))
    c.append(SC('lane64', 304, 140, 40, [140, 131], [0, 1, 63, 64], mll=64, blank=39))
    c.append(SC('lane127', 305, 264, 40, [264, 258], [1, 127, 40], mll=127))
    c.append(SC('lane128', 306, 264, 40, [264, 259], [0, 127, 128], mll=128))
    c.append(SC('L255', 307, 520, 24, [520], [255, 100, 3], mll=255))
    # repeats (a = 1, b = 2): aa, aaa, abab, aabb, aabbab (L + repeats = 8), the empty string, one character, two characters
    c.append(SC('repeats', 308, 8, 6, [8, 5, 4, 1, 0], [[1, 1], [1, 1, 1], [1, 2, 1, 2], [1, 1, 2, 2], [1, 1, 2, 2, 1, 2], [], [3], [4, 5]], mll=6))
    # every string of up to 3 labels over 3 classes: the sizes oracle.ctc.ctc_brute_force enumerates
    every = [list(s) for n in range(4) for s in itertools.product((1, 2, 3), repeat=n)]
    c.append(SC('brute', 309, 5, 4, [5, 4, 2], every, mll=3))
    c.append(SC('brute_last', 310, 5, 4, [5, 4, 2], [[v - 1 for v in s] for s in every], mll=3, blank=3))
    # grid edges: K around the four candidates of a workgroup; K = 1 is the empty string alone with max_label_len = 0
    for K in GRID_K:
        rng = np.random.RandomState(400 + K)
        blank = 11 if K == 5 else 0
        c.append(SC('K%d' % K, 320 + K, 10, 12, [10, 7, 10], [[]] if K == 1 else _distinct(rng, K, 12, blank, 4), mll=0 if K == 1 else 4, blank=blank))
    # row paths: a wave per row (vector 1 / 1 / 8 / 4 / 8, C = 1024 the last), then 256, 512 and 1024 threads per row; first and last class in a label
    for C in ROW_PATH_CLASSES:
        blank = C - 1 if C == 38 else 0
        ends = [0, C - 2] if blank else [1, C - 1]
        c.append(SC('C%d' % C, 340 + len(c), 6, C, [6, 4], [ends, 0, 1, 3, 3], mll=3, blank=blank))
    # bad labels and lengths: label = C, label = -1, the blank inside, far out of range both ways, declared length -1 and max_label_len + 1
    c.append(SC('bad', 360, 10, 12, [10, 7, 10], [[3, 4], [3, 12, 4], [3, -1], [5, 0, 6], [7], [3, 2 ** 31 - 1], [-2 ** 31], [1, 2], [1, 2, 3]], mll=3,
                lens=[2, 3, 2, 3, 1, 2, 1, -1, 4]))
    # duplicates: the string at index 2 again at index 9, and the best candidate of sample 0
    rng = np.random.RandomState(361)
    c.append(SC('dups', 361, 12, 12, [12, 12, 9], [l if l else [5] for l in _distinct(rng, 12, 12, 0, 4)], mll=4, dups=[(2, 9)], boost=(0, 2)))
    # saturated frames
    rng = np.random.RandomState(362)
    c.append(SC('saturated', 362, 10, 12, [10, 10, 8], [l if l else [6] for l in _distinct(rng, 8, 12, 0, 4)], mll=4, saturate=True))
    return c


PER_SAMPLE_CASES = ('K5', 'K257', 'dups', 'bad')

_CASES = None
_REF = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def case(name):
    return [k for k in cases() if k.name == name][0]


def reference(k):
    """float64 costs [N, K], best, best_cost, log_norm of a case: computed once per process, shared and left unchanged by every test."""
    if k.name not in _REF:
        out = score_model(k, np.float64)
        for v in out:
            v.setflags(write=False)
        _REF[k.name] = out
    return _REF[k.name]


def margin(k):
    """The smallest lead of a sample's best candidate over its runner-up in the reference, the deliberate duplicates counted once."""
    costs = reference(k)[0]
    keep = [j for j in range(k.K) if j not in [b for _, b in k.dups]]
    lead = np.inf
    for row in costs[:, keep]:
        fin = np.sort(row[np.isfinite(row)])
        if len(fin) >= 2:
            lead = min(lead, fin[1] - fin[0])
    return lead
