"""Cases, float32 model and bounds of the long-label CTC kernel (ctc_long.hip: ctc_long_kernel).  A helper module, not collected.

Reference: the float64 oracle (oracle/ctc.py::ctc_loss_numpy).  Bounds, by the rule of tests/test_gpu_ctc_trained.py: the kernels' recursion in
numpy float32 (that file's ctc_recursion) against the oracle gives the floor that float32 log-space arithmetic has of its own on these inputs,
and the bound is 8 x that floor (the recursion waves use v_exp_f32 / v_log_f32, about 2^-21 relative against libm's 2^-24).  The bf16 training
form adds one rounding: scale * GRAD_BOUND + half a bf16 ulp of the reference.

Measured float32 floor per case (tests/test_ctc_long_cases.py recomputes and prints it; L + repeats - Tn per sample in brackets):

    case             T    N  C    max_label_len  tables     [L + repeats - Tn]          cost floor   gradient floor   oracle costs
    handover          72  4   37   33            lds        [-41, -40, -37, -4]         8.222e-06    3.001e-05        29.7 .. 249.6
    L63               72  3   37   63            lds        [-9, -3, -62]               4.264e-06    7.598e-05        290.3 .. 311.0
    L64               73  3   37   64            workspace  [-9, -3, -63]               3.188e-05    1.698e-04        298.0 .. 324.2
    L127             136  3   37  127            workspace  [-9, -2, -127]              3.243e-04    4.691e-04        582.0 .. 648.3
    L128             137  3   37  128            workspace  [-9, -2, -128]              2.414e-04    2.766e-04        587.7 .. 668.9
    L255             264  3   37  255            workspace  [-9, -2, -234]              7.414e-04    1.066e-03        1017.7 .. 1302.6
    stride           140  3   11  255            workspace  [-137, -50, -10]            1.260e-04    1.557e-04        169.0 .. 448.0
    feasible         150  6   65  130            workspace  [0, 1, -10, 0, 1, -10]      2.493e-04    4.274e-04        0 (twice), 229.0 .. 798.3
    repeats          120  3  129   40            workspace  [0, -41, -80]               1.367e-04    2.628e-04        506.4 .. 655.0
    C200_blank_last  100  3  200   64            workspace  [-50, -44, -36]             3.376e-05    1.133e-04        363.9 .. 543.9
    ragged            96  4   37   45            workspace  [0, -51, -15, -17]          9.298e-05    1.301e-04        5.5 .. 326.6
    saturated        100  3   37   70            workspace  [-60, -30, -26]             4.385e-04    7.327e-04        689.6 .. 2171.6
    lds_last          83  3   37   40            lds        [-43, -50, -38]             4.884e-05    9.438e-05        189.7 .. 282.5
    lds_past          84  3   37   40            workspace  [-44, -51, -38]             9.278e-05    1.158e-04        186.8 .. 274.8
    line200          420  3   96  200            workspace  [-220, -210, -380]          9.967e-04    1.120e-03        1358.3 .. 2186.2

Random logits of spread 2 cost 4 to 5 nats a frame, so alpha + beta runs to -2000 and a float32 there has an ulp of 1.2e-4: the posteriors
exp(alpha + beta - logy - logp) carry that error whatever computes them in float32, which is why the floor grows with T and is far above the
one of trained logits (tests/test_gpu_ctc_trained.py: 1.4e-6).

                                   float32 floor          bound (8 x)
    cost, absolute                 9.97e-4 (line200)      7.98e-3
    gradient entry, absolute       1.121e-3 (line200)     8.97e-3

The device's own figures are in tests/test_gpu_ctc_long.py's docstring."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_ctc_trained as tt  # noqa: E402   (ctc_recursion, and the oracle import it sets up)

octc = tt.octc
ctc_recursion = tt.ctc_recursion

COST_FLOOR = 9.97e-04     # line200: T = 420, costs up to 2186
GRAD_FLOOR = 1.121e-03    # line200
COST_BOUND = 8 * COST_FLOOR
GRAD_BOUND = 8 * GRAD_FLOOR

# ---------------------------------------------------------------- the kernel's table placement rule, restated (ocr_ctc_long_placement)
CTC_NW = 16
LDS_MAX = 128 * 1024
MAX_LABEL = 255


def slots_per_lane(max_label_len):
    s = 2 * max_label_len + 1
    return 2 if s <= 128 else 4 if s <= 256 else 8


def placement(C, T, max_label_len):
    """'lds' / 'workspace' / None, as ops.ctc_long_placement answers."""
    if C <= 0 or T <= 0 or not 0 < max_label_len <= MAX_LABEL:
        return None
    sp = 64 * slots_per_lane(max_label_len)
    base = (T + CTC_NW * C + sp) * 4
    if base > LDS_MAX:
        return None
    return 'lds' if base + 3 * T * sp * 4 <= LDS_MAX else 'workspace'


def last_T_in_lds(C, max_label_len):
    T = 1
    while placement(C, T + 1, max_label_len) == 'lds':
        T += 1
    return T


# ---------------------------------------------------------------- cases
def repeats(label):
    return sum(1 for i in range(1, len(label)) if label[i] == label[i - 1])


def _draw(rng, L, C, blank, norep=True):
    lo, hi = (1, C) if blank == 0 else (0, C - 1)
    out = []
    for _ in range(L):
        v = int(rng.randint(lo, hi))
        while norep and out and v == out[-1]:
            v = int(rng.randint(lo, hi))
        out.append(v)
    return out


def _with_repeats(label, k):
    """k adjacent repeats put into a label that has none: positions 3, 7, 11, ... copy their left neighbour (and differ from their right one)."""
    label = list(label)
    for i in range(k):
        p = 3 + 4 * i
        label[p] = label[p - 1]
        assert label[p + 1] != label[p]
    assert repeats(label) == k
    return label


class Case(object):
    def __init__(self, name, seed, T, C, labels, in_lens, max_label_len=None, blank=0, gain=2.0, slack=None, place=None):
        self.name, self.seed, self.T, self.C, self.blank, self.gain = name, seed, T, C, blank, gain
        rng = np.random.RandomState(seed)
        self.acts = (rng.randn(T, len(labels), C) * gain).astype(np.float32)
        self.labels = [_draw(rng, l, C, blank) if isinstance(l, int) else l(rng) if callable(l) else list(l) for l in labels]
        self.N = len(labels)
        assert 3 <= self.N <= 6
        self.flat = np.array([v for l in self.labels for v in l], np.int32)
        self.ll = np.array([len(l) for l in self.labels], np.int32)
        self.il = np.array(in_lens, np.int32)
        self.mll = int(self.ll.max()) if max_label_len is None else max_label_len
        self.slack = slack                     # the intended L + repeats - Tn list (asserted literally by the CPU test), or None
        self.place = place                     # the intended table placement, or None
        assert all(0 <= v < C and v != blank for v in self.flat)

    def feasibility(self):
        return [len(l) + repeats(l) - min(int(t), self.T) for l, t in zip(self.labels, self.il)]

    def infeasible(self):
        return np.array([f > 0 for f in self.feasibility()])


def _one_class(k, L):
    return lambda rng: [k] * L


def build_cases():
    c = []
    # the S = 63 / 65 hand-over from the 64-lane kernel: L = 31, 32, 33 and 1 in one batch
    c.append(Case('handover', 101, 72, 37, [31, 32, 33, 1], [72, 72, 70, 5], max_label_len=33, place='lds'))
    # each slots-per-lane boundary, T = L + 9 and one ragged Tn
    c.append(Case('L63', 102, 72, 37, [63, 63, 10], [72, 66, 72], place='lds'))
    c.append(Case('L64', 103, 73, 37, [64, 64, 10], [73, 67, 73], place='workspace'))
    c.append(Case('L127', 104, 136, 37, [127, 127, 9], [136, 129, 136], place='workspace'))
    c.append(Case('L128', 105, 137, 37, [128, 128, 9], [137, 130, 137], place='workspace'))
    c.append(Case('L255', 106, 264, 37, [255, 255, 30], [264, 257, 264], place='workspace'))
    # table stride != every S; the product's C = 11
    c.append(Case('stride', 107, 140, 11, [3, 40, 130], [140, 90, 140], max_label_len=255))
    # barely feasible / infeasible at L = 40 and L = 130, labels with 3 and 5 repeats; C = 65
    l40 = lambda rng: _with_repeats(_draw(rng, 40, 65, 0), 3)
    l130 = lambda rng: _with_repeats(_draw(rng, 130, 65, 0), 5)
    c.append(Case('feasible', 108, 150, 65, [l40, l40, l40, l130, l130, l130], [43, 42, 53, 135, 134, 145], slack=[0, 1, -10, 0, 1, -10]))
    # one repeated class: Tn = 79 is a single alignment; C = 129
    c.append(Case('repeats', 109, 120, 129, [_one_class(7, 40), _one_class(7, 40), 40], [79, 120, 120], slack=[0, -41, -80]))
    # C = 200 with the blank last
    c.append(Case('C200_blank_last', 110, 100, 200, [50, 20, 64], [100, 64, 100], blank=199))
    # ragged: Tn = 1 with L = 1, Tn = T, Tn below every other sample's
    c.append(Case('ragged', 111, 96, 37, [1, 45, 45, 33], [1, 96, 60, 50], slack=[0, -51, -15, -17], blank=36))
    # saturated logits
    c.append(Case('saturated', 112, 100, 37, [40, 70, 5], [100, 100, 31], gain=16.0))
    # the last T with the three tables in LDS and the first one without, at max_label_len = 40
    t_in = last_T_in_lds(37, 40)
    c.append(Case('lds_last', 113, t_in, 37, [40, 30, 12], [t_in, t_in - 3, 50], place='lds'))
    c.append(Case('lds_past', 114, t_in + 1, 37, [40, 30, 12], [t_in + 1, t_in - 2, 50], place='workspace'))
    # a text line: 200 characters at T = 420, C = 96
    c.append(Case('line200', 115, 420, 96, [200, 90, 40], [420, 300, 420], place='workspace'))
    return c


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
    """float64 oracle costs and gradients of a case: computed once per process, shared and left unchanged by every test."""
    if k.name not in _REF:
        rc, rg = octc.ctc_loss_numpy(k.acts, k.flat, k.ll, k.il, k.blank)
        rc.setflags(write=False); rg.setflags(write=False)
        _REF[k.name] = (rc, rg)
    return _REF[k.name]
