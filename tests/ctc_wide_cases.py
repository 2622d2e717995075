"""Cases, bounds and host arithmetic of the wide-alphabet CTC loss (ctc_long.hip: ctc_wide_rows_kernel + ctc_wide_samples_kernel).  A helper module,
not collected; the Case class, the float32 model and the oracle are those of tests/ctc_long_cases.py.

Reference: the float64 oracle (oracle/ctc.py::ctc_loss_numpy).  Bounds, by the rule of tests/test_gpu_ctc_trained.py: the kernels' recursion in
numpy float32 (that file's ctc_recursion) against the oracle gives the floor that float32 log-space arithmetic has of its own on these inputs,
and the bound is 8 x that floor (the recursion waves use v_exp_f32 / v_log_f32, the rows kernel v_exp_f32 for the softmax: about 2^-21
relative against libm's 2^-24).  The bf16 training form adds one rounding: scale * GRAD_BOUND + half a bf16 ulp of the reference.

Measured float32 floor per case (tests/test_ctc_wide_cases.py recomputes and prints it; L + repeats - Tn per sample in brackets):

    case          T    N  C      max_label_len  slots/lane  row path (threads, vector)  [L + repeats - Tn]    cost floor   gradient floor   oracle costs
    past_long      64  3   2100   40            2           256, 4                      [-24, -33, -2]        6.824e-05    9.945e-05        26.2 .. 497.0
    odd_C          20  3   4097    8            2           512, 1                      [-12, -12, -17]       1.904e-05    3.117e-05        151.0 .. 188.0
    charset        24  3   6625   12            2           512, 1                      [-12, -17, -9]        1.720e-05    4.193e-05        177.7 .. 217.8
    max_C          12  3  16384    5            2           1024, 8                     [-7, -8, -8]          8.043e-06    9.570e-06        98.7 .. 119.9
    L64            73  3   2100   64            4           256, 4                      [-9, -3, -63]         1.041e-04    1.955e-04        584.8 .. 628.0
    L255          264  3   2100  255            8           256, 4                      [-9, -2, -234]        8.953e-04    1.112e-03        2202.4 .. 2401.7
    feasible       53  3   4096   40            2           256, 8                      [0, 1, -10]           1.197e-04    2.024e-04        0 (once), 457.8 .. 469.0
    one_class      45  3   8196   30            2           1024, 4                     [0, -15, -35]         6.909e-05    8.065e-05        418.6 .. 425.9
    ragged         40  4   4100   20            2           512, 4                      [0, -20, -5, -10]     7.419e-05    8.127e-05        9.7 .. 336.2
    saturated      30  3   4096   25            2           256, 8                      [-20, -5, -6]         1.253e-04    2.386e-04        571.9 .. 1502.5
    C8192          10  3   8192    4            2           512, 8                      [-6, -5, -8]          4.398e-06    1.244e-05        75.1 .. 99.6
    odd_wide       10  3   8193    4            2           1024, 1                     [-6, -7, -5]          9.828e-06    8.873e-06        69.7 .. 96.7

The floor is that of random logits of spread 2 (7 to 10 nats a frame at these class counts: alpha + beta runs to -2400 at T = 264, where a
float32 has an ulp of 2.4e-4), as in tests/ctc_long_cases.py; the class count itself adds little (the softmax denominator is one float32
sum of C terms).

                                   float32 floor          bound (8 x)
    cost, absolute                 8.96e-4 (L255)         7.17e-3
    gradient entry, absolute       1.113e-3 (L255)        8.90e-3

The device's own figures are in tests/test_gpu_ctc_wide.py's docstring."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_long_cases as lc  # noqa: E402

octc = lc.octc
ctc_recursion = lc.ctc_recursion
Case = lc.Case

COST_FLOOR = 8.96e-04     # L255: T = 264, costs up to 2402
GRAD_FLOOR = 1.113e-03    # L255
COST_BOUND = 8 * COST_FLOOR
GRAD_BOUND = 8 * GRAD_FLOOR

# ---------------------------------------------------------------- the library's host arithmetic, restated (ocr_ctc_wide_supported / _workspace_size)
MAX_C = 16384
MAX_LABEL = 255
ROW_ELEMENTS_PER_THREAD = 16


def supported(C, T, max_label_len):
    return 0 < C <= MAX_C and T > 0 and 1 <= max_label_len <= MAX_LABEL


def workspace_bytes(C, max_label_len, T, N):
    """Three [T][64 * slots-per-lane] float tables per sample (logy, alpha, beta), rounded up to 256 bytes; None where the shape is refused."""
    if N <= 0 or not supported(C, T, max_label_len):
        return None
    return (N * 3 * T * 64 * lc.slots_per_lane(max_label_len) * 4 + 255) // 256 * 256


def row_path(C):
    """(threads of a row's workgroup, elements per load) of ctc_wide_rows_kernel for 16-byte aligned tensors."""
    return ([nt for nt in (256, 512, 1024) if C <= nt * ROW_ELEMENTS_PER_THREAD][0], 8 if C % 8 == 0 else 4 if C % 4 == 0 else 1)


# ---------------------------------------------------------------- cases
def _abab(a, b, pairs):
    return lambda rng: [a, b] * pairs


def build_cases():
    c = []
    # the shape the long kernel's placement refuses (tests/test_ctc_long_cases.py pins (2100, 64, 40) -> 0)
    c.append(Case('past_long', 201, 64, 2100, [40, 17, 1], [64, 50, 3], max_label_len=40))
    # unaligned rows: the scalar row path, blank last
    c.append(Case('odd_C', 202, 20, 4097, [8, 5, 3], [20, 17, 20], blank=4096))
    # a common character-set size, unaligned rows
    c.append(Case('charset', 203, 24, 6625, [12, 7, 10], [24, 24, 19]))
    # the class-count cap, with the first and the last class in the labels
    c.append(Case('max_C', 204, 12, 16384, [[1, 16383, 5000, 16383, 1], [16383], 4], [12, 9, 12], max_label_len=5))
    # 4 and 8 slots per lane
    c.append(Case('L64', 205, 73, 2100, [64, 64, 10], [73, 67, 73]))
    c.append(Case('L255', 206, 264, 2100, [255, 255, 30], [264, 257, 264]))
    # barely feasible / infeasible, labels with 3 repeats
    l40 = lambda rng: lc._with_repeats(lc._draw(rng, 40, 4096, 0), 3)
    c.append(Case('feasible', 207, 53, 4096, [l40, l40, l40], [43, 42, 53], slack=[0, 1, -10]))
    # one class in many non-adjacent slots (the sum through the class's first slot): [7] * 20 is a single alignment at Tn = 39; a b a b ...
    c.append(Case('one_class', 208, 45, 8196, [lc._one_class(7, 20), _abab(3, 9, 15), 10], [39, 45, 45], slack=[0, -15, -35]))
    # ragged: Tn = 1 with L = 1, Tn = T, Tn below every other sample's
    c.append(Case('ragged', 209, 40, 4100, [1, 20, 20, 12], [1, 40, 25, 22], slack=[0, -20, -5, -10], blank=4099))
    # saturated logits
    c.append(Case('saturated', 210, 30, 4096, [10, 25, 5], [30, 30, 11], gain=16.0))
    # the row paths no case above takes: 512 threads with 8 elements per load, 1024 threads with scalar loads
    c.append(Case('C8192', 211, 10, 8192, [4, 3, 2], [10, 8, 10]))
    c.append(Case('odd_wide', 212, 10, 8193, [4, 3, 2], [10, 10, 7], blank=8192))
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
