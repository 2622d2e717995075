"""The cases of the wide-alphabet CTC loss (tests/ctc_wide_cases.py) checked on the CPU: they are the edge cases they claim to be, the
library's host-only arithmetic is the one the helper restates, and the float32 floor their bounds quote is the measured one."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_wide_cases as wc  # noqa: E402

lc = wc.lc


def test_cases_are_the_intended_edges():
    by = {k.name: k for k in wc.cases()}
    assert list(by) == ['past_long', 'odd_C', 'charset', 'max_C', 'L64', 'L255', 'feasible', 'one_class', 'ragged', 'saturated', 'C8192', 'odd_wide']
    for k in wc.cases():
        assert k.slack is None or k.feasibility() == k.slack, k.name
        assert 3 <= k.N <= 4 and 1 <= k.ll.min() and k.ll.max() <= k.mll <= 255
        assert wc.supported(k.C, k.T, k.mll) and k.acts.nbytes <= 8 << 20, k.name
    # the shape the long kernel refuses
    p = by['past_long']
    assert (p.C, p.T, p.mll) == (2100, 64, 40) and list(p.ll) == [40, 17, 1] and list(p.il) == [64, 50, 3]
    assert lc.placement(2100, 64, 40) is None
    # unaligned rows; the character set; the cap with its first and last class in a label
    assert (by['odd_C'].C, by['odd_C'].T, by['odd_C'].blank) == (4097, 20, 4096)
    assert (by['charset'].C, by['charset'].T) == (6625, 24) and by['charset'].ll.max() <= 12
    m = by['max_C']
    assert (m.C, m.T) == (16384, 12) and m.ll.max() <= 5 and {1, 16383} <= set(m.flat.tolist())
    # every row path: 256, 512 and 1024 threads, 8 / 4 / 1 elements per load ((256, 1): the small alphabets of tests/test_gpu_ctc_wide.py)
    assert {wc.row_path(k.C) for k in wc.cases()} == {(256, 8), (256, 4), (512, 8), (512, 4), (512, 1), (1024, 8), (1024, 4), (1024, 1)}
    assert wc.row_path(4096) == (256, 8) and wc.row_path(4097) == (512, 1) and wc.row_path(8192)[0] == 512 and wc.row_path(8193)[0] == 1024
    # slots per lane
    assert (by['L64'].C, by['L64'].T, by['L255'].C, by['L255'].T) == (2100, 73, 2100, 264) and list(by['L255'].il) == [264, 257, 264]
    assert [lc.slots_per_lane(by[n].mll) for n in ('past_long', 'L64', 'L255')] == [2, 4, 8]
    # barely feasible / infeasible with repeats; it is the only case with an infeasible sample
    f = by['feasible']
    assert f.C == 4096 and f.feasibility() == [0, 1, -10] and all(lc.repeats(l) == 3 for l in f.labels)
    assert [k.name for k in wc.cases() if k.infeasible().any()] == ['feasible']
    # one class in many slots
    o = by['one_class']
    assert o.labels[0] == [7] * 20 and o.il[0] == 39 and o.labels[1] == [3, 9] * 15 and o.feasibility()[0] == 0
    # ragged
    r = by['ragged']
    assert r.il[0] == 1 and r.ll[0] == 1 and r.il.max() == r.T and r.il.min() < r.T
    # saturated logits
    assert by['saturated'].gain == 16.0 and by['saturated'].C == 4096 and all(k.gain == 2.0 for k in wc.cases() if k.name != 'saturated')
    assert {k.blank for k in wc.cases()} >= {0} and any(k.blank == k.C - 1 for k in wc.cases())


def test_host_arithmetic_is_the_librarys():
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    for C, T, mll in [(16384, 63, 25), (16385, 63, 25), (4096, 63, 0), (4096, 63, 1), (4096, 63, 255), (4096, 63, 256), (0, 63, 25), (1, 1, 1),
                      (4096, 0, 25), (-1, 63, 25)]:
        assert bool(lib.ocr_ctc_wide_supported(C, T, mll)) == wc.supported(C, T, mll), (C, T, mll)
    assert [lib.ocr_ctc_wide_supported(16384, 63, 25), lib.ocr_ctc_wide_supported(16385, 63, 25)] == [1, 0]
    assert [lib.ocr_ctc_wide_supported(4096, 63, m) for m in (0, 1, 255, 256)] == [0, 1, 1, 0]
    sz = ctypes.c_size_t(0)
    for k in wc.cases():
        assert lib.ocr_ctc_wide_workspace_size(k.C, k.mll, k.T, k.N, ctypes.byref(sz)) == 0, k.name
        assert sz.value == wc.workspace_bytes(k.C, k.mll, k.T, k.N) and sz.value % 256 == 0, k.name
    for C, mll, T, N in [(16385, 25, 63, 4), (4096, 0, 63, 4), (4096, 256, 63, 4), (4096, 25, 0, 4), (4096, 25, 63, 0)]:
        assert wc.workspace_bytes(C, mll, T, N) is None and lib.ocr_ctc_wide_workspace_size(C, mll, T, N, ctypes.byref(sz)) == 2, (C, mll, T, N)
    assert lib.ocr_ctc_wide_workspace_size(4096, 25, 63, 4, None) == 2
    assert lib.ocr_ctc_long_placement(2100, 64, 40) == 0          # the long kernel still refuses what it refused
    assert lib.ocr_abi_version() == 1


def test_float32_floor_is_what_the_bounds_quote():
    worst_c = worst_g = 0.0
    for k in wc.cases():
        ref_c, ref_g = wc.reference(k)
        bad = k.infeasible()
        assert np.all(ref_c[bad] == 0) and not ref_g[:, bad].any(), k.name
        assert np.all(np.isfinite(ref_c)) and np.all(ref_c[~bad] > 0), k.name
        assert not ref_g[k.il.min():, int(np.argmin(k.il))].any()                                            # frames past Tn: zero gradient
        c32, g32 = wc.ctc_recursion(k.acts, k.flat, k.ll, k.il, k.blank, np.float32)
        ec, eg = float(np.abs(c32 - ref_c).max()), float(np.abs(g32 - ref_g).max())
        print('%-10s T=%3d N=%d C=%5d max_label_len=%3d row path %s float32 floor: cost %.3e, gradient entry %.3e; costs %.4g .. %.4g'
              % (k.name, k.T, k.N, k.C, k.mll, wc.row_path(k.C), ec, eg, ref_c.min(), ref_c.max()))
        worst_c, worst_g = max(worst_c, ec), max(worst_g, eg)
    print('float32 floor over the cases: cost %.3e, gradient entry %.3e' % (worst_c, worst_g))
    # the quoted floor is the measured one within a factor of two and is not exceeded
    assert wc.COST_FLOOR / 2 <= worst_c <= wc.COST_FLOOR, (worst_c, wc.COST_FLOOR)
    assert wc.GRAD_FLOOR / 2 <= worst_g <= wc.GRAD_FLOOR, (worst_g, wc.GRAD_FLOOR)
    assert wc.COST_BOUND == 8 * wc.COST_FLOOR and wc.GRAD_BOUND == 8 * wc.GRAD_FLOOR
