"""The cases of the long-label CTC kernel (tests/ctc_long_cases.py) checked on the CPU: they are the edge cases they claim to be, both
oracles agree on them, and the float32 floor their bounds quote is the measured one."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_long_cases as lc  # noqa: E402


def test_cases_are_the_intended_edges():
    by = {k.name: k for k in lc.cases()}
    # barely feasible / infeasible, at L = 40 and L = 130; one repeated class; ragged
    assert by['feasible'].feasibility() == [0, 1, -10, 0, 1, -10]
    assert [len(l) for l in by['feasible'].labels] == [40, 40, 40, 130, 130, 130]
    assert by['repeats'].feasibility() == [0, -41, -80] and set(by['repeats'].labels[0]) == {7} and len(by['repeats'].labels[0]) == 40
    assert by['ragged'].feasibility() == [0, -51, -15, -17] and by['ragged'].il[0] == 1 and by['ragged'].ll[0] == 1
    for k in lc.cases():
        assert k.slack is None or k.feasibility() == k.slack, k.name
        assert 3 <= k.N <= 6 and 1 <= k.ll.min() and k.ll.max() <= k.mll <= 255
    # every case but 'feasible' has feasible samples only
    assert [k.name for k in lc.cases() if k.infeasible().any()] == ['feasible']
    # the hand-over, the slots-per-lane boundaries, the stride, the class axis, both blanks
    assert list(by['handover'].ll) == [31, 32, 33, 1] and by['handover'].mll == 33 and (by['handover'].T, by['handover'].C) == (72, 37)
    assert [lc.slots_per_lane(by[n].mll) for n in ('L63', 'L64', 'L127', 'L128', 'L255')] == [2, 4, 4, 8, 8]
    assert all(by[n].T == by[n].mll + 9 and by[n].il.min() < by[n].T for n in ('L63', 'L64', 'L127', 'L128', 'L255'))
    assert by['stride'].mll == 255 and list(by['stride'].ll) == [3, 40, 130]
    assert {11, 65, 129, 200} <= {k.C for k in lc.cases()}
    assert {k.blank for k in lc.cases()} >= {0} and any(k.blank == k.C - 1 for k in lc.cases())
    assert by['saturated'].gain == 16.0 and all(k.gain == 2.0 for k in lc.cases() if k.name != 'saturated')
    # table placement: one shape just inside LDS, the next frame count outside
    assert by['lds_past'].T == by['lds_last'].T + 1 and by['lds_past'].mll == by['lds_last'].mll and by['lds_past'].C == by['lds_last'].C
    for k in lc.cases():
        assert lc.placement(k.C, k.T, k.mll) is not None, k.name
        assert k.place is None or lc.placement(k.C, k.T, k.mll) == k.place, k.name
    assert {lc.placement(k.C, k.T, k.mll) for k in lc.cases()} == {'lds', 'workspace'}
    assert lc.placement(37, 600, 256) is None and lc.placement(37, 600, 0) is None and lc.placement(37, 600, 255) == 'workspace'


def test_placement_rule_is_the_librarys():
    from lstm_ctc_ocr_amd import _native as nat
    code = {None: 0, 'lds': 1, 'workspace': 2}
    shapes = [(k.C, k.T, k.mll) for k in lc.cases()] + [(96, 128, 48), (96, 520, 255), (11, 20, 31), (37, 10, 255), (2100, 64, 40), (37, 64, 256)]
    for C, T, mll in shapes:
        assert nat.lib().ocr_ctc_long_placement(C, T, mll) == code[lc.placement(C, T, mll)], (C, T, mll)


def test_oracles_agree_and_float32_floor_is_what_the_bounds_quote():
    worst_c = worst_g = 0.0
    for k in lc.cases():
        ref_c, ref_g = lc.reference(k)
        cc, gc = lc.octc.ctc_loss_c(k.acts, k.flat, k.ll, k.il, k.blank)
        assert np.allclose(cc, ref_c, rtol=1e-6, atol=1e-6) and np.abs(gc - ref_g).max() < 1e-6, k.name     # ctc_loss_c returns float32
        c64, g64 = lc.ctc_recursion(k.acts, k.flat, k.ll, k.il, k.blank, np.float64)
        assert np.abs(c64 - ref_c).max() < 1e-9 and np.abs(g64 - ref_g).max() < 1e-11, k.name                # the same recursion as the oracle's
        bad = k.infeasible()
        assert np.all(ref_c[bad] == 0) and not ref_g[:, bad].any(), k.name
        assert np.all(np.isfinite(ref_c)) and np.all(ref_c[~bad] > 0), k.name
        assert not ref_g[k.il.min():, int(np.argmin(k.il))].any()                                            # frames past Tn: zero gradient
        c32, g32 = lc.ctc_recursion(k.acts, k.flat, k.ll, k.il, k.blank, np.float32)
        ec, eg = float(np.abs(c32 - ref_c).max()), float(np.abs(g32 - ref_g).max())
        print('%-16s T=%3d N=%d C=%3d max_label_len=%3d %-9s float32 floor: cost %.3e, gradient entry %.3e; costs %.4g .. %.4g'
              % (k.name, k.T, k.N, k.C, k.mll, lc.placement(k.C, k.T, k.mll), ec, eg, ref_c.min(), ref_c.max()))
        worst_c, worst_g = max(worst_c, ec), max(worst_g, eg)
    print('float32 floor over the cases: cost %.3e, gradient entry %.3e' % (worst_c, worst_g))
    # the quoted floor is the measured one within a factor of two and is not exceeded
    assert lc.COST_FLOOR / 2 <= worst_c <= lc.COST_FLOOR, (worst_c, lc.COST_FLOOR)
    assert lc.GRAD_FLOOR / 2 <= worst_g <= lc.GRAD_FLOOR, (worst_g, lc.GRAD_FLOOR)
    assert lc.COST_BOUND == 8 * lc.COST_FLOOR and lc.GRAD_BOUND == 8 * lc.GRAD_FLOOR
