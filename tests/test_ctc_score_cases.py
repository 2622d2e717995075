"""Lexicon scoring under CTC checked on the CPU (tests/ctc_score_cases.py): the reference against brute force and against the oracle's loss, the
float32 floor its bounds quote, the arg-min margin of every case, the cases being the edges they claim, and the library's host-only side
(ocr_ctc_score_supported, ocr_ctc_score_workspace_size, the refusals of ocr_ctc_score, the header)."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_score_cases as sc  # noqa: E402

lc = sc.lc


def test_reference_against_brute_force():
    """Every string of up to three labels over three classes at T <= 5: the reference is -log of the summed probability of the paths that collapse
    to the string, and +inf exactly where no path does."""
    for name in ('brute', 'brute_last'):
        k = sc.case(name)
        assert k.T <= 5 and k.C <= 4 and k.K == 40
        costs = sc.reference(k)[0]
        for n in range(k.N):
            Tn = int(k.il[n])
            _, table = sc.octc.ctc_brute_force(k.acts[:Tn, n], [], k.blank)
            assert abs(sum(table.values()) - 1) < 1e-12
            for j, label in enumerate(k.lexicon):
                p = table.get(tuple(label), 0.0)
                if p > 0:
                    assert abs(costs[n, j] + np.log(p)) < 1e-10, (name, n, label)
                else:
                    assert costs[n, j] == np.inf, (name, n, label)
            # the lexicon holds every string of up to 3 labels: with Tn <= 3 the posteriors within it sum to one
            if Tn <= 3:
                assert abs(sc.reference(k)[3][n]) < 1e-10


def test_reference_against_the_oracle_loss():
    """The written-out alpha half equals oracle.ctc.ctc_loss_numpy on the one sample with the one label, wherever that is feasible."""
    for name in ('lane32', 'repeats', 'K5', 'C38', 'dups', 'saturated'):
        k = sc.case(name)
        costs = sc.reference(k)[0]
        for n in range(k.N):
            for j in range(0, k.K, 2):
                if np.isfinite(costs[n, j]):
                    want, _ = sc.octc.ctc_loss_numpy(k.acts[:, n:n + 1], np.array(k.lexicon[j], np.int32), [len(k.lexicon[j])], k.il[n:n + 1], k.blank)
                    assert abs(want[0] - costs[n, j]) <= 1e-11 * max(1.0, want[0]), (name, n, j)


def test_float32_floor_is_what_the_bounds_quote():
    worst_c = worst_n = 0.0
    for k in sc.cases():
        ref_c, ref_b, _, ref_n = sc.reference(k)
        c32, b32, _, n32 = sc.score_model(k, np.float32)
        fin = np.isfinite(ref_c)
        assert np.array_equal(np.isfinite(c32), fin) and np.all(c32[~fin] == np.inf), k.name
        assert np.array_equal(np.isfinite(n32), np.isfinite(ref_n)), k.name
        ec = float(np.abs(c32[fin] - ref_c[fin]).max()) if fin.any() else 0.0
        nf = np.isfinite(ref_n)
        en = float(np.abs(n32[nf] - ref_n[nf]).max()) if nf.any() else 0.0
        print('%-10s T=%3d N=%d C=%5d K=%3d max_label_len=%3d slots/lane %d row path %-9s float32 floor: cost %.3e, log_norm %.3e; finite costs %.1f .. %.1f'
              % (k.name, k.T, k.N, k.C, k.K, k.mll, sc.slots_per_lane(k.mll), sc.row_path(k.C), ec, en, ref_c[fin].min(), ref_c[fin].max()))
        assert np.array_equal(b32, ref_b), k.name          # (the float32 model agrees on every arg-min: the margins below are far above its error)
        worst_c, worst_n = max(worst_c, ec), max(worst_n, en)
    print('float32 floor over the cases: cost %.3e, log_norm %.3e' % (worst_c, worst_n))
    # the quoted floor is the measured one within a factor of two and is not exceeded
    assert sc.COST_FLOOR / 2 <= worst_c <= sc.COST_FLOOR, (worst_c, sc.COST_FLOOR)
    assert sc.NORM_FLOOR / 2 <= worst_n <= sc.NORM_FLOOR, (worst_n, sc.NORM_FLOOR)
    assert sc.COST_BOUND == 8 * sc.COST_FLOOR and sc.NORM_BOUND == 8 * sc.NORM_FLOOR


def test_arg_min_is_well_defined():
    """Outside the deliberate duplicates the best candidate of every sample leads the runner-up by more than 2 x COST_BOUND."""
    leads = {k.name: sc.margin(k) for k in sc.cases()}
    print('smallest lead per case: ' + ', '.join('%s %.3g' % v for v in leads.items()))
    for name, lead in leads.items():
        assert lead > 2 * sc.COST_BOUND, (name, lead)


def test_cases_are_the_intended_edges():
    by = {k.name: k for k in sc.cases()}
    assert list(by) == (['lane31', 'lane32', 'lane63', 'lane64', 'lane127', 'lane128', 'L255', 'repeats', 'brute', 'brute_last'] +
                        ['K%d' % K for K in sc.GRID_K] + ['C%d' % C for C in sc.ROW_PATH_CLASSES] + ['bad', 'dups', 'saturated'])
    for k in sc.cases():
        assert sc.supported(k.C, k.T, k.mll, k.K) and k.acts.nbytes <= 8 << 20, k.name
        lab, lens = k.packed()
        assert lab.shape == (k.K, k.mll) and lab.dtype == np.int32 and lens.dtype == np.int32
        for j in range(k.K):          # padding words: -1 and C + 7
            assert set(lab[j, max(int(lens[j]), 0):].tolist()) <= {-1, k.C + 7}, (k.name, j)
    # lane boundaries
    assert [(by[n].T, by[n].N, by[n].C, by[n].mll, sc.slots_per_lane(by[n].mll)) for n in ('lane31', 'lane32', 'lane63', 'lane64', 'lane127', 'lane128')] == \
        [(72, 2, 40, 31, 1), (72, 2, 40, 32, 2), (140, 2, 40, 63, 2), (140, 2, 40, 64, 4), (264, 2, 40, 127, 4), (264, 2, 40, 128, 8)]
    assert sorted(by['lane32'].lens.tolist()) == [0, 1, 9, 31, 32] and {63, 64} <= set(by['lane64'].lens.tolist()) and {127, 128} <= set(by['lane128'].lens.tolist())
    L = by['L255']
    assert (L.T, L.N, L.C, L.mll) == (520, 1, 24, 255) and L.lens.tolist().count(255) == 1 and sc.slots_per_lane(255) == 8
    # repeats
    r = by['repeats']
    assert (r.T, r.C, r.il.tolist()) == (8, 6, [8, 5, 4, 1, 0])
    assert r.lexicon[:5] == [[1, 1], [1, 1, 1], [1, 2, 1, 2], [1, 1, 2, 2], [1, 1, 2, 2, 1, 2]]
    rc, rb, _, rn = sc.reference(r)
    assert len(r.lexicon[4]) + lc.repeats(r.lexicon[4]) == 8 and np.isfinite(rc[0, 4]) and rc[1, 4] == np.inf          # exactly feasible at Tn = 8
    assert len(r.lexicon[1]) + lc.repeats(r.lexicon[1]) == 5 and np.isfinite(rc[1, 1]) and rc[2, 1] == np.inf          # at Tn = 5, not at Tn - 1
    assert np.isfinite(rc[3]).tolist() == [False, False, False, False, False, True, True, False]                       # Tn = 1: '' and one character
    assert np.all(rc[4] == np.inf) and rb[4] == -1 and rn[4] == -np.inf                                               # Tn = 0: nothing is feasible
    # grid edges, blank positions, row paths
    assert [by['K%d' % K].K for K in sc.GRID_K] == [1, 3, 4, 5, 257] and all(by['K%d' % K].N == 3 for K in sc.GRID_K)
    assert by['K1'].mll == 0 and by['K1'].lexicon == [[]]
    assert {k.blank for k in sc.cases()} >= {0} and sum(k.blank == k.C - 1 for k in sc.cases()) >= 4
    assert {sc.row_path(C) for C in sc.ROW_PATH_CLASSES} == {(64, 1), (64, 8), (64, 4), (256, 4), (512, 4), (1024, 8)}
    assert [sc.row_path(C) for C in (37, 38, 40, 1024, 1028, 4100, 8200, 16384)] == [(64, 1), (64, 1), (64, 8), (64, 8), (256, 4), (512, 4), (1024, 8), (1024, 8)]
    for C in sc.ROW_PATH_CLASSES:
        k = by['C%d' % C]
        assert (k.T, k.N, k.K) == (6, 2, 5) and ({0, C - 2} if k.blank else {1, C - 1}) <= set(k.lexicon[0])
    # bad labels and lengths: +inf for every sample; the good ones stay finite
    b = by['bad']
    bc = sc.reference(b)[0]
    assert 12 in b.lexicon[1] and -1 in b.lexicon[2] and b.blank in b.lexicon[3] and b.lens.tolist()[-2:] == [-1, 4] and b.mll == 3
    assert np.isfinite(bc).all(axis=0).tolist() == [True, False, False, False, True, False, False, False, False]
    assert np.isinf(bc[:, [1, 2, 3, 5, 6, 7, 8]]).all()
    # duplicates: index 9 repeats index 2, which is sample 0's best
    d = by['dups']
    assert d.lexicon[9] == d.lexicon[2] and sc.reference(d)[1][0] == 2 and np.array_equal(sc.reference(d)[0][:, 9], sc.reference(d)[0][:, 2])
    # saturated frames
    s = by['saturated']
    assert s.acts[3].max() == 80.0 and s.acts[5].min() == -80.0
    # per-sample lexicons are permutations of the shared one
    for name in sc.PER_SAMPLE_CASES:
        k = by[name]
        lab, lens, perm = k.per_sample()
        assert lab.shape == (k.N, k.K, k.mll) and lens.shape == (k.N, k.K)
        assert all(sorted(perm[n].tolist()) == list(range(k.K)) for n in range(k.N)) and len({tuple(p) for p in perm.tolist()}) == k.N
        assert np.array_equal(lab[1, 0], k.packed()[0][perm[1, 0]])


def test_host_arithmetic_is_the_librarys():
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    grid = [(C, T, L, K) for C in (0, 1, 40, 16384, 16385) for T in (0, 1, 63) for L in (-1, 0, 255, 256) for K in (0, 1, 65536, 65537)]
    for C, T, L, K in grid:
        assert bool(lib.ocr_ctc_score_supported(C, T, L, K)) == sc.supported(C, T, L, K), (C, T, L, K)
    assert [lib.ocr_ctc_score_supported(6625, 63, 25, K) for K in (0, 65536, 65537)] == [0, 1, 0]
    assert [lib.ocr_ctc_score_supported(6625, 63, L, 1024) for L in (255, 256)] == [1, 0]
    assert [lib.ocr_ctc_score_supported(C, 63, 25, 1024) for C in (16384, 16385)] == [1, 0]
    assert lib.ocr_ctc_score_supported(6625, 0, 25, 1024) == 0
    sz = ctypes.c_size_t(0)
    for k in sc.cases():
        assert lib.ocr_ctc_score_workspace_size(k.C, k.T, k.N, ctypes.byref(sz)) == 0, k.name
        assert sz.value == sc.workspace_bytes(k.C, k.T, k.N) and sz.value % 256 == 0 and sz.value >= 4 * k.T * k.N, k.name
    assert lib.ocr_ctc_score_workspace_size(6625, 63, 64, ctypes.byref(sz)) == 0 and sz.value == 16128 == sc.workspace_bytes(6625, 63, 64)
    for C, T, N in [(16385, 63, 4), (0, 63, 4), (40, 0, 4), (40, 63, 0), (40, 63, -1)]:
        assert sc.workspace_bytes(C, T, N) is None and lib.ocr_ctc_score_workspace_size(C, T, N, ctypes.byref(sz)) == 2, (C, T, N)
    assert lib.ocr_ctc_score_workspace_size(40, 63, 4, None) == 2
    assert lib.ocr_abi_version() == 1


def test_refusals_come_before_any_launch():
    """OCR_ERR_INVALID (2) for a NULL required operand, partly NULL optional outputs, a blank outside [0, C), a sample stride other than 0 or K, a
    short workspace and every shape ocr_ctc_score_supported refuses: host memory stands in for the operands, nothing reads it."""
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(acts=p, il=p, labels=p, lens=p, stride=0, C=40, N=4, T=63, K=16, L=8, blank=0, costs=p, best=p, best_cost=p, norm=p, ws=p, ws_bytes=1024)

    def status(**kw):
        v = dict(good, **kw)
        return lib.ocr_ctc_score(v['acts'], v['il'], v['labels'], v['lens'], v['stride'], v['C'], v['N'], v['T'], v['K'], v['L'], v['blank'], v['costs'],
                                 v['best'], v['best_cost'], v['norm'], v['ws'], v['ws_bytes'], None)
    assert sc.workspace_bytes(40, 63, 4) == 1024
    for operand in ('acts', 'il', 'labels', 'lens', 'costs', 'ws'):
        assert status(**{operand: None}) == 2, operand
    assert status(best=None) == 2 and status(best_cost=None, norm=None) == 2
    assert status(blank=-1) == 2 and status(blank=40) == 2
    assert status(stride=1) == 2 and status(stride=15) == 2 and status(stride=-16) == 2
    assert status(ws_bytes=1023) == 2
    assert status(K=0) == 2 and status(K=65537) == 2 and status(L=-1) == 2 and status(L=256) == 2 and status(C=16385, blank=0) == 2 and status(C=0) == 2
    assert status(T=0) == 2 and status(N=0) == 2 and status(N=65536, ws_bytes=1 << 30) == 2


def test_header_declares_the_entry_points():
    from lstm_ctc_ocr_amd import _native as nat
    declared = nat.declared_symbols()
    for name in ('ocr_ctc_score_supported', 'ocr_ctc_score_workspace_size', 'ocr_ctc_score'):
        assert name in declared and name in nat._SIGS and hasattr(nat.lib(), name), name
    assert len(nat._SIGS['ocr_ctc_score'][0]) == 18


def test_lexicon_decode_needs_a_lexicon():
    """The check precedes every use of the engine's state, so it is made on an Engine that was never initialised (building one needs a GPU);
    the other methods keep their defaults."""
    from lstm_ctc_ocr_amd.engine import Engine
    eng = object.__new__(Engine)
    with pytest.raises(ValueError):
        eng.decode(None, None, method='lexicon')
    with pytest.raises(ValueError):
        eng.decode(None, None, method='lexicon', lexicon=None)
    sig = inspect.signature(Engine.decode)
    assert [(n, p.default) for n, p in sig.parameters.items()][3:] == [('method', 'beam'), ('beam_width', 100), ('lexicon', None)]
    assert list(inspect.signature(Engine.score).parameters) == ['self', 'data', 'seq_len', 'lexicon', 'blank']
