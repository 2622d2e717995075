"""The device edit distance checked on the CPU (tests/edit_distance_cases.py): the textbook table on known answers; the kernel's recursion, lane by
lane and vectorised over pairs, against the textbook on random pairs; the `ignore` rule and the three "no string" rules; the MBR model on its
known answer and the majority property; ocr_edit_distance_supported against its restatement; the refusals of the three entries before any
launch; the declarations; the ops' shape checks and the Engine's new methods beside its unchanged ones."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_distance_cases as ed  # noqa: E402

S = lambda w: [ord(c) for c in w]


def test_textbook_known_answers():
    assert ed.textbook(S('kitten'), S('sitting')) == 3
    assert ed.textbook([], S('x')) == 1 and ed.textbook(S('x'), []) == 1 and ed.textbook([], []) == 0
    assert ed.textbook(S('saturday'), S('sunday')) == 3 and ed.textbook(S('abc'), S('abc')) == 0
    rng = np.random.RandomState(0)
    for La, Lb in ((0, 5), (5, 0), (3, 9), (9, 3), (7, 7)):
        a, b = [int(v) for v in rng.randint(1, 9, La)], [int(v) for v in rng.randint(11, 19, Lb)]
        assert ed.textbook(a, b) == max(La, Lb)                             # disjoint alphabets
        assert ed.textbook(a, a) == 0


def _random_pairs(rng, count, Lmax_a, Lmax_b):
    out = []
    for _ in range(count):
        C = (2, 3, 40)[rng.randint(3)]
        a = [int(v) for v in rng.randint(1, C + 1, rng.randint(Lmax_a + 1))]
        b = [int(v) for v in rng.randint(1, C + 1, rng.randint(Lmax_b + 1))]
        if rng.randint(4) == 0 and a:
            b = ed.derive('one_edit', a, C, rng, 0)[:Lmax_b]
        out.append((a, b))
    return out


def test_pairs_model_against_the_textbook():
    rng = np.random.RandomState(1)
    pairs = _random_pairs(rng, 600, 40, 40) + _random_pairs(rng, 40, 100, 90) + [([], []), ([1], []), ([], [1]), ([1] * 70, [1] * 20)]
    got = ed.pairs_model([a for a, _ in pairs], [b for _, b in pairs])
    want = [ed.textbook(a, b) for a, b in pairs]
    assert got.tolist() == want
    assert ed.pairs_model([S('kitten')], [S('sitting')]).tolist() == [3]


@pytest.mark.parametrize('CPL,W,La,Lb', [(1, 16, 15, 15), (1, 64, 40, 63), (4, 64, 30, 255)])
def test_lane_model_against_the_textbook(CPL, W, La, Lb):
    """The kernel's three instances lane by lane: segments of a wave advancing together with rows beyond a segment's own La masked, the
    columns beyond Lb computing values nobody reads, the scan's fills."""
    rng = np.random.RandomState(CPL * 100 + W)
    for rep in range(25 if W == 16 else 8):
        pairs = _random_pairs(rng, 64 // W, La, Lb)
        if rep == 0:
            pairs[0] = ([1] * La, [1 + (k % 2) for k in range(Lb)])          # the longest of both
        if rep == 1:
            pairs[-1] = ([], [2] * Lb)
        assert ed.lane_model(pairs, CPL, W) == [ed.textbook(a, b) for a, b in pairs], (CPL, W, rep)


def test_ignore_and_no_string_rules():
    row = np.array([5, 0, 6, 0, 0, 7, 9, 9], np.int32)
    assert ed.string_of(row, 6, 8) == [5, 0, 6, 0, 0, 7] and ed.string_of(row, 6, 8, ignore=0) == [5, 6, 7]
    assert ed.string_of(row, 0, 8) == [] and ed.string_of(row, 8, 8, ignore=9) == [5, 0, 6, 0, 0, 7]
    assert ed.string_of(row, -1, 8) is None and ed.string_of(row, 9, 8) is None                      # below 0, above the pitch
    long = np.ones(600, np.int32)
    long[::2] = 0
    assert ed.string_of(long, 256, 600) is None and len(ed.string_of(long, 255, 600)) == 255          # 256 counted characters
    assert len(ed.string_of(long, 510, 600, ignore=0)) == 255 and ed.string_of(long, 512, 600, ignore=0) is None
    # the entry's model: -1 for exactly the pairs of a "no string", the counts
    a = np.array([[[1, 2, 3, 0], [1, 2, 0, 0]]], np.int32)
    b = np.array([[[1, 0, 3, 0], [4, 4, 4, 4], [1, 2, 3, 9]]], np.int32)
    dist, ac, bc = ed.distance_model(a, np.array([[4, -1]], np.int32), b, np.array([[3, 5, 4]], np.int32), ignore=0)
    assert dist.tolist() == [[[1, -1, 1], [-1, -1, -1]]] and ac.tolist() == [[3, -1]] and bc.tolist() == [[2, -1, 4]]
    dist, ac, bc = ed.distance_model(a, np.array([[4, 2]], np.int32), b[0], np.array([3, 4, 4], np.int32), shared_b=True)
    assert dist.tolist() == [[[2, 4, 1], [2, 4, 2]]] and ac.tolist() == [[4, 2]] and bc.tolist() == [3, 4, 4]
    d2, c2 = ed.self_model(b, np.array([[3, 5, 4]], np.int32), ignore=0)
    assert d2.tolist() == [[[0, -1, 2], [-1, -1, -1], [2, -1, 0]]] and c2.tolist() == [[2, -1, 4]]
    assert ed.stats_model(dist, np.broadcast_to(np.array([3, 4, 4]), (1, 2, 3))) == [15, 22, 0, 6]
    assert ed.stats_model([0, -1, 3, 0], [4, 100, 2, 0]) == [3, 6, 2, 3]


def test_self_cases_cover_the_grid():
    for C in ed.ALPHABETS:
        s, s_len, ignore = ed.self_case(C)
        assert s.shape == (3, 100, 520) and ignore == 0 and s_len.max() > 255 and s_len.max() <= 520
        counted = [[len(ed.string_of(s[n, k], s_len[n, k], 520, 0) or []) for k in range(100)] for n in range(3)]
        for n in range(3):
            assert set(ed.LENGTHS + ed.OWN_EDGES) <= set(counted[n]), (C, n)          # so every pair of lengths occurs among the 100 x 100 pairs
        assert all(ed.string_of(s[n, k], s_len[n, k], 520, 0) is not None for n in range(3) for k in range(100))
        syms = set(int(v) for n in range(3) for k in range(0, 100, 2) for v in s[n, k, :s_len[n, k]]) - {0}
        assert max(syms) <= 2 * C and (C > 40 or set(range(1, C + 1)) <= syms)


def test_mbr_known_answer_and_majority():
    cands, dist, costs = ed.mbr_known()
    assert dist[0].tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]]
    risk, best, best_risk = ed.mbr_model(dist, costs)
    assert np.allclose(risk[0], [1.20, 1.05, 1.15], atol=1e-6) and best.tolist() == [1] and abs(best_risk[0] - 1.05) < 1e-6
    assert int(np.argmin(costs[0])) == 0                                    # the MAP choice differs
    # one candidate above half of the posterior is the MBR choice: risk(y) - risk(top) >= d(y, top) * (2 p_top - 1)
    rng = np.random.RandomState(5)
    for rep in range(40):
        K = int(rng.randint(2, 9))
        strs = [[int(v) for v in rng.randint(1, 4, rng.randint(0, 8))] for _ in range(K)]
        strs = [list(x) for x in dict.fromkeys(tuple(x) for x in strs)]
        K = len(strs)
        d = np.array([[[ed.textbook(x, y) for y in strs] for x in strs]], np.int32)
        p = rng.rand(K) * 0.4
        top = int(rng.randint(K))
        p[top] = 0.0
        p = p / max(p.sum(), 1e-9) * (0.49 - 0.4 * rng.rand())
        p[top] = 1.0 - p.sum()
        assert p[top] > 0.5
        costs = (-np.log(np.maximum(p, 1e-30))).astype(np.float32)[None, :]
        assert ed.mbr_model(d, costs)[1].tolist() == [top]
    # the order (risk, cost, index), invalid candidates, nobody valid
    d, costs = ed.mbr_random(4, 6, 3)
    risk, best, best_risk = ed.mbr_model(d, costs)
    valid = ed.mbr_valid(d, costs)
    assert best[3] == -1 and best_risk[3] == np.inf and best[2] == -1 and np.all(risk[~valid] == np.inf) and np.all(np.isfinite(risk[valid]))
    tie = np.array([[[0, 1], [1, 0]]], np.int32)
    assert ed.mbr_model(tie, np.array([[2.0, 2.0]], np.float32))[1].tolist() == [0]
    assert ed.mbr_model(tie, np.array([[2.0, 1.0]], np.float32))[1].tolist() == [1]


def test_trained_fixture_figures():
    """What Engine.evaluate must return on the trained fixture (tests/test_gpu_edit_distance.py), from the oracle's strings in
    tests/golden/trained_expect.npz: exact / edits / ref_chars, greedy and beam alike; V0's 29 edits are its one infeasible sample."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_trained_fixture as fx
    d, e = np.load(fx.BATCHES), np.load(fx.EXPECT)
    for name, want in (('C1', (8, 0, 32)), ('V0', (63, 29, 476))):
        truth, pos = [], 0
        for n in d[name + '/label_len']:
            truth.append(d[name + '/labels'][pos:pos + n].tolist())
            pos += n
        for decoder in ('greedy', 'beam'):
            strings = [[int(v) for v in r if v != 0] for r in e[name + '/' + decoder]]
            dist = ed.pairs_model(strings, truth)
            assert dist.tolist() == [ed.textbook(g, t) for g, t in zip(strings, truth)]
            assert (int((dist == 0).sum()), int(dist.sum()), sum(len(t) for t in truth)) == want, (name, decoder)
        if name == 'V0':
            k = int(np.argmin(d['V0/seq_len']))
            assert dist[k] == 29 and dist.sum() == 29


# ---------------------------------------------------------------- the entry points on the host
def test_supported_matches_its_restatement_and_the_names_are_declared():
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    lib = nat.lib()
    declared = nat.declared_symbols()
    for name, nargs in (('ocr_edit_distance_supported', 3), ('ocr_edit_distance', 16), ('ocr_edit_stats', 5), ('ocr_mbr_select', 8)):
        assert name in declared and name in nat._SIGS and hasattr(lib, name), name
        assert len(nat._SIGS[name][0]) == nargs
    for N in (0, 1, 3, 64, 65535, 65536):
        for Ka in (0, 1, 100, 128, 16384, 65536, 65537):
            for Kb in (0, 1, 100, 127, 16384, 65536, 65537):
                assert bool(lib.ocr_edit_distance_supported(Ka, Kb, N)) == ed.supported(Ka, Kb, N) == ops.edit_distance_supported(Ka, Kb, N), (Ka, Kb, N)
    assert lib.ocr_edit_distance_supported(32768, 32768, 1) == 1 and lib.ocr_edit_distance_supported(32768, 32769, 1) == 0
    assert lib.ocr_edit_distance_supported(128, 128, 65535) == 1 and lib.ocr_edit_distance_supported(129, 128, 65535) == 0


def test_refusals_come_before_any_launch():
    """OCR_ERR_INVALID (2) for NULL and out-of-limit arguments: host memory stands in for the operands, nothing reads it."""
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(a=p, a_len=p, a_ld=8, a_sn=40, Ka=5, b=p, b_len=p, b_ld=8, b_sn=0, Kb=3, N=4, ignore=0, dist=p, ac=p, bc=p)

    def status(**kw):
        v = dict(good, **kw)
        return lib.ocr_edit_distance(v['a'], v['a_len'], v['a_ld'], v['a_sn'], v['Ka'], v['b'], v['b_len'], v['b_ld'], v['b_sn'], v['Kb'], v['N'],
                                     v['ignore'], v['dist'], v['ac'], v['bc'], None)
    for operand in ('a', 'a_len', 'b', 'b_len', 'dist'):
        assert status(**{operand: None}) == 2, operand
    for name, value in (('N', 0), ('N', 65536), ('N', -1), ('Ka', 0), ('Ka', 65537), ('Kb', 0), ('Kb', 65537), ('a_ld', -1), ('b_ld', -1),
                        ('a_sn', -1), ('b_sn', -8)):
        assert status(**{name: value}) == 2, (name, value)
    assert status(Ka=32768, Kb=32768, N=2) == 2                             # 2^31 pairs
    assert status(a=ctypes.c_void_p(p.value + 2)) == 2 and status(dist=ctypes.c_void_p(p.value + 1)) == 2
    assert lib.ocr_edit_stats(None, p, 8, p, None) == 2 and lib.ocr_edit_stats(p, None, 8, p, None) == 2 and lib.ocr_edit_stats(p, p, 8, None, None) == 2
    assert lib.ocr_edit_stats(p, p, 0, p, None) == 2 and lib.ocr_edit_stats(p, p, -5, p, None) == 2 and lib.ocr_edit_stats(p, p, (1 << 30) + 1, p, None) == 2
    assert lib.ocr_edit_stats(p, p, 8, ctypes.c_void_p(p.value + 4), None) == 2
    mbr = dict(dist=p, costs=p, N=2, K=5, risk=p, best=p, best_risk=p)

    def mstatus(**kw):
        v = dict(mbr, **kw)
        return lib.ocr_mbr_select(v['dist'], v['costs'], v['N'], v['K'], v['risk'], v['best'], v['best_risk'], None)
    for operand in ('dist', 'costs', 'risk', 'best', 'best_risk'):
        assert mstatus(**{operand: None}) == 2, operand
    assert mstatus(K=0) == 2 and mstatus(K=129) == 2 and mstatus(N=0) == 2 and mstatus(N=65536) == 2


def test_ops_check_shapes_on_the_host():
    import torch
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    with pytest.raises(nat.NativeError):
        ops.edit_distance(i32(2, 8), i32(2), i32(2, 8), i32(2))            # CPU tensors: there is no fallback
    with pytest.raises(nat.NativeError):
        ops.edit_stats(i32(4), i32(4))
    with pytest.raises(nat.NativeError):
        ops.mbr_select(i32(2, 3, 3), torch.zeros(2, 3))
    for bad in (lambda: ops.edit_distance(i32(2, 8).long(), i32(2), i32(2, 8), i32(2)),            # dtype
                lambda: ops.edit_distance(i32(2, 8), i32(3), i32(2, 8), i32(2)),                   # lengths of another shape
                lambda: ops.edit_distance(i32(2, 8), i32(2), i32(3, 8), i32(3)),                   # sample counts differ
                lambda: ops.edit_distance(i32(2, 4, 8), i32(2, 4), i32(4, 8), i32(4)),             # a [K, L] list is not shared unless said so
                lambda: ops.edit_distance(i32(2, 8, 4).transpose(1, 2), i32(2, 4), i32(2, 8), i32(2)),          # last dimension strided
                lambda: ops.edit_distance(i32(2, 4, 8), i32(2, 4), i32(2, 4, 8), i32(2, 4), shared_b=True),
                lambda: ops.edit_distance(i32(1, 4, 8).expand(3, 4, 8), i32(3, 4), i32(3, 8), i32(3)),          # stride 0 without shared_a
                lambda: ops.edit_stats(i32(4), i32(5)), lambda: ops.edit_stats(i32(4).float(), i32(4)),
                lambda: ops.mbr_select(i32(2, 3, 4), torch.zeros(2, 3)), lambda: ops.mbr_select(i32(2, 3, 3), torch.zeros(2, 4)),
                lambda: ops.mbr_select(i32(2, 129, 129), torch.zeros(2, 129)), lambda: ops.mbr_select(i32(2, 3, 3), torch.zeros(2, 3).double())):
        with pytest.raises(ValueError):
            bad()
    assert ops.edit_distance_supported(100, 100, 64) and not ops.edit_distance_supported(65537, 1, 1)


def test_engine_has_the_new_methods_and_keeps_its_signatures():
    import inspect
    from lstm_ctc_ocr_amd.engine import Engine
    params = lambda f: [(n, q.default) for n, q in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert params(Engine.evaluate)[1:] == [('data', E), ('seq_len', E), ('labels', E), ('method', 'beam'), ('beam_width', 100), ('per_sample', False)]
    assert params(Engine.decode_mbr)[1:] == [('data', E), ('seq_len', E), ('candidates', 16), ('beam_width', 100)]
    assert params(Engine.decode)[3:] == [('method', 'beam'), ('beam_width', 100), ('lexicon', None)]
    assert params(Engine.decode_nbest_beam)[3:] == [('k', 5), ('beam_width', 100), ('candidates', None), ('rescore', True)]
    eng = object.__new__(Engine)
    x = np.zeros((2, 8, 4), np.float32)
    with pytest.raises(ValueError):
        eng.evaluate(x, None, [[1], [2]], method='lexicon')                 # before any use of the engine's state
    with pytest.raises(ValueError):
        eng.evaluate(x, None, [[1]])
    for kw in (dict(candidates=0), dict(candidates=17, beam_width=16), dict(candidates=16, beam_width=129)):
        with pytest.raises(ValueError):
            eng.decode_mbr(x, None, **kw)
