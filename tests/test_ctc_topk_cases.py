"""The k best of a lexicon checked on the CPU (tests/ctc_topk_cases.py): the numpy model against a plain Python sorted() on tiny rows, the model
telling three deliberately wrong variants apart (unstable tie order, +inf returned as a hit, zeros ordered by their bits), the invariants of
ocr_ctc_topk_supported / _plan / _workspace_size against their restatement, the refusals of ocr_ctc_topk before any launch, the declarations,
and the Engine's new methods beside its unchanged ones."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_topk_cases as tk  # noqa: E402


def _bits(v):
    return struct.unpack('<i', struct.pack('<f', float(v)))[0]


def sorted_reference(costs, k, log_norm=None):
    """The contract in plain Python: finite entries, sorted by (cost, index) with Python's float comparison (-0.0 == 0.0), the first k."""
    out = []
    for n, row in enumerate(costs.tolist()):
        hits = sorted((i for i in range(len(row)) if row[i] != float('inf')), key=lambda i: (row[i], i))[:k]
        out.append([(i, _bits(row[i])) for i in hits])
    return out


def as_pairs(index, cost, count):
    return [[(int(index[n, j]), _bits(cost[n, j])) for j in range(int(count[n]))] for n in range(index.shape[0])]


TINY = [(regime, N, K, k) for regime in tk.REGIMES for N in (1, 3) for K in (1, 2, 5, 9, 65) for k in (1, 2, 5, 64)]


def test_model_against_python_sorted():
    for seed, (regime, N, K, k) in enumerate(TINY):
        c = tk.make_rows(regime, N, K, k, seed)
        ln = np.linspace(-3.0, 2.0, N).astype(np.float32)
        index, cost, post, count = tk.topk_model(c, k, ln)
        assert index.dtype == np.int32 and cost.dtype == np.float32 and post.dtype == np.float32 and count.dtype == np.int32
        assert as_pairs(index, cost, count) == sorted_reference(c, k), (regime, N, K, k)
        for n in range(N):
            m = int(count[n])
            assert m == min(k, int(np.isfinite(c[n]).sum()))
            assert np.all(index[n, m:] == -1) and np.all(cost[n, m:] == np.inf) and np.all(post[n, m:] == -np.inf)
            assert tk.same_bits(post[n, :m], (-cost[n, :m]) - ln[n])
        assert tk.topk_model(c, k)[2] is None


def test_model_covers_what_the_regimes_claim():
    c = tk.make_rows('zeros', 3, 257, 5, 3)
    index, cost, _, count = tk.topk_model(c, 5)
    signs = np.signbit(cost)
    assert np.all(cost == 0) and signs.any(axis=1).all() and (~signs).any(axis=1).all()          # both zeros among the winners of every row
    assert np.all(np.diff(index, axis=1) > 0)                                                    # equal under the order: by index
    for regime, want in (('finite_k-1', 4), ('finite_k', 5), ('finite_k+1', 5)):
        assert tk.topk_model(tk.make_rows(regime, 3, 257, 5, 4), 5)[3].tolist() == [want] * 3
    assert tk.topk_model(tk.make_rows('last_only', 3, 257, 5, 5), 5)[0][:, 0].tolist() == [256] * 3
    assert tk.topk_model(tk.make_rows('all_inf', 3, 257, 5, 6), 5)[3].tolist() == [0] * 3
    assert len(np.unique(tk.make_rows('ties8', 1, 4097, 5, 7))) == 8
    c = tk.segment_edge_rows()
    segments, seg_len = tk.plan(2, 1 << 20, 64)
    index, cost, _, count = tk.topk_model(c, 64)
    assert count.tolist() == [64, 64]
    for n in range(2):
        at = np.sort(index[n])
        assert np.all((at[0::2] + 1) % seg_len == 0) and np.all(at[1::2] % seg_len == 0) and np.all(at[1::2] == at[0::2] + 1)
        assert int((cost[n] == np.float32(-1.25)).sum()) == 32


# ---------------------------------------------------------------- the model rejects wrong variants
def _variant(costs, k, kind):
    """A wrong selection: 'unstable' breaks ties by the HIGHER index, 'inf_hit' returns +inf entries, 'zero_bits' orders -0.0 before +0.0."""
    N, K = costs.shape
    index = np.full((N, k), -1, np.int32)
    cost = np.full((N, k), np.inf, np.float32)
    count = np.zeros(N, np.int32)
    for n in range(N):
        row = costs[n]
        if kind == 'unstable':
            order = np.lexsort((-np.arange(K), row))
            order = order[row[order] != np.inf]
        elif kind == 'inf_hit':
            order = np.lexsort((np.arange(K), row))
        else:
            order = np.lexsort((np.arange(K), np.signbit(row) == 0, row))
            order = order[row[order] != np.inf]
        order = order[:k]
        index[n, :len(order)], cost[n, :len(order)], count[n] = order, row[order], len(order)
    return index, cost, count


@pytest.mark.parametrize('kind,regime', [('unstable', 'ties8'), ('unstable', 'equal'), ('inf_hit', 'finite_k-1'), ('inf_hit', 'all_inf'),
                                         ('zero_bits', 'zeros')])
def test_model_rejects_wrong_variants(kind, regime):
    c = tk.make_rows(regime, 3, 65, 5, 11)
    if kind == 'zero_bits':
        c[:, 0], c[:, 1] = 0.0, -0.0                         # a +0.0 in front of a -0.0: equal, so the lower index leads
    index, cost, _, count = tk.topk_model(c, 5)
    vi, vc, vn = _variant(c, 5, kind)
    assert not (np.array_equal(index, vi) and tk.same_bits(cost, vc) and np.array_equal(count, vn)), (kind, regime)
    # and the variant with the mistake taken out is the model
    if kind == 'unstable':
        assert np.array_equal(np.sort(cost, axis=1), np.sort(vc, axis=1))          # the same values, other entries


# ---------------------------------------------------------------- host arithmetic
def test_supported_plan_and_workspace_invariants():
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    lib = nat.lib()
    declared = nat.declared_symbols()
    for name in ('ocr_ctc_topk_supported', 'ocr_ctc_topk_plan', 'ocr_ctc_topk_workspace_size', 'ocr_ctc_topk'):
        assert name in declared and name in nat._SIGS and hasattr(lib, name), name
    assert len(nat._SIGS['ocr_ctc_topk'][0]) == 13
    for K in (0, 1, 64, 8192, 8193, 1 << 20, (1 << 20) + 1):
        for k in (0, 1, 5, 64, 65):
            assert bool(lib.ocr_ctc_topk_supported(K, k)) == tk.supported(K, k), (K, k)
    assert lib.ocr_ctc_topk_supported(1 << 20, 64) == 1
    for K, k in ((1024, 0), (1024, 65), (0, 5), ((1 << 20) + 1, 5)):          # the limits
        assert lib.ocr_ctc_topk_supported(K, k) == 0
        with pytest.raises(ValueError):
            ops.ctc_topk_plan(4, K, k)
        with pytest.raises(ValueError):
            ops.ctc_topk_workspace_bytes(4, K, k)
    seg, seg_len, sz = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    for N in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 1023, 1024, 1025, 65535):
        for K in (1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 12289, 65536, 100000, (1 << 20) - 1, 1 << 20):
            for k in (1, 5, 64):
                assert lib.ocr_ctc_topk_plan(N, K, k, ctypes.byref(seg), ctypes.byref(seg_len)) == 0
                s, sl = seg.value, seg_len.value
                assert (s, sl) == tk.plan(N, K, k) == ops.ctc_topk_plan(N, K, k), (N, K, k)
                assert s >= 1 and s * sl >= K > (s - 1) * sl and sl % tk.ROUND == 0                # covers the row, no empty segment
                assert s <= 256 and s * k <= 256 * 64                                              # what the merge launch reads per sample
                if K <= tk.ONE_WG or N >= tk.TARGET_WGS:
                    assert s == 1, (N, K, k)                                                       # one workgroup a row suffices
                else:
                    assert s >= 2 and (N * s >= 256 or sl == tk.ROUND), (N, K, k)                  # the chip is covered, or the cut is the finest
                assert lib.ocr_ctc_topk_workspace_size(N, K, k, ctypes.byref(sz)) == 0
                assert sz.value == tk.workspace_bytes(N, K, k) == ops.ctc_topk_workspace_bytes(N, K, k)
                assert sz.value == (0 if s == 1 else -(-N * s * k * 8 // 256) * 256)
    assert tk.plan(1, 1 << 20, 5) == (256, 4096) and tk.plan(64, 1 << 20, 5) == (16, 65536) and tk.plan(64, 65536, 5) == (16, 4096)
    for N, K, k in ((0, 64, 5), (65536, 64, 5), (4, 0, 5), (4, (1 << 20) + 1, 5), (4, 64, 0), (4, 64, 65)):
        assert lib.ocr_ctc_topk_plan(N, K, k, ctypes.byref(seg), ctypes.byref(seg_len)) == 2
        assert lib.ocr_ctc_topk_workspace_size(N, K, k, ctypes.byref(sz)) == 2
        assert tk.plan(N, K, k) is None and tk.workspace_bytes(N, K, k) is None
    assert lib.ocr_ctc_topk_plan(4, 64, 5, None, ctypes.byref(seg_len)) == 2 and lib.ocr_ctc_topk_plan(4, 64, 5, ctypes.byref(seg), None) == 2
    assert lib.ocr_ctc_topk_workspace_size(4, 64, 5, None) == 2


def test_refusals_come_before_any_launch():
    """OCR_ERR_INVALID (2) for NULL and out-of-range arguments: host memory stands in for the operands, nothing reads it."""
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(costs=p, ld=20000, N=4, K=20000, k=5, norm=p, index=p, cost=p, post=p, count=p, ws=p, ws_bytes=tk.workspace_bytes(4, 20000, 5))

    def status(**kw):
        v = dict(good, **kw)
        return lib.ocr_ctc_topk(v['costs'], v['ld'], v['N'], v['K'], v['k'], v['norm'], v['index'], v['cost'], v['post'], v['count'], v['ws'],
                                v['ws_bytes'], None)
    assert tk.plan(4, 20000, 5)[0] > 1 and good['ws_bytes'] > 0
    for operand in ('costs', 'index', 'cost', 'count', 'ws'):
        assert status(**{operand: None}) == 2, operand
    assert status(norm=None) == 2                                      # log_post without log_norm
    assert status(ld=19999) == 2 and status(ws_bytes=good['ws_bytes'] - 1) == 2
    assert status(ws=ctypes.c_void_p(p.value + 4)) == 2               # the keys are 64-bit words
    assert status(costs=ctypes.c_void_p(p.value + 2)) == 2
    assert status(k=0) == 2 and status(k=65) == 2 and status(K=0, ld=8) == 2 and status(K=(1 << 20) + 1, ld=1 << 21, ws_bytes=1 << 30) == 2
    assert status(N=0) == 2 and status(N=65536, ws_bytes=1 << 30) == 2 and status(N=-1) == 2


def test_ops_entry_refuses_on_the_host():
    import torch
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    with pytest.raises(nat.NativeError):
        ops.ctc_topk(torch.zeros(2, 8), 3)                            # a CPU tensor: there is no fallback
    assert ops.ctc_topk_supported(1 << 20, 64) and not ops.ctc_topk_supported(1 << 20, 65)


def test_engine_has_the_nbest_methods_and_keeps_its_signatures():
    import inspect
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie
    assert [(n, q.default) for n, q in inspect.signature(Engine.nbest).parameters.items()][3:] == [('lexicon', inspect.Parameter.empty), ('k', 5),
                                                                                                  ('blank', 0)]
    assert [(n, q.default) for n, q in inspect.signature(Engine.decode_nbest).parameters.items()][3:] == [('lexicon', inspect.Parameter.empty), ('k', 5)]
    assert [(n, q.default) for n, q in inspect.signature(Engine.decode).parameters.items()][3:] == [('method', 'beam'), ('beam_width', 100), ('lexicon', None)]
    eng = object.__new__(Engine)
    trie = LexiconTrie([[1, 2], [3]], 12, blank=11)
    with pytest.raises(ValueError):
        eng.nbest(None, None, trie)                                   # blank 0 against the trie's 11, before any use of the engine's state
    with pytest.raises(ValueError):
        eng.decode_nbest(None, None, trie)
