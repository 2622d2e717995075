"""Lexicon scoring on a prefix tree checked on the CPU (tests/ctc_trie_cases.py): the invariants of the chunked tree ocr_ctc_trie_build writes,
the chunked recursion over the builder's arrays against the per-word float64 reference of tests/ctc_score_cases.py (and its float32 floor
against the bounds quoted there), the refusals of the builder and of ocr_ctc_score_trie, the declarations, and the Engine's blank check."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_trie_cases as tc  # noqa: E402

sc = tc.sc

_DENSE = {}


def dense(name):
    """Dense lexicons for the CPU tests (N = 2, T = 10, C = 12, one input length short): 3 symbols to depth 3 (40 words), 4 to depth 4 (341) and
    the first with a repeated word, a word with a repeated label beyond the dense depth and an invalid one behind it."""
    if not _DENSE:
        _DENSE['a3d3'] = tc.dense_case('a3d3', 3, 3)
        _DENSE['a4d4'] = tc.dense_case('a4d4', 4, 4, seed=501)
        _DENSE['a3d3x'] = tc.dense_case('a3d3x', 3, 3, seed=502, extra=[[2, 1], [1, 1, 2, 2, 3], [1, 0, 2], [3, 3, 3, 3]])
    return _DENSE[name]


def check_invariants(k, trie, chunk_nodes):
    K = k.K
    lab, lens = k.packed()
    assert trie.num_words == K and len(trie) == K
    cns, cws = trie.chunk_node_start, trie.chunk_word_start
    assert cns[0] == 0 and cns[-1] == trie.num_nodes == len(trie.nodes) and cws[0] == 0 and cws[-1] == K
    assert len(cns) == len(cws) == trie.num_chunks + 1 and np.all(np.diff(cws) >= 0)
    sizes = np.diff(cns)
    assert np.all(sizes >= 1) and np.all(sizes <= trie.chunk_nodes), (k.name, chunk_nodes, sizes.max())
    assert chunk_nodes is None or trie.chunk_nodes == chunk_nodes
    # every word once, the sorted ranges contiguous
    assert sorted(trie.word_index.tolist()) == list(range(K))
    label, parent, flag = trie.node_label, trie.node_parent, trie.node_flag
    for ch in range(trie.num_chunks):
        a, b = int(cns[ch]), int(cns[ch + 1])
        assert label[a] == k.blank and parent[a] == 0 and flag[a] == 0                       # node 0 is the root
        loc = np.arange(1, b - a)
        assert np.all(parent[a + 1:b] < loc)                                                  # parent < child
        assert np.all((label[a + 1:b] >= 0) & (label[a + 1:b] < k.C) & (label[a + 1:b] != k.blank))
        plab = label[a + parent[a + 1:b]]
        assert np.array_equal(flag[a + 1:b] == 1, (parent[a + 1:b] > 0) & (label[a + 1:b] != plab))
        # no two nodes of a chunk spell the same prefix
        keys = list(zip(parent[a + 1:b].tolist(), label[a + 1:b].tolist()))
        assert len(set(keys)) == len(keys), (k.name, ch)
    seen = {}
    order = []
    for ch in range(trie.num_chunks):
        for w in range(int(cws[ch]), int(cws[ch + 1])):
            j, v = int(trie.word_index[w]), int(trie.word_node[w])
            if not tc.valid(k, j):
                assert v == -1 and ch == 0, (k.name, j)
                continue
            word = lab[j, :lens[j]].tolist()
            assert 0 <= v < sizes[ch] and tc.spell(trie, ch, v) == word, (k.name, j, word)    # the path spells the word
            assert seen.setdefault((ch, tuple(word)), v) == v                                 # equal words share a node
            order.append(word)
            assert trie[j] == word
    assert order == sorted(order)                                                             # the valid words in lexicographic order
    for a_, b_ in k.dups:
        wa, wb = (int(np.nonzero(trie.word_index == i)[0][0]) for i in (a_, b_))
        assert trie.word_node[wa] == trie.word_node[wb] and np.searchsorted(cws, wa, 'right') == np.searchsorted(cws, wb, 'right')
    if trie.num_chunks == 1:
        prefixes = {tuple(lab[j, :n]) for j in range(K) if tc.valid(k, j) for n in range(1, lens[j] + 1)}
        assert trie.num_nodes == len(prefixes) + 1, (k.name, trie.num_nodes, len(prefixes))


@pytest.mark.parametrize('name', [k.name for k in sc.cases()] + ['a3d3', 'a4d4', 'a3d3x'])
def test_builder_invariants(name):
    k = sc.case(name) if name not in ('a3d3', 'a4d4', 'a3d3x') else dense(name)
    for cn in tc.chunk_sizes(k):
        check_invariants(k, tc.build(k, cn), cn)
    # with one chunk, nodes = distinct prefixes + 1: the capacity holds every case here whole
    from lstm_ctc_ocr_amd.lexicon import chunk_capacity
    trie = tc.build(k, chunk_capacity())
    assert trie.num_chunks == 1
    check_invariants(k, trie, chunk_capacity())
    # padding words (-1, C + 7) and words at or beyond a word's length are never read: other values there give the same tree
    lab, lens = k.packed()
    if lab.size:
        from lstm_ctc_ocr_amd.lexicon import LexiconTrie
        other = lab.copy()
        beyond = np.arange(lab.shape[1])[None, :] >= np.clip(lens, 0, None)[:, None]
        other[beyond] = 1 if k.blank != 1 else 2
        t2 = LexiconTrie((other, lens), k.C, blank=k.blank, chunk_nodes=trie.chunk_nodes)
        for f in ('nodes', 'chunk_node_start', 'chunk_word_start', 'word_node', 'word_index'):
            assert np.array_equal(getattr(trie, f), getattr(t2, f)), (name, f)


def test_dense_lexicons_count_as_stated():
    for a, d in ((3, 3), (4, 4), (9, 4), (10, 4)):
        words = tc.dense_words(a, d)
        assert len(words) == sum(a ** i for i in range(d + 1)) and words[0] == [] and len({tuple(w) for w in words}) == len(words)
    assert len(tc.dense_words(9, 4)) == 7381 and len(tc.dense_words(10, 4)) == 11111
    k = dense('a4d4')
    for m in (1, 2, 5, 6, 100, 341):                      # every leading part is closed under prefixes: as many nodes as words
        from lstm_ctc_ocr_amd.lexicon import LexiconTrie
        assert LexiconTrie(k.lexicon[:m], k.C, chunk_nodes=512).num_nodes == m
    # a tree that does not fit one chunk is cut, and shared ancestors are built again in the next chunk
    t = tc.build(k, 64)
    assert t.num_chunks > 341 // 64 and t.num_nodes > 341 and np.diff(t.chunk_node_start).max() <= 64


def LexiconTrieOf(words, C=12):
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie
    return LexiconTrie(words, C)


def test_default_chunk_rule():
    from lstm_ctc_ocr_amd import lexicon as lx
    assert lx.chunk_capacity() == 8192 and lx.DEFAULT_CHUNK_NODES <= lx.chunk_capacity()
    assert lx.DEFAULT_CHUNK_NODES == 1024 and lx.MIN_CHUNKS == 16
    # 1024 nodes a chunk; 512 or 256 where 1024 would make fewer than 16 chunks; never below the longest word + 1
    assert [lx.default_chunk_nodes(n, 4) for n in (1, 4096, 4097, 8192, 8193, 16384, 10 ** 7)] == [256, 256, 512, 512, 1024, 1024, 1024]
    assert lx.default_chunk_nodes(40, 255) == 256 and lx.default_chunk_nodes(5000, 255) == 512 and lx.default_chunk_nodes(300, 300) == 301
    t = tc.build(dense('a4d4'))
    assert t.chunk_nodes == 256 and t.num_chunks == 2 and 341 < t.num_nodes <= 341 + 5          # (the second chunk's root and shared ancestors)
    big = LexiconTrieOf(tc.dense_words(9, 4))
    assert big.chunk_nodes == 512 and big.num_chunks >= 7381 // 512


@pytest.mark.parametrize('name', [k.name for k in sc.cases()] + ['a3d3', 'a4d4', 'a3d3x'])
def test_model_against_reference(name):
    """The chunked recursion over the builder's arrays, in float64 and in float32, against per-word alpha_cost in float64."""
    k = sc.case(name) if name not in ('a3d3', 'a4d4', 'a3d3x') else dense(name)
    ref_c, ref_b = sc.reference(k)[:2]                     # (cached by name: the dense cases' names are their own)
    fin = np.isfinite(ref_c)
    worst64 = worst32 = 0.0
    sizes = tc.chunk_sizes(k)
    for cn in sizes:
        trie = tc.build(k, cn)
        c64 = tc.trie_model(trie, k.acts, k.il, np.float64)
        assert np.array_equal(np.isfinite(c64), fin) and np.all(c64[~fin] == np.inf), (name, cn)          # +inf exactly where the reference has it
        if fin.any():
            worst64 = max(worst64, float(np.abs(c64[fin] - ref_c[fin]).max()))
        assert np.array_equal(sc.summary(c64)[0], ref_b), (name, cn)                                      # lowest index on ties
        if cn in (sizes[0], None):
            c32 = tc.trie_model(trie, k.acts, k.il, np.float32)
            assert np.array_equal(np.isfinite(c32), fin) and np.all(c32[~fin] == np.inf), (name, cn)
            if fin.any():
                worst32 = max(worst32, float(np.abs(c32[fin] - ref_c[fin]).max()))
            assert np.array_equal(sc.summary(c32)[0], ref_b), (name, cn)
    print('%-10s float64 model against the reference %.3e; float32 floor of the tree recursion %.3e (ctc_score_cases.COST_FLOOR %.3e, bound %.3e)'
          % (name, worst64, worst32, sc.COST_FLOOR, sc.COST_BOUND))
    assert worst64 <= 1e-9
    assert worst32 <= sc.COST_BOUND


def test_host_arithmetic_and_declarations():
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    declared = nat.declared_symbols()
    for name in ('ocr_ctc_trie_chunk_capacity', 'ocr_ctc_trie_supported', 'ocr_ctc_trie_build', 'ocr_ctc_trie_workspace_size', 'ocr_ctc_score_trie'):
        assert name in declared and name in nat._SIGS and hasattr(lib, name), name
    assert len(nat._SIGS['ocr_ctc_score'][0]) == 18 and lib.ocr_abi_version() == 1
    for C in (0, 1, 40, 16384, 16385):
        for T in (0, 1, 63):
            for K in (0, 1, 65537, 1 << 20, (1 << 20) + 1):
                assert bool(lib.ocr_ctc_trie_supported(C, T, K)) == tc.supported(C, T, K), (C, T, K)
    assert lib.ocr_ctc_trie_supported(6625, 63, 1048576) == 1
    sz = ctypes.c_size_t(0)
    assert lib.ocr_ctc_trie_workspace_size(6625, 63, 64, ctypes.byref(sz)) == 0 and sz.value == sc.workspace_bytes(6625, 63, 64)
    for C, T, N in [(16385, 63, 4), (0, 63, 4), (40, 0, 4), (40, 63, 0)]:
        assert lib.ocr_ctc_trie_workspace_size(C, T, N, ctypes.byref(sz)) == 2
    assert lib.ocr_ctc_trie_workspace_size(40, 63, 4, None) == 2


def test_builder_refusals():
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie, chunk_capacity
    lib = nat.lib()
    words = np.array([[1, 2, 3], [4, 5, 0], [1, 2, 0]], np.int32)
    lens = np.array([3, 2, 2], np.int32)
    nc, nn = ctypes.c_int(0), ctypes.c_int(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def query(K=3, C=12, blank=0, chunk=8, words_=words, lens_=lens, counts=True):
        return lib.ocr_ctc_trie_build(p(words_) if words_ is not None else None, p(lens_) if lens_ is not None else None, K, 3, C, blank, chunk,
                                      ctypes.byref(nc) if counts else None, ctypes.byref(nn) if counts else None, None, None, None, None, None)
    assert query() == 0 and (nc.value, nn.value) == (1, 6)
    assert query(chunk=4) == 0 and (nc.value, nn.value) == (2, 7)          # root 1 2 3 | root 4 5: deepest word + 1 is taken
    assert query(chunk=3) == 2                                                # below (deepest valid word + 1)
    assert query(chunk=chunk_capacity()) == 0 and query(chunk=chunk_capacity() + 1) == 2 and query(chunk=0) == 2
    assert query(K=0) == 2 and query(K=-1) == 2 and query(K=(1 << 20) + 1) == 2
    assert query(blank=-1) == 2 and query(blank=12) == 2 and query(C=0) == 2 and query(C=16385) == 2
    assert query(words_=None) == 2 and query(lens_=None) == 2 and query(counts=False) == 2
    # an invalid word does not count as deep: [1 2 3] with label 3 out of range at C = 3 leaves depth 2
    assert query(C=3, chunk=3) == 0 and (nc.value, nn.value) == (1, 3)
    # the fill pass: arrays missing, or sized for less than the tree needs
    nodes, cn_, cw_, wn, wi = (np.zeros(16, np.int32) for _ in range(5))

    def fill(chunks, n_nodes, arrays=(nodes, cn_, cw_, wn, wi)):
        nc.value, nn.value = chunks, n_nodes
        return lib.ocr_ctc_trie_build(p(words), p(lens), 3, 3, 12, 0, 4, ctypes.byref(nc), ctypes.byref(nn), *[p(a) if a is not None else None for a in arrays])
    assert fill(2, 7) == 0 and (nc.value, nn.value) == (2, 7) and fill(3, 9) == 0 and (nc.value, nn.value) == (2, 7)
    assert nodes[:7].tolist() == [0, 1, 2 | 1 << 14 | 1 << 27, 3 | 2 << 14 | 1 << 27, 0, 4, 5 | 1 << 14 | 1 << 27]
    assert (cn_[:3].tolist(), cw_[:3].tolist(), wn[:3].tolist(), wi[:3].tolist()) == ([0, 4, 7], [0, 2, 3], [2, 3, 2], [2, 0, 1])
    assert fill(1, 7) == 2 and fill(2, 6) == 2
    for i in range(1, 5):
        arr = [nodes, cn_, cw_, wn, wi]
        arr[i] = None
        assert fill(2, 7, arr) == 2, i
    with pytest.raises(ValueError):
        LexiconTrie([], 12)
    with pytest.raises(nat.NativeError):
        LexiconTrie([[1, 2, 3]], 12, chunk_nodes=3)


def test_refusals_come_before_any_launch():
    """OCR_ERR_INVALID (2) for a NULL operand, partly NULL outputs, a blank outside [0, C), a short workspace, chunk sizes and counts out of range
    and every shape ocr_ctc_trie_supported refuses: host memory stands in for the operands, nothing reads it."""
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(acts=p, il=p, nodes=p, cns=p, cws=p, wn=p, wi=p, chunks=2, chunk_nodes=64, C=40, N=4, T=63, K=16, blank=0, costs=p, best=p, best_cost=p,
                norm=p, ws=p, ws_bytes=1024)

    def status(**kw):
        v = dict(good, **kw)
        return lib.ocr_ctc_score_trie(v['acts'], v['il'], v['nodes'], v['cns'], v['cws'], v['wn'], v['wi'], v['chunks'], v['chunk_nodes'], v['C'], v['N'],
                                      v['T'], v['K'], v['blank'], v['costs'], v['best'], v['best_cost'], v['norm'], v['ws'], v['ws_bytes'], None)
    assert sc.workspace_bytes(40, 63, 4) == 1024
    for operand in ('acts', 'il', 'nodes', 'cns', 'cws', 'wn', 'wi', 'costs', 'ws'):
        assert status(**{operand: None}) == 2, operand
    assert status(best=None) == 2 and status(best_cost=None, norm=None) == 2
    assert status(blank=-1) == 2 and status(blank=40) == 2
    assert status(ws_bytes=1023) == 2
    assert status(chunk_nodes=0) == 2 and status(chunk_nodes=8193) == 2 and status(chunks=0) == 2 and status(chunks=18) == 2
    assert status(K=0) == 2 and status(K=(1 << 20) + 1) == 2 and status(C=16385) == 2 and status(C=0) == 2
    assert status(T=0) == 2 and status(N=0) == 2 and status(N=65536, ws_bytes=1 << 30) == 2


def test_engine_checks_the_blank_and_keeps_its_signatures():
    """The blank check precedes every use of the engine's state, so it is made on an Engine that was never initialised."""
    import inspect
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie
    eng = object.__new__(Engine)
    trie = LexiconTrie([[1, 2], [3]], 12, blank=11)
    with pytest.raises(ValueError):
        eng.score(None, None, trie)                       # blank 0 against the trie's 11
    with pytest.raises(ValueError):
        eng.score(None, None, trie, blank=3)
    with pytest.raises(ValueError):
        eng.decode(None, None, method='lexicon', lexicon=trie)          # decode's lexicons have blank 0
    assert list(inspect.signature(Engine.score).parameters) == ['self', 'data', 'seq_len', 'lexicon', 'blank']
    assert [(n, q.default) for n, q in inspect.signature(Engine.decode).parameters.items()][3:] == [('method', 'beam'), ('beam_width', 100), ('lexicon', None)]
    assert len(trie) == 2 and trie[0] == [1, 2] and trie[-1] == [3] and trie[:] == [[1, 2], [3]]
