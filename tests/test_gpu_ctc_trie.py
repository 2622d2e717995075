"""-m gpu: lexicon scoring on a prefix tree (ctc_trie.hip, lexicon.LexiconTrie, ops.ctc_score_trie, Engine.score / Engine.decode with a
LexiconTrie) against the float64 reference on the cases of tests/ctc_score_cases.py, against ops.ctc_score on the same lexicon, at the edges of
the kernel's thread layout, and on the trained fixture.  Bounds: ctc_score_cases.COST_BOUND / NORM_BOUND as they stand (tests/ctc_trie_cases.py).

Measured on an MI355X (the tests print every figure before they assert):

    the 27 cases, least chunk size and default     every cost, best_cost and log_norm has the bits ops.ctc_score gives (|tree - ctc_score| = 0), so
                                                   the errors against the float64 reference are test_gpu_ctc_score.py's: cost 6.66e-4, log_norm
                                                   6.32e-4 at L255 (bounds 5.33e-3 / 5.06e-3), at most 9.0e-6 where T <= 12
    thread-layout edges (T = 10, 1 .. 8193 nodes)  cost error at most 6.5e-6 (bound 5.33e-3)
    trained logits (C1, V0)                        Engine.score with the tree: the list route's bits; 69 913 and 1 048 576 words keep the truth as
                                                   the best on 8 of 8 and 63 of 64 samples, as the small lexicon does
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_trie_cases as tc  # noqa: E402
import test_gpu_ctc_score as gs  # noqa: E402

sc, fx = tc.sc, gs.fx
pytestmark = pytest.mark.gpu
NAN, UNSET = gs.NAN, gs.UNSET
trained_engine = gs.trained_engine          # the module-scoped fixture of the list route's tests, instantiated for this module


def _native_run(k, trie, dev, want_best=True):
    """ocr_ctc_score_trie itself on a workspace and outputs filled with NaN bytes -> costs, best, best_cost, log_norm (device tensors)."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    a, il = (torch.from_numpy(np.array(v)).to(dev) for v in (k.acts, k.il))
    need = ops.ctc_trie_workspace_bytes(k.C, k.T, k.N)
    assert need == sc.workspace_bytes(k.C, k.T, k.N)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    costs = torch.full((k.N, k.K), NAN, device=dev)
    best = torch.full((k.N,), UNSET, dtype=torch.int32, device=dev)
    bc, ln = torch.full((k.N,), NAN, device=dev), torch.full((k.N,), NAN, device=dev)
    p = nat.ptr
    opt = (p(best), p(bc), p(ln)) if want_best else (None, None, None)
    nat.call('ocr_ctc_score_trie', p(a), p(il), *[p(t) for t in trie.device_arrays(dev)], trie.num_chunks, trie.chunk_nodes, k.C, k.N, k.T, k.K,
             k.blank, p(costs), *opt, p(ws), need, nat.stream())
    torch.cuda.synchronize()
    return costs, best, bc, ln


@pytest.mark.parametrize('chunk', ['minimal', 'default'])
@pytest.mark.parametrize('name', [k.name for k in sc.cases()])
def test_cases_against_reference(dev, name, chunk):
    from lstm_ctc_ocr_amd import ops
    k = sc.case(name)
    assert ops.ctc_trie_supported(k.C, k.T, k.K)
    trie = tc.build(k, tc.deepest(k) + 1 if chunk == 'minimal' else None)
    costs, best, bc, ln = _native_run(k, trie, dev)
    gs._check(k, 'tree, %s chunks of %d nodes (%d chunks, %d nodes)' % (chunk, trie.chunk_nodes, trie.num_chunks, trie.num_nodes), costs, best, bc, ln)
    # score only: the same costs, nothing else written
    c2, b2, bc2, ln2 = _native_run(k, trie, dev, want_best=False)
    assert torch.equal(c2.view(torch.int32), costs.view(torch.int32)) and bool((b2 == UNSET).all()) and bool(torch.isnan(bc2).all() and torch.isnan(ln2).all())
    # the ops entry: allocates what it is not given, same bits
    a, il, lab, lens = gs._inputs(k, dev)
    c3, b3, bc3, ln3 = ops.ctc_score_trie(a, il, trie)
    c4, b4, bc4, ln4 = ops.ctc_score_trie(a, il, trie, want_best=False, costs=torch.full((k.N, k.K), NAN, device=dev))
    assert (b4, bc4, ln4) == (None, None, None)
    for got, want in ((c3, costs), (c4, costs), (b3, best), (bc3, bc), (ln3, ln)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # against the per-candidate kernel on the same lexicon: both within COST_BOUND of the reference
    c5 = ops.ctc_score(a, il, lab, lens, blank=k.blank, want_best=False)[0]
    torch.cuda.synchronize()
    t, s = costs.cpu().numpy(), c5.cpu().numpy()
    fin = np.isfinite(s)
    assert np.array_equal(np.isfinite(t), fin)
    diff = float(np.abs(t[fin] - s[fin]).max()) if fin.any() else 0.0
    print('%s %s: |tree - ctc_score| at most %.3e (bound %.3e); bits %s' % (name, chunk, diff, 2 * sc.COST_BOUND,
                                                                            'agree' if np.array_equal(t.view(np.uint32), s.view(np.uint32)) else 'differ'))
    assert diff <= 2 * sc.COST_BOUND


# ------------------------------------------------------------------------------------------------ thread-layout edges
_EDGE = {}


def _edge_case():
    """N = 2, T = 10, C = 12, one input length short.  The lexicon: every string of up to 4 labels over 9 symbols, shortest first (7381 words and
    nodes), then 812 words of 5 labels, each one new node below a word of 4.  Every leading part of the list has as many nodes as words, so a
    node count is chosen by cutting the list; the float64 reference of the whole list is computed once and cut with it."""
    if not _EDGE:
        base = tc.dense_words(9, 4)
        extra = [w + [1 + (w[-1] % 9)] for w in base[-812:]]
        k = tc.dense_case('edge', 9, 4, extra=extra)
        assert k.K == 8193 and (k.N, k.T, k.C, k.il.tolist()) == (2, 10, 12, [10, 7])
        _EDGE['case'], _EDGE['ref'] = k, sc.reference(k)[0]
    return _EDGE['case'], _EDGE['ref']


# (words = nodes, chunk_nodes, chunks expected, the kernel form that runs it: threads x nodes a thread)
EDGES = [(1, 1, 1, '256x1'), (1, None, 1, '256x1'),                                           # a chunk of the root alone: the lexicon [[]]
         (255, 256, 1, '256x1'), (256, 256, 1, '256x1'), (257, 256, 2, '256x1'),              # every form one node short, full, and one node more,
         (257, 512, 1, '256x2'), (511, 512, 1, '256x2'), (512, 512, 1, '256x2'), (513, 512, 2, '256x2'),      # which makes two chunks; every
         (513, 1024, 1, '256x4'), (1023, 1024, 1, '256x4'), (1024, 1024, 1, '256x4'), (1025, 1024, 2, '256x4'),      # form's first size, one
         (1025, 4096, 1, '512x8'), (4095, 4096, 1, '512x8'), (4096, 4096, 1, '512x8'), (4097, 4096, 2, '512x8'),     # node above a multiple
         (4097, 8192, 1, '1024x8'),                                                           # of the workgroup
         (8191, 8192, 1, '1024x8'), (8192, 8192, 1, '1024x8'), (8193, 8192, 2, '1024x8')]     # the capacity - 1, the capacity, and two chunks


def _form(chunk_nodes):
    """ocr_ctc_score_trie's choice, restated: the smallest form that holds the largest chunk."""
    return [f for n, f in ((256, '256x1'), (512, '256x2'), (1024, '256x4'), (4096, '512x8'), (8192, '1024x8')) if chunk_nodes <= n][0]


@pytest.mark.parametrize('words,chunk_nodes,chunks,form', EDGES)
def test_thread_layout_edges(dev, words, chunk_nodes, chunks, form):
    from lstm_ctc_ocr_amd import ops
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie, chunk_capacity
    assert chunk_capacity() == 8192
    k, ref = _edge_case()
    trie = LexiconTrie(k.lexicon[:words], k.C, blank=k.blank, chunk_nodes=chunk_nodes)
    # (a second chunk builds the root and the ancestors of its first word again)
    assert trie.num_chunks == chunks and (trie.num_nodes == words if chunks == 1 else words < trie.num_nodes <= words + 5), (trie.num_chunks, trie.num_nodes)
    assert _form(trie.chunk_nodes) == form
    if chunks == 1:
        assert int(np.diff(trie.chunk_node_start).max()) == words
    a, il = (torch.from_numpy(np.array(v)).to(dev) for v in (k.acts, k.il))
    costs = torch.full((k.N, words), NAN, device=dev)
    c, best, bc, ln = ops.ctc_score_trie(a, il, trie, costs=costs)
    torch.cuda.synchronize()
    c = c.cpu().numpy()
    want = ref[:, :words]
    fin = np.isfinite(want)
    assert not np.isnan(c).any() and np.array_equal(np.isfinite(c), fin) and np.all(c[~fin] == np.inf)
    err = float(np.abs(c[fin] - want[fin]).max())
    print('%d nodes in chunks of %d: cost error %.3e (bound %.3e)' % (words, trie.chunk_nodes, err, sc.COST_BOUND))
    assert err <= sc.COST_BOUND
    # the arg-min: the device's own lowest cost, bit for bit, and a word whose reference cost is within the two words' error bounds of the least
    # (at 8191 words and more the reference's best leads its runner-up by 6.7e-3, less than 2 x COST_BOUND)
    b = best.cpu().numpy()
    assert np.array_equal(b, np.argmin(c, axis=1))
    assert np.all(want[np.arange(k.N), b] <= want.min(axis=1) + 2 * sc.COST_BOUND)
    assert np.array_equal(bc.cpu().numpy().view(np.uint32), c[np.arange(k.N), b].view(np.uint32))
    norm = np.array([np.logaddexp.reduce(-r) for r in want])
    assert float(np.abs(ln.cpu().numpy() - norm).max()) <= sc.NORM_BOUND


# ------------------------------------------------------------------------------------------------ trained logits
@pytest.mark.parametrize('name', ['C1', 'V0'])
def test_engine_on_trained_logits(trained_engine, name):
    """Engine.score and Engine.decode(method='lexicon') with a LexiconTrie against the same calls with the list; then a lexicon the list route
    refuses: the truth strings plus every string of up to 4 labels over 16 symbols (69905 of them)."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie
    eng = trained_engine
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, name)
    N = x.shape[0]
    truth = gs._truth_of(d, name)
    C = eng.forward(x, sl).shape[2]
    rng = np.random.RandomState(77)
    lexicon = [list(t) for t in truth] + [e for t in truth for e in gs._edits(list(t), C, rng)]
    trie = LexiconTrie(lexicon, C)
    costs, best, best_cost, log_norm = eng.score(x, sl, lexicon)
    tcosts, tbest, tbest_cost, tlog_norm = eng.score(x, sl, trie)
    assert tcosts.shape == (N, 4 * N) and tcosts.dtype == np.float32 and tbest.dtype == np.int32
    fin = np.isfinite(costs)
    assert np.array_equal(np.isfinite(tcosts), fin)
    diff = float(np.abs(tcosts[fin] - costs[fin]).max())
    print('%s: |Engine.score(trie) - Engine.score(list)| at most %.3e (bound %.3e); bits %s; %d chunks of at most %d nodes'
          % (name, diff, 2 * sc.COST_BOUND, 'agree' if np.array_equal(tcosts.view(np.uint32), costs.view(np.uint32)) else 'differ', trie.num_chunks,
             trie.chunk_nodes))
    assert diff <= 2 * sc.COST_BOUND
    assert np.array_equal(tbest, best)
    assert float(np.abs(tlog_norm - log_norm)[np.isfinite(log_norm)].max()) <= 2 * sc.NORM_BOUND
    picked = eng.decode(x, sl, method='lexicon', lexicon=lexicon)
    assert eng.decode(x, sl, method='lexicon', lexicon=trie) == picked
    # above 65536 words
    big = lexicon[:N] + tc.dense_words(16, 4)
    assert len(big) == N + 69905 > 65536
    with pytest.raises(nat.NativeError):
        eng.score(x, sl, big)
    big_trie = LexiconTrie(big, C)
    bpicked = eng.decode(x, sl, method='lexicon', lexicon=big_trie)
    bbest = eng.score(x, sl, big_trie)[1]
    hit = [i for i in range(N) if picked[i] == truth[i]]
    print('%s: %d words, %d nodes in %d chunks; the truth is the best of the small lexicon on %d of %d samples and of the large one on %d of those'
          % (name, len(big), big_trie.num_nodes, big_trie.num_chunks, len(hit), N, sum(bpicked[i] == truth[i] for i in hit)))
    assert len(hit) >= 0.9 * N
    for i in hit:
        assert bpicked[i] == truth[i] and big[bbest[i]] == truth[i], (i, bpicked[i], truth[i])


def test_a_million_words(trained_engine):
    """The largest lexicon the entry point takes, 1048576 words: the batch's truth strings and random words of 2 .. 12 labels, as dense arrays.
    Engine.decode returns the truth wherever the small lexicon of test_engine_on_trained_logits does, and Engine.score's best is that word."""
    from lstm_ctc_ocr_amd import ops
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie
    eng = trained_engine
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, 'C1')
    N = x.shape[0]
    truth = gs._truth_of(d, 'C1')
    C = eng.forward(x, sl).shape[2]
    K = 1 << 20
    assert ops.ctc_trie_supported(C, 63, K) and not ops.ctc_trie_supported(C, 63, K + 1)
    rng = np.random.RandomState(78)
    lens = rng.randint(2, 13, size=K).astype(np.int32)
    dense = rng.randint(1, C, size=(K, max(12, max(len(t) for t in truth)))).astype(np.int32)
    for i, t in enumerate(truth):
        lens[i] = len(t)
        dense[i, :len(t)] = t
    trie = LexiconTrie((dense, lens), C)
    assert len(trie) == K and trie[N - 1] == list(truth[N - 1])
    small = eng.decode(x, sl, method='lexicon', lexicon=[list(t) for t in truth])
    picked = eng.decode(x, sl, method='lexicon', lexicon=trie)
    costs, best, best_cost, log_norm = eng.score(x, sl, trie)
    hit = [i for i in range(N) if small[i] == truth[i]]
    print('1048576 words: %d nodes in %d chunks of at most %d; the truth is decoded on %d of %d samples' % (trie.num_nodes, trie.num_chunks, trie.chunk_nodes,
                                                                                                           sum(picked[i] == truth[i] for i in hit), N))
    assert costs.shape == (N, K) and len(hit) >= 0.9 * N
    for i in hit:
        assert picked[i] == truth[i] and trie[best[i]] == truth[i] and best_cost[i] == costs[i, best[i]]
