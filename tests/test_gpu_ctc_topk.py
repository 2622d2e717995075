"""-m gpu: the k best of a lexicon (ctc_topk.hip, ops.ctc_topk, Engine.nbest / Engine.decode_nbest) against the numpy model of
tests/ctc_topk_cases.py.  The result is fully determined, so every comparison is on the bits and there is no tolerance anywhere.

    synthetic rows through ocr_ctc_topk itself     N in {1, 3} x k in {1, 2, 5, 63, 64} x 14 row lengths (1 .. 257, around a segment's 4096 entries
                                                   and around the 8192 at which a row is cut) x 11 regimes x 2 layouts (tight and 16-byte aligned;
                                                   ld = K + 3 from a base one float past an aligned address, the gaps filled with -1e30, which would
                                                   win every selection); outputs between poisoned guard rows, the workspace filled with 0xFF
    segment edges                                  K = 2^20, N = 2, k = 64: the winners on the last entry of a segment and the first of the next
    real costs                                     the 27 cases of tests/ctc_score_cases.py through ops.ctc_score, then ops.ctc_topk at k = 1, 5, 64
    the engine on the trained fixture              Engine.nbest by the list and by a LexiconTrie, Engine.decode_nbest, Engine.decode unchanged

Measured on an MI355X (build 90586dbd28e3df51; the tests print every figure before they assert):

    every comparison                               equal bits: 308 launches per (N, k) of the synthetic grid, the segment-edge rows twice, the 27 scoring
                                                   cases at k = 1, 5, 64, both engine routes
    sum of the returned posteriors                 at most 1.000004712 (lane32, k = 5 and 64; asserted: at most 1 + 1e-5); the 5 best of the trained
                                                   fixture's lexicon hold 0.999208 .. 1.000000 of the posterior
    tools/ctc_topk_bench.py, N = 64                K = 1048576: k = 1 / 5 / 64 in 54.3 / 56.0 / 81.8 us on random costs (78 / 76 / 52 % of the 6.3 TB/s
                                                   streaming rate; torch.topk 659 / 673 / 677 us; costs.cpu() + np.argpartition 165 .. 169 ms) and in
                                                   370 / 370 / 547 us on descending rows, the worst case (torch.topk 670 / 675 / 684 us); K = 65536:
                                                   19.4 / 20.4 / 35.5 us (torch.topk 118 / 123 / 132 us); K = 1024: 18.6 / 19.0 / 18.6 us (26 / 35 / 40 us);
                                                   behind ctc_score_trie on 1048576 words (21 064 us): 55.2 us, 0.26 % of it
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_topk_cases as tk  # noqa: E402
import test_gpu_ctc_score as gs  # noqa: E402

sc, fx = gs.sc, gs.fx
pytestmark = pytest.mark.gpu
NAN = float('nan')
UNSET = 0x7fffffff
GAP = -1e30
trained_engine = gs.trained_engine          # the module-scoped fixture of the list route's tests, instantiated for this module


def _layout(c, layout, dev):
    """The device matrix of a numpy [N, K]: 'tight' (ld = K, 16-byte aligned) or 'view' (ld = K + 3, the base one float past an aligned address,
    every float outside the rows GAP)."""
    N, K = c.shape
    if layout == 'tight':
        t = torch.from_numpy(c).to(dev)
        assert t.data_ptr() % 16 == 0 and t.stride(0) == K
        return t
    ld = K + 3
    buf = torch.full((1 + N * ld + 4,), GAP, dtype=torch.float32, device=dev)
    view = buf[1:1 + N * ld].view(N, ld)[:, :K]
    view.copy_(torch.from_numpy(c).to(dev))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.stride(0) == ld and view.shape == (N, K)
    return view


def _native_run(costs, k, log_norm):
    """ocr_ctc_topk itself: outputs filled with NaN / 0x7fffffff between one poisoned guard row before and one after, the workspace filled with
    0xFF bytes -> (index, cost, log_post or None, count) as numpy; asserts that the guards came back untouched."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    dev = costs.device
    N, K = costs.shape
    need = ops.ctc_topk_workspace_bytes(N, K, k)
    assert need == tk.workspace_bytes(N, K, k)
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device=dev)
    index = torch.full((N + 2, k), UNSET, dtype=torch.int32, device=dev)
    cost = torch.full((N + 2, k), NAN, device=dev)
    post = torch.full((N + 2, k), NAN, device=dev)
    count = torch.full((N + 2,), UNSET, dtype=torch.int32, device=dev)
    p = nat.ptr
    ld = costs.stride(0) if N > 1 else K
    nat.call('ocr_ctc_topk', p(costs), ld, N, K, k, p(log_norm), p(index[1:]), p(cost[1:]), p(post[1:]) if log_norm is not None else None,
             p(count[1:]), p(ws) if need else None, need, nat.stream())
    torch.cuda.synchronize()
    index, cost, post, count = (v.cpu().numpy() for v in (index, cost, post, count))
    for g in (0, N + 1):
        assert np.all(index[g] == UNSET) and np.all(np.isnan(cost[g])) and np.all(np.isnan(post[g])) and count[g] == UNSET, 'guard row %d written' % g
    if log_norm is None:
        assert np.all(np.isnan(post))
    return index[1:-1], cost[1:-1], post[1:-1] if log_norm is not None else None, count[1:-1]


def _same(got, want, tag):
    for name, g, w in zip(('index', 'cost', 'log_post', 'count'), got, want):
        if w is None:
            assert g is None, (tag, name)
            continue
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        if not tk.same_bits(g, w):
            bad = np.argwhere(np.ascontiguousarray(g).view(np.int32) != np.ascontiguousarray(w).view(np.int32))[0]
            raise AssertionError('%s: %s differs first at %s: got %r, want %r' % (tag, name, tuple(bad), g[tuple(bad)], w[tuple(bad)]))


# ------------------------------------------------------------------------------------------------ synthetic rows
@pytest.mark.parametrize('k', tk.SELECT)
@pytest.mark.parametrize('N', tk.BATCH)
def test_synthetic_rows(dev, N, k):
    from lstm_ctc_ocr_amd import ops
    lengths = tk.row_lengths(N, k)
    assert lengths[:8] == [1, 2, 63, 64, 65, 255, 256, 257] and lengths[8:] == [4095, 4096, 4097, 8191, 8192, 8193]
    assert ops.ctc_topk_plan(N, 1 << 20, k) == (256, 4096) and ops.ctc_topk_plan(N, 8193, k) == (3, 4096) and ops.ctc_topk_plan(N, 8192, k) == (1, 8192)
    runs = 0
    for K in lengths:
        for r, regime in enumerate(tk.REGIMES):
            c = tk.make_rows(regime, N, K, k, 1000 * N + 10 * k + r + K)
            ln = (np.random.RandomState(K + r).randn(N) * 2.0).astype(np.float32)
            want = tk.topk_model(c, k, ln)
            for layout in ('tight', 'view'):
                tag = 'N=%d k=%d K=%d %s %s' % (N, k, K, regime, layout)
                costs = _layout(c, layout, dev)
                _same(_native_run(costs, k, torch.from_numpy(ln).to(dev)), want, tag)
                runs += 1
            if r == K % len(tk.REGIMES):                   # one regime per length: the ops entry on the view, and no log_norm
                _same(ops.ctc_topk(costs, k, log_norm=torch.from_numpy(ln).to(dev)), want, tag + ' ops')
                _same(_native_run(costs, k, None), (want[0], want[1], None, want[3]), tag + ' no log_norm')
    assert runs == 14 * len(tk.REGIMES) * 2


def test_plan_sizes_are_what_the_lengths_assume():
    """segment_len - 1, segment_len, segment_len + 1 and 2 * segment_len + 1 of the finest cut, and the one-segment limit - 1, limit, limit + 1:
    six lengths, because 2 * segment_len + 1 is the limit + 1."""
    assert tk.plan_sizes(1, 5) == tk.plan_sizes(3, 64) == [4095, 4096, 4097, 8191, 8192, 8193]


# ------------------------------------------------------------------------------------------------ segment edges
def test_segment_edges_at_a_million_entries(dev):
    from lstm_ctc_ocr_amd import ops
    N, K, k = 2, 1 << 20, 64
    c = tk.segment_edge_rows(N, K, k)
    segments, seg_len = ops.ctc_topk_plan(N, K, k)
    assert (segments, seg_len) == tk.plan(N, K, k) == (256, 4096)
    ln = np.array([0.5, -2.0], np.float32)
    want = tk.topk_model(c, k, ln)
    at = np.sort(want[0], axis=1)
    assert np.all((at[:, 0::2] + 1) % seg_len == 0) and np.all(at[:, 1::2] % seg_len == 0)          # the winners sit on the segments' edges
    for layout in ('tight', 'view'):
        got = _native_run(_layout(c, layout, dev), k, torch.from_numpy(ln).to(dev))
        _same(got, want, 'segment edges, ' + layout)
    # determinism: the same launch again, and through the ops entry
    costs = _layout(c, 'tight', dev)
    first = _native_run(costs, k, torch.from_numpy(ln).to(dev))
    _same(_native_run(costs, k, torch.from_numpy(ln).to(dev)), first, 'second run')
    _same(ops.ctc_topk(costs, k, log_norm=torch.from_numpy(ln).to(dev)), first, 'ops entry')


@pytest.mark.parametrize('N,K,k', [(200, 50000, 5), (3, 100001, 64), (1025, 8193, 2)])
def test_plans_between_the_extremes(dev, N, K, k):
    """Segments of three rounds with a ragged last one, 25 segments of one round, and rows of more than two rounds taken by one workgroup each
    because the samples alone fill the chip."""
    from lstm_ctc_ocr_amd import ops
    rng = np.random.default_rng(N + k)
    c = rng.standard_normal((N, K), dtype=np.float32) * np.float32(3.0)
    c[:, K - 1] = -100.0                                                                              # the last entry of the row wins
    c[0, :] = np.linspace(5.0, -5.0, K, dtype=np.float32)                                            # one descending row
    assert ops.ctc_topk_plan(N, K, k) == tk.plan(N, K, k) == {200: (5, 12288), 3: (25, 4096), 1025: (1, 12288)}[N]
    ln = rng.standard_normal(N, dtype=np.float32)
    want = tk.topk_model(c, k, ln)
    _same(_native_run(_layout(c, 'tight', dev), k, torch.from_numpy(ln).to(dev)), want, 'N=%d K=%d k=%d' % (N, K, k))
    if N == 3:
        _same(_native_run(_layout(c, 'view', dev), k, torch.from_numpy(ln).to(dev)), want, 'N=%d K=%d k=%d view' % (N, K, k))


# ------------------------------------------------------------------------------------------------ real costs
@pytest.mark.parametrize('name', [k.name for k in sc.cases()])
def test_on_the_scorer_costs(dev, name):
    from lstm_ctc_ocr_amd import ops
    case = sc.case(name)
    a, il, lab, lens = gs._inputs(case, dev)
    costs, best, best_cost, log_norm = ops.ctc_score(a, il, lab, lens, blank=case.blank)
    torch.cuda.synchronize()
    c, ln = costs.cpu().numpy(), log_norm.cpu().numpy()
    b, bc = best.cpu().numpy(), best_cost.cpu().numpy()
    for k in (1, 5, 64):
        got = ops.ctc_topk(costs, k, log_norm=log_norm)
        torch.cuda.synchronize()
        _same(got, tk.topk_model(c, k, ln), '%s k=%d' % (name, k))
        index, cost, post, count = (v.cpu().numpy() for v in got)
        if k == 1:
            assert np.array_equal(index[:, 0], b) and np.array_equal(count, (b >= 0).astype(np.int32))          # -1 <-> count 0
            assert tk.same_bits(cost[:, 0], bc)
        total = np.exp(post.astype(np.float64)).sum(axis=1)
        print('%s k=%d: sum of the returned posteriors %.9f .. %.9f (at most 1 + 1e-5)' % (name, k, total.min(), total.max()))
        assert np.all(total <= 1 + 1e-5)


# ------------------------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize('name', ['C1', 'V0'])
def test_engine_nbest_on_trained_logits(trained_engine, name):
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
    picked = eng.decode(x, sl, method='lexicon', lexicon=lexicon)
    for route, lex in (('list', lexicon), ('trie', trie)):
        costs, best, best_cost, log_norm = eng.score(x, sl, lex)
        assert eng.decode(x, sl, method='lexicon', lexicon=lex) == [[v for v in lexicon[b]] if b >= 0 else [] for b in best] == picked          # unchanged
        for k in (1, 5):
            got = eng.nbest(x, sl, lex, k=k)
            assert all(isinstance(v, np.ndarray) for v in got) and got[0].shape == (N, k) and got[3].shape == (N,)
            _same(got, tk.topk_model(costs, k, log_norm), '%s %s k=%d' % (name, route, k))
        index, ncost, post, count = eng.nbest(x, sl, lex)                                             # k = 5
        assert np.array_equal(index[:, 0], best) and tk.same_bits(ncost[:, 0], best_cost)
        pairs = eng.decode_nbest(x, sl, lex, k=3)
        i3, _, p3, n3 = eng.nbest(x, sl, lex, k=3)
        assert len(pairs) == N
        for n in range(N):
            assert len(pairs[n]) == n3[n] == min(3, int(np.isfinite(costs[n]).sum()))
            assert [w for w, _ in pairs[n]] == [[v for v in lexicon[i] if v != 0] for i in i3[n, :n3[n]]]
            assert [np.float32(q) for _, q in pairs[n]] == p3[n, :n3[n]].tolist()
            assert all(pairs[n][j][1] >= pairs[n][j + 1][1] for j in range(len(pairs[n]) - 1))          # best first
            assert (pairs[n][0][0] if pairs[n] else []) == picked[n]
        total = np.exp(post.astype(np.float64)).sum(axis=1)
        print('%s, %s: the 5 best hold %.6f .. %.6f of the posterior; %d samples with fewer than 5 feasible words'
              % (name, route, total.min(), total.max(), int((count < 5).sum())))
        assert np.all(total <= 1 + 1e-5)
