"""-m gpu: CTC forced alignment (ctc_align.hip, ops.ctc_align, Engine.align, Engine.decode_spans) on the cases of tests/ctc_align_cases.py: bit for
bit against the float32 model fed the device's own lse table, against the float64 reference, against the shipped scorer, across the label
layouts, the refusals, and on the trained fixture.  Bounds and their derivation: ctc_align_cases.py.

Measured on an MI355X (worst over the cases; the tests print every figure before they assert):

                                   float32 floor     bound (8 x)     device
    path_cost, absolute            9.40e-4           7.52e-3         9.40e-4 (L255; lane128 5.60e-4, lane127 4.35e-4, T129 1.88e-4, T <= 31: at most 1.1e-5)
    span score, absolute           1.47e-4           1.18e-3         1.74e-4 (lane63; lane127 1.47e-4, L255 1.04e-4, T <= 31: at most 5.0e-6)
    bit for bit against the float32 model fed the device's lse table: 0 of 1295 (sample, candidate) pairs differ
    the float64 score of the device's path is the float64 optimum (below it by at most 1.6e-12, summation order) on all 1179 feasible pairs: the
    device path is the reference's on every pair, the 55 with a margin at or below 2 x PATH_BOUND = 1.50e-2 included
    against ops.ctc_score: cost - path_cost at most 0 (bound 1.29e-2); on 'tight' the two are equal
    trained logits (C1, V0): the greedy strings' spans are the per-frame arg-max runs on every sample (smallest float64 margins 0.25 and 0.019,
    2 x bound 9.98e-5); Engine.score cost - path_cost at most -2.7e-6 (bound 1.15e-4), path_cost - cost up to 0.92; confidences 0.71 .. 1.00
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_cases as ac  # noqa: E402
import test_gpu_ctc_trained as tt  # noqa: E402

sc = ac.sc
fx = tt.fx
pytestmark = pytest.mark.gpu
NAN = float('nan')
UNSET = -777          # start's and end's fill: NaN bytes would read -1, which is an answer
NAMES = [k.name for k in ac.cases()]


def _inputs(k, dev, per_sample=False):
    lab, lens = k.per_sample()[:2] if per_sample else k.packed()
    return tuple(torch.from_numpy(np.array(v)).to(dev) for v in (k.acts, k.il, lab, lens))          # (copies: the case's arrays are read-only)


def _native_run(k, dev, per_sample=False):
    """ocr_ctc_align itself on a 0xFF-filled workspace and NaN / UNSET-filled outputs -> start, end, score, path_cost, lse [T, N] as numpy."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    a, il, lab, lens = _inputs(k, dev, per_sample)
    need = ops.ctc_align_workspace_bytes(k.C, k.T, k.N, k.K, k.mll)
    assert need == ac.workspace_bytes(k.C, k.T, k.N, k.K, k.mll)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)          # 0xFFFFFFFF: a NaN in every float
    start = torch.full((k.N, k.K, k.mll), UNSET, dtype=torch.int32, device=dev)
    end = torch.full((k.N, k.K, k.mll), UNSET, dtype=torch.int32, device=dev)
    score = torch.full((k.N, k.K, k.mll), NAN, device=dev)
    cost = torch.full((k.N, k.K), NAN, device=dev)
    p = nat.ptr
    nat.call('ocr_ctc_align', p(a), p(il), p(lab), p(lens), k.K if per_sample else 0, k.C, k.N, k.T, k.K, k.mll, k.blank,
             p(start), p(end), p(score), p(cost), p(ws), need, nat.stream())
    torch.cuda.synchronize()
    lse = ws[:k.T * k.N * 4].view(torch.float32).reshape(k.T, k.N).cpu().numpy()
    return start.cpu().numpy(), end.cpu().numpy(), score.cpu().numpy(), cost.cpu().numpy(), lse


_RUNS = {}


def _run(k, dev):
    """The shared-list run of a case, made once and left unchanged."""
    if k.name not in _RUNS:
        out = _native_run(k, dev)
        for v in out:
            v.setflags(write=False)
        _RUNS[k.name] = out
    return _RUNS[k.name]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', NAMES)
def test_bit_for_bit_against_the_float32_model(dev, name):
    """The model runs the kernel's arithmetic on the lse table the device computed: every output word is equal, nothing is left unset, and the
    slots beyond a length and the infeasible candidates hold exactly -1 / -1 / -inf / +inf."""
    from lstm_ctc_ocr_amd import ops
    k = ac.case(name)
    assert ops.ctc_align_supported(k.C, k.T, k.mll, k.K)
    start, end, score, cost, lse = _run(k, dev)
    for n in range(k.N):          # the table: written for the frames a sample owns, untouched beyond
        Tn = max(min(int(k.il[n]), k.T), 0)
        assert np.isfinite(lse[:Tn, n]).all() and np.isnan(lse[Tn:, n]).all(), (name, n)
    model = ac.align_model(k, np.float32, lse=lse)
    assert not (start == UNSET).any() and not (end == UNSET).any() and not np.isnan(score).any() and not np.isnan(cost).any(), name
    bad = [(n, j) for n in range(k.N) for j in range(k.K)
           if not (_same_bits(start[n, j], model.start[n, j]) and _same_bits(end[n, j], model.end[n, j]) and _same_bits(score[n, j], model.score[n, j])
                   and cost[n, j].tobytes() == model.cost[n, j].tobytes())]
    print('%s: %d of %d (sample, candidate) pairs differ from the float32 model%s' % (name, len(bad), k.N * k.K, ': %s' % bad[:6] if bad else ''))
    assert not bad, (name, bad[:6])
    for n in range(k.N):
        for j in range(k.K):
            L = int(k.lens[j]) if ac.feasible(k, n, j) else 0
            assert np.all(start[n, j, L:] == -1) and np.all(end[n, j, L:] == -1) and np.all(score[n, j, L:] == -np.inf), (name, n, j)
            assert (cost[n, j] == np.inf) == (not ac.feasible(k, n, j)), (name, n, j)


@pytest.mark.parametrize('name', NAMES)
def test_against_the_float64_reference(dev, name):
    """Independent of the model: every span set is a valid alignment whose float64 score is within PATH_BOUND of the float64 optimum, path_cost and
    the span scores are within their bounds, and the spans are the reference's wherever the margin exceeds 2 x PATH_BOUND (the share of pairs at
    or below it is capped in tests/test_ctc_align_cases.py).

    Measured on an MI355X: see the module docstring."""
    k = ac.case(name)
    start, end, score, cost, _ = _run(k, dev)
    ref, mg = ac.reference(k), ac.margins(k)
    worst_gap = worst_cost = worst_score = above = 0.0
    exact = differ = 0
    problems = []
    for n in range(k.N):
        for j in range(k.K):
            if (n, j) not in ref.paths:
                assert cost[n, j] == np.inf and np.all(start[n, j] == -1), (name, n, j)
                continue
            L, Tn = int(k.lens[j]), min(int(k.il[n]), k.T)
            label = k.lexicon[j][:L]
            st, en = start[n, j, :L], end[n, j, :L]
            if not ac.valid_alignment(label, st, en, Tn):
                problems.append(('invalid', n, j, st.tolist(), en.tolist()))
                continue
            lyx, _ = ac.slot_logprobs(k, n, j, np.float64)
            path = ac.path_of(st, en, L, Tn)
            got = float(lyx[np.arange(Tn), path].sum())
            worst_gap = max(worst_gap, -float(ref.cost[n, j]) - got)
            above = max(above, got + float(ref.cost[n, j]))          # (no path beats the optimum)
            worst_cost = max(worst_cost, abs(float(cost[n, j]) - float(ref.cost[n, j])))
            if L:
                own = ac.span_scores(lyx, st, en)          # the float64 score of the device's own spans
                worst_score = max(worst_score, float(np.abs(score[n, j, :L].astype(np.float64) - own).max()))
            same = np.array_equal(st, ref.start[n, j, :L]) and np.array_equal(en, ref.end[n, j, :L])
            differ += not same
            if mg[(n, j)] > 2 * ac.PATH_BOUND:
                exact += 1
                if not same:
                    problems.append(('spans', n, j, mg[(n, j)]))
    msg = ('%s: float64 score of the device path below the optimum by at most %.3e, path_cost error %.3e (bound %.3e); span score error %.3e '
           '(bound %.3e); %d of %d feasible pairs compared exactly, %d differ from the reference in all'
           % (name, worst_gap, worst_cost, ac.PATH_BOUND, worst_score, ac.SCORE_BOUND, exact, len(mg), differ))
    print(msg)
    assert not problems, (msg, problems[:4])
    assert above <= 1e-9 * max(1.0, float(np.abs(ref.cost[np.isfinite(ref.cost)]).max()) if mg else 1.0) and worst_gap <= ac.PATH_BOUND and worst_cost <= ac.PATH_BOUND and worst_score <= ac.SCORE_BOUND, msg
    if name in ac.PLANTED:
        n, j, st, en = ac.PLANTED[name]
        assert np.array_equal(start[n, j], st) and np.array_equal(end[n, j], en)
    if name == 'flat':
        for n in range(k.N):
            for j, label in enumerate(k.lexicon):
                st, en = ac.left_packed(label)
                assert np.array_equal(start[n, j, :len(label)], st) and np.array_equal(end[n, j, :len(label)], en), (n, j)
    if name == 'ends':
        S = 2 * len(k.lexicon[0]) + 1
        assert end[0, 0, len(k.lexicon[0]) - 1] == k.T - 1 and end[1, 0, len(k.lexicon[0]) - 1] < k.T - 1 and ac.ENDS == {0: 2, 1: 1} and S == 7


@pytest.mark.parametrize('name', NAMES)
def test_against_the_shipped_scorer(dev, name):
    """The best path carries no more probability than all paths: path_cost >= ops.ctc_score's cost within the sum of the two bounds (each a float32
    recursion within its bound of its float64 value); where one alignment exists ('tight') the two agree within that sum; +inf in the same places."""
    from lstm_ctc_ocr_amd import ops
    k = ac.case(name)
    cost = _run(k, dev)[3]
    a, il, lab, lens = _inputs(k, dev)
    total = ops.ctc_score(a, il, lab, lens, blank=k.blank, want_best=False)[0].cpu().numpy()
    fin = np.isfinite(total)
    assert np.array_equal(np.isfinite(cost), fin) and np.all(cost[~fin] == np.inf) and np.all(total[~fin] == np.inf), name
    slack = ac.PATH_BOUND + sc.COST_BOUND
    low = float((total[fin].astype(np.float64) - cost[fin]).max()) if fin.any() else 0.0
    print('%s: ctc_score cost - path_cost at most %.3e (bound %.3e); path_cost - cost up to %.3f' %
          (name, low, slack, float((cost[fin].astype(np.float64) - total[fin]).max()) if fin.any() else 0.0))
    assert low <= slack, name
    if name == 'tight':
        for n, j in ac.TIGHT_PAIRS:
            print('tight (%d, %d): |path_cost - cost| %.3e (bound %.3e)' % (n, j, abs(float(cost[n, j]) - float(total[n, j])), slack))
            assert abs(float(cost[n, j]) - float(total[n, j])) <= slack, (n, j)


@pytest.mark.parametrize('name', list(ac.PER_SAMPLE_CASES))
def test_layouts(dev, name):
    """Per-sample lists (each sample's candidates permuted) give the shared run's results under the permutation; the [N, L] form is K = 1; two
    calls, and a caller's workspace against an allocated one, give the same bits."""
    from lstm_ctc_ocr_amd import ops
    k = ac.case(name)
    shared = _run(k, dev)[:4]
    per = _native_run(k, dev, per_sample=True)[:4]
    perm = k.per_sample()[2]
    for got, want in zip(per[:3], shared[:3]):
        assert _same_bits(got, np.take_along_axis(want, perm[:, :, None], axis=1)), name
    assert _same_bits(per[3], np.take_along_axis(shared[3], perm, axis=1)), name
    again = _native_run(k, dev, per_sample=True)[:4]
    assert all(_same_bits(x, y) for x, y in zip(per, again)), name
    # the ops entry: the three layouts
    a, il, lab, lens = _inputs(k, dev)
    out = ops.ctc_align(a, il, lab, lens, blank=k.blank, shared=True)
    assert [tuple(v.shape) for v in out] == [(k.N, k.K, k.mll)] * 3 + [(k.N, k.K)] and out[0].dtype == torch.int32 and out[2].dtype == torch.float32
    assert all(_same_bits(v.cpu().numpy(), w) for v, w in zip(out, shared)), name
    ws = torch.full((ops.ctc_align_workspace_bytes(k.C, k.T, k.N, k.K, k.mll) + 512,), 0x5A, dtype=torch.uint8, device=dev)
    out_ws = ops.ctc_align(a, il, lab, lens, blank=k.blank, shared=True, workspace=ws)
    assert all(_same_bits(v.cpu().numpy(), w) for v, w in zip(out_ws, shared)), name
    a, il, plab, plens = _inputs(k, dev, per_sample=True)
    out = ops.ctc_align(a, il, plab, plens, blank=k.blank)
    assert all(_same_bits(v.cpu().numpy(), w) for v, w in zip(out, per)), name
    with pytest.raises(ValueError):
        ops.ctc_align(a, il, plab, plens, blank=k.blank, shared=True)
    # one transcript per sample: sample n takes candidate n mod K
    pick = np.arange(k.N) % k.K
    tp = torch.from_numpy(pick).to(dev)
    one = ops.ctc_align(a, il, lab[tp].contiguous(), lens[tp].contiguous(), blank=k.blank)
    k1 = ops.ctc_align(a, il, lab[tp][:, None, :].contiguous(), lens[tp][:, None].contiguous(), blank=k.blank)
    assert [tuple(v.shape) for v in one] == [(k.N, k.mll)] * 3 + [(k.N,)] and [tuple(v.shape) for v in k1] == [(k.N, 1, k.mll)] * 3 + [(k.N, 1)]
    for v, w, s in zip(one, k1, shared):
        assert _same_bits(v.cpu().numpy(), w[:, 0].cpu().numpy()) and _same_bits(v.cpu().numpy(), s[np.arange(k.N), pick]), name


def test_refused_inputs_launch_nothing(dev):
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    k = ac.case('T65')
    a, il, lab, lens = _inputs(k, dev)
    need = ops.ctc_align_workspace_bytes(k.C, k.T, k.N, k.K, k.mll)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    start = torch.full((k.N, k.K, k.mll), 7, dtype=torch.int32, device=dev)
    end = torch.full((k.N, k.K, k.mll), 7, dtype=torch.int32, device=dev)
    score = torch.full((k.N, k.K, k.mll), 7.0, device=dev)
    cost = torch.full((k.N, k.K), 7.0, device=dev)
    p = nat.ptr
    good = dict(acts=p(a), il=p(il), lab=p(lab), lens=p(lens), stride=0, C=k.C, N=k.N, T=k.T, K=k.K, L=k.mll, blank=k.blank, start=p(start), end=p(end),
                score=p(score), cost=p(cost), ws=p(ws), ws_bytes=need)

    def status(**kw):
        v = dict(good, **kw)
        return nat.lib().ocr_ctc_align(v['acts'], v['il'], v['lab'], v['lens'], v['stride'], v['C'], v['N'], v['T'], v['K'], v['L'], v['blank'],
                                       v['start'], v['end'], v['score'], v['cost'], v['ws'], v['ws_bytes'], nat.stream())
    for operand in ('acts', 'il', 'lab', 'lens', 'start', 'end', 'score', 'cost', 'ws'):
        assert status(**{operand: None}) == 2, operand
    assert status(blank=-1) == 2 and status(blank=k.C) == 2 and status(stride=1) == 2 and status(ws_bytes=need - 1) == 2
    assert status(K=0) == 2 and status(K=65537) == 2 and status(L=256) == 2 and status(C=16385) == 2 and status(N=65536) == 2 and status(T=0) == 2
    torch.cuda.synchronize()
    assert bool((start == 7).all()) and bool((end == 7).all()) and bool((score == 7.0).all()) and bool((cost == 7.0).all()) and not bool(ws.any())
    with pytest.raises(nat.NativeError):
        ops.ctc_align(a, il, lab, lens, blank=k.C, shared=True)
    assert status() == 0                      # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    want = _run(k, dev)
    for got, w in zip((start, end, score, cost), want):
        assert _same_bits(got.cpu().numpy(), w)


# ------------------------------------------------------------------------------------------------ trained logits
@pytest.fixture(scope='module')
def trained_engine(dev):
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    cfg.TRAIN.WEIGHT_DECAY = 1e-5
    eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=1, max_label_len=31)
    eng.load_arrays(fx.load_weights())
    return eng


def _argmax_runs(rows):
    """(label, first frame, last frame) of every run of equal non-blank per-frame arg-max classes (blank 0)."""
    frames = rows.argmax(axis=1).tolist()
    out, t = [], 0
    while t < len(frames):
        e = t
        while e + 1 < len(frames) and frames[e + 1] == frames[t]:
            e += 1
        if frames[t] != 0:
            out.append((frames[t], t, e))
        t = e + 1
    return out


@pytest.mark.parametrize('name', list(ac.TRAINED_BATCHES))
def test_trained_logits(trained_engine, name):
    """decode_spans(method='greedy') returns decode's strings, and their spans are the runs of the per-frame arg-max of the logits (the best path
    of all is the best path of the string it collapses to) for every sample whose float64 margin on those logits exceeds 2 x TRAINED_PATH_BOUND
    (8 x the float32 floor of the committed logits); at most 2 samples of a batch may lie under it.  Engine.align on the true labels: [] and +inf
    for V0's infeasible sample, confidences in (0, 1], path_cost at least Engine.score's cost of the same label within the two bounds."""
    eng = trained_engine
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, name)
    N = x.shape[0]
    truth = ac.trained_truth(name)[1]
    logits = eng.forward(x, sl).cpu().numpy()
    T = logits.shape[0]
    greedy = eng.decode(x, sl, method='greedy')
    strings, spans = eng.decode_spans(x, sl, method='greedy')
    assert strings == greedy and len(spans) == N
    under, lead = 0, np.inf
    for n in range(N):
        Tn = min(int(sl[n]), T)
        assert [c for c, _, _, _ in spans[n]] == greedy[n], n
        if not greedy[n]:
            continue
        path, _, _, _, _, lyx, skip = ac.align_rows(logits[:Tn, n], greedy[n], 0, np.float64)
        m = ac.margin_of(lyx, skip, path)
        lead = min(lead, m)
        if m <= 2 * ac.TRAINED_PATH_BOUND:
            under += 1
            continue
        assert [(c, s, e) for c, s, e, _ in spans[n]] == _argmax_runs(logits[:Tn, n]), (name, n)
        assert all(0.0 < conf <= 1.0 for _, _, _, conf in spans[n]), (name, n)
    print('%s: smallest float64 margin of a greedy string %.3e (2 x bound %.3e); %d samples under it' % (name, lead, 2 * ac.TRAINED_PATH_BOUND, under))
    assert under <= 2
    # the true labels
    tspans, cost = eng.align(x, sl, truth)
    costs = eng.score(x, sl, truth)[0]
    own = costs[np.arange(N), np.arange(N)]
    bad = np.array([len(t) + sc.lc.repeats(list(t)) > min(int(s), T) for t, s in zip(truth, sl)])
    assert bad.sum() == (1 if name == 'V0' else 0) and cost.dtype == np.float32 and cost.shape == (N,)
    assert np.all(cost[bad] == np.inf) and np.all(own[bad] == np.inf) and all(tspans[n] == [] for n in np.nonzero(bad)[0])
    slack = ac.TRAINED_PATH_BOUND + tt.COST_BOUND
    low = float((own[~bad].astype(np.float64) - cost[~bad]).max())
    confs = [conf for n in np.nonzero(~bad)[0] for _, _, _, conf in tspans[n]]
    print('%s: Engine.score cost - path_cost at most %.3e (bound %.3e); path_cost - cost up to %.3e; confidences %.4f .. %.4f'
          % (name, low, slack, float((cost[~bad].astype(np.float64) - own[~bad]).max()), min(confs), max(confs)))
    assert low <= slack
    assert all(0.0 < conf <= 1.0 for conf in confs)
    for n in np.nonzero(~bad)[0]:
        Tn = min(int(sl[n]), T)
        assert [c for c, _, _, _ in tspans[n]] == truth[n]
        assert ac.valid_alignment(truth[n], [s for _, s, _, _ in tspans[n]], [e for _, _, e, _ in tspans[n]], Tn), (name, n)
    # the lexicon decoder's strings, aligned from the same forward pass
    picked = eng.decode(x, sl, method='lexicon', lexicon=truth)
    lstrings, lspans = eng.decode_spans(x, sl, method='lexicon', lexicon=truth)
    assert lstrings == picked
    for n in range(N):
        assert [c for c, _, _, _ in lspans[n]] == picked[n], (name, n)
    # and through the prefix-tree route: the same strings, the same spans
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie
    tstrings, ttspans = eng.decode_spans(x, sl, method='lexicon', lexicon=LexiconTrie(truth, logits.shape[2]))
    assert tstrings == picked and ttspans == lspans
    with pytest.raises(ValueError):
        eng.decode_spans(x, sl, method='beam')
