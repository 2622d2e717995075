"""-m gpu: lexicon scoring under CTC (ctc_score.hip, ops.ctc_score, Engine.score, Engine.decode(method='lexicon')) against the float64 reference
on the cases of tests/ctc_score_cases.py, against the shipped loss, and on the trained fixture.  Bounds and their derivation: ctc_score_cases.py.

Measured on an MI355X (worst over the cases; the tests print every figure before they assert):

                                   float32 floor     bound (8 x)     device
    cost, absolute                 6.66e-4           5.33e-3         6.66e-4 (L255; lane128 5.60e-4, lane63 3.04e-4, saturated 1.59e-5, T <= 12: at most 9.0e-6)
    log_norm, absolute             6.32e-4           5.06e-3         6.32e-4 (L255; lane127 5.44e-4, T <= 12: at most 4.6e-6)
    against ops.ctc_loss on the same label (lane31, repeats, K5, dups): at most 3.8e-6, bound 2 x 5.33e-3
    trained logits (C1, V0): |Engine.score - ops.ctc_loss| on the true labels at most 3.8e-6 (bound 2 x 6.49e-5); the lexicon decode returns the
    truth on every sample the greedy decoder reads (8 of 8, 63 of 64); posterior of the truth within the lexicon 0.9997 .. 1.0000
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_score_cases as sc  # noqa: E402
import test_gpu_ctc_trained as tt  # noqa: E402

fx = tt.fx
pytestmark = pytest.mark.gpu
NAN = float('nan')
UNSET = -777          # best's fill: its NaN bytes would read -1, which is an answer


def _inputs(k, dev, per_sample=False):
    lab, lens = k.per_sample()[:2] if per_sample else k.packed()
    return tuple(torch.from_numpy(np.array(v)).to(dev) for v in (k.acts, k.il, lab, lens))          # (copies: the case's arrays are read-only)


def _native_run(k, dev, per_sample=False, want_best=True):
    """ocr_ctc_score itself on a workspace and outputs filled with NaN bytes -> costs, best, best_cost, log_norm (device tensors)."""
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    a, il, lab, lens = _inputs(k, dev, per_sample)
    need = ops.ctc_score_workspace_bytes(k.C, k.T, k.N)
    assert need == sc.workspace_bytes(k.C, k.T, k.N)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)          # 0xFFFFFFFF: a NaN in every float
    costs = torch.full((k.N, k.K), NAN, device=dev)
    best = torch.full((k.N,), UNSET, dtype=torch.int32, device=dev)
    bc, ln = torch.full((k.N,), NAN, device=dev), torch.full((k.N,), NAN, device=dev)
    p = nat.ptr
    opt = (p(best), p(bc), p(ln)) if want_best else (None, None, None)
    nat.call('ocr_ctc_score', p(a), p(il), p(lab) if lab.numel() else p(lens), p(lens), k.K if per_sample else 0, k.C, k.N, k.T, k.K, k.mll, k.blank,
             p(costs), *opt, p(ws), need, nat.stream())
    torch.cuda.synchronize()
    return costs, best, bc, ln


def _check(k, tag, costs, best, bc, ln):
    ref_c, ref_b, _, ref_n = sc.reference(k)
    c = costs.cpu().numpy()
    b, bcv, n = best.cpu().numpy(), bc.cpu().numpy(), ln.cpu().numpy()
    fin, nf = np.isfinite(ref_c), np.isfinite(ref_n)
    ok_shape = not np.isnan(c).any() and np.array_equal(np.isfinite(c), fin)
    ec = float(np.abs(c[fin].astype(np.float64) - ref_c[fin]).max()) if fin.any() and ok_shape else NAN
    en = float(np.abs(n[nf].astype(np.float64) - ref_n[nf]).max()) if nf.any() else 0.0
    msg = '%s %s: cost error %.3e (bound %.3e); log_norm error %.3e (bound %.3e); best %s (reference %s)' \
        % (k.name, tag, ec, sc.COST_BOUND, en, sc.NORM_BOUND, b.tolist()[:8], ref_b.tolist()[:8])
    print(msg)
    assert not np.isnan(c).any() and not np.isnan(bcv).any() and not np.isnan(n).any() and not (b == UNSET).any(), msg
    assert np.array_equal(np.isfinite(c), fin) and np.all(c[~fin] == np.inf), msg          # +inf exactly where the reference has it, never 0
    assert not fin.any() or ec <= sc.COST_BOUND, msg
    assert np.array_equal(b, ref_b), msg
    for i in range(k.N):
        want = c[i, b[i]] if b[i] >= 0 else np.float32(np.inf)
        assert bcv[i].tobytes() == np.float32(want).tobytes(), (msg, i)                     # best_cost == costs[n, best], bit for bit
    assert np.array_equal(np.isfinite(n), nf) and np.all(n[~nf] == -np.inf), msg
    assert en <= sc.NORM_BOUND, msg
    for a_, b_ in k.dups:
        assert np.array_equal(c[:, a_].view(np.uint32), c[:, b_].view(np.uint32)) and not (b == b_).any(), msg
    return ec, en


@pytest.mark.parametrize('name', [k.name for k in sc.cases()])
def test_cases_against_reference(dev, name):
    from lstm_ctc_ocr_amd import ops
    k = sc.case(name)
    assert ops.ctc_score_supported(k.C, k.T, k.mll, k.K)
    costs, best, bc, ln = _native_run(k, dev)
    _check(k, 'NaN-filled buffers', costs, best, bc, ln)
    # score only: the same costs, nothing else written
    c2, b2, bc2, ln2 = _native_run(k, dev, want_best=False)
    assert torch.equal(c2.view(torch.int32), costs.view(torch.int32)) and bool((b2 == UNSET).all()) and bool(torch.isnan(bc2).all() and torch.isnan(ln2).all())
    # the ops entry: allocates what it is not given, same bits
    a, il, lab, lens = _inputs(k, dev)
    c3, b3, bc3, ln3 = ops.ctc_score(a, il, lab, lens, blank=k.blank)
    c4, b4, bc4, ln4 = ops.ctc_score(a, il, lab, lens, blank=k.blank, want_best=False, costs=torch.full((k.N, k.K), NAN, device=dev))
    torch.cuda.synchronize()
    assert (b4, bc4, ln4) == (None, None, None)
    assert c3.shape == (k.N, k.K) and c3.dtype == torch.float32 and b3.dtype == torch.int32
    for got, want in ((c3, costs), (c4, costs), (b3, best), (bc3, bc), (ln3, ln)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('name', list(sc.PER_SAMPLE_CASES))
def test_per_sample_lexicon(dev, name):
    """sample_stride = K: the same strings in another order for every sample give the shared run's costs under the permutation, bit for bit."""
    from lstm_ctc_ocr_amd import ops
    k = sc.case(name)
    shared = _native_run(k, dev)[0].cpu().numpy()
    costs, best, bc, ln = _native_run(k, dev, per_sample=True)
    perm = k.per_sample()[2]
    c = costs.cpu().numpy()
    assert np.array_equal(c.view(np.uint32), np.take_along_axis(shared, perm, axis=1).view(np.uint32))
    b = best.cpu().numpy()
    ref_c, ref_b, _, ref_n = sc.reference(k)
    dup_of = {b_: a_ for a_, b_ in k.dups}
    for i in range(k.N):
        if ref_b[i] < 0:
            assert b[i] == -1
        else:          # the lowest position that holds the best string (a duplicate of it may come first in this sample's order)
            j = int(perm[i, b[i]])
            assert dup_of.get(j, j) == ref_b[i] and b[i] == min(p for p in range(k.K) if dup_of.get(int(perm[i, p]), int(perm[i, p])) == ref_b[i])
            assert bc.cpu().numpy()[i].tobytes() == c[i, b[i]].tobytes()
    nf = np.isfinite(ref_n)
    en = float(np.abs(ln.cpu().numpy()[nf] - ref_n[nf]).max()) if nf.any() else 0.0
    print('%s per-sample lexicon: log_norm error %.3e (bound %.3e)' % (name, en, sc.NORM_BOUND))
    assert en <= sc.NORM_BOUND
    a, il, lab, lens = _inputs(k, dev, per_sample=True)
    c2 = ops.ctc_score(a, il, lab, lens, blank=k.blank, per_sample=True, want_best=False)[0]
    assert torch.equal(c2.view(torch.int32), costs.view(torch.int32))
    with pytest.raises(ValueError):
        ops.ctc_score(a, il, lab, lens, blank=k.blank)          # a [N, K, L] lexicon passed as a shared one


@pytest.mark.parametrize('name', ['lane31', 'repeats', 'K5', 'dups'])
def test_against_the_shipped_loss(dev, name):
    """For a feasible (sample, candidate), ops.ctc_score and ops.ctc_loss(want_grad=False) of that label agree within the sum of the two bounds:
    both are float32 recursions on the same logits, each within COST_BOUND (8 x the float32 floor of these inputs) of the float64 reference."""
    from lstm_ctc_ocr_amd import ops
    k = sc.case(name)
    a, il, lab, lens = _inputs(k, dev)
    costs = ops.ctc_score(a, il, lab, lens, blank=k.blank, want_best=False)[0].cpu().numpy()
    ref = sc.reference(k)[0]
    worst = 0.0
    for j in range(k.K):
        L = len(k.lexicon[j])
        if L == 0 or not np.isfinite(ref[:, j]).any():
            continue          # (the loss kernels take labels of at least one character)
        flat = torch.tensor(k.lexicon[j] * k.N, dtype=torch.int32, device=dev)
        ll = torch.full((k.N,), L, dtype=torch.int32, device=dev)
        loss = ops.ctc_loss(a, flat, ll, il, max(k.mll, 1), k.blank, want_grad=False)[0].cpu().numpy()
        fin = np.isfinite(ref[:, j])
        assert np.all(loss[~fin] == 0) and np.all(costs[~fin, j] == np.inf)          # the two conventions for an infeasible label
        worst = max(worst, float(np.abs(loss[fin].astype(np.float64) - costs[fin, j]).max()))
    print('%s: worst |ctc_score - ctc_loss| %.3e (bound %.3e)' % (name, worst, 2 * sc.COST_BOUND))
    assert worst <= 2 * sc.COST_BOUND


def test_refused_inputs_launch_nothing(dev):
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    k = sc.case('K5')
    a, il, lab, lens = _inputs(k, dev)
    need = ops.ctc_score_workspace_bytes(k.C, k.T, k.N)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    costs = torch.full((k.N, k.K), 7.0, device=dev)
    best = torch.full((k.N,), 7, dtype=torch.int32, device=dev)
    bc, ln = torch.full((k.N,), 7.0, device=dev), torch.full((k.N,), 7.0, device=dev)
    p = nat.ptr
    good = dict(acts=p(a), il=p(il), lab=p(lab), lens=p(lens), stride=0, C=k.C, K=k.K, L=k.mll, blank=k.blank, costs=p(costs), best=p(best), ws=p(ws),
                ws_bytes=need)

    def status(**kw):
        v = dict(good, **kw)
        return nat.lib().ocr_ctc_score(v['acts'], v['il'], v['lab'], v['lens'], v['stride'], v['C'], k.N, k.T, v['K'], v['L'], v['blank'], v['costs'],
                                       v['best'], p(bc), p(ln), v['ws'], v['ws_bytes'], nat.stream())
    for operand in ('acts', 'il', 'lab', 'lens', 'costs', 'ws', 'best'):
        assert status(**{operand: None}) == 2, operand
    assert status(blank=-1) == 2 and status(blank=k.C) == 2 and status(stride=1) == 2 and status(ws_bytes=need - 1) == 2
    assert status(K=0) == 2 and status(K=65537) == 2 and status(L=256) == 2 and status(C=16385) == 2
    torch.cuda.synchronize()
    assert bool((costs == 7.0).all()) and bool((best == 7).all()) and bool((bc == 7.0).all()) and bool((ln == 7.0).all()) and not bool(ws.any())
    with pytest.raises(nat.NativeError):
        ops.ctc_score(a, il, lab, lens, blank=k.C)
    assert status() == 0                      # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    _check(k, 'after the refusals', costs, best, bc, ln)


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


def _truth_of(d, name):
    out, pos = [], 0
    for n in d[name + '/label_len']:
        out.append(d[name + '/labels'][pos:pos + n].tolist())
        pos += n
    return out


def _edits(label, C, rng):
    """Three strings at edit distance 1 from a label: one class replaced, one character dropped, one character put in."""
    i = int(rng.randint(len(label)))
    sub = list(label); sub[i] = 1 + (label[i] - 1 + int(rng.randint(1, C - 1))) % (C - 1)
    cut = label[:i] + label[i + 1:]
    ins = label[:i] + [int(rng.randint(1, C))] + label[i:]
    assert sub != label and len(cut) == len(label) - 1 and len(ins) == len(label) + 1
    return [sub, cut, ins]


@pytest.mark.parametrize('name', ['C1', 'V0'])
def test_trained_logits(trained_engine, name):
    """The lexicon: the batch's true labels, then three strings at edit distance 1 from each; shared by all samples.  Engine.decode(method='lexicon')
    returns the truth for every sample the greedy decoder reads correctly, and Engine.score's costs of the true labels are the CTC costs of the
    step (ops.ctc_loss on the same logits) within the two bounds: both are float32 recursions on trained logits, whose floor
    tests/test_gpu_ctc_trained.py measures (COST_BOUND = 8 x 8.11e-6 each)."""
    from lstm_ctc_ocr_amd import ops
    eng = trained_engine
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, name)
    N = x.shape[0]
    truth = _truth_of(d, name)
    logits = eng.forward(x, sl)
    C = logits.shape[2]
    rng = np.random.RandomState(77)
    lexicon = [list(t) for t in truth] + [e for t in truth for e in _edits(list(t), C, rng)]
    assert len(lexicon) == 4 * N
    greedy = eng.decode(x, sl, method='greedy')
    picked = eng.decode(x, sl, method='lexicon', lexicon=lexicon)
    costs, best, best_cost, log_norm = eng.score(x, sl, lexicon)
    assert costs.shape == (N, 4 * N) and costs.dtype == np.float32 and best.dtype == np.int32 and best_cost.shape == (N,) and log_norm.shape == (N,)
    assert eng._lexicon[0] is lexicon                                   # packed once for the two calls
    read = [i for i in range(N) if greedy[i] == truth[i]]
    print('%s: greedy reads %d of %d; lexicon decode returns the truth on %d of those and on %d of all'
          % (name, len(read), N, sum(picked[i] == truth[i] for i in read), sum(picked[i] == truth[i] for i in range(N))))
    assert len(read) >= 0.9 * N
    for i in read:
        assert picked[i] == truth[i], (i, picked[i], truth[i])
    assert [[v for v in lexicon[b]] if b >= 0 else [] for b in best] == picked
    fl, lld, sld = (torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(logits.device) for v in (labels, ll, sl))
    loss = ops.ctc_loss(logits, fl, lld, sld, int(ll.max()), 0, want_grad=False)[0].cpu().numpy()
    own = costs[np.arange(N), np.arange(N)]
    bad = np.array([len(t) + sc.lc.repeats(list(t)) > min(int(s), logits.shape[0]) for t, s in zip(truth, sl)])
    assert bad.sum() == (1 if name == 'V0' else 0)
    assert np.all(own[bad] == np.inf) and np.all(loss[bad] == 0)         # V0's infeasible sample: +inf here, 0 from the loss
    err = float(np.abs(own[~bad].astype(np.float64) - loss[~bad]).max())
    post = np.exp(-own[~bad].astype(np.float64) - log_norm[~bad])
    print('%s: worst |Engine.score - ops.ctc_loss| on the true labels %.3e (bound %.3e); posterior of the truth within the lexicon %.4f .. %.4f'
          % (name, err, 2 * tt.COST_BOUND, post.min(), post.max()))
    assert err <= 2 * tt.COST_BOUND
    assert np.all(post <= 1 + 1e-5) and np.all(np.isfinite(log_norm))
    with pytest.raises(ValueError):
        eng.decode(x, sl, method='lexicon')
