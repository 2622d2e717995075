"""-m gpu: the lowered network end-to-end against the CPU oracle on the same weights and batch.

Bars (north star): greedy-decoded label sequences identical; CTC loss within 1e-3 relative.  The oracle runs
with sim_bf16=True (rounding at the points where the device stores bf16) so only fp32 summation order differs;
the fp32-oracle distance is printed for information.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lstm_ctc_ocr_amd.config import cfg
from lstm_ctc_ocr_amd.engine import Engine
from lstm_ctc_ocr_amd.models import get_network
from oracle import decode as odec
from oracle import graph as og


def make_batch(N, W, Lmin, Lmax, seed, varlen=False):
    rng = np.random.RandomState(seed)
    x = rng.rand(N, W, 32).astype(np.float32)
    widths = rng.randint(W // 2, W + 1, N) if varlen else np.full(N, W)
    widths[0] = W
    for n in range(N):
        x[n, widths[n]:] = 0.0                       # right padding with 0 (gen.py:62)
    sl = (widths // 4 - 1).astype(np.int32)
    ll = rng.randint(Lmin, Lmax + 1, N).astype(np.int32)
    labels = rng.randint(1, 63, size=int(ll.sum())).astype(np.int32)
    return x, labels, ll, sl


@pytest.fixture(scope="module")
def engine(dev):
    cfg.TRAIN.WEIGHT_DECAY = 1e-5
    cfg.TRAIN.LEARNING_RATE = 1e-4
    cfg.TRAIN.SOLVER = 'Adam'
    return Engine(get_network('LSTM_train'), device='cuda:0', seed=3)


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12))


@pytest.mark.parametrize("N,W,varlen", [(8, 88, False), (6, 64, True)])
def test_forward_parity(engine, N, W, varlen):
    x, labels, ll, sl = make_batch(N, W, 2, 4, 1, varlen)
    params = {k: torch.from_numpy(v) for k, v in engine.state_arrays().items()}
    logits = engine.forward(x, sl).float().cpu()
    ref, inter = og.forward(params, torch.from_numpy(x), sl.tolist(), sim_bf16=True, keep=True)
    sp = engine.plan(N, W)
    for op in engine.ops:
        if op.name in inter and op.name != 'logits' and op.node.op == 'conv' and getattr(op, 'fused_pool', None) is None:
            got = op.y(sp).float().cpu().reshape(inter[op.name].shape)
            print(op.name, 'rel err', relerr(got, inter[op.name]))
    for n in range(N):
        t = int(sl[n])
        assert float((logits[:t, n] - ref[:t, n]).abs().max()) < 5e-3
    ref32 = og.forward(params, torch.from_numpy(x), sl.tolist(), sim_bf16=False)
    print('max |logits(bf16 path) - logits(fp32 oracle)| =', float((logits - ref32).abs().max()))
    dec = engine.decode(x, sl, method='greedy')
    # kernel-level: bit-exact best path of the device's own logits, and the reference's beam decode (blank C-1, zeros stripped)
    assert dec == odec.greedy_decode(logits.numpy(), sl)
    assert engine.decode(x, sl, method='beam') == odec.reference_decode(logits.numpy(), sl, beam_width=100)
    # end-to-end string identity (device vs fp32 oracle, every sample) is asserted on trained weights: test_trained_fixture.py


def _oracle_grads(params, x, labels, ll, sl, wd, sim, grad_rounding=True):
    og.SIM_GRAD_ROUNDING = grad_rounding
    try:
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        total, ctc, _ = og.loss_fn(leaves, torch.from_numpy(x), labels, ll, sl.tolist(), wd, sim_bf16=sim)
        total.backward()
    finally:
        og.SIM_GRAD_ROUNDING = True
    grads = {}
    for k, v in leaves.items():
        g = v.grad if v.grad is not None else torch.zeros_like(v)
        grads[k] = g - wd * params[k] if og.REGULARISED(k) else g          # the device adds wd * w inside the optimiser kernel
    return grads, float(ctc.detach())


# Bars for |g_dev - g_oracle|_2 / |g_oracle|_2, per tensor, against the bf16-simulating oracle (rounds values AND activation
# gradients where the device stores bf16: oracle/graph.py qa()).  Measured on MI355X in round 2 (N = 8, W = 88, random init;
# printed by the test): 5e-5 .. 9e-4 for the FC / LSTM / conv5 tensors, then growing smoothly through the conv stack —
# conv4_2 6.9e-3, conv4_1 8.7e-3, conv3_2 1.1e-2, conv3_1 1.3e-2, conv2 1.6e-2, conv1 2.0e-2.  Switching the oracle's
# gradient rounding off changes these numbers by < 3 % of their value, i.e. the residual is NOT storage noise of the gradients:
# it is max-pool / ReLU routing that flips where device and oracle activations differ in the last bf16 bit (each flip moves a
# whole gradient element), the same mechanism that puts the bf16-simulating oracle itself 2.4e-2 .. 9.9e-2 away from the
# pure-fp32 oracle on these tensors.  Bars = 2x measured.  A wiring error (wrong tap, missed mask or residual branch, missing
# exchange) is O(1) here; errors of a few percent inside ONE kernel are caught where routing cannot flip — the kernel-level
# tests feed identical inputs to kernel and reference (test_gpu_kernels.py: conv fwd/dgrad/wgrad, BN, pools, LSTM, <= 1e-2).
GRAD_L2_BAR = {'default': 4e-2, 'conv4_1/weights': 2e-2, 'conv4_1/conv4_1/beta': 2e-2, 'conv4_1/conv4_1/gamma': 2e-2,
               'conv4_2/weights': 1.5e-2, 'conv4_2/conv4_2/beta': 5e-3, 'conv4_2/conv4_2/gamma': 2e-3,
               'conv5/weights': 2e-3, 'conv5/biases': 2e-3, 'logits/weights': 1.5e-3, 'logits/biases': 5e-4,
               'logits/fw/weights': 2e-3, 'logits/fw/biases': 2e-3, 'logits/bw/weights': 2e-3, 'logits/bw/biases': 2e-3}
GRAD_L2_BAR_FP32 = 0.2       # distance to the pure-fp32 oracle (dominated by the forward rounding): measured <= 9.9e-2


def oracle_step(params, x, labels, ll, sl, wd=1e-5):
    """The oracle's gradients and CTC losses for one batch: bf16-simulating (with / without gradient rounding) and pure fp32."""
    g_sim, ctc_ref = _oracle_grads(params, x, labels, ll, sl, wd, sim=True)
    g_sim_nr, _ = _oracle_grads(params, x, labels, ll, sl, wd, sim=True, grad_rounding=False)
    g_f32, ctc_f32 = _oracle_grads(params, x, labels, ll, sl, wd, sim=False)
    return g_sim, g_sim_nr, g_f32, ctc_ref, ctc_f32


def check_step_against_oracle(engine, sp, oracle):
    """Loss and raw gradients of the forward + backward pass that just ran on plan `sp` against oracle_step()'s answer, by the bars above
    (shared with test_gpu_kernel_generations.py, which runs the same step under the other engine generations)."""
    g_sim, g_sim_nr, g_f32, ctc_ref, ctc_f32 = oracle
    ctc_dev = float(sp.costs.cpu().numpy().mean())
    assert abs(ctc_dev - ctc_ref) / ctc_ref < 1e-3, (ctc_dev, ctc_ref)
    assert abs(ctc_dev - ctc_f32) / ctc_f32 < 1e-3, (ctc_dev, ctc_f32)          # north-star bar against the fp32 graph
    l2 = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
    bad = []
    for name in engine.specs:
        g = engine.grad(name).cpu()
        if name in ('conv4_1/biases', 'conv4_2/biases'):
            # a bias in front of batch-norm has a mathematically zero gradient (BN removes the mean): both sides
            # hold rounding noise only — require it to be negligible against the layer's weight gradient
            scale = float(g_sim[name.replace('biases', 'weights')].abs().max())
            print('grad %-28s |noise| %.3e (weight-grad scale %.3e)' % (name, float(g.abs().max()), scale))
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) < scale
            continue
        if float(g_sim[name].abs().max()) < 1e-9:
            assert float(g.abs().max()) < 1e-5, name
            continue
        e_sim, e_nr, e_f32 = l2(g, g_sim[name]), l2(g, g_sim_nr[name]), l2(g, g_f32[name])
        mx = float((g - g_sim[name]).abs().max() / g_sim[name].abs().max())
        print('grad %-28s L2-rel vs bf16sim %.3e (no grad rounding %.3e) vs fp32 %.3e | max-rel vs bf16sim %.3e'
              % (name, e_sim, e_nr, e_f32, mx))
        if not (e_sim < GRAD_L2_BAR.get(name, GRAD_L2_BAR['default']) and e_f32 < GRAD_L2_BAR_FP32):
            bad.append((name, e_sim, e_f32))
    assert not bad, bad


def test_train_step_parity(engine):
    N, W = 8, 88
    x, labels, ll, sl = make_batch(N, W, 2, 4, 2)
    params = {k: torch.from_numpy(v) for k, v in engine.state_arrays().items()}
    oracle = oracle_step(params, x, labels, ll, sl)
    # run forward+backward only (no optimiser) and compare raw gradients
    sp = engine.plan(N, W)
    engine._bind(sp, x, sl, labels, ll)
    engine._run(sp, 'fb')
    torch.cuda.synchronize()
    check_step_against_oracle(engine, sp, oracle)


@pytest.mark.parametrize("N,W", [(8, 88), (64, 256)])
def test_deferred_weight_gradient_reduction_is_bit_identical(dev, monkeypatch, N, W):
    """OCR_W9_DEFER (default on): the 3x3 weight-gradient slab kernels leave their reductions pending and ONE launch at the end of
    the backward body adds all layers' slabs — same per-element summation order as the per-layer reduce kernels, so the conv
    weight and bias gradients must be bit-identical to the undeferred schedule (and to themselves under the two-graph DP split)."""
    x, labels, ll, sl = make_batch(N, W, 2, 4, 7)
    names = ['conv%s/%s' % (l, k) for l in ('2', '3_1', '3_2', '4_1', '4_2') for k in ('weights', 'biases')]

    def grads(defer, split, flush_mb='0'):
        monkeypatch.setenv('OCR_W9_DEFER', defer)
        monkeypatch.setenv('OCR_W9_FLUSH_MB', flush_mb)                  # '0': ONE reduction per backward body; the default flushes after 80 MB of slabs
        monkeypatch.setenv('OCR_W9_OVERLAP', '1' if split else '0')      # the reduction beside the rest of the chain, too
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3)
        assert eng.defer_w9 == (defer == '1')
        sp = eng.plan(N, W)
        eng._bind(sp, x, sl, labels, ll)
        if split:
            eng._run_split(sp)()
        else:
            eng._run(sp, 'fb')
            eng._run(sp, 'fb')                       # the second call replays the captured graph
        torch.cuda.synchronize()
        assert not sp.w9_pending
        if defer == '1':
            assert sum(k.endswith('/w9ws') for k in sp.buf) == 5
            if flush_mb == '0':
                assert len(sp.w9_tables) == (2 if split else 1)
            elif (N, W) == (64, 256) and not split:
                assert len(sp.w9_tables) == 2        # 37.8 + 37.8 + 37.8 MB of slabs (conv4_2, conv4_1, conv3_2) reduced while hot, conv3_1 + conv2 at the end
        return {n: eng.grad(n).clone() for n in names}

    base = grads('0', False)
    for split, flush_mb in ((False, '0'), (True, '0'), (False, '80'), (True, '80')):
        g = grads('1', split, flush_mb)
        for n in names:
            assert float(base[n].abs().max()) > 0 and torch.equal(g[n], base[n]), (n, split, flush_mb)


def test_round4_fusions_match_the_unfused_schedule(dev, monkeypatch):
    """Round 4 moved work into neighbouring kernels (batch-norm statistics / pool / backward sums in convolution write-outs, two plain weight-
    gradient products as one gemm_tn3 launch, slab reductions flushed after 80 MB, the gradient clear and the pool routing codes on the conv1
    launch).  With every one of them switched off the engine runs round 3's schedule: same loss, same gradients up to fp32 summation order
    (the statistics are summed per 256-pixel tile instead of per row block, which moves a few bf16 roundings downstream of them)."""
    N, W = 64, 128
    x, labels, ll, sl = make_batch(N, W, 2, 5, 21, varlen=True)
    off = dict(OCR_FUSE_BN_STATS='0', OCR_FUSE_BN_POOL='0', OCR_FUSE_BN_BWD='0', OCR_TN_JOBS='0', OCR_FUSE_ZERO='0', OCR_CONV1_CODES='0',
               OCR_W9_FLUSH_MB='0', OCR_FUSE_RINGFILL='0')

    def run(env):
        for k in off:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=5)
        sp = eng.plan(N, W)
        eng._bind(sp, x, sl, labels, ll)
        eng._run(sp, 'fb')
        eng._run(sp, 'fb')                            # the captured graph
        torch.cuda.synchronize()
        active = dict(stats=sum(1 for v in getattr(sp, 'bn_stat_rows', {}).values() if v), bwd=sum(1 for v in getattr(sp, 'bn_bwd_rows', {}).values() if v),
                      pool=sum(1 for op in eng.ops if getattr(op, 'bn_pool', None) is not None), codes=sum(k.endswith('/codes') for k in sp.buf),
                      rings=int(bool(getattr(sp, 'rings_armed', False))))
        # the LSTM hand-off blocks' error words: 0 where the launches prepared their own blocks, -1 (untouched all-ones) where the conv1 launch did; 1 = time-out
        assert [int(w[-1]) for w in sp.lstm_sync] == [-1 if active['rings'] else 0] * len(sp.lstm_sync)
        return {n: eng.grad(n).clone() for n in eng.specs}, float(sp.costs.double().mean()), active

    g0, c0, a0 = run(off)
    g1, c1, a1 = run({})
    assert a0 == dict(stats=0, bwd=0, pool=0, codes=0, rings=0) and a1 == dict(stats=2, bwd=1, pool=1, codes=1, rings=1), (a0, a1)
    assert abs(c1 - c0) < 1e-5 * abs(c0)
    for n in g0:
        ref = g0[n].double()
        if n in ('conv4_1/biases', 'conv4_2/biases'):                  # mathematically zero (batch norm removes the mean): rounding noise
            continue
        e = float((g1[n].double() - ref).norm() / ref.norm().clamp_min(1e-30))
        assert e < 2e-3, (n, e)


def test_lstm_bias_job_follows_the_updated_parameter(dev):
    """The LSTM bias permutation is a job of the re-pack launch behind the optimiser: after training steps the packed bias is the
    permutation (u / 16) * 64 + g * 16 + u % 16 of the UPDATED gate-major TF vector."""
    N, W = 8, 88
    x, labels, ll, sl = make_batch(N, W, 2, 4, 11, varlen=True)
    eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3)
    lstm = [op for op in eng.ops if hasattr(op, 'whT')][0]
    bias0 = lstm.bias.clone()
    eng.setup_optimizer('Adam', 1e-3)
    for _ in range(3):
        eng.train_step(x, labels, ll, sl)
    U = 256
    want = eng.param('logits/fw/biases').view(4, U // 16, 16).permute(1, 0, 2).reshape(-1)
    assert torch.equal(lstm.bias[:4 * U], want) and not torch.equal(lstm.bias, bias0)


def test_lagged_loss_reports_are_the_right_iterations(dev):
    """with the loss of iteration k read while k + 1 runs (report_async / report_wait, the training loop's default) the
    engine's own every-64-steps time-out check used to take the ring slot a pending handle still pointed at, so one logged loss in 64
    was the next step's.  More than 64 lagged iterations must give exactly the losses of the loop that waits at once."""
    N, W, steps = 8, 88, 70
    batches = [make_batch(N, W, 2, 4, 100 + i, varlen=True) for i in range(4)]

    def run(lagged):
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3)
        eng.setup_optimizer('Momentum', 1e-3)           # (no atomics-order dependence worth mentioning over 70 steps at this lr)
        out, pending = [], None
        for it in range(steps):
            x, labels, ll, sl = batches[it % len(batches)]
            if not lagged:
                out.append(eng.train_step(x, labels, ll, sl, fetch_loss=True))
                continue
            eng.train_step(x, labels, ll, sl, fetch_loss=False)
            h = eng.report_async()
            if pending is not None:
                out.append(eng.report_wait(pending))
            pending = h
        if pending is not None:
            out.append(eng.report_wait(pending))
        return np.array(out)

    a, b = run(False), run(True)
    assert len(a) == len(b) == steps
    # same kernels, same order: the two loops differ only in WHEN the host reads; fp32-atomics order noise of the plain GEMM weight
    # gradients is far below the step-to-step change of the loss
    assert np.allclose(a, b, rtol=2e-3), np.abs(a - b).max()
    step_change = np.abs(np.diff(a)).min()
    assert np.abs(a - b).max() < 0.25 * step_change + 1e-6 or np.allclose(a, b, rtol=1e-4)
    with pytest.raises(RuntimeError):                    # slot ownership is enforced: a fifth outstanding handle is refused
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3)
        x, labels, ll, sl = batches[0]
        eng.train_step(x, labels, ll, sl, fetch_loss=False)
        for _ in range(Engine.REPORT_SLOTS + 1):
            eng.report_async()


def test_training_reduces_loss_and_matches_oracle_update(engine):
    N, W = 8, 88
    x, labels, ll, sl = make_batch(N, W, 2, 4, 3)
    params = {k: torch.from_numpy(v) for k, v in engine.state_arrays().items()}
    state = {}
    new, total, ctc, norm, _ = og.train_step(params, state, (torch.from_numpy(x), labels, ll, sl.tolist()), 1e-4, 1e-5,
                                             sim_bf16=True)
    engine.setup_optimizer('Adam', 1e-4)
    loss0 = engine.train_step(x, labels, ll, sl)
    assert abs(loss0 - total) / total < 1e-3
    assert abs(engine.last_gnorm - norm) / norm < 3e-2
    # first Adam step is lr * sign(g): compare the update direction on the big tensors
    after = engine.state_arrays()
    for name in ('conv4_2/weights', 'logits/fw/weights', 'logits/weights'):
        d_dev = torch.from_numpy(after[name]) - params[name]
        d_ref = new[name] - params[name]
        agree = float((torch.sign(d_dev) == torch.sign(d_ref)).float().mean())
        print(name, 'update sign agreement', agree)
        assert agree > 0.97
    losses = [loss0] + [engine.train_step(x, labels, ll, sl) for _ in range(30)]
    print('losses', losses[0], losses[-1])
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------- beyond the reference: config 5
DEEP_GRAD_L2_BAR = 0.15       # tightened from the measured values once the oracle rounds activation gradients too (see below)


def test_residual_stacked_network_parity(dev):
    """BASELINE configs[4] in miniature: residual BasicBlocks (add / relu / 1x1 projection, tensors with two consumers),
    two stacked BiLSTMs and a 96-class alphabet, lowered by the same engine and checked against the plan-walking oracle."""
    from lstm_ctc_ocr_amd import models
    from oracle import plan_exec
    old = (cfg.NCLASSES, cfg.TRAIN.NUM_LAYERS, cfg.TRAIN.WEIGHT_DECAY)
    cfg.NCLASSES, cfg.TRAIN.NUM_LAYERS, cfg.TRAIN.WEIGHT_DECAY = 96, 2, 1e-5
    try:
        class Tiny(models.RESNET_train):
            blocks, widths = (1, 1, 1, 1), (64, 128, 128, 256)
        net = Tiny()
        eng = Engine(net, device='cuda:0', seed=5)
        N, W = 16, 96
        x, labels, ll, sl = make_batch(N, W, 2, 3, 7)
        labels = (labels % 94) + 1
        params = {k: torch.from_numpy(v) for k, v in eng.state_arrays().items()}
        logits = eng.forward(x, sl).float().cpu()
        ref = plan_exec.forward(net, params, torch.from_numpy(x), sl.tolist(), sim_bf16=True)
        assert tuple(logits.shape) == (W // 4 - 1, N, 96)
        assert float((logits - ref).abs().max()) < 1e-2, float((logits - ref).abs().max())
        # gradients through the residual DAG (multi-consumer accumulation) against autograd on the oracle
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        lg = plan_exec.forward(net, leaves, torch.from_numpy(x), sl.tolist(), sim_bf16=True)
        costs = og._CTC.apply(lg, labels.astype(np.int32), ll.astype(np.int32), np.asarray(sl, np.int32))
        costs.mean().backward()
        sp = eng.plan(N, W)
        eng._bind(sp, x, sl, labels, ll)
        eng._run(sp, 'fb')
        torch.cuda.synchronize()
        assert abs(float(sp.costs.cpu().numpy().mean()) - float(costs.mean())) / float(costs.mean()) < 2e-3
        bad = []
        for name in ('logits/weights', 'logits/fw/weights', 'logits/stack0/fw/weights', 'conv5/weights', 'res4_0_b/weights',
                     'res4_0_a/weights', 'res4_0_proj/weights', 'res3_0_b/weights', 'res3_0_a/weights', 'res2_0_b/weights',
                     'res2_0_a/weights', 'res2_0_proj/weights', 'res1_0_b/weights', 'res1_0_a/weights', 'conv1/weights'):
            g, r = eng.grad(name).cpu(), leaves[name].grad
            e = float((g - r).abs().max()) / float(r.abs().max())
            e2 = float((g - r).norm() / r.norm())
            cos = float((g * r).sum() / (g.norm() * r.norm()))
            print('grad %-28s max-rel %.3e  l2-rel %.3e  cos %.5f' % (name, e, e2, cos))
            # The oracle back-propagates in fp32; the device stores every activation gradient as bf16.  Each batch-norm
            # backward subtracts the per-channel mean and the x-hat component of dz, which amplifies that rounding noise
            # by |dz| / |dz - projections|: measured ~1 % L2 per BN layer (0.2-0.4 % for the BN-free tail), growing smoothly
            # from the loss to conv1 (11 BN layers here).  A structural error (missed residual contribution, wrong mask,
            # wrong halo) would show as O(1), so the bars are: L2-relative < 15 %, cosine > 0.99, and SGD still converges.
            if not (e2 < DEEP_GRAD_L2_BAR and cos > 0.99):
                bad.append((name, e2, cos))
        assert not bad, bad
        eng.setup_optimizer('Adam', 1e-4)
        l0 = eng.train_step(x, labels, ll, sl)
        l1 = [eng.train_step(x, labels, ll, sl) for _ in range(15)][-1]
        assert l1 < l0
    finally:
        cfg.NCLASSES, cfg.TRAIN.NUM_LAYERS, cfg.TRAIN.WEIGHT_DECAY = old


def test_lstm_handoff_timeout_drops_the_update_instead_of_applying_it(dev, capsys):
    """Round 5: the persistent LSTM kernels bound their inter-workgroup waits and report through an error word (1 = results invalid).  Seen twice
    in ~20 runs of the live-pipeline loop (tools/cli_throughput.py; also with round 4's kernels) — before, the garbage gradient was applied and the run died
    on the report one step later.  Now the optimiser step is guarded on the device: with an error word at 1 neither parameters, nor moments, nor
    the step count / bias-correction powers move, scalars[73] counts the dropped step, the report warns and returns NaN, and the next step is normal."""
    eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3, use_graphs=False)
    eng.setup_optimizer('Adam', 1e-3)
    x, labels, ll, sl = make_batch(8, 88, 2, 4, 2)
    l0 = eng.train_step(x, labels, ll, sl)
    assert np.isfinite(l0) and float(eng.scalars[6]) == 1.0 and float(eng.scalars[73]) == 0.0
    before, m1, m2, sc = eng.params.clone(), eng.state1.clone(), eng.state2.clone(), eng.scalars.clone()
    sp = eng.plan(8, 88)
    eng._bind(sp, x, sl, labels, ll)
    eng._run(sp, 'fb')
    assert len(sp.lstm_sync) == 2
    sp.lstm_sync[0][-1] = 1                                  # fault injection: "the forward launch's wait expired"
    eng.optimizer_step(sp)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before) and torch.equal(eng.state1, m1) and torch.equal(eng.state2, m2)
    assert float(eng.scalars[6]) == 1.0 and torch.equal(eng.scalars[2:7], sc[2:7])          # lr, lr_t, beta powers, step count untouched
    assert float(eng.scalars[72]) == 1.0 and float(eng.scalars[73]) == 1.0
    eng.last_plan = sp
    v = eng.report_wait(eng.report_async())
    assert np.isnan(v) and 'dropped on the device' in capsys.readouterr().err
    # a SECOND report that covers the same dropped step (the every-64-steps watchdog's, queued by train_step beside the loop's own) is a NaN too —
    # the decision is the step's own scalars[72], exported by the report kernel, not a comparison of the global counter
    assert np.isnan(eng.report_wait(eng.report_async(_slot='watch'), update_mirrors=False))
    l2 = eng.train_step(x, labels, ll, sl)                   # the next step is a normal one
    assert np.isfinite(l2) and float(eng.scalars[6]) == 2.0 and float(eng.scalars[72]) == 0.0 and float(eng.scalars[73]) == 1.0
    assert not torch.equal(eng.params, before)
    # two dropped steps in a row, their reports read one step late (OCR_LOSS_LAG = 1): each is its own step's
    handles = []
    for word in (0, 1):
        eng._bind(sp, x, sl, labels, ll)
        eng._run(sp, 'fb')
        sp.lstm_sync[word][-1] = 1
        eng.optimizer_step(sp)
        eng.last_plan = sp
        handles.append(eng.report_async())
    assert all(np.isnan(eng.report_wait(h)) for h in handles)
    assert eng.guard_counters() == (3, 3) and float(eng.scalars[6]) == 2.0
    l3 = eng.train_step(x, labels, ll, sl)
    assert np.isfinite(l3) and float(eng.scalars[6]) == 3.0
    # without the guard (several ranks, or OCR_LSTM_TIMEOUT_GUARD=0) the report raises as before
    sp.lstm_sync[1][-1] = 1
    eng.last_plan = sp
    from lstm_ctc_ocr_amd._native import NativeError
    with pytest.raises(NativeError):
        eng.report_wait(eng.report_async())
