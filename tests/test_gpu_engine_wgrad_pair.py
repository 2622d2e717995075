"""The engine's paired slab launch (OCR_W9_PAIR, default on: conv3_1's weight-gradient kernel waits and runs inside conv2's launch) against
the same engine with the switch off: one training step of LSTM_train must leave the SAME gradient buffer, bit for bit — the paired launch
writes the slabs the two launches write, and the reductions join the pending list in the same order — with one slab launch fewer
per pair.  (At batch 8 the plan holds a second pair beside conv3_1 + conv2: conv4_1 has 22 or 25 columns there, fewer than a plane-layout
step of H = 4, so it runs wgrad9_kernel on 32 workgroups and takes conv4_2's; at the 64 x 256 product shape conv3_1 + conv2 is the only
pair.)  Once more under the multi-graph data-parallel schedule (two emulated ranks on one GPU): the early backward body, where conv3_1 +
conv2 lie, is a graph of its own behind the exchange of the late gradients, and a gradient still held when a body ends would reach the
exchange or the optimiser unreduced."""
import io
import os
import sys

import numpy as np
import pytest
import torch

from lstm_ctc_ocr_amd import _native as nat
from lstm_ctc_ocr_amd.config import cfg
from lstm_ctc_ocr_amd.engine import Engine
from lstm_ctc_ocr_amd.models import get_network

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
from launch_trace import Traced  # noqa: E402

pytestmark = pytest.mark.gpu

SINGLE, PAIR, REDUCE = 'ocr_conv3x3_wgrad_defer_bf16', 'ocr_conv3x3_wgrad_pair_defer_bf16', 'ocr_wgrad9_reduce_jobs'


def _batch(N, W):
    rng = np.random.RandomState(7)
    T = W // 4 - 1
    L = max(1, min(4, T // 3))
    x = rng.rand(N, W, cfg.NUM_FEATURES).astype(np.float32)
    labels = rng.randint(1, cfg.NCLASSES - 1, N * L).astype(np.int32)
    return x, labels, np.full(N, L, np.int32), np.full(N, T, np.int32)


def _engine(monkeypatch, pair, out, **kw):
    monkeypatch.setenv('OCR_W9_PAIR', pair)
    monkeypatch.setattr(nat, '_lib', Traced(nat.lib(), nat._SIGS, out))          # tools/launch_trace.py's hook: one line per native call
    return Engine(get_network('LSTM_train'), device='cuda:0', seed=5, **kw)


def _calls(out):
    names = [line.split('(')[0] for line in out.getvalue().splitlines()]
    return {k: names.count(k) for k in (SINGLE, PAIR, REDUCE)}


@pytest.mark.parametrize("W", [88, 100])        # 100: conv3_1 has 25 columns, no multiple of a step's 16 — and M % 128 != 0: wgrad9_kernel's body twice
def test_one_step_same_gradients_one_launch_less(dev, monkeypatch, W):
    N = 8
    x, labels, ll, sl = _batch(N, W)
    res = {}
    for pair in ('0', '1'):
        out = io.StringIO()
        with monkeypatch.context() as m:
            eng = _engine(m, pair, out, use_graphs=False)
            assert eng.w9_pair == (pair == '1')
            sp = eng.plan(N, W)
            name = {op.key: op.name for op in eng.ops}
            held = {name[a]: name[b] for a, b in sp.w9_hold_for.items()}          # waiting layer -> the layer whose launch it joins
            print('held layers:', held)
            assert (held.get('conv3_1') == 'conv2') if pair == '1' else (not held), held
            assert len(set(held.values())) == len(held) and not set(held) & set(held.values())
            npairs = len(held)
            out.seek(0); out.truncate()              # the step only: plan-time queries are not launches
            eng._bind(sp, x, sl, labels, ll)
            eng._run(sp, 'fb')
            torch.cuda.synchronize()
            assert sp.w9_held is None and not sp.w9_pending
            res[pair] = (eng.grads.clone(), _calls(out), float(sp.costs.double().mean()))
    (g0, c0, l0), (g1, c1, l1) = res['0'], res['1']
    print('native calls without / with pairing:', c0, c1)
    assert c0[PAIR] == 0 and c1[PAIR] == npairs >= 1    # every pair of the plan is launched as one, exactly once
    assert c1[SINGLE] == c0[SINGLE] - 2 * npairs        # two single launches became one paired launch:
    assert c1[SINGLE] + c1[PAIR] == c0[SINGLE] - npairs # ... exactly one slab launch fewer per pair
    assert c1[REDUCE] == c0[REDUCE]                     # the flush policy groups the same layers
    assert l0 == l1 and np.isfinite(l0)
    assert bool(g0.abs().max() > 0) and torch.equal(g0, g1)


def test_pair_under_the_multi_graph_data_parallel_schedule(dev, monkeypatch):
    """OCR_FAKE_WORLD=2: forward + late backward | exchange | early backward | exchange | optimiser, as captured graphs.  lr = 0: the buffer
    after the step is the exchanged gradient itself."""
    N, W = 8, 88
    x, labels, ll, sl = _batch(N, W)
    res = {}
    for pair in ('0', '1'):
        out = io.StringIO()
        with monkeypatch.context() as m:
            m.setenv('OCR_FAKE_WORLD', '2')
            m.setenv('OCR_OVERLAP_ALLREDUCE', '1')
            m.setenv('OCR_DP_GRAPH', '0')
            eng = _engine(m, pair, out)
            assert eng.force_allreduce and eng.world == 2 and eng.use_graphs and eng.split_layer == 'conv4_1' and eng.split_op > 0
            names = [op.name for op in eng.ops]
            assert names.index('conv2') < names.index('conv3_1') < eng.split_op       # the pair lies in the early body
            eng.setup_optimizer('Adam', 0.0)
            loss = eng.train_step(x, labels, ll, sl)
            torch.cuda.synchronize()
            sp = eng.plan(N, W)
            assert sp.graph_fb1 is not None and sp.graph_fb2 is not None and sp.w9_held is None and not sp.w9_pending
            res[pair] = (eng.grads.clone(), _calls(out), loss)
    (g0, c0, l0), (g1, c1, l1) = res['0'], res['1']
    print('native calls without / with pairing:', c0, c1)
    assert c0[PAIR] == 0 and c1[PAIR] >= 1
    assert c0[SINGLE] - c1[SINGLE] == 2 * c1[PAIR] and c1[REDUCE] == c0[REDUCE]      # (every body runs eagerly once, then under capture)
    assert l0 == l1
    assert bool(g0.abs().max() > 0) and torch.equal(g0, g1)
