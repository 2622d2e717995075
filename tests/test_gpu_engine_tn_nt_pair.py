"""The engine's paired head launch (OCR_TN_NT_PAIR, default on: conv5's data-gradient GEMM runs inside the launch of the two plain
weight-gradient products, on the CUs their tiles leave idle) against the same engine with the switch off: one training step of LSTM_train
— forward, backward, optimiser — must leave the SAME gradients, parameters and loss, bit for bit, with exactly one launch fewer.
34 images of width 128 are the smallest batch of that width at which the policy engages: the GEMM has 34 x 31 = 1054 rows, the large-tile
engine's floor is 1024.  Below it (batch 8) the policy declines and the step's launches are the switched-off ones."""
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

JOBS, JOBS_NT, NT, QUERY = 'ocr_gemm_tn_jobs_bf16', 'ocr_gemm_tn_jobs_nt_bf16', 'ocr_gemm_nt_bf16', 'ocr_gemm_tn_jobs_nt_supported'


def _batch(N, W):
    rng = np.random.RandomState(7)
    T = W // 4 - 1
    L = max(1, min(4, T // 3))
    x = rng.rand(N, W, cfg.NUM_FEATURES).astype(np.float32)
    labels = rng.randint(1, cfg.NCLASSES - 1, N * L).astype(np.int32)
    return x, labels, np.full(N, L, np.int32), np.full(N, T, np.int32)


def _step(monkeypatch, pair, N, W):
    """One eager training step with the switch set -> (gradients, parameters, loss, names of the native calls of the step)."""
    out = io.StringIO()
    x, labels, ll, sl = _batch(N, W)
    with monkeypatch.context() as m:
        m.setenv('OCR_TN_NT_PAIR', pair)
        m.setattr(nat, '_lib', Traced(nat.lib(), nat._SIGS, out))          # tools/launch_trace.py's hook: one line per native call
        for k, v in (('SOLVER', 'Adam'), ('LEARNING_RATE', 1e-4), ('WEIGHT_DECAY', 1e-5)):
            m.setattr(cfg.TRAIN, k, v)
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=5, use_graphs=False)
        assert eng.tn_nt_pair == (pair == '1')
        sp = eng.plan(N, W)
        out.seek(0); out.truncate()              # the step only
        eng._bind(sp, x, sl, labels, ll)
        eng._run(sp, 'fb')
        grads = eng.grads.clone()
        eng.optimizer_step(sp)
        torch.cuda.synchronize()
        assert not sp.tn_pending
        names = [line.split('(')[0] for line in out.getvalue().splitlines()]
        return grads, eng.params.clone(), float(sp.costs.double().mean()), names


def test_one_step_same_results_one_launch_less(dev, monkeypatch):
    N, W = 34, 128
    g0, p0, l0, n0 = _step(monkeypatch, '0', N, W)
    g1, p1, l1, n1 = _step(monkeypatch, '1', N, W)
    print('off:', {k: n0.count(k) for k in (JOBS, JOBS_NT, NT, QUERY)}, len(n0), ' on:', {k: n1.count(k) for k in (JOBS, JOBS_NT, NT, QUERY)}, len(n1))
    assert n0.count(JOBS) == 1 and n0.count(JOBS_NT) == 0 and n0.count(QUERY) == 0          # switched off: not even the query
    assert n1.count(JOBS) == 0 and n1.count(JOBS_NT) == 1 and n1.count(NT) == n0.count(NT) - 1
    launches0, launches1 = [n for n in n0 if n != QUERY], [n for n in n1 if n != QUERY]
    assert len(launches1) == len(launches0) - 1
    # the launch list is the switched-off one with (jobs, gemm_nt) replaced by the one paired call
    i = launches0.index(JOBS)
    assert launches0[i + 1] == NT and launches1 == launches0[:i] + [JOBS_NT] + launches0[i + 2:]
    assert l0 == l1 and np.isfinite(l0)
    assert bool(g0.abs().max() > 0) and torch.equal(g0, g1)
    assert torch.equal(p0, p1)


def test_declined_below_the_gemm_floor_runs_the_same_launches(dev, monkeypatch):
    N, W = 8, 88                                 # 8 x 21 = 168 GEMM rows: the policy declines
    g0, p0, l0, n0 = _step(monkeypatch, '0', N, W)
    g1, p1, l1, n1 = _step(monkeypatch, '1', N, W)
    assert n1.count(JOBS_NT) == 0
    assert [n for n in n1 if n != QUERY] == n0
    assert l0 == l1 and torch.equal(g0, g1) and torch.equal(p0, p1)
