"""CPU: the fp64 batch-norm reference of tests/bn_reference.py against fp64 autograd of the oracle's own formula
(oracle.graph.batch_norm_train, oracle.graph.max_pool), and the input generators of tests/test_gpu_bn_train.py against what they claim."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as bnr  # noqa: E402
from oracle import graph as og  # noqa: E402

BF, F64 = torch.bfloat16, torch.float64
EPS = bnr.f32(1e-3)


def _case(M, C, seed=5):
    x = bnr.make_x(M, C, seed, ratio=8.0)
    gamma, beta = bnr.make_gamma_beta(C, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    return x, gamma, beta, g


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", [(24, 16), (7, 8), (130, 24)])
def test_forward_and_backward_are_the_oracles_formula(M, C, relu):
    x, gamma, beta, g = _case(M, C)
    dy = (torch.rand(M, C, generator=g) * 2 - 1).to(BF)
    xr = x.to(F64).requires_grad_(True); gr = gamma.to(F64).requires_grad_(True); br = beta.to(F64).requires_grad_(True)
    pre = og.batch_norm_train(xr.view(1, 1, M, C), gr, br, eps=EPS).view(M, C)
    ref = bnr.forward(x, gamma, beta, EPS, relu=relu)
    mu, var, rs = bnr.statistics(x, EPS)
    assert torch.allclose(mu, x.to(F64).mean(0), rtol=0, atol=1e-14)
    assert torch.allclose(var, x.to(F64).var(0, unbiased=False), rtol=1e-12, atol=1e-15)       # biased: / M, not / (M - 1)
    assert torch.allclose(ref['pre'], pre.detach(), rtol=1e-12, atol=1e-12)
    want_y = (torch.relu(pre) if relu else pre).detach()
    assert torch.equal(ref['y'], want_y.to(BF))
    # backward with the rounded y as the mask: a bf16 rounding never moves a value across zero, so it is autograd's own mask
    (torch.relu(pre) if relu else pre).backward(dy.to(F64))
    b = bnr.backward(x, ref['y'], dy, gamma, mu, rs, relu, dgamma0=torch.full((C,), 2.0), dbeta0=torch.full((C,), -3.0))
    assert torch.allclose(b['dx'], xr.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(b['dgamma'] - 2.0, gr.grad, rtol=1e-10, atol=1e-11)
    assert torch.allclose(b['dbeta'] + 3.0, br.grad, rtol=1e-10, atol=1e-11)


def test_residual_is_added_to_the_rounded_batch_norm_output():
    M, C = 40, 16
    x, gamma, beta, g = _case(M, C)
    res = (torch.rand(M, C, generator=g) * 2 - 1).to(BF)
    plain = bnr.forward(x, gamma, beta, EPS)
    ref = bnr.forward(x, gamma, beta, EPS, relu=True, residual=res)
    want = torch.relu(plain['y'].to(F64) + res.to(F64)).to(BF)
    assert torch.equal(ref['y'], want) and torch.equal(bnr.tail(plain['y'], res, True), want)
    unrounded = torch.relu(plain['pre'] + res.to(F64)).to(BF)
    assert not torch.equal(unrounded, want)                  # the rounding before the add is visible at this size


@pytest.mark.parametrize("relu", [False, True])
def test_pool_and_its_routing_are_max_pool2d(relu):
    """Row pairs (2q, 2q + 1) of the [M, C] view are the H pairs of an [N, W, H, C] map with H even: og.max_pool(., 1, 2) is the pool, and its
    autograd routes a tie to the first row, as bn_pool_route does (every fourth pair of make_x is tied, gamma = 0 channels tie everywhere)."""
    N, W, H, C = 2, 5, 4, 16
    M = N * W * H
    x, gamma, beta, g = _case(M, C)
    dp = (torch.rand(M // 2, C, generator=g) * 2 - 1).to(BF)
    ref = bnr.forward(x, gamma, beta, EPS, relu=relu, pool=True)
    yr = ref['y'].to(F64).requires_grad_(True)
    pooled = og.max_pool(yr.view(N, W, H, C), 1, 2)
    assert torch.equal(ref['pooled'], pooled.detach().reshape(M // 2, C).to(BF))
    pooled.backward(dp.to(F64).view(N, W, H // 2, C))
    assert torch.equal(bnr.route_pairs(ref['y'], dp), yr.grad)
    ties = (ref['y'][0::2] == ref['y'][1::2])
    assert int(ties.sum()) >= (M // 2 // bnr.TIE_EVERY) * C and bool((bnr.route_pairs(ref['y'], dp)[1::2][ties] == 0).all())
    # the whole backward: autograd through batch norm, ReLU and the pool, against backward(pooled_dy=True)
    xr = x.to(F64).requires_grad_(True)
    pre = og.batch_norm_train(xr.view(N, W, H, C), gamma.to(F64), beta.to(F64), eps=EPS)
    act = torch.relu(pre) if relu else pre
    # autograd's pool sees unrounded values; hand it the rounded ones' selection instead by pooling the rounded y with act's gradient path
    sel = bnr.route_pairs(ref['y'], torch.ones(M // 2, C)).view(N, W, H, C)
    (act * sel).view(M // 2, 2, C).sum(1).backward(dp.to(F64))
    mu, _, rs = bnr.statistics(x, EPS)
    b = bnr.backward(x, ref['y'], dp, gamma, mu, rs, relu, pooled_dy=True)
    assert torch.allclose(b['dx'], xr.grad, rtol=1e-9, atol=1e-11)


# ------------------------------------------------------------------------------------------------ generators and launch arithmetic
@pytest.mark.parametrize("ratio", [8.0, 24.0, 48.0])
def test_input_regimes_are_what_they_claim(ratio):
    M, C = 4096, 32
    x = bnr.make_x(M, C, 11, ratio)
    gamma, beta = bnr.make_gamma_beta(C, 12)
    k = bnr.kappa(x, EPS)
    x64 = x.to(F64)
    mu, var, _ = bnr.statistics(x, EPS)
    for c in range(C):
        r = bnr.regime_of(c)
        if r in ('benign', 'gamma_zero', 'gamma_neg'):
            assert 1.0 < k[c] < 1.4 and abs(mu[c] - 0.5) < 0.08                  # uniform [-1.5, 2.5): 1 + 0.25 / (4 / 3) = 1.19
        elif r.startswith('offset'):
            assert mu[c] * (1 if r == 'offset_pos' else -1) > 0
            got = float(mu[c].abs() / var[c].sqrt())
            assert abs(got / ratio - 1) < 0.06 and abs(float(k[c]) / (1 + ratio * ratio) - 1) < 0.12
        elif r == 'constant':
            assert bool((x[:, c] == x[0, c]).all()) and float(x[0, c]) in bnr.CONSTANTS and var[c] == 0          # bit-constant
        elif r == 'outlier':
            other = x[:, c] != x[(bnr.outlier_row(M) + 2) % M, c]
            assert int(other.sum()) == 1 and float(x[bnr.outlier_row(M), c]) == bnr.OUTLIER
    assert {float(x[0, c]) for c in bnr.channels_of(C, 'constant')} == set(bnr.CONSTANTS)        # both signs
    assert bool((gamma[bnr.channels_of(C, 'gamma_zero')] == 0).all()) and bool((gamma[bnr.channels_of(C, 'gamma_neg')] < 0).all())
    assert bool((beta != 0).all())
    # exact ties: every TIE_EVERY-th pair in every channel; gamma = 0 and constant channels tie in every pair of y
    pairs_equal = (x[0::2] == x[1::2])
    tied_rows = pairs_equal.all(1).nonzero().flatten()
    assert tied_rows.tolist() == list(range(0, M // 2, bnr.TIE_EVERY))
    y = bnr.forward(x, gamma, beta, EPS, relu=True)['y']
    ties_y = (y[0::2] == y[1::2])
    for c in bnr.channels_of(C, 'gamma_zero') + bnr.channels_of(C, 'constant'):
        assert bool(ties_y[:, c].all())
    # ReLU-dead share: a real mask in the benign channels, whole channels dead or alive where beta alone decides
    dead = (y == 0).double().mean(0)
    for c in bnr.channels_of(C, 'benign') + bnr.channels_of(C, 'gamma_neg'):
        assert 0.02 < dead[c] < 0.98
    for c in bnr.channels_of(C, 'gamma_zero') + bnr.channels_of(C, 'constant'):
        assert dead[c] == (1.0 if beta[c] < 0 else 0.0)


def test_offset_ratio_keeps_the_derived_bound_below_2_to_minus_10():
    for M, C in [(16384, 512), (20480, 512), (131072, 64), (32768, 128), (8192, 512)]:
        chain = bnr.layout(M, C)['chain_fwd']
        ratio = bnr.offset_ratio_for(chain, 48.8)
        assert 0 < ratio <= 48.8 and (chain + 2) * 2.0 ** -24 * (1 + ratio * ratio) / 2 < 0.95 * 2.0 ** -10
        assert bnr.offset_ratio_for(chain, 4.0) == 4.0


def test_launch_arithmetic():
    la = bnr.layout(16384, 512)
    assert (la['groups'], la['rlanes'], la['rpb_fwd'], la['nblk_fwd'], la['rpb_bwd'], la['nblk_bwd'], la['arows']) == (64, 4, 64, 256, 32, 512, 16)
    assert la['chain_fwd'] == 16 + 4 and la['chain_bwd'] == 8 + 4 and la['idle_threads'] == 0 and la['red_used'] == bnr.RED_FLOATS
    assert bnr.workspace_bytes(16384, 512) == 512 * 2 * 512 * 4 + 2 * 512 * 8
    assert bnr.layout(131072, 64)['chain_fwd'] == 16 + 32
    assert bnr.layout(100, 24)['idle_threads'] == 1 and bnr.layout(100, 24)['red_used'] == 2040
    assert bnr.layout(1, 8)['chain_fwd'] == 1 + 256 and bnr.layout(5, 2048)['rlanes'] == 1
    assert bnr.rows_per_block(1, 256) == 8 and bnr.rows_per_block(2049, 256) == 16
