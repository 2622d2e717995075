"""-m gpu: training-mode batch norm (csrc/batchnorm.hip: bn_stats / bn_finalize / bn_apply / bn_apply_pool / bn_bwd_stats / bn_bwd_finalize /
bn_bwd_apply) and the per-tile statistics of the convolution epilogues (conv_k3.hip) against the fp64 reference of tests/bn_reference.py.

Shapes: the product tensors (headline, variable width, the ResNet stages) and the edges of the thread layout — groups = C / 8 channel
groups along the 256 threads, rlanes = 256 / groups row lanes — each with the conditions it reaches computed from the launch arithmetic
and asserted.  Data: eight per-channel regimes mixed across the channels of every tensor (bn_reference.REGIMES: benign, |mean| >> std with
both signs, a constant channel, a constant channel with one outlier row, gamma = 0, gamma < 0) and every fourth row pair duplicated.
Every comparison is element by element against a bound derived beside it from the kernel's rounding steps; selections and copies are
compared bit for bit.  The workspace is filled with NaN bit patterns before every call and carries a guard tail that must survive.
Every check prints its worst error / bound ratio (pytest -s); the "worst measured on MI355X" figures in the comments are those ratios.
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as bnr  # noqa: E402
from test_gpu_memory_bound_kernels import EPS32, _assert_bits_equal, _half_ulp_bf16, _within_each  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

BF, F64 = torch.bfloat16, torch.float64
EPS = bnr.f32(1e-3)                 # the `float eps` the entry point receives
GUARD = 4096                        # bytes behind the workspace that no pass may touch
GUARD_BYTE, POISON = 0xA5, 0xFF     # 0xFFFFFFFF is a NaN as fp32 and 0xFFFF...FF as a double: any read of an unwritten word poisons the result
# |mean| / std of the `offset` channels.  Measured with the fp32 oracle on tests/golden/trained_weights.npz over the rendered batches C1, C2
# and V0 of tests/golden/captcha_batches.npz: the largest per-channel |mean| / std at a batch-norm input is 12.2 (conv4_1, batch V0; 11.4 on
# C2, 9.7 on C1; conv4_2: 1.3).  Four times that is 48.8 > 32, so 48.8 is asked for; offset_ratio_for() lowers it per product shape to where
# the derived rstd bound still stays below 2^-10 (see test_statistics_forward_and_backward).
OFFSET_RATIO = 48.8


def _check(what, err, bound):
    """Print the worst error / bound ratio, then assert err <= bound element by element."""
    err, bound = torch.as_tensor(err, dtype=F64), torch.as_tensor(bound, dtype=F64)
    if err.numel():
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, float('inf'), 0.0).to(F64))
        print("%-58s worst error / bound %.3g (largest error %.3g)" % (what, float(ratio.max()), float(err.max())))
        _within_each(what, err, bound.expand_as(err))


class _Workspace:
    """ocr_bn_workspace_bytes(M, C) bytes as an exact-size view in front of a guard tail; poisoned before every call."""

    def __init__(self, M, C, dev, poison=POISON):
        self.n = int(nat.lib().ocr_bn_workspace_bytes(M, C))
        assert self.n == bnr.workspace_bytes(M, C)
        self.buf = torch.empty(self.n + GUARD, dtype=torch.uint8, device=dev)
        self.poison = poison
        self.ws = self.buf[:self.n]

    def fresh(self):
        self.buf[:self.n].fill_(self.poison)
        self.buf[self.n:].fill_(GUARD_BYTE)
        return self.ws

    def with_rows(self, part):
        """Poisoned, then `part` [R, 2, C] fp32 written at its front as a producing convolution would leave it."""
        ws = self.fresh()
        ws[:part.numel() * 4].view(torch.float32).copy_(part.flatten().to(ws.device))
        return ws

    def check_guard(self, what):
        assert bool((self.buf[self.n:] == GUARD_BYTE).all()), what + ": the bytes behind the workspace were written"


def _nan(shape, dev, dtype=BF):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


@functools.lru_cache(maxsize=8)
def _inputs(M, C, ratio):
    """x, gamma, beta, dy (CPU; dy uniform in [-1, 1), bf16), computed once per shape and shared by the tests that use it."""
    x = bnr.make_x(M, C, 100 + C, ratio)
    gamma, beta = bnr.make_gamma_beta(C, 200 + C)
    g = torch.Generator().manual_seed(300 + C)
    dy = (torch.rand(M, C, generator=g) * 2 - 1).to(BF)
    return x, gamma, beta, dy


# ================================================================================================ bounds
def _stats_bounds(x64, chain, block_rows):
    """Bounds on the device's mean and rstd against the fp64 statistics of x64 [M, C], for fp32 summation chains of `chain` additions over
    blocks of `block_rows` rows whose results are then added in double.

    sum of squares: `chain` fp32 roundings (the fma rounds once per row, the LDS lane sum once per lane), each at most 2^-24 of the partial
      sum, which never exceeds the block's sum of x^2: |ss' - ss| <= chain 2^-24 sum x^2 to first order; the + 2 covers the second-order
      terms ((1 + u)^chain - 1 <= (chain + 2) u for chain <= 2^10) and the double arithmetic behind it.
    sum: the same with E|x|.  It is EXACT where every partial sum of a block is representable: all addends are multiples of q, the ulp of
      the channel's smallest non-zero bf16 magnitude, and block_rows max|x| <= 2^24 q.  That holds in the `offset`, `constant` and
      `outlier` channels (one binade or two, at most a few hundred rows), which is what keeps the mean's share 2 |mu| d(mu) of the variance
      error out of exactly the channels where |mu| is large.
    variance = ss / M - mu^2 in double: (chain + 2) 2^-24 E[x^2] + 2 |mu| d(mu) + d(mu)^2; a negative result is clamped to 0, which only
      moves it towards the true value.  rstd = (float) 1 / sqrt(var + eps): the interval the variance bound allows, plus the final rounding.
    Returns mean_bound, rstd_bound and rel = var_bound / (2 (var + eps)), the first-order relative rstd bound.
    Worst measured on MI355X (error / bound): mean 0.998 at [1013, 72] — an offset channel whose sums are exact, so the error is the
    half ulp of the final fp32 rounding and the bound is just that; rstd 0.26 at [7, 520], 0.07 or less at the product shapes (largest
    rstd error there 2.7e-6, at [131072, 64]) and 0.058 at [262144, 8] (4.6e-4 absolute at |mean| / std = 32).  bf16 data use the fp32
    accumulator far below the worst case: squares of one binade carry 16 bits, so chains of up to 2^8 of them add without rounding.
    From caller-written partial rows (chain 1, blocks of 256): mean 0.82, rstd 0.33."""
    mu, var, rs = bnr.statistics(x64, EPS)
    ax = x64.abs()
    ex2, eabs, amax = (x64 * x64).mean(0), ax.mean(0), ax.max(0).values
    smallest = torch.where(ax > 0, ax, torch.full_like(ax, float('inf'))).min(0).values
    _, e = torch.frexp(torch.where(torch.isinf(smallest), torch.ones_like(smallest), smallest))
    q = torch.ldexp(torch.ones_like(smallest), e - 8)                       # bf16 ulp of a value in [2^(e-1), 2^e)
    exact = (block_rows * amax <= 2.0 ** 24 * q) | torch.isinf(smallest)
    d_sum = torch.where(exact, torch.zeros_like(mu), (chain + 2) * EPS32 * eabs)
    mean_bound = d_sum + EPS32 * mu.abs()
    var_bound = (chain + 2) * EPS32 * ex2 + 2 * mu.abs() * d_sum + d_sum * d_sum
    hi = 1.0 / torch.sqrt((var - var_bound).clamp_min(0.0) + EPS)
    lo = 1.0 / torch.sqrt(var + var_bound + EPS)
    rstd_bound = torch.maximum(hi - rs, rs - lo) + EPS32 * hi
    return mean_bound, rstd_bound, var_bound / (2 * (var + EPS))


def _check_y(what, y, x64, mu, rs, gamma, beta, relu, prop=None):
    """y (device, bf16) against [relu]((x - mu) rs gamma + beta) in fp64.
    The device evaluates it in fp32: one subtraction, two products and one addition (or an fma), four roundings of at most 2^-24 each
    on terms no larger than |x - mu| |rs gamma| + |beta|: within delta = 2^-21 (|x - mu| |rs gamma| + |beta|) with a factor 2 to spare;
    then one rounding to bf16: half a bf16 ulp at |ref| + 2 delta, plus 2 delta.  With mu, rs the device's own statistics this is tight
    whatever the statistics pass did; against the fp64 statistics `prop`, the propagated statistics bound, widens delta.
    ReLU may change sign only where the pre-activation is within that distance of zero.
    Worst measured on MI355X: 1.0 of the bound with the device's statistics and end to end (a pre-activation halfway between two bf16
    values: the `outlier` and `constant` channels hold few distinct values, and ties are common among them)."""
    g64, b64 = gamma.to(F64), beta.to(F64)
    xm = x64 - mu
    pre = xm * (rs * g64) + b64
    ref = pre.clamp_min(0.0) if relu else pre
    delta = 2 * 2.0 ** -21 * (xm.abs() * (rs * g64).abs() + b64.abs())
    if prop is not None:
        delta = delta + prop
    yc = y.cpu()
    _check(what, (yc.to(F64) - ref).abs(), _half_ulp_bf16(ref.abs() + delta) + delta)
    if relu:
        flip = (yc > 0) != (pre > 0)
        _check(what + " ReLU sign flips", pre.abs()[flip], delta[flip])


def _check_backward(what, ref, dx, dg, db, dg0, db0, gamma, rs, M, chain):
    """dx, dgamma, dbeta (device) against bn_reference.backward(...) = ref, evaluated with the device's own mean, rstd and y.
    dbeta / dgamma: an fp32 chain of `chain` additions per block (rows per thread, then the LDS lane sum), the blocks added in double; a
      dgamma term (x - mu) rs dz carries two more roundings; then the conversion of the total to fp32 and the addition onto the start value:
      (chain + 4) 2^-24 (|start| + sum |terms|).
    dx = gr (dz - mdz - xhat mdzx), gr = gamma rs, in fp32: gr, xhat (two), the product, two subtractions and the final product round once
      each — at most 8 roundings on terms bounded by |gr| (|dz| + |mdz| + |xhat| |mdzx|): eval = 2^-21 of that.  The two means come from the
      sums above, converted to fp32: |d mdz| <= (chain + 3) 2^-24 sum|dz| / M, likewise mdzx; they enter dx as |gr| (d mdz + |xhat| d mdzx).
      Then one rounding to bf16: half an ulp at |dx| + eval + prop.
    Worst measured on MI355X (error / bound): dgamma 0.14 ([1013, 1000]; 0.24 from partial rows, 0.11 with pooled_dy), dbeta 0.17
    ([1, 2048]), dx 1.0 (half-ulp ties, as in the forward pass)."""
    for name, got, start, want, scale in (("dgamma", dg, dg0, ref['dgamma'], ref['abs_dzx']), ("dbeta", db, db0, ref['dbeta'], ref['abs_dz'])):
        _check("%s %s" % (what, name), (got.cpu().to(F64) - want).abs(), (chain + 4) * EPS32 * (start.to(F64).abs() + scale))
    gr = (gamma.to(F64) * rs).abs()
    ev = 2.0 ** -21 * gr * (ref['dz'].abs() + ref['mdz'].abs() + ref['xhat'].abs() * ref['mdzx'].abs())
    prop = gr * (chain + 3) * EPS32 * (ref['abs_dz'] + ref['xhat'].abs() * ref['abs_dzx']) / M
    _check(what + " dx", (dx.cpu().to(F64) - ref['dx']).abs(), _half_ulp_bf16(ref['dx'].abs() + ev + prop) + ev + prop)


# ================================================================================================ shapes
def _tags(M, C):
    """The conditions a shape reaches, from the kernels' own launch arithmetic (bn_reference.layout mirrors bn_rows_per_block_host, groups
    and rlanes of batchnorm.hip)."""
    la = bnr.layout(M, C)
    t = set()
    if la['idle_threads']: t.add('idle')                              # 256 % groups != 0: threads with rl >= rlanes must stay out
    if la['red_used'] == bnr.RED_FLOATS: t.add('full_red')             # block_channel_reduce's 2048-float LDS array is exactly full
    if M < la['rlanes']: t.add('short')                                # fewer rows than row lanes: lanes without a single row
    if la['nblk_fwd'] > 1: t.add('blocks')                             # more than one statistics block: bn_pair_sum adds rows
    if la['nblk_fwd'] > 16: t.add('lanes16')                           # more partial rows than bn_pair_sum has row lanes
    if M % la['rpb_fwd']: t.add('tail_stats')                          # a partial last block in the forward statistics pass
    if M % la['rpb_bwd']: t.add('tail_bwd')                            # ... in the backward statistics pass
    if M % la['arows']: t.add('tail_apply')                            # ... in the apply passes (4 rlanes rows per block)
    if M % 8: t.add('odd8')                                            # M is no multiple of 8 (rows per block always is)
    return t


PRODUCT = [  # (M, C, relu): what it is
    (16384, 512, True),      # the headline: conv4_1 / conv4_2 at [64 * 64 * 4, 512]; chain 16 + 4
    (20480, 512, True),      # the variable-width plan (W = 320): 80 rows per statistics block, chain 20 + 4
    (131072, 64, True),      # ResNet stage 1: the longest fp32 chains of the product, 16 + 32
    (32768, 128, True),      # ResNet stage 2: chain 8 + 16
    (8192, 512, True),       # ResNet stage 4: chain 8 + 4
]
PRODUCT_TAGS = {'full_red', 'blocks', 'lanes16'}                        # all five: power-of-two C, M a multiple of every block size
EDGES = [  # (M, C, relu, conditions)
    (1013, 8, True, {'full_red', 'blocks', 'lanes16', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),      # 256 row lanes, 8 rows a block: 248 lanes idle by row count
    (262144, 8, True, {'full_red', 'blocks', 'lanes16'}),                      # the narrowest C with the longest lane sum: 4 rows + 256 lanes of 1024-row blocks
    (24, 24, False, {'idle', 'short', 'blocks', 'tail_apply'}),                  # groups 3, rlanes 85: thread 255 idle, red[] 2040 of 2048, M < rlanes
    (1013, 72, True, {'idle', 'blocks', 'lanes16', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),         # groups 9, rlanes 28: 4 idle threads
    (7, 520, False, {'idle', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),  # groups 65, rlanes 3: 61 idle threads, 7 rows
    (1013, 1000, True, {'idle', 'blocks', 'lanes16', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),       # groups 125, rlanes 2: 6 idle threads
    (2, 2040, True, {'idle', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),  # groups 255, one row lane, thread 255 idle
    (1, 2048, False, {'full_red', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),                          # the widest C: one row lane, red[] full; M = 1
    (1, 512, True, {'full_red', 'short', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),                   # M = 1 at the headline width (the batch-1 path): var = 0
    (2, 512, False, {'full_red', 'short', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),                  # M = 2 < 4 row lanes
    (7, 64, True, {'full_red', 'short', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),                    # M = 7 < 32 row lanes
    (24, 128, False, {'full_red', 'blocks', 'tail_apply'}),                    # M = 24: three whole statistics blocks of 8, less than one apply block
    (4105, 128, True, {'full_red', 'blocks', 'lanes16', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),    # 171 * 24 + 1: one row past the forward pass's rows per block
    (2113, 128, False, {'full_red', 'blocks', 'lanes16', 'tail_stats', 'tail_bwd', 'tail_apply', 'odd8'}),   # 33 * 64 + 1: one row past the apply pass's 4 * rlanes rows
]


def test_shapes_reach_what_they_claim():
    for M, C, _ in PRODUCT:
        assert _tags(M, C) == PRODUCT_TAGS, (M, C, _tags(M, C))
    for M, C, _, tags in EDGES:
        assert _tags(M, C) == tags, (M, C, sorted(_tags(M, C)))
    la = bnr.layout(4105, 128)
    assert 4105 % la['rpb_fwd'] == 1 and la['rpb_fwd'] == 24
    la = bnr.layout(2113, 128)
    assert 2113 % la['arows'] == 1 and la['arows'] == 64
    assert bnr.layout(24, 24)['red_used'] == 2040 and bnr.layout(262144, 8)['chain_fwd'] == 260
    assert {C for _, C, _, _ in EDGES} >= {8, 24, 72, 520, 1000, 2040, 2048} and {M for M, _, _, _ in EDGES} >= {1, 2, 7, 24, 1013}


def _ratio(M, C):
    """|mean| / std of the offset channels.  Product shapes: OFFSET_RATIO lowered to where the derived rstd bound of the shape's chain stays
    below 2^-10 — 48.8 fits no product chain: 47.0 at (8192, 512), 37.5 at (16384, 512), 34.5 at (20480, 512) and (32768, 128), 24.5 at
    (131072, 64).  Edge shapes: 32, with whatever bound their chain gives (260 additions at (262144, 8): 2^-7)."""
    return bnr.offset_ratio_for(bnr.layout(M, C)['chain_fwd'], OFFSET_RATIO) if (M, C) in {s[:2] for s in PRODUCT} else 32.0


# ================================================================================================ (a) (b) (c) (f): forward and backward
@pytest.mark.parametrize("M,C,relu,product", [c + (True,) for c in PRODUCT] + [c[:3] + (False,) for c in EDGES])
def test_statistics_forward_and_backward(dev, M, C, relu, product):
    la = bnr.layout(M, C)
    x, gamma, beta, dy = _inputs(M, C, _ratio(M, C))
    x64 = x.to(F64)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    wk = _Workspace(M, C, dev)
    y, sm, sr = ops.bn_train_fwd(xd, gd, bd, EPS, relu, wk.fresh(), out=_nan((M, C), dev), save_mean=_nan((C,), dev, torch.float32),
                                 save_rstd=_nan((C,), dev, torch.float32))
    wk.check_guard("forward")
    what = "[%d, %d]" % (M, C)
    # (a) statistics against fp64 (bounds and the worst measured figures: _stats_bounds)
    mu, var, rs = bnr.statistics(x64, EPS)
    mean_bound, rstd_bound, rel = _stats_bounds(x64, la['chain_fwd'], la['rpb_fwd'])
    if product:                                          # the derived bound itself must stay below 2^-10 wherever the product can be
        keep = [c for c in range(C) if bnr.regime_of(c) != 'outlier']
        assert float(rel[keep].max()) < 2.0 ** -10, "derived rstd bound %.3e at a product shape" % float(rel[keep].max())
    smc, src = sm.cpu().to(F64), sr.cpu().to(F64)
    _check(what + " save_mean", (smc - mu).abs(), mean_bound)
    _check(what + " save_rstd", (src - rs).abs(), rstd_bound)
    for c in bnr.channels_of(C, 'constant'):             # one value in the channel: the sums are exact, var = 0, y = beta
        assert float(smc[c]) == float(x[0, c]) and float(src[c]) == float(torch.tensor(1.0 / (EPS ** 0.5), dtype=torch.float32))
        want = (beta[c].clamp_min(0.0) if relu else beta[c]).to(BF)
        assert bool((y[:, c].cpu() == want).all())
    # (b) the apply pass alone: fp64 with the device's statistics
    _check_y(what + " y | device statistics", y, x64, smc, src, gamma, beta, relu)
    # (c) end to end: fp64 throughout; the statistics bounds propagate as |gamma| (|rs| d mu + |x - mu| d rs + d mu d rs)
    prop = gamma.to(F64).abs() * (rs * mean_bound + (x64 - mu).abs() * rstd_bound + mean_bound * rstd_bound)
    _check_y(what + " y end to end", y, x64, mu, rs, gamma, beta, relu, prop=prop)
    # (f) backward, accumulating onto non-zero dgamma / dbeta
    g = torch.Generator().manual_seed(7)
    dg0, db0 = torch.rand(C, generator=g) * 10 - 5, torch.rand(C, generator=g) * 10 - 5
    dg, db = dg0.to(dev, copy=True), db0.to(dev, copy=True)
    dx = ops.bn_train_bwd(xd, y, dy.to(dev), gd, sm, sr, dg, db, relu, wk.fresh(), out=_nan((M, C), dev))
    wk.check_guard("backward")
    ref = bnr.backward(x, y.cpu(), dy, gamma, smc, src, relu, dgamma0=dg0, dbeta0=db0)
    _check_backward(what + " backward", ref, dx, dg, db, dg0, db0, gamma, src, M, la['chain_bwd'])


# ================================================================================================ (d) residual tail
@pytest.mark.parametrize("M,C,relu", [(32768, 128, True), (1013, 72, True), (7, 520, False), (1, 2048, True)])
def test_residual_tail_is_bit_identical(dev, M, C, relu):
    """y = [relu](bf16(bn) + residual): the sum of two bf16 values is exact in fp32 unless their exponents lie more than 16 apart, and then
    the smaller one cannot reach a bf16 rounding boundary of the larger, so fp32 and fp64 round to the same bf16: bit-identical."""
    x, gamma, beta, dy = _inputs(M, C, _ratio(M, C))
    wk = _Workspace(M, C, dev)
    xd, gd, bd, res = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    y_plain, sm0, sr0 = ops.bn_train_fwd(xd, gd, bd, EPS, False, wk.fresh())
    y_tail, sm1, sr1 = ops.bn_train_fwd(xd, gd, bd, EPS, relu, wk.fresh(), out=_nan((M, C), dev), residual=res)
    wk.check_guard("residual")
    _assert_bits_equal("residual tail", y_tail, bnr.tail(y_plain.cpu(), dy, relu))
    _assert_bits_equal("mean", sm1, sm0); _assert_bits_equal("rstd", sr1, sr0)


# ================================================================================================ (e) fused pool, forward and backward
@pytest.mark.parametrize("M,C,relu", [(16384, 512, True), (20480, 512, False), (2, 2040, True), (2, 512, False), (1014, 72, True), (26, 24, False)])
def test_fused_pool_against_the_reference(dev, M, C, relu):
    """bn_apply_pool_kernel and bn_pool_route against bn_reference (not against maxpool_fwd / maxpool_bwd): the pooled tensor is a selection
    from the device's y, so bit for bit; the routed backward equals the plain backward on the reference's routed gradient bit for bit (the
    routed gradient holds dp or 0: no arithmetic), so an element that must receive no gradient gets exactly the formula's value for g = 0."""
    x, gamma, beta, dy = _inputs(M, C, _ratio(M, C))
    wk = _Workspace(M, C, dev)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    y0, sm0, sr0 = ops.bn_train_fwd(xd, gd, bd, EPS, relu, wk.fresh())
    pooled = _nan((M // 2, C), dev)
    y1, sm1, sr1 = ops.bn_train_fwd(xd, gd, bd, EPS, relu, wk.fresh(), out=_nan((M, C), dev), pooled=pooled)
    wk.check_guard("pooled forward")
    _assert_bits_equal("y with the pool", y1, y0); _assert_bits_equal("mean", sm1, sm0); _assert_bits_equal("rstd", sr1, sr0)
    yc = y0.cpu()
    _assert_bits_equal("pooled", pooled, bnr.pool_pairs(yc))
    ties = (yc[0::2] == yc[1::2])
    assert int(ties.sum()) >= (M // 2) * len(bnr.channels_of(C, 'gamma_zero'))              # gamma = 0: every pair ties
    dp = dy[:M // 2].contiguous()
    g = torch.Generator().manual_seed(9)
    dg0, db0 = torch.rand(C, generator=g) * 10 - 5, torch.rand(C, generator=g) * 10 - 5
    dg1, db1 = dg0.to(dev, copy=True), db0.to(dev, copy=True)
    dx1 = ops.bn_train_bwd(xd, y0, dp.to(dev), gd, sm0, sr0, dg1, db1, relu, wk.fresh(), out=_nan((M, C), dev), pooled_dy=True)
    wk.check_guard("pooled backward")
    routed = bnr.route_pairs(yc, dp).to(BF)                                                   # dp or 0: exact
    dg2, db2 = dg0.to(dev, copy=True), db0.to(dev, copy=True)
    dx2 = ops.bn_train_bwd(xd, y0, routed.to(dev), gd, sm0, sr0, dg2, db2, relu, wk.fresh(), out=_nan((M, C), dev))
    _assert_bits_equal("dx, routed in the kernel", dx1, dx2)
    _assert_bits_equal("dgamma", dg1, dg2); _assert_bits_equal("dbeta", db1, db2)
    ref = bnr.backward(x, yc, dp, gamma, sm0.cpu(), sr0.cpu(), relu, pooled_dy=True, dgamma0=dg0, dbeta0=db0)
    _check_backward("[%d, %d] pooled backward" % (M, C), ref, dx1, dg1, db1, dg0, db0, gamma, sr0.cpu().to(F64), M, bnr.layout(M, C)['chain_bwd'])


# ================================================================================================ (g) partial rows
def _rows256(a, R):
    """Per-256-row fp64 column sums of a [256 R, C], rounded to fp32: what a producing convolution leaves per tile."""
    return a.view(R, 256, a.shape[1]).sum(1).to(torch.float32)


@pytest.mark.parametrize("M,C", [(256, 72), (17 * 256, 64), (16384, 512)])         # 1, 17 and M / 256 = 64 partial rows; bn_pair_sum has 16 row lanes
def test_partial_rows_without_a_convolution(dev, M, C):
    """partial_rows: the statistics passes are skipped and bn_finalize / bn_bwd_finalize add the rows the caller left in the workspace.
    The test writes them itself — fp64 sums of 256 rows rounded to fp32, one rounding per row, so the chain of every bound is 1 — and
    poisons the rest of the workspace."""
    R = M // 256
    x, gamma, beta, dy = _inputs(M, C, _ratio(M, C))
    x64 = x.to(F64)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    wk = _Workspace(M, C, dev)
    assert R <= bnr.layout(M, C)['nblk_bwd']
    part = torch.stack([_rows256(x64, R), _rows256(x64 * x64, R)], 1)
    y, sm, sr = ops.bn_train_fwd(xd, gd, bd, EPS, True, wk.with_rows(part), out=_nan((M, C), dev), partial_rows=R)
    wk.check_guard("forward from partial rows")
    what = "[%d, %d] %d partial rows" % (M, C, R)
    mu, var, rs = bnr.statistics(x64, EPS)
    mean_bound, rstd_bound, _ = _stats_bounds(x64, 1, 256)
    smc, src = sm.cpu().to(F64), sr.cpu().to(F64)
    _check(what + " save_mean", (smc - mu).abs(), mean_bound)
    _check(what + " save_rstd", (src - rs).abs(), rstd_bound)
    _check_y(what + " y | device statistics", y, x64, smc, src, gamma, beta, True)
    prop = gamma.to(F64).abs() * (rs * mean_bound + (x64 - mu).abs() * rstd_bound + mean_bound * rstd_bound)
    _check_y(what + " y end to end", y, x64, mu, rs, gamma, beta, True, prop=prop)
    # backward: dy is pre-masked, the rows hold (sum g, sum g xhat); the passes read neither y nor a mask
    yc = y.cpu()
    dym = torch.where(yc > 0, dy, torch.zeros_like(dy))
    xhat = (x64 - smc) * src
    partb = torch.stack([_rows256(dym.to(F64), R), _rows256(dym.to(F64) * xhat, R)], 1)
    g = torch.Generator().manual_seed(8)
    dg0, db0 = torch.rand(C, generator=g) * 10 - 5, torch.rand(C, generator=g) * 10 - 5
    dg, db = dg0.to(dev, copy=True), db0.to(dev, copy=True)
    dx = ops.bn_train_bwd(xd, _nan((M, C), dev), dym.to(dev), gd, sm, sr, dg, db, True, wk.with_rows(partb), out=_nan((M, C), dev), partial_rows=R)
    wk.check_guard("backward from partial rows")
    ref = bnr.backward(x, yc, dym, gamma, smc, src, False, dgamma0=dg0, dbeta0=db0)
    _check_backward(what + " backward", ref, dx, dg, db, dg0, db0, gamma, src, M, 1)


# ================================================================================================ (h) workspace
@pytest.mark.parametrize("M,C", [(16384, 512), (1013, 72), (2, 2040), (4105, 128)])
def test_workspace_is_neither_read_before_written_nor_overrun(dev, M, C):
    x, gamma, beta, dy = _inputs(M, C, _ratio(M, C))
    xd, gd, bd, dyd = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    runs = []
    for poison in (0xFF, 0x7F):                          # NaN words, and 3.39e38 as fp32 / 1.38e306 as a double
        wk = _Workspace(M, C, dev, poison)
        y, sm, sr = ops.bn_train_fwd(xd, gd, bd, EPS, True, wk.fresh())
        wk.check_guard("forward")
        dg, db = torch.ones(C, device=dev), torch.ones(C, device=dev)
        dx = ops.bn_train_bwd(xd, y, dyd, gd, sm, sr, dg, db, True, wk.fresh())
        wk.check_guard("backward")
        out = [y, sm, sr, dx, dg, db]
        if M % 2 == 0:
            pooled = _nan((M // 2, C), dev)
            out.append(ops.bn_train_fwd(xd, gd, bd, EPS, True, wk.fresh(), pooled=pooled)[0]); out.append(pooled)
            wk.check_guard("pooled forward")
            out.append(ops.bn_train_bwd(xd, y, dyd[:M // 2].contiguous(), gd, sm, sr, dg, db, True, wk.fresh(), pooled_dy=True))
            wk.check_guard("pooled backward")
        assert all(bool(torch.isfinite(t.float()).all()) for t in out)
        runs.append(out)
    for a, b in zip(*runs):
        _assert_bits_equal("two workspace fill patterns", a, b)


# ================================================================================================ (i) refusals
def test_refusals_leave_the_outputs_untouched(dev):
    def refused(M, C, call):
        wk = _Workspace(M, C, dev)
        t = dict(x=torch.ones(M, C, dtype=BF, device=dev), gamma=torch.ones(C, device=dev), beta=torch.ones(C, device=dev),
                 y=_nan((M, C), dev), dx=_nan((M, C), dev), pooled=_nan((max(M // 2, 1), C), dev), sm=_nan((C,), dev, torch.float32),
                 sr=_nan((C,), dev, torch.float32), dg=torch.full((C,), 3.0, device=dev), db=torch.full((C,), -3.0, device=dev),
                 res=torch.ones(M, C, dtype=BF, device=dev), dp=torch.ones(M // 2, C, dtype=BF, device=dev), ws=wk.fresh())
        keep = {k: v.clone() for k, v in t.items()}
        with pytest.raises(nat.NativeError, match="status 2"):
            call(t, bnr.layout(M, C)['nblk_bwd'] if C % 8 == 0 and C <= 2048 else 0)
        torch.cuda.synchronize()
        for k in t:
            assert torch.equal(t[k].view(torch.uint8), keep[k].view(torch.uint8)), "%s was written by a refused call" % k
        wk.check_guard("refused call")

    fwd = lambda t, **kw: ops.bn_train_fwd(t['x'], t['gamma'], t['beta'], EPS, True, t['ws'], out=t['y'], save_mean=t['sm'], save_rstd=t['sr'], **kw)
    bwd = lambda t, dy, **kw: ops.bn_train_bwd(t['x'], t['y'], dy, t['gamma'], t['sm'], t['sr'], t['dg'], t['db'], True, t['ws'], out=t['dx'], **kw)
    for M, C in ((16, 12), (4, 2056)):                                                           # C % 8 != 0; C > 2048
        refused(M, C, lambda t, n: fwd(t))
        refused(M, C, lambda t, n: bwd(t, t['x']))
    refused(7, 64, lambda t, n: fwd(t, pooled=t['pooled']))                                       # pooled with odd M
    refused(8, 64, lambda t, n: fwd(t, pooled=t['pooled'], residual=t['res']))                    # pooled with a residual
    refused(7, 64, lambda t, n: bwd(t, t['dp'], pooled_dy=True))                                  # pooled_dy with odd M
    refused(512, 64, lambda t, n: bwd(t, t['dp'], pooled_dy=True, partial_rows=1))                # partial_rows together with pooled_dy
    refused(512, 64, lambda t, n: fwd(t, partial_rows=n + 1))                                     # more partial rows than the workspace holds
    refused(512, 64, lambda t, n: bwd(t, t['x'], partial_rows=n + 1))
    refused(1013, 72, lambda t, n: fwd(t, partial_rows=n + 1))
    refused(512, 64, lambda t, n: fwd(t, partial_rows=-1))


# ================================================================================================ convolution epilogues (conv_k3.hip)
# The epilogue of conv_k3 adds, per 256-pixel tile and channel, the stored bf16 outputs of the tile: a thread keeps one 16-byte unit (8
# channels) and walks NIT = U / 2 rows of the staged tile (U = BN / 8 units a row: 8 rows at BN = 128, 4 at BN = 64) in fp32, then the
# 512 / U = 32 or 64 threads of a unit meet in LDS and one thread adds them in fp32: a chain of 8 + 32 = 40 or 4 + 64 = 68 additions.
# |sum' - sum| <= (68 + 2) 2^-24 sum |terms| per tile and channel, for the sums and for the sums of squares; the backward second column's
# term g (z - mean) rstd carries two more roundings: (68 + 4) 2^-24 sum |g xhat|.
# Worst measured on MI355X (error / bound): forward sums 0 (outputs near +-8 share a binade: every partial sum is exact), sums of squares
# 0.11 at (32, 64, 2, 512, 512); backward sum g 0.005, sum g xhat 0.032.
K3_CHAIN = 68
CONV_BIAS = 8.0          # bias magnitude: the outputs' |mean| / std per channel is about 10 (std 0.8 from 9 Ci products of 0.05-scale weights)


def _tiles(a, rows):
    return a.view(rows, 256, a.shape[1]).sum(1)


def _gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


@pytest.mark.parametrize("Nb,W,H,Ci,Co", [(64, 64, 4, 256, 512), (64, 64, 4, 512, 512), (64, 80, 4, 256, 512), (32, 64, 4, 256, 256), (32, 64, 2, 512, 512)])
def test_conv3x3_epilogue_statistics_every_tile(dev, Nb, W, H, Ci, Co):
    """Every partial row, both columns, against fp64 sums over the device's own stored output; (64, 80, 4, ..): 320 pixels an image, so the
    256-pixel tiles cross image boundaries."""
    M = Nb * W * H
    rows = ops.conv3x3_stats_rows(Nb, W, H, Ci, Co)
    assert rows == M // 256
    x = _gen((Nb, W, H, Ci), 1).to(BF).to(dev); w = _gen((3, 3, Ci, Co), 2, 0.05).to(BF).float()
    sign = torch.where(torch.arange(Co) % 2 == 0, 1.0, -1.0)
    b = (sign * CONV_BIAS + _gen((Co,), 3)).to(dev)
    wpack = torch.empty((Co, 3, 3, Ci), dtype=BF, device=dev)
    ops.pack_transpose(w.reshape(9 * Ci, Co).to(dev), wpack)
    wk = _Workspace(M, Co, dev)
    y = _nan((Nb, W, H, Co), dev)
    ops.conv3x3_stats(x, wpack, y, wk.fresh(), bias=b)
    wk.check_guard("conv3x3_stats")
    _assert_bits_equal("stored output", y, ops.conv3x3(x, wpack, bias=b, relu=False))
    part = wk.ws[:rows * 2 * Co * 4].view(torch.float32).view(rows, 2, Co).cpu().to(F64)
    yd = y.view(M, Co).cpu().to(F64)
    assert float((yd.mean(0).abs() / yd.std(0)).min()) > 4                      # |mean| >> std in every channel
    what = "conv3x3_stats (%d, %d, %d, %d, %d)" % (Nb, W, H, Ci, Co)
    _check(what + " tile sums", (part[:, 0] - _tiles(yd, rows)).abs(), (K3_CHAIN + 2) * EPS32 * _tiles(yd.abs(), rows))
    _check(what + " tile sums of squares", (part[:, 1] - _tiles(yd * yd, rows)).abs(), (K3_CHAIN + 2) * EPS32 * _tiles(yd * yd, rows))
    # the rest of the partial-row space stays as it was: rows * 2 * Co floats and nothing behind them
    assert bool((wk.ws[rows * 2 * Co * 4:] == POISON).all())


@pytest.mark.parametrize("Nb,W,H,Ci,Co", [(64, 64, 4, 512, 256), (64, 64, 4, 512, 512), (64, 80, 4, 512, 256), (32, 64, 8, 128, 128)])
def test_conv3x3_dgrad_epilogue_sums_every_tile(dev, Nb, W, H, Ci, Co):
    M = Nb * W * H
    rows = ops.conv3x3_bnbwd_rows(Nb, W, H, Ci, Co)
    assert rows == M // 256
    dy = _gen((Nb, W, H, Ci), 1).to(BF).to(dev); w = _gen((3, 3, Co, Ci), 2, 0.05).to(BF).float()
    wd = torch.empty((Co, 3, 3, Ci), dtype=BF, device=dev)
    ops.pack_conv_dgrad(w.to(dev), wd)
    sign = torch.where(torch.arange(Co) % 2 == 0, 1.0, -1.0)
    z = (_gen((M, Co), 3) * 2 + sign * CONV_BIAS).to(BF).to(dev)                 # the batch-norm input, |mean| >> std
    gamma = (_gen((Co,), 4) + 1.5).to(dev); beta = _gen((Co,), 5).to(dev)
    wk = _Workspace(M, Co, dev)
    yb, mean, rstd = ops.bn_train_fwd(z, gamma, beta, EPS, True, wk.fresh())
    dx = _nan((Nb, W, H, Co), dev)
    ops.conv3x3_dgrad_bnbwd(dy, wd, dx, yb.view(Nb, W, H, Co), z, mean, rstd, wk.fresh())
    wk.check_guard("conv3x3_dgrad_bnbwd")
    _assert_bits_equal("stored gradient", dx, ops.conv3x3(dy, wd, mask=yb.view(Nb, W, H, Co)))
    part = wk.ws[:rows * 2 * Co * 4].view(torch.float32).view(rows, 2, Co).cpu().to(F64)
    g = dx.view(M, Co).cpu().to(F64)
    xhat = (z.cpu().to(F64) - mean.cpu().to(F64)) * rstd.cpu().to(F64)
    what = "conv3x3_dgrad_bnbwd (%d, %d, %d, %d, %d)" % (Nb, W, H, Ci, Co)
    _check(what + " tile sums of g", (part[:, 0] - _tiles(g, rows)).abs(), (K3_CHAIN + 2) * EPS32 * _tiles(g.abs(), rows))
    _check(what + " tile sums of g xhat", (part[:, 1] - _tiles(g * xhat, rows)).abs(), (K3_CHAIN + 4) * EPS32 * _tiles((g * xhat).abs(), rows))
    assert bool((wk.ws[rows * 2 * Co * 4:] == POISON).all())
