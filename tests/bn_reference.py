"""fp64 reference of the training batch norm exactly as the device defines it (csrc/batchnorm.hip: bn_stats / bn_finalize / bn_apply /
bn_apply_pool / bn_bwd_stats / bn_bwd_finalize / bn_bwd_apply), plus the input generators and the launch arithmetic that the GPU test
(tests/test_gpu_bn_train.py) and the CPU test of this module (tests/test_bn_reference.py) share.  Plain module, no GPU.

bf16 inputs are taken as exact; every rounding to bf16 is torch's own `.to(torch.bfloat16)`.

  forward   mu, biased var, rstd = 1 / sqrt(var + eps), pre = (x - mu) rstd gamma + beta; with a residual the bn output is rounded to bf16
            BEFORE the add; optional ReLU; optional 1 x 2 max-pool over the row pairs (2q, 2q + 1), the first maximum winning.
  backward  dz = dy (y > 0) with the y that is passed in (the device's own); with pooled_dy the gradient [M / 2, C] is first routed to the
            first maximum of each pair; dbeta += sum dz, dgamma += sum dz xhat, dx = gamma rstd (dz - mean(dz) - xhat mean(dz xhat)).
            mean and rstd are arguments, as they are inputs of the device's backward pass.
"""
import math

import torch

BF = torch.bfloat16
F64 = torch.float64


def f32(v):
    """A Python float rounded to fp32 (what a `float` argument of the C entry point holds), as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


# ================================================================================================ forward
def statistics(x, eps):
    """mean, biased variance, rstd of the columns of x [M, C], fp64."""
    x = x.to(F64)
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    return mu, var, 1.0 / torch.sqrt(var + eps)


def forward(x, gamma, beta, eps, relu=False, residual=None, pool=False, mean=None, rstd=None):
    """-> dict: mean, var, rstd (fp64 [C]); pre (fp64 [M, C], the batch-norm output before any rounding); y (bf16 [M, C]); pooled (bf16
    [M / 2, C]) when pool.  mean / rstd given: they replace the batch statistics (the apply pass alone, with the device's statistics)."""
    x = x.to(F64)
    mu, var, rs = statistics(x, eps)
    out = dict(mean=mu, var=var, rstd=rs)
    if mean is not None:
        mu, rs = mean.to(F64), rstd.to(F64)
    pre = (x - mu) * rs * gamma.to(F64) + beta.to(F64)
    out['pre'] = pre
    o = pre
    if residual is not None:
        o = pre.to(BF).to(F64) + residual.to(F64)
    if relu:
        o = o.clamp_min(0.0)
    out['y'] = o.to(BF)
    if pool:
        out['pooled'] = pool_pairs(out['y'])
    return out


def tail(y_plain, residual, relu):
    """[relu](y_plain + residual) of a residual block from the bf16 batch-norm output y_plain: one fp64 add (exact for two bf16 values),
    one rounding."""
    o = y_plain.to(F64) + residual.to(F64)
    return (o.clamp_min(0.0) if relu else o).to(BF)


def first_max_is_second(y):
    """[M / 2, C] bool: row 2q + 1 wins its pair, which it does only when it is strictly greater (the first maximum wins a tie)."""
    return y[1::2].to(F64) > y[0::2].to(F64)


def pool_pairs(y):
    """1 x 2 max-pool over the row pairs of a bf16 [M, C] tensor: a selection, so bit-exact."""
    return torch.where(first_max_is_second(y), y[1::2], y[0::2])


def route_pairs(y, dp):
    """The full-resolution gradient [M, C] (fp64) of that pool: dp [M / 2, C] goes to the first maximum of each pair, 0 to the other row."""
    second = first_max_is_second(y)
    dp = dp.to(F64)
    g = torch.zeros(y.shape, dtype=F64)
    g[0::2] = torch.where(second, torch.zeros_like(dp), dp)
    g[1::2] = torch.where(second, dp, torch.zeros_like(dp))
    return g


# ================================================================================================ backward
def backward(x, y, dy, gamma, mean, rstd, relu, pooled_dy=False, dgamma0=None, dbeta0=None):
    """-> dict: dz, xhat, dx (fp64 [M, C], unrounded), dgamma, dbeta (fp64 [C], start values included), mdz, mdzx (fp64 [C]) and
    abs_dz, abs_dzx = sum |dz|, sum |dz xhat| (the scale of the accumulation bounds)."""
    x = x.to(F64)
    M = x.shape[0]
    mu, rs, gm = mean.to(F64), rstd.to(F64), gamma.to(F64)
    dz = route_pairs(y, dy) if pooled_dy else dy.to(F64)
    if relu:
        dz = dz * (y.to(F64) > 0)
    xhat = (x - mu) * rs
    s, sx = dz.sum(0), (dz * xhat).sum(0)
    mdz, mdzx = s / M, sx / M
    dx = gm * rs * (dz - mdz - xhat * mdzx)
    dg0 = torch.zeros_like(s) if dgamma0 is None else dgamma0.to(F64)
    db0 = torch.zeros_like(s) if dbeta0 is None else dbeta0.to(F64)
    return dict(dz=dz, xhat=xhat, dx=dx, dgamma=dg0 + sx, dbeta=db0 + s, mdz=mdz, mdzx=mdzx,
                abs_dz=dz.abs().sum(0), abs_dzx=(dz * xhat).abs().sum(0))


# ================================================================================================ launch arithmetic (batchnorm.hip)
def rows_per_block(M, target):
    """bn_rows_per_block_host: rows per block for about `target` blocks, a multiple of 8, at least 8."""
    r = (M + target - 1) // target
    r = (r + 7) // 8 * 8
    return max(r, 8)


FWD_TARGET, BWD_TARGET, ROWS_PER_THREAD, RED_FLOATS = 256, 512, 4, 2048


def layout(M, C):
    """The thread layout and grid of the passes over [M, C]: groups of 8 channels along the 256 threads of a workgroup, rlanes row lanes.
    chain_fwd / chain_bwd: the longest fp32 summation chain of the statistics passes = rows per thread + row lanes (the LDS lane sum)."""
    groups = C // 8
    rlanes = 256 // groups
    rpb_f, rpb_b = rows_per_block(M, FWD_TARGET), rows_per_block(M, BWD_TARGET)
    arows = ROWS_PER_THREAD * rlanes
    per_thread = lambda rpb: -(-min(rpb, M) // rlanes)
    return dict(groups=groups, rlanes=rlanes, idle_threads=256 - groups * rlanes, red_used=rlanes * C,
                rpb_fwd=rpb_f, nblk_fwd=-(-M // rpb_f), rpb_bwd=rpb_b, nblk_bwd=-(-M // rpb_b),
                arows=arows, nblk_apply=-(-M // arows),
                chain_fwd=per_thread(rpb_f) + rlanes, chain_bwd=per_thread(rpb_b) + rlanes)


def workspace_bytes(M, C):
    """ocr_bn_workspace_bytes: the backward pass's partial rows [nblk][2][C] fp32, then 2 C doubles."""
    return -(-M // rows_per_block(M, BWD_TARGET)) * 2 * C * 4 + 2 * C * 8


# ================================================================================================ input generators
# Eight per-channel regimes, channel c takes REGIMES[c % 8], so every tensor of the GPU test carries all of them (C = 8: one channel each).
REGIMES = ('benign', 'offset_pos', 'offset_neg', 'constant', 'outlier', 'gamma_zero', 'gamma_neg', 'benign')
CONSTANTS = (0.5, -0.75)           # bf16 values whose square times (chain + 2) 2^-24 / eps stays below 2^-9 at every product shape
OUTLIER = 100.0
TIE_EVERY = 4                      # dense ties: in every fourth row pair the second row duplicates the first


def regime_of(c):
    return REGIMES[c % len(REGIMES)]


def channels_of(C, name):
    return [c for c in range(C) if regime_of(c) == name]


def make_x(M, C, seed, ratio, ties=True):
    """bf16 [M, C].  benign / gamma_*: uniform on [-1.5, 2.5) (mean 0.5, std 1.15: E[x^2] / var about 1.2);  offset_pos / offset_neg:
    normal with std 1 around +ratio / -ratio (|mean| / std = ratio);  constant: one bf16 value in the whole channel;  outlier: that
    value, but OUTLIER in one row.  ties: rows 2q + 1 = rows 2q for every TIE_EVERY-th pair, in all channels."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, C, generator=g) * 4 - 1.5
    n = torch.randn(M, C, generator=g)
    for c in range(C):
        r = regime_of(c)
        if r == 'offset_pos':
            x[:, c] = n[:, c] + ratio
        elif r == 'offset_neg':
            x[:, c] = n[:, c] - ratio
        elif r in ('constant', 'outlier'):
            x[:, c] = CONSTANTS[(c // len(REGIMES)) % 2]
            if r == 'outlier':
                x[outlier_row(M), c] = OUTLIER
    x = x.to(BF)
    if ties:
        first = torch.arange(0, M - 1, 2 * TIE_EVERY)
        x[first + 1] = x[first]
    return x


def outlier_row(M):
    """The one row of an `outlier` channel that differs: in the last block of every pass, and the first row of a pair that is not tied."""
    r = (M - 1) // 2 * 2
    return r if (r // 2) % TIE_EVERY or M < 2 else max(r - 2, 0)


def make_gamma_beta(C, seed):
    """gamma in [0.5, 2.5), exactly 0 in gamma_zero channels and negative in gamma_neg channels; beta in [-1, 1), never 0."""
    g = torch.Generator().manual_seed(seed)
    gamma = torch.rand(C, generator=g) * 2 + 0.5
    beta = torch.rand(C, generator=g) * 2 - 1
    beta = torch.where(beta == 0, torch.full_like(beta, 0.25), beta)
    for c in range(C):
        if regime_of(c) == 'gamma_zero':
            gamma[c] = 0.0
        elif regime_of(c) == 'gamma_neg':
            gamma[c] = -gamma[c]
    return gamma, beta


def kappa(x, eps):
    """E[x^2] / (var + eps) per channel: the factor by which the one-pass variance ss / M - mu^2 amplifies the rounding of ss."""
    x = x.to(F64)
    _, var, _ = statistics(x, eps)
    return (x * x).mean(0) / (var + eps)


def offset_ratio_for(chain, asked):
    """The largest |mean| / std <= asked at which the derived rstd bound (chain + 2) 2^-24 kappa / 2 with kappa = 1 + ratio^2 still stays
    5 % below 2^-10 (the margin is for the sample's own kappa, which is not exactly 1 + ratio^2)."""
    most = math.sqrt(0.95 * 2.0 ** 15 / (chain + 2) - 1)
    return min(asked, math.floor(most * 2) / 2)
