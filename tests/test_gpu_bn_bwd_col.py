"""-m gpu: ocr_bn_train_bwd_codes_col — the batch-norm backward passes of a layer whose consumer is a 1 x 2 max-pool, with the overlap-add of the
full-height convolution behind the pool (conv5's col2im) inside the statistics pass — bit for bit against ops.conv5_col2im ->
ops.bn_train_bwd(codes=...): the pooled gradient it leaves for the apply pass, dx, dgamma and dbeta.

Four feature rows before the pool (two behind it, HC = 2 C); (Nb, W) cover w = 0, w = W - 1, an interior column and a row count that is no
multiple of the statistics pass's rows per block; C = 64 / 512 are 32 / 4 row lanes per block.  dgamma / dbeta start from non-zero contents: the
finalize kernel adds to them.  No tolerances."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import bn_reference as bnr  # noqa: E402
from test_gpu_memory_bound_kernels import _assert_bits_equal  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

BF = torch.bfloat16
EPS = bnr.f32(1e-3)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("Nb,W", [(1, 2), (2, 5), (3, 9)])
@pytest.mark.parametrize("C", [64, 512])
def test_bn_bwd_with_col2im_inside_equals_col2im_then_bn_bwd(dev, C, Nb, W, relu):
    H = 4                                               # feature rows before the pool
    M, HC = Nb * W * H, (H // 2) * C
    x = bnr.make_x(M, C, seed=M + C, ratio=4.0)
    gamma, beta = bnr.make_gamma_beta(C, seed=5)
    g = torch.Generator().manual_seed(100 * W + C)
    col = torch.randn(Nb * (W - 1), 2 * HC, generator=g).to(BF).to(dev)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    ws = ops.bn_workspace(M, C, dev)
    nan = lambda s, dt=BF: torch.full(s, float('nan'), dtype=dt, device=dev)
    codes = torch.full((M // 2, C // 8), -1, dtype=torch.int32, device=dev)
    _, mean, rstd = ops.bn_train_fwd(xd, gd, bd, EPS, relu, ws, pooled=nan((M // 2, C)), codes=codes)
    dg0, db0 = torch.rand(C, generator=g) * 4 - 2, torch.rand(C, generator=g) * 4 - 2
    # the unfused pair
    dp0 = nan((M // 2, C))
    ops.conv5_col2im(col, dp0, Nb, W, HC)
    dg_a, db_a = dg0.to(dev, copy=True), db0.to(dev, copy=True)
    dx0 = ops.bn_train_bwd(xd, None, dp0, gd, mean, rstd, dg_a, db_a, relu, ws, out=nan((M, C)), pooled_dy=True, codes=codes)
    # col2im inside the statistics pass
    dp1 = nan((M // 2, C))
    dg_b, db_b = dg0.to(dev, copy=True), db0.to(dev, copy=True)
    dx1 = ops.bn_train_bwd_codes_col(xd, codes, col, Nb, W, HC, dp1, gd, mean, rstd, dg_b, db_b, relu, ws, out=nan((M, C)))
    what = "C=%d Nb=%d W=%d relu=%d" % (C, Nb, W, relu)
    _assert_bits_equal(what + " pooled gradient", dp1, dp0)
    _assert_bits_equal(what + " dx", dx1, dx0)
    _assert_bits_equal(what + " dgamma", dg_b, dg_a)
    _assert_bits_equal(what + " dbeta", db_b, db_a)
    assert bool(torch.isfinite(dx1.float()).all()) and bool(torch.isfinite(dp1.float()).all())
    assert not torch.equal(dg_b.cpu(), dg0) and not torch.equal(db_b.cpu(), db0)
