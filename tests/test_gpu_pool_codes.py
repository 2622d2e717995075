"""-m gpu: the max-pool routing codes (4 bits per pooled output, conv1's format) that the training forward pass of a pooled layer writes
instead of its full-resolution output, and the backward kernels that read them — bit for bit against the kernels that work on the stored
tensor: maxpool_bwd_codes against maxpool_bwd, the codes forms of conv_ws / conv_k3's pool write-outs against their storing forms, batch
norm + pool from codes against the y-based passes, and one training step of the engine with OCR_POOL_CODES=1 against =0.

The codes themselves are checked against tests/pool_codes_model.py (numpy), which tests/test_pool_codes_model.py checks on the CPU."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import bn_reference as bnr  # noqa: E402
from pool_codes_model import pool_codes, windows  # noqa: E402
from test_gpu_memory_bound_kernels import _assert_bits_equal  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

BF = torch.bfloat16
EPS = bnr.f32(1e-3)
GRID = (-1.0, -0.5, -0.0, 0.0, 0.5, 1.0)      # coarse: ties decide most windows; -0.0 == 0.0 and neither is > 0


def _codes_dev(words, dev):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)


def _codes_host(t):
    return t.cpu().numpy().view(np.uint32)


# ================================================================================================ maxpool_bwd_codes
@pytest.mark.parametrize("relu_mask", [False, True])
@pytest.mark.parametrize("shape", [(2, 8, 4, 64), (1, 2, 2, 8), (3, 6, 8, 136)])
@pytest.mark.parametrize("kw,kh", [(2, 2), (1, 2)])
def test_maxpool_bwd_codes_equals_maxpool_bwd(dev, kw, kh, shape, relu_mask):
    N, W, H, C = shape
    g = torch.Generator().manual_seed(1000 * kw + 10 * C + W)
    grid = torch.tensor(GRID)
    x = grid[torch.randint(0, len(GRID), shape, generator=g)]
    # two of every five (window, channel) repeat the window's first value in its last element (a 1 x 2 pair of independent draws ties only
    # 22 % of the time); window 0, channel 0 holds no positive value and ties -0.0 with 0.0
    xw = x.view(N, W // kw, kw, H // kh, kh, C)
    tie = (torch.arange(N * (W // kw) * (H // kh) * C) % 5 < 2).view(N, W // kw, H // kh, C)
    xw[:, :, kw - 1, :, kh - 1, :] = torch.where(tie, xw[:, :, 0, :, 0, :], xw[:, :, kw - 1, :, kh - 1, :])
    xw[0, 0, :, 0, :, 0] = torch.tensor([-0.0, 0.0, -0.5, 0.0])[:kw * kh].view(kw, kh)
    x = x.to(BF)
    assert set(x.float().flatten().tolist()) <= set(GRID)
    dy = (torch.randn(N, W // kw, H // kh, C, generator=g) * 2).to(BF)
    # the inputs prove something only if ties and all-non-positive windows are common (checked on the CPU)
    win = windows(x.float().numpy(), kw, kh)
    mx = win.max(axis=-2, keepdims=True)
    shared = ((win == mx).sum(axis=-2) > 1).mean()
    nonpos = (mx <= 0).mean()
    assert shared >= 0.30, "only %.0f %% of the windows hold a shared maximum" % (100 * shared)
    assert (mx <= 0).any(), "no window without a positive element"
    print("shared maxima in %.0f %% of the windows, %.1f %% without a positive element" % (100 * shared, 100 * nonpos))
    words, _ = pool_codes(x.float().numpy(), kw, kh)
    assert words.shape == (N * (W // kw) * (H // kh), C // 8)
    xd, dyd = x.to(dev), dy.to(dev)
    want = ops.maxpool_bwd(xd, dyd, kw, kh, relu_mask=relu_mask, out=torch.full(shape, float('nan'), dtype=BF, device=dev))
    got = ops.maxpool_bwd_codes(_codes_dev(words, dev), dyd, kw, kh, relu_mask, out=torch.full(shape, float('nan'), dtype=BF, device=dev))
    _assert_bits_equal("maxpool_bwd_codes %dx%d %s relu_mask=%d" % (kw, kh, shape, relu_mask), got, want)


# ================================================================================================ convolution forward
# The smallest shapes at which the plan takes each kernel with a fused pool (the candidates are in ascending size; the plan functions decide):
# conv_ws (Cin = 64, H = 16) from two 256-pixel tiles per CU on — a grid of 64 pixel tiles x 8 channel tiles; one whose 65 pixel tiles do
# not divide among the workgroups (the last workgroup of a channel tile runs short); conv_k3 with both tiles and both windows.
CONV_WS_CANDIDATES = [(4, 256, 16, 64, 512), (8, 128, 16, 64, 512), (8, 256, 16, 64, 512)]
CONV_WS_RAGGED = [(5, 208, 16, 64, 512), (5, 416, 16, 64, 512)]
CONV_K3_CANDIDATES = {
    "conv_k3/A": [(8, 128, 8, 128, 1024), (64, 64, 8, 256, 256)],       # 224 tiles of 256 pixels x 128 channels; else conv3_2 of the headline step
    "conv_k3/D": [(8, 64, 8, 128, 512), (8, 128, 8, 128, 256)],
    "conv_k3/D, H = 4": [(16, 64, 4, 128, 512), (8, 128, 4, 128, 512)],
    "conv_k3/D, H = 16": [(4, 64, 16, 128, 512), (8, 64, 16, 128, 256)]}


def _first_planned(cands, kernel, pool):
    for s in cands:
        if (ops.conv3x3_kernel_choice(*s, pool=pool) == kernel and ops.conv3x3_pool_supported(*s, *pool)):
            return s
    pytest.fail("no candidate shape is planned on %s with a %d x %d pool: %r" % (kernel, pool[0], pool[1],
                                                                              [ops.conv3x3_kernel_choice(*s, pool=pool) for s in cands]))


def _conv_case(dev, shape, pool):
    N, W, H, Ci, Co = shape
    kw, kh = pool
    assert ops.conv3x3_pool_codes_supported(N, W, H, Ci, Co, kw, kh)
    g = torch.Generator().manual_seed(N * 1000 + W)
    # coarse inputs and weights: many outputs round to the same bf16 value (ties inside windows), about half are cut by the ReLU
    x = (torch.randint(-2, 3, (N, W, H, Ci), generator=g).float() * 0.5).to(BF).to(dev)
    w = (torch.randint(-1, 2, (Co, 3, 3, Ci), generator=g).float() * 0.125).to(BF).to(dev)
    b = (torch.randint(-2, 3, (Co,), generator=g).float() * 0.25).to(dev)
    po = (N, W // kw, H // kh, Co)
    nan = lambda s: torch.full(s, float('nan'), dtype=BF, device=dev)
    y0, p0 = ops.conv3x3_relu_pool(x, w, nan((N, W, H, Co)), nan(po), b, kw, kh)
    words, _ = pool_codes(y0.float().cpu().numpy(), kw, kh)
    win = windows(y0.float().cpu().numpy(), kw, kh)
    shared = ((win == win.max(axis=-2, keepdims=True)).sum(axis=-2) > 1).mean()
    print("%s %dx%d: shared maxima in %.0f %% of the windows" % (shape, kw, kh, 100 * shared))
    assert shared > 0.05
    nwin = N * (W // kw) * (H // kh)
    for keep_y in (True, False):
        codes = torch.full((nwin, Co // 8), -1, dtype=torch.int32, device=dev)
        y1 = nan((N, W, H, Co)) if keep_y else None
        _, p1, _ = ops.conv3x3_relu_pool_codes(x, w, y1, nan(po), codes, b, kw, kh)
        what = "%s %dx%d %s" % (shape, kw, kh, "codes + store" if keep_y else "codes only")
        _assert_bits_equal(what + " pooled", p1, p0)
        if keep_y:
            _assert_bits_equal(what + " y", y1, y0)
        got = _codes_host(codes)
        bad = np.argwhere(got != words)
        assert len(bad) == 0, "%s: %d of %d code words differ, first at %r: got %#x, want %#x" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], words[tuple(bad[0])])


@pytest.mark.parametrize("pool", [(2, 2), (1, 2)])
@pytest.mark.parametrize("ragged", [False, True])
def test_conv_ws_codes_forms(dev, pool, ragged):
    _conv_case(dev, _first_planned(CONV_WS_RAGGED if ragged else CONV_WS_CANDIDATES, "conv_ws", pool), pool)


@pytest.mark.parametrize("pool", [(2, 2), (1, 2)])
@pytest.mark.parametrize("kernel", sorted(CONV_K3_CANDIDATES))
def test_conv_k3_codes_forms(dev, kernel, pool):
    _conv_case(dev, _first_planned(CONV_K3_CANDIDATES[kernel], kernel.split(',')[0], pool), pool)


def test_codes_form_only_where_the_planned_kernel_has_it(dev):
    """conv_k2 / conv_halo / the general-width conv_k3 have no codes write-out: the query says so and the call refuses."""
    seen = set()
    for s, pool in [((32, 24, 8, 64, 128), (1, 2)), ((4, 32, 16, 64, 128), (2, 2)), ((32, 40, 8, 128, 256), (1, 2)), ((64, 80, 8, 256, 256), (1, 2)),
                    ((8, 64, 8, 128, 512), (2, 2))]:
        k = ops.conv3x3_kernel_choice(*s, pool=pool)
        seen.add(k)
        has = ops.conv3x3_pool_codes_supported(*s, *pool)
        assert has == (ops.conv3x3_pool_supported(*s, *pool) and k in ("conv_ws", "conv_k3/A", "conv_k3/D")), (s, k, has)
    assert {"conv_halo", "conv_k3w/A", "conv_k3w/D", "conv_k3/D"} <= seen, seen
    s = (4, 32, 16, 64, 128)
    assert not ops.conv3x3_pool_codes_supported(*s, 2, 2)
    N, W, H, Ci, Co = s
    x = torch.zeros((N, W, H, Ci), dtype=BF, device=dev)
    w = torch.zeros((Co, 3, 3, Ci), dtype=BF, device=dev)
    with pytest.raises(Exception):
        ops.conv3x3_relu_pool_codes(x, w, None, torch.empty((N, W // 2, H // 2, Co), dtype=BF, device=dev),
                                    torch.empty((N * (W // 2) * (H // 2), Co // 8), dtype=torch.int32, device=dev), torch.zeros(Co, device=dev), 2, 2)


# ================================================================================================ batch norm + pool
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("M,C", [(64, 64), (64, 512)])
def test_bn_pool_from_codes_equals_from_y(dev, M, C, relu):
    x = bnr.make_x(M, C, seed=M + C, ratio=4.0)
    tied = bnr.channels_of(C, 'benign')[0]
    x[1::2, tied] = x[0::2, tied]                         # a channel whose pairs ALL tie (a constant channel is one too, with var = 0)
    assert bnr.channels_of(C, 'constant')
    gamma, beta = bnr.make_gamma_beta(C, seed=5)
    g = torch.Generator().manual_seed(9)
    dp = torch.randn(M // 2, C, generator=g).to(BF).to(dev)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    ws = ops.bn_workspace(M, C, dev)
    nan = lambda s, dt=BF: torch.full(s, float('nan'), dtype=dt, device=dev)
    pooled0 = nan((M // 2, C))
    y0, sm0, sr0 = ops.bn_train_fwd(xd, gd, bd, EPS, relu, ws, out=nan((M, C)), pooled=pooled0)
    pooled1, codes = nan((M // 2, C)), torch.full((M // 2, C // 8), -1, dtype=torch.int32, device=dev)
    y1, sm1, sr1 = ops.bn_train_fwd(xd, gd, bd, EPS, relu, ws, save_mean=nan((C,), torch.float32), save_rstd=nan((C,), torch.float32),
                                    pooled=pooled1, codes=codes)
    what = "[%d, %d] relu=%d" % (M, C, relu)
    assert y1 is None
    _assert_bits_equal(what + " pooled", pooled1, pooled0)
    _assert_bits_equal(what + " mean", sm1, sm0)
    _assert_bits_equal(what + " rstd", sr1, sr0)
    words, code = pool_codes(y0.float().cpu().numpy().reshape(1, M // 2, 2, C), 1, 2)
    assert np.array_equal(_codes_host(codes), words), what + " codes"
    assert not (code[0, :, 0, tied] & 1).any() and not (code[0, :, 0, bnr.channels_of(C, 'constant')[0]] & 1).any()       # ties: the first row wins
    dg0, db0 = torch.rand(C, generator=g) * 4 - 2, torch.rand(C, generator=g) * 4 - 2
    outs = []
    for use_codes in (False, True):
        dg, db = dg0.to(dev, copy=True), db0.to(dev, copy=True)
        dz = ops.bn_train_bwd(xd, None if use_codes else y0, dp, gd, sm0, sr0, dg, db, relu, ws, out=nan((M, C)), pooled_dy=True,
                              codes=codes if use_codes else None)
        outs.append((dz, dg, db))
    for name, a, b in zip(("dz", "dgamma", "dbeta"), outs[1], outs[0]):
        _assert_bits_equal("%s %s" % (what, name), a, b)
    assert bool(torch.isfinite(outs[1][0].float()).all())


# ================================================================================================ engine
def _one_step_digest():
    """(child process) one training step of the headline network at N = 4, W = 32 -> sha256 of every parameter and of the loss."""
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    from test_gpu_engine import make_batch
    cfg.TRAIN.WEIGHT_DECAY, cfg.TRAIN.LEARNING_RATE, cfg.TRAIN.SOLVER = 1e-5, 1e-4, 'Adam'
    eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3)
    eng.setup_optimizer('Adam', 1e-3)
    x, labels, ll, sl = make_batch(4, 32, 2, 4, 21)
    loss = eng.train_step(x, labels, ll, sl)
    sp = eng.plan(4, 32)
    out = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(eng.state_arrays().items())}
    out['loss'] = repr(float(loss))
    out['code buffers'] = sorted(k for k in sp.buf if k.endswith('/pool_codes'))
    out['y buffers'] = sorted(k for k in sp.buf if k.endswith('/y'))
    print(json.dumps(out))


def test_engine_step_is_bit_identical_with_and_without_codes(dev):
    def run(flag):
        env = {k: v for k, v in os.environ.items() if not k.startswith("OCR_")}
        env.update(OCR_POOL_CODES=flag)
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.splitlines()[-1])
    on, off = run('1'), run('0')
    extra = set(on['code buffers']) - set(off['code buffers'])
    assert extra, "OCR_POOL_CODES=1 added no code buffer to the plan: %r" % on['code buffers']
    for k in extra:                                       # a layer with codes keeps no full-resolution output in a training plan
        assert k[:-len('/pool_codes')] + '/y' not in on['y buffers'] and k[:-len('/pool_codes')] + '/y' in off['y buffers']
    diff = [k for k in off if k not in ('code buffers', 'y buffers') and on[k] != off[k]]
    assert not diff, "differs between OCR_POOL_CODES=1 and =0: %r" % diff
    assert len(on) > 10


if __name__ == "__main__":
    _one_step_digest()
