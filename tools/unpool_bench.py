"""Per-launch time of the three backward hand-offs of the headline step (N = 64, W = 256) that moved into the kernels in front of them:
  the data gradients of conv3_1 (behind pool2, 2 x 2) and conv4_1 (behind conv3_2's pool, 1 x 2): conv3x3 + maxpool_bwd_codes against
  conv3x3_dgrad_unpool;
  conv5's col2im + conv4_2's batch-norm backward (3 launches) against bn_train_bwd_codes_col (3 launches).
Hot (back to back) and cold (a 512 MB scrub before every timed launch), as tools/pool_codes_bench.py.
    python tools/unpool_bench.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstm_ctc_ocr_amd import ops  # noqa: E402

dev = torch.device('cuda:0'); BF = torch.bfloat16
scrub = torch.empty(512 << 20, dtype=torch.uint8, device=dev)


def timeit(fn, cold):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(7 if cold else 3):
        if cold:
            scrub.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 1 if cold else 50
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return sorted(ts)[len(ts) // 2]


def report(name, forms):
    print('%-44s' % name + '  '.join('%s %.1f / %.1f' % (k, timeit(f, False), timeit(f, True)) for k, f in forms) + '   (us hot / cold)', flush=True)


N = 64
for name, W, H, Ci, Co, (kw, kh) in [('conv3_1 dgrad + pool2 bwd', 64, 8, 256, 128, (2, 2)), ('conv4_1 dgrad + pool bwd', 64, 4, 512, 256, (1, 2))]:
    dy = torch.randn(N, W, H, Ci, device=dev).to(BF)
    wd = (torch.randn(Co, 3, 3, Ci, device=dev) * 0.05).to(BF)
    pooled = torch.empty(N, W, H, Co, dtype=BF, device=dev)
    full = torch.empty(N, W * kw, H * kh, Co, dtype=BF, device=dev)
    codes = torch.randint(0, kw * kh, (N * W * H, Co // 8, 8), device=dev, dtype=torch.int32)
    codes = ((codes | 4) << (4 * torch.arange(8, device=dev, dtype=torch.int32))).sum(-1).to(torch.int32)
    kn = ops.conv3x3_kernel_choice(N, W, H, Ci, Co, bias=False, relu=False)

    def pair():
        ops.conv3x3(dy, wd, out=pooled)
        ops.maxpool_bwd_codes(codes, pooled, kw, kh, True, out=full)
    forms = [('dgrad', lambda: ops.conv3x3(dy, wd, out=pooled)), ('pool bwd', lambda: ops.maxpool_bwd_codes(codes, pooled, kw, kh, True, out=full)),
             ('pair', pair)]
    if ops.conv3x3_unpool_supported(N, W, H, Ci, Co, kw, kh):
        forms.append(('unpool', lambda: ops.conv3x3_dgrad_unpool(dy, wd, codes, kw, kh, True, out=full)))
    report('%s (%s)' % (name, kn), forms)

M, C, W, HC = N * 64 * 4, 512, 64, 2 * 512         # conv4_2: [16384, 512]; conv5's column matrix [64 * 63][2 * 1024]
z = torch.randn(M, C, device=dev).to(BF)
gamma, beta = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) - 0.5
ws = ops.bn_workspace(M, C, dev)
pooled = torch.empty(M // 2, C, dtype=BF, device=dev)
codes = torch.empty(M // 2, C // 8, dtype=torch.int32, device=dev)
sm, sr = torch.empty(C, device=dev), torch.empty(C, device=dev)
ops.bn_train_fwd(z, gamma, beta, 1e-3, True, ws, save_mean=sm, save_rstd=sr, pooled=pooled, codes=codes)
col = torch.randn(N * (W - 1), 2 * HC, device=dev).to(BF)
dp, dz = torch.empty_like(pooled), torch.empty_like(z)
dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)


def pair():
    ops.conv5_col2im(col, dp, N, W, HC)
    ops.bn_train_bwd(z, None, dp, gamma, sm, sr, dg, db, True, ws, out=dz, pooled_dy=True, codes=codes)


report('col2im + bn bwd of conv4_2', [('col2im', lambda: ops.conv5_col2im(col, dp, N, W, HC)),
                                      ('bn bwd', lambda: ops.bn_train_bwd(z, None, dp, gamma, sm, sr, dg, db, True, ws, out=dz, pooled_dy=True, codes=codes)),
                                      ('pair', pair),
                                      ('fused', lambda: ops.bn_train_bwd_codes_col(z, codes, col, N, W, HC, dp, gamma, sm, sr, dg, db, True, ws, out=dz))])
