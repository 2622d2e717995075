"""Per-launch time of the launches around the three coded max-pools of the headline step (N = 64, W = 256), each in its forms:
  conv2 forward (conv_ws, 2 x 2 pool) and conv3_2 forward (conv_k3, 1 x 2 pool): storing form / codes + store / codes only;
  maxpool_bwd against maxpool_bwd_codes behind either; batch norm + 1 x 2 pool of conv4_2 forward and backward from y / from codes.
Hot (back to back) and cold (a 512 MB scrub before every timed launch), as tools/ws_bench.py.
    python tools/pool_codes_bench.py"""
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
    print('%-34s' % name + '  '.join('%s %.1f / %.1f' % (k, timeit(f, False), timeit(f, True)) for k, f in forms) + '   (us hot / cold)', flush=True)


N = 64
for name, W, H, Ci, Co, (kw, kh) in [('conv2', 128, 16, 64, 128, (2, 2)), ('conv3_2', 64, 8, 256, 256, (1, 2))]:
    x = torch.randn(N, W, H, Ci, device=dev).to(BF)
    w = (torch.randn(Co, 3, 3, Ci, device=dev) * 0.05).to(BF)
    b = torch.zeros(Co, device=dev)
    y = torch.empty(N, W, H, Co, dtype=BF, device=dev)
    p = torch.empty(N, W // kw, H // kh, Co, dtype=BF, device=dev)
    codes = torch.empty(p.numel() // 8, dtype=torch.int32, device=dev).view(-1, Co // 8)
    kn = ops.conv3x3_kernel_choice(N, W, H, Ci, Co, pool=(kw, kh))
    forms = [('store', lambda: ops.conv3x3_relu_pool(x, w, y, p, b, kw, kh))]
    if ops.conv3x3_pool_codes_supported(N, W, H, Ci, Co, kw, kh):
        forms += [('codes+store', lambda: ops.conv3x3_relu_pool_codes(x, w, y, p, codes, b, kw, kh)),
                  ('codes', lambda: ops.conv3x3_relu_pool_codes(x, w, None, p, codes, b, kw, kh))]
    report('%s fwd (%s)' % (name, kn), forms)
    ops.conv3x3_relu_pool(x, w, y, p, b, kw, kh)
    dp, dx = torch.randn_like(p), torch.empty_like(y)
    forms = [('from y', lambda: ops.maxpool_bwd(y, dp, kw, kh, True, out=dx)),
             ('from codes', lambda: ops.maxpool_bwd_codes(codes, dp, kw, kh, True, out=dx))]
    report('maxpool_bwd %dx%d behind %s' % (kw, kh, name), forms)

M, C = N * 64 * 4, 512                          # conv4_2: [16384, 512]
z = torch.randn(M, C, device=dev).to(BF)
gamma, beta = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) - 0.5
ws = ops.bn_workspace(M, C, dev)
y, pooled = torch.empty_like(z), torch.empty(M // 2, C, dtype=BF, device=dev)
codes = torch.empty(M // 2, C // 8, dtype=torch.int32, device=dev)
sm, sr = torch.empty(C, device=dev), torch.empty(C, device=dev)
report('bn + pool fwd (3 launches)', [('y', lambda: ops.bn_train_fwd(z, gamma, beta, 1e-3, True, ws, out=y, save_mean=sm, save_rstd=sr, pooled=pooled)),
                                      ('codes', lambda: ops.bn_train_fwd(z, gamma, beta, 1e-3, True, ws, save_mean=sm, save_rstd=sr, pooled=pooled, codes=codes))])
dp, dz = torch.randn_like(pooled), torch.empty_like(z)
dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
report('bn + pool bwd (3 launches)', [('y', lambda: ops.bn_train_bwd(z, y, dp, gamma, sm, sr, dg, db, True, ws, out=dz, pooled_dy=True)),
                                      ('codes', lambda: ops.bn_train_bwd(z, None, dp, gamma, sm, sr, dg, db, True, ws, out=dz, pooled_dy=True, codes=codes))])
