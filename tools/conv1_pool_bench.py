"""Per-launch time of the fused conv1 + ReLU + 2 x 2 max-pool launches of the train step, stand-alone, by the loaded library:
  forward-train (pooled map + routing codes) with and without the two fills that ride on it in the step (the flat gradient buffer's clear and
  the LSTM hand-off blocks' all-ones fill, at the headline step's sizes), the inference forward, and the slab backward from saved codes and
  from recomputed windows — at the headline shape 64 x 256 x 32 and the variable-width extreme 64 x 320 x 32.
Beside each time: the bytes the launch has to move, computed from the shapes, per microsecond, and the time those bytes take at RATE (the
5.8 TB/s adam_update_kernel reaches in profiles/r11_pmc_step_fixed.json).  Hot (back to back) and cold (a 512 MB scrub before every timed launch).
    python tools/conv1_pool_bench.py
    OCR_NATIVE_LIB=lstm_ctc_ocr_amd/libocrhip_exp.so OCR_CONV1_FWD_PPB=64 python tools/conv1_pool_bench.py        # another forward block size"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

dev = torch.device('cuda:0'); BF = torch.bfloat16
RATE = 5.8e6                                    # bytes per microsecond
ZERO_WORDS, ONES_WORDS = 7_000_000, 1_048_576   # the step's gradient buffer (28 MB) and hand-off blocks (4 MB), rounded
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


def report(name, fn, nbytes):
    hot, cold = timeit(fn, False), timeit(fn, True)
    print('%-44s %7.1f / %7.1f us hot / cold   %6.1f MB  %7.0f / %7.0f bytes/us   floor %5.1f us'
          % (name, hot, cold, nbytes / 1e6, nbytes / hot, nbytes / cold, nbytes / RATE), flush=True)


print('library %s  build %s  OCR_CONV1_FWD_PPB=%s OCR_CONV1_PPB=%s'
      % (os.path.basename(nat.LIB_PATH), nat.build_id(), *(os.environ.get(k, '-') for k in ('OCR_CONV1_FWD_PPB', 'OCR_CONV1_PPB'))))
for N, W, H in ((64, 256, 32), (64, 320, 32)):
    Co = 64
    npix = N * (W // 2) * (H // 2)
    x = torch.rand(N, W, H, device=dev)
    w = (torch.rand(9, Co, device=dev) - 0.5) * 0.6
    b = (torch.rand(Co, device=dev) - 0.5) * 0.2
    p = torch.empty(N, W // 2, H // 2, Co, dtype=BF, device=dev)
    codes = torch.empty(npix, 8, dtype=torch.int32, device=dev)
    zero = torch.empty(ZERO_WORDS, device=dev)
    ones = torch.empty(ONES_WORDS, dtype=torch.int32, device=dev)
    dp = torch.randn(N, W // 2, H // 2, Co, device=dev).to(BF)
    slab = torch.empty(ops.conv1_pool_bwd_slab_rows(N, W, H), 640, device=dev)
    b_x, b_p, b_c, b_par = x.numel() * 4, p.numel() * 2, codes.numel() * 4, (w.numel() + b.numel()) * 4
    print('%d x %d x %d: %d pooled pixels, slab rows %d' % (N, W, H, npix, slab.shape[0]))
    report('fwd train, with fills', lambda: ops.conv1_pool_fwd(x, w, b, out=p, zero=zero, codes=codes, ones=ones),
           b_x + b_par + b_p + b_c + (ZERO_WORDS + ONES_WORDS) * 4)
    report('fwd train, without fills', lambda: ops.conv1_pool_fwd(x, w, b, out=p, codes=codes), b_x + b_par + b_p + b_c)
    report('fwd inference', lambda: ops.conv1_pool_fwd(x, w, b, out=p), b_x + b_par + b_p)
    ops.conv1_pool_fwd(x, w, b, out=p, codes=codes)
    report('bwd slab, codes', lambda: ops.conv1_pool_bwd_slab(x, w, b, dp, slab, codes=codes), b_x + b_p + b_c + slab.numel() * 4)
    report('bwd slab, recompute', lambda: ops.conv1_pool_bwd_slab(x, w, b, dp, slab), b_x + b_par + b_p + slab.numel() * 4)
