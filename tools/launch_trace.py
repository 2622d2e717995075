"""Print every call the host makes into libocrhip.so while it builds an engine and a plan and runs one eager training step: one line per
call with the entry point's name, its scalar arguments, and each pointer replaced by the ordinal of its first appearance (p0, p1, ...).
Two checkouts that issue the same work print the same text, whatever addresses the allocator hands out — run this file on both
(under the same OCR_* environment) and compare the outputs byte for byte.

    python tools/launch_trace.py --model LSTM_train --batch 8 --width 88 > trace.txt
    python tools/launch_trace.py --model deep --batch 4 --width 32 > trace.txt
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Traced(object):
    """Stands in for the ctypes library object of _native.lib(): every function it hands out logs the call before making it."""

    def __init__(self, lib, sigs, out):
        self._lib, self._sigs, self._out, self._ordinal = lib, sigs, out, {}

    def __getattr__(self, name):
        fn, argtypes = getattr(self._lib, name), self._sigs[name][0]

        def traced(*args):
            shown = []
            for t, a in zip(argtypes, args):
                if t is ctypes.c_void_p and (a is None or isinstance(a, int)):
                    shown.append('null' if not a else 'p%d' % self._ordinal.setdefault(a, len(self._ordinal)))
                elif t is ctypes.c_void_p:
                    shown.append('host')            # a ctypes object: a table in host memory (its address says nothing)
                elif issubclass(t, ctypes._Pointer):
                    shown.append('&')               # a host output slot (sizes)
                else:
                    shown.append(repr(a))
            self._out.write('%s(%s)\n' % (name, ', '.join(shown)))
            return fn(*args)
        return traced


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=['LSTM_train', 'deep'], default='LSTM_train')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--width', type=int, default=88)
    args = ap.parse_args()

    import torch
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network

    nat._lib = Traced(nat.lib(), nat._SIGS, sys.stdout)     # ops reaches the library through nat.call / nat.lib(), the engine too
    cfg.TRAIN.SOLVER, cfg.TRAIN.LEARNING_RATE, cfg.TRAIN.WEIGHT_DECAY = 'Adam', 1e-4, 1e-5
    name = args.model
    if name == 'deep':                                      # what `bench.py --workload deep` builds
        cfg.NCLASSES, cfg.TRAIN.NUM_LAYERS, cfg.TRAIN.NUM_HID, name = 96, 2, 1024, 'RESNET_train'
    N, W = args.batch, args.width
    T = W // 4 - 1
    rng = np.random.RandomState(7)
    L = max(1, min(4, T // 3))
    x = rng.rand(N, W, cfg.NUM_FEATURES).astype(np.float32)
    labels = rng.randint(1, cfg.NCLASSES - 1, N * L).astype(np.int32)
    ll, sl = np.full(N, L, np.int32), np.full(N, T, np.int32)

    eng = Engine(get_network(name), device='cuda:0', seed=5, use_graphs=False)
    sp = eng.plan(N, W)
    eng._bind(sp, x, sl, labels, ll)
    eng._run(sp, 'fb')
    eng.optimizer_step(sp)
    torch.cuda.synchronize()
    sys.stdout.write('# mean CTC cost %r\n' % float(sp.costs.double().mean()))      # the step's result rides along in the comparison


if __name__ == '__main__':
    main()
