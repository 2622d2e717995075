"""Time the beam search fused with a label automaton (ocr_ctc_beam_decode_lm) at N = 64, T = 63, K = 100 on the logits recipe of
tools/beam_bench.py (randn * 3 with boosted blank and class-0 frames):

  1. with --parent <another build's libocrhip.so>: ocr_ctc_beam_decode and ocr_ctc_beam_decode_nbest on that library and on this build, three
     alternating pairs in one process, the outputs hashed (both libraries are loaded side by side with ctypes; the parent lacks the new
     entry points, so it cannot go through _native);
  2. the fused entry against ocr_ctc_beam_decode_nbest on this build at C = 40: the zero automaton, a bigram (40 states) and a trigram (1561
     states), top_paths 1 and 5;
  3. with --engine: Engine.decode_nbest_beam(k=5) beside Engine.decode_nbest_beam_lm(trigram, k=5) on the trained fixture's batch C2 (host clock).

Device calls sit between their own pair of events; min / median / max over the repetitions, in microseconds.
    python tools/beam_lm_bench.py [--reps 20] [--warmup 5] [--parent PATH] [--engine]"""
import argparse
import ctypes
import hashlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from lstm_ctc_ocr_amd.automaton import LabelAutomaton  # noqa: E402
from lstm_ctc_ocr_amd.rescoring import CharNGram  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctc_score_bench import timed  # noqa: E402

T, N, K = 63, 64, 100
P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def logits(C, dev):
    rng = np.random.RandomState(7)
    a = (rng.randn(T, N, C) * 3).astype(np.float32)
    a[rng.rand(T, N) < 0.3, C - 1] += 5.0
    a[rng.rand(T, N) < 0.3, 0] += 5.0
    return torch.tensor(a, device=dev)


def fitted(order, C):
    rng = np.random.RandomState(order)
    return CharNGram(order, C).fit([list(1 + rng.randint(0, C - 1, rng.randint(3, 12))) for _ in range(4 * C)])


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:12]


def old_entries(path, C, dev, args):
    """(name -> (min, median, max, hash)) of the two existing entries on the library at `path`."""
    lib = ctypes.CDLL(path)
    lib.ocr_build_id.restype = ctypes.c_char_p
    lib.ocr_ctc_beam_workspace_size.argtypes = [I, I, I, I, ctypes.POINTER(Z)]
    lib.ocr_ctc_beam_decode.argtypes = [P, P, I, I, I, I, I, I, P, P, P, P, Z, P]
    lib.ocr_ctc_beam_decode_nbest.argtypes = [P, P, I, I, I, I, I, I, I, I, P, P, P, P, P, Z, P]
    a = logits(C, dev)
    il = torch.full((N,), T, dtype=torch.int32, device=dev)
    sz = Z(0)
    assert lib.ocr_ctc_beam_workspace_size(C, N, T, K, ctypes.byref(sz)) == 0
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    out = torch.zeros((N, 5, T), dtype=torch.int32, device=dev)
    lens = torch.zeros((N, 5), dtype=torch.int32, device=dev)
    nlp = torch.zeros((N, 5), dtype=torch.float32, device=dev)
    count = torch.zeros(N, dtype=torch.int32, device=dev)
    st = nat.stream()

    def single():
        assert lib.ocr_ctc_beam_decode(a.data_ptr(), il.data_ptr(), C, N, T, K, 1, 0, out.data_ptr(), lens.data_ptr(), nlp.data_ptr(), ws.data_ptr(),
                                       ws.numel(), st) == 0

    def nbest():
        assert lib.ocr_ctc_beam_decode_nbest(a.data_ptr(), il.data_ptr(), C, N, T, K, 5, 0, 0, 0, out.data_ptr(), lens.data_ptr(), nlp.data_ptr(),
                                             count.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    res = {}
    for name, fn in (("ocr_ctc_beam_decode", single), ("ocr_ctc_beam_decode_nbest(5, blank 0)", nbest)):
        for t in (out, lens, nlp, count):
            t.zero_()
        res[name] = timed(fn, args.reps, args.warmup) + (digest(out, lens, nlp, count),)
    return lib.ocr_build_id().decode(), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--engine', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    print('build %s' % nat.build_id(), flush=True)
    ok = True
    C = 40
    if args.parent:
        hashes = {}
        for pair in range(3):
            for tag, path in (('parent', args.parent), ('this build', nat.LIB_PATH)):
                build, res = old_entries(path, C, dev, args)
                for name, (lo, med, hi, h) in res.items():
                    print('pair %d  %-10s %s  %-40s min %.1f median %.1f max %.1f us  hash %s' % (pair, tag, build, name, lo, med, hi, h), flush=True)
                    hashes.setdefault(name, set()).add(h)
        for name, hs in hashes.items():
            print('%s: outputs %s' % (name, 'equal in all six runs' if len(hs) == 1 else 'DIFFER'), flush=True)
            ok &= len(hs) == 1

    a = logits(C, dev)
    il = torch.full((N,), T, dtype=torch.int32, device=dev)
    automata = (('zero', LabelAutomaton.zero(C)), ('bigram', LabelAutomaton.from_ngram(fitted(2, C), 0.7, 0.3)),
                ('trigram', LabelAutomaton.from_ngram(fitted(3, C), 0.7, 0.3)))
    for top in (1, 5):
        lo, med, hi = timed(lambda: ops.ctc_beam_nbest(a, il, top, beam_width=K, blank=0), args.reps, args.warmup)
        print('C = %d top_paths %d  ocr_ctc_beam_decode_nbest                  min %.1f median %.1f max %.1f us' % (C, top, lo, med, hi), flush=True)
        base = ops.ctc_beam_nbest(a, il, top, beam_width=K, blank=0)
        for name, automaton in automata:
            automaton.device_arrays(dev)
            lo, m2, hi = timed(lambda: ops.ctc_beam_lm(a, il, automaton, top, beam_width=K, blank=0), args.reps, args.warmup)
            print('C = %d top_paths %d  ocr_ctc_beam_decode_lm, %-8s (%4d states) min %.1f median %.1f max %.1f us  (x %.3f)'
                  % (C, top, name, automaton.num_states, lo, m2, hi, m2 / med), flush=True)
            if name == 'zero':
                got = ops.ctc_beam_lm(a, il, automaton, top, beam_width=K, blank=0)
                same = digest(base[0], base[1], base[2], base[3]) == digest(got[0], got[1], got[2], got[4])
                print('    zero automaton: outputs %s the n-best entry\'s' % ('equal' if same else 'DIFFER FROM'), flush=True)
                ok &= same

    if args.engine:
        sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
        import make_trained_fixture as fx
        from lstm_ctc_ocr_amd.config import cfg
        from lstm_ctc_ocr_amd.engine import Engine
        from lstm_ctc_ocr_amd.models import get_network
        cfg.TRAIN.WEIGHT_DECAY = 1e-5
        eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=1, max_label_len=31)
        eng.load_arrays(fx.load_weights())
        d = np.load(fx.BATCHES)
        x, labels, ll, sl = fx.load_batch(d, 'C2')
        truth, pos = [], 0
        for n in d['C2/label_len']:
            truth.append(d['C2/labels'][pos:pos + n].tolist())
            pos += n
        Ce = int(eng.forward(x, sl).shape[2])
        t0 = time.perf_counter()
        trigram = LabelAutomaton.from_ngram(CharNGram(3, Ce).fit(truth), 0.7, 0.3)
        print('engine: C = %d, trigram of %d states compiled in %.2f s' % (Ce, trigram.num_states, time.perf_counter() - t0), flush=True)
        trigram.device_arrays(dev)
        for tag, call in (('decode_nbest_beam(k=5)', lambda: eng.decode_nbest_beam(x, sl, k=5)),
                          ('decode_nbest_beam_lm(trigram, k=5)', lambda: eng.decode_nbest_beam_lm(x, sl, trigram, k=5))):
            for _ in range(args.warmup):
                call()
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            ts.sort()
            print('engine: %-36s min %.0f median %.0f max %.0f us (host clock, T = %d)' % (tag, ts[0], ts[len(ts) // 2], ts[-1], int(eng.forward(x, sl).shape[0])),
                  flush=True)
    print('OK' if ok else 'MISMATCH', flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
