"""Time the wide beam search fused with a sparse back-off automaton (ocr_ctc_beam_decode_lm_sparse) at N = 64, T = 63, K = 100 on the logits
recipe of tools/beam_bench.py (randn * 3 with boosted blank and class-0 frames):

  1. with --parent <another build's libocrhip.so>: ocr_ctc_beam_decode, ocr_ctc_beam_decode_nbest and (at 40 classes) ocr_ctc_beam_decode_lm on
     that library and on this build, at 40 and 6625 classes, three alternating pairs in one process, the outputs hashed (both libraries are
     loaded side by side with ctypes; the parent lacks the new entry points, so it cannot go through _native);
  2. at 6625 classes the fused sparse search against ops.ctc_beam_nbest on the wide kernel (the baseline): the zero automaton, a back-off
     bigram and a back-off trigram, top_paths 1 and 5, at the default cutoff K + 1 and at cutoff 40;
  3. at 40 classes against the dense ops.ctc_beam_lm with the same models (through to_dense, so both search the same automaton);
  4. with --engine: Engine.decode_nbest_beam_lm(k=5) with a dense trigram and with its sparse conversion and a sparse back-off trigram on
     the trained fixture's batch C2 (host clock).

Device calls sit between their own pair of events; min / median / max over the repetitions, in microseconds.
    python tools/beam_lm_sparse_bench.py [--reps 20] [--warmup 5] [--parent PATH] [--engine]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from lstm_ctc_ocr_amd.automaton import LabelAutomaton, SparseLabelAutomaton  # noqa: E402
from lstm_ctc_ocr_amd.rescoring import BackoffNGram, CharNGram  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from beam_lm_bench import digest, logits  # noqa: E402
from ctc_score_bench import timed  # noqa: E402

T, N, K = 63, 64, 100
P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def fitted(order, C):
    """A BackoffNGram fitted on 4 * C uniform random strings of 3 .. 11 labels: at 6625 classes nearly every n-gram the search asks for is
    unseen, so nearly every lookup backs off to the empty context."""
    rng = np.random.RandomState(order)
    return BackoffNGram(order, C).fit([list(1 + rng.randint(0, C - 1, rng.randint(3, 12))) for _ in range(4 * C)])


def old_entries(path, C, dev, args):
    """(build id, name -> (min, median, max, hash)) of the existing entries on the library at `path`."""
    lib = ctypes.CDLL(path)
    lib.ocr_build_id.restype = ctypes.c_char_p
    lib.ocr_ctc_beam_workspace_size.argtypes = [I, I, I, I, ctypes.POINTER(Z)]
    lib.ocr_ctc_beam_lm_workspace_size.argtypes = [I, I, I, I, ctypes.POINTER(Z)]
    lib.ocr_ctc_beam_decode.argtypes = [P, P, I, I, I, I, I, I, P, P, P, P, Z, P]
    lib.ocr_ctc_beam_decode_nbest.argtypes = [P, P, I, I, I, I, I, I, I, I, P, P, P, P, P, Z, P]
    lib.ocr_ctc_beam_decode_lm.argtypes = [P, P, I, I, I, I, I, I, I, P, P, P, I, P, P, P, P, P, P, Z, P]
    a = logits(C, dev)
    il = torch.full((N,), T, dtype=torch.int32, device=dev)
    sz = Z(0)
    assert lib.ocr_ctc_beam_workspace_size(C, N, T, K, ctypes.byref(sz)) == 0
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    out = torch.zeros((N, 5, T), dtype=torch.int32, device=dev)
    lens = torch.zeros((N, 5), dtype=torch.int32, device=dev)
    nlp = torch.zeros((N, 5), dtype=torch.float32, device=dev)
    lm = torch.zeros((N, 5), dtype=torch.float32, device=dev)
    count = torch.zeros(N, dtype=torch.int32, device=dev)
    st = nat.stream()

    def single():
        assert lib.ocr_ctc_beam_decode(a.data_ptr(), il.data_ptr(), C, N, T, K, 1, 0, out.data_ptr(), lens.data_ptr(), nlp.data_ptr(), ws.data_ptr(),
                                       ws.numel(), st) == 0

    def nbest():
        assert lib.ocr_ctc_beam_decode_nbest(a.data_ptr(), il.data_ptr(), C, N, T, K, 5, 0, 0, 0, out.data_ptr(), lens.data_ptr(), nlp.data_ptr(),
                                             count.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    entries = [("ocr_ctc_beam_decode", single), ("ocr_ctc_beam_decode_nbest(5, blank 0)", nbest)]
    if C == 40:
        rng = np.random.RandomState(2)
        automaton = LabelAutomaton.from_ngram(CharNGram(2, C).fit([list(1 + rng.randint(0, C - 1, rng.randint(3, 12))) for _ in range(4 * C)]), 0.7, 0.3)
        tabs = automaton.device_arrays(dev)
        assert lib.ocr_ctc_beam_lm_workspace_size(C, N, T, K, ctypes.byref(sz)) == 0
        ws_lm = torch.empty(sz.value, dtype=torch.uint8, device=dev)

        def fused():
            assert lib.ocr_ctc_beam_decode_lm(a.data_ptr(), il.data_ptr(), C, N, T, K, 5, 0, 0, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                              tabs[2].data_ptr(), automaton.num_states, out.data_ptr(), lens.data_ptr(), nlp.data_ptr(),
                                              lm.data_ptr(), count.data_ptr(), ws_lm.data_ptr(), ws_lm.numel(), st) == 0
        entries.append(("ocr_ctc_beam_decode_lm(5, bigram)", fused))
    res = {}
    for name, fn in entries:
        for t in (out, lens, nlp, lm, count):
            t.zero_()
        res[name] = timed(fn, args.reps, args.warmup) + (digest(out, lens, nlp, lm, count),)
    return lib.ocr_build_id().decode(), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--engine', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    commit = os.path.join(ROOT, '.build_commit')
    print('build %s commit %s' % (nat.build_id(), open(commit).read().strip() if os.path.exists(commit) else '?'), flush=True)
    ok = True
    if args.parent:
        for C in (40, 6625):
            hashes = {}
            for pair in range(3):
                for tag, path in (('parent', args.parent), ('this build', nat.LIB_PATH)):
                    build, res = old_entries(path, C, dev, args)
                    for name, (lo, med, hi, h) in res.items():
                        print('C = %4d pair %d  %-10s %s  %-38s min %.1f median %.1f max %.1f us  hash %s' % (C, pair, tag, build, name, lo, med, hi, h),
                              flush=True)
                        hashes.setdefault(name, set()).add(h)
            for name, hs in hashes.items():
                print('C = %4d %s: outputs %s' % (C, name, 'equal in all six runs' if len(hs) == 1 else 'DIFFER'), flush=True)
                ok &= len(hs) == 1

    il = torch.full((N,), T, dtype=torch.int32, device=dev)
    for C in (6625, 40):
        a = logits(C, dev)
        t0 = time.perf_counter()
        automata = [('zero', SparseLabelAutomaton.zero(C)), ('bigram', SparseLabelAutomaton.from_backoff_ngram(fitted(2, C), 0.7, 0.3)),
                    ('trigram', SparseLabelAutomaton.from_backoff_ngram(fitted(3, C), 0.7, 0.3))]
        print('C = %d: automata built in %.1f s: %s' % (C, time.perf_counter() - t0, ', '.join(
            '%s %d states %d arcs %.2f MB' % (name, m.num_states, m.num_arcs, sum(v.nbytes for v in m.arrays()) / 1e6) for name, m in automata)), flush=True)
        dense = {name: m.to_dense() for name, m in automata} if C == 40 else {}
        try:
            ops.set_beam_engine(2)                   # the baseline is the wide kernel at both alphabets
            for top in (1, 5):
                lo, med, hi = timed(lambda: ops.ctc_beam_nbest(a, il, top, beam_width=K, blank=0), args.reps, args.warmup)
                print('C = %d top_paths %d  ocr_ctc_beam_decode_nbest (wide kernel)                        min %.1f median %.1f max %.1f us' % (C, top, lo, med, hi),
                      flush=True)
                base = ops.ctc_beam_nbest(a, il, top, beam_width=K, blank=0)
                for cutoff in (K + 1, 40):
                    for name, automaton in automata:
                        automaton.device_arrays(dev)
                        run = lambda: ops.ctc_beam_lm_sparse(a, il, automaton, top, beam_width=K, cutoff=cutoff, blank=0)      # noqa: E731
                        lo, m2, hi = timed(run, args.reps, args.warmup)
                        print('C = %d top_paths %d  ocr_ctc_beam_decode_lm_sparse cutoff %3d %-8s (%5d states) min %.1f median %.1f max %.1f us  (x %.3f)'
                              % (C, top, cutoff, name, automaton.num_states, lo, m2, hi, m2 / med), flush=True)
                        if name == 'zero' and cutoff == K + 1:
                            got = run()
                            same = digest(base[0], base[1], base[2], base[3]) == digest(got[0], got[1], got[2], got[4])
                            print('    zero automaton: outputs %s the wide n-best entry\'s' % ('equal' if same else 'DIFFER FROM'), flush=True)
                            ok &= same
                if C == 40:
                    for name, automaton in dense.items():
                        automaton.device_arrays(dev)
                        lo, m2, hi = timed(lambda: ops.ctc_beam_lm(a, il, automaton, top, beam_width=K, blank=0), args.reps, args.warmup)
                        print('C = %d top_paths %d  ocr_ctc_beam_decode_lm (dense, table kernel)   %-8s (%5d states) min %.1f median %.1f max %.1f us  (x %.3f)'
                              % (C, top, name, automaton.num_states, lo, m2, hi, m2 / med), flush=True)
                        mine = ops.ctc_beam_lm_sparse(a, il, dict(automata)[name], top, beam_width=K, blank=0)
                        theirs = ops.ctc_beam_lm(a, il, automaton, top, beam_width=K, blank=0)
                        same = digest(mine[0], mine[1], mine[4]) == digest(theirs[0], theirs[1], theirs[4])
                        print('    %s: strings, lengths and counts %s the dense entry\'s' % (name, 'equal' if same else 'DIFFER FROM'), flush=True)
                        ok &= same
        finally:
            ops.set_beam_engine(0)

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
        dense = LabelAutomaton.from_ngram(CharNGram(3, Ce).fit(truth), 0.7, 0.3)
        converted = SparseLabelAutomaton.from_dense(dense)
        backoff = SparseLabelAutomaton.from_backoff_ngram(BackoffNGram(3, Ce).fit(truth), 0.7, 0.3)
        print('engine: C = %d, dense trigram %d states (%.1f MB), converted %d arcs (%.1f MB), back-off trigram %d states %d arcs (%.3f MB)' % (
            Ce, dense.num_states, (dense.next.nbytes + dense.weight.nbytes) / 1e6, converted.num_arcs, sum(v.nbytes for v in converted.arrays()) / 1e6,
            backoff.num_states, backoff.num_arcs, sum(v.nbytes for v in backoff.arrays()) / 1e6), flush=True)
        for tag, lm in (('dense trigram', dense), ('from_dense(trigram)', converted), ('back-off trigram', backoff)):
            lm.device_arrays(dev)
            call = lambda: eng.decode_nbest_beam_lm(x, sl, lm, k=5)      # noqa: E731
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
            print('engine: decode_nbest_beam_lm(%-20s k=5) min %.0f median %.0f max %.0f us (host clock)' % (tag + ',', ts[0], ts[len(ts) // 2], ts[-1]), flush=True)
    print('OK' if ok else 'MISMATCH', flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
