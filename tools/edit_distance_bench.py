"""Edit distance on the device (ops.edit_distance: edit_distance_kernel; ops.edit_stats; ops.mbr_select) at N = 64 against what a user did before
it existed: the strings copied to the host and a numpy row-vectorised table per pair there.

    self-pairing 100 x 100 of the prefixes ops.ctc_beam_nbest returns on the trained fixture's batch C2 (about 10 characters, pitch T)
    self-pairing 100 x 100 of random 255-character strings at 6625 classes
    Engine.evaluate (one forward pass, decode, one distance per sample, the four sums) against Engine.decode + accuracy_calculation
    Engine.decode_mbr(candidates=16) split into search, scoring, distances and selection

Device calls sit between their own pair of events and end in a synchronise; min / median / max over the repetitions.  The host route is timed
with the host clock, the copy included, on a share of the pairs (--host-pairs) and scaled to all of them.  The distances of those pairs are
compared with the device's.
    python tools/edit_distance_bench.py [--reps 50] [--warmup 10] [--host-pairs 2000]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctc_score_bench import timed  # noqa: E402

N = 64


def host_distance(a, b):
    """One pair on the host, a numpy row at a time: t = min(above + 1, diagonal + neq), D = j + running minimum of (t - j)."""
    j = np.arange(len(b) + 1)
    prev = j.copy()
    for i, ch in enumerate(a, 1):
        t = prev + 1
        t[1:] = np.minimum(t[1:], prev[:-1] + (b != ch))
        t[0] = i
        prev = np.minimum.accumulate(t - j) + j
    return int(prev[-1])


def host_route(paths, lens, pairs):
    """paths.cpu() + the table per pair for the first `pairs` pairs of the self-pairing -> (seconds for them, their distances)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, l = paths.cpu().numpy(), lens.cpu().numpy()
    K = p.shape[1]
    out = []
    for q in range(pairs):
        n, r = divmod(q, K * K)
        i, j = divmod(r, K)
        out.append(host_distance(p[n, i, :l[n, i]], p[n, j, :l[n, j]]) if l[n, i] >= 0 and l[n, j] >= 0 else -1)
    return time.perf_counter() - t0, np.array(out)


def self_pairing(tag, paths, lens, args):
    Nn, K, L = paths.shape
    total = Nn * K * K
    d_min, d_med, d_max = timed(lambda: ops.edit_distance(paths, lens, paths, lens), args.reps, args.warmup)
    dist = ops.edit_distance(paths, lens, paths, lens)
    torch.cuda.synchronize()
    pairs = min(args.host_pairs, total)
    secs, want = host_route(paths, lens, pairs)
    same = bool(np.array_equal(dist.cpu().numpy().reshape(-1)[:pairs], want))
    host_us = secs / pairs * total * 1e6
    ll = lens.cpu().numpy()
    print('%s: %d pairs, lengths %d .. %d (mean %.1f), pitch %d; edit_distance min %.1f median %.1f max %.1f us (%.2f ns a pair); paths.cpu() + numpy '
          '%.0f us for %d pairs = %.0f us for all (host / ours %.0f); distances %s the host\'s'
          % (tag, total, ll[ll >= 0].min(), ll.max(), ll[ll >= 0].mean(), L, d_min, d_med, d_max, d_med * 1e3 / total, secs * 1e6, pairs, host_us,
             host_us / d_med, 'equal' if same else 'DIFFER FROM'), flush=True)
    return d_med, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--host-pairs', type=int, default=2000)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    print('build %s, commit %s' % (nat.build_id(), open(os.path.join(ROOT, '.build_commit')).read().strip()
                                   if os.path.exists(os.path.join(ROOT, '.build_commit')) else 'unknown'), flush=True)
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_trained_fixture as fx
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    from lstm_ctc_ocr_amd.utils.training import accuracy_calculation
    cfg.TRAIN.WEIGHT_DECAY = 1e-5
    eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=1, max_label_len=31)
    eng.load_arrays(fx.load_weights())
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, 'C2')
    truth, pos = [], 0
    for n in d['C2/label_len']:
        truth.append(d['C2/labels'][pos:pos + n].tolist())
        pos += n
    assert x.shape[0] == N
    ok = True

    # 1. the prefixes of the search on C2, 100 x 100 per sample
    logits = eng.forward(x, sl)
    sp_len = eng.plan(x.shape[0], x.shape[1]).seq_len
    search = lambda k: ops.ctc_beam_nbest(logits, sp_len, k, beam_width=100, blank=0, merge_repeated=False, pad_value=0)
    paths, lens, _, _ = search(100)
    ok &= self_pairing('C2 prefixes, 100 x 100', paths, lens, args)[1]

    # 2. random strings of 255 characters at 6625 classes
    gen = torch.Generator(device=dev)
    gen.manual_seed(6625)
    rnd = torch.randint(1, 6625, (N, 100, 255), device=dev, generator=gen, dtype=torch.int32)
    rlen = torch.full((N, 100), 255, dtype=torch.int32, device=dev)
    ok &= self_pairing('random, 255 characters, 6625 classes, 100 x 100', rnd, rlen, args)[1]

    # 3. evaluate against decode + accuracy_calculation
    for method in ('greedy', 'beam'):
        e_min, e_med, e_max = timed(lambda: eng.evaluate(x, sl, truth, method=method), args.reps, args.warmup)
        o_min, o_med, o_max = timed(lambda: accuracy_calculation(truth, eng.decode(x, sl, method=method), isPrint=False), args.reps, args.warmup)
        res = eng.evaluate(x, sl, truth, method=method)
        acc = accuracy_calculation(truth, eng.decode(x, sl, method=method), isPrint=False)
        ok &= res['accuracy'] == acc
        print('evaluate(%s) on C2: min %.1f median %.1f max %.1f us (accuracy %.4f, cer %.5f); decode + accuracy_calculation min %.1f median %.1f '
              'max %.1f us (accuracy %.4f)' % (method, e_min, e_med, e_max, res['accuracy'], res['cer'], o_min, o_med, o_max, acc), flush=True)

    # 4. decode_mbr(candidates=16) by its parts
    cand = 16
    paths, lens, _, _ = search(cand)
    width = max(min(int(paths.shape[2]), 255), 1)
    score = lambda: ops.ctc_score(logits, sp_len, paths[:, :, :width].contiguous(), lens, blank=0, per_sample=True)
    costs = score()[0]
    dist = ops.edit_distance(paths, lens, paths, lens)
    parts = (('search', lambda: search(cand)), ('scoring', score), ('distances', lambda: ops.edit_distance(paths, lens, paths, lens)),
             ('selection', lambda: ops.mbr_select(dist, costs)), ('decode_mbr', lambda: eng.decode_mbr(x, sl, candidates=cand)))
    med = {}
    for tag, fn in parts:
        t_min, med[tag], t_max = timed(fn, args.reps, args.warmup)
        print('decode_mbr(candidates=%d) on C2, %s: min %.1f median %.1f max %.1f us' % (cand, tag, t_min, med[tag], t_max), flush=True)
    print('the distance launch is %s the search (%.1f us against %.1f us)'
          % ('below' if med['distances'] < med['search'] else 'NOT below', med['distances'], med['search']), flush=True)
    if not ok:
        sys.exit('device results differ from the host route')


if __name__ == '__main__':
    main()
