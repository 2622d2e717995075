"""The k best of a lexicon (ops.ctc_topk: ctc_topk_rows_kernel, and ctc_topk_merge_kernel where a row is cut into segments) at N = 64,
K in {1024, 65536, 1048576}, k in {1, 5, 64}, on random costs and on descending rows (every entry beats the threshold: the worst case), against
    torch.topk(costs, k, dim=1, largest=False) on the same device tensor, and
    the only route there was before: costs.cpu() and np.argpartition on the host (host clock, the copy included).
Device calls sit between their own pair of events; min / median / max over the repetitions.  The rate is the bytes of the cost matrix over the
median, as a fraction of the 6.3 TB/s a streaming kernel reaches on this chip; a matrix of up to 16 MB stays in the caches between repetitions.
The selected costs are compared with torch.topk's (values only: torch does not promise the lower index on ties).
Last, the selection beside the scoring in front of it: ops.ctc_score_trie on a dictionary of 1048576 words at C = 40, T = 63 (the dense
lexicon of tools/ctc_trie_bench.py), then ops.ctc_topk with k = 5 on its costs and log_norm.
    python tools/ctc_topk_bench.py [--reps 50] [--warmup 10] [--no-trie]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstm_ctc_ocr_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctc_score_bench import timed  # noqa: E402

N = 64
STREAM_TBS = 6.3


def host_route(costs, k, reps):
    """costs.cpu() + np.argpartition + the sort of the k kept: median wall time in us."""
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = costs.cpu().numpy()
        if k < c.shape[1]:
            part = np.argpartition(c, k - 1, axis=1)[:, :k]
        else:
            part = np.broadcast_to(np.arange(c.shape[1]), c.shape)
        vals = np.take_along_axis(c, part, axis=1)
        np.take_along_axis(part, np.argsort(vals, axis=1, kind='stable'), axis=1)
        times.append((time.perf_counter() - t0) * 1e6)
    return sorted(times)[len(times) // 2]


def point(tag, costs, k, log_norm, args):
    Nn, K = costs.shape
    ws = torch.empty(max(ops.ctc_topk_workspace_bytes(Nn, K, k), 1), dtype=torch.uint8, device=costs.device)
    o_min, o_med, o_max = timed(lambda: ops.ctc_topk(costs, k, log_norm=log_norm, workspace=ws), args.reps, args.warmup)
    kk = min(k, K)
    t_min, t_med, t_max = timed(lambda: torch.topk(costs, kk, dim=1, largest=False), args.reps, args.warmup)
    h_med = host_route(costs, kk, 3 if K > 100000 else 10)
    got = ops.ctc_topk(costs, k, log_norm=log_norm, workspace=ws)[1][:, :kk]
    want = torch.topk(costs, kk, dim=1, largest=False).values
    torch.cuda.synchronize()
    same = bool(torch.equal(got, want))
    segments, seg_len = ops.ctc_topk_plan(Nn, K, k)
    rate = Nn * K * 4 / (o_med * 1e-6) / 1e12
    print('%s k=%d: %d segment(s) of %d; ctc_topk min %.1f median %.1f max %.1f us (%.2f TB/s, %.0f%% of %.1f); torch.topk min %.1f median %.1f max %.1f us '
          '(torch / ours %.2f); costs.cpu() + np.argpartition median %.0f us (host / ours %.0f); selected costs %s torch.topk\'s'
          % (tag, k, segments, seg_len, o_min, o_med, o_max, rate, 100 * rate / STREAM_TBS, STREAM_TBS, t_min, t_med, t_max, t_med / o_med, h_med,
             h_med / o_med, 'equal' if same else 'DIFFER FROM'), flush=True)
    return o_med, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--k-entries', default='1024,65536,1048576')
    ap.add_argument('--select', default='1,5,64')
    ap.add_argument('--no-trie', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    ok = True
    for K in [int(v) for v in args.k_entries.split(',')]:
        gen = torch.Generator(device=dev)
        gen.manual_seed(K)
        random = torch.randn((N, K), device=dev, generator=gen) * 3.0 + 20.0
        descending = (torch.arange(K, 0, -1, device=dev, dtype=torch.float32) * 0.125)[None, :].repeat(N, 1) + torch.arange(N, device=dev)[:, None]
        for name, costs in (('random', random), ('descending', descending)):
            for k in [int(v) for v in args.select.split(',')]:
                ok &= point('N=%d K=%d %s' % (N, K, name), costs, k, None, args)[1]
        del random, descending
    if not args.no_trie:
        from ctc_trie_bench import lexicon
        from lstm_ctc_ocr_amd.lexicon import LexiconTrie
        C, T, K = 40, 63, 1 << 20
        rng = np.random.RandomState(C)
        acts = torch.from_numpy((rng.randn(T, N, C) * 2).astype(np.float32)).to(dev)
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        lab, lens = lexicon(np.random.RandomState(C + K + 26), K, 26)
        trie = LexiconTrie((lab, lens), C, blank=0)
        trie.device_arrays(dev)
        ws = torch.empty(ops.ctc_trie_workspace_bytes(C, T, N), dtype=torch.uint8, device=dev)
        costs = torch.empty((N, K), device=dev)
        s_min, s_med, s_max = timed(lambda: ops.ctc_score_trie(acts, il, trie, workspace=ws, costs=costs), args.reps, args.warmup)
        log_norm = ops.ctc_score_trie(acts, il, trie, workspace=ws, costs=costs)[3]
        o_med, same = point('N=%d K=%d scored costs (C=%d T=%d, %d nodes)' % (N, K, C, T, trie.num_nodes), costs, 5, log_norm, args)
        ok &= same
        print('N=%d K=%d: ctc_score_trie min %.1f median %.1f max %.1f us; ctc_topk k=5 behind it median %.1f us = %.2f%% of the scoring'
              % (N, K, s_min, s_med, s_max, o_med, 100 * o_med / s_med), flush=True)
    if not ok:
        sys.exit('selected costs differ from torch.topk')


if __name__ == '__main__':
    main()
