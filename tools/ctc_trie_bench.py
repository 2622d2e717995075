"""Lexicon scoring on a prefix tree (ops.ctc_score_trie: rows launch + ctc_trie_kernel + arg-min launch) against the per-candidate route
(ops.ctc_score) on the same lexicon, at N = 64, T = 63, C in {40, 6625}, words of 2 .. 12 labels drawn once over 26 symbols (dense sharing of
prefixes) and once over all classes (sparse).  K in {1024, 16384, 65536}: both routes; K = 1048576: the tree alone (the per-candidate route
stops at 65536).  Every call sits between its own pair of events; min / median / max over the repetitions.  The builder's host time
(LexiconTrie from the dense arrays: size queries and fill) is taken once per lexicon.
    python tools/ctc_trie_bench.py [--reps 60] [--warmup 10] [--chunk-nodes default,256,1024,4096,8192] [--k 1024,16384,65536,1048576]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstm_ctc_ocr_amd import ops  # noqa: E402
from lstm_ctc_ocr_amd.lexicon import LexiconTrie  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctc_score_bench import timed  # noqa: E402

N, T, LMIN, LMAX = 64, 63, 2, 12
LIST_MAX_K = 65536


def lexicon(rng, K, symbols):
    """K words of LMIN .. LMAX labels over the classes 1 .. symbols: dense int32 [K, LMAX] (zeros beyond a word's length) and lengths."""
    lens = rng.randint(LMIN, LMAX + 1, size=K).astype(np.int32)
    lab = rng.randint(1, symbols + 1, size=(K, LMAX)).astype(np.int32)
    lab[np.arange(LMAX)[None, :] >= lens[:, None]] = 0
    return lab, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--chunk-nodes', default='default')
    ap.add_argument('--k', default='1024,16384,65536,1048576')
    ap.add_argument('--classes', default='40,6625')
    args = ap.parse_args()
    chunk_list = [None if c == 'default' else int(c) for c in args.chunk_nodes.split(',')]
    dev = torch.device('cuda:0')
    for C in [int(c) for c in args.classes.split(',')]:
        rng = np.random.RandomState(C)
        acts = torch.from_numpy((rng.randn(T, N, C) * 2).astype(np.float32)).to(dev)
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.ctc_trie_workspace_bytes(C, T, N), dtype=torch.uint8, device=dev)
        for sharing, symbols in (('dense', min(26, C - 1)), ('sparse', C - 1)):
            for K in [int(k) for k in args.k.split(',')]:
                lab, lens = lexicon(np.random.RandomState(C + K + symbols), K, symbols)
                costs = torch.empty((N, K), device=dev)
                tag = 'C=%d N=%d T=%d K=%d %s (%d symbols)' % (C, N, T, K, sharing, symbols)
                s_med = None
                if K <= LIST_MAX_K:
                    lab_d, lens_d = torch.from_numpy(lab).to(dev), torch.from_numpy(lens).to(dev)
                    ref = torch.empty((N, K), device=dev)
                    s_min, s_med, s_max = timed(lambda: ops.ctc_score(acts, il, lab_d, lens_d, blank=0, workspace=ws, costs=ref), args.reps, args.warmup)
                    print('%s: ctc_score min %.1f median %.1f max %.1f us (%d slots)' % (tag, s_min, s_med, s_max, int((2 * lens + 1).sum())), flush=True)
                for chunk in chunk_list:
                    t0 = time.perf_counter()
                    trie = LexiconTrie((lab, lens), C, blank=0, chunk_nodes=chunk)
                    host = time.perf_counter() - t0
                    trie.device_arrays(dev)
                    t_min, t_med, t_max = timed(lambda: ops.ctc_score_trie(acts, il, trie, workspace=ws, costs=costs), args.reps, args.warmup)
                    line = '%s: tree, chunks of %d%s: %d nodes in %d chunks, built in %.1f ms on the host; ctc_score_trie min %.1f median %.1f max %.1f us' \
                        % (tag, trie.chunk_nodes, ' (default)' if chunk is None else '', trie.num_nodes, trie.num_chunks, host * 1e3, t_min, t_med, t_max)
                    if s_med is not None:
                        diff = float((costs - ref).abs().max())
                        line += '; ctc_score / tree %.2f; costs differ by at most %.3e, bits %s' % (s_med / t_med, diff, 'agree' if torch.equal(
                            costs.view(torch.int32), ref.view(torch.int32)) else 'differ')
                    print(line, flush=True)
                    del trie


if __name__ == '__main__':
    main()
