"""CTC forced alignment (ops.ctc_align: ctc_score_rows_kernel + ctc_align_kernel) at four shapes with N = 64:
    T = 63, C = 40, one transcript per sample (1 .. 31 characters);
    the same at C = 6625;
    T = 63, C = 6625, K = 5 strings per sample (an n-best list);
    T = 520, C = 40, one transcript of 255 characters per sample (the back-pointer words go through the workspace),
against two yardsticks:
    ops.ctc_score on the same operands, the forward-only twin of the recursion (sum instead of max, no back-pointers, no back-trace), and
    the only route there was before: acts.cpu() and a numpy float32 Viterbi on the host (host clock, the copy included).
Device calls sit between their own pair of events; min / median / max over the repetitions.  The spans are compared with the host route's
(float32 against float32 with another lse table: they may differ where two paths are within rounding of each other; the count is printed).
    python tools/ctc_align_bench.py [--reps 50] [--warmup 10] [--host-reps 1]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lstm_ctc_ocr_amd import _native, ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctc_score_bench import lexicon, timed  # noqa: E402

N = 64


def host_viterbi(rows, label, blank):
    """start, end of the best alignment of one label against rows [Tn, C] in numpy float32, the library's tie rules."""
    NEG = np.float32(-np.inf)
    ext = np.full(2 * len(label) + 1, blank, np.int64)
    ext[1::2] = label
    S = len(ext)
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    m = rows.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(rows - m).sum(axis=1, keepdims=True)))
    ly = rows[:, ext] - lse
    v = np.full(S, NEG, np.float32)
    v[:2] = ly[0, :2]
    bp = np.zeros((len(rows), S), np.int8)
    for t in range(1, len(rows)):
        x1 = np.full(S, NEG, np.float32); x1[1:] = v[:-1]
        x2 = np.full(S, NEG, np.float32); x2[2:] = np.where(skip[2:], v[:-2], NEG)
        best, step = v.copy(), bp[t]
        k = x1 > best
        best[k] = x1[k]; step[k] = 1
        k = x2 > best
        best[k] = x2[k]; step[k] = 2
        v = best + ly[t]
    s = S - 2 if S >= 2 and v[S - 2] > v[S - 1] else S - 1
    start, end = np.full(len(label), -1, np.int32), np.full(len(label), -1, np.int32)
    for t in range(len(rows) - 1, -1, -1):
        if s & 1:
            start[s >> 1] = t
            if end[s >> 1] < 0:
                end[s >> 1] = t
        if t:
            s -= int(bp[t, s])
    return start, end


def host_route(acts, lab, lens, reps):
    """acts.cpu() + the numpy Viterbi of every (sample, string): median wall time in us, and the spans."""
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = acts.cpu().numpy()
        out = [[host_viterbi(a[:, n], lab[n, j, :lens[n, j]], 0) for j in range(lab.shape[1])] for n in range(lab.shape[0])]
        times.append((time.perf_counter() - t0) * 1e6)
    return sorted(times)[len(times) // 2], out


def point(tag, T, C, K, lmax, fixed_len, args, dev):
    rng = np.random.RandomState(T + C + K)
    acts = torch.from_numpy((rng.randn(T, N, C) * 2).astype(np.float32)).to(dev)
    il = torch.full((N,), T, dtype=torch.int32, device=dev)
    lab, lens = lexicon(np.random.RandomState(T + C + K + 1), (N, K), C, lmax)
    if fixed_len:
        lens[:] = lmax
    dlab, dlens = torch.from_numpy(lab).to(dev), torch.from_numpy(lens).to(dev)
    ws = torch.empty(ops.ctc_align_workspace_bytes(C, T, N, K, lmax), dtype=torch.uint8, device=dev)
    a_min, a_med, a_max = timed(lambda: ops.ctc_align(acts, il, dlab, dlens, workspace=ws), args.reps, args.warmup)
    sws = torch.empty(ops.ctc_score_workspace_bytes(C, T, N), dtype=torch.uint8, device=dev)
    costs = torch.empty((N, K), device=dev)
    s_min, s_med, s_max = timed(lambda: ops.ctc_score(acts, il, dlab, dlens, per_sample=True, workspace=sws, costs=costs, want_best=False), args.reps,
                                args.warmup)
    start, end, score, cost = (v.cpu().numpy() for v in ops.ctc_align(acts, il, dlab, dlens, workspace=ws))
    h_med, host = host_route(acts, lab, lens, args.host_reps)
    differ = sum(1 for n in range(N) for j in range(K)
                 if not (np.array_equal(start[n, j, :lens[n, j]], host[n][j][0]) and np.array_equal(end[n, j, :lens[n, j]], host[n][j][1])))
    total = ops.ctc_score(acts, il, dlab, dlens, per_sample=True, workspace=sws, want_best=False)[0].cpu().numpy()
    print('%s: N=%d T=%d C=%d K=%d labels %d .. %d, workspace %d bytes: ctc_align min %.1f median %.1f max %.1f us; ctc_score min %.1f median %.1f max %.1f us '
          '(align / score %.2f); acts.cpu() + numpy Viterbi median %.0f us (host / ours %.0f); spans differ from the host route on %d of %d pairs; '
          'path_cost - ctc_score cost %.3f .. %.3f'
          % (tag, N, T, C, K, lens.min(), lens.max(), ws.numel(), a_min, a_med, a_max, s_min, s_med, s_max, a_med / s_med, h_med, h_med / a_med, differ,
             N * K, float((cost - total).min()), float((cost - total).max())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=1)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    try:
        commit = open(os.path.join(ROOT, '.build_commit')).read().strip()
    except OSError:
        commit = 'unknown'
    print('build id %s, built at commit %s; %s; reps %d, warm-up %d' % (_native.build_id(), commit, torch.cuda.get_device_name(0), args.reps, args.warmup),
          flush=True)
    point('one transcript per sample', 63, 40, 1, 31, False, args, dev)
    point('one transcript per sample, wide alphabet', 63, 6625, 1, 31, False, args, dev)
    point('5 strings per sample', 63, 6625, 5, 31, False, args, dev)
    point('long labels', 520, 40, 1, 255, True, args, dev)


if __name__ == '__main__':
    main()
