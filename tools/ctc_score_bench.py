"""Lexicon scoring (ops.ctc_score: ctc_score_rows_kernel + ctc_score_cands_kernel + ctc_score_best_kernel) against the only route the loss kernels
offer: the logits copied once per candidate of a chunk of 16, [T][N * 16][C], through ops.ctc_loss (where its one-launch kernel covers the shape) or
ops.ctc_loss_wide with want_grad=False, the chunk's time multiplied by K / 16.  The copies themselves are made once, outside the timed calls, so the
scaled figure is a lower bound of that route.  Every call sits between its own pair of events; min / median / max over the repetitions.
    python tools/ctc_score_bench.py [--reps 50] [--warmup 10] [--score-only]
Per-launch times: the same command with --score-only under tools/prof_cmd.sh (rocprofv3 --kernel-trace --stats)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstm_ctc_ocr_amd import ops  # noqa: E402

N, T, CHUNK = 64, 63, 16
SHAPES = [(40, 1024, 8, False), (6625, 1024, 8, False), (6625, 64, 24, True)]          # C, K, longest candidate, a lexicon per sample


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs)
    return us[0], us[len(us) // 2], us[-1]


def lexicon(rng, shape, C, lmax):
    """Random candidates of 1 .. lmax labels without adjacent repeats (feasible at T = 63): labels shape + (lmax,), lengths shape."""
    lens = rng.randint(1, lmax + 1, size=shape).astype(np.int32)
    lab = rng.randint(1, C, size=shape + (lmax,)).astype(np.int32)
    same = lab[..., 1:] == lab[..., :-1]
    while same.any():
        lab[..., 1:][same] = 1 + lab[..., 1:][same] % (C - 1)
        same = lab[..., 1:] == lab[..., :-1]
    return lab, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--score-only', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for C, K, lmax, per_sample in SHAPES:
        rng = np.random.RandomState(C + K)
        acts = torch.from_numpy((rng.randn(T, N, C) * 2).astype(np.float32)).to(dev)
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        lab, lens = lexicon(rng, (N, K) if per_sample else (K,), C, lmax)
        lab_d, lens_d = torch.from_numpy(lab).to(dev), torch.from_numpy(lens).to(dev)
        ws = torch.empty(ops.ctc_score_workspace_bytes(C, T, N), dtype=torch.uint8, device=dev)
        costs = torch.empty((N, K), device=dev)

        def score():
            return ops.ctc_score(acts, il, lab_d, lens_d, blank=0, per_sample=per_sample, workspace=ws, costs=costs)

        s_min, s_med, s_max = timed(score, args.reps, args.warmup)
        tag = 'C=%d N=%d T=%d K=%d%s L<=%d' % (C, N, T, K, ' per sample' if per_sample else '', lmax)
        print('%s: ctc_score min %.1f median %.1f max %.1f us' % (tag, s_min, s_med, s_max), flush=True)
        if args.score_only:
            continue
        # the first CHUNK candidates through the loss kernels: sample n * CHUNK + j of the replicated batch is (sample n, candidate j)
        rep = acts[:, :, None, :].expand(T, N, CHUNK, C).reshape(T, N * CHUNK, C).contiguous()
        clab = (lab[:, :CHUNK] if per_sample else np.broadcast_to(lab[:CHUNK], (N, CHUNK, lmax)))
        clen = (lens[:, :CHUNK] if per_sample else np.broadcast_to(lens[:CHUNK], (N, CHUNK))).reshape(-1)
        flat = np.concatenate([row[:n] for row, n in zip(clab.reshape(-1, lmax), clen)]).astype(np.int32)
        fl, ll = torch.from_numpy(flat).to(dev), torch.from_numpy(np.ascontiguousarray(clen, np.int32)).to(dev)
        il_r = torch.full((N * CHUNK,), T, dtype=torch.int32, device=dev)
        c_r = torch.empty(N * CHUNK, device=dev)
        if ops.ctc_train_supported(C, T, lmax):
            route = 'ops.ctc_loss'
            ws_r = torch.empty(ops.ctc_workspace_bytes(lmax, T, N * CHUNK), dtype=torch.uint8, device=dev)
            loss = lambda: ops.ctc_loss(rep, fl, ll, il_r, lmax, 0, want_grad=False, workspace=ws_r, costs=c_r)
        else:
            route = 'ops.ctc_loss_wide'
            ws_r = torch.empty(ops.ctc_wide_workspace_bytes(C, lmax, T, N * CHUNK), dtype=torch.uint8, device=dev)
            loss = lambda: ops.ctc_loss_wide(rep, fl, ll, il_r, lmax, 0, want_grad=False, workspace=ws_r, costs=c_r)
        l_min, l_med, l_max = timed(loss, args.reps, args.warmup)
        diff = float((c_r.view(N, CHUNK) - costs[:, :CHUNK]).abs().max())
        print('%s: %s on %d replicated candidates min %.1f median %.1f max %.1f us; x %d chunks = %.1f us median for K; ratio to ctc_score %.1f; '
              'costs of the chunk differ by at most %.3e (costs %.1f .. %.1f)'
              % (tag, route, CHUNK, l_min, l_med, l_max, K // CHUNK, l_med * K / CHUNK, l_med * K / CHUNK / s_med, diff, float(c_r.min()), float(c_r.max())),
              flush=True)
        del rep


if __name__ == '__main__':
    main()
