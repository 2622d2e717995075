"""CTC loss + bf16 training-form gradient at wide alphabets: the general path (ctc_loss_grad_kernel + ocr_tnc_to_ntc_bf16
over a float32 [T][N][C] scratch) against the wide path (ctc_wide_rows_kernel + ctc_wide_samples_kernel), in one process, as alternating pairs
of timed windows.  Prints every window, the range of each path per shape, and the bytes the wide path's launches move (from the shapes).
    python tools/ctc_wide_bench.py [--pairs 3] [--reps 20] [--shapes '6625,64,63,25;...']
Per-launch times: the same command under tools/prof_cmd.sh (rocprofv3 --kernel-trace --stats)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstm_ctc_ocr_amd import ops  # noqa: E402

SHAPES = [(6625, 64, 63, 25), (16384, 64, 63, 25)]          # C, N, T, max_label_len
HBM_TBS = 6.3                                                # streaming ceiling the write-up quotes bytes / time beside


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--shapes', default=None, help='C,N,T,max_label_len[;C,N,T,max_label_len...] instead of the built-in shapes')
    args = ap.parse_args()
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split(',')) for s in args.shapes.split(';')]
    dev = torch.device('cuda:0')
    for C, N, T, mll in shapes:
        rng = np.random.RandomState(C)
        acts = torch.from_numpy((rng.randn(T, N, C) * 2).astype(np.float32)).to(dev)
        flat = []
        for _ in range(N):
            lab = []
            while len(lab) < mll:
                v = int(rng.randint(1, C))
                if not lab or v != lab[-1]:
                    lab.append(v)
            flat += lab
        fl = torch.tensor(flat, dtype=torch.int32, device=dev)
        ll = torch.full((N,), mll, dtype=torch.int32, device=dev)
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        costs_g, costs_w = torch.empty(N, device=dev), torch.empty(N, device=dev)
        grad32 = torch.empty_like(acts)
        gb_g = torch.empty((N, T, C), dtype=torch.bfloat16, device=dev)
        gb_w = torch.empty_like(gb_g)
        ws_g = torch.empty(ops.ctc_workspace_bytes(mll, T, N), dtype=torch.uint8, device=dev)
        ws_w = torch.empty(ops.ctc_wide_workspace_bytes(C, mll, T, N), dtype=torch.uint8, device=dev)
        scale = 1.0 / N

        def general():
            ops.ctc_loss(acts, fl, ll, il, mll, 0, workspace=ws_g, costs=costs_g, grads=grad32)
            ops.tnc_to_ntc_bf16(grad32, gb_g, scale)

        def wide():
            ops.ctc_loss_wide(acts, fl, ll, il, mll, 0, want_grad=False, grad_ntc_bf16=gb_w, scale=scale, workspace=ws_w, costs=costs_w)

        for _ in range(3):
            general()
            wide()
        torch.cuda.synchronize()
        dc = float((costs_g - costs_w).abs().max())
        dg = float((gb_g.float() - gb_w.float()).abs().max())
        print('C=%d N=%d T=%d max_label_len=%d: costs %.1f .. %.1f, paths differ by %.3e (cost) and %.3e (bf16 gradient, largest |g| %.3e)'
              % (C, N, T, mll, float(costs_g.min()), float(costs_g.max()), dc, dg, float(gb_g.float().abs().max())), flush=True)
        tg, tw = [], []
        for p in range(args.pairs):
            tg.append(window(general, args.reps))
            tw.append(window(wide, args.reps))
            print('  pair %d: general %.1f us, wide %.1f us' % (p + 1, tg[-1], tw[-1]), flush=True)
        sp = 64 * (2 if 2 * mll + 1 <= 128 else 4 if 2 * mll + 1 <= 256 else 8)
        rows_bytes = N * T * C * (4 + 2) + N * T * sp * 4                   # logits read once, bf16 gradient written once, logy table written
        samples_bytes = N * T * sp * 4 * 5 + N * T * (2 * mll + 1) * 2      # logy read twice (recursions, fix-up); alpha, beta written and read; fix-up stores
        print('  general %.1f .. %.1f us; wide %.1f .. %.1f us; ratio of medians %.2f' % (min(tg), max(tg), min(tw), max(tw), sorted(tg)[len(tg) // 2] / sorted(tw)[len(tw) // 2]))
        print('  wide path bytes: rows launch %.1f MB (%.1f us at %.1f TB/s), samples launch %.2f MB; both launches over the wide path time: %.2f TB/s'
              % (rows_bytes / 1e6, rows_bytes / HBM_TBS / 1e6, HBM_TBS, samples_bytes / 1e6, (rows_bytes + samples_bytes) / (sorted(tw)[len(tw) // 2] * 1e-6) / 1e12), flush=True)


if __name__ == '__main__':
    main()
