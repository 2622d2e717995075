"""CTC forced alignment checked on the CPU (tests/ctc_align_cases.py): the float64 reference against brute force over every frame labelling, the
float32 model against the reference wherever the margin says the path is well defined, the float32 floors the bounds quote, the span validator,
and the cases being the edges they claim (all paths tied, a single path, a planted path, one frame, the block edges, the final slot)."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_cases as ac  # noqa: E402

sc = ac.sc


def _collapse(frames, blank):
    out, prev = [], None
    for c in frames:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def test_reference_against_brute_force():
    """Over all C^Tn frame labellings (1024 at Tn = 5): the best labelling that collapses to the string has the reference's score, and it is the
    reference's path (random logits: no two labellings tie)."""
    for name in ('brute', 'brute_last'):
        k = ac.case(name)
        ref = ac.reference(k)
        assert k.T == 5 and k.C == 4
        for n in range(k.N):
            Tn = int(k.il[n])
            rows = k.acts[:Tn, n].astype(np.float64)
            logy = rows - ac._lse(rows, 1)[:, None]
            best = {}
            for frames in itertools.product(range(k.C), repeat=Tn):
                key = tuple(_collapse(frames, k.blank))
                score = sum(logy[t, c] for t, c in enumerate(frames))
                if key not in best or score > best[key][0]:
                    best[key] = (score, frames)
            for j, label in enumerate(k.lexicon):
                if (n, j) not in ref.paths:
                    assert tuple(label) not in best and ref.cost[n, j] == np.inf, (name, n, label)
                    continue
                score, frames = best[tuple(label)]
                assert abs(ref.cost[n, j] + score) < 1e-12, (name, n, label)
                ext = ac.extended(label, k.blank)[0]
                assert tuple(ext[ref.paths[(n, j)]]) == frames, (name, n, label)


def test_model_finds_the_reference_path_where_the_margin_allows():
    """float32 and float64 give the same path on every pair whose margin exceeds 2 x PATH_BOUND; at most a tenth of the feasible pairs lie at or
    below it, and no case lies there entirely."""
    total = close = 0
    for k in ac.cases():
        ref, m32, mg = ac.reference(k), ac.align_model(k, np.float32), ac.margins(k)
        assert set(mg) == set(ref.paths) == set(m32.paths)
        kept = [p for p in mg if mg[p] > 2 * ac.PATH_BOUND]
        for p in kept:
            assert np.array_equal(m32.paths[p], ref.paths[p]), (k.name, p, mg[p])
            assert np.array_equal(m32.start[p], ref.start[p]) and np.array_equal(m32.end[p], ref.end[p]), (k.name, p)
        # infeasible pairs and the slots beyond a length: the fill
        for n in range(k.N):
            for j in range(k.K):
                L = int(k.lens[j]) if (n, j) in ref.paths else 0
                for out in (ref, m32):
                    assert np.all(out.start[n, j, L:] == -1) and np.all(out.end[n, j, L:] == -1) and np.all(out.score[n, j, L:] == -np.inf)
                    assert ((n, j) in ref.paths) == bool(np.isfinite(out.cost[n, j])) and ((n, j) in ref.paths or out.cost[n, j] == np.inf)
        print('%-10s feasible %4d, margin at or below %.3e: %3d, smallest positive margin %.3e'
              % (k.name, len(mg), 2 * ac.PATH_BOUND, len(mg) - len(kept), min([v for v in mg.values() if v > 0] or [np.inf])))
        assert not mg or kept, k.name
        total += len(mg)
        close += len(mg) - len(kept)
    print('pairs left out of the exact comparison: %d of %d (%.1f %%)' % (close, total, 100.0 * close / total))
    assert close <= 0.10 * total


def test_float32_floor_is_what_the_bounds_quote():
    worst_p = worst_s = 0.0
    for k in ac.cases():
        ep, es, same = ac.floors(k)
        print('%-10s T=%3d N=%d C=%5d K=%3d max_label_len=%3d float32 floor: path_cost %.3e, span score %.3e; float32 path = float64 path on %d of %d'
              % (k.name, k.T, k.N, k.C, k.K, k.mll, ep, es, same, len(ac.reference(k).paths)))
        qp, qs = ac.FLOORS[k.name]
        # (per case the table is a record, checked loosely from above: the small floors are single roundings of the host's expf; the two
        # constants the bounds are made of are held within a factor of two below)
        assert ep <= 4 * max(qp, 1e-5) and es <= 4 * max(qs, 1e-5), (k.name, ep, es)
        worst_p, worst_s = max(worst_p, ep), max(worst_s, es)
    print('float32 floor over the cases: path_cost %.3e, span score %.3e' % (worst_p, worst_s))
    assert ac.PATH_FLOOR / 2 <= worst_p <= ac.PATH_FLOOR * 2, (worst_p, ac.PATH_FLOOR)
    assert ac.SCORE_FLOOR / 2 <= worst_s <= ac.SCORE_FLOOR * 2, (worst_s, ac.SCORE_FLOOR)
    assert ac.PATH_BOUND == 8 * ac.PATH_FLOOR and ac.SCORE_BOUND == 8 * ac.SCORE_FLOOR
    assert sorted(ac.FLOORS) == sorted(k.name for k in ac.cases())


def test_trained_floor_is_what_the_trained_bound_quotes():
    """On the committed trained logits the float32 path of every true label is the float64 one, which is the per-frame arg-max path wherever the
    greedy decoder reads the label; the margins are far above the bound."""
    worst = 0.0
    for name in ac.TRAINED_BATCHES:
        floor, lead, differ = ac.trained_floor(name)
        print('%s: float32 floor of the path cost %.3e, smallest margin %.3e, float32 path differs on %d samples' % (name, floor, lead, differ))
        assert differ == 0 and lead > 2 * ac.TRAINED_PATH_BOUND
        worst = max(worst, floor)
        acts, truth, sl = ac.trained_truth(name)
        for n, label in enumerate(truth):
            Tn = min(int(sl[n]), acts.shape[0])
            frames = acts[:Tn, n].argmax(axis=1).tolist()
            if _collapse(frames, 0) == label:
                path = ac.align_rows(acts[:Tn, n], label, 0, np.float64)[0]
                assert ac.extended(label, 0)[0][path].tolist() == frames, (name, n)
    assert ac.TRAINED_PATH_FLOOR / 2 <= worst <= ac.TRAINED_PATH_FLOOR * 2 and ac.TRAINED_PATH_BOUND == 8 * ac.TRAINED_PATH_FLOOR


def test_valid_alignment_rejects_mutated_spans():
    label, Tn = [1, 1, 2, 3], 10
    start, end = [0, 3, 5, 8], [1, 4, 6, 9]
    assert ac.valid_alignment(label, start, end, Tn)
    assert ac.valid_alignment([], [], [], 4) and ac.valid_alignment([3], [0], [0], 1)
    bad = [
        ([0, 2, 5, 8], [1, 4, 6, 9]),          # no blank between the two equal characters
        ([0, 3, 5, 8], [1, 5, 6, 9]),          # spans overlap
        ([0, 5, 3, 8], [1, 6, 4, 9]),          # out of order
        ([0, 3, 5, 8], [1, 4, 6, 10]),         # past the input length
        ([-1, 3, 5, 8], [1, 4, 6, 9]),         # before frame 0
        ([0, 3, 5, 8], [1, 2, 6, 9]),          # a character without a frame
        ([0, 3, 5, -1], [1, 4, 6, -1]),        # a character left unset
        ([0, 3, 5], [1, 4, 6]),                # a character missing
    ]
    for st, en in bad:
        assert not ac.valid_alignment(label, st, en, Tn), (st, en)
    assert ac.valid_alignment([1, 2], [0, 1], [0, 1], 2) and not ac.valid_alignment([1, 1], [0, 1], [0, 1], 2)
    # every reference alignment is valid and path_of / spans_of are inverse to each other
    for k in ac.cases():
        ref = ac.reference(k)
        for (n, j), path in ref.paths.items():
            L, Tn = int(k.lens[j]), min(int(k.il[n]), k.T)
            assert ac.valid_alignment(k.lexicon[j][:L], ref.start[n, j, :L], ref.end[n, j, :L], Tn), (k.name, n, j)
            assert np.array_equal(ac.path_of(ref.start[n, j, :L], ref.end[n, j, :L], L, Tn), path), (k.name, n, j)


def test_flat_tight_planted():
    for dtype in (np.float64, np.float32):
        # flat: the tie rules alone decide: one frame per character from frame 0, one blank between equal neighbours
        k = ac.case('flat')
        out = ac.align_model(k, dtype)
        assert np.all(k.acts[:, 0] == k.acts[0, 0, 0]) and np.all(k.acts[:, 1] == k.acts[:, 1, :1]) and len(set(k.acts[:, 1, 0].tolist())) == k.T
        assert k.lexicon == [[1, 2, 3], [1, 1], []]
        for n in range(k.N):
            for j, label in enumerate(k.lexicon):
                st, en = ac.left_packed(label)
                assert np.array_equal(out.start[n, j, :len(label)], st) and np.array_equal(out.end[n, j, :len(label)], en), (n, j)
        assert out.start[0, 0, :3].tolist() == [0, 1, 2] and out.start[0, 1, :2].tolist() == [0, 2]
        rows = k.acts[:, 0].astype(np.float64)
        assert abs(float(out.cost[0, 2]) + (rows[:, 0] - ac._lse(rows, 1)).sum()) < 1e-5          # the empty string: minus the blank's log-probabilities
        # tight: the only alignment
        k = ac.case('tight')
        out = ac.align_model(k, dtype)
        for n, j in ac.TIGHT_PAIRS:
            label, Tn = k.lexicon[j], int(k.il[n])
            assert len(label) + ac.lc.repeats(label) == Tn and ac.margins(k)[(n, j)] == np.inf
            st, en = ac.left_packed(label)
            assert np.array_equal(out.start[n, j, :len(label)], st) and np.array_equal(out.end[n, j, :len(label)], en) and en[-1] == Tn - 1
        assert [len(k.lexicon[j]) for j in range(3)] == [3, 3, 31] and k.il.tolist() == [3, 4, 31]
        # planted: the chosen alignment comes back
        k = ac.case('planted')
        out = ac.align_model(k, dtype)
        n, j, st, en = ac.PLANTED['planted']
        spans, gaps = en - st + 1, np.concatenate([st[:1], st[1:] - en[:-1] - 1])
        assert (k.T, k.C, len(k.lexicon[0])) == (70, 40, 20) and spans.min() == 1 and spans.max() == 6 and gaps.min() == 0 and gaps.max() == 4
        assert np.array_equal(out.start[n, j], st) and np.array_equal(out.end[n, j], en)


def test_cases_are_the_intended_edges():
    by = {k.name: k for k in ac.cases()}
    assert list(by)[:len(ac.FROM_SCORE)] == list(ac.FROM_SCORE)
    assert list(by)[len(ac.FROM_SCORE):] == ['flat', 'tight', 'planted', 'T1', 'T64', 'T65', 'T128', 'T129', 'ends', 'short']
    for name in ac.FROM_SCORE:
        assert by[name] is sc.case(name)
    for k in ac.cases():
        assert ac.supported(k.C, k.T, k.mll, k.K) and ac.workspace_bytes(k.C, k.T, k.N, k.K, k.mll) <= 8 << 20, k.name
    assert {sc.slots_per_lane(by[n].mll) for n in ('lane31', 'lane32', 'lane64', 'lane128')} == {1, 2, 4, 8}
    assert by['L255'].T == 520 and by['L255'].mll == 255
    # one frame: '', one character, two characters
    t1 = ac.reference(by['T1'])
    assert by['T1'].T == 1 and by['T1'].lexicon == [[], [3], [3, 4]]
    assert np.isfinite(t1.cost).tolist() == [[True, True, False]] * 2 and t1.start[0, 1, 0] == 0 and t1.end[0, 1, 0] == 0
    # block edges: one sample at T, one a frame below, five characters
    for T in (64, 65, 128, 129):
        k = by['T%d' % T]
        assert (k.T, k.il.tolist(), k.mll) == (T, [T, T - 1], 5) and 5 in k.lens.tolist()
    # the final slot
    e, er = by['ends'], ac.reference(by['ends'])
    S = 2 * len(e.lexicon[0]) + 1
    assert er.paths[(0, 0)][-1] == S - 2 and er.paths[(1, 0)][-1] == S - 1 and ac.ENDS == {0: 2, 1: 1}
    # input lengths: 0 and below T; NaN in every frame a sample does not own, and nowhere else
    s = by['short']
    assert s.il.tolist() == [20, 13, 0, 7]
    for n, tn in enumerate(s.il):
        assert np.isnan(s.acts[tn:, n]).all() and not np.isnan(s.acts[:tn, n]).any()
    sr = ac.reference(s)
    assert not any(n == 2 for n, _ in sr.paths) and np.all(sr.cost[2] == np.inf) and not np.isnan(sr.cost).any() and not np.isnan(sr.score).any()
    # per-sample layouts are permutations
    for name in ac.PER_SAMPLE_CASES:
        k = by[name]
        lab, lens, perm = k.per_sample()
        assert lab.shape == (k.N, k.K, k.mll) and all(sorted(perm[n].tolist()) == list(range(k.K)) for n in range(k.N))
