"""-m gpu: the n-best beam-search entry (ctc_beam.hip: ocr_ctc_beam_decode_nbest, ops.ctc_beam_nbest) against the float64 reference of
tests/beam_nbest_cases.py with the blank at C - 1, 0 and C // 2 on the table and the wide kernel, against ocr_ctc_beam_decode bit for
bit, on TensorFlow's known-answer vector, on beams shorter than top_paths, its refusals; and Engine.decode(method='prefix'),
decode_nbest_beam and decode_spans(method='prefix') on the committed trained weights and batches.

Label sequences, lengths and counts are compared exactly (the inputs are conditioned for that: beam_nbest_cases.py), -neg_log_prob within
1e-3 * max(1, |score|) of the reference as in the other beam tests.  Every output buffer is pre-filled with a sentinel so that a slot the
kernel did not write shows.

Measured on an MI355X (the tests print every figure before they assert): worst |-neg_log_prob - score| 8.8e-4 of the tolerance over all cases;
the table and the wide kernel's neg_log_prob bits equal on all 36 (case, blank, merge) runs both cover; on the trained batches C1 and V0 prefix ==
greedy on 8 of 8 and 64 of 64 samples, |cost - Engine.score| 0 (bound 6.5e-5), exact cost - beam cost at most 2.0e-6, |logsumexp(log_post)| at most
1.4e-7."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_nbest_cases as bn  # noqa: E402
import ctc_align_cases as ac  # noqa: E402
import test_gpu_ctc_trained as tt  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

fx = tt.fx
SENTINEL = -7
PAD = -3              # not a label, not the sentinel, not the "no string" length


def score_tol(score):
    return 1e-3 * max(1.0, abs(score))


def workspace_bytes(C, N, T, K):
    sz = ctypes.c_size_t(0)
    nat.call("ocr_ctc_beam_workspace_size", C, N, T, K, ctypes.byref(sz))
    return sz.value


def nbest(dev, acts, il, K, P, blank, merge, pad=PAD):
    """ocr_ctc_beam_decode_nbest into sentinel-filled buffers -> (paths [N, P, T], lens [N, P], nlp [N, P], count [N]) as numpy."""
    T, N, C = acts.shape
    a = torch.tensor(np.array(acts), device=dev)
    l = torch.tensor(np.array(il), device=dev)
    paths = torch.full((N, P, T), SENTINEL, dtype=torch.int32, device=dev)
    lens = torch.full((N, P), SENTINEL, dtype=torch.int32, device=dev)
    nlp = torch.full((N, P), float("nan"), dtype=torch.float32, device=dev)
    count = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.empty(workspace_bytes(C, N, T, K), dtype=torch.uint8, device=dev)
    nat.call("ocr_ctc_beam_decode_nbest", a.data_ptr(), l.data_ptr(), C, N, T, K, P, blank, int(merge), pad, paths.data_ptr(), lens.data_ptr(),
             nlp.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    return paths.cpu().numpy(), lens.cpu().numpy(), nlp.cpu().numpy(), count.cpu().numpy()


def check_layout(got, pad, tag):
    """What holds for every answer: counts in range, lengths in range below count, the padding, and pad / -1 / +inf at and beyond count."""
    paths, lens, nlp, count = got
    N, P, T = paths.shape
    for n in range(N):
        assert 1 <= count[n] <= P, (tag, n, count[n])
        for r in range(P):
            if r < count[n]:
                assert 0 <= lens[n, r] <= T and np.isfinite(nlp[n, r]), (tag, n, r, lens[n, r], nlp[n, r])
                assert (paths[n, r, lens[n, r]:] == pad).all(), (tag, n, r)
            else:
                assert lens[n, r] == -1 and nlp[n, r] == np.inf and (paths[n, r] == pad).all(), (tag, n, r, lens[n, r], nlp[n, r])


def check(got, ref, scores, tag):
    paths, lens, nlp, count = got
    check_layout(got, PAD, tag)
    worst = 0.0
    for n in range(paths.shape[0]):
        assert count[n] == len(ref[n]), (tag, n, count[n], len(ref[n]))
        for r in range(count[n]):
            assert paths[n, r, :lens[n, r]].tolist() == ref[n][r], (tag, n, r, paths[n, r, :lens[n, r]].tolist(), ref[n][r])
            worst = max(worst, abs(-float(nlp[n, r]) - scores[n][r]) / score_tol(scores[n][r]))
            assert abs(-float(nlp[n, r]) - scores[n][r]) < score_tol(scores[n][r]), (tag, n, r, -nlp[n, r], scores[n][r])
    print("%s: worst |-nlp - score| / tolerance = %.3e" % (tag, worst))


@pytest.mark.parametrize("case", sorted(bn.CASES))
def test_oracle_parity(dev, case):
    """Every case with the blank at C - 1, 0 and C // 2 and merge_repeated both ways on the kernels named for it; where the table and the wide
    kernel both run, their sequences, lengths and counts are equal."""
    T, N, C, K, n = case
    try:
        for blank in bn.blanks(C):
            acts, il, ref, scores = bn.build_case(case, blank)
            for merge in (False, True):
                runs = {}
                for mode, kernel in bn.CASES[case]:
                    ops.set_beam_engine(2 if mode == "forced" else 0)
                    assert ops.ctc_beam_kernel_choice(C, K) == kernel
                    got = nbest(dev, acts, il, K, n, blank, merge)
                    check(got, ref[merge], scores, "%s %s %r blank=%d merge=%d" % (mode, kernel, case, blank, merge))
                    runs[kernel] = got
                if len(runs) == 2:
                    for a, b in zip(runs["table"][:2] + runs["table"][3:], runs["wide"][:2] + runs["wide"][3:]):
                        assert (a == b).all(), (case, blank, merge)
                    print("%r blank=%d merge=%d: table and wide neg_log_prob bits %s" % (
                        case, blank, merge, "equal" if runs["table"][2].tobytes() == runs["wide"][2].tobytes() else "differ"))
        if case in bn.HIGH_LABEL_CASES:
            assert any(v >= 256 for s in ref[False] for p in s for v in p)
    finally:
        ops.set_beam_engine(0)


def _tf_inputs(T, N, C):
    """The inputs of test_gpu_beam_wide.py's tf_case (only the inputs: the two entries are compared with each other here)."""
    rng = np.random.RandomState(T + C)
    acts = (rng.randn(T, N, C) * 3).astype(np.float32)
    acts[rng.rand(T, N) < 0.3, C - 1] += 5.0
    acts[rng.rand(T, N) < 0.3, 0] += 5.0
    il = rng.randint(max(1, T // 2), T + 1, N).astype(np.int32)
    return acts, il


@pytest.mark.parametrize("T,N,C,beam", [(12, 6, 8, 100), (20, 5, 16, 4), (63, 8, 64, 100), (30, 3, 96, 25), (7, 4, 5, 2)])
def test_top_path_with_the_last_class_as_blank_is_the_existing_entry_bit_for_bit(dev, T, N, C, beam):
    acts, il = _tf_inputs(T, N, C)
    a, l = torch.tensor(acts, device=dev), torch.tensor(il, device=dev)
    try:
        for engine in (0, 2):
            ops.set_beam_engine(engine)
            for merge in (True, False):
                out = torch.full((N, T), SENTINEL, dtype=torch.int32, device=dev)
                lens = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
                nlp = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
                ws = torch.empty(workspace_bytes(C, N, T, beam), dtype=torch.uint8, device=dev)
                nat.call("ocr_ctc_beam_decode", a.data_ptr(), l.data_ptr(), C, N, T, beam, int(merge), 0, out.data_ptr(), lens.data_ptr(),
                         nlp.data_ptr(), ws.data_ptr(), ws.numel(), nat.stream())
                torch.cuda.synchronize()
                paths, plens, pnlp, count = nbest(dev, acts, il, beam, 1, C - 1, merge, pad=0)
                tag = (T, N, C, beam, engine, merge)
                assert (count == 1).all(), tag
                assert (paths[:, 0] == out.cpu().numpy()).all() and (plens[:, 0] == lens.cpu().numpy()).all(), tag
                assert pnlp[:, 0].tobytes() == nlp.cpu().numpy().tobytes(), tag
                assert np.isfinite(pnlp).all() and (plens >= 0).all(), tag
    finally:
        ops.set_beam_engine(0)


def test_tensorflows_known_answer(dev):
    """Beam 2, top_paths 2, blank 5, no merge: [1, 0] then [0, 1, 0]; the sixth frame lies beyond seq_len."""
    logits, il = bn.tf_known_answer()
    try:
        for engine in (0, 2):
            ops.set_beam_engine(engine)
            paths, lens, nlp, count = got = nbest(dev, logits, il, 2, 2, 5, False)
            check_layout(got, PAD, "tf known answer, engine %d" % engine)
            assert count.tolist() == [2]
            assert [paths[0, r, :lens[0, r]].tolist() for r in range(2)] == bn.TF_KNOWN_PATHS, engine
            assert nlp[0, 0] < nlp[0, 1]
    finally:
        ops.set_beam_engine(0)


def test_beams_shorter_than_top_paths(dev):
    """C = 3: after one frame the beam holds the empty prefix and two labels, after none the empty prefix alone.  Frames beyond input_lengths are
    NaN: one read of them would poison the scores."""
    T, N, C, K, P = 4, 2, 3, 8, 5
    rng = np.random.RandomState(5)
    acts = np.full((T, N, C), np.nan, np.float32)
    acts[0, 0] = rng.randn(C) * 2
    il = np.array([1, 0], np.int32)
    row = acts[0, 0].astype(np.float64)
    logp = row - (row.max() + np.log(np.exp(row - row.max()).sum()))
    try:
        for engine in (0, 2):
            ops.set_beam_engine(engine)
            for blank in (2, 0, 1):
                for merge in (False, True):
                    paths, lens, nlp, count = got = nbest(dev, acts, il, K, P, blank, merge)
                    tag = (engine, blank, merge)
                    check_layout(got, PAD, tag)
                    assert count.tolist() == [3, 1], tag
                    want = sorted([(-logp[c], [] if c == blank else [c]) for c in range(C)])
                    for r, (cost, seq) in enumerate(want):
                        assert paths[0, r, :lens[0, r]].tolist() == seq, (tag, r)
                        assert abs(nlp[0, r] - cost) < score_tol(cost), (tag, r, nlp[0, r], cost)
                    assert 0 in lens[0, :3].tolist()                      # the empty prefix is one of the three
                    assert lens[1, 0] == 0 and nlp[1, 0] == 0.0, tag       # and the only one without a frame: probability 1
    finally:
        ops.set_beam_engine(0)


def test_refusals_return_invalid_and_write_nothing(dev):
    T, N = 6, 3
    lib = nat.lib()
    st = nat.stream()

    def attempt(C, K, P, blank, ws_bytes=None, null=None):
        acts = torch.zeros((T, N, C), dtype=torch.float32, device=dev)
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        width = max(1, min(P, 160))
        out = torch.full((N, width, T), SENTINEL, dtype=torch.int32, device=dev)
        lens = torch.full((N, width), SENTINEL, dtype=torch.int32, device=dev)
        nlp = torch.full((N, width), -1.0, dtype=torch.float32, device=dev)
        count = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        p = dict(acts=acts.data_ptr(), il=il.data_ptr(), out=out.data_ptr(), lens=lens.data_ptr(), nlp=nlp.data_ptr(), count=count.data_ptr(),
                 ws=ws.data_ptr())
        if null:
            p[null] = None
        rc = lib.ocr_ctc_beam_decode_nbest(p["acts"], p["il"], C, N, T, K, P, blank, 0, 0, p["out"], p["lens"], p["nlp"], p["count"], p["ws"],
                                           ws.numel() if ws_bytes is None else ws_bytes, st)
        torch.cuda.synchronize()
        tag = (C, K, P, blank, ws_bytes, null, rc)
        assert rc == 2, tag
        assert (out == SENTINEL).all() and (lens == SENTINEL).all() and (nlp == -1.0).all() and (count == SENTINEL).all(), tag

    try:
        for engine in (0, 2):
            ops.set_beam_engine(engine)
            for C, K in ((64, 100), (512, 100)):                       # table (or forced wide) and wide kernel
                assert workspace_bytes(C, N, T, K) < (1 << 20)
                attempt(C, K, 0, 0)
                attempt(C, K, K + 1, 0)
                attempt(C, 128, 129, 0)
                attempt(C, K, -1, 0)
                attempt(C, K, 5, -1)
                attempt(C, K, 5, C)
                attempt(C, K, 5, 0, ws_bytes=workspace_bytes(C, N, T, K) - 1)
                for null in ("acts", "il", "out", "lens", "nlp", "count", "ws"):
                    attempt(C, K, 5, 0, null=null)
            attempt(64, 129, 5, 0)
            attempt(16385, 128, 5, 0)
    finally:
        ops.set_beam_engine(0)


def test_ops_wrapper(dev):
    """ops.ctc_beam_nbest: blank=None is C - 1, the shapes and dtypes, and a refusal is a NativeError."""
    case = (7, 4, 5, 2, 2)
    T, N, C, K, n = case
    acts, il, ref, scores = bn.build_case(case, C - 1)
    a, l = torch.tensor(np.array(acts), device=dev), torch.tensor(np.array(il), device=dev)
    paths, lens, nlp, count = ops.ctc_beam_nbest(a, l, n, beam_width=K, pad_value=PAD)
    assert paths.shape == (N, n, T) and paths.dtype == torch.int32 and lens.shape == (N, n) and lens.dtype == torch.int32
    assert nlp.shape == (N, n) and nlp.dtype == torch.float32 and count.shape == (N,) and count.dtype == torch.int32
    check((paths.cpu().numpy(), lens.cpu().numpy(), nlp.cpu().numpy(), count.cpu().numpy()), ref[False], scores, "ops default blank")
    acts0, il0, ref0, scores0 = bn.build_case(case, 0)
    a0, l0 = torch.tensor(np.array(acts0), device=dev), torch.tensor(np.array(il0), device=dev)
    got = ops.ctc_beam_nbest(a0, l0, n, beam_width=K, blank=0, merge_repeated=True, pad_value=PAD)
    check(tuple(v.cpu().numpy() for v in got), ref0[True], scores0, "ops blank 0, merged")
    for kw in (dict(top_paths=K + 1), dict(top_paths=0), dict(top_paths=1, blank=C), dict(top_paths=1, blank=-1)):
        with pytest.raises(nat.NativeError):
            ops.ctc_beam_nbest(a, l, beam_width=K, **kw)


# ---------------------------------------------------------------------------------------------- the engine on the trained fixture
@pytest.fixture(scope='module')
def trained_engine(dev):
    from lstm_ctc_ocr_amd.config import cfg
    from lstm_ctc_ocr_amd.engine import Engine
    from lstm_ctc_ocr_amd.models import get_network
    cfg.TRAIN.WEIGHT_DECAY = 1e-5
    eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=1, max_label_len=31)
    eng.load_arrays(fx.load_weights())
    return eng


def _logsumexp(v):
    v = np.asarray(v, np.float64)
    return float(v.max() + np.log(np.exp(v - v.max()).sum()))


@pytest.mark.parametrize('name', list(ac.TRAINED_BATCHES))
def test_engine_on_trained_logits(trained_engine, name):
    eng = trained_engine
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, name)
    N = x.shape[0]
    logits = eng.forward(x, sl).cpu().numpy()
    T = logits.shape[0]
    # decode(method='prefix') is the greedy string wherever that string's best path leads by more than the bound test_gpu_ctc_align.py uses
    greedy = eng.decode(x, sl, method='greedy')
    prefix = eng.decode(x, sl, method='prefix')
    assert len(prefix) == N and all(0 not in s for s in prefix)
    compared = 0
    for n in range(N):
        if not greedy[n]:
            continue
        Tn = min(int(sl[n]), T)
        path, _, _, _, _, lyx, skip = ac.align_rows(logits[:Tn, n], greedy[n], 0, np.float64)
        if ac.margin_of(lyx, skip, path) > 2 * ac.TRAINED_PATH_BOUND:
            compared += 1
            assert prefix[n] == greedy[n], (name, n, prefix[n], greedy[n])
    print('%s: prefix == greedy on the %d of %d samples with a margin above %.3e' % (name, compared, N, 2 * ac.TRAINED_PATH_BOUND))
    assert compared > 0
    # decode_nbest_beam
    k = 5
    exact = eng.decode_nbest_beam(x, sl, k=k)
    beam = eng.decode_nbest_beam(x, sl, k=k, rescore=False)
    wide = eng.decode_nbest_beam(x, sl, k=k, candidates=100)
    assert len(exact) == len(beam) == len(wide) == N
    assert [b[0][0] for b in beam] == prefix            # the beam's own first path is decode(method='prefix')
    lexicon = sorted({tuple(e[0]) for lst in exact + wide for e in lst})
    costs = eng.score(x, sl, [list(s) for s in lexicon])[0]
    col = {s: j for j, s in enumerate(lexicon)}
    worst_cost, worst_under, worst_post = 0.0, -np.inf, 0.0
    for n in range(N):
        for lst in (exact[n], beam[n], wide[n]):
            assert 1 <= len(lst) <= k, (name, n)
            strings = [tuple(e[0]) for e in lst]
            assert len(set(strings)) == len(strings), (name, n, strings)
            assert all(0 not in s for s in strings)
            assert all(lst[j][1] >= lst[j + 1][1] for j in range(len(lst) - 1)), (name, n)          # costs ascend
        for lst in (exact[n], wide[n]):
            for labels_, log_prob, _ in lst:
                want = float(costs[n, col[tuple(labels_)]])
                worst_cost = max(worst_cost, abs(-log_prob - want))
                assert abs(-log_prob - want) <= tt.COST_BOUND, (name, n, labels_, -log_prob, want)
        # the beam sums a subset of a string's alignments: its probability is a lower bound of the exact one
        own = {tuple(e[0]): e[1] for e in beam[n]}
        assert set(own) == {tuple(e[0]) for e in exact[n]}, (name, n)
        for labels_, log_prob, _ in exact[n]:
            over = -log_prob - (-own[tuple(labels_)])
            worst_under = max(worst_under, over)
            assert over <= score_tol(own[tuple(labels_)]), (name, n, labels_, -log_prob, -own[tuple(labels_)])
        for lst in (exact[n], beam[n]):
            post = _logsumexp([e[2] for e in lst])
            worst_post = max(worst_post, abs(post))
            assert abs(post) <= 1e-5, (name, n, post)
        assert len(wide[n]) >= len(exact[n])
        for j in range(len(exact[n])):              # the j-th cheapest of a superset; both costs are float32 values within COST_BOUND of the exact ones
            assert -wide[n][j][1] <= -exact[n][j][1] + tt.COST_BOUND, (name, n, j, wide[n][j], exact[n][j])
    print('%s: |cost - Engine.score| at most %.3e (bound %.3e); exact cost - beam cost at most %.3e; |logsumexp(log_post)| at most %.3e'
          % (name, worst_cost, tt.COST_BOUND, worst_under, worst_post))
    # decode_spans(method='prefix')
    strings, spans = eng.decode_spans(x, sl, method='prefix')
    assert strings == prefix and len(spans) == N
    for n in range(N):
        Tn = min(int(sl[n]), T)
        assert [c for c, _, _, _ in spans[n]] == prefix[n], (name, n)
        assert ac.valid_alignment(prefix[n], [s for _, s, _, _ in spans[n]], [e for _, _, e, _ in spans[n]], Tn), (name, n)
        assert all(0.0 < conf <= 1.0 for _, _, _, conf in spans[n]), (name, n)
    with pytest.raises(ValueError):
        eng.decode_spans(x, sl, method='beam')
    with pytest.raises(ValueError):
        eng.decode_spans(x, sl, method='nonsense')
