"""-m gpu: the wide beam search fused with a sparse back-off automaton (ctc_beam.hip: ocr_ctc_beam_decode_lm_sparse, ops.ctc_beam_lm_sparse)
against the float64 reference of tests/beam_lm_sparse_cases.py with the blank at C - 1, 0 and C // 2: bit for bit against the wide kernel's
ocr_ctc_beam_decode_nbest under the zero automaton, against brute force at the exhaustive shapes, on pruned beams up to 6625 classes, under a
class cutoff, on re-entering beams, against the dense entry where both cover the shape, under constraints, on malformed arrays, at its edges
and refusals; and Engine.decode_lm, decode_spans_lm and decode_nbest_beam_lm with sparse automata on the committed trained weights.

Label sequences, lengths and counts are compared exactly (the inputs are conditioned for that: beam_lm_sparse_cases.py), -neg_log_prob and
lm_score within 1e-3 * max(1, |score|) of the reference as in the other beam tests.  Every output buffer is pre-filled with a sentinel so
that a slot the kernel did not write shows.  The tests print every figure before they assert."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_cases as bl  # noqa: E402
import beam_lm_sparse_cases as bs  # noqa: E402
import beam_nbest_cases as bn  # noqa: E402
import test_gpu_beam_lm as tl  # noqa: E402
import test_gpu_beam_nbest as tn  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from lstm_ctc_ocr_amd.automaton import LabelAutomaton, SparseLabelAutomaton  # noqa: E402
from lstm_ctc_ocr_amd.rescoring import BackoffNGram, CharNGram  # noqa: E402

fx = tn.fx
trained_engine = tn.trained_engine          # the module-scoped fixture of the n-best tests, instantiated for this module
SENTINEL = tn.SENTINEL
PAD = tn.PAD
NEG = bs.NEG
score_tol = tn.score_tol
check_layout = tl.check_layout
check = tl.check
strings_of = tl.strings_of


def workspace_bytes(C, N, T, K):
    sz = ctypes.c_size_t(0)
    nat.call("ocr_ctc_beam_lm_sparse_workspace_size", C, N, T, K, ctypes.byref(sz))
    return sz.value


def raw_arrays(automaton):
    return automaton.arrays() if isinstance(automaton, SparseLabelAutomaton) else automaton


def fused(dev, acts, il, automaton, K, P, blank, cutoff=None, pad=PAD):
    """ocr_ctc_beam_decode_lm_sparse into sentinel-filled buffers, the automaton a SparseLabelAutomaton or seven raw arrays that go to the entry
    as they are -> (paths [N, P, T], lens [N, P], nlp [N, P], lm [N, P], count [N]) as numpy."""
    T, N, C = acts.shape
    arrays = [torch.tensor(np.ascontiguousarray(v if v.size else np.zeros(1, v.dtype)), device=dev) for v in raw_arrays(automaton)]
    assert [v.dtype for v in arrays] == [torch.int32] * 3 + [torch.float32, torch.int32, torch.float32, torch.float32]
    H, A = int(raw_arrays(automaton)[6].shape[0]), int(raw_arrays(automaton)[1].shape[0])
    a = torch.tensor(np.array(acts), device=dev)
    l = torch.tensor(np.array(il), device=dev)
    paths = torch.full((N, P, T), SENTINEL, dtype=torch.int32, device=dev)
    lens = torch.full((N, P), SENTINEL, dtype=torch.int32, device=dev)
    nlp = torch.full((N, P), float("nan"), dtype=torch.float32, device=dev)
    lm = torch.full((N, P), float("nan"), dtype=torch.float32, device=dev)
    count = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.empty(workspace_bytes(C, N, T, K), dtype=torch.uint8, device=dev)
    nat.call("ocr_ctc_beam_decode_lm_sparse", a.data_ptr(), l.data_ptr(), C, N, T, K, K + 1 if cutoff is None else cutoff, P, blank, pad,
             *[v.data_ptr() for v in arrays], H, A, paths.data_ptr(), lens.data_ptr(), nlp.data_ptr(), lm.data_ptr(), count.data_ptr(),
             ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    return paths.cpu().numpy(), lens.cpu().numpy(), nlp.cpu().numpy(), lm.cpu().numpy(), count.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the zero automaton
@pytest.mark.parametrize("case", sorted(bn.CASES))
def test_zero_automaton_is_the_wide_nbest_entry_bit_for_bit(dev, case):
    """One state, an arc of weight 0 to itself per class, final 0, the default cutoff K + 1: decoded, lengths, count and the bits of
    neg_log_prob are ocr_ctc_beam_decode_nbest(merge_repeated=0)'s on the wide kernel, and lm_score is exactly 0."""
    T, N, C, K, n = case
    assert ops.ctc_beam_lm_sparse_supported(C, K, K + 1, 1, C - 1)
    try:
        ops.set_beam_engine(2)
        assert ops.ctc_beam_kernel_choice(C, K) == "wide"
        for blank in bn.blanks(C):
            acts, il, ref, scores = bn.build_case(case, blank)
            want = tn.nbest(dev, acts, il, K, n, blank, False)
            got = fused(dev, acts, il, bs.zero_automaton(C, blank), K, n, blank)
            check_layout(got, PAD, (case, blank))
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[4] == want[3]).all(), (case, blank)
            assert got[2].tobytes() == want[2].tobytes(), (case, blank)
            for i in range(N):
                assert (got[3][i, :got[4][i]] == 0.0).all(), (case, blank, i)
                assert strings_of(got, i) == ref[False][i], (case, blank, i)
    finally:
        ops.set_beam_engine(0)


# ---------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("kind", bs.FAIR_KINDS)
@pytest.mark.parametrize("case", bs.FAIR_CASES)
def test_pruned_beams_against_the_reference(dev, case, kind):
    T, N, C, K, n = case
    for blank in bs.blanks(C):
        acts, il, automaton, cutoff, ref = bs.build_case("fair", case, kind, blank)
        check(fused(dev, acts, il, automaton, K, n, blank), ref, "%r %s blank=%d" % (case, kind, blank))


def test_the_fused_best_string_is_not_the_acoustic_best(dev):
    """Where the reference says the automaton changes the answer at 300 classes, the fused entry returns the reference's string and the plain
    search another."""
    case = (16, 4, 300, 100, 5)
    T, N, C, K, n = case
    found = bs.fused_differs_from_acoustic(case)[:4]
    assert found
    for kind, blank, i in found:
        acts, il, automaton, cutoff, (seqs, _, _) = bs.build_case("fair", case, kind, blank)
        plain = tn.nbest(dev, acts, il, K, 1, blank, False)
        got = fused(dev, acts, il, automaton, K, 1, blank)
        mine, theirs = strings_of(got, i)[:1], [plain[0][i, 0, :plain[1][i, 0]].tolist()]
        assert mine == seqs[i][:1] and mine != theirs, (kind, blank, i, mine, theirs, seqs[i][:1])


def test_the_cutoff_is_honoured(dev):
    """cutoff 3 at 40 classes: the reference's answer under that cutoff, which is not the default cutoff's."""
    T, N, C, K, n = bs.CUTOFF_CASE
    for blank in bs.blanks(C):
        acts, il, automaton, cutoff, ref = bs.build_case("cutoff", bs.CUTOFF_CASE, bs.CUTOFF_KIND, blank)
        got = fused(dev, acts, il, automaton, K, n, blank, cutoff=cutoff)
        check(got, ref, "cutoff %d blank=%d" % (cutoff, blank))
        default = fused(dev, acts, il, automaton, K, n, blank)
        assert any(strings_of(got, i) != strings_of(default, i) for i in range(N)), blank


def test_a_prefix_that_leaves_the_beam_and_returns_keeps_its_state_and_weight(dev):
    T, N, C, K, n = bs.REENTRY_CASE
    for blank in bs.blanks(C):
        acts, il, automaton, cutoff, ref = bs.build_case("reentry", bs.REENTRY_CASE, bs.REENTRY_KIND, blank)
        check(fused(dev, acts, il, automaton, K, n, blank), ref, "re-entry blank=%d" % blank)


@pytest.mark.parametrize("kind", bs.EXHAUSTIVE_KINDS)
@pytest.mark.parametrize("case", bs.EXHAUSTIVE_CASES)
def test_exhaustive_shapes_against_brute_force(dev, case, kind):
    """The beam of 128 keeps every string the sample can emit and M = C - 1 selects nothing away: -neg_log_prob is the brute-force CTC
    log-probability plus automaton.score."""
    T, N, C, K, n = case
    worst = 0.0
    for blank in bs.blanks(C):
        acts, il, automaton, cutoff, ref = bs.build_case("exhaustive", case, kind, blank)
        got = fused(dev, acts, il, automaton, K, n, blank)
        tag = "%r %s blank=%d" % (case, kind, blank)
        check(got, ref, tag)
        paths, lens, nlp, lm, count = got
        for i in range(N):
            exact = bs.brute_force(acts[:il[i], i, :], blank)
            accepted = {s: lp for s, lp in exact.items() if automaton.accepts(s)}
            assert count[i] == len(accepted), (tag, i, count[i], len(accepted))
            for r, p in enumerate(strings_of(got, i)):
                want = accepted[tuple(p)] + automaton.score(p)
                worst = max(worst, abs(-float(nlp[i, r]) - want) / score_tol(want))
                assert abs(-float(nlp[i, r]) - want) < score_tol(want), (tag, i, r, -nlp[i, r], want)
                assert abs(float(lm[i, r]) - automaton.score(p)) < score_tol(automaton.score(p)), (tag, i, r)
    print("%r %s: worst |-nlp - (brute force + score)| %.3e of the tolerance" % (case, kind, worst))


# ---------------------------------------------------------------------------------------------- against the dense entry
@pytest.mark.parametrize("kind", bs.DENSE_KINDS)
@pytest.mark.parametrize("case", bs.DENSE_CASES)
def test_from_dense_returns_what_the_dense_entry_returns(dev, case, kind):
    T, N, C, K, n = case
    equal_bits = True
    for blank in bs.blanks(C):
        acts, il, dense, ref = bs.build_dense_case(case, kind, blank)
        want = tl.fused(dev, acts, il, dense, K, n, blank)
        got = fused(dev, acts, il, SparseLabelAutomaton.from_dense(dense), K, n, blank)
        tag = "dense %r %s blank=%d" % (case, kind, blank)
        check(got, ref, tag)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[4] == want[4]).all(), tag
        for i in range(N):
            for r in range(got[4][i]):
                assert abs(float(got[2][i, r]) - float(want[2][i, r])) < score_tol(want[2][i, r]), (tag, i, r)
                assert abs(float(got[3][i, r]) - float(want[3][i, r])) < score_tol(want[3][i, r]), (tag, i, r)
        equal_bits &= got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
    print("%r %s: the scores of the sparse and the dense entry are %s" % (case, kind, "equal to the bit" if equal_bits else "not equal to the bit"))


def test_to_dense_of_a_backoff_trigram_on_the_dense_entry(dev):
    case = (12, 4, 8, 100, 5)
    T, N, C, K, n = case
    equal_bits = True
    for blank in bs.blanks(C):
        acts, il = bl.make_inputs(case, bs.DENSE_SEEDS[(case, "trigram", blank)])
        sparse = bs.make_automaton("trigram", C, blank)
        got = fused(dev, acts, il, sparse, K, n, blank)
        want = tl.fused(dev, acts, il, sparse.to_dense(), K, n, blank)
        check_layout(got, PAD, blank)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[4] == want[4]).all(), blank
        for i in range(N):
            for r in range(got[4][i]):
                assert abs(float(got[2][i, r]) - float(want[2][i, r])) < score_tol(want[2][i, r]), (blank, i, r)
                assert abs(float(got[3][i, r]) - float(want[3][i, r])) < score_tol(want[3][i, r]), (blank, i, r)
        equal_bits &= got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
    print("to_dense: the scores of the sparse and the dense entry are %s" % ("equal to the bit" if equal_bits else "not equal to the bit"))


# ---------------------------------------------------------------------------------------------- constraints
def test_a_lexicon_automaton_at_6625_classes_returns_words_only(dev):
    T, N, C, K, n = 8, 2, 6625, 16, 4
    for blank in bs.blanks(C):
        acts, il = bs.build_case("fair", (T, N, C, K, n), "bigram", blank)[:2]
        classes = np.array([k for k in range(C) if k != blank])
        rng = np.random.RandomState(11 + blank)
        words = {tuple(int(v) for v in rng.choice(classes, rng.randint(1, 6))) for _ in range(3000)}
        for i in range(N):                          # and words the sample can emit: runs of its frames' likeliest classes
            best = [int(c) for c in np.argmax(np.delete(np.array(acts[:il[i], i]), blank, axis=1), axis=1)]
            best = [int(classes[c]) for c in best]
            words |= {tuple(bn.merge_repeats(best[:j])) for j in range(1, len(best) + 1)}
        automaton = SparseLabelAutomaton.from_lexicon([list(w) for w in sorted(words)], C, blank=blank)
        got = fused(dev, acts, il, automaton, K, n, blank)
        ref = bs.beam_search_sparse(acts, il, automaton, beam_width=K, blank=blank, top_paths=n)
        check_layout(got, PAD, blank)
        for i in range(N):
            mine = strings_of(got, i)
            assert len(mine) >= 1 and all(tuple(p) in words for p in mine), (blank, i, mine)
            assert mine[:1] == ref[0][i][:1] and len(mine) == len(ref[0][i]), (blank, i, mine, ref[0][i])
            assert (got[3][i, :len(mine)] == 0.0).all()


def test_an_automaton_that_accepts_nothing_returns_nothing(dev):
    case = (12, 4, 40, 8, 4)
    T, N, C, K, n = case
    acts, il = bs.build_case("fair", case, "bigram", 0)[:2]
    for blank in bs.blanks(C):
        zero = SparseLabelAutomaton.zero(C, blank=blank)
        none_ends = SparseLabelAutomaton(*(zero.arrays()[:6] + (np.full(1, NEG, np.float32),)), C, blank=blank)
        nothing_moves = SparseLabelAutomaton(np.zeros(3, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                             np.array([1, -1], np.int32), np.zeros(2, np.float32), np.full(2, NEG, np.float32), C, blank=blank)
        for automaton in (none_ends, nothing_moves):
            got = fused(dev, acts, il, automaton, K, n, blank)
            check_layout(got, PAD, "accepts nothing")
            assert (got[4] == 0).all()


# ---------------------------------------------------------------------------------------------- hostile arrays
def test_malformed_arrays_forbid_their_transitions_and_nothing_else(dev):
    """arc_begin inverted and beyond A, arc_next of -1, H, 1 << 30 and INT_MIN, NaN and +inf weights, a back-off cycle, a chain of 9 hops,
    unsorted labels and a NaN final go to the entry as they are (SparseLabelAutomaton refuses them): the kernel clamps, bounds-checks and caps,
    so the result is the reference's, which reads the same raw arrays."""
    T, N, C, K, n = bs.HOSTILE_CASE
    for blank in bs.blanks(C):
        acts, il, arrays, cutoff, ref = bs.build_case("hostile", bs.HOSTILE_CASE, "bigram", blank)
        with pytest.raises(ValueError):
            SparseLabelAutomaton(*arrays, C, blank=blank)
        check(fused(dev, acts, il, arrays, K, n, blank), ref, "hostile blank=%d" % blank)


# ---------------------------------------------------------------------------------------------- edges
def test_beams_shorter_than_top_paths_nan_frames_and_empty_inputs(dev):
    """C = 3: after one frame the beam holds the empty prefix and two labels, after none the empty prefix alone, whose lm_score is final[0].
    Frames beyond input_lengths are NaN: one read of them would poison the scores."""
    T, N, C, K, P = 4, 2, 3, 8, 5
    rng = np.random.RandomState(5)
    acts = np.full((T, N, C), np.nan, np.float32)
    acts[0, 0] = rng.randn(C) * 2
    il = np.array([1, 0], np.int32)
    row = acts[0, 0].astype(np.float64)
    logp = row - (row.max() + np.log(np.exp(row - row.max()).sum()))
    for blank in (2, 0, 1):
        dense = LabelAutomaton((np.arange(2 * C, dtype=np.int32).reshape(2, C) % 2), rng.randn(2, C).astype(np.float32),
                               np.array([-0.25, 0.5], np.float32), blank=blank)
        automaton = SparseLabelAutomaton.from_dense(dense)
        got = paths, lens, nlp, lm, count = fused(dev, acts, il, automaton, K, P, blank)
        check_layout(got, PAD, blank)
        assert count.tolist() == [3, 1], blank
        want = sorted([(-(logp[c] + automaton.score([] if c == blank else [c])), [] if c == blank else [c]) for c in range(C)])
        for r, (cost, seq) in enumerate(want):
            assert paths[0, r, :lens[0, r]].tolist() == seq, (blank, r)
            assert abs(nlp[0, r] - cost) < score_tol(cost), (blank, r, nlp[0, r], cost)
            assert abs(lm[0, r] - automaton.score(seq)) < score_tol(automaton.score(seq)), (blank, r)
        assert lens[1, 0] == 0 and nlp[1, 0] == 0.25 and lm[1, 0] == -0.25, blank


def test_refusals_return_invalid_and_write_nothing(dev):
    T, N = 6, 3
    lib = nat.lib()
    st = nat.stream()
    names = ("acts", "il", "begin", "label", "next", "weight", "backoff", "bweight", "final", "out", "lens", "nlp", "lm", "count", "ws")

    def attempt(C, K, P, blank, cutoff=None, H=4, A=8, ws_bytes=None, null=None):
        acts = torch.zeros((T, N, C), dtype=torch.float32, device=dev)
        il = torch.full((N,), T, dtype=torch.int32, device=dev)
        ints = [torch.zeros(16, dtype=torch.int32, device=dev) for _ in range(4)]
        floats = [torch.zeros(16, dtype=torch.float32, device=dev) for _ in range(3)]
        width = max(1, min(P, 160))
        out = torch.full((N, width, T), SENTINEL, dtype=torch.int32, device=dev)
        lens = torch.full((N, width), SENTINEL, dtype=torch.int32, device=dev)
        nlp = torch.full((N, width), -1.0, dtype=torch.float32, device=dev)
        lm = torch.full((N, width), -1.0, dtype=torch.float32, device=dev)
        count = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        tensors = (acts, il, ints[0], ints[1], ints[2], floats[0], ints[3], floats[1], floats[2], out, lens, nlp, lm, count, ws)
        p = {name: t.data_ptr() for name, t in zip(names, tensors)}
        if null:
            p[null] = None
        rc = lib.ocr_ctc_beam_decode_lm_sparse(p["acts"], p["il"], C, N, T, K, K + 1 if cutoff is None else cutoff, P, blank, 0, p["begin"],
                                               p["label"], p["next"], p["weight"], p["backoff"], p["bweight"], p["final"], H, A, p["out"],
                                               p["lens"], p["nlp"], p["lm"], p["count"], p["ws"], ws.numel() if ws_bytes is None else ws_bytes, st)
        torch.cuda.synchronize()
        tag = (C, K, P, blank, cutoff, H, A, ws_bytes, null, rc)
        assert rc == 2, tag
        assert (out == SENTINEL).all() and (lens == SENTINEL).all() and (nlp == -1.0).all() and (lm == -1.0).all() and (count == SENTINEL).all(), tag

    C, K = 64, 100
    assert workspace_bytes(C, N, T, K) < (1 << 20)
    attempt(C, K, 0, 0)
    attempt(C, K, K + 1, 0)
    attempt(C, 128, 129, 0)
    attempt(C, K, -1, 0)
    attempt(C, K, 5, -1)
    attempt(C, K, 5, C)
    attempt(C, K, 5, 0, cutoff=0)
    attempt(C, K, 5, 0, cutoff=-3)
    attempt(C, K, 5, 0, cutoff=K + 2)
    attempt(C, K, 5, 0, H=0)
    attempt(C, K, 5, 0, H=-1)
    attempt(C, K, 5, 0, H=(1 << 24) + 1)
    attempt(C, K, 5, 0, A=-1)
    attempt(C, K, 5, 0, A=(1 << 28) + 1)
    attempt(C, K, 5, 0, ws_bytes=workspace_bytes(C, N, T, K) - 1)
    for null in names:
        attempt(C, K, 5, 0, null=null)
    attempt(C, 129, 5, 0)
    attempt(C, 0, 1, 0)
    attempt(1, K, 1, 0)
    attempt(16385, 4, 1, 0)


def test_the_size_and_support_queries(dev):
    T, N = 9, 5
    for C, K in ((5, 2), (40, 100), (257, 100), (6625, 100), (16384, 128)):
        assert ops.ctc_beam_lm_sparse_supported(C, K, K + 1, 1, 0) and ops.ctc_beam_lm_sparse_supported(C, K, 1, 1 << 24, 1 << 28)
        pool = T * K + 2
        assert workspace_bytes(C, N, T, K) == (N * pool * (4 * 4 + 2) + 255) & ~255, (C, K)
    sz = ctypes.c_size_t(0)
    for args in ((16385, N, T, 100), (40, 0, T, 100), (40, N, 0, 100), (40, N, T, 129), (1, N, T, 10)):
        assert nat.lib().ocr_ctc_beam_lm_sparse_workspace_size(*args, ctypes.byref(sz)) == 2, args
    assert nat.lib().ocr_ctc_beam_lm_sparse_workspace_size(40, N, T, 100, None) == 2


def test_the_entry_runs_the_wide_kernel_whatever_the_engine_knob_says(dev):
    case, kind, blank = (12, 4, 40, 8, 4), "trigram", 20
    T, N, C, K, n = case
    acts, il, automaton, cutoff, ref = bs.build_case("fair", case, kind, blank)
    try:
        results = []
        for engine in (0, 2):
            ops.set_beam_engine(engine)
            results.append(fused(dev, acts, il, automaton, K, n, blank))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(*results))
        check(results[0], ref, "engine knob")
    finally:
        ops.set_beam_engine(0)


def test_ops_wrapper(dev):
    """ops.ctc_beam_lm_sparse: shapes and dtypes, the default and an explicit cutoff, the cached device arrays, a mismatched automaton, and a
    refusal is a NativeError."""
    T, N, C, K, n = bs.CUTOFF_CASE
    blank = 20
    acts, il, automaton, cutoff, ref_cut = bs.build_case("cutoff", bs.CUTOFF_CASE, bs.CUTOFF_KIND, blank)
    ref = bs.build_case("fair", bs.CUTOFF_CASE, bs.CUTOFF_KIND, blank)[4]
    a, l = torch.tensor(np.array(acts), device=dev), torch.tensor(np.array(il), device=dev)
    paths, lens, nlp, lm, count = got = ops.ctc_beam_lm_sparse(a, l, automaton, n, beam_width=K, blank=blank, pad_value=PAD)
    assert paths.shape == (N, n, T) and paths.dtype == torch.int32 and lens.shape == (N, n) and lens.dtype == torch.int32
    assert nlp.shape == lm.shape == (N, n) and nlp.dtype == lm.dtype == torch.float32 and count.shape == (N,) and count.dtype == torch.int32
    check(tuple(v.cpu().numpy() for v in got), ref, "ops")
    got = ops.ctc_beam_lm_sparse(a, l, automaton, n, beam_width=K, cutoff=cutoff, blank=blank, pad_value=PAD)
    check(tuple(v.cpu().numpy() for v in got), ref_cut, "ops, cutoff %d" % cutoff)
    first = automaton.device_arrays(a.device)
    assert len(first) == 7 and all(x is y for x, y in zip(first, automaton.device_arrays(a.device)))
    assert first[0].dtype == torch.int32 and first[3].dtype == torch.float32 and first[0].is_contiguous()
    with pytest.raises(ValueError):
        ops.ctc_beam_lm_sparse(a, l, bs.zero_automaton(C + 1, blank), n, beam_width=K, blank=blank)
    with pytest.raises(ValueError):                      # an automaton built for another blank
        ops.ctc_beam_lm_sparse(a, l, automaton, n, beam_width=K, blank=0)
    for kw in (dict(top_paths=K + 1, blank=blank), dict(top_paths=0, blank=blank), dict(top_paths=1, blank=blank, cutoff=0),
               dict(top_paths=1, blank=blank, cutoff=K + 2)):
        with pytest.raises(nat.NativeError):
            ops.ctc_beam_lm_sparse(a, l, automaton, beam_width=K, **kw)


# ---------------------------------------------------------------------------------------------- the engine on the trained fixture
@pytest.mark.parametrize('name', list(tn.ac.TRAINED_BATCHES))
def test_engine_with_a_sparse_automaton_on_trained_logits(trained_engine, name):
    eng = trained_engine
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, name)
    truth = tl._truth(d, name)
    C = int(eng.forward(x, sl).shape[2])
    kws = (dict(k=5), dict(k=5, rescore=False), dict(k=3, candidates=40))
    # the zero automaton changes nothing (at the default cutoff the wide search is exact)
    zero = SparseLabelAutomaton.zero(C)
    assert eng.decode_lm(x, sl, zero) == eng.decode(x, sl, method='prefix')
    assert eng.decode_spans_lm(x, sl, zero) == eng.decode_spans(x, sl, method='prefix')
    for kw in kws:
        assert eng.decode_nbest_beam_lm(x, sl, zero, **kw) == eng.decode_nbest_beam(x, sl, **kw), kw
    # the dense trigram automaton and its sparse conversion
    dense = LabelAutomaton.from_ngram(CharNGram(3, C).fit(truth), 0.7, 0.3)
    sparse = SparseLabelAutomaton.from_dense(dense)
    assert min(101, C - 1) == C - 1                      # beam 100: nothing is selected away, so the two searches are the same
    assert eng.decode_lm(x, sl, sparse) == eng.decode_lm(x, sl, dense)
    assert eng.decode_spans_lm(x, sl, sparse) == eng.decode_spans_lm(x, sl, dense)
    for kw in kws:
        mine, theirs = eng.decode_nbest_beam_lm(x, sl, sparse, **kw), eng.decode_nbest_beam_lm(x, sl, dense, **kw)
        assert [[e[0] for e in lst] for lst in mine] == [[e[0] for e in lst] for lst in theirs], kw
        for a, b in zip(mine, theirs):
            for (_, p1, q1), (_, p2, q2) in zip(a, b):
                assert abs(p1 - p2) < score_tol(p2) and abs(q1 - q2) < 1e-3, kw
    # a sparse back-off trigram fitted on the batch's labels
    model = BackoffNGram(3, C).fit(truth)
    trigram = SparseLabelAutomaton.from_backoff_ngram(model, 0.7, 0.3)
    k = 5
    lists = eng.decode_nbest_beam_lm(x, sl, trigram, k=k)
    own = eng.decode_nbest_beam_lm(x, sl, trigram, k=k, rescore=False)
    assert [lst[0][0] for lst in own] == eng.decode_lm(x, sl, trigram)
    strings, spans = eng.decode_spans_lm(x, sl, trigram)
    assert strings == eng.decode_lm(x, sl, trigram)
    lexicon = sorted({tuple(e[0]) for lst in lists for e in lst})
    costs = eng.score(x, sl, [list(s) for s in lexicon])[0]
    col = {s: j for j, s in enumerate(lexicon)}
    worst = 0.0
    for n in range(x.shape[0]):
        assert 1 <= len(lists[n]) <= k and [c for c, _, _, _ in spans[n]] == strings[n], (name, n)
        for labels_, log_prob, _ in lists[n]:
            want = -float(costs[n, col[tuple(labels_)]]) + trigram.score(labels_)
            worst = max(worst, abs(log_prob - want))
            assert abs(log_prob - want) <= tl.tt.COST_BOUND, (name, n, labels_, log_prob, want)
    print('%s: |log_prob - (-Engine.score + automaton.score)| at most %.3e (bound %.3e)' % (name, worst, tl.tt.COST_BOUND))
