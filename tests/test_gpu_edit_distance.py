"""-m gpu: edit distance, CER sums and MBR selection on the device (edit_distance.hip; ops.edit_distance / edit_stats / mbr_select;
Engine.evaluate / Engine.decode_mbr) against the host models of tests/edit_distance_cases.py.  Every distance, count and sum is compared as an
exact integer; the one tolerance is the fp32 bound of the MBR risks.

    self-pairing grid through ocr_edit_distance itself    4 alphabets (2, 3, 40, 16384 symbols) x 3 launches of [3, 100] x [3, 100] strings:
                                    'full'   counted lengths {0, 1, 2, 14, 15, 16, 17, 31, 63, 64, 65, 127, 128, 254, 255} and the kernel's own
                                             edges 3 and 62 (inside the 16-lane segment; the last length of one column per lane: 63 | 64 is where
                                             four columns per lane begin, 15 | 16 raw characters where a pair leaves its segment, 255 | 256 the
                                             last string | "no string"), pitch 520, class 0 sprinkled in up to 520 raw characters and ignored
                                    'short'  lengths up to 15 at pitch 15: every wave takes the four-pairs-a-wave route
                                    'mixed'  lengths up to 17 at pitch 17: waves of both routes side by side
                                    string 2m + 1 is string 2m's partner under one of 8 regimes (random, identical, one edit apart, reversed,
                                    one repeated character, disjoint alphabets, a common prefix or suffix, random with the ignored class);
                                    the 100 x 100 pairs of a sample hold every pair of lengths; dist and the counts sit between poisoned
                                    guards; symmetry, zero diagonal and |La - Lb| <= d <= max(La, Lb) are asserted on the device's output
    layouts                         [N,1]x[N,1], [N,K]x[N,1], a shared B, a pitch wider than every length with the partner's continuation behind
                                    each string, a strided view 4 bytes past a 16-byte boundary; N in {1, 3}, K in {1, 5, 100}
    "no string"                     length -1, raw length above the pitch, 256 characters counted (with and without ignored ones), on both routes
    ocr_edit_stats                  the four sums on dist with -1 entries, M up to 300 000
    ocr_mbr_select                  abc / xbd / xbe; random dist and costs at K in {1, 2, 5, 64, 100, 128}
    the engine on the trained fixture   evaluate (C1: 8 / 0 / 32, V0: 63 / 29 / 476), decode_mbr against its recomputation, decode unchanged

Measured on an MI355X (build 57e23c49bfb24a67 on commit ae26bc6; the tests print every figure before they assert):

    every distance, count and sum                  equal integers: 12 grid launches of 30 000 pairs, 6 layout cases, both "no string" routes, 7 sums
    MBR risks against the float64 model            worst |risk - risk64| / ((K + 16) 2^-23 risk64): 0.011 on abc / xbd / xbe, 0.000 / 0.000 / 0.073 /
                                                   0.043 / 0.041 / 0.037 at K = 1 / 2 / 5 / 64 / 100 / 128 (asserted: at most 1); best equals the
                                                   float64 choice on every sample
    the trained fixture                            evaluate: C1 8 / 0 / 32, V0 63 / 29 / 476 with greedy, beam and prefix alike (cer 0 and 0.06092); one
                                                   candidate holds more than half of the posterior of the 16-best list on 8 of 8 (C1) and 64 of 64 (V0)
                                                   samples and MBR departs from the top string on none; expected edits at most 0.0006 / 0.0112
    tools/edit_distance_bench.py, N = 64           100 x 100 self-pairing of C2's prefixes (9 .. 11 characters): 85.6 / 87.0 / 104.3 us min / median / max
                                                   (paths.cpu() + numpy: 16.5 s); of random 255-character strings at 6625 classes: 11.14 / 11.17 /
                                                   11.22 ms (562 s); evaluate on C2 540 us greedy, 5614 us beam (decode + accuracy_calculation 566 and
                                                   5662 us); decode_mbr(candidates=16): search 5109 us, scoring 33.8 us, distances 19.4 us, selection
                                                   17.2 us, the whole call 5776 us
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_distance_cases as ed  # noqa: E402
import test_gpu_ctc_score as gs  # noqa: E402

fx = gs.fx
pytestmark = pytest.mark.gpu
UNSET = 0x7fffffff
trained_engine = gs.trained_engine          # the module-scoped fixture of the scorer's tests, instantiated for this module
EXPECT = {'C1': (8, 0, 32), 'V0': (63, 29, 476)}          # exact / edits / ref_chars, from tests/golden/trained_expect.npz on the CPU


def _native_run(a, a_len, a_ld, a_sn, Ka, b, b_len, b_ld, b_sn, Kb, N, ignore, counts=True):
    """ocr_edit_distance itself: dist between one poisoned guard row [Ka, Kb] before and one after, the counts between poisoned guard words
    -> (dist [N, Ka, Kb], a_count, b_count flat) as numpy; asserts that the guards came back untouched."""
    from lstm_ctc_ocr_amd import _native as nat
    dev = a.device
    dist = torch.full((N + 2, Ka, Kb), UNSET, dtype=torch.int32, device=dev)
    ac = torch.full((a_len.numel() + 2,), UNSET, dtype=torch.int32, device=dev)
    bc = torch.full((b_len.numel() + 2,), UNSET, dtype=torch.int32, device=dev)
    p = nat.ptr
    nat.call('ocr_edit_distance', p(a), p(a_len), a_ld, a_sn, Ka, p(b), p(b_len), b_ld, b_sn, Kb, N, ignore, p(dist[1:]),
             p(ac[1:]) if counts else None, p(bc[1:]) if counts else None, nat.stream())
    torch.cuda.synchronize()
    dist, ac, bc = (v.cpu().numpy() for v in (dist, ac, bc))
    assert np.all(dist[0] == UNSET) and np.all(dist[N + 1] == UNSET), 'a guard row of dist written'
    assert ac[0] == ac[-1] == bc[0] == bc[-1] == UNSET, 'a guard word of the counts written'
    if not counts:
        assert np.all(ac == UNSET) and np.all(bc == UNSET)
    return dist[1:-1], ac[1:-1], bc[1:-1]


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = tuple(np.argwhere(got != want)[0])
        raise AssertionError('%s: %d of %d differ, first at %s: got %d, want %d' % (tag, int((got != want).sum()), got.size, bad, got[bad], want[bad]))


def _i32(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev)


# ------------------------------------------------------------------------------------------------ the grid
GRID = {'full': dict(pitch=520, lengths=ed.LENGTHS + ed.OWN_EDGES), 'short': dict(pitch=15, lengths=(0, 1, 2, 3, 7, 14, 15)),
        'mixed': dict(pitch=17, lengths=(0, 1, 2, 14, 15, 16, 17))}
_GRID_CACHE = {}


def _grid_case(C, kind):
    """(s, s_len, ignore, dist, count) of one launch, the host model computed once."""
    if (C, kind) not in _GRID_CACHE:
        s, s_len, ignore = ed.self_case(C, seed={'full': 0, 'short': 1, 'mixed': 2}[kind], **GRID[kind])
        _GRID_CACHE[(C, kind)] = (s, s_len, ignore) + ed.self_model(s, s_len, ignore)
    return _GRID_CACHE[(C, kind)]


@pytest.mark.parametrize('kind', list(GRID))
@pytest.mark.parametrize('C', ed.ALPHABETS)
def test_self_pairing_grid(dev, C, kind):
    from lstm_ctc_ocr_amd import ops
    s, s_len, ignore, want, want_count = _grid_case(C, kind)
    N, K, pitch = s.shape
    raw_short = (s_len <= ed.SHORT)
    print('C=%d %s: %d x %d x %d pairs, counted lengths %d .. %d, raw up to %d, %d of %d strings within a segment'
          % (C, kind, N, K, K, want_count.min(), want_count.max(), s_len.max(), int(raw_short.sum()), s_len.size))
    assert {'full': not raw_short.all() and raw_short.any(), 'short': raw_short.all(), 'mixed': not raw_short.all() and raw_short.any()}[kind]
    t, t_len = _i32(s, dev), _i32(s_len, dev)
    dist, ac, bc = _native_run(t, t_len, pitch, K * pitch, K, t, t_len, pitch, K * pitch, K, N, ignore)
    _same(ac.reshape(N, K), want_count, 'a_count')
    _same(bc.reshape(N, K), want_count, 'b_count')
    _same(dist, want, 'dist')
    # properties of the device output itself
    assert np.array_equal(dist, dist.transpose(0, 2, 1)) and np.all(dist[:, np.arange(K), np.arange(K)] == 0)
    la, lb = want_count[:, :, None], want_count[:, None, :]
    assert np.all(np.abs(la - lb) <= dist) and np.all(dist <= np.maximum(la, lb))
    # the ops entry: the same launch from the tensors' strides, and without the counts
    got = ops.edit_distance(t, t_len, t, t_len, ignore=ignore, want_counts=True)
    torch.cuda.synchronize()
    _same(got[0].cpu().numpy(), want, 'ops dist')
    _same(got[1].cpu().numpy(), want_count, 'ops a_count')
    _same(got[2].cpu().numpy(), want_count, 'ops b_count')
    if kind != 'full':
        _same(_native_run(t, t_len, pitch, K * pitch, K, t, t_len, pitch, K * pitch, K, N, ignore, counts=False)[0], want, 'dist without counts')


# ------------------------------------------------------------------------------------------------ layouts
def _strings(rng, shape, lengths, C, L):
    x = np.zeros(shape + (L,), np.int32)
    n = np.zeros(shape, np.int32)
    for at in np.ndindex(*shape):
        k = int(lengths[rng.randint(len(lengths))])
        x[at][:k] = rng.randint(1, C + 1, size=k)
        n[at] = k
    return x, n


@pytest.mark.parametrize('K', [1, 5, 100])
@pytest.mark.parametrize('N', [1, 3])
def test_layouts(dev, N, K):
    from lstm_ctc_ocr_amd import ops
    rng = np.random.RandomState(10 * N + K)
    lengths = (0, 1, 2, 5, 14, 15, 16, 17, 31, 63, 64, 65, 70) + ((255,) if K <= 5 else ())
    L, C = 256, 3
    a, a_len = _strings(rng, (N, K), lengths, C, L)
    b1, b1_len = _strings(rng, (N,), lengths, C, L)
    bs, bs_len = _strings(rng, (7,), lengths, C, L)
    A, A_len = _i32(a, dev), _i32(a_len, dev)
    # [N,1] x [N,1]: one string a sample on both sides
    got = ops.edit_distance(A[:, 0], A_len[:, 0].contiguous(), _i32(b1, dev), _i32(b1_len, dev), want_counts=True)
    want = ed.distance_model(a[:, :1], a_len[:, :1], b1[:, None], b1_len[:, None])
    _same(got[0].cpu().numpy(), want[0], '[N,1]x[N,1]')
    _same(got[1].cpu().numpy(), want[1][:, 0], '[N,1]x[N,1] a_count')
    _same(got[2].cpu().numpy(), want[2][:, 0], '[N,1]x[N,1] b_count')
    # [N,K] x [N,1]
    want = ed.distance_model(a, a_len, b1[:, None], b1_len[:, None])
    _same(ops.edit_distance(A, A_len, _i32(b1, dev), _i32(b1_len, dev)).cpu().numpy(), want[0], '[N,K]x[N,1]')
    _same(ops.edit_distance(_i32(b1, dev), _i32(b1_len, dev), A, A_len).cpu().numpy(), want[0].transpose(0, 2, 1), '[N,1]x[N,K]')
    # a shared B (b_sn = 0), by the ops entry and by the C entry between guards
    want = ed.distance_model(a, a_len, bs, bs_len, shared_b=True)
    got = ops.edit_distance(A, A_len, _i32(bs, dev), _i32(bs_len, dev), shared_b=True, want_counts=True)
    _same(got[0].cpu().numpy(), want[0], 'shared B')
    _same(got[2].cpu().numpy(), want[2], 'shared B b_count')
    nat_got = _native_run(A, A_len, L, K * L, K, _i32(bs, dev), _i32(bs_len, dev), L, 0, 7, N, -1)
    _same(nat_got[0], want[0], 'shared B, C entry')
    _same(nat_got[1].reshape(N, K), want[1], 'shared B, C entry a_count')
    _same(nat_got[2], want[2], 'shared B, C entry b_count')
    want_t = ed.distance_model(bs, bs_len, a, a_len, shared_a=True)
    _same(ops.edit_distance(_i32(bs, dev), _i32(bs_len, dev), A, A_len, shared_a=True).cpu().numpy(), want_t[0], 'shared A')
    _same(want_t[0], want[0].transpose(0, 2, 1), 'the model is symmetric')
    # a pitch wider than every length: behind each string its partner's continuation, which would make it match more if it were read
    a2, b2 = a[:, :, :80].copy(), np.zeros((N, K, 80), np.int32)
    a2_len, b2_len = np.minimum(a_len, 70), np.zeros((N, K), np.int32)
    for at in np.ndindex(N, K):
        k = int(lengths[rng.randint(len(lengths) - 1 - (K <= 5))])
        b2[at][:k] = rng.randint(1, C + 1, size=k)
        b2_len[at] = k
        la = int(a2_len[at])
        full_a, full_b = a2[at][:la].copy(), b2[at][:k].copy()
        a2[at][la:] = 0
        a2[at][la:max(la, k)] = full_b[la:k]
        b2[at][k:max(la, k)] = full_a[k:la]
    wide_a = torch.zeros((N, K, 96), dtype=torch.int32, device=dev)
    wide_a[:, :, :80] = _i32(a2, dev)
    want = ed.distance_model(a2, a2_len, b2, b2_len)
    assert np.any(want[0][:, np.arange(K), np.arange(K)] > 0)
    got = ops.edit_distance(wide_a[:, :, :80], _i32(a2_len, dev), _i32(b2, dev), _i32(b2_len, dev), want_counts=True)
    _same(got[0].cpu().numpy(), want[0], 'wide pitch')
    _same(got[1].cpu().numpy(), want[1], 'wide pitch a_count')
    # a strided view whose base is 4 bytes past a 16-byte boundary, rows 83 ints apart
    ld = 83
    buf = torch.full((1 + N * K * ld + 3,), 2, dtype=torch.int32, device=dev)
    view = buf[1:1 + N * K * ld].view(N, K, ld)[:, :, :80]
    view.copy_(_i32(a2, dev))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.stride() == (K * ld, ld, 1)
    _same(ops.edit_distance(view, _i32(a2_len, dev), _i32(b2, dev), _i32(b2_len, dev)).cpu().numpy(), want[0], 'strided view')
    _same(ops.edit_distance(_i32(b2, dev), _i32(b2_len, dev), view, _i32(a2_len, dev)).cpu().numpy(), want[0].transpose(0, 2, 1), 'strided view as B')


# ------------------------------------------------------------------------------------------------ "no string"
@pytest.mark.parametrize('route', ['short', 'long'])
def test_no_string(dev, route):
    """Each of the three rules gives -1 for exactly its own pairs, and the counts say -1 there and the counted length elsewhere."""
    from lstm_ctc_ocr_amd import ops
    rng = np.random.RandomState(3)
    N, K = 3, 9
    pitch = 12 if route == 'short' else 600
    s = rng.randint(1, 4, size=(N, K, pitch)).astype(np.int32)
    s_len = rng.randint(0, 13, size=(N, K)).astype(np.int32)
    s_len[0, 2] = -1                                                      # an empty slot of the n-best entry
    s_len[1, 0] = -5
    s_len[2, 8] = pitch + 1                                               # above the pitch
    s_len[0, 7] = 0x7fffffff
    bad = {(0, 2), (1, 0), (2, 8), (0, 7)}
    ignore = -1
    if route == 'long':
        s_len[1, 4] = 256                                                 # one character too many
        s_len[1, 5] = 255                                                 # the longest string
        s[2, 3, 1::2] = 0
        s_len[2, 3] = 513                                                 # 257 + 256 ignored: 257 counted
        s[2, 4, 1::2] = 0
        s_len[2, 4] = 510                                                 # 255 counted
        s[0, 0, :] = 0
        s_len[0, 0] = 600                                                 # nothing left: the empty string
        bad |= {(1, 4), (2, 3)}
        ignore = 0
    want, want_count = ed.self_model(s, s_len, ignore)
    for n in range(N):
        for i in range(K):
            assert (want_count[n, i] == -1) == ((n, i) in bad)
            for j in range(K):
                assert (want[n, i, j] == -1) == ((n, i) in bad or (n, j) in bad)
    if route == 'long':
        assert want_count[1, 5] == 255 and want_count[2, 4] == 255 and want_count[0, 0] == 0
    t, t_len = _i32(s, dev), _i32(s_len, dev)
    dist, ac, bc = _native_run(t, t_len, pitch, K * pitch, K, t, t_len, pitch, K * pitch, K, N, ignore)
    _same(dist, want, 'dist')
    _same(ac.reshape(N, K), want_count, 'a_count')
    _same(bc.reshape(N, K), want_count, 'b_count')
    # against one truth a sample, as the n-best paths meet their label
    ref, ref_len = s[:, 1].copy(), s_len[:, 1].copy()
    got = ops.edit_distance(t, t_len, _i32(ref, dev), _i32(ref_len, dev), ignore=None if ignore < 0 else ignore, want_counts=True)
    _same(got[0].cpu().numpy(), want[:, :, 1:2], 'against one truth')
    _same(got[2].cpu().numpy(), want_count[:, 1], 'against one truth, b_count')


# ------------------------------------------------------------------------------------------------ the sums
def test_edit_stats(dev):
    from lstm_ctc_ocr_amd import ops
    _, _, _, dist, count = _grid_case(3, 'mixed')
    d = dist.copy()
    d[0, 3, :] = -1
    d[2, :, 5] = -1
    ref = np.broadcast_to(count[:, None, :], d.shape).copy()
    cases = [('grid with -1', d, ref), ('one pair', np.array([0], np.int32), np.array([7], np.int32)),
             ('nothing counted', np.full(70, -1, np.int32), np.arange(70, dtype=np.int32))]
    rng = np.random.RandomState(8)
    for M in (1023, 1024, 1025, 300000):
        big = rng.randint(-1, 256, size=M).astype(np.int32)
        big[rng.rand(M) < 0.3] = 0
        cases.append(('M=%d' % M, big, rng.randint(0, 256, size=M).astype(np.int32)))
    for tag, dd, rr in cases:
        got = ops.edit_stats(_i32(dd, dev), _i32(rr, dev))
        torch.cuda.synchronize()
        assert got.dtype == torch.int64 and got.shape == (4,)
        want = ed.stats_model(dd, rr)
        print('%s: edits %d, ref_chars %d, exact %d, counted %d' % ((tag,) + tuple(want)))
        assert got.cpu().numpy().tolist() == want, tag


# ------------------------------------------------------------------------------------------------ MBR
def _mbr_check(dist, costs, dev, tag):
    """ocr_mbr_select against the float64 model: valid / invalid exactly, best exactly as the arg-min of the DEVICE's risk row, the risks within
    (K + 16) * 2^-23 * risk64.  -> the worst |risk - risk64| over that bound."""
    from lstm_ctc_ocr_amd import ops
    N, K = costs.shape
    risk, best, best_risk = (v.cpu().numpy() for v in ops.mbr_select(_i32(dist, dev), torch.from_numpy(costs).to(dev)))
    valid = ed.mbr_valid(dist, costs)
    risk64, best64, _ = ed.mbr_model(dist, costs)
    assert risk.dtype == np.float32 and best.dtype == np.int32 and np.all(risk[~valid] == np.inf) and np.all(np.isfinite(risk[valid]))
    _same(best, ed.mbr_pick(risk, costs, valid), tag + ': best')
    for n in range(N):
        if best[n] >= 0:
            assert best_risk[n] == risk[n, best[n]]
        else:
            assert not valid[n].any() and best_risk[n] == np.inf
    bound = (K + 16) * 2.0 ** -23 * risk64[valid]
    err = np.abs(risk[valid].astype(np.float64) - risk64[valid])
    zero = bound == 0                                                     # a risk of exactly 0: every term is 0 on both sides
    assert np.all(err[zero] == 0)
    ratio = float(np.max((err[~zero] / bound[~zero]), initial=0.0))
    print('%s: worst |risk - risk64| / ((K + 16) 2^-23 risk64) = %.3f over %d risks; best differs from the float64 choice on %d of %d samples'
          % (tag, ratio, int(valid.sum()), int((best != best64).sum()), N))
    assert ratio <= 1.0
    return ratio


def test_mbr_known_answer(dev):
    from lstm_ctc_ocr_amd import ops
    cands, dist, costs = ed.mbr_known()
    risk, best, best_risk = (v.cpu().numpy() for v in ops.mbr_select(_i32(dist, dev), torch.from_numpy(costs).to(dev)))
    print('abc / xbd / xbe: risks %s, best %d' % (risk[0].tolist(), best[0]))
    assert np.allclose(risk[0], [1.20, 1.05, 1.15], rtol=0, atol=19 * 2.0 ** -23 * 1.2) and best.tolist() == [1] and best_risk[0] == risk[0, 1]
    assert int(np.argmin(costs[0])) == 0
    _mbr_check(dist, costs, dev, 'known answer')
    # from the strings themselves: the distances on the device too
    s = _i32(np.array([cands], np.int32), dev)
    d = ops.edit_distance(s, _i32(np.full((1, 3), 3), dev), s, _i32(np.full((1, 3), 3), dev))
    _same(d.cpu().numpy(), dist, 'distances of abc / xbd / xbe')
    assert ops.mbr_select(d, torch.from_numpy(costs).to(dev))[1].cpu().numpy().tolist() == [1]


@pytest.mark.parametrize('K', [1, 2, 5, 64, 100, 128])
def test_mbr_random(dev, K):
    dist, costs = ed.mbr_random(9, K, 40 + K)
    valid = ed.mbr_valid(dist, costs)
    assert not valid[8].any() and not valid[7].any() and (K == 1 or valid[:7].any())
    _mbr_check(dist, costs, dev, 'K=%d' % K)
    # nobody valid: -1 and +inf
    from lstm_ctc_ocr_amd import ops
    _, best, best_risk = (v.cpu().numpy() for v in ops.mbr_select(_i32(dist[7:], dev), torch.from_numpy(costs[7:]).to(dev)))
    assert best.tolist() == [-1, -1] and np.all(best_risk == np.inf)


# ------------------------------------------------------------------------------------------------ the engine
def _batch(name):
    d = np.load(fx.BATCHES)
    x, labels, ll, sl = fx.load_batch(d, name)
    return x, sl, gs._truth_of(d, name)


@pytest.mark.parametrize('name', ['C1', 'V0'])
def test_engine_evaluate(trained_engine, name):
    from lstm_ctc_ocr_amd.utils.training import accuracy_calculation
    eng = trained_engine
    x, sl, truth = _batch(name)
    N = x.shape[0]
    C = eng.forward(x, sl).shape[2]
    methods = ('greedy', 'beam', 'prefix')
    before = {m: eng.decode(x, sl, method=m) for m in methods}
    before_nbest = eng.decode_nbest_beam(x, sl, k=1, candidates=16)
    rng = np.random.RandomState(91)
    edited = [gs._edits(list(t), C, rng)[int(rng.randint(3))] if n % 2 else list(t) for n, t in enumerate(truth)]
    for m in methods:
        res = eng.evaluate(x, sl, truth, method=m, per_sample=True)
        print('%s %s: exact %d, edits %d, ref_chars %d, counted %d, skipped %d, accuracy %.4f, cer %.5f'
              % (name, m, res['exact'], res['edits'], res['ref_chars'], res['counted'], res['skipped'], res['accuracy'], res['cer']))
        if m in ('greedy', 'beam'):
            assert (res['exact'], res['edits'], res['ref_chars']) == EXPECT[name]
        assert res['counted'] == N and res['skipped'] == 0
        assert res['accuracy'] == accuracy_calculation(truth, before[m], isPrint=False)
        assert res['cer'] == res['edits'] / res['ref_chars'] and res['ref_chars'] == sum(len(t) for t in truth)
        assert res['distances'].dtype == np.int32 and res['distances'].tolist() == [ed.textbook(g, t) for g, t in zip(before[m], truth)]
        assert 'distances' not in eng.evaluate(x, sl, truth, method=m)
        res = eng.evaluate(x, sl, edited, method=m, per_sample=True)
        want = [ed.textbook(g, t) for g, t in zip(before[m], edited)]
        assert res['distances'].tolist() == want and res['edits'] == sum(want) and res['exact'] == sum(v == 0 for v in want)
        assert res['ref_chars'] == sum(len(t) for t in edited)
    for m in methods:
        assert eng.decode(x, sl, method=m) == before[m]
    assert eng.decode_nbest_beam(x, sl, k=1, candidates=16) == before_nbest


@pytest.mark.parametrize('name', ['C1', 'V0'])
def test_engine_decode_mbr(trained_engine, name):
    from lstm_ctc_ocr_amd import ops
    eng = trained_engine
    x, sl, truth = _batch(name)
    N, cand = x.shape[0], 16
    before = eng.decode(x, sl, method='prefix')
    top = eng.decode_nbest_beam(x, sl, k=1, candidates=cand)
    top_of = lambda n: top[n][0][0] if top[n] else None
    got = eng.decode_mbr(x, sl, candidates=cand)
    assert len(got) == N
    # the recomputation from the same two ops
    logits = eng.forward(x, sl)
    sp_len = eng.plan(x.shape[0], x.shape[1]).seq_len
    paths, lens, _, _ = ops.ctc_beam_nbest(logits, sp_len, cand, beam_width=100, blank=0, merge_repeated=False, pad_value=0)
    width = max(min(int(paths.shape[2]), 255), 1)
    costs, _, _, log_norm = ops.ctc_score(logits, sp_len, paths[:, :, :width].contiguous(), lens, blank=0, per_sample=True)
    dist = ops.edit_distance(paths, lens, paths, lens)
    risk, best, best_risk = (v.cpu().numpy() for v in ops.mbr_select(dist, costs))
    paths, lens, costs, log_norm, dist = (v.cpu().numpy() for v in (paths, lens, costs, log_norm, dist))
    _same(dist, ed.self_model(paths, lens)[0], 'distances of the n-best paths')
    valid = ed.mbr_valid(dist, costs)
    _same(best, ed.mbr_pick(risk, costs, valid), 'best')
    risk64 = ed.mbr_model(dist, costs)[0]
    err = np.abs(risk[valid].astype(np.float64) - risk64[valid])
    assert np.all(err <= (cand + 16) * 2.0 ** -23 * risk64[valid])
    post = np.where(valid, np.exp(-costs.astype(np.float64) - log_norm[:, None].astype(np.float64)), 0.0)
    sure = [n for n in range(N) if post[n].max() > 0.5]
    moved = 0
    for n in range(N):
        if best[n] < 0:
            assert got[n] == ([], float('inf'), float('-inf'))
            continue
        b = int(best[n])
        want = ([int(v) for v in paths[n, b, :lens[n, b]]], float(best_risk[n]), float(np.float32(-costs[n, b]) - log_norm[n]))
        assert got[n] == want, (n, got[n], want)
        moved += got[n][0] != top_of(n)
    print('%s: %d of %d samples have a candidate above half of the posterior within their %d-best list; MBR departs from the top string on %d samples; '
          'expected edits %.4f .. %.4f' % (name, len(sure), N, cand, moved, min(g[1] for g in got), max(g[1] for g in got)))
    assert len(sure) >= 1
    for n in sure:
        assert got[n][0] == top_of(n), (n, got[n], top[n])
    assert eng.decode(x, sl, method='prefix') == before and eng.decode_nbest_beam(x, sl, k=1, candidates=cand) == top
