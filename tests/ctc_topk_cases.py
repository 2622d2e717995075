"""The k best of a lexicon (ctc_topk.hip: ctc_topk_rows_kernel, ctc_topk_merge_kernel; ops.ctc_topk, Engine.nbest): what its CPU and GPU tests
share.  A helper module, not collected.

The result is fully determined, so there is no tolerance anywhere: every comparison is on the bits.  The order is total: cost as a float with
-0.0 == +0.0, ties to the lower index; +inf entries are never returned; NaN is outside the contract and no case holds one.

Model: np.lexsort((arange(K), row)) sorts by cost, then by index; numpy compares -0.0 and +0.0 equal and puts +inf behind every finite value.
The finite entries' first k are the answer; the selected costs are the row's own bits (signed zeros as stored), the outputs are padded with
index -1, cost +inf, log_post -inf, and log_post = (-cost) - log_norm[n] is one float32 negate and one float32 subtract.
tests/test_ctc_topk_cases.py checks the model against a plain Python sorted() and shows that it tells three wrong variants apart.

The library's host arithmetic (ocr_ctc_topk_supported / _plan / _workspace_size) is restated below."""
import numpy as np

MAX_K = 1 << 20
MAX_SEL = 64
MAX_N = 65535
ROUND = 4096            # entries of a workgroup's round: 256 threads x 16
ONE_WG = 2 * ROUND      # rows up to here are one segment whatever N
TARGET_WGS = 1024

F32_INF = np.float32(np.inf)


def supported(K, k):
    return 1 <= K <= MAX_K and 1 <= k <= MAX_SEL


def _ceil_div(a, b):
    return (a + b - 1) // b


def plan(N, K, k):
    """(segments, segment_len), or None where the arguments are refused."""
    if not (1 <= N <= MAX_N) or not supported(K, k):
        return None
    want = 1
    if K > ONE_WG:
        want = min(_ceil_div(K, ROUND), _ceil_div(TARGET_WGS, N))
    seg_len = _ceil_div(_ceil_div(K, want), ROUND) * ROUND
    return _ceil_div(K, seg_len), seg_len


def workspace_bytes(N, K, k):
    """A 64-bit key per (sample, segment, slot), rounded up to 256 bytes; 0 for a one-segment plan; None where the arguments are refused."""
    p = plan(N, K, k)
    if p is None:
        return None
    return (N * p[0] * k * 8 + 255) // 256 * 256 if p[0] > 1 else 0


# ---------------------------------------------------------------- model
def topk_model(costs, k, log_norm=None):
    """index [N, k] int32, cost [N, k] float32, log_post [N, k] float32 (None without log_norm), count [N] int32 of a float32 [N, K] matrix."""
    costs = np.asarray(costs)
    assert costs.dtype == np.float32 and costs.ndim == 2 and not np.isnan(costs).any()
    N, K = costs.shape
    index = np.full((N, k), -1, np.int32)
    cost = np.full((N, k), np.inf, np.float32)
    count = np.zeros(N, np.int32)
    post = None if log_norm is None else np.full((N, k), -np.inf, np.float32)
    for n in range(N):
        row = costs[n]
        order = np.lexsort((np.arange(K), row))
        order = order[row[order] != F32_INF][:k]
        m = len(order)
        index[n, :m] = order
        cost[n, :m] = row[order]
        count[n] = m
        if post is not None:
            with np.errstate(invalid='ignore', over='ignore'):
                post[n, :m] = (-row[order]).astype(np.float32) - np.float32(log_norm[n])
    return index, cost, post, count


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------- cases
REGIMES = ('normal', 'ties8', 'equal', 'ascending', 'descending', 'all_inf', 'finite_k-1', 'finite_k', 'finite_k+1', 'last_only', 'zeros')
SMALL_K = (1, 2, 63, 64, 65, 255, 256, 257)
SELECT = (1, 2, 5, 63, 64)
BATCH = (1, 3)


def plan_sizes(N, k):
    """Row lengths taken from the plan itself: around the length of a segment where the chip is cut finest (K = 2^20), two segments and one entry,
    and the sizes at which a row stops being one segment."""
    seg_len = plan(N, MAX_K, k)[1]
    return sorted({seg_len - 1, seg_len, seg_len + 1, 2 * seg_len + 1, ONE_WG - 1, ONE_WG, ONE_WG + 1})


def row_lengths(N, k):
    return list(SMALL_K) + plan_sizes(N, k)


def make_rows(regime, N, K, k, seed):
    """float32 [N, K] of a regime, the same for the CPU and the GPU tests."""
    rng = np.random.RandomState(seed)
    if regime == 'normal':
        c = rng.randn(N, K) * 3.0
    elif regime == 'ties8':
        c = rng.randint(0, 8, size=(N, K)) * 0.5 - 1.5
    elif regime == 'equal':
        c = np.full((N, K), 2.25)
    elif regime == 'ascending':
        c = np.arange(K)[None, :] * 0.125 - 7.0 + np.arange(N)[:, None]
    elif regime == 'descending':
        c = -np.arange(K)[None, :] * 0.125 + 7.0 + np.arange(N)[:, None]
    elif regime == 'all_inf':
        c = np.full((N, K), np.inf)
    elif regime in ('finite_k-1', 'finite_k', 'finite_k+1'):
        want = k + {'finite_k-1': -1, 'finite_k': 0, 'finite_k+1': 1}[regime]
        c = np.full((N, K), np.inf)
        for n in range(N):
            at = rng.permutation(K)[:min(max(want, 0), K)]
            c[n, at] = rng.randn(len(at)) * 3.0
    elif regime == 'last_only':
        c = np.full((N, K), np.inf)
        c[:, K - 1] = 1.5 - np.arange(N)
    elif regime == 'zeros':
        # the winners are zeros of both signs (at most k + 2 of them, alternating in index order) below positive costs
        c = np.abs(rng.randn(N, K)) + 0.5
        for n in range(N):
            at = np.sort(rng.permutation(K)[:min(k + 2, K)])
            c[n, at[0::2]] = -0.0
            c[n, at[1::2]] = 0.0
    else:
        raise KeyError(regime)
    c = np.ascontiguousarray(c, np.float32)
    assert c.shape == (N, K) and not np.isnan(c).any()
    return c


def segment_edge_rows(N=2, K=MAX_K, k=64, seed=900):
    """Random costs above zero with k winners planted, alternating, at the last index of a segment and the first of the next; half of them
    (every other one) share one value, the others are distinct and lower than everything else."""
    segments, seg_len = plan(N, K, k)
    assert segments >= k // 2 + 1
    rng = np.random.RandomState(seed)
    c = (np.abs(rng.randn(N, K)) + 1.0).astype(np.float32)
    for n in range(N):
        edges = 1 + rng.permutation(segments - 1)[:k // 2]                 # segment boundaries s | s + 1
        at = np.sort(np.concatenate([edges * seg_len - 1, edges * seg_len]))
        vals = -1.0 - rng.rand(k).astype(np.float32)
        vals[0::2] = np.float32(-1.25)
        c[n, at] = vals[rng.permutation(k)]
    return c
