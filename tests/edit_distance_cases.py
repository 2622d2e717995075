"""Host models and cases of the device edit distance (csrc/edit_distance.hip), shared by tests/test_edit_distance_cases.py (CPU) and
tests/test_gpu_edit_distance.py (-m gpu):

    textbook(a, b)            the Wagner-Fischer table in plain Python, the definition
    lane_model(...)           ed_rows of the kernel lane by lane: columns on lanes, the shift by one, the prefix-min scan in its doubling steps
                              with the kernel's fills, rows beyond La masked, columns beyond Lb computing values nobody reads
    pairs_model(A, B)         the same recursion (t = min(above + 1, diagonal + neq), D = j + prefix-min(t - j)) vectorised over many pairs
                              in numpy: what the GPU tests compare against; checked against textbook() on the CPU
    string_of / distance_model / stats_model / mbr_model    the entry points' contracts: `ignore`, the three "no string" rules, the strides,
                              the four sums, the MBR selection in float64 on the float32 costs
"""
import numpy as np

MAX_LEN = 255            # counted characters of a string
SHORT = 15               # raw length up to which a pair takes a 16-lane segment
MAX_PAIRS = 1 << 30
MBR_MAX_K = 128
FAR = 1 << 20

# the issue's lengths, and the edges of the kernel's instances: 15 | 16 raw characters (segment or whole wave), 63 | 64 counted characters of B
# (one column per lane or four), 255 | 256 (the last string | "no string"); 3 and 62 put a length strictly inside each instance
LENGTHS = (0, 1, 2, 14, 15, 16, 17, 31, 63, 64, 65, 127, 128, 254, 255)
OWN_EDGES = (3, 62)
ALPHABETS = (2, 3, 40, 16384)
REGIMES = ('random', 'identical', 'one_edit', 'reversed', 'repeated', 'disjoint', 'common_ends', 'ignore')


def textbook(a, b):
    """Levenshtein distance, unit costs: the full table."""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D[len(a)][len(b)]


# ---------------------------------------------------------------- the kernel's table, lane by lane
def _shr(v, d, fill, W):
    """Lane sl of every W-lane segment takes v of lane sl - d, `fill` where there is none."""
    out = np.full_like(v, fill)
    for base in range(0, len(v), W):
        out[base + d:base + W] = v[base:base + W - d]
    return out


def lane_model(pairs, CPL, W):
    """ed_rows<CPL, W> on 64 lanes: pairs = 64 // W (a, b) pairs, one per segment, len(b) <= W * CPL - 1.  -> their distances."""
    assert len(pairs) == 64 // W and all(len(b) <= W * CPL - 1 for _, b in pairs)
    sl = np.arange(64) % W
    seg = np.arange(64) // W
    La = np.array([len(pairs[s][0]) for s in seg])
    rows = max(len(a) for a, _ in pairs)
    col = [sl * CPL + c for c in range(CPL)]
    bch = [np.array([pairs[seg[l]][1][col[c][l] - 1] if 1 <= col[c][l] <= len(pairs[seg[l]][1]) else -1 for l in range(64)]) for c in range(CPL)]
    prev = [col[c].copy() for c in range(CPL)]
    for i in range(1, rows + 1):
        ai = np.array([pairs[s][0][i - 1] if i <= len(pairs[s][0]) else -7 for s in seg])            # (beyond La: whatever the LDS holds)
        left = _shr(prev[CPL - 1], 1, 0, W)
        u = []
        for c in range(CPL):
            diag = prev[c - 1] if c else left
            t = np.minimum(prev[c] + 1, diag + (ai != bch[c]))
            t = np.where(col[c] == 0, i, t)
            u.append(t - col[c])
        for c in range(1, CPL):
            u[c] = np.minimum(u[c], u[c - 1])
        s = u[CPL - 1]
        d = 1
        while d < W:
            s = np.minimum(s, _shr(s, d, FAR, W))
            d *= 2
        excl = _shr(s, 1, FAR, W)
        live = i <= La
        for c in range(CPL):
            prev[c] = np.where(live, col[c] + np.minimum(u[c], excl), prev[c])
    out = []
    for q, (a, b) in enumerate(pairs):
        out.append(int(prev[len(b) % CPL][q * W + len(b) // CPL]))
    return out


# ---------------------------------------------------------------- many pairs at once
def _bucket(A, B):
    """Pairs (lists of int lists) with len(b) < width of the bucket, sorted by len(a) descending -> distances."""
    P = len(A)
    Wd = max(len(b) for b in B) + 1
    order = sorted(range(P), key=lambda p: -len(A[p]))
    la = np.array([len(A[p]) for p in order])
    rows = int(la[0]) if P else 0
    a_arr = np.full((P, max(rows, 1)), -1, np.int64)
    b_arr = np.full((P, Wd), -2, np.int64)
    for k, p in enumerate(order):
        a_arr[k, :len(A[p])] = A[p]
        b_arr[k, 1:len(B[p]) + 1] = B[p]
    j = np.arange(Wd)
    prev = np.tile(j, (P, 1))
    for i in range(1, rows + 1):
        act = int(np.searchsorted(-la, -i, side='right'))               # pairs with La >= i: a prefix
        pv = prev[:act]
        neq = (a_arr[:act, i - 1][:, None] != b_arr[:act]).astype(np.int64)
        t = pv + 1
        t[:, 1:] = np.minimum(t[:, 1:], pv[:, :-1] + neq[:, 1:])
        t[:, 0] = i
        prev[:act] = np.minimum.accumulate(t - j, axis=1) + j
    out = np.zeros(P, np.int64)
    for k, p in enumerate(order):
        out[p] = prev[k, len(B[p])]
    return out


def pairs_model(A, B):
    """Distances of the pairs (A[p], B[p]) as int64 [P]; buckets by len(b) keep the arrays narrow."""
    out = np.zeros(len(A), np.int64)
    for lo, hi in ((0, 16), (17, 64), (65, 1 << 30)):
        idx = [p for p in range(len(A)) if lo <= len(B[p]) <= hi]
        if idx:
            out[idx] = _bucket([A[p] for p in idx], [B[p] for p in idx])
    return out


# ---------------------------------------------------------------- the entry points' contracts
def string_of(row, length, pitch, ignore=-1):
    """The string the kernel compares: None for "no string" (raw length below 0 or above the pitch, more than 255 characters counted), else the
    first `length` entries of `row` without the `ignore` class."""
    length = int(length)
    if length < 0 or length > pitch:
        return None
    s = [int(v) for v in row[:length] if ignore < 0 or v != ignore]
    return s if len(s) <= MAX_LEN else None


def supported(Ka, Kb, N):
    return 1 <= N <= 65535 and 1 <= Ka <= 65536 and 1 <= Kb <= 65536 and N * Ka * Kb <= MAX_PAIRS


def distance_model(a, a_len, b, b_len, ignore=-1, shared_a=False, shared_b=False, pitch_a=None, pitch_b=None):
    """ocr_edit_distance on numpy operands: a [N, Ka, L] (or [Ka, L] shared) with lengths [N, Ka] ([Ka]); b alike.  The pitch is the last
    dimension unless given.  -> (dist int32 [N, Ka, Kb], a_count, b_count shaped like the lengths)."""
    N = b.shape[0] if shared_a else a.shape[0]
    if shared_a and shared_b:
        N = 1
    Ka, Kb = a.shape[-2], b.shape[-2]
    pa, pb = pitch_a or a.shape[-1], pitch_b or b.shape[-1]

    def strings(x, x_len, shared, pitch):
        flat = x.reshape(-1, x.shape[-1])
        strs = [string_of(flat[r], x_len.reshape(-1)[r], pitch, ignore) for r in range(flat.shape[0])]
        count = np.array([-1 if s is None else len(s) for s in strs], np.int32).reshape(x_len.shape)
        K = x.shape[-2]
        return (lambda n, i: strs[i if shared else n * K + i]), count
    sa, a_count = strings(a, a_len, shared_a, pa)
    sb, b_count = strings(b, b_len, shared_b, pb)
    dist = np.full((N, Ka, Kb), -1, np.int32)
    at, A, B = [], [], []
    for n in range(N):
        for i in range(Ka):
            for j in range(Kb):
                x, y = sa(n, i), sb(n, j)
                if x is not None and y is not None:
                    at.append((n, i, j)); A.append(x); B.append(y)
    if at:
        d = pairs_model(A, B)
        for (n, i, j), v in zip(at, d):
            dist[n, i, j] = v
    return dist, a_count, b_count


def self_model(s, s_len, ignore=-1):
    """distance_model(s, s_len, s, s_len) at half the work: the pairs i < j, mirrored; the diagonal is 0 for a string, -1 for none."""
    N, K, L = s.shape
    strs = [[string_of(s[n, i], s_len[n, i], L, ignore) for i in range(K)] for n in range(N)]
    count = np.array([[-1 if x is None else len(x) for x in row] for row in strs], np.int32)
    dist = np.full((N, K, K), -1, np.int32)
    at, A, B = [], [], []
    for n in range(N):
        for i in range(K):
            if strs[n][i] is None:
                continue
            dist[n, i, i] = 0
            for j in range(i + 1, K):
                if strs[n][j] is not None:
                    at.append((n, i, j)); A.append(strs[n][i]); B.append(strs[n][j])
    if at:
        d = pairs_model(A, B)
        for (n, i, j), v in zip(at, d):
            dist[n, i, j] = dist[n, j, i] = v
    return dist, count


def stats_model(dist, ref_count):
    d, r = np.asarray(dist).reshape(-1).astype(np.int64), np.asarray(ref_count).reshape(-1).astype(np.int64)
    ok = d >= 0
    return [int(d[ok].sum()), int(r[ok].sum()), int((d[ok] == 0).sum()), int(ok.sum())]


def mbr_valid(dist, costs):
    K = costs.shape[1]
    return np.isfinite(costs) & (dist[:, np.arange(K), np.arange(K)] >= 0)


def mbr_pick(risk, costs, valid):
    """The arg-min of each risk row over the valid candidates under (risk, cost, index); -1 where there is none."""
    best = np.full(risk.shape[0], -1, np.int32)
    for n in range(risk.shape[0]):
        keys = [(float(risk[n, j]), float(costs[n, j]), j) for j in range(risk.shape[1]) if valid[n, j]]
        if keys:
            best[n] = min(keys)[2]
    return best


def mbr_model(dist, costs):
    """ocr_mbr_select in float64 on the float32 costs: -> (risk [N, K] float64, +inf for an invalid candidate; best; best_risk)."""
    dist, costs = np.asarray(dist), np.asarray(costs, np.float32)
    N, K = costs.shape
    valid = mbr_valid(dist, costs)
    risk = np.full((N, K), np.inf)
    for n in range(N):
        v = valid[n]
        if not v.any():
            continue
        c = costs[n].astype(np.float64)
        w = np.where(v, np.exp(np.where(v, c[v].min() - c, 0.0)), 0.0)
        risk[n, v] = (dist[n][np.ix_(v, v)].astype(np.float64) * w[v][None, :]).sum(axis=1) / w[v].sum()
    best = mbr_pick(risk, costs, valid)
    best_risk = np.array([risk[n, best[n]] if best[n] >= 0 else np.inf for n in range(N)])
    return risk, best, best_risk


# ---------------------------------------------------------------- cases
def _string(rng, L, C):
    """L symbols of an alphabet of C: the classes 1 .. C (class 0 is kept free for `ignore`)."""
    return [int(v) for v in rng.randint(1, C + 1, size=L)]


def _sprinkle(rng, s, raw, ignore):
    """s with the `ignore` class put in at random places, raw characters in all."""
    out = list(s)
    while len(out) < raw:
        out.insert(int(rng.randint(len(out) + 1)), ignore)
    return out


def derive(regime, base, C, rng, Lb):
    """The partner of `base` under a regime (Lb: the length wanted where the regime leaves it free)."""
    L = len(base)
    if regime == 'identical':
        return list(base)
    if regime == 'one_edit':
        kind = 2 if L == 0 else int(rng.randint(2)) if L == MAX_LEN else int(rng.randint(3))         # substitute, delete, insert
        i = int(rng.randint(max(L, 1)))
        if kind == 0:
            return base[:i] + [1 + (base[i] - 1 + int(rng.randint(1, C))) % C] + base[i + 1:]
        if kind == 1:
            return base[:i] + base[i + 1:]
        return base[:i] + _string(rng, 1, C) + base[i:]
    if regime == 'reversed':
        return base[::-1]
    if regime == 'repeated':
        return [base[0] if L and rng.randint(2) else 1] * Lb
    if regime == 'disjoint':
        return [v + C for v in _string(rng, Lb, C)]                       # classes the base cannot hold
    if regime == 'common_ends':
        k = int(rng.randint(min(L, Lb) + 1))
        mid = _string(rng, Lb - k, C)
        return base[:k] + mid if rng.randint(2) else mid + base[L - k:]
    return _string(rng, Lb, C)                                            # 'random' and 'ignore'


def self_case(C, N=3, K=100, pitch=520, seed=0, lengths=LENGTHS + OWN_EDGES):
    """One self-pairing launch: N x K strings, string 2m a base and string 2m + 1 its partner under regime m % 8, the bases' lengths cycling
    through `lengths` from a start that moves with the sample, the partners' free lengths cycling the other way; the strings of the 'ignore'
    regime carry class 0 sprinkled in up to a raw length of `pitch`; 'repeated' bases are one character.  The space beyond each string holds
    the string's own last character (what would make it match more).  -> (s int32 [N, K, pitch], s_len int32 [N, K], ignore = 0)."""
    rng = np.random.RandomState(1000 * C + seed)
    s = np.zeros((N, K, pitch), np.int32)
    s_len = np.zeros((N, K), np.int32)
    for n in range(N):
        for m in range((K + 1) // 2):
            regime = REGIMES[m % len(REGIMES)]
            L = lengths[(m // len(REGIMES) * 3 + m + 5 * n) % len(lengths)]
            Lb = lengths[(7 * m + 3 * n + 1) % len(lengths)]
            base = [1 + int(rng.randint(C))] * L if regime == 'repeated' else _string(rng, L, C)
            other = derive(regime, base, C, rng, Lb)
            if regime == 'ignore':
                base = _sprinkle(rng, base, int(rng.randint(len(base), pitch + 1)), 0)
                other = _sprinkle(rng, other, int(rng.randint(len(other), pitch + 1)), 0)
            for k, x in ((2 * m, base[:pitch]), (2 * m + 1, other[:pitch])):
                if k < K:
                    s[n, k, :len(x)] = x
                    s[n, k, len(x):] = x[-1] if x else 1
                    s_len[n, k] = len(x)
    return s, s_len, 0


def mbr_known():
    """abc / xbd / xbe with probabilities 0.40 / 0.35 / 0.25: the MAP choice is candidate 0, the MBR choice candidate 1."""
    cands = [[1, 2, 3], [4, 2, 5], [4, 2, 6]]
    p = np.array([0.40, 0.35, 0.25])
    dist = np.array([[[textbook(x, y) for y in cands] for x in cands]], np.int32)
    return cands, dist, (-np.log(p)).astype(np.float32)[None, :]


def mbr_random(N, K, seed):
    """Random symmetric distances with a zero diagonal and costs; some costs +inf, some candidates marked "no string" (-1 in their row and
    column), one sample with no valid candidate at all, exact cost ties (the order then falls to the index)."""
    rng = np.random.RandomState(seed)
    d = rng.randint(0, 40, size=(N, K, K)).astype(np.int32)
    d = np.maximum(d, d.transpose(0, 2, 1))
    d[:, np.arange(K), np.arange(K)] = 0
    costs = (rng.rand(N, K) * 6.0 + rng.rand(N, 1) * 50.0).astype(np.float32)
    costs[rng.rand(N, K) < 0.15] = np.inf
    if K > 1:
        costs[:, 1] = costs[:, 0]                                         # a tie on the cost
    for n in range(N):
        for j in np.nonzero(rng.rand(K) < 0.1)[0]:
            d[n, j, :] = -1
            d[n, :, j] = -1
    costs[N - 1, :] = np.inf                                              # nobody valid
    if N > 2:
        d[N - 2, np.arange(K), np.arange(K)] = -1                         # nobody valid, by the diagonal
    return d, costs
