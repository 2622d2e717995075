"""Flat-logit inputs on which a prefix leaves the beam and comes back, and a float64 model of ctc_beam.hip's trie bookkeeping: shared by
test_beam_reentry_cases.py (CPU) and test_gpu_beam_reentry.py.

The kernel keeps one trie node per prefix (npar / nlab / nslot in the workspace); a beam entry finds its parent's slot through
nslot[npar[node]] and gets the parent's mass through it.  `kernel_bookkeeping_model` follows that bookkeeping literally in float64:
node ids, the parent slot recomputed through nslot every frame, child candidates suppressed only by the (parent slot, label) pairs of
entries whose parent is in the beam, the K best of {leaves} u {candidates} with ties in index order.  With canonical=False every child
that enters the beam gets a FRESH node, which is what the kernel did before node identity became per prefix: a prefix P that drops
out while its extension Q = P + c stays, and later comes back, then has a second node; Q still hangs off the first one, never gets
P's mass again, and (P, c) is scored as a new candidate that can enter the beam as a second copy of Q.  With canonical=True the node of
(parent node, label) is reused and the model is the dictionary algorithm of oracle/decode.py in different clothes.

On the boosted randn * 3 logits of the other beam tests a prefix that leaves never returns; on flat logits (randn * scale, scale <= 1,
no boosts) it happens all the time.  CASES pins inputs where, by the oracle and the model alone (nothing is measured on the code under
test), every sample's top path is stable under three N(0, 1e-4) perturbations (beam_wide_cases.conditions) and the canonical=False
model gives a different top path or a score beyond the GPU tests' tolerance on at least two samples.  Seeds were found with `find_seed`.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_wide_cases as bw  # noqa: E402

NEG = -math.inf
DEAD_LOGIT = -20.0
LIVE_CLASSES = 8          # of an alphabet beyond 64 classes: the blank and 7 others, see make_flat_logits


def make_flat_logits(T, N, C, scale, seed):
    """float32 randn * scale, no boosts; il[0] = T, the other input lengths from [T // 2, T].  On an alphabet beyond 64 classes a
    re-entry needs the mass on few classes (a flat row over 300 never brings a prefix back into a beam of 8), so there only the blank
    and 7 other classes, drawn from the whole range, keep their randn * scale and the rest sit at -20: the wide kernel's class
    selection (M = K + 1 = 9) then takes the 7 and fills up from classes tied at exactly -20."""
    rng = np.random.RandomState(seed)
    acts = (rng.randn(T, N, C) * scale).astype(np.float32)
    il = rng.randint(T // 2, T + 1, N).astype(np.int32)
    il[0] = T
    if C > 64:
        live = np.sort(rng.choice(C - 1, LIVE_CLASSES - 1, replace=False))
        dead = np.ones(C, bool)
        dead[live] = False
        dead[C - 1] = False
        acts[:, :, dead] = DEAD_LOGIT
    return acts, il


def kernel_bookkeeping_model(x_tc, K, canonical, restrict=False):
    """(top path, its log-probability, whether some frame's beam held one prefix twice) for one sample's [T, C] logits.
    restrict=True scores only the wide kernel's per-frame class selection (beam_wide_cases.select_classes)."""
    x = np.asarray(x_tc, np.float64)
    C = x.shape[1]
    blank = C - 1
    m = x.max(axis=-1, keepdims=True)
    logp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    M = min(K + 1, C - 1)
    npar, nlab, nslot, nprefix = [-1], [-1], [0], [()]
    child_of = {}                                          # canonical: (parent node, label) -> node
    node, last, ps, pb, pnb, tot = [0], [-1], [-1], [0.0], [NEG], [0.0]
    twice = False
    for t in range(x.shape[0]):
        row = logp[t]
        nb = len(node)
        classes = bw.select_classes(row, blank, M) if restrict else range(C - 1)
        # (b) leaves
        leaf = []
        for s in range(nb):
            nl = NEG
            if last[s] >= 0:
                nl = pnb[s]
                p = ps[s]
                if p >= 0:
                    nl = bw._lse(nl, pb[p] if last[s] == last[p] else tot[p])
                if nl != NEG:
                    nl += float(row[last[s]])
            npb = tot[s] + float(row[blank])
            leaf.append((npb, nl))
        cand = [(bw._lse(*leaf[s]), s, -1) for s in range(nb)]
        # (c) children that are not in the beam, as far as (parent slot, label) tells
        in_beam = set((ps[s], last[s]) for s in range(nb) if ps[s] >= 0)
        for b in range(nb):
            for c in classes:
                v = NEG
                if (b, c) not in in_beam:
                    prev = pb[b] if c == last[b] else tot[b]
                    if prev != NEG:
                        v = prev + float(row[c])
                cand.append((v, b, c))
        # (d), (e) the K best, above the threshold in index order, then ties in index order
        finite = [i for i, cv in enumerate(cand) if cv[0] != NEG]
        if len(finite) <= K:
            sel = finite
        else:
            thr = sorted((cand[i][0] for i in finite), reverse=True)[K - 1]
            sel = [i for i in finite if cand[i][0] > thr]
            sel += [i for i in finite if cand[i][0] == thr][:K - len(sel)]
        # (f) next generation
        for s in range(nb):
            nslot[node[s]] = -1
        node2, last2, pb2, pnb2, tot2 = [], [], [], [], []
        for i in sel:
            v, b, c = cand[i]
            if c < 0:
                node2.append(node[b]); last2.append(last[b]); pb2.append(leaf[b][0]); pnb2.append(leaf[b][1])
            else:
                nid = child_of.get((node[b], c)) if canonical else None
                if nid is None:
                    nid = len(npar)
                    npar.append(node[b]); nlab.append(c); nslot.append(-1); nprefix.append(nprefix[node[b]] + (c,))
                    child_of[(node[b], c)] = nid
                node2.append(nid); last2.append(c); pb2.append(NEG); pnb2.append(v)
            tot2.append(v)
        for s, nid in enumerate(node2):
            nslot[nid] = s
        ps = [nslot[npar[nid]] if npar[nid] >= 0 else -1 for nid in node2]
        node, last, pb, pnb, tot = node2, last2, pb2, pnb2, tot2
        twice = twice or len(set(nprefix[nid] for nid in node)) < len(node)
    best = 0
    for s in range(1, len(node)):
        if tot[s] > tot[best]:
            best = s
    return list(nprefix[node[best]]), tot[best], twice


def differs(path, score, ref_path, ref_score):
    """What the GPU tests would see: another label sequence, or a score beyond 1e-3 * max(1, |score|)."""
    return path != ref_path or abs(score - ref_score) >= 1e-3 * max(1.0, abs(ref_score))


def model_mismatches(acts, il, K, ref, restrict=False):
    """Samples on which the canonical=False model differs from the oracle's (sequences, scores)."""
    out = []
    for n in range(acts.shape[1]):
        path, score, _ = kernel_bookkeeping_model(acts[:il[n], n, :], K, canonical=False, restrict=restrict)
        if differs(path, score, ref[0][n], ref[1][n]):
            out.append(n)
    return out


# (T, N, C, K, scale, seed).  The last is the wide-alphabet case: the default engine runs the table kernel on it (K = 8 keeps its LDS at
# about 23 KB), so the GPU test decodes it on the forced wide kernel too, where M = 9 < C - 1 prunes.
CASES = [
    (16, 6, 5, 4, 1.0, 2384),
    (24, 6, 6, 8, 0.7, 632),
    (30, 4, 8, 16, 1.0, 55),
    (32, 6, 6, 32, 0.7, 29),
    (32, 6, 8, 100, 0.7, 26),
    (40, 6, 300, 8, 1.0, 2870),
]
MIN_MISMATCHES = 2


def find_seed(T, N, C, K, scale, tries=6000):
    """First seed that meets the conditions.  About one sample in 150 (K <= 8) to one in 15 (K = 100) shows the defect and two of a
    batch must, hence the high seeds of the small beams: a search takes a minute or two."""
    for seed in range(tries):
        acts, il = make_flat_logits(T, N, C, scale, seed)
        ref = bw.beam_search_pruned(acts, il, beam_width=K, merge_repeated=False)
        if len(model_mismatches(acts, il, K, ref, restrict=C > 64)) < MIN_MISMATCHES:
            continue
        if bw.conditions(acts, il, K, False)[0]:
            return seed
    raise RuntimeError("no seed in %d tries meets the conditions for %r" % (tries, (T, N, C, K, scale)))


_cache = {}


def build_case(case):
    """(acts, input_lengths, {merge_repeated: (sequences, scores)}) - computed once per process and shared."""
    if case not in _cache:
        T, N, C, K, scale, seed = case
        acts, il = make_flat_logits(T, N, C, scale, seed)
        seqs, scores = bw.beam_search_pruned(acts, il, beam_width=K, merge_repeated=False)
        ref = {False: (seqs, scores), True: ([bw.merge_repeats(s) for s in seqs], scores)}
        acts.setflags(write=False)
        il.setflags(write=False)
        _cache[case] = (acts, il, ref)
    return _cache[case]


if __name__ == "__main__":
    import time
    for T, N, C, K, scale, _ in CASES if len(sys.argv) < 2 else [CASES[int(v)] for v in sys.argv[1:]]:
        t0 = time.time()
        print((T, N, C, K, scale), "seed", find_seed(T, N, C, K, scale), "%.1f s" % (time.time() - t0), flush=True)
