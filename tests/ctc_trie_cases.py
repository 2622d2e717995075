"""Lexicon scoring on a prefix tree (ctc_trie.hip: ocr_ctc_trie_build, ctc_trie_kernel; lexicon.LexiconTrie, ops.ctc_score_trie): what its CPU and
GPU tests share.  A helper module, not collected.

Cases, float64 reference and bounds are those of tests/ctc_score_cases.py, unchanged: the tree's recursion is the candidates kernel's, slot for
slot (pnb(v) is alpha at the node's label slot, pb(v) alpha at the blank slot behind it), so its float32 floor is the one measured there;
tests/test_ctc_trie_cases.py measures it again with the model below in float32 and prints it.  The reference of every cost is the per-word
ctc_score_cases.alpha_cost in float64, which knows nothing of the builder.

Added here: a numpy model of the chunked recursion over the builder's own arrays, and dense lexicons, "every string of up to d labels over a
symbols" (1 + a + ... + a^d words, the empty one included, and as many nodes), in order of length, so that every leading part of the list is
closed under prefixes and has as many nodes as words."""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_score_cases as sc  # noqa: E402

_lse = sc._lse
MAX_K = 1 << 20


def supported(C, T, K):
    return 1 <= C <= sc.MAX_C and T >= 1 and 1 <= K <= MAX_K


def build(k, chunk_nodes=None):
    """The LexiconTrie of a case's packed lexicon (padding words and declared lengths as the case has them)."""
    from lstm_ctc_ocr_amd.lexicon import LexiconTrie
    lab, lens = k.packed()
    return LexiconTrie((lab, lens), k.C, blank=k.blank, chunk_nodes=chunk_nodes)


def valid(k, j):
    """ocr_ctc_score could price word j finite for some sample."""
    return sc.candidate_ok(k.lexicon[j], int(k.lens[j]), k.mll, k.C, k.blank, 1 << 30)


def deepest(k):
    return max([int(k.lens[j]) for j in range(k.K) if valid(k, j)] or [0])


def chunk_sizes(k):
    """The chunk sizes the tests run a case at: the least the builder takes, that + 3, 64, and the default (None)."""
    d = deepest(k) + 1
    return [d, d + 3, max(64, d), None]


def dense_words(a, d, first=1):
    """Every string of up to d labels over the symbols first .. first + a - 1, shortest first."""
    return [list(s) for n in range(d + 1) for s in itertools.product(range(first, first + a), repeat=n)]


def dense_case(name, a, d, T=10, C=12, in_lens=(10, 7), seed=500, extra=()):
    """A ScoreCase whose lexicon is dense_words(a, d) followed by `extra`."""
    return sc.ScoreCase(name, seed, T, C, list(in_lens), dense_words(a, d) + [list(w) for w in extra], mll=max([d] + [len(w) for w in extra]))


def trie_model(trie, acts, il, dtype):
    """costs [N, K] of the chunked recursion in `dtype` over the builder's arrays, a chunk at a time as a workgroup runs it:
        pnb_t(v) = y_t[c_v] + lse(pnb_{t-1}(v), pb_{t-1}(p_v), [flag_v] pnb_{t-1}(p_v)),  pb_t(v) = y_t[blank] + lse(pb_{t-1}(v), pnb_{t-1}(v)),
    pb_{-1}(root) = 0 and -inf elsewhere; a word that ends in v costs -lse(pb(v), pnb(v)) after the sample's last frame, +inf where that is -inf,
    where the word has no node (-1) and where the sample has no frame."""
    dtype = np.dtype(dtype).type
    NEG = dtype(-np.inf)
    T, N, _ = acts.shape
    costs = np.full((N, trie.num_words), np.inf, dtype)
    label, parent, flag = trie.node_label, trie.node_parent, trie.node_flag.astype(bool)
    for n in range(N):
        Tn = min(int(il[n]), T)
        if Tn <= 0:
            continue
        rows = acts[:Tn, n].astype(dtype)
        logy = rows - _lse(rows, 1)[:, None]
        for ch in range(trie.num_chunks):
            a, b = int(trie.chunk_node_start[ch]), int(trie.chunk_node_start[ch + 1])
            lab, par, flg = label[a:b], parent[a:b], flag[a:b]
            live = np.arange(b - a) > 0
            pb, pnb = np.full(b - a, NEG, dtype), np.full(b - a, NEG, dtype)
            pb[0] = 0
            with np.errstate(invalid='ignore'):
                for t in range(Tn):
                    take = np.stack([pnb, pb[par], np.where(flg, pnb[par], NEG)])
                    new = np.where(live, _lse(take, 0) + logy[t, lab], NEG)
                    pb = _lse(np.stack([pb, pnb]), 0) + logy[t, trie.blank]
                    pnb = new
                for w in range(int(trie.chunk_word_start[ch]), int(trie.chunk_word_start[ch + 1])):
                    v = int(trie.word_node[w])
                    if v >= 0:
                        e = _lse(np.array([pb[v], pnb[v]], dtype), 0)
                        costs[n, int(trie.word_index[w])] = -e if np.isfinite(e) else np.inf
    return costs


def spell(trie, ch, v):
    """The labels on the path from chunk ch's root to its node v."""
    a = int(trie.chunk_node_start[ch])
    out = []
    while v > 0:
        out.append(int(trie.node_label[a + v]))
        v = int(trie.node_parent[a + v])
    return out[::-1]
