"""Deterministic weighted automata over labels: what ops.ctc_beam_lm (ctc_beam.hip, ocr_ctc_beam_decode_lm) fuses into the CTC prefix search.

A LabelAutomaton has num_states states, start state 0, and three tables indexed by the caller's class ids:

    next   int32   [num_states, num_classes]   the state after reading class c in state s
    weight float32 [num_states, num_classes]   what that transition adds to the score; -inf = forbidden
    final  float32 [num_states]                what ending the string in state s adds; -inf = the string may not end here

The column of the CTC blank is never read; `blank` records which class that is, and
ops.ctc_beam_lm refuses to run an automaton with another blank than its own.  A string P = c_1 .. c_L scores

    score(P) = sum_i weight[s_{i-1}][c_i] + final[s_L],   s_i = next[s_{i-1}][c_i],   s_0 = 0

or -inf when a transition is forbidden or the last state may not end.  The builders compile the three common sources to that form: a
character n-gram (states are the histories), a word list (its trie) and a positional format (a chain of states).  The tables are float32
because that is what the device reads; `score` sums them in float64.
"""
import math

import numpy as np

NEG = -np.inf


class LabelAutomaton:
    def __init__(self, next, weight, final, blank=0):
        self.next, self.weight, self.final, self.blank = next, weight, final, int(blank)
        self.validate()
        self.num_states, self.num_classes = (int(v) for v in self.weight.shape)
        self._device = {}

    MAX_STATES = 1 << 20          # ops.ctc_beam_lm's limit

    def validate(self):
        """Raises ValueError for a malformed table: anything but int32 [H, C] / float32 [H, C] / float32 [H] numpy arrays with 1 <= H <= 1048576
        and C >= 2, a NaN or +inf weight or end weight, or a finite weight whose next state lies outside [0, H).  (A forbidden transition's
        next is never followed and may hold anything.)  The blank must be one of the classes."""
        nxt, weight, final = self.next, self.weight, self.final
        for name, arr, dtype, ndim in (('next', nxt, np.int32, 2), ('weight', weight, np.float32, 2), ('final', final, np.float32, 1)):
            if not isinstance(arr, np.ndarray) or arr.dtype != dtype or arr.ndim != ndim:
                raise ValueError('%s must be a %d-dimensional numpy array of %s (got %s)' % (
                    name, ndim, np.dtype(dtype).name, '%s %s' % (arr.dtype, arr.shape) if isinstance(arr, np.ndarray) else type(arr).__name__))
        H, C = weight.shape
        if nxt.shape != (H, C) or final.shape != (H,):
            raise ValueError('next %s, weight %s and final %s do not describe one automaton' % (nxt.shape, weight.shape, final.shape))
        if not (1 <= H <= self.MAX_STATES and C >= 2):
            raise ValueError('an automaton has 1 .. %d states over at least 2 classes (got %d states, %d classes)' % (self.MAX_STATES, H, C))
        if not 0 <= self.blank < C:
            raise ValueError('blank %d outside the %d classes' % (self.blank, C))
        if np.isnan(weight).any() or np.isposinf(weight).any() or np.isnan(final).any() or np.isposinf(final).any():
            raise ValueError('weights and end weights are finite or -inf (NaN or +inf found)')
        bad = np.isfinite(weight) & ((nxt < 0) | (nxt >= H))
        if bad.any():
            s, c = (int(v[0]) for v in np.nonzero(bad))
            raise ValueError('the transition (%d, %d) has the finite weight %r but leads to state %d of %d' % (s, c, float(weight[s, c]), int(nxt[s, c]), H))

    def walk(self, labels):
        """(W, state) after reading labels from the start state: W the float64 sum of the weights; (-inf, -1) on a forbidden transition."""
        s, total = 0, 0.0
        for c in labels:
            c = int(c)
            if not 0 <= c < self.num_classes:
                return NEG, -1
            w = float(self.weight[s, c])
            if not np.isfinite(w):
                return NEG, -1
            total += w
            s = int(self.next[s, c])
        return total, s

    def score(self, labels):
        """W(labels) + final[state], float64; -inf for a string the automaton does not accept."""
        total, s = self.walk(labels)
        if s < 0 or not np.isfinite(self.final[s]):
            return NEG
        return total + float(self.final[s])

    def accepts(self, labels):
        return self.score(labels) != NEG

    def device_arrays(self, device):
        """(next, weight, final) as contiguous tensors on `device`, copied on the first call per device (call it ahead of a graph capture)."""
        import torch
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (self.next, self.weight, self.final))
        return self._device[key]

    # ------------------------------------------------------------------------------------------------------------------ builders
    @classmethod
    def zero(cls, num_classes, blank=0):
        """One state, every weight 0: the fused search with it is the plain prefix search."""
        return cls(np.zeros((1, num_classes), np.int32), np.zeros((1, num_classes), np.float32), np.zeros(1, np.float32), blank=blank)

    @classmethod
    def from_ngram(cls, lm, alpha, beta, blank=0):
        """The shallow fusion of rescoring.rerank inside the search: weight = alpha * log P(c | history) + beta, final = alpha * log P(end |
        history), so score(s) == alpha * lm.log_prob(s) + beta * len(s).  lm is a rescoring.CharNGram (anything with order, num_classes,
        END and cond_log_prob(history, symbol)); the states are the histories of up to order - 1 labels, 1 + V + .. + V^(order-1) of them
        for V = num_classes - 1 labels.  The model's labels 1 .. num_classes - 1 are the non-blank classes in ascending order: themselves for
        blank 0 (the model's own convention), class k - 1 for a label k <= blank otherwise."""
        C, order = int(lm.num_classes), int(lm.order)
        if not 0 <= blank < C:
            raise ValueError('blank %d outside the %d classes' % (blank, C))
        V = C - 1
        classes = [k for k in range(C) if k != blank]                 # classes[j] is the class of the model's label j + 1
        starts = [0]                                                  # index of the first history of each length
        for length in range(order - 1):
            starts.append(starts[-1] + V ** length)
        H = starts[-1] + V ** (order - 1)
        if H > cls.MAX_STATES:
            raise ValueError('an order-%d model over %d labels has %d histories (at most %d states)' % (order, V, H, cls.MAX_STATES))

        def index(hist):                                              # hist: tuple of model labels 1 .. V
            v = 0
            for lab in hist:
                v = v * V + (lab - 1)
            return starts[len(hist)] + v

        nxt = np.zeros((H, C), np.int32)
        weight = np.full((H, C), NEG, np.float32)
        final = np.zeros(H, np.float32)
        hists = [()]
        while hists:
            longer = []
            for hist in hists:
                s = index(hist)
                final[s] = alpha * lm.cond_log_prob(hist, lm.END)
                for j, k in enumerate(classes):
                    after = (hist + (j + 1,))[-(order - 1):] if order > 1 else ()
                    nxt[s, k] = index(after)
                    weight[s, k] = alpha * lm.cond_log_prob(hist, j + 1) + beta
                    if len(hist) < order - 1:
                        longer.append(hist + (j + 1,))
            hists = longer
        return cls(nxt, weight, final, blank=blank)

    @classmethod
    def from_lexicon(cls, words, num_classes, blank=0):
        """The trie of a word list (label lists over the classes but the blank): weight 0 along its edges and -inf elsewhere, final 0 where a
        word ends and -inf elsewhere.  It accepts exactly the words, each with score 0."""
        child = [{}]
        ends = [False]
        for word in words:
            s = 0
            for c in word:
                c = int(c)
                if not 0 <= c < num_classes or c == blank:
                    raise ValueError('label %d in a lexicon over %d classes with blank %d' % (c, num_classes, blank))
                if c not in child[s]:
                    child[s][c] = len(child)
                    child.append({})
                    ends.append(False)
                s = child[s][c]
            ends[s] = True
        H = len(child)
        nxt = np.zeros((H, num_classes), np.int32)
        weight = np.full((H, num_classes), NEG, np.float32)
        for s, edges in enumerate(child):
            for c, t in edges.items():
                nxt[s, c] = t
                weight[s, c] = 0.0
        return cls(nxt, weight, np.where(np.array(ends), 0.0, NEG).astype(np.float32), blank=blank)

    @classmethod
    def from_pattern(cls, allowed, min_len, num_classes, blank=0):
        """A positional format: allowed[i] is the collection of classes permitted at position i, and the strings of min_len .. len(allowed)
        characters that respect it are accepted, each with score 0.  One state per position; the blank is permitted nowhere."""
        L = len(allowed)
        if not 0 <= min_len <= L:
            raise ValueError('min_len %d outside 0 .. %d' % (min_len, L))
        nxt = np.zeros((L + 1, num_classes), np.int32)
        weight = np.full((L + 1, num_classes), NEG, np.float32)
        for i, classes in enumerate(allowed):
            for c in classes:
                c = int(c)
                if not 0 <= c < num_classes or c == blank:
                    raise ValueError('class %d at position %d of a pattern over %d classes with blank %d' % (c, i, num_classes, blank))
                nxt[i, c] = i + 1
                weight[i, c] = 0.0
        final = np.where(np.arange(L + 1) >= min_len, 0.0, NEG).astype(np.float32)
        return cls(nxt, weight, final, blank=blank)


class SparseLabelAutomaton:
    """A deterministic weighted automaton with failure (back-off) transitions, start state 0, whose size follows the arcs that exist: what
    ops.ctc_beam_lm_sparse (ctc_beam.hip, ocr_ctc_beam_decode_lm_sparse) fuses into the wide-alphabet prefix search.  H states, A arcs, over the
    caller's class ids:

        arc_begin      int32   [H + 1]   the arcs of state s are arc_begin[s] .. arc_begin[s + 1] - 1
        arc_label      int32   [A]       ascending within a state, never the blank
        arc_next       int32   [A]
        arc_weight     float32 [A]       finite, or -inf = this transition is forbidden (no back-off is tried)
        backoff        int32   [H]       the state to retry in when s has no arc for the class; -1 = none
        backoff_weight float32 [H]       paid for that hop
        final          float32 [H]       as LabelAutomaton.final

    step(s, c) searches the arcs of s for c by bisection.  A hit is the transition (acc + arc_weight, arc_next), forbidden when the weight is not
    finite or the next state lies outside [0, H).  A miss adds backoff_weight[s] to acc and retries in backoff[s] when that lies in [0, H) and the
    weight is finite, else the transition is forbidden; at most MAX_HOPS hops are taken.  acc is summed in float32 in hop order and the arc
    weight is added last, so this class, to_dense and the kernel agree to the bit.  `score` sums those float32 weights in float64, like
    LabelAutomaton.score."""

    MAX_HOPS = 8
    MAX_STATES = 1 << 24          # ops.ctc_beam_lm_sparse's limits
    MAX_ARCS = 1 << 28
    FIELDS = ('arc_begin', 'arc_label', 'arc_next', 'arc_weight', 'backoff', 'backoff_weight', 'final')

    def __init__(self, arc_begin, arc_label, arc_next, arc_weight, backoff, backoff_weight, final, num_classes, blank=0):
        self.arc_begin, self.arc_label, self.arc_next, self.arc_weight = arc_begin, arc_label, arc_next, arc_weight
        self.backoff, self.backoff_weight, self.final = backoff, backoff_weight, final
        self.num_classes, self.blank = int(num_classes), int(blank)
        self.validate()
        self.num_states, self.num_arcs = int(self.final.shape[0]), int(self.arc_label.shape[0])
        self._device = {}

    def arrays(self):
        return tuple(getattr(self, name) for name in self.FIELDS)

    def validate(self):
        """Raises ValueError for: arrays of another dtype or shape than the table above, H outside 1 .. 1 << 24 or A above 1 << 28, fewer than 2
        classes or a blank outside them, an arc_begin that is not monotone from 0 to A, labels that are out of range, equal to the blank, or not
        strictly ascending within a state, a finite arc weight whose next state lies outside [0, H), a NaN or +inf weight anywhere, a backoff
        outside -1 .. H - 1, and a back-off chain that cycles or is longer than MAX_HOPS."""
        dtypes = dict(arc_begin=np.int32, arc_label=np.int32, arc_next=np.int32, arc_weight=np.float32, backoff=np.int32,
                      backoff_weight=np.float32, final=np.float32)
        for name in self.FIELDS:
            arr = getattr(self, name)
            if not isinstance(arr, np.ndarray) or arr.dtype != dtypes[name] or arr.ndim != 1:
                raise ValueError('%s must be a 1-dimensional numpy array of %s (got %s)' % (
                    name, np.dtype(dtypes[name]).name, '%s %s' % (arr.dtype, arr.shape) if isinstance(arr, np.ndarray) else type(arr).__name__))
        H, A, C = self.final.shape[0], self.arc_label.shape[0], self.num_classes
        if not (1 <= H <= self.MAX_STATES and 0 <= A <= self.MAX_ARCS and C >= 2):
            raise ValueError('an automaton has 1 .. %d states and at most %d arcs over at least 2 classes (got %d states, %d arcs, %d classes)'
                             % (self.MAX_STATES, self.MAX_ARCS, H, A, C))
        if self.arc_begin.shape != (H + 1,) or self.arc_next.shape != (A,) or self.arc_weight.shape != (A,) or self.backoff.shape != (H,) or \
                self.backoff_weight.shape != (H,):
            raise ValueError('the arrays do not describe one automaton of %d states and %d arcs' % (H, A))
        if not 0 <= self.blank < C:
            raise ValueError('blank %d outside the %d classes' % (self.blank, C))
        begin = self.arc_begin.astype(np.int64)
        if begin[0] != 0 or begin[-1] != A or (np.diff(begin) < 0).any():
            raise ValueError('arc_begin must rise monotonically from 0 to the number of arcs (%d)' % A)
        lab = self.arc_label
        if ((lab < 0) | (lab >= C) | (lab == self.blank)).any():
            raise ValueError('arc labels are classes 0 .. %d other than the blank %d' % (C - 1, self.blank))
        if A > 1:
            first = np.zeros(A, bool)
            first[begin[:-1][begin[:-1] < A]] = True              # the first arc of every state that has one
            if ((np.diff(lab.astype(np.int64)) <= 0) & ~first[1:]).any():
                raise ValueError('the labels of a state must be strictly ascending (unsorted or duplicated labels found)')
        for name in ('arc_weight', 'backoff_weight', 'final'):
            arr = getattr(self, name)
            if np.isnan(arr).any() or np.isposinf(arr).any():
                raise ValueError('%s holds finite values or -inf (NaN or +inf found)' % name)
        if (np.isfinite(self.arc_weight) & ((self.arc_next < 0) | (self.arc_next >= H))).any():
            raise ValueError('an arc of finite weight leads outside the %d states' % H)
        if ((self.backoff < -1) | (self.backoff >= H)).any():
            raise ValueError('backoff holds -1 or a state 0 .. %d' % (H - 1))
        cur = self.backoff.astype(np.int64)
        for _ in range(self.MAX_HOPS):
            cur = np.where(cur >= 0, self.backoff[np.maximum(cur, 0)], -1)
        if (cur >= 0).any():
            raise ValueError('a back-off chain cycles or is longer than %d hops' % self.MAX_HOPS)

    def step(self, s, c):
        """(weight, next state) of reading class c in state s, the weight a numpy float32; None where the transition is forbidden."""
        H, A = self.final.shape[0], self.arc_label.shape[0]
        acc = np.float32(0.0)
        hops = 0
        while True:
            lo = min(max(int(self.arc_begin[s]), 0), A)
            end = min(max(int(self.arc_begin[s + 1]), 0), A)
            hi = max(end, lo)
            while lo < hi:
                mid = (lo + hi) >> 1
                if self.arc_label[mid] < c:
                    lo = mid + 1
                else:
                    hi = mid
            if lo < end and self.arc_label[lo] == c:
                aw = self.arc_weight[lo]
                w = np.float32(acc + aw)
                nx = int(self.arc_next[lo])
                return (w, nx) if np.isfinite(aw) and np.isfinite(w) and 0 <= nx < H else None
            bo, bw = int(self.backoff[s]), self.backoff_weight[s]
            if hops == self.MAX_HOPS or not 0 <= bo < H or not np.isfinite(bw):
                return None
            acc = np.float32(acc + bw)
            s = bo
            hops += 1

    def walk(self, labels):
        """(W, state) after reading labels from the start state: W the float64 sum of the steps' float32 weights; (-inf, -1) on a forbidden
        transition."""
        s, total = 0, 0.0
        for c in labels:
            c = int(c)
            tr = self.step(s, c) if 0 <= c < self.num_classes and c != self.blank else None
            if tr is None:
                return NEG, -1
            total += float(tr[0])
            s = tr[1]
        return total, s

    def score(self, labels):
        """W(labels) + final[state], float64; -inf for a string the automaton does not accept."""
        total, s = self.walk(labels)
        if s < 0 or not np.isfinite(self.final[s]):
            return NEG
        return total + float(self.final[s])

    def accepts(self, labels):
        return self.score(labels) != NEG

    def device_arrays(self, device):
        """The seven arrays in the order of FIELDS as contiguous tensors on `device`, copied on the first call per device.  (An automaton
        without arcs gets one-element arc arrays, which are never read: the entry refuses NULL operands.)"""
        import torch
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))).to(device)
                                      for a in self.arrays())
        return self._device[key]

    # ------------------------------------------------------------------------------------------------------------------ builders
    @classmethod
    def zero(cls, num_classes, blank=0):
        """One state with an arc of weight 0 to itself for every class but the blank: the fused search with it is the plain prefix search
        restricted to each frame's `cutoff` likeliest classes."""
        labels = np.array([k for k in range(num_classes) if k != blank], np.int32)
        A = labels.shape[0]
        return cls(np.array([0, A], np.int32), labels, np.zeros(A, np.int32), np.zeros(A, np.float32), np.full(1, -1, np.int32),
                   np.zeros(1, np.float32), np.zeros(1, np.float32), num_classes, blank=blank)

    @classmethod
    def from_dense(cls, automaton):
        """The arcs of a LabelAutomaton's finite entries (the blank's column left out), no back-off."""
        weight = automaton.weight.copy()
        weight[:, automaton.blank] = NEG
        s, c = np.nonzero(np.isfinite(weight))                       # row-major: by state, labels ascending
        H = automaton.num_states
        begin = np.zeros(H + 1, np.int64)
        np.cumsum(np.bincount(s, minlength=H), out=begin[1:])
        return cls(begin.astype(np.int32), c.astype(np.int32), np.ascontiguousarray(automaton.next[s, c]), np.ascontiguousarray(weight[s, c]),
                   np.full(H, -1, np.int32), np.zeros(H, np.float32), automaton.final.copy(), automaton.num_classes, blank=automaton.blank)

    def to_dense(self):
        """The LabelAutomaton whose entries are step's float32 results (back-off resolved per state and class); for up to
        LabelAutomaton.MAX_STATES states."""
        H, C = self.num_states, self.num_classes
        if H > LabelAutomaton.MAX_STATES:
            raise ValueError('%d states, a LabelAutomaton holds at most %d' % (H, LabelAutomaton.MAX_STATES))
        nxt = np.zeros((H, C), np.int32)
        weight = np.full((H, C), NEG, np.float32)
        for s in range(H):
            for c in range(C):
                tr = self.step(s, c) if c != self.blank else None
                if tr is not None:
                    weight[s, c], nxt[s, c] = tr
        return LabelAutomaton(nxt, weight, self.final.copy(), blank=self.blank)

    @classmethod
    def from_lexicon(cls, words, num_classes, blank=0):
        """The trie of a word list (label lists over the classes but the blank): weight 0 along its edges, no back-off, final 0 where a word
        ends and -inf elsewhere.  It accepts exactly the words, each with score 0.  Memory follows the number of trie nodes."""
        sorted_words = sorted({tuple(int(c) for c in word) for word in words})
        parents, labels, ends = [], [], [False]
        path, prev = [0], ()                                          # the node of every prefix of the previous word
        for word in sorted_words:
            for c in word:
                if not 0 <= c < num_classes or c == blank:
                    raise ValueError('label %d in a lexicon over %d classes with blank %d' % (c, num_classes, blank))
            keep = 0
            while keep < len(prev) and keep < len(word) and prev[keep] == word[keep]:
                keep += 1
            del path[keep + 1:]
            for c in word[keep:]:
                parents.append(path[-1])
                labels.append(c)
                path.append(len(ends))
                ends.append(False)
            ends[path[-1]] = True
            prev = word
        H, A = len(ends), len(labels)
        parents, labels = np.array(parents, np.int64), np.array(labels, np.int64)
        order = np.lexsort((labels, parents))                         # by parent, labels ascending; node i + 1 hangs under edge i
        begin = np.zeros(H + 1, np.int64)
        np.cumsum(np.bincount(parents, minlength=H), out=begin[1:])
        return cls(begin.astype(np.int32), labels[order].astype(np.int32), (order + 1).astype(np.int32), np.zeros(A, np.float32),
                   np.full(H, -1, np.int32), np.zeros(H, np.float32), np.where(np.array(ends), 0.0, NEG).astype(np.float32), num_classes,
                   blank=blank)

    @classmethod
    def from_backoff_ngram(cls, lm, alpha, beta, blank=0):
        """The shallow fusion of a rescoring.BackoffNGram inside the search, at the size of the model's counts.  States are the contexts the
        model has seen (state 0 the begin context), arcs the seen (context, label) events with weight alpha * log P(c | h) + beta, leading to the
        longest seen suffix of h + c; backoff drops the context's oldest symbol at the price alpha * log lambda(h); the empty context carries an
        arc for every label and no back-off; final[h] = alpha * log P(END | h), resolved here.  Hence score(s) == alpha * lm.log_prob(s) +
        beta * len(s).  The model's labels 1 .. num_classes - 1 are the non-blank classes in ascending order, as in LabelAutomaton.from_ngram."""
        C, order = int(lm.num_classes), int(lm.order)
        if not 0 <= blank < C:
            raise ValueError('blank %d outside the %d classes' % (blank, C))
        if order - 1 > cls.MAX_HOPS:
            raise ValueError('an order-%d model backs off up to %d times (at most %d hops)' % (order, order - 1, cls.MAX_HOPS))
        classes = [k for k in range(C) if k != blank]                 # classes[j] is the class of the model's label j + 1
        start = lm.context(())
        contexts = {ctx for ctx, n in lm.totals.items() if n > 0} | {start, ()}
        states = [start] + sorted(contexts - {start}, key=lambda ctx: (len(ctx), ctx))
        index = {ctx: i for i, ctx in enumerate(states)}

        def longest_seen_suffix(ctx):
            while ctx not in index:
                ctx = ctx[1:]
            return index[ctx]

        begin, labels, nexts, weights = [0], [], [], []
        H = len(states)
        backoff = np.full(H, -1, np.int32)
        backoff_weight = np.zeros(H, np.float32)
        final = np.zeros(H, np.float32)
        for i, ctx in enumerate(states):
            final[i] = alpha * math.log(lm.prob(ctx, lm.END))
            if ctx:
                backoff[i] = longest_seen_suffix(ctx[1:])
                backoff_weight[i] = alpha * math.log(lm.backoff_weight(ctx))
                seen = sorted(sym for sym in lm.counts.get(ctx, ()) if sym != lm.END)
            else:
                seen = range(1, C)
            for lab in seen:
                after = (ctx + (lab,))[-(order - 1):] if order > 1 else ()
                labels.append(classes[lab - 1])
                nexts.append(longest_seen_suffix(after))
                weights.append(alpha * math.log(lm.prob(ctx, lab)) + beta)
            begin.append(len(labels))
        return cls(np.array(begin, np.int32), np.array(labels, np.int32), np.array(nexts, np.int32), np.array(weights, np.float32), backoff,
                   backoff_weight, final, C, blank=blank)
