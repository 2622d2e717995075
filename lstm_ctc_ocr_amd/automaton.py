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
