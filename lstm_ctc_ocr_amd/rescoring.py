"""Language-model re-ranking of N-best lists (host only, pure Python; no device work).

The lists are what Engine.decode_nbest_beam (triples: labels, log_prob, log_post) and Engine.decode_nbest (pairs: labels, log-posterior)
return per sample, best first.  `rerank` re-orders each by

    log_prob + alpha * lm.log_prob(labels) + beta * len(labels)

the usual shallow fusion of an acoustic score with a language model (weight alpha) and a length bonus (beta, which offsets the language
model's preference for short strings).  `CharNGram` is a small character n-gram model to go with it; anything with a
log_prob(labels) -> float method serves as `lm`.
"""
import math
from collections import defaultdict


class CharNGram:
    """Add-k smoothed character n-gram over label lists.  The vocabulary is the classes 1 .. num_classes - 1 (0 is the CTC blank and never
    occurs in a decoded string) plus an end marker; a string is padded with order - 1 begin markers, so

        log_prob(s) = sum_i log P(s_i | s_{i-order+1 .. i-1}) + log P(end | last order - 1 symbols)
        P(c | h) = (count(h, c) + add_k) / (count(h) + add_k * V),   V = num_classes  (num_classes - 1 labels and the end marker).

    Over c in the vocabulary P(. | h) sums to 1 for every history h, seen or not."""

    BEGIN = -1
    END = -2

    def __init__(self, order, num_classes, add_k=0.1):
        if order < 1:
            raise ValueError('order must be at least 1 (got %r)' % (order,))
        if num_classes < 2:
            raise ValueError('num_classes must be at least 2 (got %r)' % (num_classes,))
        if not add_k > 0:
            raise ValueError('add_k must be positive (got %r)' % (add_k,))
        self.order, self.num_classes, self.add_k = int(order), int(num_classes), float(add_k)
        self.vocab = list(range(1, self.num_classes)) + [self.END]
        self._ngram = defaultdict(int)       # (history tuple, symbol) -> count
        self._hist = defaultdict(int)        # history tuple -> count

    def _check(self, labels):
        seq = [int(v) for v in labels]
        for v in seq:
            if not 1 <= v < self.num_classes:
                raise ValueError('label %d outside 1 .. %d' % (v, self.num_classes - 1))
        return seq

    def _events(self, seq):
        padded = [self.BEGIN] * (self.order - 1) + seq + [self.END]
        for i in range(self.order - 1, len(padded)):
            yield tuple(padded[i - self.order + 1:i]), padded[i]

    def fit(self, strings):
        """Counts the n-grams of a list of label lists (adds to what was counted before).  Returns self."""
        for labels in strings:
            for hist, sym in self._events(self._check(labels)):
                self._ngram[(hist, sym)] += 1
                self._hist[hist] += 1
        return self

    def cond_log_prob(self, history, symbol):
        """log P(symbol | history): history a sequence of the preceding symbols (its last order - 1 are used, begin markers are added where it
        is shorter), symbol a label or CharNGram.END."""
        hist = tuple(([self.BEGIN] * (self.order - 1) + [int(v) for v in history])[len(history):]) if self.order > 1 else ()
        num = self._ngram.get((hist, symbol), 0) + self.add_k
        den = self._hist.get(hist, 0) + self.add_k * len(self.vocab)
        return math.log(num / den)

    def log_prob(self, labels):
        seq = self._check(labels)
        total = 0.0
        for hist, sym in self._events(seq):
            total += math.log((self._ngram.get((hist, sym), 0) + self.add_k) / (self._hist.get(hist, 0) + self.add_k * len(self.vocab)))
        return total


def rerank(nbest, lm, alpha, beta):
    """nbest: per sample a list of entries whose first field is the label list and second the log-probability (further fields are carried
    along).  -> the same lists, each re-ordered by  log_prob + alpha * lm.log_prob(labels) + beta * len(labels),  best first; entries of equal
    score keep their input order."""
    out = []
    for entries in nbest:
        scored = [(-(float(e[1]) + (alpha * lm.log_prob(e[0]) if alpha else 0.0) + beta * len(e[0])), i) for i, e in enumerate(entries)]
        out.append([entries[i] for _, i in sorted(scored)])
    return out
