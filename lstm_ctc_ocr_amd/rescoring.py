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


class BackoffNGram:
    """Character n-gram with interpolated absolute discounting, written so that it is exactly a back-off model (what
    automaton.SparseLabelAutomaton.from_backoff_ngram compiles to failure arcs).  Vocabulary, END and the BEGIN padding are CharNGram's; V =
    num_classes symbols.  With n(h, c) the count of c after the context h, n(h) its sum over c, N1+(h) the number of symbols seen after h, h'
    the context h without its oldest symbol and D the discount,

        n(h) > 0:  P(c | h) = max(n(h, c) - D, 0) / n(h) + lambda(h) * P(c | h'),   lambda(h) = D * N1+(h) / n(h)
        n(h) = 0:  P(c | h) = P(c | h')
        the empty context interpolates with the uniform 1 / V (and is uniform before anything was fitted).

    Lower-order counts are the marginals of the full-order ones.  For an unseen (h, c) the first term is 0, so P(c | h) = lambda(h) * P(c | h'):
    the failure arc.  P(. | h) sums to 1 over the vocabulary for every context."""

    BEGIN = CharNGram.BEGIN
    END = CharNGram.END

    def __init__(self, order, num_classes, discount=0.75):
        if order < 1:
            raise ValueError('order must be at least 1 (got %r)' % (order,))
        if num_classes < 2:
            raise ValueError('num_classes must be at least 2 (got %r)' % (num_classes,))
        if not 0 < discount < 1:
            raise ValueError('discount must lie in (0, 1) (got %r)' % (discount,))
        self.order, self.num_classes, self.discount = int(order), int(num_classes), float(discount)
        self.vocab = list(range(1, self.num_classes)) + [self.END]
        self.counts = {}                     # context tuple (0 .. order - 1 symbols, BEGIN included) -> {symbol: count}
        self.totals = defaultdict(int)       # context tuple -> n(h)

    _check = CharNGram._check
    _events = CharNGram._events

    def fit(self, strings):
        """Counts the n-grams of a list of label lists (adds to what was counted before).  Returns self."""
        for labels in strings:
            for hist, sym in self._events(self._check(labels)):
                for j in range(len(hist) + 1):
                    ctx = hist[j:]
                    seen = self.counts.setdefault(ctx, {})
                    seen[sym] = seen.get(sym, 0) + 1
                    self.totals[ctx] += 1
        return self

    def context(self, history):
        """The full-order context of a history: its last order - 1 symbols, begin markers where it is shorter."""
        if self.order == 1:
            return ()
        return tuple(([self.BEGIN] * (self.order - 1) + [int(v) for v in history])[-(self.order - 1):])

    def backoff_weight(self, ctx):
        """lambda(ctx); 1 for a context that was never seen."""
        n = self.totals.get(ctx, 0)
        return self.discount * len(self.counts[ctx]) / n if n else 1.0

    def prob(self, ctx, symbol):
        """P(symbol | ctx) for a context of any length up to order - 1."""
        lower = self.prob(ctx[1:], symbol) if ctx else 1.0 / len(self.vocab)
        n = self.totals.get(ctx, 0)
        if not n:
            return lower
        return max(self.counts[ctx].get(symbol, 0) - self.discount, 0.0) / n + self.backoff_weight(ctx) * lower

    def cond_log_prob(self, history, symbol):
        """log P(symbol | history), as CharNGram.cond_log_prob."""
        return math.log(self.prob(self.context(history), symbol))

    def log_prob(self, labels):
        seq = self._check(labels)
        return sum(math.log(self.prob(hist, sym)) for hist, sym in self._events(seq))


def rerank(nbest, lm, alpha, beta):
    """nbest: per sample a list of entries whose first field is the label list and second the log-probability (further fields are carried
    along).  -> the same lists, each re-ordered by  log_prob + alpha * lm.log_prob(labels) + beta * len(labels),  best first; entries of equal
    score keep their input order."""
    out = []
    for entries in nbest:
        scored = [(-(float(e[1]) + (alpha * lm.log_prob(e[0]) if alpha else 0.0) + beta * len(e[0])), i) for i, e in enumerate(entries)]
        out.append([entries[i] for _, i in sorted(scored)])
    return out
