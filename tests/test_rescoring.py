"""lstm_ctc_ocr_amd.rescoring: the character n-gram and the N-best re-ranking (host only)."""
import math

import pytest

from lstm_ctc_ocr_amd.rescoring import CharNGram, rerank

CORPUS = [[1, 2, 3], [1, 2, 2, 4], [3, 1, 2], [2], [], [4, 4, 1, 2, 3]]


@pytest.mark.parametrize("order", [1, 2, 3])
def test_next_symbol_probabilities_sum_to_one(order):
    lm = CharNGram(order, 5, add_k=0.3).fit(CORPUS)
    for history in ([], [1], [1, 2], [4, 4, 1], [3, 3, 3]):            # seen and unseen histories, shorter and longer than the order
        total = sum(math.exp(lm.cond_log_prob(history, c)) for c in lm.vocab)
        assert abs(total - 1.0) < 1e-12, (order, history, total)
    assert len(lm.vocab) == 5 and 0 not in lm.vocab and CharNGram.END in lm.vocab


def test_string_probabilities():
    """A unigram by hand: 16 labels and 6 end markers counted; and with the end marker the strings of every length share one unit of mass."""
    lm = CharNGram(1, 5, add_k=1.0).fit(CORPUS)
    counts = {1: 4, 2: 6, 3: 3, 4: 3, CharNGram.END: 6}
    p = {c: (v + 1.0) / (22 + 5.0) for c, v in counts.items()}
    assert abs(lm.log_prob([1, 2]) - math.log(p[1] * p[2] * p[CharNGram.END])) < 1e-12
    assert abs(lm.log_prob([]) - math.log(p[CharNGram.END])) < 1e-12
    small = CharNGram(2, 3, add_k=0.5).fit([[1, 2], [2, 2, 1]])

    def mass(prefix, depth):
        total = math.exp(small.log_prob(prefix))
        return total + (sum(mass(prefix + [c], depth - 1) for c in (1, 2)) if depth else 0.0)
    assert mass([], 4) < mass([], 10) <= 1.0 + 1e-12
    with pytest.raises(ValueError):
        lm.log_prob([0])
    with pytest.raises(ValueError):
        lm.fit([[5]])
    with pytest.raises(ValueError):
        CharNGram(0, 5)


def test_rerank_with_zero_weights_is_the_identity():
    lm = CharNGram(2, 5).fit(CORPUS)
    nbest = [[([1, 2], -0.1, -0.2), ([1], -0.7, -0.8), ([1, 2, 3], -2.0, -2.1)], [], [([], -0.5, 0.0)]]
    assert rerank(nbest, lm, 0.0, 0.0) == nbest
    pairs = [[([3], -0.3), ([4], -1.5)]]                                # decode_nbest's (labels, log-posterior) pairs
    assert rerank(pairs, lm, 0.0, 0.0) == pairs


def test_a_bigram_that_forbids_the_top_string_flips_the_list():
    lm = CharNGram(2, 5, add_k=1e-6).fit([[1, 2, 3]] * 50)              # 1 -> 2 -> 3 always; 1 -> 3 never
    nbest = [[([1, 3, 3], -0.2, -0.3), ([1, 2, 3], -1.6, -1.7)]]
    assert lm.log_prob([1, 2, 3]) > -1e-3 and lm.log_prob([1, 3, 3]) < -10
    out = rerank(nbest, lm, 1.0, 0.0)
    assert [e[0] for e in out[0]] == [[1, 2, 3], [1, 3, 3]]
    assert out[0][0] == nbest[0][1]                                     # entries travel whole
    assert rerank(nbest, lm, 0.01, 0.0) == nbest                        # a weak model leaves the order
    # the length bonus alone: one more label is worth beta
    two = [[([1], -1.0, 0.0), ([1, 2], -1.5, 0.0)]]
    assert rerank(two, lm, 0.0, 0.4) == two
    assert [e[0] for e in rerank(two, lm, 0.0, 0.6)[0]] == [[1, 2], [1]]


def test_ties_keep_their_input_order():
    class Flat:
        def log_prob(self, labels):
            return -1.0
    nbest = [[([2], -1.0, 'a'), ([1], -1.0, 'b'), ([3], -0.5, 'c'), ([4], -1.0, 'd')]]
    out = rerank(nbest, Flat(), 2.0, 0.0)
    assert [e[2] for e in out[0]] == ['c', 'a', 'b', 'd']
    assert [e[2] for e in rerank(out, Flat(), 2.0, 0.0)[0]] == ['c', 'a', 'b', 'd']
