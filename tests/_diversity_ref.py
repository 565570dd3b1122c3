"""Float64 restatement of the reference's diversity numbers on lists of words, and the corpora the diversity tests share.
Imports nothing from audiocaption_amd/diversity.py.

Self-BLEU restates nltk's PUBLISHED algorithm (nltk.translate.bleu_score: sentence_bleu -> corpus_bleu over one hypothesis,
modified_precision, closest_ref_length, brevity_penalty, SmoothingFunction.method1 with epsilon 0.1) for the call of the
reference's eval/diversity.py:14-31.  It is NOT a run of nltk, which is not available to this project: agreement with
nltk rests on this restatement and on the closed forms worked by hand in tests/test_diversity_cpu.py.  It is the DIRECT
formulation - for every sentence a loop over all the other sentences as references, clipping with Counters - and knows
nothing of the device's table of the two largest counts, so that the two check each other.

  num[n]   sum over the distinct n-grams g of sentence i of min(c_i(g), max_{j != i} c_j(g))
  den[n]   max(1, number of n-grams of sentence i)
  ref_len  min(other lengths, key=lambda r: (abs(r - L_i), r))
  score    0 when num[1] == 0; else bp * exp(fsum(0.25 * log(p[n]))), p[n] = num / den, or 0.1 / den when num == 0,
           bp = 1 when L_i > ref_len else exp(1 - ref_len / L_i)

The richness restates eval/old_diversity.py:10-60 (calc_richness, diversity_evaluate) operation by operation; that script
CAN be run, and tests/golden/make_golden_diversity.py records its values for the corpora below (g25_diversity.npz) and
asserts that this restatement agrees.  The distinct n-gram counts restate eval/diversity.py:49-96 (Distinct-2 divides by
the number of words) and eval/diversity_instance.py:80-92.
"""
import functools
import math
from collections import Counter

import numpy as np

from _cider_ref import END, FIRST_WORD, START, ListVocabulary, _row, row_sentence, word_list

ORDER = 4


def ngrams(words, n):
    return Counter(tuple(words[i:i + n]) for i in range(len(words) - n + 1))


def sentence_self_bleu(i, sentences, counted=None):
    """``(score, [L, ref_len, den[4], num[4]])`` of sentence i against all the others (``counted``: the n-gram Counters of
    every sentence per order, when the caller has them already)."""
    if counted is None:
        counted = [[ngrams(s, n) for n in range(1, ORDER + 1)] for s in sentences]
    refs = [s for j, s in enumerate(sentences) if j != i]
    L = len(sentences[i])
    num, den = [], []
    for n in range(1, ORDER + 1):
        counts = counted[i][n - 1]
        most = {}
        for j in range(len(sentences)):
            if j == i:
                continue
            rc = counted[j][n - 1]
            for g in counts:
                most[g] = max(most.get(g, 0), rc[g])
        num.append(sum(min(c, most[g]) for g, c in counts.items()))
        den.append(max(1, sum(counts.values())))
    ref_len = min((len(r) for r in refs), key=lambda r: (abs(r - L), r))
    stats = [L, ref_len] + den + num
    if num[0] == 0:
        return 0.0, stats
    bp = 1.0 if L > ref_len else math.exp(1 - ref_len / L)
    p = [(0.1 / d) if c == 0 else c / d for c, d in zip(num, den)]
    return bp * math.exp(math.fsum(0.25 * math.log(v) for v in p)), stats


def richness_order(sentences, n):
    """old_diversity.py calc_richness for one order (NaN where the reference divides by zero: no sentence has an n-gram)."""
    count = {}
    for s in sentences:
        for g in set(ngrams(s, n)):
            count[g] = count.get(g, 0) + 1
    freq = {g: c / len(sentences) for g, c in count.items()}
    scores = []
    for s in sentences:
        grams = set(ngrams(s, n))
        if not grams:
            continue
        score = 0
        for g in grams:
            score += np.log(1 / freq[g])
        scores.append(score / len(grams))
    return sum(scores) / len(scores) if scores else float("nan")


def richness(sentences):
    each = [richness_order(sentences, n + 1) for n in range(ORDER)]
    score = 0
    for v in each:
        score += v * (1.0 / ORDER)
    return each, score


def host_results(sentences):
    """What the kernels must return for a corpus of word lists, under the names of ``Diversity.score_ids``."""
    assert len(sentences) >= 2
    counted = [[ngrams(s, n) for n in range(1, ORDER + 1)] for s in sentences]
    scored = [sentence_self_bleu(i, sentences, counted) for i in range(len(sentences))]
    self_bleu = np.array([s for s, _ in scored], dtype=np.float64)
    total = 0.0
    for s, _ in scored:           # diversity.py:24-31: added in order
        total += s
    each, rich = richness(sentences)
    distinct = [len(set(g for s in sentences for g in ngrams(s, n))) for n in range(1, ORDER + 1)]
    return {"self_bleu": self_bleu,
            "stats": np.array([st for _, st in scored], dtype=np.int64),
            "sent_distinct": np.array([[len(ngrams(s, n)) for n in range(1, ORDER + 1)] for s in sentences], dtype=np.int64),
            "totals": np.array([sum(len(s) for s in sentences)] + distinct, dtype=np.int64),
            "summary": np.array([total / len(sentences)] + each + [rich], dtype=np.float64)}


def corpus_numbers(sentences):
    """diversity.py:49-96 / diversity_instance.py:80-92 on word lists: what ``Diversity.compute_score`` reports."""
    res = host_results(sentences)
    words = int(res["totals"][0])
    out = {"vocabulary": int(res["totals"][1]), "distinct_1": int(res["totals"][1]) / words,
           "distinct_2": int(res["totals"][2]) / words, "self_bleu": float(res["summary"][0]),
           "richness": float(res["summary"][5])}
    if all(len(s) >= 2 for s in sentences):
        out["distinct_1_instance"] = float(np.mean([len(set(s)) / len(s) for s in sentences]))
        out["distinct_2_instance"] = float(np.mean([len(ngrams(s, 2)) / (len(s) - 1) for s in sentences]))
    return out


# ---- closed forms, worked by hand -------------------------------------------------------------------------------------------
CLOSED = {
    "captions": (["a dog barks", "a dog barks loudly", "a cat meows", "rain"],
                 [0.5623413251903491, 0.3976353643835253, 0.11362193664674995, 0.0]),
    # the maximum count of "a" is held twice: the owner still sees it
    "tied-maximum": (["a a a b", "a a c", "a a a d"], [0.3976353643835253, 0.17216896116316355, 0.3976353643835253]),
    # the maximum is held once: its owner falls to the second maximum
    "single-maximum": (["a a a b", "a a c", "a d"], [0.16990442448471224, 0.24028114141347542, 0.09069748827745895]),
}
CLOSED_CAPTIONS = {"mean": 0.2683996565551561, "totals": [11, 7, 5],
                   "richness": [0.9323611173034647, 1.0012125941421433, 1.0397207708399179, 1.3862943611198906],
                   "overall": 1.089897210851354}


# ---- the corpora of the tests --------------------------------------------------------------------------------------------
def _case(V, rows, names=None):
    rows = np.asarray(rows, dtype=np.int32)
    vocabulary = ListVocabulary(names or word_list(V))
    return {"vocab_size": V, "vocabulary": vocabulary, "words": rows,
            "sentences": [row_sentence(r, vocabulary.idx2word).split() for r in rows]}


def closed_case(name):
    """A closed-form corpus as word ids (ids in order of first appearance)."""
    table = {}
    sents = [[table.setdefault(w, FIRST_WORD + len(table)) for w in s.split()] for s in CLOSED[name][0]]
    V = FIRST_WORD + len(table)
    T = max(len(s) for s in sents)
    rng = np.random.default_rng(2)
    names = word_list(V)
    for w, i in table.items():
        names[i] = w
    return _case(V, [_row(s, T, rng, V) for s in sents], names)


def edge_case():
    """9 rows, T = 10, vocabulary of 12 ids in which id 9 spells the same word as id 4.  Lengths 0, 1, 2, 3, 4, 4, 7, 8, 10:
    row 0 is empty (<end> first; it scores 0 and its length is the closest to row 1's, tied with 2: the smaller wins, as 2
    wins over 4 for row 3); row 1 starts with <start>, row 3 has one in the middle; rows 1 to 3 are shorter than the order;
    rows 4 and 5 are identical (every count tied); row 6 (7 words, closest other length 8: brevity penalty below 1) has the
    ids 0 and vocab_size - 1 and the word of ids 4 and 9 twice, as often as row 8 (a tied maximum of 2); row 7 (8 words,
    closest 7: no penalty) has ``w6`` six times against once elsewhere (its owner falls to the second maximum) and
    ``w6 w6`` three times against nobody (to 0); row 8 has no <end> and uses all T columns."""
    V = 12
    names = word_list(V)
    names[9] = names[4]
    rows = [[END, 5, 6, 7, 5, 6, 7, 8, 3, 3],
            [START, 5, END, 3, 3, 3, 3, 3, 3, 3],
            [5, 6, END, 7, 7, 7, 7, 7, 7, 7],
            [5, START, 6, 7, END, 8, 8, 8, 8, 8],
            [5, 6, 7, 8, END, 5, 6, 7, 8, 10],
            [5, 6, 7, 8, END, 3, 3, 3, 3, 3],
            [0, 11, 9, 4, 10, 5, 6, END, 6, 6],
            [6, 6, 6, 7, 6, 6, 8, 6, END, 4],
            [10, 4, 3, 3, 3, 10, 4, 3, 5, 6]]
    return _case(V, rows, names)


def random_case(N, max_words, n_words, seed, T=None):
    """N rows of 0 .. max_words words drawn from ``n_words`` words; a row in four begins with <start>."""
    rng = np.random.default_rng(seed)
    V = FIRST_WORD + n_words
    T = T or max_words
    rows = []
    for _ in range(N):
        sent = rng.integers(FIRST_WORD, V, int(rng.integers(0, max_words + 1))).tolist()
        rows.append(_row(sent, T, rng, V, start=rng.random() < 0.25))
    return _case(V, rows)


def long_case():
    """T = 1024: sentences of 70 words (more than one wave), 1024 words (the limit: no <end>, four passes of a workgroup),
    300, 0 and 5 words over 37 words, so that n-grams repeat within and between the sentences."""
    V, T = 40, 1024
    rng = np.random.default_rng(1024)
    rows = [_row(rng.integers(FIRST_WORD, V, L).tolist(), T, rng, V) for L in (70, 1024, 300, 0, 5)]
    return _case(V, rows)


def minimum_case():
    """Two rows of three columns: 6 positions, the table at its minimum size."""
    return _case(6, [[3, 4, 3], [3, END, 5]])


CASES = ["captions", "tied-maximum", "single-maximum", "edge", "crowded", "minimum", "long"]


@functools.lru_cache(maxsize=None)
def make_case(name):
    if name in CLOSED:
        return closed_case(name)
    if name == "crowded":        # 300 sentences over 30 words: almost every n-gram collides with an equal or an unequal one
        return random_case(300, 24, 30, 300)
    return {"edge": edge_case, "minimum": minimum_case, "long": long_case}[name]()


@functools.lru_cache(maxsize=None)
def want(name):
    """The restatement's results for a case: computed once, shared, left unchanged."""
    return host_results(make_case(name)["sentences"])
