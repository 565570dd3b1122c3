"""Float64 restatement of BLEU (pycocoevalcap's bleu_scorer.py, option "closest") and ROUGE-L (rouge.py, beta = 1.2) on
strings with plain dictionaries and lists, and the batches the tests of the built-in scorers share.  Written from the
published arithmetic, independently of audiocaption_amd/caption_metrics.py; imports nothing from the package.
pycocoevalcap itself is not available to this project: agreement with it rests on this restatement and on the closed-form
answers of tests/test_caption_metrics_cpu.py.

  BLEU, per key     testlen = words of the hypothesis, guess[k] = max(0, testlen - k),
                    correct[k] = sum over distinct hypothesis (k+1)-grams g of min(count_h(g), max_r count_r(g)),
                    reflen = the reference length closest to testlen, the smaller of two equally close
  score             b_k = prod_{j <= k} (correct[j] + 1e-15) / (guess[j] + 1e-9), bleu_k = b_k ** (1 / (k + 1)),
                    times exp(1 - 1 / ratio) when ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1
  corpus            the same on the four sums over the keys
  ROUGE-L, per key  p = max_r lcs(h, r) / len(h), r = max_r lcs(h, r) / len(r),
                    (1 + beta^2) p r / (r + beta^2 p) when both are non-zero, else 0

Sentences are split on whitespace (rouge.py splits on single spaces: the empty hypothesis is the one difference, 0 here).
"""
import math

import numpy as np

from _cider_ref import END, FIRST_WORD, START, ListVocabulary, _row, row_sentence, word_list

TINY, SMALL, BETA = 1e-15, 1e-9, 1.2


# ---- BLEU ------------------------------------------------------------------------------------------------------------------
def ngram_counts(words, n):
    out = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            out[g] = out.get(g, 0) + 1
    return out


def bleu_stats(hyp, refs, n=4):
    """``(testlen, reflen, guess[n], correct[n])`` of one hypothesis sentence against its reference sentences."""
    h = hyp.split()
    testlen = len(h)
    lens = [len(r.split()) for r in refs]
    reflen = min((abs(l - testlen), l) for l in lens)[1]
    most = {}
    for r in refs:
        for g, c in ngram_counts(r.split(), n).items():
            most[g] = max(most.get(g, 0), c)
    correct = [0] * n
    for g, c in ngram_counts(h, n).items():
        correct[len(g) - 1] += min(c, most.get(g, 0))
    return testlen, reflen, [max(0, testlen - k) for k in range(n)], correct


def bleu_from_stats(testlen, reflen, guess, correct):
    out = []
    b = 1.0
    for k in range(len(guess)):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [v * math.exp(1 - 1 / ratio) for v in out]
    return out


def bleu_score(references, hypothesis, n=4):
    """pycocoevalcap's contract: ``([n corpus scores], [n lists of per-key scores])`` in references' key order, and the
    per-key stats as a third item."""
    stats, per_key = [], [[] for _ in range(n)]
    for key, refs in references.items():
        assert len(hypothesis[key]) == 1 and len(refs) > 0
        st = bleu_stats(hypothesis[key][0], refs, n)
        stats.append(st)
        for k, v in enumerate(bleu_from_stats(*st)):
            per_key[k].append(v)
    total = (sum(s[0] for s in stats), sum(s[1] for s in stats),
             [sum(s[2][k] for s in stats) for k in range(n)], [sum(s[3][k] for s in stats) for k in range(n)])
    return bleu_from_stats(*total), per_key, stats


# ---- ROUGE-L ---------------------------------------------------------------------------------------------------------------
def lcs(a, b):
    """Length of the longest common subsequence of two lists: the full table, row by row."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def rouge_key(hyp, refs):
    """``(score, [lcs with each reference])`` of one hypothesis sentence."""
    h = hyp.split()
    each = [lcs(h, r.split()) for r in refs]
    if not h:
        return 0.0, each
    prec = max(l / float(len(h)) for l in each)
    rec = max(l / float(len(r.split())) for l, r in zip(each, refs))
    if prec != 0 and rec != 0:
        return ((1 + BETA ** 2) * prec * rec) / float(rec + BETA ** 2 * prec), each
    return 0.0, each


def rouge_score(references, hypothesis):
    """``(mean, float64 array per key)`` in references' key order, and the LCS lengths per key as a third item."""
    scores, each = [], []
    for key, refs in references.items():
        assert len(hypothesis[key]) == 1 and len(refs) > 0
        s, l = rouge_key(hypothesis[key][0], refs)
        scores.append(s)
        each.append(l)
    return float(np.mean(scores)), np.array(scores, dtype=np.float64), each


class BleuScorer:
    def __init__(self, n=4):
        self.n = n

    def method(self):
        return "Bleu"

    def compute_score(self, references, hypothesis):
        return bleu_score(references, hypothesis, self.n)[:2]


class RougeScorer:
    def method(self):
        return "Rouge"

    def compute_score(self, references, hypothesis):
        return rouge_score(references, hypothesis)[:2]


# ---- closed forms (computed on the CPU from the arithmetic above) --------------------------------------------------------
# (hypothesis, references, stats, BLEU-1..4)
BLEU_CLOSED = [
    ("the the the the the the the", ["the cat is on the mat", "there is a cat on the mat"],
     (7, 7, [7, 6, 5, 4], [2, 0, 0, 0]), [0.285714286, 6.90065559e-09, None, 1.24218899e-12]),
    ("a", ["a"], (1, 1, [1, 0, 0, 0], [1, 0, 0, 0]), [0.999999998, 0.000999999999, 9.99999999e-05, 3.16227766e-05]),
    ("", ["a b c"], (0, 3, [0, 0, 0, 0], [0, 0, 0, 0]), [0.0, 0.0, 0.0, 0.0]),
    ("a b c d e", ["a b c d", "a b c d e f"], (5, 4, [5, 4, 3, 2], [5, 4, 3, 2]), [1.0, 1.0, 1.0, 1.0]),
    ("a b c", ["a b c d e f"], (3, 6, [3, 2, 1, 0], [3, 2, 1, 0]), [0.367879441, 0.367879441, 0.367879441, 0.0116333694]),
    ("a b c d e", ["a b c d e"], (5, 5, [5, 4, 3, 2], [5, 4, 3, 2]), [1.0, 1.0, 1.0, 1.0]),
]
BLEU_CLOSED_CORPUS = (21, 26, [0.600478193, 0.543859732, 0.514235891, 0.481131097])
# (hypothesis, references, ROUGE-L)
ROUGE_CLOSED = [
    ("a b c", ["a b c d e f"], 0.628865979),
    ("a b c d", ["a x c d"], 0.75),
    ("a b c d e f", ["a b c x y z w v", "q f"], 0.5),     # precision from the first reference, recall from the second
    ("", ["a b c"], 0.0),
    ("a b c", ["d e f", "g"], 0.0),
]


def close(got, want):
    """A closed form above is given to nine significant digits."""
    return abs(got - want) <= 1e-12 + 6e-9 * abs(want)


# ---- the batches -----------------------------------------------------------------------------------------------------------
def host_results(case, which, n=4):
    """What both scorers must return for hypothesis set ``which`` of a batch, straight from the definitions: the sentence
    of the first row of each key scored by the restatement and handed to every row of that key.  ``stats`` (K, 2 + 2 n)
    and ``lcs`` (M,) follow the distinct keys in order of first appearance, the references of a key in their order."""
    idx2word = case["vocabulary"].idx2word
    hypothesis, references = {}, {}
    for row, key in zip(case["words"][which], case["keys"]):
        if key not in hypothesis:
            hypothesis[key] = [row_sentence(row, idx2word)]
            references[key] = case["key2refs"][key]
    corpus, per_key, stats = bleu_score(references, hypothesis, n)
    mean, rouge, each = rouge_score(references, hypothesis)
    at = {key: i for i, key in enumerate(references)}
    rows = [at[key] for key in case["keys"]]
    return {"references": references, "hypothesis": hypothesis,
            "stats": np.array([[s[0], s[1]] + s[2] + s[3] for s in stats], dtype=np.int64),
            "bleu": np.array(per_key, dtype=np.float64)[:, rows], "corpus": np.array(corpus, dtype=np.float64),
            "lcs": np.array([l for ls in each for l in ls], dtype=np.int64),
            "rouge": rouge[rows], "mean": mean}


def _sentence(ids):
    return " ".join("zebra" if i < 0 else f"w{i}" for i in ids)     # (a word outside every vocabulary)


def _case(V, keys, id_refs, sets, names=None):
    return {"vocab_size": V, "vocabulary": ListVocabulary(names or word_list(V)), "keys": keys,
            "key2refs": {k: [_sentence(r) for r in refs] for k, refs in id_refs.items()},
            "words": [np.asarray(rows, dtype=np.int32) for rows in sets]}


def edge_case():
    """6 rows over 5 keys (``a`` twice), T = 8, vocabulary of 12 ids in which id 9 spells the same word as id 4.
    Hypothesis lengths 0 (<end> first), 1, 3 (shorter than the order) and 8 without <end>; a <start> in the middle of a
    row; 1 to 7 references of 1 to 70 words; one reference word outside the vocabulary; the second row of ``a`` differs
    from the first and must not count.  Key ``d``: the hypothesis has ``w6`` six times against three, one and three in
    its references, and the bigram ``w6 w6`` three times against none, none and two, while ``w6 w7`` and ``w6 w8`` occur
    in the first reference only - the clip is a maximum over references that differ; its reference lengths 6 and 10 are
    equally far from 8 (reflen 6).  Key ``e``: precision from one reference, recall from another; a hypothesis longer
    than every reference (ratio above 1).  Key ``c``, set 0: three words against a closest reference of three (ratio at
    1 but for the two constants); keys ``a`` and ``b``: ratio below 1."""
    V = 12
    names = word_list(V)
    names[9] = names[4]
    long70 = [3 + (i * i + i // 7) % 9 for i in range(70)]
    id_refs = {
        "a": [[5, 6, 7, 5, 6, 7, 8, 11, 3, 4, 5, 6, 10, 10, 3, 8, 7, 6, 5, 11]],
        "b": [[3], long70],
        "c": [[5], [5, 4], [5, 4, 11], [5, -1, 4, 11], [10, 5, 4, 11, 3, 3, 3, 5, 4, 11, 6, 7, 8, 10, 10, 4, 5, 4, 11, 6],
              [11, 4, 5], [4, 4, 4, 4, 4, 4, 4]],
        "d": [[6, 7, 6, 8, 10, 6], [6, 7, 8], [8, 6, 6, 6, 3, 7, 3, 3, 3, 3]],
        "e": [[5, 6, 7, 10, 10, 10, 10], [3, 8]],
    }
    keys = ["a", "b", "c", "a", "d", "e"]
    sampled = [[END, 5, 6, 7, 5, 6, 7, 8],            # empty: everything after <end> is ignored
               [START, long70[0], END, 3, 3, 3, 3, 3],    # one word
               [5, START, 9, 11, END, 7, 7, 7],       # three words, <start> in the middle, id 9 = the word of id 4
               [5, 6, 7, 5, 6, 7, 8, 11],             # second row of key a: not scored
               [6, 6, 6, 7, 6, 6, 8, 6],              # eight words, no <end>, repeats beyond any one reference's counts
               [5, 6, 7, 4, 4, 8, 4, 4]]
    greedy = [[5, 6, 7, END, 0, 0, 0, 0],
              long70[10:18],
              [END, END, END, END, END, END, END, END],
              [END, 0, 0, 0, 0, 0, 0, 0],
              [START, START, 8, 6, END, 6, 6, 6],
              [3, 8, END, 5, 6, 7, 10, 10]]
    return _case(V, keys, id_refs, [sampled, greedy], names)


def closed_case():
    """The closed forms as a batch of word ids: one row per BLEU case, then one per ROUGE-L case; both sets alike."""
    table = {}
    ids = lambda s: [table.setdefault(w, FIRST_WORD + len(table)) for w in s.split()]
    rows, refs = [], {}
    for i, item in enumerate(BLEU_CLOSED + ROUGE_CLOSED):
        rows.append(ids(item[0]))
        refs[f"k{i}"] = [ids(r) for r in item[1]]
    V = FIRST_WORD + len(table)
    T = max(len(r) for r in rows)
    rng = np.random.default_rng(1)
    rows = [_row(r, T, rng, V) for r in rows]
    names = word_list(V)
    for w, i in table.items():
        names[i] = w
    case = _case(V, list(refs), refs, [rows, rows], names)
    case["key2refs"] = {k: [" ".join(names[i] for i in r) for r in rs] for k, rs in refs.items()}
    return case


def _mutate(sent, rng, word, drop=0.15, swap=0.15):
    out = []
    for w in sent:
        u = rng.random()
        if u < drop:
            continue
        out.append(word() if u < drop + swap else w)
    return out or [word()]


def random_case(vocab_size, n_keys, n_rows, T, seed, max_refs=5, max_ref_words=25):
    """``n_rows`` rows over ``n_keys`` keys (every key at least once, the rest repeats), 1 .. max_refs references of
    1 .. max_ref_words words per key.  Two hypothesis sets; in each, a row is with equal chance random words (0 .. T of
    them) or a reference of its key with words replaced or dropped; a row in four begins with <start>."""
    rng = np.random.default_rng(seed)
    word = lambda: int(rng.integers(FIRST_WORD, vocab_size))
    names = [f"clip{j}" for j in range(n_keys)]
    keys = names + [names[int(j)] for j in rng.integers(0, n_keys, n_rows - n_keys)]
    keys = [keys[int(j)] for j in rng.permutation(n_rows)]
    id_refs = {name: [[word() for _ in range(int(rng.integers(1, max_ref_words + 1)))]
                      for _ in range(int(rng.integers(1, max_refs + 1)))] for name in names}
    sets = []
    for _ in range(2):
        rows = []
        for key in keys:
            if rng.random() < 0.5:
                sent = [word() for _ in range(int(rng.integers(0, T + 1)))]
            else:
                sent = _mutate(id_refs[key][int(rng.integers(0, len(id_refs[key])))], rng, word)
            rows.append(_row(sent, T, rng, vocab_size, start=rng.random() < 0.25))
        sets.append(rows)
    return _case(vocab_size, keys, id_refs, sets)


LONG_LENGTHS = ([63, 64, 65, 129, 300, 290, 128], [65, 63, 300, 64, 0, 129, 192])
LONG_REFS = [1, 7, 3, 2, 4, 3, 2]


def long_case():
    """T = 300, 7 keys and 8 rows, a vocabulary of 40 ids (n-grams repeat).  Hypothesis lengths on both sides of the 64
    positions of a machine word and of the 256 threads of a workgroup: ``LONG_LENGTHS`` per set; 1 to 7 references per
    key, each a hypothesis of one of the sets with words dropped and replaced, cut or extended with random words to
    between 40 and 350 words (the last reference of key 4 has 350)."""
    V, T = 40, 300
    rng = np.random.default_rng(304)
    word = lambda: int(rng.integers(FIRST_WORD, V))
    names = [f"clip{j}" for j in range(len(LONG_REFS))]
    hyps = [[[word() for _ in range(L)] for L in lens] for lens in LONG_LENGTHS]
    id_refs = {}
    for j, name in enumerate(names):
        refs = []
        for i in range(LONG_REFS[j]):
            r = _mutate(hyps[i % 2][j] or hyps[0][j], rng, word)
            want = int(rng.integers(40, 351))
            r = r[:want] if i % 3 == 2 else r + [word() for _ in range(max(0, want - len(r)) if i % 3 == 1 else 0)]
            refs.append(r)
        id_refs[name] = refs
    id_refs[names[4]][-1] = (id_refs[names[4]][-1] + [word() for _ in range(350)])[:350]
    keys = names + [names[3]]
    sets = [[_row(h, T, rng, V, start=j in (1, 5)) for j, h in enumerate(hs + [hs[0]])] for hs in hyps]
    return _case(V, keys, id_refs, sets)


# (vocab_size, keys, rows, T, seed[, max_refs, max_ref_words])
RANDOM_CASES = {"small": (12, 7, 7, 20, 101), "repeated-keys": (30, 33, 40, 20, 202, 7)}
CASES = ["edge", "closed", "long"] + sorted(RANDOM_CASES)


def make_case(name):
    if name in RANDOM_CASES:
        return random_case(*RANDOM_CASES[name])
    return {"edge": edge_case, "closed": closed_case, "long": long_case}[name]()
