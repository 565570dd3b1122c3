"""Float64 restatement of CIDEr-D as pycocoevalcap's cider_scorer.py computes it (n = 4, sigma = 6, document frequencies
from the scored references), on strings with plain dictionaries, and the batches the CIDEr tests share.  Written from the
published arithmetic, independently of audiocaption_amd/cider.py; imports nothing from it.  pycocoevalcap itself is not
available to this project: agreement with it rests on this restatement and on the closed-form answers of
tests/test_cider_cpu.py.

  counts(sentence)     n-gram (tuple of words) -> occurrences, n = 1 .. 4, over sentence.split()
  df[g]                keys with g in at least one of their references (hypotheses do not count)
  vec[n][g]            tf(g) * (log(keys) - log(max(1, df[g]))), norm[n] = |vec[n]|, length = max(words - 1, 0)
  sim(h, r)[n]         sum_{g in h} min(vec_h[n][g], vec_r[n][g]) * vec_r[n][g], / (norm_h[n] norm_r[n]) if both non-zero,
                       * exp(-(length_h - length_r)^2 / (2 sigma^2))
  score(key)           10 * mean_n(sum_refs sim[n]) / refs
"""
import math

import numpy as np

PAD, START, END = 0, 1, 2
FIRST_WORD = 3


def counts(sentence, n=4):
    words = sentence.split()
    out = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            out[g] = out.get(g, 0) + 1
    return out, max(len(words) - 1, 0)


def document_frequency(references, n=4):
    df = {}
    for refs in references.values():
        seen = set()
        for r in refs:
            seen.update(counts(r, n)[0])
        for g in seen:
            df[g] = df.get(g, 0) + 1
    return df


def vector(cnt, df, ref_len, n=4):
    vec = [{} for _ in range(n)]
    norm = [0.0] * n
    for g, tf in cnt.items():
        k = len(g) - 1
        vec[k][g] = float(tf) * (ref_len - math.log(max(1.0, float(df.get(g, 0)))))
        norm[k] += vec[k][g] ** 2
    return vec, [math.sqrt(v) for v in norm]


def similarity(vec_h, vec_r, norm_h, norm_r, len_h, len_r, n=4, sigma=6.0):
    delta = float(len_h - len_r)
    val = [0.0] * n
    for k in range(n):
        for g, v in vec_h[k].items():
            r = vec_r[k].get(g, 0.0)
            val[k] += min(v, r) * r
        if norm_h[k] != 0 and norm_r[k] != 0:
            val[k] /= norm_h[k] * norm_r[k]
        val[k] *= math.exp(-(delta ** 2) / (2 * sigma ** 2))
    return val


def compute_score(references, hypothesis, n=4, sigma=6.0):
    """pycocoevalcap's contract: ``{key: [ref, ...]}``, ``{key: [hyp]}`` -> (mean, float64 array in references' key order)."""
    df = document_frequency(references, n)
    ref_len = math.log(float(len(references)))
    scores = []
    for key, refs in references.items():
        assert len(hypothesis[key]) == 1 and len(refs) > 0
        cnt_h, len_h = counts(hypothesis[key][0], n)
        vec_h, norm_h = vector(cnt_h, df, ref_len, n)
        total = [0.0] * n
        for r in refs:
            cnt_r, len_r = counts(r, n)
            vec_r, norm_r = vector(cnt_r, df, ref_len, n)
            for k, v in enumerate(similarity(vec_h, vec_r, norm_h, norm_r, len_h, len_r, n, sigma)):
                total[k] += v
        scores.append(10.0 * (sum(total) / n) / len(refs))
    return float(np.mean(scores)), np.array(scores, dtype=np.float64)


class Scorer:
    """The restatement as a scorer object for the host route of ``compute_batch_score``."""

    def method(self):
        return "CIDEr"

    def compute_score(self, references, hypothesis):
        return compute_score(references, hypothesis)


# ---- what the tests share: vocabularies, the sentence of a row, the batches ------------------------------------------
class ListVocabulary:
    """``idx2word[i]`` for i < len(words), nothing else (what the reference's Vocabulary is read for)."""

    def __init__(self, words):
        self.idx2word = list(words)


def word_list(vocab_size):
    return ["<pad>", "<start>", "<end>"] + [f"w{i}" for i in range(FIRST_WORD, vocab_size)]


def row_sentence(row, idx2word):
    """model_util.py:117-164: <start> skipped, cut at the first <end>."""
    words = []
    for w in np.asarray(row).tolist():
        if w == END:
            break
        if w != START:
            words.append(idx2word[w])
    return " ".join(words)


def host_scores(case, which):
    """Float64 scores (N,) of hypothesis set ``which`` of a batch, straight from the definition: the sentence of the first
    row of each key, scored by the restatement, handed to every row of that key."""
    idx2word = case["vocabulary"].idx2word
    hypothesis, references = {}, {}
    for row, key in zip(case["words"][which], case["keys"]):
        if key not in hypothesis:
            hypothesis[key] = [row_sentence(row, idx2word)]
            references[key] = case["key2refs"][key]
    _, per_key = compute_score(references, hypothesis)
    by_key = dict(zip(references.keys(), per_key))
    return np.array([by_key[key] for key in case["keys"]], dtype=np.float64), references, hypothesis


def _row(words, T, rng, vocab_size, start=False):
    """A decoder row of length T: [<start>] words [<end> and then arbitrary words that must not count]."""
    toks = ([START] if start else []) + list(words)
    toks = toks[:T]
    if len(toks) < T:
        toks.append(END)
        toks += rng.integers(FIRST_WORD, vocab_size, T - len(toks)).tolist()
    return toks


def random_case(vocab_size, n_keys, n_rows, T, seed, max_refs=5, max_ref_words=25):
    """``n_rows`` rows over ``n_keys`` keys (every key at least once, the rest repeats), 1 .. max_refs references of
    0 .. max_ref_words words per key, the first reference of every key containing the word ``w3`` (an n-gram in every key:
    df == keys).  Two hypothesis sets; in each, a row is with equal chance random words (0 .. T of them) or a reference
    of its key with words replaced or dropped; a row in four begins with <start>."""
    rng = np.random.default_rng(seed)
    word = lambda: int(rng.integers(FIRST_WORD, vocab_size))
    names = [f"clip{j}" for j in range(n_keys)]
    keys = names + [names[int(j)] for j in rng.integers(0, n_keys, n_rows - n_keys)]
    keys = [keys[int(j)] for j in rng.permutation(n_rows)]
    id_refs = {}
    for name in names:
        refs = [[word() for _ in range(int(rng.integers(0, max_ref_words + 1)))] for _ in range(int(rng.integers(1, max_refs + 1)))]
        refs[0].insert(int(rng.integers(0, len(refs[0]) + 1)), FIRST_WORD)
        id_refs[name] = refs
    words = []
    for _ in range(2):
        rows = []
        for key in keys:
            if rng.random() < 0.5:
                sent = [word() for _ in range(int(rng.integers(0, T + 1)))]
            else:
                ref = id_refs[key][int(rng.integers(0, len(id_refs[key])))]
                sent = []
                for w in ref:
                    u = rng.random()
                    if u < 0.15:
                        continue
                    sent.append(word() if u < 0.3 else w)
            rows.append(_row(sent, T, rng, vocab_size, start=rng.random() < 0.25))
        words.append(np.asarray(rows, dtype=np.int32))
    key2refs = {k: [" ".join(f"w{w}" for w in r) for r in refs] for k, refs in id_refs.items()}
    return {"vocab_size": vocab_size, "vocabulary": ListVocabulary(word_list(vocab_size)), "keys": keys, "key2refs": key2refs,
            "words": words}


# (vocab_size, keys, rows, T, seed[, max_refs, max_ref_words]); "long": sentences beyond one pass of a 256-thread workgroup
RANDOM_CASES = {"small": (12, 7, 7, 20, 101), "repeated-keys": (30, 33, 40, 20, 202), "long": (40, 4, 5, 300, 304, 3, 400)}


def limit_case(max_hyp_words, max_ref_words, seed=405):
    """4 rows over 3 keys (``full`` twice) with T = max_hyp_words, vocabulary of 40 ids (n-grams repeat).  Key ``full`` has
    one reference of exactly max_ref_words words and an ordinary one; ``plain0`` and ``plain1`` have ordinary references.
    Rows of exactly T words (no <start>, no <end>: the row is the sentence): for ``full`` the long reference with three
    words in ten replaced (set 0) and random words (set 1), for ``plain0`` random words (set 0), for ``plain1`` its first
    reference over and over (set 1: counts far beyond the reference's).  The other rows are ordinary; the second row of
    ``full`` differs from the first and must not count."""
    V = 40
    rng = np.random.default_rng(seed)
    word = lambda: int(rng.integers(FIRST_WORD, V))
    some = lambda n: [word() for _ in range(n)]
    long_ref = some(max_ref_words)
    id_refs = {"plain0": [some(9), some(12), some(8)], "full": [long_ref, some(12)], "plain1": [some(11), some(10)]}
    keys = ["plain0", "full", "plain1", "full"]
    T = max_hyp_words
    near_long = [word() if rng.random() < 0.3 else long_ref[i % max_ref_words] for i in range(T)]
    tiled = [id_refs["plain1"][0][i % 11] for i in range(T)]
    sets = [[some(T), near_long, _row(id_refs["plain1"][1][:7] + some(2), T, rng, V), some(T)],
            [_row(id_refs["plain0"][1][2:], T, rng, V, start=True), some(T), tiled, _row(some(5), T, rng, V)]]
    key2refs = {k: [" ".join(f"w{w}" for w in r) for r in refs] for k, refs in id_refs.items()}
    return {"vocab_size": V, "vocabulary": ListVocabulary(word_list(V)), "keys": keys, "key2refs": key2refs,
            "words": [np.asarray(rows, dtype=np.int32) for rows in sets]}


def edge_case():
    """5 rows over 4 keys (``a`` twice), T = 8, vocabulary of 12 ids in which id 9 spells the same word as id 4.
    Hypothesis lengths 0 (<end> first), 1, 3 and 8 without <end>; a <start> in the middle of a row; repeated words on both
    sides (clipping); 1 to 5 references of 0, 1, 2, 3, 4, 20 and 70 words; one reference word outside the vocabulary; the
    word vocab_size - 1; the second row of ``a`` differs from the first and must not count."""
    V = 12
    names = word_list(V)
    names[9] = names[4]
    w = lambda *ids: " ".join("zebra" if i < 0 else f"w{4 if i == 9 else i}" for i in ids)
    long70 = [3 + (i * i + i // 7) % 9 for i in range(70)]
    key2refs = {
        "a": [w(5, 6, 7, 5, 6, 7, 8, 11, 3, 4, 5, 6, 10, 10, 3, 8, 7, 6, 5, 11)],
        "b": ["", w(*long70)],
        "c": [w(5), w(5, 4), w(5, 4, 11), w(5, -1, 4, 11), w(10, 5, 4, 11, 3, 3, 3, 5, 4, 11, 6, 7, 8, 10, 10, 4, 5, 4, 11, 6)],
        "d": [w(6, 6, 7, 6), w(6, 7, 8), w(8, 6, 6, 6, 6, 7)],
    }
    keys = ["a", "b", "c", "a", "d"]
    sampled = [[END, 5, 6, 7, 5, 6, 7, 8],           # empty: everything after <end> is ignored
               [START, long70[0], END, 3, 3, 3, 3, 3],   # one word
               [5, START, 9, 11, END, 7, 7, 7],      # three words, <start> in the middle, id 9 = the word of id 4
               [5, 6, 7, 5, 6, 7, 8, 11],            # second row of key a: not scored
               [6, 6, 6, 7, 6, 6, 8, 6]]             # eight words, no <end>, repeats beyond the references' counts
    greedy = [[5, 6, 7, END, 0, 0, 0, 0],
              long70[10:18],
              [END, END, END, END, END, END, END, END],
              [END, 0, 0, 0, 0, 0, 0, 0],
              [START, START, 8, 6, END, 6, 6, 6]]
    return {"vocab_size": V, "vocabulary": ListVocabulary(names), "keys": keys, "key2refs": key2refs,
            "words": [np.asarray(sampled, dtype=np.int32), np.asarray(greedy, dtype=np.int32)]}
