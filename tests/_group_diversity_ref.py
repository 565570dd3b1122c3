"""Diversity WITHIN groups on lists of words, for the tests of ``ac_diversity_group_scores`` / ``Diversity.score_groups``: the
functions of tests/_diversity_ref.py (the direct float64 restatement of nltk's sentence_bleu against all the other
sentences) applied inside each group, so a group is scored exactly as if it were a corpus of its own.  Imports nothing
from audiocaption_amd/diversity.py.

mBLEU-k of a sentence is nltk's ``sentence_bleu(the group's other sentences, sentence, weights=(1/k,) * k, method1)``: the
same ``num`` / ``den`` / ``ref_len`` as Self-BLEU (``_diversity_ref.sentence_self_bleu``'s ``stats``), the orders above k left
out: 0 when num[1] == 0, else bp * exp(fsum((1 / k) * log(p[n]) for n <= k)).  ``bleu_k(stats, 4)`` is Self-BLEU; ``group_results``
asserts that it reproduces ``sentence_self_bleu``'s score bit for bit.
"""
import math

import numpy as np

import _diversity_ref as D


def bleu_k(stats, k):
    L, ref_len = stats[0], stats[1]
    den, num = stats[2:2 + D.ORDER], stats[2 + D.ORDER:2 + 2 * D.ORDER]
    if num[0] == 0:
        return 0.0
    bp = 1.0 if L > ref_len else math.exp(1 - ref_len / L)
    p = [(0.1 / d) if c == 0 else c / d for c, d in zip(num[:k], den[:k])]
    return bp * math.exp(math.fsum((1.0 / k) * math.log(v) for v in p))


def group_results(sentences, group_off):
    """What the grouped kernels must return for word lists ``sentences`` and row offsets ``group_off`` (G + 1 ascending, every
    group of two rows or more), under the names of ``Diversity.score_groups``."""
    group_off = [int(v) for v in group_off]
    assert group_off[0] == 0 and group_off[-1] == len(sentences)
    self_bleu, mbleu, stats, sent_distinct, group_totals, group_mean = [], [], [], [], [], []
    for b, e in zip(group_off[:-1], group_off[1:]):
        sents = sentences[b:e]
        assert len(sents) >= 2
        counted = [[D.ngrams(s, n) for n in range(1, D.ORDER + 1)] for s in sents]
        scored = [D.sentence_self_bleu(i, sents, counted) for i in range(len(sents))]
        rows = [[bleu_k(st, k) for k in range(1, D.ORDER + 1)] for _, st in scored]
        for (score, _), row in zip(scored, rows):
            assert row[D.ORDER - 1] == score
        self_bleu += [s for s, _ in scored]
        stats += [st for _, st in scored]
        mbleu += rows
        sent_distinct += [[len(D.ngrams(s, n)) for n in range(1, D.ORDER + 1)] for s in sents]
        group_totals.append([sum(len(s) for s in sents)] +
                            [len(set(g for s in sents for g in D.ngrams(s, n))) for n in range(1, D.ORDER + 1)])
        mean = []
        for k in range(D.ORDER + 1):             # added in the order of the sentences (diversity.py:24-31)
            total = 0.0
            for (score, _), row in zip(scored, rows):
                total += row[k] if k < D.ORDER else score
            mean.append(total / len(sents))
        group_mean.append(mean)
    summary = []
    for k in range(D.ORDER + 1):
        total = 0.0
        for m in group_mean:
            total += m[k]
        summary.append(total / len(group_mean))
    return {"self_bleu": np.array(self_bleu, dtype=np.float64), "mbleu": np.array(mbleu, dtype=np.float64),
            "stats": np.array(stats, dtype=np.int64), "sent_distinct": np.array(sent_distinct, dtype=np.int64),
            "group_totals": np.array(group_totals, dtype=np.int64), "group_mean": np.array(group_mean, dtype=np.float64),
            "summary": np.array(summary, dtype=np.float64)}


def group_numbers(key2sentences):
    """What ``Diversity.compute_group_score`` reports for ``{key: [sentence, ...]}`` (strings)."""
    keys = list(key2sentences)
    sentences = [s.split() for k in keys for s in key2sentences[k]]
    off = np.concatenate([[0], np.cumsum([len(key2sentences[k]) for k in keys])])
    res = group_results(sentences, off)
    names = ("mbleu_1", "mbleu_2", "mbleu_3", "mbleu_4", "self_bleu")
    per_key = {}
    for key, m, t in zip(keys, res["group_mean"].tolist(), res["group_totals"].tolist()):
        per_key[key] = dict(zip(names, m))
        per_key[key]["div_1"] = t[1] / t[0] if t[0] else float("nan")
        per_key[key]["div_2"] = t[2] / t[0] if t[0] else float("nan")
    out = dict(zip(names, res["summary"].tolist()))
    for name in ("div_1", "div_2"):
        total = 0.0
        for key in keys:
            total += per_key[key][name]
        out[name] = total / len(keys)
    out["per_key"] = per_key
    return out


# ---- a closed case, worked by hand (tests/test_multi_sample_cpu.py spells the arithmetic out) ------------------------------------
CLOSED_GROUPS = {"x": ["a b", "a c"], "y": ["a b c d", "a b c d"]}
