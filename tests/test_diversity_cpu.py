"""CPU tests of the built-in diversity scorer: the float64 restatement (tests/_diversity_ref.py) against the closed forms
worked by hand and against the reference's own richness (tests/golden/g25_diversity.npz, recorded from
eval/old_diversity.py by tests/golden/make_golden_diversity.py), the host side of audiocaption_amd/diversity.py (refusals
before any device work, ``novel``, the instance means; no kernel runs here), the C entry points refusing on their sizes,
and that the corpora the GPU tests score (tests/test_gpu_diversity.py) contain the shapes they are meant to contain.

Self-BLEU is nltk's sentence_bleu with method1 smoothing; nltk is not available to this project, so the closed forms
below - each written out from the definition - are what pins the restatement, and the restatement is what the device is
held to."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _diversity_ref as D
from _metrics_ref import close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "g25_diversity.npz")


def gate(want):
    return 1e-12 + 1e-9 * np.abs(want)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_self_bleu_closed_forms():
    for name, (sentences, want) in D.CLOSED.items():
        got = D.host_results([s.split() for s in sentences])
        assert len(got["self_bleu"]) == len(want)
        for g, w in zip(got["self_bleu"], want):
            assert close(g, w), (name, g, w)
    # the same answers written out from the definition
    c = D.CLOSED["captions"][1]
    assert c[0] == 0.1 ** 0.25 and c[1] == 0.025 ** 0.25 and c[3] == 0.0
    assert abs(c[2] - (1 / 3 * 0.05 * 0.1 * 0.1) ** 0.25) < 1e-15
    got = D.host_results([s.split() for s in D.CLOSED["captions"][0]])
    assert got["self_bleu"][3] == 0.0                                    # no unigram matches: exactly 0
    assert close(got["summary"][0], D.CLOSED_CAPTIONS["mean"]) and close(got["summary"][0], sum(c) / 4)
    # L, ref_len, den[4], num[4]: "a dog barks" is contained in "a dog barks loudly", whose own closest length is 3
    assert got["stats"].tolist() == [[3, 3, 3, 2, 1, 1, 3, 2, 1, 0], [4, 3, 4, 3, 2, 1, 3, 2, 1, 0],
                                     [3, 3, 3, 2, 1, 1, 1, 0, 0, 0], [1, 3, 1, 1, 1, 1, 0, 0, 0, 0]]
    assert got["totals"].tolist()[:3] == D.CLOSED_CAPTIONS["totals"]
    # "a" three times in two sentences: each owner is clipped at 3 by the other; held once: clipped at the runner-up's 2
    tied = D.host_results([s.split() for s in D.CLOSED["tied-maximum"][0]])["stats"]
    single = D.host_results([s.split() for s in D.CLOSED["single-maximum"][0]])["stats"]
    assert tied[0, 6] == 3 and tied[2, 6] == 3 and tied[1, 6] == 2 and single[0, 6] == 2 and single[1, 6] == 2
    assert abs(D.CLOSED["tied-maximum"][1][0] - (3 / 4 * 2 / 3 * 1 / 2 * 0.1) ** 0.25) < 1e-15
    # an empty sentence scores 0, and its length is a candidate for the others: 0 and 2 are equally close to 1
    got = D.host_results([[], ["a"], ["a", "b"]])
    assert got["self_bleu"][0] == 0.0 and got["stats"][:, :2].tolist() == [[0, 1], [1, 0], [2, 1]]
    assert abs(got["self_bleu"][1] - (1 * 0.1 ** 3) ** 0.25) < 1e-15          # bp 1: one word against a closest length of 0
    # below the closest length: the brevity penalty of nltk, exp(1 - ref_len / L)
    got = D.host_results([["a", "b"], ["a", "b", "c", "d"]])
    assert abs(got["self_bleu"][0] - math.exp(1 - 4 / 2) * (1 * 1 * 0.1 * 0.1) ** 0.25) < 1e-15
    assert abs(got["self_bleu"][1] - (2 / 4 * 1 / 3 * 0.1 / 2 * 0.1 / 1) ** 0.25) < 1e-15


def test_richness_closed_forms_and_the_reference():
    each, overall = D.richness([s.split() for s in D.CLOSED["captions"][0]])
    for g, w in zip(each, D.CLOSED_CAPTIONS["richness"]):
        assert close(g, w), (g, w)
    assert close(overall, D.CLOSED_CAPTIONS["overall"]) and abs(each[3] - math.log(4)) < 1e-15
    # unigrams written out: "a" is in 3 of 4 sentences, "dog" and "barks" in 2, the rest in 1
    a, two, one = math.log(4 / 3), math.log(2), math.log(4)
    want = ((a + 2 * two) / 3 + (a + 2 * two + one) / 4 + (a + 2 * one) / 3 + one) / 4
    assert abs(each[0] - want) < 1e-14
    # the reference's own numbers (old_diversity.py) for every corpus of the GPU tests
    fixture = np.load(GOLDEN)
    assert fixture["cases"].tolist() == D.CASES
    for c, name in enumerate(D.CASES):
        got = D.want(name)["summary"]
        ref = np.concatenate((fixture["richness_per_order"][c], fixture["richness"][c:c + 1]))
        assert np.array_equal(np.isnan(got[1:]), np.isnan(ref)), name
        ok = ~np.isnan(ref)
        assert np.all(np.abs(got[1:][ok] - ref[ok]) <= gate(ref[ok])), (name, got[1:], ref)
    assert np.isnan(D.want("minimum")["summary"][4:]).all()           # nobody has a 4-gram: the reference divides by zero


def test_corpus_numbers():
    got = D.corpus_numbers([s.split() for s in ["a b a", "a b c d", "c d"]])
    assert got["vocabulary"] == 4 and got["distinct_1"] == 4 / 9 and got["distinct_2"] == 4 / 9     # (by words, not bigrams)
    assert abs(got["distinct_1_instance"] - (2 / 3 + 1 + 1) / 3) < 1e-15 and got["distinct_2_instance"] == 1.0
    assert "distinct_1_instance" not in D.corpus_numbers([["a"], ["a", "b"]])


# ---- the scorer on the host --------------------------------------------------------------------------------------------
def test_refusals_before_any_device_work():
    import torch
    import audiocaption_amd as A
    from audiocaption_amd.cider import MAX_HYP_WORDS, PackedScorer
    from audiocaption_amd.diversity import Diversity
    assert A.Diversity is Diversity and "Diversity" in A.__all__ and issubclass(Diversity, PackedScorer)
    scorer = Diversity()
    assert not hasattr(scorer, "method")           # it takes no references: not a scorer for eval_prediction
    vocabulary = D.ListVocabulary(D.word_list(12))
    with pytest.raises(ValueError, match="closest_ref_length"):          # one sentence: nothing to choose a length from
        scorer.compute_score(["a b c"])
    with pytest.raises(ValueError, match="closest_ref_length"):
        scorer.compute_score({"k": ["a b c"]})
    with pytest.raises(ValueError, match="closest_ref_length"):
        scorer.score_ids(vocabulary, 12, torch.full((1, 5), 4), D.START, D.END)
    with pytest.raises(ValueError, match="closest_ref_length"):
        scorer.compute_score([])
    long = " ".join(["w"] * (MAX_HYP_WORDS + 1))
    with pytest.raises(ValueError, match=str(MAX_HYP_WORDS)):            # beyond the kernel's limit
        scorer.compute_score([long, "a b"], instance=False)
    with pytest.raises(ValueError, match=str(MAX_HYP_WORDS)):
        scorer.score_ids(vocabulary, 12, [torch.full((2, 5), 4), torch.full((2, MAX_HYP_WORDS + 1), 4)], D.START, D.END)
    names = D.word_list(12)
    names[7] = "two words"
    with pytest.raises(ValueError, match="whitespace"):                  # the vocabulary rule of canonical_ids
        scorer.score_ids(D.ListVocabulary(names), 12, torch.full((2, 5), 4), D.START, D.END)
    with pytest.raises(ValueError):                                      # a word id outside the vocabulary, seen on the host
        scorer.score_ids(vocabulary, 12, torch.tensor([[4, 12, D.END], [4, 5, D.END]]), D.START, D.END)
    with pytest.raises(ValueError):                                      # not (N, T)
        scorer.score_ids(vocabulary, 12, torch.full((5,), 4), D.START, D.END)
    with pytest.raises(ValueError):                                      # a string where a list of sentences belongs
        scorer.compute_score({"k": "a b c", "l": "a b"})
    with pytest.raises(ValueError, match="sentence 1 .'rain'. has 1 word"):       # the instance means, before any launch
        scorer.compute_score(["a dog barks", "rain", "b"])


def test_novel_and_instance_means_on_the_host():
    from audiocaption_amd.diversity import instance_means, novel_share
    sentences = ["a dog barks", "a dog barks loudly", "a cat meows", "rain"]
    assert novel_share(sentences, ["a dog barks", "rain", "snow falls"]) == 0.5
    assert novel_share(sentences, {"a dog barks"}) == 0.75 and novel_share(sentences, (s for s in sentences)) == 0.0
    assert novel_share(sentences, []) == 1.0
    assert novel_share(["a  dog"], ["a dog"]) == 1.0                  # the whole string is looked up, as the reference does
    want = D.host_results([s.split() for s in sentences])
    with pytest.raises(ValueError, match="sentence 3 .'rain'. has 1 word"):
        instance_means(want["stats"], want["sent_distinct"], sentences)
    with pytest.raises(ValueError, match="sentence 0 has 0 word"):
        instance_means(np.array([[0] * 10, [3] * 10]), np.array([[0] * 4, [3, 2, 1, 0]]))
    corpus = [s.split() for s in ["a b a", "a b c d", "c d"]]
    want = D.host_results(corpus)
    d1, d2 = instance_means(want["stats"], want["sent_distinct"])
    numbers = D.corpus_numbers(corpus)
    assert d1 == numbers["distinct_1_instance"] and d2 == numbers["distinct_2_instance"]


def test_string_route_packing():
    from audiocaption_amd.diversity import Diversity
    scorer = Diversity()
    assert scorer._sentences({"k": ["a b", "c"], "l": ["d"]}) == ["a b", "c", "d"] and scorer._sentences(("x", "y")) == ["x", "y"]
    rows, start, end, vocab = scorer._pack_sentences(["b a b", "", "a  c\t"])
    assert rows.dtype == np.int32 and rows.shape == (3, 3) and vocab == 2 + 3 and start not in rows
    b, a = rows[0, 0], rows[0, 1]
    assert rows.tolist() == [[b, a, b], [end] * 3, [a, rows[2, 1], end]] and rows[2, 1] not in (a, b, end)
    rows, _, end, _ = scorer._pack_sentences(["", " "])                  # no word at all: one column of <end>
    assert rows.tolist() == [[end], [end]]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_abi_header_and_build_sources():
    from audiocaption_amd import _lib, build
    assert "diversity.hip" in build.SOURCES and _lib.ABI_VERSION == 2
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    assert "#define AC_ABI_VERSION 2" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ac_diversity_workspace_bytes", "ac_diversity_scores"):
        proto = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert proto, name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_long if proto.group(1) == "long" else ctypes.c_int)
        params = [a.strip() for a in proto.group(2).split(",")]
        assert len(params) == len(args), name
        for a, w in zip(params, args):
            want = (ctypes.c_void_p if "*" in a else ctypes.c_long if a.startswith("long ") else ctypes.c_int)
            assert w is want, (name, a)


def test_entry_points_refuse_before_touching_the_device():
    """AC_ERR_ARG from the C entry points with null or oversize arguments (nothing is launched on a machine without a GPU)."""
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    size = lib.ac_diversity_workspace_bytes
    need = size(5, 8)
    # the smallest table (64 slots: 4 bytes of representative and 16 of counts each) and four ints per position at least
    assert need > 0 and need % 256 == 0 and need >= 64 * 20 + 5 * 8 * 36
    assert size(2, 1) > 0 and size(2, 1) % 256 == 0 and size(1 << 16, 1024) % 256 == 0 and size(1 << 16, 1024) > 1 << 32
    assert size(5225, 30) % 256 == 0 and size(300, 24) > size(5, 8)
    for N, T in ((1, 8), (0, 8), (-3, 8), (5, 0), (5, 1025), (5, -1), ((1 << 16) + 1, 1024), (1 << 30, 8)):
        assert size(N, T) == _lib.AC_ERR_ARG, (N, T)
    one = ctypes.c_void_p(256)            # never dereferenced: every call below is refused on its sizes

    def call(hyp=one, ld=8, N=5, T=8, canon=one, vocab=12, ws=one, ws_bytes=1 << 40, stats=one, sent=one, totals=one,
             bleu=one, summary=one):
        return lib.ac_diversity_scores(hyp, ld, N, T, 1, 2, canon, vocab, ws, ws_bytes, stats, sent, totals, bleu, summary,
                                       None)

    for name in ("hyp", "canon", "ws", "stats", "sent", "totals", "bleu", "summary"):
        assert call(**{name: None}) == _lib.AC_ERR_ARG, name
    assert call(N=1) == _lib.AC_ERR_ARG and call(N=0) == _lib.AC_ERR_ARG
    assert call(T=0, ld=8) == _lib.AC_ERR_ARG and call(T=1025, ld=1025) == _lib.AC_ERR_ARG
    assert call(N=(1 << 16) + 1, T=1024, ld=1024) == _lib.AC_ERR_ARG          # N * T over 2^26
    assert call(ld=7) == _lib.AC_ERR_ARG and call(vocab=0) == _lib.AC_ERR_ARG
    assert call(ws_bytes=need - 1) == _lib.AC_ERR_ARG and call(ws_bytes=0) == _lib.AC_ERR_ARG
    assert call(ws=ctypes.c_void_p(128)) == _lib.AC_ERR_ARG                   # not 256-byte aligned


# ---- the corpora of the GPU tests contain what they are meant to -------------------------------------------------------
def test_corpora_contain_the_shapes_that_matter():
    edge, want = D.make_case("edge"), D.want("edge")
    st = want["stats"]
    assert st[:, 0].tolist() == [0, 1, 2, 3, 4, 4, 7, 8, 10] and edge["words"].shape == (9, 10)
    assert want["self_bleu"][0] == 0.0 and np.all(want["self_bleu"][1:] > 0)
    assert st[1, 1] == 0 and st[3, 1] == 2                         # two lengths equally close: the smaller
    assert st[6, 0] < st[6, 1] and st[7, 0] > st[7, 1]             # brevity penalty below 1 and none
    assert np.array_equal(edge["words"][4, :5], edge["words"][5, :5]) and want["self_bleu"][4] == want["self_bleu"][5]
    assert np.array_equal(st[4, 6:], st[4, 2:6])                   # a twin: every n-gram matched in full
    assert edge["words"][1, 0] == D.START and D.START in edge["words"][3, 1:] and D.END not in edge["words"][8]
    assert {0, 11, 4, 9} <= set(edge["words"][6, :7].tolist()) and edge["vocabulary"].idx2word[9] == edge["vocabulary"].idx2word[4]
    assert edge["sentences"][6].count("w4") == 2 == edge["sentences"][8].count("w4")          # a tied maximum of 2
    six = [s.count("w6") for s in edge["sentences"]]
    assert six[7] == 6 and sorted(six)[-2] == 1                    # the maximum held once: clipped at the second maximum
    assert want["sent_distinct"][7].tolist() == [3, 5, 6, 5] and st[7, 6] == 3 and st[7, 7] == 1   # "w6 w6": nobody else
    crowded = D.make_case("crowded")
    assert crowded["words"].shape == (300, 24) and crowded["vocab_size"] == 33
    lens = D.want("crowded")["stats"][:, 0]
    assert lens.min() == 0 and lens.max() == 24 and D.want("crowded")["totals"][1] == 30
    assert D.make_case("minimum")["words"].size * 8 < 64                                       # the table at its minimum
    assert D.want("long")["stats"][:, 0].tolist() == [70, 1024, 300, 0, 5] and D.make_case("long")["words"].shape == (5, 1024)
    for name in D.CASES:
        w = D.want(name)
        assert 0 < w["summary"][0] < 1 and w["self_bleu"].min() >= 0 and w["self_bleu"].max() <= 1, name
