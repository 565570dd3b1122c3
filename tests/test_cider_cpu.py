"""CPU tests of the built-in CIDEr-D scorer: the float64 restatement (tests/_cider_ref.py) against closed-form answers,
the host side of audiocaption_amd/cider.py (canonical ids, packing, caching, refusals; no kernel runs here), and that the
batches the GPU tests score (tests/test_gpu_cider.py) are not trivial.  The rule that turns a decoder row into a sentence
(<start> skipped, cut at <end>) is applied on the device by the id route; here it is pinned on the host route that the GPU
tests compare against, ``compute_batch_score`` carrying the restatement."""
import math

import numpy as np
import pytest

import _cider_ref as R
from _scst_ref import StubVocabulary

REFS = {"a": ["w1 w2 w3 w4 w5"], "b": ["w6 w7"], "c": ["w8 w9 w10 w11"]}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_closed_form_answers():
    mean, s = R.compute_score(REFS, {"a": ["w1 w2 w3 w4 w5"], "b": ["w6 w7"], "c": [""]})
    assert s.dtype == np.float64 and s.shape == (3,)
    assert abs(s[0] - 10.0) < 1e-12                       # equal to the reference
    assert abs(s[1] - 5.0) < 1e-12                        # equal, but there are no 3- or 4-grams
    assert s[2] == 0.0                                    # empty
    assert abs(mean - 5.0) < 1e-12
    _, s = R.compute_score(REFS, {"a": [""], "b": ["w6"], "c": [""]})
    want = 10.0 / 4.0 * 2.0 ** -0.5 * math.exp(-1.0 / 72.0)
    assert abs(want - 1.7433843) < 1e-7 and abs(s[1] - want) < 1e-12
    _, s = R.compute_score({"a": REFS["a"]}, {"a": REFS["a"]})
    assert s.tolist() == [0.0]                            # one key: log 1


def test_document_frequency_counts_keys_not_sentences_or_hypotheses():
    refs = {"a": ["x y", "x x z"], "b": ["x"], "c": ["q"]}
    df = R.document_frequency(refs)
    assert df[("x",)] == 2 and df[("y",)] == 1 and df[("x", "x")] == 1 and ("x", "q") not in df
    # clipping: three x in the hypothesis against one in the reference count as one
    _, one = R.compute_score(refs, {"a": ["x"], "b": ["x"], "c": ["q"]})
    _, three = R.compute_score(refs, {"a": ["x"], "b": ["x x x"], "c": ["q"]})
    assert 0 < three[1] < one[1]


def test_restatement_as_scorer_on_the_host_route():
    """compute_batch_score: <start> skipped, the sentence cut at <end>, a repeated key scored on its first row."""
    from audiocaption_amd.rl_model import compute_batch_score
    vocab = StubVocabulary()
    rows = np.array([[1, 1, 2, 3, 4, 5, 2, 9],     # <start> <start> <end>: empty, whatever follows
                     [6, 1, 7, 2, 6, 7, 6, 7],     # "w6 w7"
                     [8, 9, 10, 11, 2, 2, 2, 2],   # "w8 w9 w10 w11"
                     [3, 4, 5, 2, 0, 0, 0, 0]])    # second row of key a, equal to its reference: ignored
    refs = {"a": ["w3 w4 w5"], "b": ["w6 w7"], "c": ["w8 w9 w10 w11"]}
    got = compute_batch_score(rows, refs, ["a", "b", "c", "a"], 1, 2, vocab, R.Scorer())
    assert np.abs(got - [0.0, 5.0, 10.0, 0.0]).max() < 1e-12
    assert R.row_sentence(rows[1], vocab.idx2word) == "w6 w7" and R.row_sentence(rows[0], vocab.idx2word) == ""


# ---- host packing ------------------------------------------------------------------------------------------------------
def test_canonical_ids_and_bad_vocabulary():
    from audiocaption_amd.cider import canonical_ids
    names = R.word_list(12)
    names[9] = names[4]
    word2id, canon = canonical_ids(R.ListVocabulary(names), 12)
    assert canon.dtype == np.int32 and canon[9] == 4 and word2id["w4"] == 4
    assert canon.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 4, 10, 11]
    # reads ids below vocab_size only
    word2id, canon = canonical_ids(R.ListVocabulary(names + ["bad word"]), 12)
    assert len(canon) == 12
    for bad in ("", "two words", " lead", "tab\t", None):
        broken = list(names)
        broken[7] = bad
        with pytest.raises(ValueError):
            canonical_ids(R.ListVocabulary(broken), 12)


def test_packing_of_the_edge_batch():
    from audiocaption_amd.cider import Cider
    case = R.edge_case()
    scorer = Cider()
    batch, canon = scorer.pack_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"])
    assert batch.keys == ["a", "b", "c", "d"]
    assert batch.row_key.tolist() == [0, 1, 2, 0, 3] and batch.first_row.tolist() == [0, 1, 2, 4]   # key a: its first row
    assert batch.key_off.tolist() == [0, 1, 3, 8, 11]
    lens = np.diff(batch.sent_off).tolist()
    assert lens == [20, 0, 70, 1, 2, 3, 4, 20, 4, 3, 6] and batch.max_ref_words == 70
    assert all(a.dtype == np.int32 for a in (batch.words, batch.sent_off, batch.key_off, batch.row_key, batch.first_row))
    # one word outside the vocabulary: the id vocab_size, and n_words counts it
    assert batch.n_words == 13 and int(batch.words.max()) == 12 and int((batch.words == 12).sum()) == 1
    s = batch.sent_off[6]
    assert batch.words[s:s + 4].tolist() == [5, 12, 4, 11]
    assert 9 not in batch.words.tolist() and canon[9] == 4
    # a second, different unknown word later gets the next id; the first keeps its own
    more = dict(case["key2refs"], e=["yak zebra w5"])
    b2, _ = scorer.pack_ids(more, case["vocabulary"], case["vocab_size"], ["e", "a"])
    assert b2.words[:3].tolist() == [13, 12, 5] and b2.n_words == 14


def test_references_are_packed_once_per_key():
    from audiocaption_amd.cider import Cider
    case = R.random_case(*R.RANDOM_CASES["repeated-keys"])
    scorer = Cider()
    names = sorted(case["key2refs"])
    scorer.pack_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"])
    assert scorer.packed_keys == len(names)
    a, _ = scorer.pack_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], names[:5] + names[:2])
    assert scorer.packed_keys == len(names)               # one epoch over one key2refs: every key once
    fresh, _ = Cider().pack_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], names[:5] + names[:2])
    assert np.array_equal(a.words, fresh.words) and np.array_equal(a.sent_off, fresh.sent_off)
    scorer.pack_ids(dict(case["key2refs"]), case["vocabulary"], case["vocab_size"], names[:3])   # another key2refs object
    assert scorer.packed_keys == len(names) + 3


def test_scorer_object_contract_and_refusals_on_the_host():
    import audiocaption_amd as A
    from audiocaption_amd.cider import Cider
    assert A.Cider is Cider and "Cider" in A.__all__
    assert Cider().method() == "CIDEr"
    with pytest.raises(ValueError):
        Cider(n=5)
    with pytest.raises(ValueError):
        Cider(sigma=0.0)
    with pytest.raises(ValueError):       # a key without references
        Cider().pack_ids({"a": []}, StubVocabulary(), 10, ["a"])
    with pytest.raises(ValueError):
        Cider().compute_score({"a": ["x"]}, {"b": ["x"]})
    with pytest.raises(ValueError):
        Cider().compute_score({"a": ["x"]}, {"a": ["x", "y"]})


def test_entry_point_refuses_before_touching_the_device():
    """AC_ERR_ARG from the C entry points with null or oversize arguments (nothing is launched on a machine without a GPU)."""
    import ctypes
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert lib.ac_cider_workspace_bytes(100, 10, 4, 2) > 0
    assert lib.ac_cider_workspace_bytes(100, 10, 4, 2) % 256 == 0
    assert lib.ac_cider_workspace_bytes(100, 10, 4, 5) == _lib.AC_ERR_ARG      # more sets than AC_CIDER_MAX_SETS
    assert lib.ac_cider_workspace_bytes(100, 3, 4, 2) == _lib.AC_ERR_ARG       # a key without a sentence
    assert lib.ac_cider_workspace_bytes(-1, 10, 4, 2) == _lib.AC_ERR_ARG
    assert lib.ac_cider_workspace_bytes(200, 10, 4, 2) >= lib.ac_cider_workspace_bytes(100, 10, 4, 2)
    one = ctypes.c_void_p(256)            # never dereferenced: every call below is refused on its sizes
    hyp = (ctypes.c_void_p * 2)(256, 256)
    H = ctypes.cast(hyp, ctypes.c_void_p)

    def call(sets=2, ld=8, N=5, T=8, vocab=12, n_words=13, total=100, sentences=10, max_ref=70, keys=4, order=4, sigma=6.0,
             ws=one, ws_bytes=1 << 30, hyp_=H):
        return lib.ac_cider_scores(hyp_, sets, ld, N, T, 1, 2, one, vocab, n_words, one, total, one, sentences, max_ref, one,
                                   keys, one, one, order, sigma, ws, ws_bytes, one, one, None)

    assert call(T=1025) == _lib.AC_ERR_ARG                # beyond the LDS budget of a hypothesis
    assert call(max_ref=1025) == _lib.AC_ERR_ARG          # a reference beyond the word limit
    assert call(ws_bytes=lib.ac_cider_workspace_bytes(100, 10, 4, 2) - 1) == _lib.AC_ERR_ARG
    assert call(ws=None) == _lib.AC_ERR_ARG
    assert call(sets=5) == _lib.AC_ERR_ARG and call(sets=1) == _lib.AC_ERR_ARG   # (a reward needs two sets)
    assert call(ld=7) == _lib.AC_ERR_ARG and call(n_words=11) == _lib.AC_ERR_ARG
    assert call(order=0) == _lib.AC_ERR_ARG and call(order=5) == _lib.AC_ERR_ARG
    assert call(sigma=0.0) == _lib.AC_ERR_ARG and call(sigma=float("nan")) == _lib.AC_ERR_ARG
    assert call(keys=11) == _lib.AC_ERR_ARG and call(hyp_=None) == _lib.AC_ERR_ARG


# ---- the batches of the GPU tests are worth scoring ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.RANDOM_CASES))
def test_random_batches_are_not_trivial(name):
    V, K, N, T = R.RANDOM_CASES[name][:4]
    case = R.random_case(*R.RANDOM_CASES[name])
    assert len(case["keys"]) == N and len(set(case["keys"])) == K and case["words"][0].shape == (N, T)
    assert (N > K) == (len(case["keys"]) != len(set(case["keys"])))
    if name == "long":      # both loops over positions take a second pass of their 256-thread workgroup
        assert max(len(r.split()) for refs in case["key2refs"].values() for r in refs) > 256
        assert max(len(R.row_sentence(r, case["vocabulary"].idx2word).split()) for w in case["words"] for r in w) > 256
    both = []
    for which in range(2):
        scores, references, hypothesis = R.host_scores(case, which)
        both.append(scores)
        df = R.document_frequency(references)
        assert max(df.values()) == K and min(df.values()) == 1
        assert any(g not in df for h in hypothesis.values() for g in R.counts(h[0])[0])
        print(f"{name} set {which}: scores {scores.min():.4f} .. {scores.max():.4f}, positive {(scores > 0).sum()} of {N}")
        assert (scores > 0).sum() * 2 >= N
        assert scores.max() - scores.min() > 0.1
        assert scores.min() >= 0 and scores.max() <= 10
    assert np.abs(both[0] - both[1]).max() > 0.1              # and the reward is not trivial either


def test_edge_batch_is_what_it_says():
    case = R.edge_case()
    idx2word = case["vocabulary"].idx2word
    sampled, greedy = case["words"]
    assert [len(R.row_sentence(r, idx2word).split()) for r in sampled] == [0, 1, 3, 8, 8]
    assert R.row_sentence(sampled[2], idx2word) == "w5 w4 w11" and case["vocab_size"] - 1 in sampled[2]
    assert [len(R.row_sentence(r, idx2word).split()) for r in greedy] == [3, 8, 0, 0, 2]
    s0, _, _ = R.host_scores(case, 0)
    s1, _, _ = R.host_scores(case, 1)
    print("edge batch scores", s0, s1)
    assert s0[0] == 0.0 and s0[3] == 0.0 and s1[0] == s1[3] > 0      # key a: the first row's sentence for both rows
    # (key b: a 70-word reference against at most 8 words - the length penalty leaves next to nothing)
    assert 0 <= s0[1] < 1e-20 and s0[2] > 0.1 and s0[4] > 0.1 and 0 <= s1[1] < 1e-20 and s1[2] == 0.0 and s1[4] > 0.1
