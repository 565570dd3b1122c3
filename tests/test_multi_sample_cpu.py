"""Several sampled captions per clip (``n_samples``) and diversity within groups, the parts that need no GPU: every refusal
(each raised on the host, before an encoder or a kernel runs), the header / ctypes rows of the new entry points and their
argument refusals, ``DictTokenizer.decode`` and ``write_predictions`` on several captions per clip, the packing of
``Diversity.compute_group_score``, and the grouped CPU reference (tests/_group_diversity_ref.py) against the pooled one and
against a closed case worked by hand."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import _diversity_ref as D
import _group_diversity_ref as G
from _metrics_ref import close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ac_trm_sample_multi", "ac_diversity_group_workspace_bytes", "ac_diversity_group_scores")
DEC = dict(emb_dim=128, vocab_size=60, fc_emb_dim=64, attn_emb_dim=64, dropout=0.2, nhead=2, dim_feedforward=256)


def _trm_model():
    import audiocaption_amd as A
    return A.TransformerModel(torch.nn.Identity(), A.TransformerDecoder(**DEC)).eval()


def _request(**over):
    d = {"mode": "inference", "attn_emb": torch.zeros(3, 7, 64), "fc_emb": torch.zeros(3, 64),
         "attn_emb_len": torch.tensor([7, 3, 5]), "sample_method": "sample", "max_length": 6}
    d.update(over)
    return d


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_transformer_model_refuses_n_samples_for_greedy_beam_and_bad_values():
    model = _trm_model()
    for method in ("greedy", "beam"):
        with pytest.raises(ValueError, match="n_samples"):
            model(_request(sample_method=method, n_samples=2))
        with pytest.raises(ValueError, match="n_samples"):
            model.forward_decoder(_request(sample_method=method, n_samples=2), {})
    d = _request(n_samples=2)
    del d["sample_method"]                                   # the default method is greedy
    with pytest.raises(ValueError, match="n_samples"):
        model(d)
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="n_samples"):
            model(_request(n_samples=bad))
    with pytest.raises(NotImplementedError, match="dbs"):    # keeps raising as it does
        model(_request(sample_method="dbs", n_samples=2))
    with pytest.raises(NotImplementedError, match="n_samples"):
        model.forward_async(_request(n_samples=2))
    with pytest.raises(NotImplementedError, match="n_samples"):
        model.forward_async(_request(sample_method="greedy", n_samples=2))
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="samples_per_clip"):
            model.decoder.sample(torch.zeros(3, 7, 64), [7, 3, 5], 6, 1, 2, 0, 0, 0, 0.0, 1.0, 1, samples_per_clip=bad)
    with pytest.raises(ValueError, match="samples_per_clip"):   # R * (max_length + 1) beyond the search's row index
        model.decoder.sample(torch.zeros(3, 7, 64), [7, 3, 5], 20, 1, 2, 0, 0, 0, 0.0, 1.0, 1, samples_per_clip=2 ** 26)


def test_other_models_name_the_feature():
    import audiocaption_amd as A
    import _keyword_trm_ref as K
    import _attn_gru_train_ref as R
    kdec = A.KeywordProbTransformerDecoder(**dict(K.SHAPES["d128"], dropout=0.2)).eval()
    kmodel = A.KeywordCondTransformerModel(torch.nn.Identity(), kdec).eval()
    attn, lens, kw = K.infer_inputs("d128")
    base = {"mode": "inference", "attn_emb": attn, "fc_emb": torch.zeros(K.B, 64), "attn_emb_len": lens, "keyword": kw}
    for method in ("sample", "greedy"):
        with pytest.raises(NotImplementedError, match="n_samples"):
            kmodel(dict(base, sample_method=method, n_samples=2))
    with pytest.raises(NotImplementedError, match="not built for a conditioned decoder"):
        A.TransformerDecoder.sample(kdec, attn, lens, 6, 1, 2, 0, 0, 0, 0.0, 1.0, 1, extra=kw, samples_per_clip=2)
    for cls, dec in ((A.Seq2SeqAttnModel, A.rnn_decoder.BahAttnCatFcDecoder),
                     (A.TemporalSeq2SeqAttnModel, A.rnn_decoder.TemporalBahAttnDecoder)):
        amodel = cls(torch.nn.Identity(), dec(dropout=0.0, **R.SMALL)).eval()
        for method in ("sample", "greedy", "beam"):
            with pytest.raises(NotImplementedError, match="n_samples"):
                amodel(_request(sample_method=method, n_samples=2))
            with pytest.raises(NotImplementedError, match="n_samples"):
                amodel.forward_decoder(_request(sample_method=method, n_samples=2), {})
    ens = A.EnsembleModel([_trm_model(), _trm_model()])
    with pytest.raises(NotImplementedError, match="n_samples"):
        ens(_request(n_samples=2))


def test_scst_refuses_n_samples():
    import audiocaption_amd as A
    from audiocaption_amd.train import TrainEngine
    from audiocaption_amd.train_attn_gru import AttnGruTrainEngine
    for cls in (TrainEngine, AttnGruTrainEngine):
        eng = object.__new__(cls)                  # the refusal comes first: nothing of the engine is touched
        eng.model, eng.keyword = None, False
        with pytest.raises(NotImplementedError, match="n_samples"):
            eng.rollout({"n_samples": 2})
    wrapper = A.ScstWrapper(A.init_model_from_config(A.cnn14rnn_trm_config(61), print_fn=lambda s: None))
    with pytest.raises(NotImplementedError, match="n_samples"):
        wrapper({"mode": "train", "wav": torch.zeros(2, 32000), "wav_len": [32000, 32000], "n_samples": 2})


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_rows_of_the_new_entry_points():
    from audiocaption_amd import _lib
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = dict(re.findall(r"\b(?:int|long)\s+(ac_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body))
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in protos, name
        assert len([a for a in protos[name].split(",")]) == len(_lib.SIGNATURES[name][1]), name
    multi = [a.strip() for a in protos["ac_trm_sample_multi"].split(",")]
    plain = [a.strip() for a in protos["ac_trm_sample"].split(",")]
    assert multi[:4] == plain[:4] and multi[4] == "int samples_per_clip" and multi[5:] == plain[4:]
    assert "Richness is not part of the grouped call" in header


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    w = _lib.AcTrmWeights()
    w.d_model, w.nhead, w.nlayers, w.dim_ff, w.vocab, w.max_pos, w.attn_emb_dim = 128, 2, 2, 256, 60, 100, 64
    w = ctypes.byref(w)
    P = ctypes.c_void_p(0x7f0000001000)          # never dereferenced on the host
    E = _lib.AC_ERR_ARG

    def multi(B, S, L, a=P):
        return lib.ac_trm_sample_multi(w, a, a, B, S, 7, L, 1, 2, 0, a, a, a, a, a, a, 0, 0, 0.0, 1.0, a, None)
    assert multi(3, 0, 6) == E and multi(3, -2, 6) == E and multi(0, 2, 6) == E
    assert multi(3, 2, 6, None) == E                       # a good shape, null operands
    assert multi(1 << 20, 1 << 10, 6) == E                 # R * (max_len + 1) beyond int32
    assert multi(1 << 16, 1 << 16, 6) == E                 # B * S itself beyond int32
    assert multi(3, 2, 101) == E                           # max_len beyond the positional table, as ac_trm_sample
    assert lib.ac_trm_workspace_floats(w, 33, 6) > lib.ac_trm_workspace_floats(w, 3, 6) > 0

    wsb = lib.ac_diversity_group_workspace_bytes
    assert wsb(10, 8, 5) > 0 and wsb(10, 8, 1) > 0 and wsb(10, 8, 5) % 256 == 0
    assert wsb(10, 8, 5) >= lib.ac_diversity_workspace_bytes(10, 8) + 4 * 10 + 4 * 5 * 5
    assert wsb(10, 8, 0) == E and wsb(10, 8, 6) == E       # no group; a group would have fewer than two rows
    assert wsb(1, 8, 1) == E and wsb(10, 0, 2) == E and wsb(10, 1025, 2) == E and wsb(1 << 20, 1024, 2) == E

    def scores(N=10, T=8, G=5, hyp=P, off=P, ws=P, nbytes=1 << 30, out=P, ld=8):
        return lib.ac_diversity_group_scores(hyp, ld, N, T, 1, 0, P, 12, off, G, ws, nbytes, out, out, out, out, out, out, out,
                                             None)
    assert scores(G=0) == E and scores(G=6) == E and scores(hyp=None) == E and scores(off=None) == E
    assert scores(ws=None) == E and scores(ws=ctypes.c_void_p(0x7f0000001010)) == E and scores(out=None) == E
    assert scores(nbytes=wsb(10, 8, 5) - 1) == E and scores(ld=7) == E


# ---- several captions per clip as text ---------------------------------------------------------------------------------------------
def test_decode_and_write_predictions_keep_every_caption_of_a_clip(tmp_path):
    from audiocaption_amd.text import DictTokenizer, write_predictions
    tok = DictTokenizer()
    for w in ("a", "dog", "barks", "rain"):
        tok.add_word(w)
    a, dog, barks, rain = (tok.word2idx[w] for w in ("a", "dog", "barks", "rain"))
    seq = np.array([[[a, dog, barks, tok.eos], [rain, tok.eos, dog, dog], [tok.eos, a, a, a]],
                    [[tok.bos, a, dog, rain], [dog, tok.eos, tok.eos, tok.eos], [a, a, tok.eos, tok.pad]]], dtype=np.int64)
    want = [["a dog barks", "rain", ""], ["a dog rain", "dog", "a a"]]
    assert tok.decode(seq) == want and tok.decode(torch.from_numpy(seq)) == want
    assert tok.decode(seq[0]) == want[0] and tok.decode(seq[1, 2]) == ["a a"]         # 2-D and 1-D as before
    assert tok.decode(seq[:, :1]) == [["a dog barks"], ["a dog rain"]]
    with pytest.raises(KeyError):
        tok.decode(np.full((1, 2, 3), 99))
    path = tmp_path / "pred.json"
    write_predictions({"x.wav": want[0], "y.wav": ["a dog"], "z.wav": "rain"}, str(path))
    rows = json.load(open(path))["predictions"]
    assert rows == [{"filename": "x.wav", "tokens": want[0]}, {"filename": "y.wav", "tokens": "a dog"},
                    {"filename": "z.wav", "tokens": "rain"}]


# ---- compute_group_score: packing and refusals -------------------------------------------------------------------------------------
def test_group_packing_and_refusals():
    from audiocaption_amd.diversity import Diversity, MAX_TOTAL_WORDS
    from audiocaption_amd.cider import MAX_HYP_WORDS
    scorer = Diversity()
    hyp = {"k1": ["a b", "a c"], "k2": ["d", "", "a b c d e", "b"], "k3": ["e e", "e", "a"]}      # ragged: 2, 4 and 3
    keys, rows, off, start_idx, end_idx, vocab_size = scorer._pack_groups(hyp)
    assert keys == ["k1", "k2", "k3"] and off.dtype == np.int32 and off.tolist() == [0, 2, 6, 9]
    assert rows.dtype == np.int32 and rows.shape == (9, 5) and (start_idx, end_idx, vocab_size) == (1, 0, 7)
    a, b, c, d, e = 2, 3, 4, 5, 6                                    # numbered by first appearance, the same word one id
    assert rows.tolist() == [[a, b, 0, 0, 0], [a, c, 0, 0, 0], [d, 0, 0, 0, 0], [0, 0, 0, 0, 0], [a, b, c, d, e],
                             [b, 0, 0, 0, 0], [e, e, 0, 0, 0], [e, 0, 0, 0, 0], [a, 0, 0, 0, 0]]
    assert Diversity._group_offsets([2, 5, 3]).tolist() == [0, 2, 7, 10]
    for bad in ({"k": ["alone"]}, {"k1": ["a", "b"], "k2": []}, {}):
        with pytest.raises(ValueError, match="two or more|no groups"):
            scorer.compute_group_score(bad)
    with pytest.raises(ValueError, match="sentence"):
        scorer.compute_group_score({"k": "a string"})
    with pytest.raises(ValueError, match="sentence"):
        scorer.compute_group_score(["a", "b"])
    with pytest.raises(ValueError, match="strings"):
        scorer.compute_group_score({"k": ["a", 3]})
    with pytest.raises(ValueError, match=str(MAX_HYP_WORDS)):
        scorer.compute_group_score({"k": ["w " * (MAX_HYP_WORDS + 1), "w"]})
    # score_groups: the shapes and offsets are judged on the host
    vocabulary, V = D.make_case("edge")["vocabulary"], 12
    words = torch.zeros(4, 3, dtype=torch.int64)
    for off_ in ([0, 1, 4], [0, 4, 4], [1, 4], [0, 2, 3], [0], [0, 2, 1, 4]):
        with pytest.raises(ValueError, match="two or more|group_off"):
            scorer.score_groups(vocabulary, V, words, D.START, D.END, group_off=off_)
    with pytest.raises(ValueError, match="group_off"):
        scorer.score_groups(vocabulary, V, words, D.START, D.END)
    with pytest.raises(ValueError, match="group_off"):
        scorer.score_groups(vocabulary, V, words.view(2, 2, 3), D.START, D.END, group_off=[0, 2, 4])
    with pytest.raises(ValueError, match="two or more"):
        scorer.score_groups(vocabulary, V, words.view(4, 1, 3), D.START, D.END)
    with pytest.raises(ValueError, match="outside"):
        scorer.score_groups(vocabulary, V, torch.full((2, 2, 3), 12), D.START, D.END)
    with pytest.raises(ValueError, match=str(MAX_HYP_WORDS)):
        scorer.score_groups(vocabulary, V, torch.zeros(1, 2, MAX_HYP_WORDS + 1, dtype=torch.int64), D.START, D.END)
    with pytest.raises(ValueError, match=str(MAX_TOTAL_WORDS)):
        scorer.score_groups(vocabulary, V, torch.zeros(1, 1, 1, dtype=torch.int8).expand(1 << 17, 2, 1024), D.START, D.END)
    with pytest.raises(ValueError, match="words must be"):
        scorer.score_groups(vocabulary, V, torch.zeros(5, dtype=torch.int64), D.START, D.END)


# ---- the grouped reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.CASES)
def test_one_group_is_the_pooled_reference(name):
    sentences, want = D.make_case(name)["sentences"], D.want(name)
    got = G.group_results(sentences, [0, len(sentences)])
    for k in ("stats", "sent_distinct", "self_bleu"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["group_totals"][0], want["totals"])
    assert got["group_mean"][0, 4] == want["summary"][0] == got["summary"][4]
    assert np.array_equal(got["mbleu"][:, 3], got["self_bleu"])


def test_closed_case_worked_by_hand():
    """Key x = ["a b", "a c"], key y = ["a b c d", "a b c d"].

    x, "a b" against "a c" (and the other way round, by symmetry): L = 2 = ref_len, bp = exp(1 - 2 / 2) = 1; unigrams: "a"
    matches, "b" does not: 1 / 2; bigrams: 0 of 1, smoothed to 0.1 / 1; orders 3 and 4: no n-gram, den = 1, smoothed to 0.1.
      mBLEU-1 = 1/2, mBLEU-2 = sqrt(0.5 * 0.1), mBLEU-3 = cbrt(0.5 * 0.1 * 0.1), mBLEU-4 = (0.5 * 0.1^3)^(1/4) = Self-BLEU
      4 words; distinct: {a, b, c}, {a b, a c}, none, none: div-1 = 3 / 4, div-2 = 2 / 4
    "a b" is a bigram of y's sentences as well: pooled, it would match there (the trap of one shared table) - within x it does not.
    y, two identical sentences: every n-gram matches, num = den = 4, 3, 2, 1, bp = 1: every mBLEU and Self-BLEU are 1;
      8 words; distinct 4, 3, 2, 1: div-1 = 4 / 8, div-2 = 3 / 8.
    Over the keys: the means of the two."""
    x = [0.5, 0.05 ** 0.5, 0.005 ** (1 / 3), 0.0005 ** 0.25]
    assert [round(v, 12) for v in x] == [0.5, 0.223606797750, 0.170997594668, 0.149534878122]
    sentences = [s.split() for g in G.CLOSED_GROUPS.values() for s in g]
    got = G.group_results(sentences, [0, 2, 4])
    assert got["stats"].tolist() == [[2, 2, 2, 1, 1, 1, 1, 0, 0, 0]] * 2 + [[4, 4, 4, 3, 2, 1, 4, 3, 2, 1]] * 2
    assert got["sent_distinct"].tolist() == [[2, 1, 0, 0]] * 2 + [[4, 3, 2, 1]] * 2
    assert got["group_totals"].tolist() == [[4, 3, 2, 0, 0], [8, 4, 3, 2, 1]]
    for row in got["mbleu"][:2]:
        assert all(close(g, w) for g, w in zip(row, x)), row
    assert np.array_equal(got["mbleu"][2:], np.ones((2, 4))) and got["self_bleu"].tolist()[2:] == [1.0, 1.0]
    assert all(close(g, w) for g, w in zip(got["group_mean"][0], x + [x[3]])) and got["group_mean"][1].tolist() == [1.0] * 5
    assert all(close(g, (w + 1) / 2) for g, w in zip(got["summary"], x + [x[3]]))
    numbers = G.group_numbers(G.CLOSED_GROUPS)
    assert numbers["per_key"]["x"]["div_1"] == 0.75 and numbers["per_key"]["x"]["div_2"] == 0.5
    assert numbers["per_key"]["y"]["div_1"] == 0.5 and numbers["per_key"]["y"]["div_2"] == 0.375
    assert numbers["div_1"] == 0.625 and numbers["div_2"] == 0.4375 and close(numbers["mbleu_1"], 0.75)
    assert close(numbers["self_bleu"], (x[3] + 1) / 2) and numbers["mbleu_4"] == numbers["self_bleu"]
    # pooled, x's sentences would see y's "a b": the grouped reference is not the pooled one
    pooled = D.host_results(sentences)
    assert pooled["stats"][0].tolist()[6:8] == [2, 1] and got["stats"][0].tolist()[6:8] == [1, 0]
