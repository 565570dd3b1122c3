"""Repetition and word constraints (``repetition_penalty``, ``no_repeat_ngram_size``, ``bad_words``, ``min_length``), the parts
that need no GPU: the numpy restatement of the rules (tests/_logit_rules_ref.py) on hand-made prefixes, every host refusal,
neutral parsing, the header / ctypes rows of the new entry points, and the reference searches on the four ``g4_greedy``
memories - the rules hold in their outputs, each rule changes captions, and the inputs are far enough from a tie that a
device whose logits differ from the oracle's by 1e-4 must make the same choices."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _logit_rules_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ac_logit_rules_apply", "ac_trm_search_rules", "ac_trm_beam_step_rules")
DEC = dict(emb_dim=128, vocab_size=60, fc_emb_dim=64, attn_emb_dim=64, dropout=0.2, nhead=2, dim_feedforward=256)
INF = float("inf")


def _z(V=12):
    """Positive, negative and zero logits, all different."""
    return (np.arange(V, dtype=np.float32) - 4.0) * np.float32(0.75)        # z[4] == 0


def _banned(out):
    return sorted(np.flatnonzero(np.isneginf(out)).tolist())


# ---- the rules on hand-made prefixes ---------------------------------------------------------------------------------------------
def test_no_repeat_ngram_sizes_one_two_three():
    z = _z()
    assert _banned(R.apply(z, [], no_repeat_ngram_size=1)) == []
    assert _banned(R.apply(z, [5, 7, 5], no_repeat_ngram_size=1)) == [5, 7]                 # every generated word
    # n = 2: the words that followed the last word before
    assert _banned(R.apply(z, [], no_repeat_ngram_size=2)) == []                             # t = 0 = n - 2: nothing to match
    assert _banned(R.apply(z, [5], no_repeat_ngram_size=2)) == []                            # t = n - 1: no complete bigram yet
    assert _banned(R.apply(z, [5, 7, 9, 5], no_repeat_ngram_size=2)) == [7]
    assert _banned(R.apply(z, [5, 7, 5, 9, 5], no_repeat_ngram_size=2)) == [7, 9]
    assert _banned(R.apply(z, [3, 3, 3], no_repeat_ngram_size=2)) == [3]                     # overlapping: a a a bans a
    assert _banned(R.apply(z, [3, 3], no_repeat_ngram_size=2)) == [3]
    assert _banned(R.apply(z, [5, 7, 9], no_repeat_ngram_size=2)) == []
    # n = 3
    assert _banned(R.apply(z, [5], no_repeat_ngram_size=3)) == []                            # t < n - 1
    assert _banned(R.apply(z, [5, 7], no_repeat_ngram_size=3)) == []                         # t = n - 1
    assert _banned(R.apply(z, [5, 7, 9, 5, 7], no_repeat_ngram_size=3)) == [9]
    assert _banned(R.apply(z, [5, 7, 9, 7, 5], no_repeat_ngram_size=3)) == []
    assert _banned(R.apply(z, [3, 3, 3, 3], no_repeat_ngram_size=3)) == [3]                  # overlapping trigrams
    assert _banned(R.apply(z, [3, 3, 3], no_repeat_ngram_size=3)) == [3]                     # i = 0: (3, 3) == p, bans g[2]
    out = R.apply(z, [5, 7, 9, 5], no_repeat_ngram_size=2)
    keep = np.ones(len(z), bool)
    keep[7] = False
    assert np.array_equal(out[keep], z[keep])                                                # everything else bit-identical


def test_repetition_penalty_once_per_word_and_by_sign():
    z = _z()
    rho = np.float32(1.5)
    out = R.apply(z, [9, 9, 9, 9, 9, 1, 4], repetition_penalty=1.5)
    assert out[9] == z[9] / rho and z[9] > 0                          # five occurrences, penalised once
    assert out[1] == z[1] * rho and z[1] < 0                          # a negative logit is multiplied
    assert out[4] == 0.0 and z[4] == 0.0                              # zero: z * rho
    keep = np.ones(len(z), bool)
    keep[[9, 1, 4]] = False
    assert np.array_equal(out[keep], z[keep])
    assert np.array_equal(R.apply(z, [9, 1], repetition_penalty=1.0), z)
    assert out.dtype == np.float32
    # a penalty below 1 rewards: from z, not from z'
    assert R.apply(z, [9, 9], repetition_penalty=0.5)[9] == z[9] / np.float32(0.5)


def test_min_length_bad_words_and_the_order():
    z = _z()
    assert _banned(R.apply(z, [5] * 5, min_length=6)) == [R.END]           # t = m - 1
    assert _banned(R.apply(z, [5] * 6, min_length=6)) == []                # t = m
    assert _banned(R.apply(z, [], bad_words=[3, 8])) == [3, 8]
    # all four: a banned word stays banned whatever the penalty made of it
    out = R.apply(z, [9, 7, 9], repetition_penalty=2.0, no_repeat_ngram_size=2, bad_words=[7], min_length=4)
    assert _banned(out) == [R.END, 7]                                      # bigram (9, 7) bans 7 as well
    assert out[9] == z[9] / np.float32(2.0)
    rows = R.apply_rows(np.stack([z, z]), np.array([[1, 9, 7, 9], [1, 3, 3, 3]]), 3, {"no_repeat_ngram_size": 2})
    assert _banned(rows[0]) == [7] and _banned(rows[1]) == [3]
    assert R.holds([5, 7, 9, 2, 2], {"no_repeat_ngram_size": 1}) and not R.holds([5, 7, 5, 2], {"no_repeat_ngram_size": 1})
    assert not R.holds([5, 7, 5, 7, 2], {"no_repeat_ngram_size": 2}) and R.holds([5, 7, 7, 5, 2], {"no_repeat_ngram_size": 2})
    assert not R.holds([5, 2, 2], {"min_length": 2}) and R.holds([5, 6, 2], {"min_length": 2})
    assert not R.holds([5, 6, 2], {"bad_words": [6]}) and R.holds([5, 2, 6], {"bad_words": [6]})


# ---- host validation and neutral parsing ------------------------------------------------------------------------------------------
def _parse(**d):
    from audiocaption_amd.logit_rules import LogitRules
    return LogitRules.parse(d, 4981, 20, R.START, R.END)


def test_every_value_error():
    from audiocaption_amd.logit_rules import LogitRules
    for rho in (0, 0.0, -1.5, INF, float("nan"), "1.5", True, [1.5]):
        with pytest.raises(ValueError, match="repetition_penalty"):
            _parse(repetition_penalty=rho)
    for n in (-1, 21, 1.0, "2", True):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            _parse(no_repeat_ngram_size=n)
    for m in (-1, 21, 6.0, "6", False):
        with pytest.raises(ValueError, match="min_length"):
            _parse(min_length=m)
    for bad in ([[5, 6]], [5.0], ["dog"], "dog", 5, [-1], [4981], [True], [R.END], [R.START, 9], list(range(3, 260)),
                torch.zeros(2, 2, dtype=torch.int64), torch.tensor([5.0])):
        with pytest.raises(ValueError, match="bad_words"):
            _parse(bad_words=bad)
    assert len(_parse(bad_words=list(range(3, 259))).bad_words) == 256
    # a row could be banned completely: len(bad_words) + max_length + 1 >= V
    with pytest.raises(ValueError, match="vocabulary"):
        LogitRules.parse({"bad_words": list(range(3, 43))}, 61, 20, R.START, R.END)
    assert LogitRules.parse({"bad_words": list(range(3, 42))}, 61, 20, R.START, R.END).bad_words[-1] == 41
    with pytest.raises(ValueError, match="vocabulary"):
        LogitRules.parse({"no_repeat_ngram_size": 1}, 21, 20, R.START, R.END)
    # through the model, before anything is launched (the encoder is an Identity, the tensors are on the CPU)
    model = _trm_model()
    for over in ({"repetition_penalty": 0}, {"no_repeat_ngram_size": 7}, {"min_length": -1}, {"bad_words": [R.END]},
                 {"bad_words": [[3]]}):
        for method in ("greedy", "beam", "top5"):
            with pytest.raises(ValueError, match=next(iter(over))):
                model(_request(sample_method=method, **over))
            with pytest.raises(ValueError, match=next(iter(over))):
                model.forward_decoder(_request(sample_method=method, **over), {})


def test_neutral_parsing_and_the_key():
    from audiocaption_amd.logit_rules import LogitRules
    for d in ({}, {"repetition_penalty": None, "bad_words": None}, {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0,
                                                                   "bad_words": [], "min_length": 0},
              {"repetition_penalty": 1, "bad_words": ()}, {"bad_words": torch.zeros(0, dtype=torch.int64)}):
        assert _parse(**d).neutral, d
        assert _trm_model()._check_logit_rules(dict(_request(), **d)) is None
    a = _parse(repetition_penalty=1.5, no_repeat_ngram_size=2, bad_words=[7, 9], min_length=3)
    assert not a.neutral and a.key() == (2, 1.5, 3, (7, 9))
    assert a == _parse(repetition_penalty=1.5, no_repeat_ngram_size=2, bad_words=(7, 9), min_length=3)
    assert hash(a) == hash(_parse(repetition_penalty=1.5, no_repeat_ngram_size=2, bad_words=np.array([7, 9]), min_length=3))
    others = [_parse(repetition_penalty=1.25, no_repeat_ngram_size=2, bad_words=[7, 9], min_length=3),
              _parse(repetition_penalty=1.5, no_repeat_ngram_size=3, bad_words=[7, 9], min_length=3),
              _parse(repetition_penalty=1.5, no_repeat_ngram_size=2, bad_words=[7], min_length=3),
              _parse(repetition_penalty=1.5, no_repeat_ngram_size=2, bad_words=[7, 9], min_length=4)]
    assert len({a, *others}) == 5                       # every field is part of the key
    for k in ("repetition_penalty", "no_repeat_ngram_size", "bad_words", "min_length"):
        one = _parse(**{k: {"repetition_penalty": 1.5, "no_repeat_ngram_size": 2, "bad_words": [7], "min_length": 3}[k]})
        assert not one.neutral
    got = _trm_model()._check_logit_rules(_request(min_length=2))
    assert isinstance(got, LogitRules) and got.min_length == 2


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _trm_model():
    import audiocaption_amd as A
    return A.TransformerModel(torch.nn.Identity(), A.TransformerDecoder(**DEC)).eval()


def _request(**over):
    d = {"mode": "inference", "attn_emb": torch.zeros(3, 7, 64), "fc_emb": torch.zeros(3, 64),
         "attn_emb_len": torch.tensor([7, 3, 5]), "sample_method": "greedy", "max_length": 6}
    d.update(over)
    return d


RULES = ({"repetition_penalty": 1.5}, {"no_repeat_ngram_size": 2}, {"bad_words": [7]}, {"min_length": 3})
NEUTRAL = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "bad_words": [], "min_length": 0}


def test_surfaces_without_the_rules_name_the_key():
    import audiocaption_amd as A
    import _keyword_trm_ref as K
    import _attn_gru_train_ref as G
    from audiocaption_amd import logit_rules
    model = _trm_model()
    kdec = A.KeywordProbTransformerDecoder(**dict(K.SHAPES["d128"], dropout=0.2)).eval()
    kmodel = A.KeywordCondTransformerModel(torch.nn.Identity(), kdec).eval()
    attn, lens, kw = K.infer_inputs("d128")
    kbase = {"mode": "inference", "attn_emb": attn, "fc_emb": torch.zeros(K.B, 64), "attn_emb_len": lens, "keyword": kw}
    ens = A.EnsembleModel([_trm_model(), _trm_model()])
    amodels = [cls(torch.nn.Identity(), dec(dropout=0.0, **G.SMALL)).eval()
               for cls, dec in ((A.Seq2SeqAttnModel, A.rnn_decoder.BahAttnCatFcDecoder),
                                (A.TemporalSeq2SeqAttnModel, A.rnn_decoder.TemporalBahAttnDecoder))]
    for rule in RULES:
        key = next(iter(rule))
        for method in ("greedy", "beam"):
            with pytest.raises(NotImplementedError, match=key):
                model.forward_async(_request(sample_method=method, **rule))
            with pytest.raises(NotImplementedError, match=key):
                ens(_request(sample_method=method, **rule))
            with pytest.raises(NotImplementedError, match=key):
                kmodel(dict(kbase, sample_method=method, **rule))
            for amodel in amodels:
                with pytest.raises(NotImplementedError, match=key):
                    amodel(_request(sample_method=method, **rule))
                with pytest.raises(NotImplementedError, match=key):
                    amodel.forward_decoder(_request(sample_method=method, **rule), {})
        with pytest.raises(NotImplementedError, match="conditioned decoder"):
            A.TransformerDecoder.greedy(kdec, attn, lens, 6, 1, 2, 0, extra=kw,
                                        rules=logit_rules.LogitRules.parse(rule, 60, 6, 1, 2))
    # neutral values are accepted everywhere: the refusal does not fire (what follows it needs a GPU: any other error)
    assert logit_rules.first_active_key(NEUTRAL) is None and logit_rules.first_active_key({}) is None
    for call in (lambda: model.forward_async(_request(**NEUTRAL)), lambda: ens(_request(**NEUTRAL)),
                 lambda: kmodel(dict(kbase, **NEUTRAL)), lambda: amodels[0](_request(**NEUTRAL))):
        try:
            call()
        except NotImplementedError as e:       # pragma: no cover - would be the refusal
            pytest.fail(f"a neutral request was refused: {e}")
        except Exception:                      # noqa: BLE001 - no GPU here
            pass


def test_hf_surfaces_take_the_controls():
    import inspect
    from audiocaption_amd import hf_wrapper as H
    for cls in (H.CaptioningModel, H.Effb2TrmCaptioningModel, H.Cnn14RnnTempAttnGruModel):
        sig = inspect.signature(cls.forward).parameters
        assert [sig[k].default for k in R.KEYS] == [1.0, 0, (), 0], cls.__name__
    assert H._rules(1.0, 0, (), 0) == {} and H._rules(1.0, 0, [], 0) == {}
    assert H._rules(1.5, 2, [7], 3) == {"repetition_penalty": 1.5, "no_repeat_ngram_size": 2, "bad_words": [7], "min_length": 3}
    d = H._input_dict("cpu", torch.zeros(1, 8), [8], "greedy", 3, 20, 1.0, H._rules(1.0, 2, (), 0))
    assert d["no_repeat_ngram_size"] == 2 and "bad_words" not in d and "repetition_penalty" not in d
    # the attention-GRU HF class refuses before its tagger runs
    gru = object.__new__(H.Cnn14RnnTempAttnGruModel)
    for rule in RULES:
        with pytest.raises(NotImplementedError, match=next(iter(rule))):
            H.Cnn14RnnTempAttnGruModel.forward.__wrapped__(gru, torch.zeros(1, 8), [8], **rule)
    # CaptioningModel over a model without the rules passes the keys on, and that model names the key
    import audiocaption_amd as A
    import _attn_gru_train_ref as G
    amodel = A.Seq2SeqAttnModel(torch.nn.Identity(), A.rnn_decoder.BahAttnCatFcDecoder(dropout=0.0, **G.SMALL)).eval()
    with pytest.raises(NotImplementedError, match="bad_words"):
        H.CaptioningModel(amodel)(torch.zeros(1, 8), [8], sample_method="greedy", bad_words=[7])


def test_scst_baseline_stays_unconstrained():
    """ScstWrapper strips the four keys from its greedy baseline's request: the policy is the unconstrained search."""
    import audiocaption_amd as A
    seen = {}

    class Probe(A.TransformerModel):
        def forward(self, input_dict):
            seen.update(input_dict)
            raise RuntimeError("stop")

    w = A.ScstWrapper(Probe(torch.nn.Identity(), A.TransformerDecoder(**DEC)))
    with pytest.raises(RuntimeError, match="stop"):
        w._baseline({"wav": torch.zeros(1, 8), "wav_len": [8], "seed": 3, **{k: v for r in RULES for k, v in r.items()}}, 6)
    assert seen["sample_method"] == "greedy" and not any(k in seen for k in R.KEYS)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_rows_of_the_new_entry_points():
    from audiocaption_amd import _lib
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = dict(re.findall(r"\b(?:int|long)\s+(ac_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header))
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in protos, name
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name][1]), name
    fields = re.search(r"typedef struct \{([^}]*)\}\s*ac_logit_rules;", header).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.AcLogitRules._fields_]
    assert ctypes.sizeof(_lib.AcLogitRules) == 32 and _lib.AcLogitRules.bad_words.offset == 24
    from audiocaption_amd import build
    assert "logit_rules.hip" in build.SOURCES


def test_argument_refusals_launch_nothing():
    """AC_ERR_ARG before any HIP call: these run on a machine without a GPU."""
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    a = ctypes.c_void_p(4096)       # never dereferenced: every call below is refused on its arguments

    def rules(rho=1.5, n=2, m=0, end=2, n_bad=0, bad=None):
        return ctypes.byref(_lib.AcLogitRules(rho, n, m, end, n_bad, bad))

    def call(r, V=100, ld_in=100, ld_out=100, rows=4, ld_tok=21, t=3, src=a, dst=a, tok=a):
        return lib.ac_logit_rules_apply(src, ld_in, dst, ld_out, rows, V, tok, ld_tok, t, r, None)

    assert call(rules(), V=16385, ld_in=16385, ld_out=16385) == _lib.AC_ERR_ARG
    assert call(rules(), t=-1) == _lib.AC_ERR_ARG and call(rules(), t=21) == _lib.AC_ERR_ARG     # outside the token row
    assert call(rules(n_bad=257, bad=4096)) == _lib.AC_ERR_ARG and call(rules(n_bad=3, bad=None)) == _lib.AC_ERR_ARG
    for rho in (0.0, -1.0, INF, float("nan")):
        assert call(rules(rho=rho)) == _lib.AC_ERR_ARG
    assert call(rules(n=-1)) == _lib.AC_ERR_ARG and call(rules(m=-1)) == _lib.AC_ERR_ARG
    assert call(rules(end=100)) == _lib.AC_ERR_ARG and call(rules(end=-1)) == _lib.AC_ERR_ARG
    assert call(rules(), ld_in=99) == _lib.AC_ERR_ARG and call(rules(), ld_out=99) == _lib.AC_ERR_ARG
    assert call(rules(), rows=0) == _lib.AC_ERR_ARG and call(None) == _lib.AC_ERR_ARG
    assert call(rules(), src=None) == _lib.AC_ERR_ARG and call(rules(), dst=None) == _lib.AC_ERR_ARG
    assert call(rules(), tok=None) == _lib.AC_ERR_ARG
    w = _lib.AcTrmWeights()          # a zeroed configuration is refused first
    assert lib.ac_trm_search_rules(ctypes.byref(w), a, a, 4, 1, 7, 20, 1, 2, 0, a, a, a, a, a, a, -1, 0, 0.0, 1.0, None,
                                   rules(), a, 100, None) == _lib.AC_ERR_ARG
    assert lib.ac_trm_search_rules(ctypes.byref(w), a, a, 4, 1, 7, 20, 1, 2, 0, a, a, a, a, a, a, -1, 0, 0.0, 1.0, None,
                                   None, a, 100, None) == _lib.AC_ERR_ARG
    assert lib.ac_trm_beam_step_rules(ctypes.byref(w), a, a, 4, 3, 7, 20, 0, 1.0, a, a, a, a, a, a, None, a,
                                      None) == _lib.AC_ERR_ARG


# ---- the reference searches on the four memories -----------------------------------------------------------------------------------
def _captions(res):
    seq = res["seq"]
    return seq.reshape(-1, seq.shape[-1])


@pytest.mark.parametrize("method", R.METHODS)
def test_reference_searches_hold_the_rules_and_are_admissible(method):
    for name in R.CASES:
        res, off, _ = R.reference(method, name)
        rules = R.case(name, method)
        assert all(R.holds(c, rules) for c in _captions(res)), (method, name)
        margin = res["gap"] if method == "greedy" else res["cut"]
        assert margin > 1e-3, f"{method} {name}: the inputs come within {margin} of a tie"
        base = off["gap"] if method == "greedy" else off["cut"]
        assert base > 1e-3, f"{method} unconstrained on the memories of {name}: within {base} of a tie"


def test_each_rule_is_active_in_the_greedy_search():
    """The constrained caption differs from the unconstrained one in at least 2 of the 4 clips - for n = 2 in clip 2, the
    one whose unconstrained caption repeats bigrams; min_length = 6 lengthens clip 0, which ends after 3 words."""
    changed = {}
    for name in R.ACTIVE:
        res, off, _ = R.reference("greedy", name)
        assert R.roll_of("greedy", name) == 0
        changed[name] = (res["seq"] != off["seq"]).any(1)
    off = R.search("greedy", "off", 0)["seq"]
    assert [int(w) for w in off[0, :4]] == [2125, 3158, 4835, R.END]                  # clip 0 ends after 3 words
    grams = [tuple(off[2, i:i + 2]) for i in range(18)]
    assert len(grams) - len(set(grams)) >= 5 and len(set(off[2, :19].tolist())) == 9    # clip 2: 9 distinct words in 19
    assert not R.holds(off[2], {"no_repeat_ngram_size": 2}) and not R.holds(off[2], {"no_repeat_ngram_size": 1})
    for name in ("n1", "rho", "bad"):
        assert changed[name].sum() >= 2, (name, changed[name])
    assert changed["n2"][2] and changed["min6"][0]
    assert changed["bad"].all()                                  # every clip's first word is banned
    res = R.search("greedy", "min6", 0)["seq"]
    assert R.END not in res[0, :6].tolist()
    # rho = 1.5 never bans: the penalised words may come back, fewer than before
    rho = R.search("greedy", "rho", 0)["seq"]
    assert len(set(rho[2, :16].tolist())) > 9


def test_each_rule_is_active_in_the_beam_searches():
    for method in ("beam2", "beam3"):
        for name in R.ACTIVE:
            res, off, _ = R.reference(method, name)
            n = int((res["seq"][:, 0] != off["seq"][:, 0]).any(1).sum())
            if (method, name) == ("beam3", "n2"):    # beam 3 already avoids the repeated bigrams wherever it is admissible
                continue
            assert n >= 2, (method, name, n)
