"""Group (diverse) beam search, the parts that need no GPU: every refusal of the request (raised on the host, before an
encoder or a kernel runs), the routing of ``sample_method="beam"`` with and without ``group_size``, the restatement
(tests/_group_beam_ref.py) against the reference's results in tests/golden/g_group_beam.npz with the tie guards that make
the GPU comparison of ids meaningful, the properties of the restatement, and the header / ctypes / build rows of
``ac_group_beam_select`` with its argument refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _group_beam_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC = dict(emb_dim=128, vocab_size=60, fc_emb_dim=64, attn_emb_dim=64, dropout=0.2, nhead=2, dim_feedforward=256)


def _trm_model(**over):
    import audiocaption_amd as A
    return A.TransformerModel(torch.nn.Identity(), A.TransformerDecoder(**dict(DEC, **over))).eval()


def _request(**over):
    d = {"mode": "inference", "attn_emb": torch.zeros(3, 7, 64), "fc_emb": torch.zeros(3, 64),
         "attn_emb_len": torch.tensor([7, 3, 5]), "sample_method": "beam", "max_length": 6, "group_size": 3}
    d.update(over)
    return d


# ---- the request ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,word", [
    (dict(group_size=0), "group_size"), (dict(group_size=9), "group_size"), (dict(group_size=2.0), "group_size"),
    (dict(group_size="3"), "group_size"), (dict(group_size=True), "group_size"), (dict(group_size=-1), "group_size"),
    (dict(group_size=3, beam_size=2), "beam_size"),            # bdash 0
    (dict(group_size=1, beam_size=9), "beam_size"),            # bdash 9
    (dict(group_size=8, beam_size=72), "beam_size"),
    (dict(group_size=2, beam_size=4.0), "beam_size"),
    (dict(group_size=7), "beam_size"),                         # the default beam_size 6 // 7 = 0
    (dict(diversity_lambda=-0.5), "diversity_lambda"), (dict(diversity_lambda=float("nan")), "diversity_lambda"),
    (dict(diversity_lambda=float("inf")), "diversity_lambda"), (dict(diversity_lambda="0.5"), "diversity_lambda"),
    (dict(diversity_lambda=True), "diversity_lambda"),
    (dict(group_nbest=1), "group_nbest"), (dict(group_nbest="yes"), "group_nbest"),
    (dict(n_best=True), "n_best"), (dict(n_best=False), "n_best"), (dict(n_best_size=2), "n_best_size"),
    (dict(temp=0.0), "temp"), (dict(temp=float("nan")), "temp"),
    (dict(sample_method="greedy"), "group_size"), (dict(sample_method="top5"), "group_size"),
])
def test_bad_requests_are_value_errors_before_anything_runs(over, word):
    model = _trm_model()
    model.encoder = _Refuser()
    with pytest.raises(ValueError, match=word):
        model(_request(**over))
    with pytest.raises(ValueError, match=word):
        model.forward_decoder(_request(**over), {})


class _Refuser(torch.nn.Module):
    """An encoder that must not be reached."""

    def forward(self, input_dict):
        raise AssertionError("the encoder ran before the request was checked")


def test_vocabulary_above_8192_is_a_value_error():
    model = _trm_model(vocab_size=8193)
    model.encoder = _Refuser()
    with pytest.raises(ValueError, match="8192"):
        model(_request())


def test_every_other_surface_names_group_size():
    import audiocaption_amd as A
    import _keyword_trm_ref as K
    import _attn_gru_train_ref as T
    model = _trm_model()
    with pytest.raises(NotImplementedError, match="group_size"):
        model.forward_async(_request())
    with pytest.raises(NotImplementedError, match="group_size"):
        model.forward_async(_request(sample_method="greedy"))
    for rule in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(bad_words=[5]), dict(min_length=2)):
        with pytest.raises(NotImplementedError, match="group_size"):
            model(_request(**rule))
    kdec = A.KeywordProbTransformerDecoder(**dict(K.SHAPES["d128"], dropout=0.2)).eval()
    kmodel = A.KeywordCondTransformerModel(torch.nn.Identity(), kdec).eval()
    attn, lens, kw = K.infer_inputs("d128")
    base = {"mode": "inference", "attn_emb": attn, "fc_emb": torch.zeros(K.B, 64), "attn_emb_len": lens, "keyword": kw}
    with pytest.raises(NotImplementedError, match="group_size"):
        kmodel(dict(base, sample_method="beam", group_size=2))
    for cls, dec in ((A.Seq2SeqAttnModel, A.rnn_decoder.BahAttnCatFcDecoder),
                     (A.TemporalSeq2SeqAttnModel, A.rnn_decoder.TemporalBahAttnDecoder)):
        amodel = cls(torch.nn.Identity(), dec(dropout=0.0, **T.SMALL)).eval()
        with pytest.raises(NotImplementedError, match="group_size"):
            amodel(_request())
        with pytest.raises(NotImplementedError, match="group_size"):
            amodel.forward_decoder(_request(), {})
    ens = A.EnsembleModel([_trm_model(), _trm_model()])
    with pytest.raises(NotImplementedError, match="group_size"):
        ens(_request())
    with pytest.raises(NotImplementedError, match="dbs"):       # the name stays refused, with or without the keys
        model(_request(sample_method="dbs"))


def test_neutral_logit_rules_are_accepted_beside_group_size():
    model = _trm_model()
    assert model._check_group_beam(_request(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words=[], min_length=0)) == \
        (3, 2, 0.5, True)


def test_defaults_follow_the_reference():
    model = _trm_model()
    assert model._check_group_beam(_request()) == (3, 2, 0.5, True)
    assert model._check_group_beam(_request(group_size=2, beam_size=7, diversity_lambda=2, group_nbest=False)) == \
        (2, 3, 2.0, False)
    assert model._check_group_beam(_request(group_size=None)) is None
    d = model._inference_dict(_request(), {})
    assert (d["beam_size"], d["group_size"], d["diversity_lambda"], d["group_nbest"]) == (6, 3, 0.5, True)
    plain = _request()
    del plain["group_size"]
    for req in (plain, _request(group_size=None)):
        d = model._inference_dict(req, {})
        assert d["beam_size"] == 3 and not {"group_size", "diversity_lambda", "group_nbest"} & set(d)
    d = model._inference_dict(_request(sample_method="greedy", group_size=None, diversity_lambda=0.7), {})
    assert not {"group_size", "diversity_lambda", "group_nbest", "beam_size"} & set(d)


def test_beam_without_group_size_takes_the_plain_beam_search(monkeypatch):
    model = _trm_model()
    calls = []
    monkeypatch.setattr(model, "beam_search", lambda d: calls.append(("beam", d)) or {"seq": None})
    monkeypatch.setattr(model, "group_beam_search", lambda d: calls.append(("group", d)) or {"seq": None})
    plain = _request()
    del plain["group_size"]
    model(plain)
    model(_request(group_size=None))
    model(_request(group_size=None, diversity_lambda=0.9, group_nbest=False))     # keys nobody reads without group_size
    assert [c[0] for c in calls] == ["beam"] * 3
    assert all(d["beam_size"] == 3 and d["n_best"] is False and d["n_best_size"] == 3 for _, d in calls)
    model(_request())
    model(_request(group_size=1, beam_size=4))
    assert [c[0] for c in calls[3:]] == ["group"] * 2
    assert calls[-1][1]["group_size"] == 1 and calls[-1][1]["beam_size"] == 4


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced():
    """Every case of the fixture through the restatement once: id -> (seq, trace)."""
    out = {}
    with torch.no_grad():
        for case in R.CASES:
            trace = []
            out[case[0]] = (R.run_case(case, R.case_clips(case[0]), trace=trace)["seq"], trace)
    return out


def test_fixture_lists_the_cases_of_the_module():
    f = R.fixture()
    assert list(f["cases"]) == R.CASE_IDS
    np.testing.assert_array_equal(f["case_params"], np.array([c[1:] for c in R.CASES], dtype=np.float64))
    for case in R.CASES:
        spec = R.case_clips(case[0])
        assert len(spec) == R.CLIPS_PER_CASE <= 4 and any(ln == 1 for _, ln in spec), case[0]
        assert f[f"{case[0]}/seq"].shape == (len(spec), case[3], case[6])
        assert f[f"{case[0]}/seq_best"].shape == (len(spec), case[1], case[6])


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_restatement_reproduces_the_reference(case, traced):
    f = R.fixture()
    np.testing.assert_array_equal(traced[case[0]][0].numpy(), f[f"{case[0]}/seq"])
    with torch.no_grad():
        best = R.run_case(case, R.case_clips(case[0]), group_nbest=False)["seq"]
    np.testing.assert_array_equal(best.numpy(), f[f"{case[0]}/seq_best"])
    G, bdash, beam = case[1:4]
    assert (f[f"{case[0]}/seq"][:, G * bdash:] == R.END).all()                 # rows beyond G * bdash stay end_idx
    np.testing.assert_array_equal(f[f"{case[0]}/seq_best"], f[f"{case[0]}/seq"][:, 0:G * bdash:bdash])


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_cases_have_no_near_ties(case, traced):
    """Every gap among the kept candidates and to the first cut >= 1e-3, the finished scores that decide a group's top
    bdash >= 2e-4 apart: the ids of the GPU search are a meaningful comparison, never a flaky one."""
    margin, gap = R.guards(traced[case[0]][1], case[2])
    print(f"{case[0]}: margin {margin:.3e}, score gap {gap:.3e}")
    assert margin >= R.MARGIN and gap >= R.SCORE_GAP
    stored = R.fixture()[f"{case[0]}/gaps"]
    assert abs(stored[0] - margin) <= 1e-9 + 1e-6 * margin


def test_other_lambda_of_the_cached_state_test_has_no_near_ties():
    case, trace = R.CASES[0], []
    with torch.no_grad():
        seq = R.run_case(case, R.case_clips(case[0]), trace=trace, diversity_lambda=R.OTHER_LAMBDA)["seq"]
    margin, gap = R.guards(trace, case[2])
    assert margin >= R.MARGIN and gap >= R.SCORE_GAP
    assert not np.array_equal(seq.numpy(), R.fixture()[f"{case[0]}/seq"])


def test_lambda_zero_gives_every_group_the_captions_of_group_zero():
    case, spec = R.CASES[0], R.case_clips(R.CASES[0][0])[:2]
    with torch.no_grad():
        seq = R.run_case(case, spec, diversity_lambda=0.0)["seq"]
    G, bdash = case[1], case[2]
    for g in range(1, G):
        np.testing.assert_array_equal(seq[:, g * bdash:(g + 1) * bdash].numpy(), seq[:, :bdash].numpy())
    with torch.no_grad():
        assert not torch.equal(R.run_case(case, spec)["seq"][:, bdash:2 * bdash], seq[:, :bdash])   # lambda 0.5 does differ


def test_group_zero_is_the_plain_search_of_its_own_width():
    """Group 0 of any G is the G = 1 search with beam_size = bdash, and that is oracle.cpu_path.beam_search's n-best list
    wherever no clip retires early in the latter (a clip that retires has fewer finished beams, never other ones)."""
    case, spec = R.CASES[0], R.case_clips(R.CASES[0][0])
    G, bdash, L, V = case[1], case[2], case[6], case[7]
    with torch.no_grad():
        full = R.run_case(case, spec)["seq"]
        alone = R.run_case(case, spec, group_size=1, beam_size=bdash)["seq"]
    np.testing.assert_array_equal(full[:, :bdash].numpy(), alone.numpy())
    emb, lens = R.clips(spec)
    with torch.no_grad():
        plain = R.O.beam_search(R.state(V), emb, lens, bdash, L, case[5])["seq"]
    np.testing.assert_array_equal(alone[:, 0].numpy(), plain.numpy())


def test_max_length_below_group_size():
    case = R.CASES[2]
    assert case[6] == 1 and case[1] == 3
    trace = []
    with torch.no_grad():
        seq = R.run_case(case, R.case_clips(case[0]), trace=trace)["seq"]
    assert seq.shape == (3, 3, 1)
    assert sorted({(r["g"], r["lt"]) for r in trace}) == [(0, 0), (1, 0), (2, 0)]
    spec = R.case_clips(case[0])
    emb, lens = R.clips(spec)
    step = R.decoder_step(R.state(case[7]), emb, lens)
    for i in range(3):                       # by hand: group g takes the best word after lambda per earlier choice of it
        with torch.no_grad():
            lp = torch.log_softmax(torch.log_softmax(step(i, torch.zeros(1, 0, dtype=torch.long)), 1) / case[5], 1)[0]
        for g in range(3):
            pen = lp.clone()
            for q in range(g):
                pen[seq[i, q, 0]] -= case[4]
            assert int(pen.argmax()) == int(seq[i, g, 0]), (i, g)


def test_group_steps_and_prev_planes_follow_the_reference_loop():
    from audiocaption_amd import search_state
    assert search_state.group_steps(3, 1) == [(0, 0), (1, 0), (2, 0)]
    assert search_state.group_steps(2, 3) == [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (1, 2)]
    assert len(search_state.group_steps(8, 20)) == 160
    L = 3
    books = [{"tok": [torch.zeros(2, L + 1, dtype=torch.int32) for _ in range(2)]} for _ in range(3)]
    assert search_state.group_prev_planes(books, 0, 1, L) is None
    p = search_state.group_prev_planes(books, 2, 1, L)
    # group 0 has finished its last step (2: plane 1), group 1 its step 2 as well (min(1 + 1, 2) = 2: plane 1)
    assert list(p) == [books[0]["tok"][1].data_ptr(), books[1]["tok"][1].data_ptr()]
    p = search_state.group_prev_planes(books, 2, 0, L)
    assert list(p) == [books[0]["tok"][1].data_ptr(), books[1]["tok"][0].data_ptr()]   # steps 2 and 1


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_build_rows():
    from audiocaption_amd import _lib, build
    assert "group_beam.hip" in build.SOURCES and _lib.ABI_VERSION == 2
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    assert "#define AC_GROUP_BEAM_MAX_GROUPS 8" in header
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = dict(re.findall(r"\b(?:int|long)\s+(ac_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body))
    args = [a.strip() for a in protos["ac_group_beam_select"].split(",")]
    res, sig = _lib.SIGNATURES["ac_group_beam_select"]
    assert res is ctypes.c_int and len(args) == len(sig) == 16
    want = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for a, s in zip(args, sig):
        assert s is (ctypes.c_void_p if "*" in a else want[a.split()[0]]), a
    assert args[9] == "const int* const* prev_tok" and args[10] == "int n_prev" and args[11] == "long tok_ld"


def _select(lib, **over):
    P = ctypes.c_void_p(0x7f0000001000)          # never dereferenced on the host
    a = dict(logit=P, ldl=100, B=2, bdash=3, V=100, lt=1, temp=1.0, lam=0.5, cum=P,
             prev=(ctypes.c_void_p * 2)(0x7f0000002000, 0x7f0000003000), n_prev=2, tok_ld=21, top_val=P, top_idx=P, scratch=P)
    a.update(over)
    return lib.ac_group_beam_select(a["logit"], a["ldl"], a["B"], a["bdash"], a["V"], a["lt"], a["temp"], a["lam"], a["cum"],
                                    a["prev"], a["n_prev"], a["tok_ld"], a["top_val"], a["top_idx"], a["scratch"], None)


REFUSED = [dict(bdash=0), dict(bdash=9), dict(n_prev=-1), dict(n_prev=8), dict(V=0), dict(V=8193, ldl=8193), dict(ldl=99),
           dict(lt=-1), dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")), dict(temp=float("inf")), dict(lam=-0.1),
           dict(lam=float("nan")), dict(lam=float("inf")), dict(logit=None), dict(cum=None), dict(top_val=None),
           dict(top_idx=None), dict(scratch=None), dict(prev=None), dict(prev=(ctypes.c_void_p * 2)(0x7f0000002000, None)),
           dict(B=0), dict(tok_ld=2), dict(V=2, ldl=2)]


@pytest.mark.parametrize("over", REFUSED, ids=[",".join(f"{k}={v}" if not hasattr(v, "_length_") else k for k, v in o.items())
                                               for o in REFUSED])
def test_select_refuses_bad_arguments_without_a_gpu(over):
    from audiocaption_amd import _lib, build
    build.build()
    assert _select(_lib.load(), **over) == _lib.AC_ERR_ARG
