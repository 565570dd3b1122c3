"""The attention-GRU decoder family on the CPU: tests/_attn_gru_ref.py (the restatement the GPU tests rely on) against the
reference's recorded outputs, tests/golden/g19_attn_gru.npz - identical ids, values within 1e-4 -
and the Python surface that needs no device: strict state_dict loading, the refusals, compat.install().

What in g19 is the reference's own: every id, the greedy values / top-8 logits / logit columns / attention weights / final
state, the beam attention weights, the sampling distributions and stored values.  The beam margins are the restatement's."""
import os
import sys

import numpy as np
import pytest
import torch

import _attn_gru_ref as R
import _sampling_ref as SR
from audiocaption_amd import procedural as P

SHAPES, CASES, load_g19, case_inputs = R.SHAPES, R.CASES, R.load_g19, R.case_inputs


@pytest.fixture(scope="module")
def g19():
    return load_g19()


@torch.no_grad()
@pytest.mark.parametrize("case", CASES)
def test_greedy(g19, case):
    sd, mem, lens, fc, tags = case_inputs(g19, case)
    out = R.greedy(sd, mem, lens, fc, tags, int(g19["max_length"]))
    np.testing.assert_array_equal(out["seq"].numpy(), g19[case + "_greedy_seq"])
    live = g19[case + "_greedy_live"]
    np.testing.assert_array_equal(R.live_mask(out["seq"].numpy()), live)
    tv, ti = out["logit"].topk(8, dim=2)
    np.testing.assert_array_equal((ti.numpy() * live[..., None]), g19[case + "_greedy_top_idx"])
    cols = g19["logit_cols"].tolist()
    for name, got, want in (("value", out["sampled_logprob"], g19[case + "_greedy_value"]),
                            ("top_val", tv * torch.from_numpy(live)[..., None], g19[case + "_greedy_top_val"]),
                            ("logit columns", out["logit"][:, :, cols], g19[case + "_greedy_logit_cols"]),
                            ("attn_weight", out["attn_weight"], g19[case + "_greedy_attn_weight"]),
                            ("state", out["state"], g19[case + "_greedy_state"])):
        d = float(np.abs(got.numpy() - want).max())
        print(f"{case} greedy {name}: max |restatement - fixture| {d:.3e}")
        assert d < 1e-4, name
    assert float(g19[case + "_greedy_gap"]) >= 1e-4
    # the reference's own loop (stop=False) writes finished rows as well; up to each row's first <end> the two agree
    ref_loop = R.greedy(sd, mem, lens, fc, tags, int(g19["max_length"]), stop=False)
    assert torch.equal(ref_loop["seq"], out["seq"]) and ref_loop["steps"] == out["steps"]
    assert torch.equal(ref_loop["state"], out["state"])
    assert float((ref_loop["logit"] - out["logit"])[torch.from_numpy(live)].abs().max()) == 0.0


@torch.no_grad()
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("case", CASES)
def test_beam(g19, case, k):
    sd, mem, lens, fc, tags = case_inputs(g19, case)
    L = int(g19["max_length"])
    trace = []
    out = R.beam_search(sd, mem, lens, fc, tags, k, L, trace=trace)
    np.testing.assert_array_equal(out["seq"].numpy(), g19[f"{case}_beam{k}_seq"])
    d = float(np.abs(out["attn_weight"].numpy() - g19[f"{case}_beam{k}_attn_weight"]).max())
    print(f"{case} beam {k} attn_weight: max |restatement - fixture| {d:.3e}")
    assert d < 1e-4
    steps = [max(r["t"] for r in trace if r["clip"] == i) + 1 for i in range(mem.shape[0])]
    assert steps == g19[f"{case}_beam{k}_steps"].tolist()
    for i, n in enumerate(steps):   # the columns a clip's search never reached are 0
        assert not out["attn_weight"][i, :, n:].any()
    nb = R.beam_search(sd, mem, lens, fc, tags, k, L, n_best=True, n_best_size=k)
    np.testing.assert_array_equal(nb["seq"].numpy(), g19[f"{case}_beam{k}_nbest"])
    assert float(g19[f"{case}_beam{k}_margin"]) >= 1e-4


def test_fixture_covers_what_can_go_wrong(g19):
    steps = g19["pub_t_beam3_steps"]
    assert steps.min() < int(g19["max_length"]) == steps.max()      # one clip exits early, one runs to max_length
    for case in CASES:
        ends = g19[case + "_greedy_live"].sum(1)
        assert len(set(ends.tolist())) > 1 and ends.min() > 1, case   # rows end at different steps, none is <end> alone


def test_sampling_rules(g19):
    """_sampling_ref (the restatement of the on-device sampler) against the reference's rules on fixed logits."""
    rows, seed = (int(v) for v in g19["sample_recipe"])
    logits = np.random.default_rng(seed).normal(0.0, 2.5, (rows, 4981)).astype(np.float32)
    for ci, (method, temp) in enumerate(zip(g19["sample_methods"].tolist(), g19["sample_temps"].tolist())):
        code, k, p = R.parse_method(method)
        for r in range(rows):
            w, stored, _ = SR.distribution(logits[r], code, k, p, temp)
            want = g19["sample_dist"][ci, r]
            np.testing.assert_array_equal(w > 0, np.isfinite(want))
            kept = w > 0
            got = np.log(w[kept] / w.sum())
            ref = torch.log_softmax(torch.from_numpy(want[kept]).double(), 0).numpy()
            assert float(np.abs(got - ref).max()) < 1e-5, (method, r)
            word = int(g19["sample_word"][ci, r])
            assert abs(stored[word] - float(g19["sample_value"][ci, r])) < 1e-5, (method, r)


def test_strict_state_dict_load(g19):
    """A reference state_dict - exactly its key list and shapes, as recorded - loads with strict=True."""
    from audiocaption_amd import TemporalBahAttnDecoder
    keys = g19["state_keys"].tolist()
    shapes = {k: tuple(int(v) for v in s.split(",")) for k, s in zip(keys, g19["state_shapes"].tolist())}
    assert {"word_embedding.weight", "model.weight_ih_l0", "model.weight_hh_l0", "model.bias_ih_l0", "model.bias_hh_l0",
            "attn.h2attn.weight", "attn.h2attn.bias", "attn.v", "fc_proj.weight", "fc_proj.bias", "ctx_proj.weight",
            "ctx_proj.bias", "classifier.weight", "classifier.bias", "temporal_embedding.weight"} == set(keys)
    dec = TemporalBahAttnDecoder(dropout=0.5, **SHAPES["pub"])
    own = dec.state_dict()
    assert sorted(own.keys()) == sorted(keys)
    assert {k: tuple(v.shape) for k, v in own.items()} == shapes
    sd = P.to_torch(P.bah_decoder_state(**SHAPES["pub"]))
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    dec.load_state_dict(sd, strict=True)
    assert torch.equal(dec.attn.h2attn.weight, sd["attn.h2attn.weight"])


def _small(cls_name="TemporalBahAttnDecoder", **kw):
    import audiocaption_amd as A
    return getattr(A, cls_name)(dropout=0.2, **dict(SHAPES["small"], **kw))


@pytest.mark.parametrize("kw", [dict(rnn_type="LSTM"), dict(num_layers=2), dict(bidirectional=True), dict(d_model=100),
                                dict(attn_size=2048), dict(vocab_size=16385)])
def test_constructor_refusals(kw):
    with pytest.raises(NotImplementedError):
        _small(**kw)
    with pytest.raises(NotImplementedError):
        _small("BahAttnCatFcDecoder", **kw)


def _request(**kw):
    d = {"mode": "inference", "attn_emb": torch.zeros(2, 5, 160), "fc_emb": torch.zeros(2, 96),
         "attn_emb_len": torch.tensor([5, 3]), "temporal_tag": torch.tensor([0, 3])}
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


def test_model_refusals():
    import audiocaption_amd as A
    model = A.TemporalSeq2SeqAttnModel(torch.nn.Identity(), _small())
    for tag in (None, [0, 4], [-1, 0], [0], [0.0, 1.0], [0, 1, 2]):
        for method in ("greedy", "beam", "sample"):
            with pytest.raises(ValueError, match="temporal_tag"):
                model(_request(temporal_tag=tag, sample_method=method))
    with pytest.raises(NotImplementedError, match="dbs"):
        model(_request(sample_method="dbs"))
    with pytest.raises(NotImplementedError, match="train"):
        model(_request(mode="train"))
    with pytest.raises(NotImplementedError, match="forward_async"):
        model.forward_async(_request())
    with pytest.raises(NotImplementedError, match="TransformerModel"):
        A.ScstWrapper(model)
    with pytest.raises(NotImplementedError, match="TransformerDecoder"):
        A.EnsembleModel([model])
    with pytest.raises(AssertionError, match="incompatible"):
        A.TemporalSeq2SeqAttnModel(torch.nn.Identity(), _small("BahAttnCatFcDecoder"))
    with pytest.raises(NotImplementedError, match="TemporalSeq2SeqAttnModel"):
        A.Seq2SeqAttnModel(torch.nn.Identity(), _small())
    with pytest.raises(AssertionError, match="incompatible"):
        A.TransformerModel(torch.nn.Identity(), _small())


def test_cpu_tensor_is_refused():
    """No CPU fallback: a request on CPU tensors raises HipLibraryError, for every search and for the decoder step."""
    import audiocaption_amd as A
    from audiocaption_amd._lib import HipLibraryError
    model = A.TemporalSeq2SeqAttnModel(torch.nn.Identity(), _small())
    for method in ("greedy", "beam", "top5"):
        with pytest.raises(HipLibraryError):
            model(_request(sample_method=method))
    plain = A.Seq2SeqAttnModel(torch.nn.Identity(), _small("BahAttnCatFcDecoder"))
    with pytest.raises(HipLibraryError):
        plain(_request(temporal_tag=None))
    with pytest.raises(HipLibraryError):
        plain.decoder({"word": torch.ones(2, 1, dtype=torch.long), "fc_emb": torch.zeros(2, 96),
                       "attn_emb": torch.zeros(2, 5, 160), "attn_emb_len": torch.tensor([5, 3])})


def test_compat_resolves_the_reference_paths():
    import audiocaption_amd as A
    from audiocaption_amd import compat
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] == "captioning"}
    try:
        compat.install()
        import importlib
        assert importlib.import_module("captioning.models.rnn_decoder").TemporalBahAttnDecoder is A.TemporalBahAttnDecoder
        assert importlib.import_module("captioning.models.rnn_decoder").BahAttnCatFcDecoder is A.BahAttnCatFcDecoder
        assert importlib.import_module("captioning.models.attn_model").TemporalSeq2SeqAttnModel is A.TemporalSeq2SeqAttnModel
        assert importlib.import_module("captioning.models.attn_model").Seq2SeqAttnModel is A.Seq2SeqAttnModel
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] == "captioning"]:   # the aliases only: nothing else is unloaded
            del sys.modules[k]
        sys.modules.update(saved)
