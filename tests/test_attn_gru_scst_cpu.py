"""CPU tests of self-critical sequence training for the attention-GRU captioners: the restatement
(tests/_attn_gru_scst_ref.py) against what the reference ran (tests/golden/g23_attn_gru_scst.npz), the sampler seed the GPU
pick test uses, and what ``ScstWrapper`` accepts and refuses without a device."""
import numpy as np
import pytest
import torch

import _attn_gru_scst_ref as S
import _attn_gru_train_ref as R
import _scst_ref as SC

LOGIT_BAR, LOSS_BAR, GRAD_BAR = 2e-5, 2e-5, 1e-4


@pytest.fixture(scope="module")
def g23():
    return S.load_g23()


@pytest.fixture(scope="module")
def g22():
    return R.load_g22()


def _grads_vs_fixture(g23, g22, prefix, grads):
    bad = []
    for key, grad in grads.items():
        gn = float(g23[f"{prefix}_gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g22[f"{prefix}_sample_idx/{key}"])].numpy()
        d_s = float(np.abs(sample - g23[f"{prefix}_gsample/{key}"]).max()) / (float(grad.abs().max()) + 1e-12)
        if not (d_norm < GRAD_BAR and d_s < GRAD_BAR):
            bad.append((key, d_norm, d_s))
    assert not bad, bad


def _fixture_can_fail(sampled, greedy):
    T = sampled.shape[1]
    ended = sampled == SC.END
    first = np.where(ended.any(1), ended.argmax(1), T)
    assert (first < T - 1).any() and (first == T).any() and int((sampled != greedy).any(1).sum()) >= 3


@pytest.mark.parametrize("kind", ["t", "p"])
def test_restatement_vs_reference_decoder(g23, g22, kind):
    temporal, case = kind == "t", f"small_{kind}"
    sd = R.small_state(temporal, *g23[f"{case}_recipe"])
    mem, lens, fc, tags = R.small_inputs()
    words = torch.from_numpy(g23[f"{case}_seq"])
    _fixture_can_fail(g23[f"{case}_seq"], g23[f"{case}_greedy_seq"])
    reward = g23["small_reward"]
    assert (reward > 0).any() and (reward < 0).any()
    o = S.decoder_scst_grads(sd, mem, lens, fc, S.T, S.TEMP, reward, tags if temporal else None, words=words)
    assert torch.equal(o["seq"], words)
    top_val, top_idx = o["logit"].topk(8, dim=-1)
    want = g23[f"{case}_logit_top_val"]
    assert float(np.abs(top_val.numpy() - want).max()) < LOGIT_BAR * float(np.abs(want).max())
    assert np.array_equal(top_idx.numpy()[..., 0], g23[f"{case}_logit_top_idx"][..., 0])
    mask = SC.mask_of(words).numpy()
    assert float(np.abs(o["sampled_logprob"].numpy() - g23[f"{case}_sampled_logprob"])[mask].max()) < 1e-5
    assert abs(float(o["loss"]) - float(g23[f"{case}_loss"])) < LOSS_BAR * float(o["scale"])
    named = {"decoder." + k: v for k, v in o["grads"].items()}
    named.update(attn_emb=o["d_attn_emb"], fc_emb=o["d_fc_emb"])
    assert set(named) == {k.split("/", 1)[1] for k in g23 if k.startswith(f"{case}_gnorm/")}
    _grads_vs_fixture(g23, g22, case, named)
    seq, gap = S.greedy(sd, mem, lens, fc, S.T, tags if temporal else None)
    assert np.array_equal(seq.numpy(), g23[f"{case}_greedy_seq"])


def test_restatement_vs_reference_model(g23, g22):
    state = R.pub_state(*g23["pub_recipe"])
    attn = R.pub_cnn_attn()
    assert abs(float(attn.double().sum()) - float(g23["pub_attn_sum"])) < 1e-6 * float(g23["pub_attn_sum"])
    words = torch.from_numpy(g23["pub_sampled_seqs"])
    _fixture_can_fail(g23["pub_sampled_seqs"], g23["pub_greedy_seqs"])
    reward = g23["pub_reward"]
    assert (reward > 0).any() and (reward < 0).any()
    assert g23["pub_keys"].tolist() == S.KEYS and int(g23["max_length"]) == S.T and float(g23["temp"]) == S.TEMP
    o = S.model_scst_grads(state, attn, torch.tensor(R.PUB_LENS), S.T, S.TEMP, reward, torch.tensor(R.PUB_TAGS), words=words)
    assert torch.equal(o["seq"], words)
    top_val, top_idx = o["logit"].topk(8, dim=-1)
    want = g23["pub_logit_top_val"]
    assert float(np.abs(top_val.numpy() - want).max()) < LOGIT_BAR * float(np.abs(want).max())
    assert np.array_equal(top_idx.numpy()[..., 0], g23["pub_logit_top_idx"][..., 0])
    assert abs(float(o["loss"]) - float(g23["pub_loss"])) < LOSS_BAR * float(o["scale"])
    assert set(o["grads"]) == {k.split("/", 1)[1] for k in g23 if k.startswith("pub_gnorm/")}
    _grads_vs_fixture(g23, g22, "pub", o["grads"])
    # the reward and the score are those of the package's compute_batch_score on the recorded words
    from audiocaption_amd.rl_model import compute_batch_score
    V = R.PUB["vocab_size"]
    sc = [compute_batch_score(g23[k], SC.stub_key2refs(S.KEYS, V), S.KEYS, SC.START, SC.END, SC.StubVocabulary(),
                              SC.StubScorer()) for k in ("pub_sampled_seqs", "pub_greedy_seqs")]
    assert np.array_equal(sc[0], g23["pub_score"]) and np.array_equal(sc[0] - sc[1], reward)


def test_pick_seed_exercises_the_finished_row_rule(g23):
    """The sampler seed of the GPU pick test, on the float64 restatement: no draw near a CDF boundary, a clip that ends
    before step T - 2, a clip that never ends."""
    sd = {k: v.double() for k, v in R.small_state(True, *g23["small_t_recipe"]).items()}
    mem, lens, fc, tags = R.small_inputs()
    o = S.decoder_rollout(sd, mem.double(), lens, fc.double(), S.T, S.TEMP, tags, sample_seed=S.PICK_SEED)
    seq = o["seq"].numpy()
    ended = seq == SC.END
    first = np.where(ended.any(1), ended.argmax(1), S.T)
    assert not o["ambiguous"].any() and (first < S.T - 2).any() and (first == S.T).any(), first
    assert np.array_equal(seq, SC.finished_rule(o["seq"]).numpy())


# ---- ScstWrapper without a device --------------------------------------------------------------------------------------
def _attn_model(over_crnn, temporal=True):
    import audiocaption_amd as A
    if over_crnn:
        cfg = A.cnn14rnn_trm_config(R.SMALL["vocab_size"])
        kind = "TemporalBahAttnDecoder" if temporal else "BahAttnCatFcDecoder"
        cfg["decoder"] = {"type": f"audiocaption_amd.rnn_decoder.{kind}",
                          "args": dict(R.SMALL, attn_emb_dim=512, fc_emb_dim=512, dropout=0.0)}
        cfg["type"] = "audiocaption_amd.attn_model." + ("TemporalSeq2SeqAttnModel" if temporal else "Seq2SeqAttnModel")
        return A.init_model_from_config(cfg, print_fn=lambda s: None)
    dec = A.rnn_decoder.TemporalBahAttnDecoder(dropout=0.0, **R.SMALL)
    return A.TemporalSeq2SeqAttnModel(torch.nn.Identity(), dec)


@pytest.mark.parametrize("temporal", [True, False])
def test_wrapper_takes_an_attention_model_over_a_crnn_encoder(temporal):
    import audiocaption_amd as A
    model = _attn_model(True, temporal)
    wrapper = A.ScstWrapper(model)
    assert wrapper.model is model


def test_wrapper_refuses_other_models():
    import audiocaption_amd as A
    with pytest.raises(NotImplementedError, match="TransformerModel"):
        A.ScstWrapper(_attn_model(False))
    with pytest.raises(NotImplementedError, match="TransformerModel"):
        A.ScstWrapper(torch.nn.Linear(2, 2))


def test_wrapper_checks_its_inputs_before_any_launch():
    import audiocaption_amd as A
    wrapper = A.ScstWrapper(_attn_model(True))
    full = {"mode": "train", "wav": torch.zeros(2, 32000), "wav_len": [32000, 32000], "temporal_tag": [0, 1],
            "keys": ["a", "b"], "key2refs": {"a": ["w5"], "b": ["w6"]}, "vocabulary": SC.StubVocabulary(),
            "scorer": SC.StubScorer()}
    for k in ("keys", "key2refs", "vocabulary", "scorer"):
        with pytest.raises(ValueError, match=k):
            wrapper({a: b for a, b in full.items() if a != k})
    for temp in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temp"):
            wrapper(dict(full, temp=temp))
    for method in ("greedy", "beam", "top5", "gumbel", "dbs"):
        with pytest.raises(NotImplementedError, match="sample"):
            wrapper(dict(full, sample_method=method))
    assert set(full) == {"mode", "wav", "wav_len", "temporal_tag", "keys", "key2refs", "vocabulary", "scorer"}
