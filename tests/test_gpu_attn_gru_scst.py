"""GPU tests of self-critical sequence training for the attention-GRU captioners (csrc/attn_gru_train.hip
``ac_bah_train_rollout``, ``BahAttnCatFcDecoder.train_rollout``, ``AttnGruTrainEngine.rollout``, ``ScstWrapper`` over
``Seq2SeqAttnModel`` / ``TemporalSeq2SeqAttnModel``).

Against what the REFERENCE ran (tests/golden/g23_attn_gru_scst.npz, p = 0): the decoder's rollout on the reference's drawn
words (case 1) and the whole iteration through ``ScstWrapper`` (case 2).  Against the restatement of
tests/_attn_gru_scst_ref.py in float64: dropout with the same counter-hash masks.  The pick against ``ac_sample_rows`` and
the sampler's restatement.  The bars are those of test_gpu_attn_gru_train.py and test_gpu_scst.py: logits 2e-5 relative,
loss 2e-5 of the loss scale, gradient norms and samples 1e-4, identical top-1 ids and words.  Measured worst ratios:
tests/golden/REPORT_attn_gru_scst.txt."""
import ctypes
import random

import numpy as np
import pytest
import torch

import _attn_gru_scst_ref as S
import _attn_gru_train_ref as R
import _sampling_ref as SR
import _scst_ref as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOGIT_BAR, LOSS_BAR, GRAD_BAR = 2e-5, 2e-5, 1e-4
TOL = 1e-6            # test_gpu_sampling's ambiguity rule
V = R.PUB["vocab_size"]


@pytest.fixture(scope="module")
def g23():
    from audiocaption_amd import build
    build.build()
    return S.load_g23()


@pytest.fixture(scope="module")
def g22():
    return R.load_g22()


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f"[{name}] {d:.3e}")
    return d


def _decoder(temporal, sd, p=0.0):
    import audiocaption_amd as A
    cls = A.rnn_decoder.TemporalBahAttnDecoder if temporal else A.rnn_decoder.BahAttnCatFcDecoder
    dec = cls(dropout=p, **R.SMALL)
    dec.load_state_dict(sd, strict=True)
    return dec.to(DEV).train()


def _seed_dev(seed):
    from audiocaption_amd.sampling import seed_word
    return torch.tensor([seed_word(seed)], device=DEV, dtype=torch.int64)


def _small_rollout(dec, temporal, words=None, seed=0, dropout_seed=0):
    mem, lens, fc, tags = R.small_inputs()
    return dec.train_rollout(mem.to(DEV), fc.to(DEV), lens, S.T, S.TEMP, _seed_dev(seed),
                             tags.to(device=DEV, dtype=torch.int32) if temporal else None,
                             None if words is None else torch.as_tensor(words).to(device=DEV, dtype=torch.int32).contiguous(),
                             R.START_IDX, R.END_IDX, dropout_seed=dropout_seed)


def _grads_vs_fixture(g23, g22, prefix, grads):
    """Gradient norm and 64 samples of every tensor against the fixture (g22's sample indices)."""
    worst, bad = 0.0, []
    for key, grad in grads.items():
        assert grad is not None, key
        gn = float(g23[f"{prefix}_gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g22[f"{prefix}_sample_idx/{key}"]).to(DEV)].cpu().numpy()
        d_s = float(np.abs(sample - g23[f"{prefix}_gsample/{key}"]).max()) / (float(grad.abs().max()) + 1e-12)
        print(f"[{prefix} {key}] norm {d_norm:.3e} samples {d_s:.3e}")
        worst = max(worst, d_norm, d_s)
        if not (d_norm < GRAD_BAR and d_s < GRAD_BAR):
            bad.append((key, d_norm, d_s))
    print(f"[{prefix}] worst relative gradient difference vs the reference: {worst:.3e}")
    assert not bad, f"gradients differ from the reference's: {bad}"


# ---- 1. the decoder's rollout on the reference's drawn words ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["t", "p"])
def test_decoder_rollout_vs_reference_g23(g23, g22, kind):
    from audiocaption_amd.rl_model import _launch
    temporal, case = kind == "t", f"small_{kind}"
    dec = _decoder(temporal, R.small_state(temporal, *g23[f"{case}_recipe"]))
    words = g23[f"{case}_seq"]
    out = _small_rollout(dec, temporal, words)
    B, T = words.shape
    top_val, top_idx = out["logit"].topk(8, dim=-1)
    assert rel(f"{case} logit top-8", top_val, g23[f"{case}_logit_top_val"]) < LOGIT_BAR
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g23[f"{case}_logit_top_idx"][..., 0])
    assert out["seq"].dtype == torch.int64 and out["seq_i32"].dtype == torch.int32
    assert np.array_equal(out["seq"].cpu().numpy(), words) and np.array_equal(out["seq_i32"].cpu().numpy(), words)
    mask = SC.mask_of(words).numpy()
    lp_tol = 2.0 * LOGIT_BAR * float(out["logit"].abs().max()) / S.TEMP      # what the logits' bar allows
    d_lp = float(np.abs(out["sampled_logprob"].cpu().numpy() - g23[f"{case}_sampled_logprob"])[mask].max())
    print(f"[{case} sampled_logprob] {d_lp:.3e} (bound {lp_tol:.3e})")
    assert d_lp < lp_tol
    assert torch.equal(out["embed"][:, -1], out["state"][0])
    w = out["attn_weight"].cpu()
    for b, n in enumerate(R.SMALL_LENS):
        assert float((w[b, :n].sum(0) - 1.0).abs().max()) < 1e-5 and not w[b, n:].any()
    # the recorded loss (rl_model.py:50-58 under the recorded reward) and its gradients
    reward = torch.tensor(g23["small_reward"], device=DEV, dtype=torch.float32)
    dlogit = torch.empty_like(out["logit"])
    loss, _ = _launch(out["logit"], out["seq_i32"], reward, S.TEMP, R.END_IDX, dlogit, None)
    _, _, scale = SC.scst_loss(out["logit"].cpu().double(), words, g23["small_reward"], S.TEMP)
    want = float(g23[f"{case}_loss"])
    print(f"[{case} loss] {abs(float(loss) - want) / float(scale):.3e} of the scale {float(scale):.3f}")
    assert abs(float(loss) - want) < LOSS_BAR * float(scale)
    grads, d_attn, d_fc = dec.train_backward(out["saved"], dlogit)
    named = {"decoder." + k: v for k, v in grads.items()}
    named.update(attn_emb=d_attn, fc_emb=d_fc)
    assert set(named) == {k.split("/", 1)[1] for k in g23 if k.startswith(f"{case}_gnorm/")}
    _grads_vs_fixture(g23, g22, case, named)
    for b, n in enumerate(R.SMALL_LENS):      # frames at or beyond a clip's length: exactly zero
        assert not d_attn[b, n:].any()


# ---- 2. the pick on the rollout's own logits --------------------------------------------------------------------------
def test_rollout_pick_vs_sampler_restatement(g23):
    from audiocaption_amd import _lib
    lib = _lib.load()
    dec = _decoder(True, R.small_state(True, *g23["small_t_recipe"]))
    T, temp, seed = S.T, S.TEMP, S.PICK_SEED
    out = _small_rollout(dec, True, None, seed)
    logit, seq, lp = out["logit"].cpu().numpy(), out["seq"].cpu().numpy(), out["sampled_logprob"].cpu().numpy()
    N, Vs = seq.shape[0], R.SMALL["vocab_size"]
    assert seq.shape == (N, T) and logit.shape == (N, T, Vs)
    done = np.zeros(N, dtype=bool)
    n_amb = 0
    sd = _seed_dev(seed)
    for t in range(T):
        rw, rlp, oks, amb = SR.sample_rows(logit[:, t], SR.PLAIN, temp=temp, seed=seed, step=t, rows=np.arange(N), tol=TOL)
        # ac_sample_rows on the same rows (row stride T * V, counter (t, n)): the same words and log-probabilities, bit for bit
        word = torch.empty(N, device=DEV, dtype=torch.int32)
        wlp = torch.empty(N, device=DEV, dtype=torch.float32)
        _lib.check(lib.ac_sample_rows(ctypes.c_void_p(out["logit"].data_ptr() + 4 * t * Vs), T * Vs, N, Vs, SR.PLAIN, 0, 0.0,
                                      temp, _lib.ptr(sd), t, _lib.ptr(word), _lib.ptr(wlp), _lib.stream()), "ac_sample_rows")
        word, wlp = word.cpu().numpy(), wlp.cpu().numpy()
        assert np.array_equal(wlp, lp[:, t]), f"step {t}: the rollout and ac_sample_rows store different log-probabilities"
        for n in range(N):
            if done[n]:
                assert seq[n, t] == SC.END, f"clip {n} step {t}: a word after <end>"
                continue
            assert seq[n, t] == word[n], f"clip {n} step {t}: the rollout {seq[n, t]} != ac_sample_rows {word[n]}"
            assert int(seq[n, t]) in oks[n], f"clip {n} step {t}: word {seq[n, t]}, restatement {sorted(oks[n])[:5]}"
            n_amb += int(amb[n])
            if int(seq[n, t]) == rw[n] and not amb[n]:
                assert abs(float(lp[n, t]) - rlp[n]) <= 1e-5
        done |= seq[:, t] == SC.END
    print(f"ambiguous draws on the device: {n_amb} of {N * T}; words\n{seq}")
    assert n_amb <= 1
    ended = seq == SC.END
    first = np.where(ended.any(1), ended.argmax(1), T)
    assert (first < T - 2).any() and (first == T).any(), first     # the finished-row rule was exercised


# ---- the whole model over the preset Cnn14 output ---------------------------------------------------------------------
def _pub_model(state, p_dec=0.0, p_rnn=0.0):
    import audiocaption_amd as A
    cfg = A.cnn14rnn_trm_config(V)
    cfg["encoder"]["rnn"]["args"]["dropout"] = p_rnn
    cfg["decoder"] = {"type": "audiocaption_amd.rnn_decoder.TemporalBahAttnDecoder", "args": dict(R.PUB, dropout=p_dec)}
    cfg["type"] = "audiocaption_amd.attn_model.TemporalSeq2SeqAttnModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s: None)
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.startswith("encoder.cnn.") for k in missing)   # the Cnn14 is preset: never run
    model = model.to(DEV).train()
    model.encoder.cnn.eval()
    return model


def _pub_batch(**extra):
    attn = R.pub_cnn_attn()
    B, Tq = attn.shape[:2]
    d = {"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
         "wav_len": [320 * (32 * int(n) - 1) for n in R.PUB_LENS], "specaug": False, "temporal_tag": torch.tensor(R.PUB_TAGS),
         "_cnn_attn": attn.to(DEV), "max_length": S.T, "temp": S.TEMP, "keys": list(S.KEYS),
         "key2refs": SC.stub_key2refs(S.KEYS, V), "vocabulary": SC.StubVocabulary(), "scorer": SC.StubScorer()}
    d.update(extra)
    return d


@pytest.fixture(scope="module")
def pub_state(g23):
    return R.pub_state(*g23["pub_recipe"])


# ---- 3. replay of the reference's own SCST iteration -------------------------------------------------------------------
def test_replay_of_the_reference_iteration(g23, g22, pub_state):
    import audiocaption_amd as A
    from audiocaption_amd.train_attn_gru import AttnGruTrainEngine
    model = _pub_model(pub_state)
    wrapper = A.ScstWrapper(model)
    batch = _pub_batch(_scst_words=torch.from_numpy(g23["pub_sampled_seqs"]))
    before = dict(batch)
    state = random.getstate()
    out = wrapper(batch)
    assert random.getstate() == state, "the rollout draws no scheduled-sampling coin"
    assert set(batch) == set(before) and all(batch[k] is before[k] for k in batch), "the caller's dict is not modified"
    assert set(out) == {"greedy_seqs", "sampled_seqs", "reward", "score", "loss"} and model.training
    assert isinstance(model._train_engine, AttnGruTrainEngine)
    assert np.array_equal(out["greedy_seqs"].numpy(), g23["pub_greedy_seqs"])
    assert np.array_equal(out["sampled_seqs"].numpy(), g23["pub_sampled_seqs"])
    assert np.array_equal(out["reward"].numpy(), g23["pub_reward"]) and np.array_equal(out["score"].numpy(), g23["pub_score"])
    logit = model._train_engine._saved["bah"]["logit"]
    top_val, top_idx = logit.topk(8, dim=-1)
    assert rel("pub logit top-8", top_val, g23["pub_logit_top_val"]) < LOGIT_BAR
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g23["pub_logit_top_idx"][..., 0])
    _, _, scale = SC.scst_loss(logit.cpu().double(), g23["pub_sampled_seqs"], g23["pub_reward"], S.TEMP)
    print(f"[pub loss] {float(out['loss'].detach()):.6f} vs the reference's {float(g23['pub_loss']):.6f}, scale {float(scale):.3f}")
    assert abs(float(out["loss"].detach()) - float(g23["pub_loss"])) <= LOSS_BAR * float(scale)
    out["loss"].backward()
    named = dict(model.named_parameters())
    keys = [k[len("pub_gnorm/"):] for k in g23 if k.startswith("pub_gnorm/")]
    assert sorted(keys) == sorted(k for k, p in named.items() if p.requires_grad)
    assert any(k.startswith("encoder.rnn.") for k in keys) and any(k.startswith("decoder.") for k in keys)
    _grads_vs_fixture(g23, g22, "pub", {k: named[k].grad for k in keys})
    assert model.training


# ---- 4. dropout on, forced words with a word after <end>, against the float64 restatement -----------------------------
def test_rollout_with_dropout_vs_restatement(g23, pub_state):
    from audiocaption_amd.rl_model import _launch
    from audiocaption_amd.train_attn_gru import AttnGruTrainEngine
    p_dec, p_rnn, seed, temp, T = 0.2, 0.5, 4321, 0.9, 7
    model = _pub_model(pub_state, p_dec, p_rnn)
    eng = AttnGruTrainEngine(model)
    g = torch.Generator().manual_seed(31)
    words = torch.randint(4, V, (R.PUB_N, T), generator=g)
    words[1, T // 2] = SC.END
    words[1, T - 1] = 77                    # a word after <end>: the rule turns it into <end>
    reward = [0.6, -0.4, 0.3, -0.8]
    batch = _pub_batch(max_length=T, temp=temp, dropout_seed=seed, _scst_words=words)
    out = eng.rollout(batch)
    want = S.model_scst_grads(pub_state, R.pub_cnn_attn(), torch.tensor(R.PUB_LENS), T, temp, reward,
                              torch.tensor(R.PUB_TAGS), words=words, p_dec=p_dec, p_rnn=p_rnn, base_seed=seed,
                              dtype=torch.float64)
    plain = S.model_rollout({k: v.double() for k, v in pub_state.items()}, R.pub_cnn_attn().double(),
                            torch.tensor(R.PUB_LENS), T, temp, torch.tensor(R.PUB_TAGS), words=words)
    assert rel("dropout changes the logits", plain["logit"], want["logit"]) > 1e-3
    assert torch.equal(out["seq"].cpu(), want["seq"]) and not torch.equal(want["seq"], words)
    assert torch.equal(out["seq_i32"].cpu().long(), want["seq"])
    assert rel("dropout logit", out["logit"], want["logit"]) < LOGIT_BAR
    assert rel("dropout attn_weight", out["attn_weight"], want["attn_weight"][:, :max(R.PUB_LENS)]) < LOGIT_BAR
    mask = SC.mask_of(want["seq"])
    lp_tol = 2.0 * LOGIT_BAR * float(want["logit"].abs().max()) / temp
    assert float((out["sampled_logprob"].cpu().double() - want["sampled_logprob"])[mask].abs().max()) < lp_tol
    dlogit = torch.empty_like(out["logit"])
    loss, _ = _launch(out["logit"], out["seq_i32"], torch.tensor(reward, device=DEV, dtype=torch.float32), temp, SC.END,
                      dlogit, None)
    print(f"[dropout loss] {float(loss):.6f} vs {float(want['loss']):.6f}, scale {float(want['scale']):.3f}")
    assert abs(float(loss) - float(want["loss"])) <= LOSS_BAR * float(want["scale"])
    eng.backward(dlogit)
    worst, bad = 0.0, []
    assert set(eng.flat.names) == set(want["grads"])
    for key, view in zip(eng.flat.names, eng.flat.grad_views):
        ref = want["grads"][key]
        d_norm = abs(float(view.double().norm()) - float(ref.norm())) / (float(ref.norm()) + 1e-12)
        d_s = rel(f"dropout {key}", view, ref)
        worst = max(worst, d_norm, d_s)
        if not (d_norm < GRAD_BAR and d_s < GRAD_BAR):
            bad.append((key, d_norm, d_s))
    print(f"worst relative gradient difference vs the restatement (dropout on): {worst:.3e}")
    assert not bad, bad


# ---- 5. reward routes and learning -----------------------------------------------------------------------------------
class _HostRoute:
    """The built-in CIDEr-D behind a plain scorer object: ``ScstWrapper`` takes the ``compute_batch_score`` route."""

    def __init__(self, cider):
        self.compute_score = cider.compute_score


def test_builtin_cider_on_the_device_vs_the_host_route(g23, pub_state):
    import audiocaption_amd as A
    from audiocaption_amd.cider import Cider
    from test_gpu_cider import GATE, _refs_from
    model = _pub_model(pub_state)
    wrapper = A.ScstWrapper(model)
    batch = _pub_batch(seed=77, dropout_seed=1)
    # the words this iteration draws do not depend on the scorer: take them once to build references around them
    probe = wrapper(dict(batch, scorer=SC.ConstantScorer()))
    model._train_engine._saved = None
    batch["key2refs"] = _refs_from(probe["sampled_seqs"].numpy(), probe["greedy_seqs"].numpy(), S.KEYS,
                                   np.random.default_rng(9))
    a = wrapper(dict(batch, scorer=_HostRoute(Cider())))
    lp = model._train_engine._saved["bah"]["sampled_logprob"].cpu().double()
    b = wrapper(dict(batch, scorer=Cider()))
    assert set(a) == set(b) == {"greedy_seqs", "sampled_seqs", "reward", "score", "loss"} and model.training
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].device == b[k].device and a[k].shape == b[k].shape, k
    assert torch.equal(a["sampled_seqs"], b["sampled_seqs"]) and torch.equal(a["greedy_seqs"], b["greedy_seqs"])
    assert torch.equal(a["sampled_seqs"], probe["sampled_seqs"])
    d_reward = float((a["reward"] - b["reward"]).abs().max())
    d_score = float((a["score"] - b["score"]).abs().max())
    print(f"reward {a['reward'].tolist()}, score {a['score'].tolist()}: max difference {d_reward:.3e} / {d_score:.3e}")
    assert float(a["reward"].abs().max()) > 0.01 and float(a["score"].max()) > 0.01        # worth comparing
    assert a["reward"][0] == a["reward"][2] and b["reward"][0] == b["reward"][2]            # the repeated key
    assert d_reward <= GATE and d_score <= GATE
    # loss = mean_n sum_t -(logprob * mask) * reward[n]: linear in the reward
    N, T = lp.shape
    per_clip = (lp * SC.mask_of(a["sampled_seqs"]).double()).abs().sum(1)
    rounding = 2 * N * T * 2.0 ** -24 * float((per_clip * a["reward"].abs()).mean())
    d_loss = abs(float(a["loss"].detach()) - float(b["loss"].detach()))
    print(f"loss {float(a['loss'].detach()):.6f} vs {float(b['loss'].detach()):.6f}: {d_loss:.3e}")
    assert d_loss <= d_reward * float(per_clip.mean()) + rounding
    b["loss"].backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wrapper.parameters() if p.requires_grad)


class _OneWordScorer:
    """A sentence scores the share of its words that are ``word``."""

    def __init__(self, word):
        self.word = f"w{word}"

    def compute_score(self, references, hypothesis):
        scores = []
        for key in references:
            words = hypothesis[key][0].split()
            scores.append(sum(1 for w in words if w == self.word) / len(words) if words else 0.0)
        return float(np.mean(scores)), scores


def test_a_few_iterations_raise_the_rewarded_words_probability(g23, pub_state):
    """The pattern of test_gpu_scst.py::test_wrapper_end_to_end_improves_the_rewarded_words: all rewards 0 give a zero loss
    and zero gradients; under a scorer that rewards one word - one the first rollout drew where the greedy baseline did not -
    three iterations with FusedAdam raise the probability the rollout gives that word at the place it was drawn."""
    import audiocaption_amd as A
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    model = _pub_model(pub_state)
    wrapper = A.ScstWrapper(model)
    params = [p for p in wrapper.parameters() if p.requires_grad]
    keys = ["a", "b", "c", "d"]
    batch = _pub_batch(keys=keys, key2refs={k: ["w5"] for k in keys}, seed=77, dropout_seed=1)
    out0 = wrapper(dict(batch, scorer=SC.ConstantScorer()))
    assert float(out0["reward"].abs().max()) == 0.0 and float(out0["loss"].detach()) == 0.0
    out0["loss"].backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in params)
    wrapper.zero_grad(set_to_none=True)
    words, greedy = out0["sampled_seqs"], out0["greedy_seqs"]
    live = SC.mask_of(words) & (words != SC.END)
    spot = [(n, t) for n in range(words.shape[0]) for t in range(words.shape[1])
            if live[n, t] and int(words[n, t]) not in greedy[n].tolist()]
    assert spot, "the rollout drew no word the baseline lacks: choose another seed"
    n0, t0 = spot[0]
    word = int(words[n0, t0])
    eng = model._train_engine

    def prob():
        r = eng.rollout(dict(batch, _scst_words=words))
        eng._saved = None
        return float(torch.softmax(r["logit"][n0, t0], -1)[word])

    before = prob()
    opt = FusedAdam(params, lr=5e-4, weight_decay=1e-6)
    rewards = []
    for _ in range(3):
        opt.zero_grad()
        out = wrapper(dict(batch, scorer=_OneWordScorer(word)))
        rewards.append(out["reward"].tolist())
        out["loss"].backward()
        clip_grad_norm_(params, 1.0)
        opt.step()
    after = prob()
    print(f"word {word} drawn by clip {n0} at step {t0}: probability {before:.4e} -> {after:.4e}; rewards {rewards}")
    assert rewards[0][n0] > 0 and model.training
    assert after > before


# ---- 6. determinism and isolation ------------------------------------------------------------------------------------
def _ce_step(model, ce, cap, cap_len):
    """One cross-entropy step through the autograd route: (logit, gradients by name), clones."""
    from audiocaption_amd.loss import LabelSmoothingLoss
    model.zero_grad(set_to_none=True)
    random.seed(R.COIN_SEED)
    out = model(ce)
    LabelSmoothingLoss(smoothing=0.1)({"logit": out["logit"], "tgt": cap[:, 1:].to(DEV),
                                      "tgt_len": torch.as_tensor(cap_len - 1)}).backward()
    return out["logit"].detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad}


def test_determinism_and_isolation_from_the_cross_entropy_step(g23, pub_state):
    """Published widths, decoder dropout 0.2, GRU dropout 0.5: equal seeds give bit-equal rollouts and iterations, another
    sampler seed other words, and a cross-entropy step's logits are bit-equal before and after.  (Its gradients are
    compared in the next test: the backward's split-K products add more than two slices per element with atomics, so two
    runs of the SAME step differ in the last bits whatever ran between them.)"""
    import audiocaption_amd as A
    model = _pub_model(pub_state, 0.2, 0.5)
    wrapper = A.ScstWrapper(model)
    batch = _pub_batch(seed=5, dropout_seed=9)
    cap, cap_len = R.pub_caption()
    ce = {k: batch[k] for k in ("mode", "wav", "wav_len", "specaug", "temporal_tag", "_cnn_attn")}
    ce.update(cap=cap.to(DEV), cap_len=cap_len, ss_ratio=0.7, dropout_seed=11)
    logit_before, _ = _ce_step(model, ce, cap, cap_len)
    model.zero_grad(set_to_none=True)
    eng = model._train_engine
    r1 = eng.rollout(batch)
    r2 = eng.rollout(batch)
    for k in ("logit", "seq", "seq_i32", "sampled_logprob", "attn_weight", "embed", "state"):
        assert torch.equal(r1[k], r2[k]), k
    r3 = eng.rollout(dict(batch, seed=6))
    assert not torch.equal(r1["seq"], r3["seq"])
    a = wrapper(batch)
    a["loss"].backward()
    b = wrapper(batch)
    assert torch.equal(a["sampled_seqs"], b["sampled_seqs"]) and torch.equal(a["loss"], b["loss"])
    assert torch.equal(a["sampled_seqs"], r1["seq"].cpu())
    b["loss"].backward()
    # rollout states carry their own key component: none is shared with the cross-entropy step of the same shape
    assert all(("rollout" in k) == (st.get("rollout") is not None) for k, st in eng._states.items())
    assert any("rollout" in k for k in eng._states) and any("rollout" not in k for k in eng._states)
    logit_after, _ = _ce_step(model, ce, cap, cap_len)
    assert torch.equal(logit_before, logit_after)


def test_cross_entropy_step_is_bit_equal_after_an_scst_iteration(monkeypatch):
    """A cross-entropy ``mode="train"`` step gives bit-equal logits AND gradients whether or not an SCST iteration ran
    before it.  Bit-equal gradients can be asked only of a backward that is bit-reproducible, and the training backward
    is not in general: products split over their reduction add their slices with atomics, and more than two float addends
    per element round differently from run to run (measured on an MI355X: the same step twice, nothing between, moves the
    last bits of every encoder.rnn tensor of layers 0 and 1 - the bi-GRU's input-gradient product runs in 6 slices at any
    batch size - and at the published widths the decoder's too).  So this runs where every sum has at most two addends
    (a + b = b + a): the "small" decoder widths (V 517, attn_size 96), 4 clips x 31 frames (every row-split sum has one
    part), teacher-forced captions in which no word occurs more than twice (the embedding scatter), and the engine's own
    development switch that keeps input-gradient products unsplit (``train._DX_SPLITK``).  The premise - two such steps
    in a row are bit-equal - is asserted first."""
    from audiocaption_amd import train as train_module
    monkeypatch.setattr(train_module, "_DX_SPLITK", False)
    import audiocaption_amd as A
    torch.manual_seed(3)
    Vs = R.SMALL["vocab_size"]
    cfg = A.cnn14rnn_trm_config(Vs)
    cfg["encoder"]["rnn"]["args"]["dropout"] = 0.5
    cfg["decoder"] = {"type": "audiocaption_amd.rnn_decoder.TemporalBahAttnDecoder",
                      "args": dict(R.SMALL, attn_emb_dim=512, fc_emb_dim=512, dropout=0.2)}
    cfg["type"] = "audiocaption_amd.attn_model.TemporalSeq2SeqAttnModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s: None).to(DEV).train()
    model.encoder.cnn.eval()
    wrapper = A.ScstWrapper(model)
    batch = _pub_batch(seed=5, dropout_seed=9, key2refs=SC.stub_key2refs(S.KEYS, Vs))
    cap, cap_len = R.caption(R.PUB_N, R.PUB_TC, [R.PUB_TC] * R.PUB_N, Vs, 14)
    assert int(torch.bincount(cap[:, 1:-1].reshape(-1)).max()) <= 2
    ce = {k: batch[k] for k in ("mode", "wav", "wav_len", "specaug", "temporal_tag", "_cnn_attn")}
    ce.update(cap=cap.to(DEV), cap_len=cap_len, ss_ratio=1, dropout_seed=11)
    logit_0, grad_0 = _ce_step(model, ce, cap, cap_len)
    logit_1, grad_1 = _ce_step(model, ce, cap, cap_len)
    assert torch.equal(logit_0, logit_1)
    moved = [k for k in grad_0 if not torch.equal(grad_0[k], grad_1[k])]
    assert not moved, f"the premise fails - the same step twice differs in {moved}"
    assert all(bool(g.abs().max() > 0) for g in grad_0.values())
    model.zero_grad(set_to_none=True)
    out = wrapper(batch)
    assert float(out["reward"].abs().max()) > 0
    out["loss"].backward()
    assert any(not torch.equal(p.grad, grad_0[k]) for k, p in model.named_parameters() if p.requires_grad)
    logit_2, grad_2 = _ce_step(model, ce, cap, cap_len)
    assert torch.equal(logit_0, logit_2)
    differ = [k for k in grad_0 if not torch.equal(grad_0[k], grad_2[k])]
    assert not differ, differ


# ---- 7. refusals before any launch -------------------------------------------------------------------------------------
def test_rollout_entry_refuses_bad_arguments(g23):
    from audiocaption_amd import _lib
    lib = _lib.load()
    B, Tm, T = 5, 70, 8
    sd = R.small_state(True, *g23["small_t_recipe"])
    dec_t, dec_p = _decoder(True, sd), _decoder(False, R.small_state(False, *g23["small_p_recipe"]))
    w, w_plain = dec_t.weights(), dec_p.weights()
    bad = _lib.AcBahWeights.from_buffer_copy(w)
    bad.attn_size = 100
    mem, lens, fc, tags = R.small_inputs()
    f32, i32 = dict(device=DEV, dtype=torch.float32), dict(device=DEV, dtype=torch.int32)
    mem, fc, lens, tags = mem.to(DEV), fc.to(DEV), lens.to(**i32), tags.to(**i32)
    forced = torch.full((B, T), 5, **i32)
    n = lib.ac_bah_train_workspace_floats(ctypes.byref(w), B, Tm, T)
    assert n > 0
    Vs, d = R.SMALL["vocab_size"], R.SMALL["d_model"]
    outs = {"seq": torch.full((B, T), -7, **i32), "scratch": torch.full((2 * B,), -7, **i32),
            "logit": torch.full((B, T, Vs), -7.0, **f32), "logprob": torch.full((B, T), -7.0, **f32),
            "embed": torch.full((B, T, d), -7.0, **f32), "attn_weight": torch.full((B, Tm, T), -7.0, **f32),
            "state": torch.full((B, d), -7.0, **f32), "ws": torch.full((n,), -7.0, **f32)}
    P = _lib.ptr
    seed = _seed_dev(1)
    good = [ctypes.byref(w), P(mem), P(fc), P(lens), P(tags), B, Tm, T, R.START_IDX, R.END_IDX, 0.8, P(seed), P(forced), T,
            0.0, 0, None, P(outs["seq"]), P(outs["scratch"]), P(outs["logit"]), P(outs["logprob"]), P(outs["embed"]),
            P(outs["attn_weight"]), P(outs["state"]), P(outs["ws"]), _lib.stream()]
    cases = [(0, None), (0, ctypes.byref(bad)), (1, None), (2, None), (3, None), (11, None), (17, None), (18, None), (19, None),
             (20, None), (21, None), (22, None), (23, None), (24, None),                      # null pointers
             (7, 0), (7, -1),                                                                  # T < 1
             (10, 0.0), (10, -1.0), (10, float("nan")), (10, float("inf")),                    # temp
             (13, T - 1),                                                                      # forced row stride below T
             (4, None),                                                                        # tags missing
             (0, ctypes.byref(w_plain)),                                                       # tags given to a plain decoder
             (5, 0), (6, 0), (6, 4096), (14, 1.0), (14, -0.1)]                                 # train_dims_ok's limits
    for i, v in cases:
        args = list(good)
        args[i] = v
        assert lib.ac_bah_train_rollout(*args) == _lib.AC_ERR_ARG, (i, v)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == -7).all()), f"{k} was written by a refused call"
    # the Python surface refuses the same before it allocates
    for kw in (dict(max_length=0), dict(temp=0.0), dict(temp=float("nan"))):
        args = dict(max_length=T, temp=0.8)
        args.update(kw)
        with pytest.raises(ValueError):
            dec_t.train_rollout(mem, fc, lens, args["max_length"], args["temp"], seed, tags)
    with pytest.raises(ValueError, match="tags"):
        dec_t.train_rollout(mem, fc, lens, T, 0.8, seed, None)
    with pytest.raises(ValueError, match="tags"):
        dec_p.train_rollout(mem, fc, lens, T, 0.8, seed, tags)
