"""GPU tests of self-critical sequence training on the HIP path: the two kernels of csrc/scst.hip against the float64
restatement (tests/_scst_ref.py), the rollout of TrainEngine against the sampler's restatement and the CPU oracle, the replay
of what the reference's own ScstWrapper produced (tests/golden/g17_scst.npz), and ScstWrapper end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _sampling_ref as S
import _scst_ref as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-6            # test_gpu_sampling's ambiguity rule
V = 4981


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g17(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g17_scst.npz")))


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f"[{name}] {d:.3e}")
    return d


def _rnn_model(state, p_dec=0.0, p_rnn=0.0, cnn_train=False):
    import audiocaption_amd as A
    model = A.init_model_from_config(A.cnn14rnn_trm_config(V), print_fn=lambda s: None)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    for m in model.decoder.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p_dec
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = p_dec
    model.encoder.rnn.network.dropout = p_rnn
    model.encoder.cnn.train(cnn_train)
    return model


@pytest.fixture(scope="module")
def cnn_attn4(lib, state4981):
    """The Cnn14 output of g17's four clips (the synthetic log-mel) from the exact-f32 conv kernels, computed once."""
    from audiocaption_amd import procedural as Pr
    from test_gpu_model import _cnn_from_logmel
    model = _rnn_model(state4981)
    cnn = model.encoder.cnn
    cnn.conv_algo = "winograd"
    attn, _ = _cnn_from_logmel(cnn, torch.from_numpy(Pr.synthetic_logmel(4, 1001)).to(DEV))
    return attn.clone()


def _g17_batch(g17, cnn_attn, **extra):
    keys = g17["keys"].tolist()
    d = {"mode": "train", "wav": torch.zeros(4, 320000, device=DEV), "wav_len": g17["wav_len"].tolist(), "specaug": False,
         "max_length": int(g17["max_length"]), "temp": float(g17["temp"]), "_cnn_attn": cnn_attn, "keys": keys,
         "key2refs": SC.stub_key2refs(keys, V), "vocabulary": SC.StubVocabulary(), "scorer": SC.StubScorer()}
    d.update(extra)
    return d


# ---- 1. ac_scst_loss -----------------------------------------------------------------------------------------------
def _loss_case(N, T, Vc, seed):
    g = torch.Generator().manual_seed(seed)
    logit = torch.randn(N, T, Vc, generator=g) * 2.5
    seq = torch.randint(3, Vc, (N, T), generator=g)
    if N > 1:
        seq[1, 0] = SC.END                  # ends at t = 0: only its first step counts
    if N > 2:
        seq[2, T // 2] = SC.END             # ends mid-way
    seq = SC.finished_rule(seq)             # row 0 (and the others) never end
    return logit, seq


@pytest.mark.parametrize("temp", [0.7, 1.0])
@pytest.mark.parametrize("N,T,Vc", [(1, 1, 100), (5, 7, 4981), (3, 4, 16384)])
def test_scst_loss_kernel_vs_float64(lib, N, T, Vc, temp):
    from audiocaption_amd.rl_model import _launch, scst_loss
    logit, seq = _loss_case(N, T, Vc, 100 * N + T)
    rewards = [[1.3, -0.7, 0.0, 2.1, -0.2][:N]]
    if N == 1:
        rewards += [[-0.7], [0.0]]
    lg, sq = logit.to(DEV), seq.to(device=DEV, dtype=torch.int32)
    mask = SC.mask_of(seq)
    if N > 2:
        assert mask[0].all() and int(mask[1].sum()) == 1 and 1 < int(mask[2].sum()) < T
    for reward in rewards:
        r64 = torch.tensor(reward, dtype=torch.float64)
        want, terms, scale = SC.scst_loss(logit.double(), seq, r64, temp)
        dwant = SC.scst_dlogit(logit.double(), seq, r64, temp)
        dlogit = torch.full_like(lg, float("nan"))
        loss, row_loss = _launch(lg, sq, r64.to(device=DEV, dtype=torch.float32), temp, SC.END, dlogit, None)
        print(f"N {N} T {T} V {Vc} temp {temp} reward {reward}: loss {float(loss):.6f} vs {float(want):.6f}, scale "
              f"{float(scale):.3e}")
        assert abs(float(loss) - float(want)) <= 2e-5 * float(scale)
        assert float((row_loss.cpu().double().view(N, T) - terms).abs().max()) <= 2e-5 * (float(terms.abs().max()) + 1e-30)
        assert rel("dlogit", dlogit, dwant) < 1e-5
        dl = dlogit.cpu().numpy()
        assert not np.isnan(dl).any()
        assert np.abs(dl[(~mask).numpy()]).max(initial=0.0) == 0.0            # exact 0 on masked rows
        zero = np.asarray(reward) == 0
        assert np.abs(dl[zero]).max(initial=0.0) == 0.0                       # and for a zero reward
    # the autograd function: value and gradient under an upstream factor
    r = torch.tensor(rewards[0])
    la = lg.clone().requires_grad_(True)
    (scst_loss(la, sq, r, temp, SC.END) * 3.0).backward()
    lr = logit.double().requires_grad_(True)
    (SC.scst_loss(lr, seq, r.double(), temp)[0] * 3.0).backward()
    assert rel("dlogit (autograd, x3)", la.grad, lr.grad) < 1e-5


def test_scst_loss_kernel_refuses_bad_arguments(lib):
    from audiocaption_amd import _lib
    x = torch.zeros(2, 3, 10, device=DEV)
    sq = torch.zeros(2, 3, device=DEV, dtype=torch.int32)
    r = torch.zeros(2, device=DEV)
    rl, ls = torch.zeros(6, device=DEV), torch.zeros(1, device=DEV)
    P = _lib.ptr
    args = lambda temp, Vc: (P(x), P(sq), 3, P(r), temp, SC.END, 2, 3, Vc, P(rl), P(ls), None, None, _lib.stream())
    assert lib.ac_scst_loss(*args(1.0, 10)) == 0
    assert lib.ac_scst_loss(*args(0.0, 10)) == _lib.AC_ERR_ARG
    assert lib.ac_scst_loss(*args(float("nan"), 10)) == _lib.AC_ERR_ARG
    assert lib.ac_scst_loss(*args(1.0, 16385)) == _lib.AC_ERR_ARG


# ---- 2. the pick on the engine's own rollout logits -------------------------------------------------------------------
def test_rollout_pick_vs_sampler_restatement(lib, state4981, cnn_attn4, g17):
    from audiocaption_amd import _lib
    from audiocaption_amd import sampling as SM
    from audiocaption_amd.train import TrainEngine
    model = _rnn_model(state4981)
    eng = TrainEngine(model)
    T, temp, seed = 8, 0.8, SC.PICK_SEED
    batch = _g17_batch(g17, cnn_attn4, max_length=T, temp=temp, seed=seed, dropout_seed=3)
    out = eng.rollout(batch)
    logit, seq, lp = out["logit"].cpu().numpy(), out["seq"].cpu().numpy(), out["sampled_logprob"].cpu().numpy()
    N = seq.shape[0]
    assert out["seq"].dtype == torch.int64 and seq.shape == (N, T) and logit.shape == (N, T, V)
    done = np.zeros(N, dtype=bool)
    n_amb = 0
    sd = torch.tensor([SM.seed_word(seed)], device=DEV, dtype=torch.int64)
    for t in range(T):
        rw, rlp, oks, amb = S.sample_rows(logit[:, t], S.PLAIN, temp=temp, seed=seed, step=t, rows=np.arange(N), tol=TOL)
        # ac_sample_rows on the same rows (row stride T * V, counter (t, n)): the same words and log-probabilities, bit for bit
        word = torch.empty(N, device=DEV, dtype=torch.int32)
        wlp = torch.empty(N, device=DEV, dtype=torch.float32)
        _lib.check(lib.ac_sample_rows(ctypes.c_void_p(out["logit"].data_ptr() + 4 * t * V), T * V, N, V, S.PLAIN, 0, 0.0, temp,
                                      _lib.ptr(sd), t, _lib.ptr(word), _lib.ptr(wlp), _lib.stream()), "ac_sample_rows")
        word, wlp = word.cpu().numpy(), wlp.cpu().numpy()
        assert np.array_equal(wlp, lp[:, t]), f"step {t}: ac_scst_pick and ac_sample_rows store different log-probabilities"
        for n in range(N):
            if done[n]:
                assert seq[n, t] == SC.END, f"clip {n} step {t}: a word after <end>"
                continue
            assert seq[n, t] == word[n], f"clip {n} step {t}: ac_scst_pick {seq[n, t]} != ac_sample_rows {word[n]}"
            assert int(seq[n, t]) in oks[n], f"clip {n} step {t}: word {seq[n, t]}, restatement {sorted(oks[n])[:5]}"
            n_amb += int(amb[n])
            if int(seq[n, t]) == rw[n] and not amb[n]:
                assert abs(float(lp[n, t]) - rlp[n]) <= 1e-5
        done |= seq[:, t] == SC.END
    print(f"ambiguous draws on the device: {n_amb} of {N * T}; words\n{seq}")
    assert n_amb <= 1
    ended = seq == SC.END
    first = np.where(ended.any(1), ended.argmax(1), T)
    assert (first < T - 1).any() and (first == T).any(), first     # the finished-row rule was exercised


# ---- 3. replay of the reference's own SCST iteration -----------------------------------------------------------------
def test_replay_of_the_reference_iteration(lib, state4981, cnn_attn4, g17):
    import audiocaption_amd as A
    assert str(g17["decoder"]) == "default"
    model = _rnn_model(state4981)
    wrapper = A.ScstWrapper(model)
    out = wrapper(_g17_batch(g17, cnn_attn4, _scst_words=torch.from_numpy(g17["sampled_seqs"])))
    assert np.array_equal(out["greedy_seqs"].numpy(), g17["greedy_seqs"])
    assert np.array_equal(out["sampled_seqs"].numpy(), g17["sampled_seqs"])
    assert np.array_equal(out["reward"].numpy(), g17["reward"]) and np.array_equal(out["score"].numpy(), g17["score"])
    assert model.training
    sv = model._train_engine._saved
    N, T = g17["sampled_seqs"].shape
    logit = sv["ws"].tensor("logit")[:N * T * V].view(N, T, V).clone()
    top_val, top_idx = logit.topk(8, dim=-1)
    assert rel("logit top-8", top_val, g17["logit_top_val"]) < 2e-5
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g17["logit_top_idx"][..., 0])
    _, _, scale = SC.scst_loss(logit.cpu().double(), g17["sampled_seqs"], g17["reward"], float(g17["temp"]))
    print(f"loss {float(out['loss']):.6f} vs the reference's {float(g17['loss']):.6f}, scale {float(scale):.3f}")
    assert abs(float(out["loss"]) - float(g17["loss"])) <= 2e-5 * float(scale)
    out["loss"].backward()
    g8 = np.load(os.path.join(os.path.dirname(__file__), "golden", "g8_train.npz"))
    named = dict(model.named_parameters())
    worst, bad = 0.0, []
    keys = [k[len("gnorm/"):] for k in g17 if k.startswith("gnorm/")]
    assert sorted(keys) == sorted(k for k, p in named.items() if p.requires_grad)
    for key in keys:
        grad = named[key].grad
        assert grad is not None, key
        gn = float(g17[f"gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g8[f"sample_idx/{key}"]).to(DEV)].cpu().numpy()
        d_s = float(np.abs(sample - g17[f"gsample/{key}"]).max()) / (float(grad.abs().max()) + 1e-12)
        worst = max(worst, d_norm, d_s)
        if not (d_norm < 1e-4 and d_s < 1e-4):
            bad.append((key, d_norm, d_s))
    print(f"worst relative gradient difference vs the reference: {worst:.3e}")
    assert not bad, bad


# ---- 4. dropout active, words forced, against the restatement -------------------------------------------------------
def _forced_words(N, T, seed):
    g = torch.Generator().manual_seed(seed)
    words = torch.randint(4, V, (N, T), generator=g)
    words[1, T // 2] = SC.END
    words[1, T - 1] = 77                    # a word after <end>: the rule turns it into <end>
    return words


def _rollout_vs_restatement(eng, batch, state, cnn_attn, lens, words, reward, temp, seed, p_dec, p_enc, enc_kind, gates,
                            kink, bounds):
    from audiocaption_amd.rl_model import _launch
    out = eng.rollout(batch)
    sv = eng._saved
    if cnn_attn is None:
        cnn_attn = sv["cnn_attn"].cpu()
    dt = torch.float64 if enc_kind == "trm" else torch.float32
    st = {k: v.to(dt) if v.is_floating_point() else v for k, v in state.items()}
    ro = SC.rollout(st, cnn_attn.to(dt), lens, words.shape[1], temp=temp, base_seed=seed, p_dec=p_dec, p_enc=p_enc,
                    words=words, enc_kind=enc_kind, relu_gates=gates(sv, dt), kink=kink)
    assert torch.equal(out["seq"].cpu(), ro["seq"]) and not torch.equal(ro["seq"], words)
    o = SC.scst_grads(ro, reward, temp)
    d_logit = rel("logit", out["logit"], ro["logit"])
    dlogit = torch.empty_like(out["logit"])
    loss, _ = _launch(out["logit"], out["seq_i32"], torch.tensor(reward, device=DEV, dtype=torch.float32), temp, SC.END,
                      dlogit, None)
    print(f"loss {float(loss):.6f} vs {float(o['loss']):.6f}, scale {float(o['scale']):.3f}")
    assert d_logit < bounds["logit"]
    assert abs(float(loss) - float(o["loss"])) <= 2e-5 * float(o["scale"])
    lp = torch.log_softmax(ro["logit"].detach().double(), -1).gather(-1, ro["seq"].unsqueeze(-1)).squeeze(-1) / temp
    # the stored log-probabilities are the forced words': within what the logits' bound allows
    lp_tol = 2.0 * bounds["logit"] * float(ro["logit"].detach().abs().max()) / temp
    assert float((out["sampled_logprob"].cpu().double() - lp)[SC.mask_of(ro["seq"])].abs().max()) < lp_tol
    eng.backward(dlogit)
    worst, bad = 0.0, []
    for key, view in zip(eng.flat.names, eng.flat.grad_views):
        d = rel(key, view, o["grads"][key])
        worst = max(worst, d)
        if not d < bounds["grad"]:
            bad.append((key, d))
    print(f"worst relative gradient difference vs the restatement (dropout on): {worst:.3e}")
    assert not bad, bad
    return sv


def test_rollout_with_dropout_and_specaug_vs_oracle(lib, state4981):
    """Cnn14 0.2, GRU 0.5, decoder 0.2 and SpecAugment on, from the waveform: the bounds of
    test_training_step_with_dropout_vs_oracle (with its ReLU-kink gates)."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.train import TrainEngine
    from oracle import train_path as OT
    model = _rnn_model(state4981, 0.2, 0.5, True)
    model.encoder.cnn.conv_algo = "winograd"
    B, L, T, temp, seed = 3, 192000, 7, 0.9, 4321
    wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=3)).to(DEV)
    wav_len = [192000, 150000, 100000]
    words = _forced_words(B, T, 31)
    batch = {"mode": "train", "wav": wav, "wav_len": wav_len, "specaug": True, "max_length": T, "temp": temp,
             "dropout_seed": seed, "_scst_words": words}

    def gates(sv, dt):
        ws_, R_ = sv["ws"], sv["lay"]["R"]
        rows_m = sv["N"] * sv["Tq"]
        return {"mem": ws_.tensor("mem_a")[:rows_m * 256].view(rows_m, 256).cpu(),
                "ffn": [ws_.tensor(f"hdn{l}")[:R_ * sv["F"]].view(R_, sv["F"]).cpu() for l in range(model.decoder.nlayers)]}

    eng = TrainEngine(model)
    sv = _rollout_vs_restatement(eng, batch, state4981, None, OT.O.cnn14_feat_len(wav_len), words, [0.6, -0.4, 0.3], temp,
                                 seed, 0.2, 0.5, "rnn", gates, OT.KINK, {"logit": 5e-5, "grad": 2e-4})
    assert sv["specaug"] is not None and sv["p_cnn"] == 0.2 and sv["key"][-1] == "rollout"


def test_rollout_transformer_encoder_vs_restatement(lib):
    """The Cnn14-TransformerEncoder captioner, dropout 0.2 in the encoder and the decoder: the bounds of
    test_gpu_train_trm's test_training_step_vs_restatement."""
    import audiocaption_amd as A
    from audiocaption_amd import procedural as P
    from audiocaption_amd.train import TrainEngine
    state = P.to_torch(P.cnn14trm_trm_state(V))
    model = A.init_model_from_config(A.config.cnn14trm_trm_config(V), print_fn=lambda s: None)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    for part in (model.decoder, model.encoder.trm):
        for m in part.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.2
            if isinstance(m, torch.nn.MultiheadAttention):
                m.dropout = 0.2
    model.encoder.cnn.train(False)
    B, Tq, T, temp, seed = 3, 13, 6, 0.7, 515
    g = torch.Generator().manual_seed(seed)
    cnn_attn = torch.randn(B, Tq, 2048, generator=g).abs() * 0.5
    lens = torch.tensor([Tq, 1, Tq - 2])
    words = _forced_words(B, T, 32)
    batch = {"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
             "wav_len": [320 * (32 * int(n) - 1) for n in lens], "specaug": False, "max_length": T, "temp": temp,
             "dropout_seed": seed, "_scst_words": words, "_cnn_attn": cnn_attn.to(DEV)}
    Fe = model.encoder.trm.dim_feedforward

    def gates(sv, dt):
        ws_, R_ = sv["ws"], sv["lay"]["R"]
        N, L = sv["N"], sv["Tm"]
        return {"proj": ws_.tensor("enc_a")[:N * Tq * 256].view(N * Tq, 256).cpu().to(dt),
                "ffn": [ws_.tensor(f"enc_hdn{l}")[:N * L * Fe].view(N * L, Fe).cpu().to(dt) for l in range(2)],
                "mem": ws_.tensor("mem_a")[:N * L * 256].view(N * L, 256).cpu().to(dt),
                "dec_ffn": [ws_.tensor(f"hdn{l}")[:R_ * sv["F"]].view(R_, sv["F"]).cpu().to(dt) for l in range(2)]}

    eng = TrainEngine(model)
    _rollout_vs_restatement(eng, batch, state, cnn_attn, lens, words, [-0.5, 0.8, 0.25], temp, seed, 0.2, 0.2, "trm", gates,
                            1e-4, {"logit": 5e-5, "grad": 2e-4})


# ---- 5. the wrapper end to end ----------------------------------------------------------------------------------------
def _wav_batch(B=3, L=96000, **extra):
    from audiocaption_amd import procedural as Pr
    keys = ["a", "b", "a"][:B]
    d = {"mode": "train", "wav": torch.from_numpy(Pr.synthetic_wav(B, L, seed=5)).to(DEV), "wav_len": [L, L - 20000, L // 2][:B],
         "specaug": False, "max_length": 6, "temp": 0.9, "keys": keys, "key2refs": SC.stub_key2refs(keys, V),
         "vocabulary": SC.StubVocabulary(), "scorer": SC.StubScorer()}
    d.update(extra)
    return d


def test_wrapper_end_to_end_improves_the_rewarded_words(lib, state4981):
    import audiocaption_amd as A
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    model = _rnn_model(state4981)
    wrapper = A.ScstWrapper(model)
    params = [p for p in wrapper.parameters() if p.requires_grad]
    batch = _wav_batch(seed=77, dropout_seed=1)
    # all rewards 0: the loss is 0 and every gradient is exactly 0
    out0 = wrapper(dict(batch, scorer=SC.ConstantScorer()))
    assert float(out0["reward"].abs().max()) == 0.0 and float(out0["loss"]) == 0.0
    out0["loss"].backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in params)
    # the stub scorer: one update raises the reward-weighted log-probability of the same words (dropout 0 in every
    # trainable part; the frozen Cnn14 draws the same masks in every call: the same dropout_seed)
    wrapper.zero_grad(set_to_none=True)
    words = out0["sampled_seqs"]
    eng = model._train_engine

    def logp():
        r = eng.rollout(dict(batch, _scst_words=words))
        eng._saved = None
        return (r["sampled_logprob"].cpu().double() * SC.mask_of(r["seq"].cpu())).sum(1)

    infer = dict(batch, mode="inference", sample_method="greedy")
    model.eval()
    logit_before = model(infer)["logit"][:, 0].clone()
    model.train()
    before = logp()
    out = wrapper(dict(batch, _scst_words=words))
    assert torch.equal(out["sampled_seqs"], words) and model.training
    reward = out["reward"].double()
    assert float(reward.abs().max()) > 0
    assert set(out) == {"greedy_seqs", "sampled_seqs", "reward", "score", "loss"}
    assert abs(float(out["loss"]) + float((before * reward).mean())) <= 2e-5 * float((before * reward).abs().mean()) + 1e-6
    out["loss"].backward()
    clip_grad_norm_(params, 1.0)
    FusedAdam(params, lr=5e-4, weight_decay=1e-6).step()
    after = logp()
    gain = float((reward * (after - before)).sum())
    print(f"reward {reward.tolist()}, reward-weighted log-probability gain {gain:.4e}")
    assert gain > 0
    # a following greedy inference runs on the updated weights: the logits a fresh model gives with them
    model.eval()
    logit_after = model(infer)["logit"][:, 0].clone()
    assert float((logit_after - logit_before).abs().max()) > 1e-4
    fresh = _rnn_model({k[len("model."):]: v.detach().cpu() for k, v in wrapper.state_dict().items()}).eval()
    assert rel("greedy logits of a fresh model", logit_after, fresh(infer)["logit"][:, 0]) < 1e-5


# ---- 6. determinism and isolation ------------------------------------------------------------------------------------
def test_determinism_and_isolation_from_the_cross_entropy_step(lib, state4981):
    import audiocaption_amd as A
    model = _rnn_model(state4981, 0.2, 0.5, True)
    wrapper = A.ScstWrapper(model)
    batch = _wav_batch(seed=5, dropout_seed=9, specaug=True)
    g = torch.Generator().manual_seed(2)
    cap = torch.randint(4, V, (3, 7), generator=g)
    cap[:, 0], cap[:, -1] = 1, 2
    ce = {"mode": "train", "wav": batch["wav"], "wav_len": batch["wav_len"], "specaug": True, "cap": cap.to(DEV),
          "cap_len": np.array([7, 7, 7]), "ss_ratio": 0.5, "_use_cap": [1, 0, 1, 0, 0, 1], "dropout_seed": 11}
    with torch.no_grad():
        ce_before = model(ce)["logit"].clone()
    a = wrapper(batch)
    a["loss"].backward()
    b = wrapper(batch)
    assert torch.equal(a["sampled_seqs"], b["sampled_seqs"]) and torch.equal(a["loss"], b["loss"])
    c = wrapper(dict(batch, seed=6))
    assert not torch.equal(a["sampled_seqs"], c["sampled_seqs"])
    c["loss"].backward()
    eng = model._train_engine
    assert sum(1 for k in eng._states if k[-1] == "rollout") == 1 and len(eng._states) == 2
    with torch.no_grad():
        ce_after = model(ce)["logit"]
    assert torch.equal(ce_before, ce_after)
