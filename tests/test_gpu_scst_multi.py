"""GPU tests of multi-rollout self-critical sequence training: the reward kernel ac_scst_group_reward against float64, the
K-rollout TrainEngine.rollout against K single rollouts (the code as it stood before, the reference here), against the
restatement tests/_scst_multi_ref.py with dropout on, and against the sampler's restatement; ScstWrapper(model, n_rollouts=K,
baseline=...) end to end.  Shapes: g17's four clips through the ``_cnn_attn`` hook and its max_length, as test_gpu_scst.py.

Worst cases measured on an MI355X are recorded in tests/golden/REPORT_scst_multi.txt."""
import os

import numpy as np
import pytest
import torch

import _sampling_ref as S
import _scst_multi_ref as SM
import _scst_ref as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-6            # test_gpu_sampling's ambiguity rule
V = 4981
# test_gpu_scst.py's bounds on the same quantities: logits and gradients of a rollout (both encoders), and the
# relative-to-max rule of its replay test
BOUNDS = {"logit": 5e-5, "grad": 2e-4}
REPLAY = 1e-4


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g17(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g17_scst.npz")))


@pytest.fixture(scope="module")
def cnn_attn4(lib, state4981):
    """The Cnn14 output of g17's four clips (the synthetic log-mel) from the exact-f32 conv kernels, computed once."""
    from audiocaption_amd import procedural as Pr
    from test_gpu_model import _cnn_from_logmel
    from test_gpu_scst import _rnn_model
    cnn = _rnn_model(state4981).encoder.cnn
    cnn.conv_algo = "winograd"
    attn, _ = _cnn_from_logmel(cnn, torch.from_numpy(Pr.synthetic_logmel(4, 1001)).to(DEV))
    return attn.clone()


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f"[{name}] {d:.3e}")
    return d


def _forced(N, K, T, seed):
    """Forced words (N, K, T); rollout 1 of clip 1 ends early and carries a word after its <end>."""
    g = torch.Generator().manual_seed(seed)
    words = torch.randint(4, V, (N, K, T), generator=g)
    words[min(1, N - 1), min(1, K - 1), T // 2] = SC.END
    words[min(1, N - 1), min(1, K - 1), T - 1] = 77
    return words


# ---- 1. ac_scst_group_reward ----------------------------------------------------------------------------------------
def _reward_launch(lib, scores, mode, greedy, reward, K=None, N=None):
    from audiocaption_amd import _lib
    return lib.ac_scst_group_reward(_lib.ptr(scores), scores.shape[0] if K is None else K, scores.shape[1] if N is None else N,
                                    mode, _lib.ptr(greedy), _lib.ptr(reward), _lib.stream())


@pytest.mark.parametrize("mode", ["greedy", "mean"])
@pytest.mark.parametrize("N", [1, 5, 64])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_group_reward_kernel_vs_float64(lib, K, N, mode):
    from audiocaption_amd.rl_model import BASELINES, group_reward
    rng = np.random.default_rng(100 * K + N)
    s = (rng.random((K, N)) * 4.0).astype(np.float32)
    s[0, 0] = 0.0                                                    # a clip with an empty caption among its rollouts
    g = (rng.random(N) * 4.0).astype(np.float32)
    sd, gd = torch.from_numpy(s).to(DEV), torch.from_numpy(g).to(DEV)
    reward = torch.full((K * N,), float("nan"), device=DEV)
    assert _reward_launch(lib, sd, BASELINES.index(mode), gd if mode == "greedy" else None, reward) == 0
    got = reward.cpu().numpy().reshape(K, N)
    want32 = SM.group_reward_f32(s, mode, g)
    want64 = SM.group_reward(s, mode, g)
    ulps = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32).astype(np.float32))
    d64 = float(np.abs(got - want64).max())
    print(f"K {K} N {N} {mode}: worst {float(ulps.max()):.2f} ulp of the f32 evaluation, {d64:.3e} from float64")
    assert not np.isnan(got).any()
    assert float(ulps.max()) <= 1.0
    # float64: the K - 1 additions of the sum, the difference, the quotient and the final difference, each rounded once at
    # the scale of the largest score
    assert d64 <= (K + 2) * np.finfo(np.float32).eps * float(np.abs(s).max() + np.abs(g).max())
    if mode == "mean":
        assert np.abs(got.astype(np.float64).sum(0)).max() <= K * (K + 2) * np.finfo(np.float32).eps * float(np.abs(s).max())
    assert torch.equal(group_reward(sd, mode, gd if mode == "greedy" else None), reward)


def test_group_reward_kernel_refusals_leave_the_output_untouched(lib):
    from audiocaption_amd import _lib
    s = torch.rand(9, 4, device=DEV)
    g = torch.rand(4, device=DEV)
    reward = torch.full((36,), -7.5, device=DEV)
    GREEDY, MEAN = 0, 1
    bad = [dict(K=0, mode=GREEDY), dict(K=9, mode=GREEDY), dict(K=9, mode=MEAN), dict(K=1, mode=MEAN), dict(K=-1, mode=MEAN),
           dict(K=2, N=0, mode=MEAN), dict(K=2, N=-3, mode=GREEDY), dict(K=2, mode=2), dict(K=2, mode=-1)]
    for case in bad:
        mode = case.pop("mode")
        assert _reward_launch(lib, s, mode, g, reward, **case) == _lib.AC_ERR_ARG, (case, mode)
    assert _reward_launch(lib, s, GREEDY, None, reward, K=2) == _lib.AC_ERR_ARG           # the greedy mode without its scores
    assert lib.ac_scst_group_reward(None, 2, 4, MEAN, _lib.ptr(g), _lib.ptr(reward), _lib.stream()) == _lib.AC_ERR_ARG
    assert lib.ac_scst_group_reward(_lib.ptr(s), 2, 4, MEAN, _lib.ptr(g), None, _lib.stream()) == _lib.AC_ERR_ARG
    torch.cuda.synchronize()
    assert bool((reward == -7.5).all())
    assert _reward_launch(lib, s, MEAN, None, reward, K=2) == 0                          # the mean mode reads no greedy scores
    assert _reward_launch(lib, s, GREEDY, g, reward, K=1) == 0
    torch.cuda.synchronize()
    assert bool((reward[8:] == -7.5).all()) and bool((reward[:4] == s[0] - g).all())


# ---- 2. / 6. K rollouts in one row space == K single rollouts ----------------------------------------------------------
def _single_grads(eng, batch, words_k, reward_k, temp):
    """Logits and gradients of ONE single-rollout iteration forced with ``words_k`` (N, T) under ``reward_k`` (N,): the
    rollout, loss kernel and backward as they stood before the multi-rollout form."""
    from audiocaption_amd.rl_model import _launch
    out = eng.rollout(dict(batch, _scst_words=words_k))
    dlogit = torch.empty_like(out["logit"])
    _launch(out["logit"], out["seq_i32"], torch.as_tensor(reward_k, device=DEV, dtype=torch.float32), temp, SC.END, dlogit, None)
    eng.backward(dlogit)
    return out, [g.detach().clone() for g in eng.flat.grad_views]


def _equivalence(eng, batch, N, K, T, temp, tag):
    from audiocaption_amd.rl_model import _launch
    words = _forced(N, K, T, 41)
    g = torch.Generator().manual_seed(7)
    reward = (torch.rand(N, K, generator=g) * 2.0 - 1.0)
    singles = [_single_grads(eng, batch, words[:, k], reward[:, k], temp) for k in range(K)]
    out = eng.rollout(dict(batch, _scst_words=words), n_rollouts=K)
    J = K * N
    assert out["logit"].shape == (J, T, V) and out["seq"].shape == (J, T) and out["sampled_logprob"].shape == (J, T)
    assert out["seq"].dtype == torch.int64 and out["seq_i32"].dtype == torch.int32 and out["logit"].is_cuda
    assert torch.equal(out["seq"].cpu(), SC.finished_rule(SM.rows_of(words)))
    assert not torch.equal(out["seq"].cpu(), SM.rows_of(words))                 # the finished-row rule was exercised
    worst_logit = 0.0
    for k in range(K):
        single = singles[k][0]
        assert torch.equal(out["seq"][k * N:(k + 1) * N], single["seq"])
        worst_logit = max(worst_logit, rel(f"{tag} logit block {k}", out["logit"][k * N:(k + 1) * N], single["logit"]))
        lp_tol = 2.0 * BOUNDS["logit"] * float(single["logit"].abs().max()) / temp
        mask = SC.mask_of(single["seq"].cpu())
        assert float((out["sampled_logprob"][k * N:(k + 1) * N] - single["sampled_logprob"]).cpu()[mask].abs().max()) < lp_tol
    dlogit = torch.empty_like(out["logit"])
    _launch(out["logit"], out["seq_i32"], SM.rows_of(reward[:, :, None])[:, 0].contiguous().to(DEV), temp, SC.END, dlogit, None)
    eng.backward(dlogit)
    worst_grad, worst_norm, bad = 0.0, 0.0, []
    for i, (key, view) in enumerate(zip(eng.flat.names, eng.flat.grad_views)):
        want = sum(singles[k][1][i].double() for k in range(K)) / K
        d = rel(f"{tag} {key}", view, want)
        d_norm = abs(float(view.double().norm()) - float(want.norm())) / (float(want.norm()) + 1e-12)
        worst_grad, worst_norm = max(worst_grad, d), max(worst_norm, d_norm)
        if not (d < BOUNDS["grad"] and d < REPLAY and d_norm < REPLAY):
            bad.append((key, d, d_norm))
    print(f"{tag}: K {K} N {N} T {T}: worst logit {worst_logit:.3e} (bound {BOUNDS['logit']:.0e}), worst gradient "
          f"{worst_grad:.3e} relative to max, {worst_norm:.3e} in norm (bounds {BOUNDS['grad']:.0e} / {REPLAY:.0e})")
    assert worst_logit < BOUNDS["logit"]
    assert not bad, bad


def test_multi_rollout_equals_k_single_rollouts(lib, state4981, cnn_attn4, g17):
    from audiocaption_amd.train import TrainEngine
    from test_gpu_scst import _g17_batch, _rnn_model
    model = _rnn_model(state4981)
    eng = TrainEngine(model)
    T, temp = int(g17["max_length"]), float(g17["temp"])
    _equivalence(eng, _g17_batch(g17, cnn_attn4, dropout_seed=3), 4, 3, T, temp, "bi-GRU")
    # the single rollouts keep their own state, keyed as before; the K-rollout state carries K
    assert sorted(str(k[-1]) for k in eng._states) == ["3", "rollout"]


def test_multi_rollout_equals_k_single_rollouts_transformer_encoder(lib, g17):
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
                m.p = 0.0
            if isinstance(m, torch.nn.MultiheadAttention):
                m.dropout = 0.0
    model.encoder.cnn.train(False)
    B, Tq, T, temp = 4, 13, int(g17["max_length"]), 0.7
    g = torch.Generator().manual_seed(515)
    cnn_attn = torch.randn(B, Tq, 2048, generator=g).abs() * 0.5
    lens = torch.tensor([Tq, 1, Tq - 2, 5])
    batch = {"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
             "wav_len": [320 * (32 * int(n) - 1) for n in lens], "specaug": False, "max_length": T, "temp": temp,
             "dropout_seed": 5, "_cnn_attn": cnn_attn.to(DEV)}
    _equivalence(TrainEngine(model), batch, B, 2, T, temp, "Transformer encoder")


# ---- 3. dropout on: the mask indexing of the J-row decoder over the N-clip encoder -------------------------------------
def test_multi_rollout_with_dropout_vs_restatement(lib, state4981, cnn_attn4, g17):
    from audiocaption_amd.rl_model import _launch
    from audiocaption_amd.train import TrainEngine
    from oracle import cpu_path as O
    from oracle import train_path as OT
    from test_gpu_scst import _g17_batch, _rnn_model
    bounds = {"logit": 5e-5, "grad": 2e-4}          # test_rollout_with_dropout_and_specaug_vs_oracle's
    model = _rnn_model(state4981, 0.2, 0.5, False)
    eng = TrainEngine(model)
    N, K, T, temp, seed = 4, 2, int(g17["max_length"]), float(g17["temp"]), 4321
    J = K * N
    words = _forced(N, K, T, 31)
    reward = [0.6, -0.4, 0.3, -0.9, 0.2, 0.7, -0.5, 0.1]
    out = eng.rollout(dict(_g17_batch(g17, cnn_attn4, dropout_seed=seed), _scst_words=words), n_rollouts=K)
    sv = eng._saved
    assert sv["key"][-2:] == ("rollout", K) and (sv["N"], sv["J"]) == (N, J)
    ws_, R_ = sv["ws"], sv["lay"]["R"]
    rows_m = N * sv["Tq"]
    gates = {"mem": ws_.tensor("mem_a")[:rows_m * 256].view(rows_m, 256).cpu(),
             "ffn": [ws_.tensor(f"hdn{l}")[:R_ * sv["F"]].view(R_, sv["F"]).cpu() for l in range(model.decoder.nlayers)]}
    ro = SM.rollout(state4981, cnn_attn4.cpu(), O.cnn14_feat_len(g17["wav_len"].tolist()), T, K, temp=temp, base_seed=seed,
                    p_dec=0.2, p_enc=0.5, words=words, relu_gates=gates, kink=OT.KINK)
    assert torch.equal(out["seq"].cpu(), ro["seq"]) and not torch.equal(ro["seq"], SM.rows_of(words))
    o = SM.scst_grads(ro, reward, temp)
    d_logit = rel("logit (dropout on)", out["logit"], ro["logit"])
    dlogit = torch.empty_like(out["logit"])
    loss, _ = _launch(out["logit"], out["seq_i32"], torch.tensor(reward, device=DEV, dtype=torch.float32), temp, SC.END,
                      dlogit, None)
    print(f"loss {float(loss):.6f} vs {float(o['loss']):.6f}, scale {float(o['scale']):.3f}")
    assert d_logit < bounds["logit"]
    assert abs(float(loss) - float(o["loss"])) <= 2e-5 * float(o["scale"])
    eng.backward(dlogit)
    worst, bad = 0.0, []
    for key, view in zip(eng.flat.names, eng.flat.grad_views):
        d = rel(key, view, o["grads"][key])
        worst = max(worst, d)
        if not d < bounds["grad"]:
            bad.append((key, d))
    print(f"worst relative gradient difference vs the restatement (dropout on, K {K}): {worst:.3e}")
    assert not bad, bad
    # rollouts of one clip see different decoder masks: the same forced words give different logits
    same = eng.rollout(dict(_g17_batch(g17, cnn_attn4, dropout_seed=seed),
                            _scst_words=words[:, :1].expand(N, K, T).contiguous()), n_rollouts=K)
    eng._saved = None
    assert torch.equal(same["seq"][:N], same["seq"][N:]) and not torch.equal(same["logit"][:N], same["logit"][N:])


# ---- 4. sampling ----------------------------------------------------------------------------------------------------
def test_multi_rollout_draws_vs_sampler_restatement(lib, state4981, cnn_attn4, g17):
    from audiocaption_amd.train import TrainEngine
    from test_gpu_scst import _g17_batch, _rnn_model
    model = _rnn_model(state4981)
    eng = TrainEngine(model)
    N, K, T, temp, seed = 4, 4, int(g17["max_length"]), float(g17["temp"]), SC.PICK_SEED
    J = K * N
    batch = _g17_batch(g17, cnn_attn4, seed=seed, dropout_seed=3)
    out = eng.rollout(batch, n_rollouts=K)
    logit, seq = out["logit"].cpu().numpy(), out["seq"].cpu().numpy()
    assert seq.shape == (J, T) and logit.shape == (J, T, V)
    done = np.zeros(J, dtype=bool)
    n_amb = 0
    for t in range(T):
        # the sampler's restatement on the device's own logits: counter (step t, row j) of a batch of J clips
        _, _, oks, amb = S.sample_rows(logit[:, t], S.PLAIN, temp=temp, seed=seed, step=t, rows=np.arange(J), tol=TOL)
        for j in range(J):
            if done[j]:
                assert seq[j, t] == SC.END, f"row {j} step {t}: a word after <end>"
                continue
            assert int(seq[j, t]) in oks[j], f"row {j} (rollout {j // N} of clip {j % N}) step {t}: word {seq[j, t]}"
            n_amb += int(amb[j])
        done |= seq[:, t] == SC.END
    by_clip = SM.clips_of(seq, K).numpy()                           # (N, K, T)
    differing = sum(int(not np.array_equal(by_clip[n, a], by_clip[n, b])) for n in range(N) for a in range(K) for b in range(a))
    print(f"ambiguous draws {n_amb} of {J * T}; differing rollout pairs {differing} of {N * K * (K - 1) // 2}")
    assert differing >= 1
    again = eng.rollout(batch, n_rollouts=K)
    assert torch.equal(again["seq"], out["seq"]) and torch.equal(again["logit"], out["logit"])
    other = eng.rollout(dict(batch, seed=seed + 1), n_rollouts=K)
    assert not torch.equal(other["seq"], out["seq"])
    # K = 1 is the rollout as it was: the same state key, the same bits with and without the argument, and its draws are
    # ac_scst_pick's on rows 0..N-1 (test_gpu_scst.py pins those against ac_sample_rows)
    one = eng.rollout(batch, n_rollouts=1)
    assert eng._saved["key"][-1] == "rollout" and eng._saved["J"] == N
    plain = eng.rollout(batch)
    assert torch.equal(one["seq"], plain["seq"]) and torch.equal(one["logit"], plain["logit"])
    assert torch.equal(one["sampled_logprob"], plain["sampled_logprob"]) and one["seq"].shape == (N, T)
    l1 = one["logit"].cpu().numpy()
    done = np.zeros(N, dtype=bool)
    for t in range(T):
        _, _, oks, _ = S.sample_rows(l1[:, t], S.PLAIN, temp=temp, seed=seed, step=t, rows=np.arange(N), tol=TOL)
        for n in range(N):
            assert (one["seq"][n, t] == SC.END) if done[n] else (int(one["seq"][n, t]) in oks[n])
        done |= one["seq"][:, t].cpu().numpy() == SC.END
    eng._saved = None


# ---- 5. the wrapper end to end ----------------------------------------------------------------------------------------
def _check_wrapper_output(out, model, scorer_kind, batch, N, K, T, baseline):
    from audiocaption_amd.rl_model import compute_batch_score
    want_keys = {"sampled_seqs", "reward", "score", "loss"} | ({"greedy_seqs"} if baseline == "greedy" else set())
    assert set(out) == want_keys
    assert out["sampled_seqs"].shape == (N, K, T) and out["sampled_seqs"].dtype == torch.int64
    assert out["reward"].shape == out["score"].shape == (N, K) and out["reward"].dtype == out["score"].dtype == torch.float64
    assert all(not out[k].is_cuda for k in want_keys - {"loss"}) and out["loss"].is_cuda and out["loss"].dim() == 0
    assert model.training
    sampled = out["sampled_seqs"]
    assert torch.equal(SC.finished_rule(sampled.reshape(N * K, T)).view(N, K, T), sampled)
    score = out["score"].numpy()
    greedy_score = None
    args = (batch["key2refs"], batch["keys"], model.start_idx, model.end_idx, batch["vocabulary"])
    if scorer_kind == "stub":
        for k in range(K):       # one compute_batch_score per set: a repeated key shares a score within a set only
            want = compute_batch_score(sampled[:, k].numpy(), *args, SC.StubScorer())
            assert np.array_equal(score[:, k], want.astype(np.float32).astype(np.float64)), k
        if baseline == "greedy":
            greedy_score = compute_batch_score(out["greedy_seqs"].numpy(), *args, SC.StubScorer()).astype(np.float32)
    else:
        from audiocaption_amd.cider import Cider
        ids = lambda words: Cider().score_ids(batch["key2refs"], batch["vocabulary"], model.vocab_size, batch["keys"],
                                              (words,), model.start_idx, model.end_idx)["scores"][0].cpu().numpy()
        for k in range(K):       # a set's scores do not depend on the sets scored beside it (f32 rounding of the kernel's sums)
            alone = ids(sampled[:, k].to(torch.int32)).astype(np.float64)
            assert np.abs(score[:, k] - alone).max() <= 8 * np.finfo(np.float32).eps * max(1.0, float(np.abs(alone).max())), k
        if baseline == "greedy":
            greedy_score = ids(out["greedy_seqs"].to(torch.int32))
    if baseline == "greedy":
        assert out["greedy_seqs"].shape == (N, T) and out["greedy_seqs"].dtype == torch.int64
    want = SM.group_reward(score.T, baseline, greedy_score).T                       # (N, K) float64
    eps = np.finfo(np.float32).eps
    tol = (K + 2) * eps * (float(np.abs(score).max()) + (float(np.abs(greedy_score).max()) if greedy_score is not None else 0))
    d = float(np.abs(out["reward"].numpy() - want).max())
    print(f"{scorer_kind} / {baseline}: reward vs the restatement {d:.3e} (tolerance {tol:.3e}); scores\n{score}")
    assert d <= tol
    if baseline == "mean":
        assert np.abs(out["reward"].numpy().sum(1)).max() <= K * (K + 2) * eps * float(np.abs(score).max())
    return want


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
@pytest.mark.parametrize("scorer_kind", ["stub", "cider"])
def test_wrapper_end_to_end(lib, state4981, cnn_attn4, g17, scorer_kind, baseline):
    import audiocaption_amd as A
    from audiocaption_amd.cider import Cider
    from test_gpu_cider import _refs_from
    from test_gpu_scst import _g17_batch, _rnn_model
    model = _rnn_model(state4981)
    N, K, T = 4, 3, int(g17["max_length"])
    wrapper = A.ScstWrapper(model, n_rollouts=K, baseline=baseline)
    batch = _g17_batch(g17, cnn_attn4, seed=21, dropout_seed=2)
    assert len(set(batch["keys"])) == N - 1                                       # one repeated key
    if scorer_kind == "cider":
        # references of real length around the words this iteration draws (they do not depend on the scorer)
        probe = A.ScstWrapper(model, n_rollouts=K, baseline="mean")(dict(batch, scorer=SC.ConstantScorer()))
        model._train_engine._saved = None
        batch["key2refs"] = _refs_from(probe["sampled_seqs"][:, 0].numpy(), probe["sampled_seqs"][:, 1].numpy(), batch["keys"],
                                       np.random.default_rng(9))
        batch["scorer"] = Cider()
    if baseline == "mean":
        assert model.decoder._greedy_state is None                                  # the inference path was never entered
    out = wrapper(batch)
    if baseline == "mean":
        assert not model.decoder._greedy_state, "baseline='mean' ran a greedy decode"
        assert "greedy_seqs" not in out
    else:
        assert model.decoder._greedy_state
    want = _check_wrapper_output(out, model, scorer_kind, batch, N, K, T, baseline)
    assert float(np.abs(want).max()) > 0
    # the repeated key is scored once within a rollout set, never across rollouts
    keys = batch["keys"]
    dup = [i for i, k in enumerate(keys) if keys.index(k) != i][0]
    assert torch.equal(out["score"][dup], out["score"][keys.index(keys[dup])])
    assert not all(torch.equal(out["sampled_seqs"][dup, k], out["sampled_seqs"][keys.index(keys[dup]), k]) for k in range(K))
    # loss = mean_j sum_t -(sampled_logprob * reward * mask) over the J rows
    eng = model._train_engine
    lp = eng._saved["ws"].tensor("scst_logprob")[:K * N * T].view(K * N, T).cpu().double()
    rows = SM.rows_of(out["sampled_seqs"])
    terms = -(lp * SC.mask_of(rows).double()) * SM.rows_of(out["reward"][:, :, None])[:, :1]
    assert abs(float(out["loss"].detach()) - float(terms.sum(1).mean())) <= 2e-5 * float(terms.abs().sum() / (K * N)) + 1e-12
    out["loss"].backward()
    params = [(k, p) for k, p in wrapper.named_parameters() if p.requires_grad]
    assert params and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in params)
    assert any(float(p.grad.abs().max()) > 0 for _, p in params)
    assert model.training


# ---- 7. ragged and edge cases ------------------------------------------------------------------------------------------
def test_ragged_lengths_and_single_clip_with_eight_rollouts(lib, state4981, cnn_attn4, g17):
    import audiocaption_amd as A
    from audiocaption_amd.cider import Cider
    from test_gpu_scst import _g17_batch, _rnn_model
    model = _rnn_model(state4981)
    T = int(g17["max_length"])
    full = _g17_batch(g17, cnn_attn4, seed=5, dropout_seed=4)
    # N = 3, three different lengths, K = 2: against K single rollouts of the same ragged batch
    lens = [320000, 200000, 90000]
    assert len(set(lens)) == 3
    b3 = dict(full, wav=full["wav"][:3], wav_len=lens, _cnn_attn=cnn_attn4[:3].contiguous(), keys=full["keys"][:3])
    from audiocaption_amd.train import TrainEngine
    eng = model._train_engine = TrainEngine(model)
    _equivalence(eng, {k: v for k, v in b3.items() if k != "seed"}, 3, 2, T, float(g17["temp"]), "ragged N 3")
    out = A.ScstWrapper(model, n_rollouts=2, baseline="mean")(b3)
    _check_wrapper_output(out, model, "stub", b3, 3, 2, T, "mean")
    out["loss"].backward()
    # N = 1, K = 8, both baselines
    b1 = dict(full, wav=full["wav"][:1], wav_len=full["wav_len"][:1], _cnn_attn=cnn_attn4[:1].contiguous(),
              keys=full["keys"][:1])
    for baseline in ("mean", "greedy"):
        out = A.ScstWrapper(model, n_rollouts=8, baseline=baseline)(b1)
        want = _check_wrapper_output(out, model, "stub", b1, 1, 8, T, baseline)
        assert float(np.abs(want).max()) > 0
        out["loss"].backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.requires_grad)
    # more hypothesis sets than one score_ids call takes (the built-in scorer, K = 5 and the greedy set): four clips, so
    # that the document frequencies of CIDEr-D leave scores that are not all zero
    from test_gpu_cider import _refs_from
    probe = A.ScstWrapper(model, n_rollouts=5, baseline="mean")(dict(full, scorer=SC.ConstantScorer()))
    b4 = dict(full, scorer=Cider(), key2refs=_refs_from(probe["sampled_seqs"][:, 0].numpy(), probe["sampled_seqs"][:, 4].numpy(),
                                                        full["keys"], np.random.default_rng(3)))
    out = A.ScstWrapper(model, n_rollouts=5, baseline="greedy")(b4)
    want = _check_wrapper_output(out, model, "cider", b4, 4, 5, T, "greedy")
    assert float(np.abs(want).max()) > 0 and float(out["score"][:, 4].abs().max()) > 0
    out["loss"].backward()


def test_one_rollout_with_the_greedy_baseline_is_the_wrapper_as_it_was(lib, state4981, cnn_attn4, g17):
    import audiocaption_amd as A
    from test_gpu_scst import _g17_batch, _rnn_model
    model = _rnn_model(state4981, 0.2, 0.5, False)
    batch = _g17_batch(g17, cnn_attn4, seed=9, dropout_seed=6)
    outs, grads = [], []
    for wrapper in (A.ScstWrapper(model), A.ScstWrapper(model, n_rollouts=1, baseline="greedy")):
        wrapper.zero_grad(set_to_none=True)
        out = wrapper(batch)
        out["loss"].backward()
        outs.append(out)
        grads.append(torch.cat([p.grad.reshape(-1) for p in wrapper.parameters() if p.requires_grad]).clone())
    a, b = outs
    assert set(a) == set(b) == {"greedy_seqs", "sampled_seqs", "reward", "score", "loss"}
    assert torch.equal(a["loss"], b["loss"])                                                  # the same bits
    for k in ("greedy_seqs", "sampled_seqs", "reward", "score"):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    assert a["sampled_seqs"].dim() == 2 and a["reward"].dim() == 1
    assert len(model._train_engine._states) == 1 and next(iter(model._train_engine._states))[-1] == "rollout"
    # (the gradients: equal up to the order of the backward's atomic accumulation)
    assert rel("gradients", grads[1], grads[0]) < REPLAY
