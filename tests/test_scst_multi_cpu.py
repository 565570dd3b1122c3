"""CPU tests of multi-rollout self-critical sequence training (ScstWrapper(model, n_rollouts=K, baseline=...)): the
constructor's validation and refusals before any device work, the float64 restatement of the group reward
(tests/_scst_multi_ref.py) on hand-computed cases, the engine's argument checks, and the new entry of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _attn_gru_train_ref as R
import _scst_multi_ref as SM
import _scst_ref as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(vocab=50):
    import audiocaption_amd as A
    return A.init_model_from_config(A.cnn14rnn_trm_config(vocab), print_fn=lambda s: None)


def _attn_gru_model():
    import audiocaption_amd as A
    cfg = A.cnn14rnn_trm_config(R.SMALL["vocab_size"])
    cfg["decoder"] = {"type": "audiocaption_amd.rnn_decoder.TemporalBahAttnDecoder",
                      "args": dict(R.SMALL, attn_emb_dim=512, fc_emb_dim=512, dropout=0.0)}
    cfg["type"] = "audiocaption_amd.attn_model.TemporalSeq2SeqAttnModel"
    return A.init_model_from_config(cfg, print_fn=lambda s: None)


def test_constructor_validation_names_the_argument():
    from audiocaption_amd.rl_model import ScstWrapper
    model = _model()
    for bad in (0, 9, -1, 2.0, "2", None, True, False):
        with pytest.raises(ValueError, match="n_rollouts"):
            ScstWrapper(model, n_rollouts=bad)
    for bad in ("loo", "Mean", None, 1, ""):
        with pytest.raises(ValueError, match="baseline"):
            ScstWrapper(model, n_rollouts=2, baseline=bad)
    with pytest.raises(ValueError, match="baseline"):
        ScstWrapper(model, n_rollouts=1, baseline="mean")
    with pytest.raises(ValueError, match="baseline"):
        ScstWrapper(model, baseline="mean")
    for K in range(1, 9):
        w = ScstWrapper(model, n_rollouts=K)
        assert (w.n_rollouts, w.baseline) == (K, "greedy")
        if K > 1:
            assert ScstWrapper(model, K, "mean").baseline == "mean"


def test_defaults_are_todays_configuration():
    from audiocaption_amd.rl_model import ScstWrapper
    model = _model()
    a, b = ScstWrapper(model), ScstWrapper(model, 1, "greedy")
    assert (a.n_rollouts, a.baseline) == (b.n_rollouts, b.baseline) == (1, "greedy")
    assert list(a.state_dict()) == list(b.state_dict())


def test_constructor_arguments_arrive_from_a_config():
    import audiocaption_amd as A
    cfg = {"type": "captioning.models.rl_model.ScstWrapper", "args": {"n_rollouts": 5, "baseline": "mean"},
           "model": A.cnn14rnn_trm_config(50)}
    w = A.init_model_from_config(cfg, print_fn=lambda s: None)
    assert (w.n_rollouts, w.baseline) == (5, "mean") and isinstance(w.model, A.TransformerModel)
    with pytest.raises(ValueError, match="n_rollouts"):
        A.init_model_from_config(dict(cfg, args={"n_rollouts": 9}), print_fn=lambda s: None)


def test_attention_gru_models_are_refused_by_the_constructor():
    from audiocaption_amd.rl_model import ScstWrapper
    model = _attn_gru_model()
    assert ScstWrapper(model).n_rollouts == 1 and ScstWrapper(model, 1, "greedy").baseline == "greedy"
    with pytest.raises(NotImplementedError, match="n_rollouts"):
        ScstWrapper(model, n_rollouts=2)
    with pytest.raises(NotImplementedError, match="n_rollouts"):
        ScstWrapper(model, n_rollouts=2, baseline="mean")


def test_multi_wrapper_refusals_come_before_any_device_work():
    """The input checks of the single-rollout wrapper hold for the multi-rollout one, on CPU tensors: nothing is launched."""
    from audiocaption_amd.rl_model import ScstWrapper
    w = ScstWrapper(_model(), n_rollouts=3, baseline="mean")
    keys = ["a", "b"]
    full = {"mode": "train", "wav": torch.zeros(2, 32000), "wav_len": [32000, 32000], "keys": keys,
            "key2refs": SC.stub_key2refs(keys, 50), "vocabulary": SC.StubVocabulary(), "scorer": SC.StubScorer()}
    with pytest.raises(NotImplementedError, match="n_samples"):
        w(dict(full, n_samples=3))
    for missing in ("keys", "key2refs", "vocabulary", "scorer"):
        with pytest.raises(ValueError, match=missing):
            w({k: v for k, v in full.items() if k != missing})
    with pytest.raises(ValueError, match="temp"):
        w(dict(full, temp=0.0))
    with pytest.raises(NotImplementedError, match="plain sampling"):
        w(dict(full, sample_method="beam"))
    assert full["mode"] == "train" and "sample_method" not in full


def test_engine_rollout_checks_its_arguments_on_the_host():
    from audiocaption_amd.train import TrainEngine
    eng = TrainEngine(_model())
    d = {"wav": torch.zeros(2, 32000), "wav_len": [32000, 32000]}
    with pytest.raises(NotImplementedError, match="n_samples"):
        eng.rollout(dict(d, n_samples=2), n_rollouts=2)
    for bad in (0, 9, True, 2.0, "3", None):
        with pytest.raises(ValueError, match="n_rollouts"):
            eng.rollout(d, n_rollouts=bad)
    # a row space beyond int32 row indices is refused before anything is launched (a static check on the shapes)
    TrainEngine._check_row_space(32, 8, 20, 32, 4981)
    with pytest.raises(ValueError, match="int32"):
        TrainEngine._check_row_space(4096, 8, 64, 126, 4981)
    with pytest.raises(ValueError, match="int32"):
        TrainEngine._check_row_space(1 << 20, 8, 2, 126, 4981)


def test_layout_with_rollouts_is_the_layout_of_j_clips():
    """The row space of K rollouts of N clips is the row space of K*N clips; only ``clip`` folds back onto the N clips."""
    from audiocaption_amd.train import TrainEngine
    N, K, T, Tm = 3, 2, 4, 5
    multi = TrainEngine._layout(N, T, Tm, False, "cpu", K)
    flat = TrainEngine._layout(K * N, T, Tm, False, "cpu")
    assert multi["passes"] == flat["passes"] and (multi["R"], multi["S"]) == (flat["R"], flat["S"])
    for k in ("pos", "qrow0", "qlen", "cls_rows", "mrow0", "mklen"):
        assert torch.equal(multi[k], flat[k]), k
    assert torch.equal(multi["clip"], flat["clip"] % N)
    one = TrainEngine._layout(N, T, Tm, False, "cpu", 1)
    base = TrainEngine._layout(N, T, Tm, False, "cpu")
    assert all(torch.equal(one[k], base[k]) for k in ("pos", "clip", "qrow0", "qlen", "cls_rows", "mrow0", "mklen"))


def test_group_reward_hand_computed():
    s = [[1.0, 0.5], [3.0, 0.5], [5.0, 2.0]]                      # K = 3, N = 2
    r = SM.group_reward(s, "mean")
    # clip 0: 1 - (3 + 5) / 2 = -3, 3 - (1 + 5) / 2 = 0, 5 - (1 + 3) / 2 = 3; clip 1: 0.5 - 1.25, 0.5 - 1.25, 2 - 0.5
    assert np.array_equal(r, np.array([[-3.0, -0.75], [0.0, -0.75], [3.0, 1.5]]))
    g = SM.group_reward(s, "greedy", [2.0, 0.5])
    assert np.array_equal(g, np.array([[-1.0, 0.0], [1.0, 0.0], [3.0, 1.5]]))
    # K = 2: each rollout against the other one
    assert np.array_equal(SM.group_reward([[0.25], [1.0]], "mean"), np.array([[-0.75], [0.75]]))
    # equal scores (exact in binary): no reward at all
    assert np.array_equal(SM.group_reward(np.full((4, 3), 0.75), "mean"), np.zeros((4, 3)))
    assert np.array_equal(SM.group_reward_f32(s, "mean"), r.astype(np.float32))
    assert np.array_equal(SM.group_reward_f32(s, "greedy", [2.0, 0.5]), g.astype(np.float32))


@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_leave_one_out_rewards_of_a_clip_sum_to_zero(K):
    rng = np.random.default_rng(K)
    s = rng.random((K, 64)) * 3.0
    r64 = SM.group_reward(s, "mean")
    assert np.abs(r64.sum(0)).max() < 1e-13
    r32 = SM.group_reward_f32(s, "mean")
    assert r32.dtype == np.float32
    # each f32 reward carries a few roundings at the scale of the clip's largest score (the sum: K - 1, the difference, the
    # quotient and the final difference one each), and K of them are added
    bound = K * (K + 2) * np.finfo(np.float32).eps * np.abs(s).max(0)
    assert (np.abs(r32.astype(np.float64).sum(0)) <= bound).all()
    assert np.abs(r32 - r64).max() <= (K + 2) * np.finfo(np.float32).eps * np.abs(s).max()


def test_rows_and_clips_are_inverse_orders():
    w = torch.arange(4 * 3 * 5).view(4, 3, 5)
    rows = SM.rows_of(w)
    assert rows.shape == (12, 5) and torch.equal(rows[2 * 4 + 1], w[1, 2])       # row j = k*N + n
    assert torch.equal(SM.clips_of(rows, 3), w)


def test_group_reward_symbol_in_header_and_ctypes_table():
    from audiocaption_amd import _lib
    from audiocaption_amd import rl_model
    from audiocaption_amd.train import TrainEngine
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+ac_scst_group_reward\s*\(([^)]*)\)", bare)
    assert m, "ac_scst_group_reward is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 7
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    want = [ctypes.c_void_p if "*" in p else ctype[p.split()[0]] for p in params]
    res, args = _lib.SIGNATURES["ac_scst_group_reward"]
    assert res is ctypes.c_int and list(args) == want
    assert re.search(r"#define AC_SCST_MAX_ROLLOUTS 8\b", header)
    assert rl_model.MAX_ROLLOUTS == TrainEngine.MAX_ROLLOUTS == 8
    assert re.search(r"#define AC_SCST_BASELINE_GREEDY 0\b", header) and re.search(r"#define AC_SCST_BASELINE_MEAN 1\b", header)
    assert rl_model.BASELINES == ("greedy", "mean")
    assert _lib.ABI_VERSION == 2 and re.search(r"#define AC_ABI_VERSION 2\b", header)
    lib_path = os.path.join(REPO, "audiocaption_amd", "libaudiocaption_hip.so")
    if os.path.exists(lib_path):
        assert hasattr(ctypes.CDLL(lib_path), "ac_scst_group_reward")


def test_restatement_of_k_rollouts_against_the_single_rollout_restatement(state4981):
    """Dropout 0: block k of the J-row restatement is the single-rollout restatement forced with words[:, k], and its
    gradients are (1 / K) of the sum of theirs; K = 1 is the single-rollout restatement itself."""
    g = torch.Generator().manual_seed(3)
    N, K, T, Tq, temp = 2, 2, 3, 4, 0.8
    cnn_attn = torch.randn(N, Tq, 2048, generator=g).abs() * 0.5
    lens = torch.tensor([Tq, 2])
    words = torch.randint(4, 4981, (N, K, T), generator=g)
    words[1, 1, 0] = SC.END
    reward = torch.tensor([[0.5, -1.0], [0.25, 0.75]], dtype=torch.float64)          # (N, K)
    multi = SM.rollout(state4981, cnn_attn, lens, T, K, temp=temp, words=words)
    assert multi["logit"].shape == (K * N, T, 4981)
    gm = SM.scst_grads(multi, SM.rows_of(reward[:, :, None])[:, 0], temp)
    total = None
    for k in range(K):
        one = SC.rollout(state4981, cnn_attn, lens, T, temp=temp, words=words[:, k])
        assert torch.equal(multi["seq"][k * N:(k + 1) * N], one["seq"])
        d = (multi["logit"][k * N:(k + 1) * N] - one["logit"]).detach().abs().max() / one["logit"].detach().abs().max()
        assert float(d) < 1e-5
        go = SC.scst_grads(one, reward[:, k], temp)["grads"]
        total = go if total is None else {key: total[key] + go[key] for key in go}
    for key, want in total.items():
        want = want / K
        assert float((gm["grads"][key] - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-12, key
    single = SM.rollout(state4981, cnn_attn, lens, T, 1, temp=temp, words=words[:, :1])
    assert torch.equal(single["logit"], SC.rollout(state4981, cnn_attn, lens, T, temp=temp, words=words[:, 0])["logit"])
    # with dropout on, a clip's rollouts see different decoder masks but ONE encoder pass
    drop = SM.rollout(state4981, cnn_attn, lens, T, K, temp=temp, base_seed=5, p_dec=0.2, p_enc=0.5,
                      words=words[:, :1].expand(N, K, T))
    assert torch.equal(drop["seq"][:N], drop["seq"][N:]) and not torch.equal(drop["logit"][:N], drop["logit"][N:])
