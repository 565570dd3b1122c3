"""CPU tests of self-critical sequence training: the restatement tests/_scst_ref.py against what the reference's own
ScstWrapper produced (tests/golden/g17_scst.npz, made by tests/golden/make_golden_scst.py), compute_batch_score, the
wrapper's refusals and config alias, and the new entries of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _scst_ref as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g17(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g17_scst.npz")))


def test_fixture_can_fail_a_test(g17):
    """What the generator asserted of the reference's outputs still holds for the committed file."""
    T = int(g17["max_length"])
    sampled, greedy, reward = g17["sampled_seqs"], g17["greedy_seqs"], g17["reward"]
    assert sampled.shape == greedy.shape == (4, T) and T == 8 and float(g17["temp"]) == 0.8
    assert (reward > 0).any() and (reward < 0).any()
    ended = sampled == SC.END
    first = np.where(ended.any(1), ended.argmax(1), T)
    assert (first < T - 1).any() and (first == T).any()
    assert int((sampled != greedy).any(1).sum()) >= 3
    keys = g17["keys"].tolist()
    assert len(set(keys)) == len(keys) - 1
    assert np.array_equal(SC.finished_rule(sampled).numpy(), sampled)


def test_restatement_vs_reference_loss_and_gradients(g17, state4981):
    """Forced words = the reference's draws: logits' top-8, the loss at the scale of its terms and every gradient (norm and
    sampled entries, the bounds of test_training_step_vs_reference_gradients) against the reference's."""
    from audiocaption_amd import procedural as Pr
    from oracle import cpu_path as O
    assert str(g17["decoder"]) == "default"
    T, temp = int(g17["max_length"]), float(g17["temp"])
    lms = torch.from_numpy(Pr.synthetic_logmel(4, 1001))
    ro = SC.rollout(state4981, O.cnn14_from_logmel(state4981, lms), O.cnn14_feat_len(g17["wav_len"].tolist()), T, temp=temp,
                    words=g17["sampled_seqs"])
    top = ro["logit"].detach().topk(8, -1)
    assert float(np.abs(top.values.numpy() - g17["logit_top_val"]).max()) < 2e-5 * float(np.abs(g17["logit_top_val"]).max())
    assert np.array_equal(top.indices.numpy()[..., 0], g17["logit_top_idx"][..., 0])
    o = SC.scst_grads(ro, g17["reward"], temp)
    print(f"loss {float(o['loss']):.6f} vs {float(g17['loss']):.6f}, scale {float(o['scale']):.3f}")
    assert abs(float(o["loss"]) - float(g17["loss"])) <= 2e-5 * float(o["scale"])
    g8 = np.load(os.path.join(os.path.dirname(__file__), "golden", "g8_train.npz"))
    keys = [k[len("gnorm/"):] for k in g17 if k.startswith("gnorm/")]
    assert sorted(keys) == sorted(ro["keys"])
    for key in keys:
        grad = o["grads"][key]
        gn = float(g17[f"gnorm/{key}"])
        assert gn > 0
        d_norm = abs(float(grad.double().norm()) - gn) / gn
        sample = grad.reshape(-1)[torch.from_numpy(g8[f"sample_idx/{key}"])].numpy()
        d_s = float(np.abs(sample - g17[f"gsample/{key}"]).max()) / float(grad.abs().max())
        assert d_norm < 1e-4 and d_s < 1e-4, (key, d_norm, d_s)
    # the closed form the kernel implements is the gradient autograd takes
    lg = ro["logit"].detach().double().requires_grad_(True)
    SC.scst_loss(lg, ro["seq"], g17["reward"], temp)[0].backward()
    assert float((lg.grad - SC.scst_dlogit(lg.detach(), ro["seq"], g17["reward"], temp)).abs().max()) < 1e-12


def test_pick_seed_has_no_ambiguous_draw_on_the_oracle(g17, state4981):
    """The seed the GPU pick test uses: no draw of the restatement's rollout within 1e-6 of a CDF boundary, and rows that
    end at once, mid-way and never."""
    from audiocaption_amd import procedural as Pr
    from oracle import cpu_path as O
    lms = torch.from_numpy(Pr.synthetic_logmel(4, 1001))
    with torch.no_grad():
        ro = SC.rollout(state4981, O.cnn14_from_logmel(state4981, lms), O.cnn14_feat_len(g17["wav_len"].tolist()), 8,
                        temp=0.8, sample_seed=SC.PICK_SEED, tol=1e-6)
    assert not bool(ro["ambiguous"].any())
    ended = ro["seq"].numpy() == SC.END
    assert np.where(ended.any(1), ended.argmax(1), 8).tolist() == [0, 6, 8, 8]
    assert np.array_equal(SC.finished_rule(ro["seq"]).numpy(), ro["seq"].numpy())


def test_compute_batch_score_vs_reference(g17):
    from audiocaption_amd.rl_model import compute_batch_score
    keys = g17["keys"].tolist()
    refs = SC.stub_key2refs(keys, 4981)
    args = (refs, keys, SC.START, SC.END, SC.StubVocabulary(), SC.StubScorer())
    s = compute_batch_score(g17["sampled_seqs"], *args)
    g = compute_batch_score(g17["greedy_seqs"], *args)
    assert np.array_equal(s, g17["score"]) and np.array_equal(s - g, g17["reward"])
    dup = [i for i, k in enumerate(keys) if keys.index(k) != i]
    assert dup and all(s[i] == s[keys.index(keys[i])] for i in dup)       # a repeated key takes its first clip's score
    assert not np.array_equal(g17["sampled_seqs"][dup[0]], g17["sampled_seqs"][keys.index(keys[dup[0]])])
    # <start> is skipped, the sentence stops at the first <end>
    seen = {}

    class Spy:
        def compute_score(self, references, hypothesis):
            seen.update(hypothesis)
            return 0.0, [0.0] * len(references)

    compute_batch_score(np.array([[SC.START, 7, 9, SC.END, 11], [SC.END, 5, 5, 5, 5]]), {"a": ["x"], "b": ["y"]}, ["a", "b"],
                        SC.START, SC.END, SC.StubVocabulary(), Spy())
    assert seen == {"a": ["w7 w9"], "b": [""]}
    with pytest.raises(ValueError):
        compute_batch_score(g17["sampled_seqs"], refs, keys, SC.START, SC.END, SC.StubVocabulary(), None)


def _wrapper(vocab=50):
    import audiocaption_amd as A
    cfg = {"type": "captioning.models.rl_model.ScstWrapper", "args": {}, "model": A.cnn14rnn_trm_config(vocab)}
    return A.init_model_from_config(cfg, print_fn=lambda s: None)


def test_config_alias_and_state_dict_keys(tmp_path):
    import audiocaption_amd as A
    from audiocaption_amd.rl_model import ScstWrapper
    assert A.config.ALIASES["captioning.models.rl_model.ScstWrapper"] == "audiocaption_amd.rl_model.ScstWrapper"
    assert A.ScstWrapper is ScstWrapper
    w = _wrapper()
    assert isinstance(w, ScstWrapper) and isinstance(w.model, A.TransformerModel)
    inner = A.init_model_from_config(A.cnn14rnn_trm_config(50), print_fn=lambda s: None)
    assert list(w.state_dict()) == ["model." + k for k in inner.state_dict()]
    assert (w.start_idx, w.end_idx, w.pad_idx) == (1, 2, 0)
    # ``pretrained`` of the inner model is honoured
    state = {k: v + 1.0 if v.is_floating_point() else v for k, v in inner.state_dict().items()}
    path = str(tmp_path / "inner.pth")
    torch.save({"model": state}, path)
    cfg = {"type": "captioning.models.rl_model.ScstWrapper", "args": {},
           "model": dict(A.cnn14rnn_trm_config(50), pretrained=path)}
    w2 = A.init_model_from_config(cfg, print_fn=lambda s: None)
    k = "decoder.classifier.weight"
    assert torch.equal(w2.model.state_dict()[k], state[k])


def test_wrapper_refusals_come_before_any_device_work():
    from audiocaption_amd.rl_model import ScstWrapper
    with pytest.raises(NotImplementedError):
        ScstWrapper(torch.nn.Linear(2, 2))
    w = _wrapper()
    keys = ["a", "b"]
    full = {"mode": "train", "wav": torch.zeros(2, 32000), "wav_len": [32000, 32000], "keys": keys,
            "key2refs": SC.stub_key2refs(keys, 50), "vocabulary": SC.StubVocabulary(), "scorer": SC.StubScorer()}
    for missing in ("keys", "key2refs", "vocabulary", "scorer"):
        with pytest.raises(ValueError, match=missing):
            w({k: v for k, v in full.items() if k != missing})
    for temp in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temp"):
            w(dict(full, temp=temp))
    for method in ("greedy", "beam", "top5", "top0.9", "gumbel"):
        with pytest.raises(NotImplementedError, match="plain sampling"):
            w(dict(full, sample_method=method))
    assert "mode" in full and full["mode"] == "train" and "sample_method" not in full   # the caller's dict is left alone


def test_scst_symbols_in_header_and_ctypes_table():
    from audiocaption_amd import _lib
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ac_scst_pick", "ac_scst_loss"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["ac_scst_pick"][1][5] is ctypes.c_void_p      # the sampler seed: a device pointer
    assert _lib.SIGNATURES["ac_scst_loss"][1][3] is ctypes.c_void_p      # the reward: device memory
    assert _lib.ABI_VERSION == 2 and re.search(r"#define AC_ABI_VERSION 2\b", header)
    lib_path = os.path.join(REPO, "audiocaption_amd", "libaudiocaption_hip.so")
    if os.path.exists(lib_path):
        lib = ctypes.CDLL(lib_path)
        assert hasattr(lib, "ac_scst_pick") and hasattr(lib, "ac_scst_loss")
