"""The sound-event tagger without a GPU: the CPU restatement tests/_sed_ref.py against the reference's recorded outputs
(tests/golden/g21_sed.npz, written by tests/golden/make_golden_sed.py), the NumPy restatement of the tag rule on the
hand-built set (float64 ties included), the declared C ABI and the key list of ``Cnn14RnnTempAttnGruModel``."""
import os
import re

import numpy as np
import pytest
import torch

import _sed_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATE = 1e-4
SYMBOLS = ["ac_pool_avgmax", "ac_sed_head", "ac_sed_tag_workspace_bytes", "ac_sed_temporal_tag"]


@pytest.fixture(scope="module")
def g21():
    return np.load(os.path.join(GOLDEN, "g21_sed.npz"))


@pytest.fixture(scope="module")
def state(g21):
    from audiocaption_amd import procedural as P
    seed, head_seed, scale = g21["recipe"]
    return P.to_torch(P.sed_state(seed=int(seed), head_seed=int(head_seed), head_scale=float(scale)))


def test_restatement_matches_the_fixture(g21, state):
    from audiocaption_amd import procedural as P
    with torch.no_grad():
        for B, T in g21["cases"].tolist():
            pre = R.stack(state, torch.from_numpy(P.synthetic_logmel(B, T)))
            key = f"b{B}_t{T}"
            if key + "_pre" in g21.files:
                d = float((pre - torch.from_numpy(g21[key + "_pre"])).abs().max())
            else:
                d = float((pre[:, :, ::2] - torch.from_numpy(g21[key + "_pre_cols"])).abs().max())
                ds = float((pre.double().sum(2) - torch.from_numpy(g21[key + "_pre_rowsum"])).abs().max())
                print(f"B {B} T {T}: row sums over all classes differ by {ds:.2e}")
                assert ds < GATE * pre.shape[2]
            print(f"B {B} T {T}: restatement vs fixture {d:.2e}")
            assert d < GATE
            assert R.temporal_tags(R.probs(pre).numpy(), T) == g21[key + "_tags"].tolist()


def _hand():
    return [c + (R.RATIO,) for c in R.handbuilt_cases()] + [R.handbuilt_ratio1()]


def test_tag_rule_matches_the_reference_on_the_handbuilt_set(g21):
    seen = set()
    for name, prob, frames, ratio in _hand():
        want = g21[f"hand_{name}_tags"].tolist()
        assert R.temporal_tags(prob, frames, ratio) == want, name
        seen |= set(want)
    assert seen == {0, 1, 2, 3}
    # the two tie pairs, in frames: the float64 rounding of frame * 0.01 decides them
    assert R.tag_of_segments([(0, 760, 936), (1, 892, 980)]) == 2
    assert R.tag_of_segments([(0, 460, 888), (1, 832, 944)]) == 1


def test_integer_form_mutant_is_rejected(g21):
    assert R.tag_of_segments([(0, 760, 936), (1, 892, 980)], integer_form=True) == 0
    assert R.tag_of_segments([(0, 460, 888), (1, 832, 944)], integer_form=True) == 0
    wrong = [name for name, prob, frames, ratio in _hand()
             if R.temporal_tags(prob, frames, ratio, integer_form=True) != g21[f"hand_{name}_tags"].tolist()]
    assert "mixed_1001" in wrong and "mixed_1000" in wrong


def test_tie_sweep_rejects_both_mutants(g21):
    """The sweep the GPU test runs through the tag kernel: the restatement equals the reference's recorded tags on all of
    it, and each wrong arithmetic - integer frames, durations with the product fused into the subtraction - fails on many."""
    pairs = R.tie_sweep()
    want = g21["sweep_tags"].tolist()
    assert len(pairs) == len(want) == 4096 and R.sweep_tags(pairs) == want
    n_c = sum(a != b for a, b in zip(want, R.sweep_tags(pairs, contracted=True)))
    n_i = sum(a != b for a, b in zip(want, R.sweep_tags(pairs, integer_form=True)))
    print(f"tie sweep: contracted-duration mutant wrong on {n_c}, integer-form mutant wrong on {n_i} of {len(pairs)}")
    assert n_c > 100 and n_i > 100
    # the named pairs: the issue's two (reference: after / while) and two that contracted durations get wrong
    assert want[:4] == [2, 1, 0, 0] and R.sweep_tags(pairs[:4], contracted=True) == [2, 1, 1, 2]
    assert R.temporal_tags(R.sweep_probabilities(pairs[:200]), 4 * R.SWEEP_S) == want[:200]


def test_merge_rule_is_discriminated(g21):
    name, prob, frames, ratio = R.handbuilt_ratio1()
    want = g21[f"hand_{name}_tags"].tolist()
    assert want == [1, 2] and R.temporal_tags(prob, frames, ratio) == want
    assert R.temporal_tags(prob, frames, ratio, n_connect=0) != want      # never merging
    assert R.temporal_tags(prob, frames, ratio, n_connect=2) != want      # merging across two frames


def test_segments_are_the_frame_level_regions():
    """The segment-level run finder against the frame-wise array handled frame by frame."""
    name, prob, frames = R.handbuilt_cases()[0]
    for clip in prob:
        fr = R.framewise(clip[None], frames)[0]
        assert R.segments(clip, frames) == R.segments(fr, frames, ratio=1)


def test_abi_symbols_are_declared():
    from audiocaption_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "audiocaption_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["ac_sed_temporal_tag"][1]) == 14


def test_hf_class_builds_with_the_reference_keys(g21):
    import audiocaption_amd as A
    from audiocaption_amd import hf_wrapper as H
    assert A.Cnn8rnnSedModel is H.Cnn8rnnSedModel
    cfg = H.Cnn14RnnTempAttnGruConfig()
    assert (cfg.sample_rate, cfg.vocab_size, cfg.decoder_d_model, cfg.encoder_rnn_num_layers) == (32000, 4981, 512, 3)
    model = H.Cnn14RnnTempAttnGruModel(cfg)
    sd = model.state_dict()
    mel = [k for k in sd if "melspec_extractor." in k]
    # the reference's mel front-end is a stub where the fixture was recorded: its keys are the rest
    assert [k for k in sd if k not in mel] == g21["state_keys"].tolist()
    assert [",".join(str(v) for v in sd[k].shape) for k in sd if k not in mel] == g21["state_shapes"].tolist()
    assert mel == ["melspec_extractor.spectrogram.window", "melspec_extractor.mel_scale.fb",
                   "cap_model.encoder.cnn.melspec_extractor.spectrogram.window",
                   "cap_model.encoder.cnn.melspec_extractor.mel_scale.fb"]
    # a reference state dict (no mel buffers) loads strictly, into the whole model and into the tagger alone
    ref_sd = {k: v for k, v in sd.items() if k not in mel}
    model.load_state_dict(ref_sd, strict=True)
    A.Cnn8rnnSedModel(447).load_state_dict({k[len("sed_model."):]: v for k, v in ref_sd.items() if k.startswith("sed_model.")},
                                           strict=True)
    with pytest.raises(NotImplementedError):
        model.sed_model.train().forward(torch.zeros(1, 64, 40))
