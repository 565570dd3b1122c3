"""Generate g17_scst.npz by running the REFERENCE's ``ScstWrapper.scst`` (captioning/models/rl_model.py:24-85, with
``compute_batch_score`` of captioning/utils/model_util.py:117-164) unmodified on CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_scst.py

rl_model.py is stale: it reads ``"seqs"``, ``"sampled_logprobs"`` and ``input_dict["raw_feats"]``, which the reference's
``CaptionModel`` no longer produces.  ``_Adapter`` below (this file's, not the reference's) wraps the reference
``TransformerModel`` - the full Cnn14Rnn-Trm model at the real size (d 256, V 4981), built by the reference's own
``init_model_from_config`` like g8 - and only renames ``seq`` -> ``seqs``, ``sampled_logprob`` -> ``sampled_logprobs``,
supplies ``raw_feats`` and forwards ``start_idx`` / ``end_idx``; like g8 it keeps the frozen Cnn14 in eval mode (no
F.dropout inside it), and it memoises the Cnn14's output (frozen, eval mode, the same clips in every call).  Baseline,
rollout (``torch.distributions.Categorical``), mask, loss and the reward plumbing are the reference's code.

Dropout 0, SpecAugment off, N = 4 clips from the synthetic log-mel (g8's), max_length 8, temp 0.8.  The scorer, vocabulary
and references are the deterministic stubs of tests/_scst_ref.py (recipes).  The fixture stores the recipe, the reference's
outputs (``sampled_seqs``, ``greedy_seqs``, ``reward``, ``score``, ``loss``), the top-8 of the rollout's logits per step and,
per trainable parameter, the gradient norm and the entries at g8's ``sample_idx``.

Decoder draws and torch seeds are tried in order until the reference's own outputs make a test that can fail (asserted
below): rewards of both signs; a clip whose sample ends before the last step and one that never ends; sampled != greedy
on at least 3 clips; every greedy top-1 / top-2 gap on a live step >= 1e-4; one duplicated key.  The CPU restatement
tests/_scst_ref.py is compared with the reference here as well.
"""
import copy
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

import numpy as np
import torch
import torch.nn as nn

V = 4981
N, MAXLEN, TEMP = 4, 8, 0.8
KEYS = ["clip_a", "clip_b", "clip_a", "clip_c"]          # one duplicated key
WAV_LEN = [320000, 280000, 160000, 300000]                # g8's
DECODERS = ["default", "greedy", "beam"]                  # procedural.cnn14rnn_trm_state's decoder, then decoder_state_diverse
SEEDS = range(17, 17 + 40)
GATE = 1e-4


class _Adapter(nn.Module):
    """See the module docstring: today's output keys under the names rl_model.py reads."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.start_idx, self.end_idx = model.start_idx, model.end_idx
        self.calls = []
        cnn, memo = model.encoder.cnn, {}
        plain = cnn.forward

        def cnn_once(input_dict):
            if "out" not in memo:
                with torch.no_grad():
                    memo["out"] = plain(input_dict)
            return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in memo["out"].items()}

        cnn.forward = cnn_once

    def train(self, mode=True):
        super().train(mode)
        self.model.encoder.cnn.eval()
        return self

    def forward(self, input_dict):
        input_dict.setdefault("raw_feats", input_dict["wav"])
        out = self.model(input_dict)
        out["seqs"], out["sampled_logprobs"] = out["seq"], out["sampled_logprob"]
        self.calls.append({"method": input_dict["sample_method"], "logit": out["logit"].detach().clone(),
                           "seq": out["seq"].clone()})
        return out


def decoder_state(P, kind):
    state = P.cnn14rnn_trm_state(vocab_size=V)
    if kind != "default":
        state.update(P.decoder_state_diverse(kind, vocab_size=V))
    return P.to_torch(state)


def main():
    from make_golden import _PRESET, _install_stubs
    _install_stubs()
    from captioning.models.rl_model import ScstWrapper        # reference
    from captioning.utils import train_util                   # reference
    from audiocaption_amd import procedural as P
    from oracle import cpu_path as O
    import _scst_ref as SC

    cfg = train_util.load_config(os.path.join(REF, "eg_configs/audiocaps/waveform/cnn14rnn_trm.yaml"))["model"]
    cfg = copy.deepcopy(cfg)
    assert cfg["decoder"]["args"]["vocab_size"] == V
    cfg["decoder"]["args"]["dropout"] = 0.0
    cfg["encoder"]["rnn"]["args"]["dropout"] = 0.0
    lms = torch.from_numpy(P.synthetic_logmel(N, 1001))
    _PRESET["lms"] = lms
    key2refs = SC.stub_key2refs(KEYS, V)
    g8 = np.load(os.path.join(HERE, "g8_train.npz"))
    sample_idx = {k[len("sample_idx/"):]: g8[k] for k in g8.files if k.startswith("sample_idx/")}

    found = None
    for kind in DECODERS:
        state = decoder_state(P, kind)
        model = train_util.init_model_from_config(cfg, print_fn=lambda s: None)
        model.load_state_dict(state, strict=True)
        adapter = _Adapter(model)
        wrapper = ScstWrapper(adapter)
        for seed in SEEDS:
            wrapper.zero_grad(set_to_none=True)
            adapter.calls.clear()
            torch.manual_seed(seed)
            out = wrapper({"mode": "train", "wav": torch.zeros(N, 320000), "wav_len": list(WAV_LEN), "specaug": False,
                           "max_length": MAXLEN, "temp": TEMP, "keys": list(KEYS), "key2refs": key2refs,
                           "vocabulary": SC.StubVocabulary(), "scorer": SC.StubScorer()})
            greedy_call, sample_call = adapter.calls
            assert greedy_call["method"] == "greedy" and sample_call["method"] == "sample"
            sampled, greedy = out["sampled_seqs"].numpy(), out["greedy_seqs"].numpy()
            reward = out["reward"].numpy()
            ended = (sampled == SC.END)
            first_end = np.where(ended.any(1), ended.argmax(1), MAXLEN)
            g_ended = (greedy == SC.END)
            g_first = np.where(g_ended.any(1), g_ended.argmax(1), MAXLEN - 1)
            top2 = greedy_call["logit"].topk(2, -1).values
            gaps = (top2[..., 0] - top2[..., 1]).numpy()
            live_gap = min(float(gaps[n, :g_first[n] + 1].min()) for n in range(N))
            ok = ((reward > 0).any() and (reward < 0).any() and (first_end < MAXLEN - 1).any()
                  and (first_end == MAXLEN).any() and int((sampled != greedy).any(1).sum()) >= 3 and live_gap >= GATE)
            print(f"decoder {kind:8s} seed {seed}: reward {np.round(reward, 3)} first <end> {first_end} "
                  f"differ {int((sampled != greedy).any(1).sum())} min live greedy gap {live_gap:.2e} -> {'ok' if ok else 'no'}")
            if ok:
                found = (kind, seed, state, model, wrapper, out, sample_call)
                break
        if found:
            break
    assert found, "no (decoder, seed) gives a fixture whose tests can fail"
    kind, seed, state, model, wrapper, out, sample_call = found
    out["loss"].backward()
    trainable = [(k, p_) for k, p_ in model.named_parameters() if p_.requires_grad]
    assert sorted(k for k, _ in trainable) == sorted(sample_idx), "trainable key set differs from g8's"

    # ---- the restatement against the reference -------------------------------------------------------------------
    lens = O.cnn14_feat_len(WAV_LEN)
    ro = SC.rollout(state, O.cnn14_from_logmel(state, lms), lens, MAXLEN, temp=TEMP, words=out["sampled_seqs"])
    d_logit = float((ro["logit"].detach() - sample_call["logit"]).abs().max())
    mine = SC.scst_grads(ro, out["reward"].numpy(), TEMP)
    d_loss = abs(float(mine["loss"]) - float(out["loss"]))
    worst_g = 0.0
    for k, p_ in trainable:
        worst_g = max(worst_g, float((mine["grads"][k] - p_.grad).abs().max()) / (float(p_.grad.abs().max()) + 1e-12))
    print(f"restatement vs reference: max |logit diff| {d_logit:.3e}, |loss diff| {d_loss:.3e} (scale "
          f"{float(mine['scale']):.3e}), worst relative gradient diff {worst_g:.3e}")
    assert torch.equal(ro["seq"], out["sampled_seqs"]), "the finished-row rule differs"
    assert d_logit < 2e-4 and d_loss < 2e-5 * float(mine["scale"]) and worst_g < 2e-4
    mine_score = {}
    from audiocaption_amd.rl_model import compute_batch_score
    for name, seqs in (("sampled", out["sampled_seqs"]), ("greedy", out["greedy_seqs"])):
        mine_score[name] = compute_batch_score(seqs.numpy(), key2refs, KEYS, SC.START, SC.END, SC.StubVocabulary(),
                                               SC.StubScorer())
    assert np.array_equal(mine_score["sampled"], out["score"].numpy())
    assert np.array_equal(mine_score["sampled"] - mine_score["greedy"], out["reward"].numpy())

    top = sample_call["logit"].topk(8, dim=-1)
    g17 = {"decoder": np.array(kind), "torch_seed": np.array(seed), "keys": np.array(KEYS), "wav_len": np.array(WAV_LEN),
           "max_length": np.array(MAXLEN), "temp": np.array(TEMP),
           "sampled_seqs": out["sampled_seqs"].numpy(), "greedy_seqs": out["greedy_seqs"].numpy(),
           "reward": out["reward"].numpy(), "score": out["score"].numpy(), "loss": np.array(float(out["loss"])),
           "logit_top_val": top.values.numpy(), "logit_top_idx": top.indices.numpy()}
    for k, p_ in trainable:
        g17[f"gnorm/{k}"] = np.array(float(p_.grad.double().norm()))
        g17[f"gsample/{k}"] = p_.grad.reshape(-1)[sample_idx[k]].numpy()
    np.savez_compressed(os.path.join(HERE, "g17_scst.npz"), **g17)
    print(f"wrote g17_scst.npz: decoder {kind}, torch seed {seed}, loss {float(out['loss']):.6f}")
    print("sampled\n", out["sampled_seqs"].numpy(), "\ngreedy\n", out["greedy_seqs"].numpy())


if __name__ == "__main__":
    main()
