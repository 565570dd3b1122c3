"""Generate tests/golden/g15_trm_train.npz: one TRAINING step of the Cnn14-TransformerEncoder captioner, run by the
REFERENCE on CPU (imported from /root/reference, with the import stubs of make_golden.py).

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_trm_train.py

Recipe (the G8 recipe of make_golden.py for this model): the reference's ``Cnn14TransformerEncoder`` (freeze_cnn,
freeze_cnn_bn) around its ``TransformerEncoder`` (d_model 256, 2 layers) + ``TransformerDecoder`` (attn_emb_dim 256) in
its ``TransformerModel``, every dropout p = 0, the procedural weights of ``audiocaption_amd.procedural.cnn14trm_trm_state``.
The model starts from a PRESET Cnn14 output: ``encoder.cnn`` is replaced by a module that returns ``attn`` (a seeded
torch draw the tests regenerate; its sum is stored as a check) and the clip lengths, so no golden depends on the conv
stack.  Cases: ragged lengths with T' = 31; teacher forcing (ss_ratio 1) and scheduled sampling (0.7, draws recorded).
Stored: loss, top-8 logits, greedy tokens, every tensor's gradient norm / sum / 64 samples, the clip's total norm and
the change of the same samples after one torch.optim.Adam step.  The CPU restatement of tests/_trm_train_ref.py is
compared with the reference here as well (REPORT_trm_train.txt).
"""
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

# the case (the tests rebuild the inputs from these)
N, TQ, TC, V = 4, 31, 13, 4981
ATTN_SEED = 15
LENS = [31, 20, 9, 1]
CAP_LEN = [13, 10, 8, 12]


def preset_attn():
    """The preset Cnn14 output (N, T', 2048): non-negative like a post-ReLU mean."""
    g = torch.Generator().manual_seed(ATTN_SEED)
    return torch.randn(N, TQ, 2048, generator=g).abs() * 0.5


def caption():
    gen = torch.Generator().manual_seed(11)
    cap = torch.randint(4, V, (N, TC), generator=gen)
    cap[:, 0] = 1
    for i, n in enumerate(CAP_LEN):
        cap[i, n - 1] = 2
        cap[i, n:] = 0
    return cap, np.array(CAP_LEN)


class PresetCnn(nn.Module):
    """Stands in for the frozen Cnn14: returns the preset attn and the clip lengths."""

    def __init__(self, attn, lens):
        super().__init__()
        self.attn, self.lens = attn, lens

    def forward(self, input_dict):
        return {"attn_emb": self.attn, "attn_emb_len": torch.tensor(self.lens), "fc_emb": self.attn.mean(1)}


def main():
    from make_golden import _install_stubs
    _install_stubs()
    torch.manual_seed(0)
    from captioning.models.crnn_trm_encoder import Cnn14TransformerEncoder
    from captioning.models.transformer_decoder import TransformerDecoder
    from captioning.models.transformer_encoder import TransformerEncoder
    from captioning.models.transformer_model import TransformerModel
    from captioning.losses.loss import LabelSmoothingLoss
    from audiocaption_amd import procedural as P
    import _trm_train_ref as TR
    from oracle import train_path as OT

    state = P.to_torch(P.cnn14trm_trm_state(V))
    attn = preset_attn()
    trm = TransformerEncoder(spec_dim=-1, fc_feat_dim=2048, attn_feat_dim=2048, d_model=256, dropout=0.0)
    enc = Cnn14TransformerEncoder(PresetCnn(attn, LENS), trm, freeze_cnn=True, freeze_cnn_bn=True)
    dec = TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=256, attn_emb_dim=256, dropout=0.0, nlayers=2)
    model = TransformerModel(enc, dec)
    own = {k: v for k, v in state.items() if not k.startswith("encoder.cnn.")}
    assert set(model.state_dict()) == set(own), set(model.state_dict()) ^ set(own)
    cap, cap_len = caption()
    loss_fn = LabelSmoothingLoss(smoothing=0.1)
    trainable = [(k, p_) for k, p_ in model.named_parameters() if p_.requires_grad]
    assert sorted(k for k, _ in trainable) == sorted(TR.trainable_keys(own)), "trainable key sets differ"
    idx_gen = np.random.default_rng(3)
    sample_idx = {k: idx_gen.integers(0, p_.numel(), size=min(64, p_.numel())) for k, p_ in trainable}
    g15 = {"cap": cap.numpy(), "cap_len": cap_len, "lens": np.array(LENS), "attn_seed": np.array(ATTN_SEED),
           "attn_sum": np.array(float(attn.double().sum()))}
    report = {}
    torch.set_grad_enabled(True)
    for tag, ss_ratio in (("ss", 0.7), ("tf", 1)):
        model.load_state_dict(own, strict=True)
        model.train()
        model.zero_grad(set_to_none=True)
        random.seed(5)
        use_cap = [random.random() < ss_ratio for _ in range(TC - 1)] if ss_ratio != 1 else [True] * (TC - 1)
        random.seed(5)
        out = model({"mode": "train", "wav": torch.zeros(N, 10), "wav_len": [10] * N, "specaug": False,
                     "cap": cap, "cap_len": cap_len, "ss_ratio": ss_ratio})
        out["tgt"] = cap[:, 1:]
        out["tgt_len"] = torch.as_tensor(cap_len - 1)
        loss = loss_fn(out)
        loss.backward()
        total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        coef = min(1.0, float(1.0 / (total_norm + 1e-6)))
        raw = {k: p_.grad.detach().clone() / coef for k, p_ in trainable}
        opt = torch.optim.Adam([p_ for _, p_ in trainable], lr=5e-4, weight_decay=1e-6)
        before = {k: p_.detach().clone() for k, p_ in trainable}
        opt.step()
        # the restatement of the tests on the same inputs
        o = TR.train_step_grads(own, attn, torch.tensor(LENS), cap, cap_len, [int(u) for u in use_cap], p_dec=0.0,
                                p_enc=0.0, teacher_forcing=(ss_ratio == 1))
        report[f"G15 {tag} logit"] = float((o["logit"] - out["logit"].detach().double()).abs().max())
        report[f"G15 {tag} loss (relative)"] = abs(float(o["loss"]) - float(loss)) / float(loss)
        report[f"G15 {tag} grads (rel. to max)"] = max(
            float((o["grads"][k] - raw[k].double()).abs().max()) / (float(raw[k].abs().max()) + 1e-12) for k, _ in trainable)
        if ss_ratio != 1:
            assert torch.equal(o["seq"], out["seq"]), "greedy tokens of the training forward differ"
        print(f"  G15 {tag}: loss {float(loss):.6f}, grad norm {float(total_norm):.6f}, restatement "
              f"{report[f'G15 {tag} grads (rel. to max)']:.2e}")
        g15[f"{tag}_use_cap"] = np.array(use_cap, dtype=np.int32)
        g15[f"{tag}_loss"] = np.array(float(loss))
        g15[f"{tag}_total_norm"] = np.array(float(total_norm))
        if "seq" in out:
            g15[f"{tag}_seq"] = out["seq"].numpy()
        top = out["logit"].detach().topk(8, dim=-1)
        g15[f"{tag}_logit_top_val"] = top.values.numpy()
        g15[f"{tag}_logit_top_idx"] = top.indices.numpy()
        for k, p_ in trainable:
            g15[f"{tag}_gnorm/{k}"] = np.array(float(raw[k].double().norm()))
            g15[f"{tag}_gsum/{k}"] = np.array(float(raw[k].double().sum()))
            g15[f"{tag}_gsample/{k}"] = raw[k].reshape(-1)[sample_idx[k]].numpy()
            g15[f"{tag}_delta/{k}"] = (p_.detach() - before[k]).reshape(-1)[sample_idx[k]].numpy()
    for k in sample_idx:
        g15[f"sample_idx/{k}"] = sample_idx[k]
    path = os.path.join(HERE, "g15_trm_train.npz")
    np.savez_compressed(path, **g15)
    with open(os.path.join(HERE, "REPORT_trm_train.txt"), "w") as f:
        f.write("max |restatement - reference| of g15 (written by make_golden_trm_train.py, torch %s)\n" % torch.__version__)
        for k, v in report.items():
            f.write(f"{k:32s} {v:.3e}\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
