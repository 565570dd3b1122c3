"""CPU checks of tests/_trm_train_ref.py, the restatement the Transformer-encoder training step is compared with on the
GPU (tests/test_gpu_train_trm.py): at p = 0 it is torch's own nn.TransformerEncoder (the module the reference builds,
transformer_encoder.py:80-84) forward and backward; its dropout sites are the engine's op codes; the step cases have no
near-tie at a token a free-running pass reads."""
import pytest
import torch

import _train_ref as R
import _trm_train_ref as TR
from oracle import train_path as OT


def _reference_encoder(state, attn, attn_len):
    """The reference's TransformerEncoder.forward in eval mode (transformer_encoder.py:95-116) on torch modules."""
    from audiocaption_amd.transformer_encoder import TransformerEncoder
    enc = TransformerEncoder(-1, 2048, 2048, 256).double()
    enc.load_state_dict({k[len(TR.PREFIX):]: v for k, v in state.items() if k.startswith(TR.PREFIX)}, strict=True)
    enc.eval()
    N, Tq, _ = attn.shape
    x = enc.attn_proj(attn)
    x = torch.cat([enc.cls_token.reshape(1, 1, -1).expand(N, 1, -1), x], dim=1).transpose(0, 1)
    lens = torch.as_tensor(attn_len) + 1
    pad = torch.arange(Tq + 1)[None, :] >= lens[:, None]
    return enc.model(x, src_key_padding_mask=pad).transpose(0, 1), enc


@pytest.fixture(scope="module")
def trm_state():
    from audiocaption_amd import procedural as P
    return P.to_torch(P.cnn14trm_trm_state(4981))


def test_restatement_is_torch_transformer_encoder_at_p0(trm_state):
    g = torch.Generator().manual_seed(5)
    N, Tq = 3, 31
    attn = (torch.randn(N, Tq, 2048, generator=g).abs() * 0.5).double()
    lens = torch.tensor([31, 1, 17])
    st = {k: v.double().requires_grad_(True) for k, v in trm_state.items() if k.startswith(TR.PREFIX)}
    mine = TR.encoder_train_forward(st, attn, lens, base_seed=3, p=0.0)
    want, enc = _reference_encoder(trm_state, attn, lens)
    assert mine.shape == (N, Tq + 1, 256)
    err = float((mine - want).detach().abs().max())
    assert err < 1e-10, err
    dy = torch.randn(mine.shape, generator=g, dtype=torch.float64)
    gm = torch.autograd.grad((mine * dy).sum(), list(st.values()))
    gw = torch.autograd.grad((want * dy).sum(), [dict(enc.named_parameters())[k[len(TR.PREFIX):]] for k in st])
    for k, a, b in zip(st, gm, gw):
        assert float((a - b).abs().max()) <= 1e-9 * (1.0 + float(b.abs().max())), k


def test_dropout_sites_are_the_engines_op_codes():
    from audiocaption_amd import train as T
    assert (TR.OP_ENC_PROJ, TR.OP_ENC_LAYER) == (T.OP_ENC_PROJ, T.OP_ENC_LAYER)
    taken = set(range(OT.OP_CNN_BLOCK, OT.OP_CNN_BLOCK + 6)) | {OT.OP_SPECAUG, OT.OP_MEM, OT.OP_EMB_A, OT.OP_EMB_B}
    taken |= set(range(OT.OP_GRU_LAYER, OT.OP_GRU_LAYER + 3))
    taken |= {OT.OP_LAYER + 10 * l + k for l in range(2) for k in range(6)}
    mine = {TR.OP_ENC_PROJ} | {TR.OP_ENC_LAYER + 10 * l + k for l in range(2) for k in range(4)}
    assert not (mine & taken)
    # every site draws its own mask: a restatement with one site's code changed gives another output
    g = torch.Generator().manual_seed(9)
    from audiocaption_amd import procedural as P
    st = {k: v.double() for k, v in P.to_torch(P.trm_encoder_state(TR.PREFIX)).items()}
    attn = (torch.randn(2, 7, 2048, generator=g).abs() * 0.5).double()
    base = TR.encoder_train_forward(st, attn, [7, 3], base_seed=4, p=0.2)
    assert torch.equal(base, TR.encoder_train_forward(st, attn, [7, 3], base_seed=4, p=0.2))
    assert not torch.allclose(base, TR.encoder_train_forward(st, attn, [7, 3], base_seed=5, p=0.2))


@pytest.mark.parametrize("name", list(TR.STEP_CASES))
def test_step_cases_have_no_near_ties(trm_state, name):
    """The GPU step test compares greedy tokens of free-running passes: the restatement's top-1 / top-2 margin at every
    token such a pass reads must exceed the float32 error of the step."""
    cnn_attn, lens, cap, cap_len, use_cap, seed = TR.step_batch(name)
    with torch.no_grad():
        st = {k: v.double() if v.is_floating_point() else v for k, v in trm_state.items()}
        emb = TR.encoder_train_forward(st, cnn_attn.double(), lens, seed, 0.2)
        out = OT.train_forward(st, emb, lens + 1, cap, use_cap, seed, 0.2)
    gap = float(R.free_running_gaps(out["logit"], use_cap).min())
    assert gap >= 1e-3, gap


def g15_inputs(golden_dir):
    """The g15 fixture and the inputs of its training step (tests/golden/make_golden_trm_train.py)."""
    import os
    import numpy as np
    g15 = dict(np.load(os.path.join(golden_dir, "g15_trm_train.npz")))
    lens = torch.from_numpy(g15["lens"])
    gen = torch.Generator().manual_seed(int(g15["attn_seed"]))
    attn = torch.randn(len(lens), int(lens.max()), 2048, generator=gen).abs() * 0.5
    assert abs(float(attn.double().sum()) - float(g15["attn_sum"])) < 1e-6 * abs(float(g15["attn_sum"]))
    return g15, attn, lens, torch.from_numpy(g15["cap"]), g15["cap_len"]


@pytest.mark.parametrize("tag", ["ss", "tf"])
def test_restatement_matches_reference_training_step(golden_dir, trm_state, tag):
    """The restatement at p = 0 against one training step the REFERENCE ran (g15): logits, loss, every gradient, the
    clip's total norm and the first Adam update, at the bars of the G8 fixture."""
    import numpy as np
    g15, attn, lens, cap, cap_len = g15_inputs(golden_dir)
    use_cap = g15[f"{tag}_use_cap"].tolist()
    o = TR.train_step_grads(trm_state, attn, lens, cap, cap_len, use_cap, p_dec=0.0, p_enc=0.0,
                            teacher_forcing=(tag == "tf"))
    assert abs(float(o["loss"]) - float(g15[f"{tag}_loss"])) < 2e-5 * float(g15[f"{tag}_loss"])
    top = o["logit"].topk(8, dim=-1)
    assert np.abs(top.values.numpy() - g15[f"{tag}_logit_top_val"]).max() < 5e-5
    assert np.array_equal(top.indices.numpy()[..., 0], g15[f"{tag}_logit_top_idx"][..., 0])
    if tag == "ss":
        assert np.array_equal(o["seq"].numpy(), g15["ss_seq"])
    assert set(o["grads"]) == {k[len("sample_idx/"):] for k in g15 if k.startswith("sample_idx/")}
    for key, grad in o["grads"].items():
        gn = float(g15[f"{tag}_gnorm/{key}"])
        assert abs(float(grad.norm()) - gn) < 1e-4 * gn + 1e-12, key
        sample = grad.reshape(-1)[torch.from_numpy(g15[f"sample_idx/{key}"])].numpy()
        assert np.abs(sample - g15[f"{tag}_gsample/{key}"]).max() < 1e-4 * float(grad.abs().max()) + 1e-12, key
    keys = list(o["grads"])
    params = {k: trm_state[k].double().clone() for k in keys}
    m1 = {k: torch.zeros_like(v) for k, v in params.items()}
    m2 = {k: torch.zeros_like(v) for k, v in params.items()}
    norm = OT.clip_and_adam(params, o["grads"], m1, m2, 1)
    assert abs(float(norm) - float(g15[f"{tag}_total_norm"])) < 1e-4 * float(norm)
    for k in keys:
        idx = torch.from_numpy(g15[f"sample_idx/{k}"])
        delta = (params[k] - trm_state[k].double()).reshape(-1)[idx].numpy()
        gs = np.abs(g15[f"{tag}_gsample/{k}"])
        solid = gs > 1e-5 * (gs.max() + 1e-30) + 1e-7
        assert np.abs(delta - g15[f"{tag}_delta/{k}"])[solid].max(initial=0.0) < 5e-6, k
