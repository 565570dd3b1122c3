"""GPU tests of the training step of the Cnn14-TransformerEncoder captioner (TrainEngine with model.encoder a
Cnn14TransformerEncoder): the whole step against the CPU restatement of tests/_trm_train_ref.py with dropout active,
the reference runner's surface (model(input_dict) + loss.backward() + a torch optimiser), graph replay, the Cnn14
look-ahead, training progress and the refusals."""
import random

import numpy as np
import pytest
import torch

import _train_ref as R
import _trm_train_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINK = 1e-4


@pytest.fixture(scope="module")
def trm_state():
    from audiocaption_amd import procedural as P
    return P.to_torch(P.cnn14trm_trm_state(4981))


def _model(state, **enc_args):
    import audiocaption_amd as A
    from audiocaption_amd import build
    build.build()
    cfg = A.config.cnn14trm_trm_config(4981)
    cfg["encoder"]["args"].update(enc_args)
    model = A.init_model_from_config(cfg, print_fn=lambda s: None)
    model.load_state_dict(state, strict=True)
    return model.to("cuda:0").train()


@pytest.fixture()
def trm_model(trm_state):
    return _model(trm_state)


def _set_dropout(model, p_dec, p_enc, cnn_train):
    for part, p in ((model.decoder, p_dec), (model.encoder.trm, p_enc)):
        for m in part.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = p
            if isinstance(m, torch.nn.MultiheadAttention):
                m.dropout = p
    model.encoder.cnn.train(cnn_train)


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f"[{name}] {d:.3e}")
    return d


def _hook_batch(name):
    cnn_attn, lens, cap, cap_len, use_cap, seed = TR.step_batch(name)
    B, Tq = cnn_attn.shape[:2]
    batch = {"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
             "wav_len": [320 * (32 * int(n) - 1) for n in lens], "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len,
             "ss_ratio": 0.85, "_use_cap": use_cap, "dropout_seed": seed, "_cnn_attn": cnn_attn.to(DEV)}
    return batch, (cnn_attn, lens, cap, cap_len, use_cap, seed)


def _compare_step(model, state, batch, cnn_attn, lens, cap, cap_len, use_cap, seed, p, teacher_forcing=False):
    from audiocaption_amd.loss import _launch
    from audiocaption_amd.train import TrainEngine
    eng = TrainEngine(model)
    out = eng.forward(batch)
    sv = eng._saved
    ws_, R_ = sv["ws"], sv["lay"]["R"]
    N, Tq, L = sv["N"], sv["Tq"], sv["Tm"]
    Fe = model.encoder.trm.dim_feedforward
    gates = {"proj": ws_.tensor("enc_a")[:N * Tq * 256].view(N * Tq, 256).cpu(),
             "ffn": [ws_.tensor(f"enc_hdn{l}")[:N * L * Fe].view(N * L, Fe).cpu() for l in range(2)],
             "mem": ws_.tensor("mem_a")[:N * L * 256].view(N * L, 256).cpu(),
             "dec_ffn": [ws_.tensor(f"hdn{l}")[:R_ * sv["F"]].view(R_, sv["F"]).cpu() for l in range(2)]}
    if cnn_attn is None:
        cnn_attn = sv["cnn_attn"].cpu()
    o = TR.train_step_grads(state, cnn_attn, lens, cap, cap_len, use_cap, base_seed=seed, p_dec=p, p_enc=p,
                            teacher_forcing=teacher_forcing, relu_gates=gates, kink=KINK)
    if not teacher_forcing:
        gap = float(R.free_running_gaps(o["logit"], use_cap).min())
        assert gap >= 1e-3, f"near-tie {gap:.1e}: choose another seed"
        assert torch.equal(out["seq"].cpu(), o["seq"])
    assert torch.equal(torch.as_tensor(out["attn_emb_len"]), torch.as_tensor(lens) + 1)
    worst = {"logit": rel("logit", out["logit"], o["logit"])}
    tgt_len = torch.as_tensor(cap_len - 1)
    count = float(tgt_len.sum())
    dlogit = torch.empty_like(out["logit"])
    loss, _ = _launch(out["logit"], cap[:, 1:].to(DEV), tgt_len.to(device=DEV, dtype=torch.int32), 0.1, 1.0 / count,
                      dlogit, 1.0 / count, None)
    worst["loss"] = abs(float(loss) - float(o["loss"])) / float(o["loss"])
    eng.backward(dlogit)
    bad = []
    worst["grad"] = 0.0
    for key, view in zip(eng.flat.names, eng.flat.grad_views):
        d = rel(key, view, o["grads"][key])
        worst["grad"] = max(worst["grad"], d)
        if not d < 2e-4:
            bad.append((key, d))
    print("worst relative differences vs the restatement", worst)
    assert worst["logit"] < 5e-5 and worst["loss"] < 2e-5
    assert not bad, bad
    assert all(k.startswith("encoder.trm.") for k in eng.flat.names[:eng.flat.names.index("decoder.word_embedding.weight")])
    return eng


@pytest.mark.parametrize("name", list(TR.STEP_CASES))
def test_training_step_vs_restatement(trm_model, trm_state, name):
    """32 clips x 10 s (L 32) and 8 clips x 30 s (L 95, beyond the one-workgroup attention backward): dropout 0.2 in
    the encoder and the decoder, scheduled sampling 0.85 with free-running passes."""
    _set_dropout(trm_model, 0.2, 0.2, False)
    batch, (cnn_attn, lens, cap, cap_len, use_cap, seed) = _hook_batch(name)
    _compare_step(trm_model, trm_state, batch, cnn_attn, lens, cap, cap_len, use_cap, seed, 0.2)


def test_training_step_from_a_30s_wav_through_cnn14(trm_model, trm_state):
    """A 30 s clip through the whole step including the frozen Cnn14 (T' 93, L 94); teacher forcing, dropout 0.2."""
    from audiocaption_amd import procedural as Pr
    _set_dropout(trm_model, 0.2, 0.2, False)
    B, n = 4, 30 * 32000
    wav = torch.from_numpy(Pr.synthetic_wav(B, n, seed=4, varied=True)).to(DEV)
    wav_len = [n, n // 2, n - 40000, 5 * 32000]
    g = torch.Generator().manual_seed(8)
    cap = torch.randint(4, 4981, (B, 12), generator=g)
    cap[:, 0], cap[:, -1] = 1, 2
    cap_len = np.array([12] * B)
    batch = {"mode": "train", "wav": wav, "wav_len": wav_len, "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len,
             "ss_ratio": 1, "dropout_seed": 21}
    from audiocaption_amd.cnn_encoder import cnn14_feat_len
    cnn = trm_model.encoder.cnn
    lens = cnn14_feat_len(wav_len, cnn.hop_length, cnn.downsample_ratio)
    eng = _compare_step(trm_model, trm_state, batch, None, lens, cap, cap_len, [1] * 11, 21, 0.2, teacher_forcing=True)
    assert eng._saved is None and eng._states and next(iter(eng._states.values()))["Tq"] == 93


def test_reference_runner_surface_equals_the_fused_step(trm_state):
    """model(input_dict) + LabelSmoothingLoss + loss.backward() + torch.optim.Adam == TrainEngine.step + FusedAdam."""
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    a, b = _model(trm_state), _model(trm_state)
    for m in (a, b):
        _set_dropout(m, 0.2, 0.2, False)
    batch, _ = _hook_batch("bench_10s")
    batch = dict(batch, ss_ratio=1, dropout_seed=5)
    batch.pop("_use_cap")
    opt_a = torch.optim.Adam([p for p in a.parameters() if p.requires_grad], lr=5e-4, eps=1e-5, weight_decay=1e-6)
    out = a(batch)
    loss_a = LabelSmoothingLoss(smoothing=0.1)({"logit": out["logit"], "tgt": batch["cap"][:, 1:],
                                                 "tgt_len": torch.as_tensor(batch["cap_len"] - 1)})
    opt_a.zero_grad()
    loss_a.backward()
    torch.nn.utils.clip_grad_norm_([p for p in a.parameters() if p.requires_grad], 1.0)
    opt_a.step()
    eng = TrainEngine(b)
    opt_b = FusedAdam([p for p in b.parameters() if p.requires_grad], lr=5e-4, eps=1e-5, weight_decay=1e-6)
    r = eng.step(batch, opt_b, smoothing=0.1, max_grad_norm=1.0, use_graph=False)
    assert abs(float(r["loss"]) - float(loss_a)) <= 1e-5 * float(loss_a)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and set(trm_state) <= set(sa)
    worst = max(float((sa[k] - sb[k]).abs().max()) for k in sa if k.startswith(("encoder.trm.", "decoder.")))
    print("largest parameter difference after one step:", worst)
    assert worst < 5e-6


def _fixed_batch(B=4, seconds=10, seed=9):
    from audiocaption_amd import procedural as Pr
    n = seconds * 32000
    wav = torch.from_numpy(Pr.synthetic_wav(B, n, seed=seed)).to(DEV)
    g = torch.Generator().manual_seed(seed)
    cap = torch.randint(4, 4981, (B, 10), generator=g)
    cap[:, 0], cap[:, -1] = 1, 2
    return {"mode": "train", "wav": wav, "wav_len": [n] * B, "specaug": False, "cap": cap.to(DEV),
            "cap_len": np.array([10] * B), "ss_ratio": 0.8}


def _trajectory(state, batch, steps, **kw):
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    m = _model(state)
    eng = TrainEngine(m, seed=40)
    opt = FusedAdam([p for p in m.parameters() if p.requires_grad], lr=5e-4, eps=1e-5, weight_decay=1e-6)
    random.seed(3)
    losses = []
    for it in range(steps):
        nxt = batch if kw.get("lookahead") and it + 1 < steps else None
        r = eng.step(batch, opt, use_graph=kw.get("use_graph", True), next_batch=nxt)
        losses.append(float(r["loss"]))
    return losses, m, eng


def test_graph_replay_and_look_ahead_equal_eager(trm_state):
    batch = _fixed_batch()
    eager, _, _ = _trajectory(trm_state, batch, 4, use_graph=False)
    graph, _, eng = _trajectory(trm_state, batch, 4, use_graph=True)
    ahead, _, _ = _trajectory(trm_state, batch, 4, use_graph=True, lookahead=True)
    print("eager", eager, "graph", graph, "look-ahead", ahead)
    assert any(st["graphs"] for st in eng._states.values())
    np.testing.assert_allclose(graph, eager, rtol=1e-5)
    np.testing.assert_allclose(ahead, eager, rtol=1e-5)


def test_loss_falls_and_inference_uses_the_updated_weights(trm_state):
    batch = _fixed_batch()
    m0 = _model(trm_state).eval()
    inf = {"mode": "inference", "wav": batch["wav"], "wav_len": batch["wav_len"], "specaug": False,
           "sample_method": "greedy", "max_length": 10}
    with torch.no_grad():
        logit0 = m0(dict(inf))["logit"][:, 0].clone()
    losses, m, eng = _trajectory(trm_state, batch, 20)
    print("losses", [f"{v:.3f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.5
    assert eng.skipped_updates() == 0
    m.eval()
    with torch.no_grad():
        out = m(dict(inf))
    first = batch["cap"][:, 1]
    gain = out["logit"][:, 0].gather(1, first[:, None]) - logit0.gather(1, first[:, None])
    assert float(gain.min()) > 0.0
    # state_dict round trip: same keys, and a fresh model loaded from it decodes the same
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert sd.keys() == m0.state_dict().keys()
    m2 = _model(sd).eval()
    with torch.no_grad():
        out2 = m2(dict(inf))
    assert torch.equal(out2["seq"], out["seq"])


@pytest.mark.parametrize("tag", ["ss", "tf"])
def test_training_step_vs_reference_g15(trm_model, golden_dir, tag):
    """model(input_dict) + loss.backward() + clip + FusedAdam at p = 0 against one step the REFERENCE ran
    (tests/golden/g15_trm_train.npz): top-8 logits, greedy tokens, loss, every gradient, the total norm and the first
    Adam update, at the bars of the G8 step test."""
    from test_trm_train_ref_cpu import g15_inputs
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    g15, attn, lens, cap, cap_len = g15_inputs(golden_dir)
    model = trm_model
    _set_dropout(model, 0.0, 0.0, False)
    B, Tq = attn.shape[:2]
    ss_ratio = 1 if tag == "tf" else 0.7
    random.seed(5)   # the reference drew its scheduled-sampling choices from this stream
    out = model({"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
                 "wav_len": [320 * (32 * int(n) - 1) for n in lens], "specaug": False, "cap": cap.to(DEV),
                 "cap_len": cap_len, "ss_ratio": ss_ratio, "_cnn_attn": attn.to(DEV)})
    logit = out["logit"]
    top_val, top_idx = logit.detach().topk(8, dim=-1)
    assert rel("logit top-8", top_val, g15[f"{tag}_logit_top_val"]) < 2e-5
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g15[f"{tag}_logit_top_idx"][..., 0])
    if tag == "ss":
        assert np.array_equal(out["seq"].cpu().numpy(), g15["ss_seq"])
    loss = LabelSmoothingLoss(smoothing=0.1)({"logit": logit, "tgt": cap[:, 1:].to(DEV),
                                              "tgt_len": torch.as_tensor(cap_len - 1)})
    assert abs(float(loss) - float(g15[f"{tag}_loss"])) < 2e-5 * float(g15[f"{tag}_loss"])
    loss.backward()
    named = dict(model.named_parameters())
    bad = []
    keys = [k[len("sample_idx/"):] for k in g15 if k.startswith("sample_idx/")]
    assert set(keys) == {k for k, p in named.items() if p.requires_grad}
    for key in keys:
        grad = named[key].grad
        gn = float(g15[f"{tag}_gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g15[f"sample_idx/{key}"]).to(DEV)].cpu().numpy()
        d_s = float(np.abs(sample - g15[f"{tag}_gsample/{key}"]).max()) / (float(grad.abs().max()) + 1e-12)
        if not (d_norm < 1e-4 and d_s < 1e-4):
            bad.append((key, d_norm, d_s))
    assert not bad, f"gradients differ from the reference's: {bad}"
    params = [p for p in model.parameters() if p.requires_grad]
    before = {k: named[k].detach().clone() for k in keys}
    clip = clip_grad_norm_(params, 1.0)
    assert abs(float(clip.total_norm) - float(g15[f"{tag}_total_norm"])) < 1e-4 * float(g15[f"{tag}_total_norm"])
    FusedAdam(params, lr=5e-4, weight_decay=1e-6).step()
    for key in keys:
        idx = torch.from_numpy(g15[f"sample_idx/{key}"]).to(DEV)
        delta = (named[key].detach() - before[key]).reshape(-1)[idx].cpu().numpy()
        gs = np.abs(g15[f"{tag}_gsample/{key}"])
        solid = gs > 1e-4 * (gs.max() + 1e-30) + 1e-6
        assert np.abs(delta - g15[f"{tag}_delta/{key}"])[solid].max(initial=0.0) < 5e-6, key


def test_swa_over_the_encoder_and_decoder_flat_layout(trm_model):
    """SwaAverager over the flat buffer that now starts with the Transformer encoder's tensors: the running mean of the
    snapshots, for an encoder tensor (cls_token, first in the layout) and a decoder tensor."""
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    from audiocaption_amd.trainer import SwaAverager
    model = trm_model
    batch = _fixed_batch(B=2, seconds=3, seed=4)
    eng = TrainEngine(model)
    model._train_engine = eng
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    swa = SwaAverager(model)
    keys = ("encoder.trm.cls_token", "encoder.trm.model.layers.1.linear2.weight", "decoder.classifier.weight")
    snaps = []
    for _ in range(3):
        eng.step(batch, opt)
        named = dict(model.named_parameters())
        snaps.append({k: named[k].detach().clone() for k in keys})
        swa.update_parameters(model)
    assert eng.flat.names[0].startswith("encoder.trm.")
    for k in keys:
        want = sum(s[k] for s in snaps) / 3
        assert not torch.equal(snaps[0][k], snaps[2][k]), k
        assert rel(f"swa {k}", swa.state_dict()[k], want) < 1e-6
    assert swa.n_averaged == 3 and set(swa.state_dict()) == set(model.state_dict())


def test_refusals(trm_state):
    from audiocaption_amd.train import TrainEngine
    from audiocaption_amd.transformer_encoder import TransformerEncoder
    with pytest.raises(NotImplementedError):
        TrainEngine(_model(trm_state, freeze_cnn=False, freeze_cnn_bn=False))
    with pytest.raises(NotImplementedError):
        TransformerEncoder(-1, 2048, 2048, 512)
    # the engine's own checks: an encoder that is not 256 wide with 64-wide heads, a decoder memory of another width
    m = _model(trm_state)
    m.encoder.trm.d_model = 512
    with pytest.raises(NotImplementedError, match="d_model 256"):
        TrainEngine(m)
    import audiocaption_amd as A
    cfg = A.config.cnn14trm_trm_config(4981)
    cfg["decoder"]["args"]["attn_emb_dim"] = 512
    with pytest.raises(NotImplementedError, match="attn_emb_dim 512"):
        TrainEngine(A.init_model_from_config(cfg, print_fn=lambda s: None).to("cuda:0").train())
    m = _model(trm_state)
    with pytest.raises(NotImplementedError, match="whole-model training step"):
        m.encoder.trm({"attn": torch.zeros(1, 4, 2048, device=DEV), "attn_len": [4]})
    eng = TrainEngine(m)
    Tq = 126                                                  # L = 127: beyond the self-attention forward
    batch = {"mode": "train", "wav": torch.zeros(1, 320 * 32 * Tq, device=DEV), "wav_len": [320 * 32 * Tq - 320],
             "specaug": False, "cap": torch.tensor([[1, 5, 2]], device=DEV), "cap_len": np.array([3]), "ss_ratio": 1,
             "_cnn_attn": torch.zeros(1, Tq, 2048, device=DEV)}
    with pytest.raises(ValueError, match="at most 126 rows"):
        eng.forward(batch)
