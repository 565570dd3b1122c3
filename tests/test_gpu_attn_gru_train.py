"""GPU tests of the training path of the attention-GRU captioners (csrc/attn_gru_train.hip, rnn_decoder.train_forward /
train_backward, train_attn_gru.AttnGruTrainEngine, Seq2SeqAttnModel.forward with mode="train").

Against steps the REFERENCE ran (tests/golden/g22_attn_gru_train.npz, p = 0): the decoder alone (case 1) and the whole
model through the reference runner's surface (case 2).  Against the restatement of tests/_attn_gru_train_ref.py in
float64: dropout with the same counter-hash masks, and an audio memory longer than one round of the attention kernels'
256 threads.  The bars are those of test_gpu_train_trm.py::test_training_step_vs_reference_g15: logits and loss 2e-5
relative, gradient norms and samples 1e-4, total norm 1e-4, Adam deltas 5e-6 on the solid samples, identical top-1 ids
and seq.  Measured worst ratios: tests/golden/REPORT_attn_gru_train.txt."""
import ctypes
import random

import numpy as np
import pytest
import torch

import _attn_gru_train_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOGIT_BAR, LOSS_BAR, GRAD_BAR, NORM_BAR, DELTA_BAR = 2e-5, 2e-5, 1e-4, 1e-4, 5e-6
GATE = 1e-4


@pytest.fixture(scope="module")
def g22():
    from audiocaption_amd import build
    build.build()
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


def _loss_and_dlogit(logit, cap, cap_len):
    """LabelSmoothingLoss(0.1) of the package on the device: (loss, d loss / d logit)."""
    from audiocaption_amd.loss import LabelSmoothingLoss
    leaf = logit.detach().clone().requires_grad_(True)
    loss = LabelSmoothingLoss(smoothing=0.1)({"logit": leaf, "tgt": cap[:, 1:].to(DEV), "tgt_len": torch.as_tensor(cap_len - 1)})
    loss.backward()
    return float(loss.detach()), leaf.grad


def _decoder_step(dec, mem, lens, fc, cap, cap_len, use_cap, tags, seed=0):
    out = dec.train_forward(mem.to(DEV), fc.to(DEV), lens, cap.to(DEV), use_cap,
                            None if tags is None else tags.to(device=DEV, dtype=torch.int32), R.START_IDX, dropout_seed=seed)
    loss, dlogit = _loss_and_dlogit(out["logit"], cap, cap_len)
    grads, d_attn, d_fc = dec.train_backward(out["saved"], dlogit)
    return out, loss, grads, d_attn, d_fc


def _grads_vs_fixture(g22, prefix, idx_prefix, grads):
    """Gradient norm and 64 samples of every tensor against the fixture; returns (worst norm ratio, worst sample ratio)."""
    worst_n = worst_s = 0.0
    bad = []
    for key, grad in grads.items():
        gn = float(g22[f"{prefix}_gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g22[f"{idx_prefix}_sample_idx/{key}"]).to(DEV)].cpu().numpy()
        d_s = float(np.abs(sample - g22[f"{prefix}_gsample/{key}"]).max()) / (float(grad.abs().max()) + 1e-12)
        print(f"[{prefix} {key}] norm {d_norm:.3e} samples {d_s:.3e}")
        worst_n, worst_s = max(worst_n, d_norm), max(worst_s, d_s)
        if not (d_norm < GRAD_BAR and d_s < GRAD_BAR):
            bad.append((key, d_norm, d_s))
    assert not bad, f"gradients differ from the reference's: {bad}"
    return worst_n, worst_s


# ---- case 1: the decoder alone against the reference ---------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", [("t", "tf"), ("t", "ss"), ("p", "tf"), ("p", "ss")])
def test_decoder_step_vs_reference_g22(g22, kind, tag):
    temporal = kind == "t"
    case = f"small_{kind}_{tag}"
    sd = R.small_state(temporal, *g22[f"small_{kind}_recipe"])
    mem, lens, fc, tags = R.small_inputs()
    cap, cap_len = R.small_caption()
    dec = _decoder(temporal, sd)
    out, loss, grads, d_attn, d_fc = _decoder_step(dec, mem, lens, fc, cap, cap_len, g22[f"{case}_use_cap"].tolist(),
                                                   tags if temporal else None)
    top_val, top_idx = out["logit"].topk(8, dim=-1)
    assert rel(f"{case} logit top-8", top_val, g22[f"{case}_logit_top_val"]) < LOGIT_BAR
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g22[f"{case}_logit_top_idx"][..., 0])
    assert np.array_equal(out["seq"].cpu().numpy(), g22[f"{case}_seq"])
    assert rel(f"{case} attn_weight", out["attn_weight"], g22[f"{case}_attn_weight"]) < LOGIT_BAR
    want = float(g22[f"{case}_loss"])
    print(f"[{case} loss] {abs(loss - want) / want:.3e}")
    assert abs(loss - want) < LOSS_BAR * want
    # embed is the GRU output of every step, state the last one; sampled_logprob the value of the arg-max
    assert torch.equal(out["embed"][:, -1], out["state"][0])
    lp = torch.log_softmax(out["logit"], -1).max(-1).values
    assert float((out["sampled_logprob"] - lp).abs().max()) < 1e-5
    named = {"decoder." + k: v for k, v in grads.items()}
    named.update(attn_emb=d_attn, fc_emb=d_fc)
    assert set(named) == {k.split("/", 1)[1] for k in g22 if k.startswith(f"{case}_gnorm/")}
    _grads_vs_fixture(g22, case, f"small_{kind}", named)
    # frames at or beyond a clip's length: exactly zero
    for b, n in enumerate(R.SMALL_LENS):
        assert not d_attn[b, n:].any()


# ---- case 2: the whole model through the reference runner's surface ------------------------------------------------------
def _pub_model(state, p_dec=0.0, p_rnn=0.0):
    import audiocaption_amd as A
    cfg = A.cnn14rnn_trm_config(R.PUB["vocab_size"])
    cfg["encoder"]["rnn"]["args"]["dropout"] = p_rnn
    cfg["decoder"] = {"type": "audiocaption_amd.rnn_decoder.TemporalBahAttnDecoder", "args": dict(R.PUB, dropout=p_dec)}
    cfg["type"] = "audiocaption_amd.attn_model.TemporalSeq2SeqAttnModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s: None)
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.startswith("encoder.cnn.") for k in missing)   # the Cnn14 is preset: never run
    model = model.to("cuda:0").train()
    model.encoder.cnn.eval()
    return model


def _pub_batch(ss_ratio=0.7):
    attn = R.pub_cnn_attn()
    cap, cap_len = R.pub_caption()
    B, Tq = attn.shape[:2]
    return {"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
            "wav_len": [320 * (32 * int(n) - 1) for n in R.PUB_LENS], "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len,
            "ss_ratio": ss_ratio, "temporal_tag": torch.tensor(R.PUB_TAGS), "_cnn_attn": attn.to(DEV)}, cap, cap_len


@pytest.fixture(scope="module")
def pub_state(g22):
    return R.pub_state(*g22["pub_recipe"])


def test_model_step_vs_reference_g22(g22, pub_state):
    """model(input_dict) + LabelSmoothingLoss + loss.backward() + clip_grad_norm_ + FusedAdam at p = 0 against the step the
    reference ran: top-8 logits, seq, loss, the encoder GRU's and the decoder's gradients, the total norm, the first update."""
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    model = _pub_model(pub_state)
    batch, cap, cap_len = _pub_batch()
    assert abs(float(batch["_cnn_attn"].double().sum()) - float(g22["pub_attn_sum"])) < 1e-6 * float(g22["pub_attn_sum"])
    random.seed(int(g22["coin_seed"]))
    out = model(batch)
    after = random.random()
    random.seed(int(g22["coin_seed"]))
    assert after == [random.random() for _ in range(cap.shape[1])][-1], "one coin per step, drawn from Python's stream"
    logit = out["logit"]
    assert logit.requires_grad and tuple(logit.shape) == (R.PUB_N, R.PUB_TC - 1, R.PUB["vocab_size"])
    assert tuple(out["attn_weight"].shape) == (R.PUB_N, R.PUB_TQ, R.PUB_TC - 1) and not out["seq"].is_cuda
    assert tuple(out["state"].shape) == (1, R.PUB_N, 512) and tuple(out["embed"].shape) == (R.PUB_N, R.PUB_TC - 1, 512)
    assert torch.equal(torch.as_tensor(out["attn_emb_len"]), torch.tensor(R.PUB_LENS))
    top_val, top_idx = logit.detach().topk(8, dim=-1)
    assert rel("pub logit top-8", top_val, g22["pub_ss_logit_top_val"]) < LOGIT_BAR
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g22["pub_ss_logit_top_idx"][..., 0])
    assert np.array_equal(out["seq"].numpy(), g22["pub_ss_seq"])
    loss = LabelSmoothingLoss(smoothing=0.1)({"logit": logit, "tgt": cap[:, 1:].to(DEV), "tgt_len": torch.as_tensor(cap_len - 1)})
    want = float(g22["pub_ss_loss"])
    print(f"[pub loss] {abs(float(loss) - want) / want:.3e}")
    assert abs(float(loss) - want) < LOSS_BAR * want
    loss.backward()
    named = dict(model.named_parameters())
    keys = [k[len("pub_sample_idx/"):] for k in g22 if k.startswith("pub_sample_idx/")]
    assert set(keys) == {k for k, p in named.items() if p.requires_grad}
    assert any(k.startswith("encoder.rnn.") for k in keys) and any(k.startswith("decoder.") for k in keys)
    _grads_vs_fixture(g22, "pub_ss", "pub", {k: named[k].grad for k in keys})
    params = [p for p in model.parameters() if p.requires_grad]
    before = {k: named[k].detach().clone() for k in keys}
    clip = clip_grad_norm_(params, 1.0)
    tn = float(g22["pub_ss_total_norm"])
    print(f"[pub total norm] {abs(float(clip.total_norm) - tn) / tn:.3e}")
    assert abs(float(clip.total_norm) - tn) < NORM_BAR * tn
    FusedAdam(params, lr=5e-4, weight_decay=1e-6).step()
    worst = 0.0
    for key in keys:
        idx = torch.from_numpy(g22[f"pub_sample_idx/{key}"]).to(DEV)
        delta = (named[key].detach() - before[key]).reshape(-1)[idx].cpu().numpy()
        gs = np.abs(g22[f"pub_ss_gsample/{key}"])
        solid = gs > 1e-4 * (gs.max() + 1e-30) + 1e-6
        d = np.abs(delta - g22[f"pub_ss_delta/{key}"])[solid].max(initial=0.0)
        worst = max(worst, float(d))
        assert d < DELTA_BAR, key
    print(f"[pub Adam delta] {worst:.3e}")


def test_eval_and_no_grad_return_plain_logits(pub_state):
    model = _pub_model(pub_state, p_dec=0.5)
    batch, _, _ = _pub_batch()
    random.seed(1)
    with torch.no_grad():
        a = model(batch)["logit"]
    model.eval()
    random.seed(1)
    b = model(batch)["logit"]
    assert not a.requires_grad and not b.requires_grad and a.grad_fn is None and b.grad_fn is None
    assert not torch.equal(a, b)      # train mode drops inputs at p = 0.5, eval mode does not
    with pytest.raises(ValueError, match="temporal_tag"):
        model(dict(batch, temporal_tag=[0, 1, 2, 4]))


def test_loss_goes_down(pub_state):
    """30 steps on case 2's batch through the autograd route with FusedAdam: finite throughout, and the loss ends below
    where it started by the margin test_gpu_train_trm.py asks of its own run."""
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    model = _pub_model(pub_state, p_dec=0.2, p_rnn=0.2)
    batch, cap, cap_len = _pub_batch()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdam(params, lr=5e-4, eps=1e-5, weight_decay=1e-6)
    loss_fn = LabelSmoothingLoss(smoothing=0.1)
    tgt, tgt_len = cap[:, 1:].to(DEV), torch.as_tensor(cap_len - 1)
    random.seed(3)
    losses = []
    for _ in range(30):
        out = model(batch)
        loss = loss_fn({"logit": out["logit"], "tgt": tgt, "tgt_len": tgt_len})
        opt.zero_grad()
        loss.backward()
        clip_grad_norm_(params, 1.0)
        opt.step()
        losses.append(float(loss))
    print("losses", [f"{v:.3f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.5


# ---- against the restatement: dropout, long memory --------------------------------------------------------------------
def _vs_restatement(name, dec, sd, mem, lens, fc, cap, cap_len, use_cap, tags, p, seed):
    want = R.decoder_step_grads(sd, mem, lens, fc, cap, cap_len, use_cap, tags, p=p, base_seed=seed, dtype=torch.float64)
    gap = R.fed_back_gaps(want["gap"], use_cap, tags is not None)
    assert gap.numel() and float(gap.min()) >= GATE, f"near-tie {float(gap.min()):.1e} on a fed-back step: choose another seed"
    out, loss, grads, d_attn, d_fc = _decoder_step(dec, mem, lens, fc, cap, cap_len, use_cap, tags, seed)
    assert torch.equal(out["seq"].cpu(), want["seq"])
    assert rel(f"{name} logit", out["logit"], want["logit"]) < LOGIT_BAR
    assert rel(f"{name} attn_weight", out["attn_weight"], want["attn_weight"]) < LOGIT_BAR
    print(f"[{name} loss] {abs(loss - float(want['loss'])) / float(want['loss']):.3e}")
    assert abs(loss - float(want["loss"])) < LOSS_BAR * float(want["loss"])
    bad = []
    for key, got in list(grads.items()) + [("attn_emb", d_attn), ("fc_emb", d_fc)]:
        ref = want["grads"][key] if key in want["grads"] else want["d_" + key]
        d_norm = abs(float(got.double().norm()) - float(ref.norm())) / (float(ref.norm()) + 1e-12)
        d_s = rel(f"{name} {key}", got, ref)
        if not (d_norm < GRAD_BAR and d_s < GRAD_BAR):
            bad.append((key, d_norm, d_s))
    assert not bad, bad
    return out, d_attn


def test_dropout_vs_restatement(g22):
    """Case 1 (temporal, ss_ratio 0.7's coins) with in_dropout 0.2: the same counter-hash masks in the restatement."""
    sd = R.small_state(True, *g22["small_t_recipe"])
    mem, lens, fc, tags = R.small_inputs()
    cap, cap_len = R.small_caption()
    use_cap = g22["small_t_ss_use_cap"].tolist()
    dec = _decoder(True, sd, p=0.2)
    out, _ = _vs_restatement("dropout", dec, sd, mem, lens, fc, cap, cap_len, use_cap, tags, 0.2, 77)
    args = (mem.to(DEV), fc.to(DEV), lens, cap.to(DEV), use_cap, tags.to(device=DEV, dtype=torch.int32), R.START_IDX)
    again = dec.train_forward(*args, dropout_seed=77)["logit"]
    other = dec.train_forward(*args, dropout_seed=78)["logit"]
    assert torch.equal(again, out["logit"]) and not torch.equal(other, out["logit"])
    dec.eval()      # the constructor's dropout takes effect in train mode only
    plain = dec.train_forward(*args, dropout_seed=77)["logit"]
    assert rel("eval == p 0", plain, _decoder(True, sd).train_forward(*args)["logit"]) == 0.0


def test_long_memory_vs_restatement():
    """B 2, Tm 300, lengths [300, 257], T 3: the frame loops of the attention kernels run a second round of 256 threads."""
    sd = R.small_state(False, 19, 3.0)
    mem = torch.from_numpy(np.random.default_rng(23).normal(0.0, 0.25, (2, 300, 160)).astype(np.float32))
    lens = torch.tensor([300, 257])
    valid = (torch.arange(300)[None, :] < lens[:, None]).float()
    fc = ((mem * valid[:, :, None]).sum(1) / lens[:, None].float())[:, :R.SMALL["fc_emb_dim"]].contiguous()
    cap, cap_len = R.caption(2, 4, [4, 3], R.SMALL["vocab_size"], 14)
    dec = _decoder(False, sd)
    _, d_attn = _vs_restatement("long", dec, sd, mem, lens, fc, cap, cap_len, [1, 0, 0], None, 0.0, 0)
    assert not d_attn[1, 257:].any() and d_attn[1, 256].any() and d_attn[0, 299].any()


# ---- refusals before any launch ----------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(g22):
    import audiocaption_amd as A
    from audiocaption_amd import _lib
    lib = _lib.load()
    dec = _decoder(True, R.small_state(True, 19, 3.0))
    w = dec.weights()
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(w), 5, 70, 8) > 0
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(w), 5, 4096, 8) == -1
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(w), 0, 70, 8) == -1
    assert lib.ac_bah_train_workspace_floats(None, 5, 70, 8) == -1
    bad = _lib.AcBahWeights.from_buffer_copy(w)
    bad.attn_size = 100
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(bad), 5, 70, 8) == -1
    one = torch.zeros(64, device=DEV)
    p = ctypes.c_void_p(one.data_ptr())
    coins = (ctypes.c_int * 8)(*([1] * 8))
    s = _lib.stream()
    fwd = [ctypes.byref(w), p, p, p, p, 9, coins, p, 5, 70, 8, 1, 0.0, 0, None, p, p, p, p, p, p, p, s]
    for i, v in ((0, ctypes.byref(bad)), (1, None), (6, None), (7, None), (9, 4096), (12, 1.0), (15, None), (21, None)):
        args = list(fwd)
        args[i] = v
        assert lib.ac_bah_train_forward(*args) == _lib.AC_ERR_ARG, i
    g = dec.grad_struct(lambda name: one.data_ptr())
    bwd = [ctypes.byref(w), ctypes.byref(g), p, p, p, p, 5, 70, 8, 0.0, 0, None, p, p, p, s]
    no_emb = dec.grad_struct(lambda name: one.data_ptr())
    no_emb.emb = None
    for i, v in ((0, ctypes.byref(bad)), (1, None), (1, ctypes.byref(no_emb)), (5, None), (7, 4096), (12, None), (14, None)):
        args = list(bwd)
        args[i] = v
        assert lib.ac_bah_train_backward(*args) == _lib.AC_ERR_ARG, i
    assert lib.ac_bah_mean_lens_bwd(None, p, p, 2, 3, 64, 64, s) == _lib.AC_ERR_ARG
    assert lib.ac_bah_mean_lens_bwd(p, p, p, 2, 3, 32, 64, s) == _lib.AC_ERR_ARG     # F > A
    torch.cuda.synchronize()
    model = A.TemporalSeq2SeqAttnModel(torch.nn.Identity(), dec)
    with pytest.raises(NotImplementedError, match="train"):
        model({"mode": "train", "attn_emb": one, "cap": torch.zeros(1, 3, dtype=torch.long), "ss_ratio": 1})


def test_mean_lens_backward_into_the_first_features():
    """d attn_emb[b, t, c] += d fc_emb[b, c] / len[b] on the valid frames, only into the first F features."""
    from audiocaption_amd import _lib
    lib = _lib.load()
    B, Tm, A_, F = 3, 7, 64, 32
    g = torch.Generator().manual_seed(2)
    d_fc, base = torch.randn(B, F, generator=g), torch.randn(B, Tm, A_, generator=g)
    lens = torch.tensor([7, 3, 1], dtype=torch.int32)
    got, d_fc_dev, lens_dev = base.clone().to(DEV), d_fc.to(DEV), lens.to(DEV)
    _lib.check(lib.ac_bah_mean_lens_bwd(d_fc_dev.data_ptr(), lens_dev.data_ptr(), got.data_ptr(), B, Tm, A_, F,
                                        _lib.stream()), "ac_bah_mean_lens_bwd")
    want = base.clone()
    for b in range(B):
        want[b, :int(lens[b]), :F] += d_fc[b] / float(lens[b])
    assert float((got.cpu() - want).abs().max()) < 1e-6
