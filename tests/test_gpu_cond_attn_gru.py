"""GPU tests of the condition-controlled attention-GRU captioners (ConditionalBahAttnDecoder, SpecificityBahAttnDecoder,
ConditionalSeq2SeqAttnModel; csrc/attn_gru.hip, csrc/attn_gru_train.hip under ac_bah_weights.variant) and of the specificity
loss (SpecificityLossWrapper, csrc/spec_loss.hip).

Against what the REFERENCE computed (tests/golden/g26_cond_attn_gru.npz): every id, the top-8 logits, the training steps of
the decoder alone and of the whole model.  Against the restatement of tests/_cond_attn_gru_ref.py in float64: every logit,
the attention weights, dropout with the project's counter-hash masks, the loss kernels.  Against BahAttnCatFcDecoder: the
metamorphic identity of the conditional decoder.

Bars: inference ids identical, logits GATE = 1e-4 absolute (tests/test_gpu_attn_gru.py); training LOGIT_BAR = LOSS_BAR = 2e-5
relative, GRAD_BAR = 1e-4 on gradient norms and samples, NORM_BAR, DELTA_BAR (tests/test_gpu_attn_gru_train.py); the loss
kernels LOSS_BAR / GRAD_BAR as recorded in the fixture (``loss_gate``: the reference's own float32 run stays within a quarter
of both).  Every figure is printed before it is asserted; tests/golden/REPORT_cond_attn_gru.txt keeps one run's.
"""
import random

import numpy as np
import pytest
import torch

import _attn_gru_ref as AR
import _attn_gru_train_ref as TR
import _cond_attn_gru_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GATE = 1e-4
LOGIT_BAR, LOSS_BAR, GRAD_BAR, NORM_BAR, DELTA_BAR = 2e-5, 2e-5, 1e-4, 1e-4, 5e-6


@pytest.fixture(scope="module")
def g26():
    from audiocaption_amd import build
    build.build()
    return R.load_g26()


def absdiff(name, got, want, gate):
    d = float((torch.as_tensor(got).detach().double().cpu() - torch.as_tensor(want).detach().double().cpu()).abs().max())
    print(f"[{name}] max |gpu - reference| {d:.3e} (gate {gate:.1e})")
    assert d <= gate, name


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f"[{name}] {d:.3e}")
    return d


def decoder_state(g26, kind, shape):
    if shape != "pub":
        return R.state(kind, shape, *R.recipe(g26, kind, shape))
    return {k[len("decoder."):]: v for k, v in R.pub_state(kind, *R.recipe(g26, kind, "pub")).items() if k.startswith("decoder.")}


def make_decoder(kind, shape, sd, p=0.0):
    import audiocaption_amd as A
    cls = {"cond": A.ConditionalBahAttnDecoder, "spec": A.SpecificityBahAttnDecoder}[kind]
    dec = cls(dropout=p, **R.SHAPES[shape])
    dec.load_state_dict(sd, strict=True)
    return dec.to(DEV)


# ---- inference ---------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.INFER))
def test_search_matches_the_reference(g26, kind, name):
    import audiocaption_amd as A
    shape = R.INFER[name][0]
    key = R.infer_prefix(kind, name)
    sd = decoder_state(g26, kind, shape)
    mem, lens, cond, L, beams = R.infer_inputs(name)
    B, Tm, _ = mem.shape
    model = A.ConditionalSeq2SeqAttnModel(torch.nn.Identity(), make_decoder(kind, shape, sd, 0.5)).eval()
    # fc_emb is not read by these decoders: NaNs in it must change nothing
    req = {"mode": "inference", "attn_emb": mem.to(DEV), "fc_emb": torch.full((B, R.SHAPES[shape]["fc_emb_dim"]), float("nan")),
           "attn_emb_len": lens, "max_length": L, "condition": cond}
    out = model(dict(req))
    ref64 = R.greedy(kind, sd, mem, lens, cond, L, dtype=torch.float64)
    assert out["seq"].dtype == torch.int64 and not out["seq"].is_cuda and not out["sampled_logprob"].is_cuda
    np.testing.assert_array_equal(out["seq"].numpy(), g26[f"{key}_greedy_seq"])
    live_np = AR.live_mask(out["seq"].numpy())
    live = torch.from_numpy(live_np)
    logit = out["logit"].cpu()
    tv, ti = logit.topk(8, dim=2)
    np.testing.assert_array_equal((ti.numpy() * live_np[..., None])[..., 0], g26[f"{key}_greedy_top_idx"][..., 0])
    absdiff(f"{kind} {name} top-8 logits", tv * live[..., None], g26[f"{key}_greedy_top_val"], GATE)
    absdiff(f"{kind} {name} logits (float64 restatement, every column)", logit, ref64["logit"], GATE)
    absdiff(f"{kind} {name} attn_weight", out["attn_weight"], ref64["attn_weight"], GATE)
    absdiff(f"{kind} {name} state", out["state"], ref64["state"], GATE)
    absdiff(f"{kind} {name} embed", out["embed"], ref64["embed"], GATE)
    assert tuple(out["attn_weight"].shape) == (B, Tm, L) and tuple(out["state"].shape) == (1, B, model.decoder.d_model)
    # the finished-row contract of attn_model.py
    dead = ~live
    assert not logit[dead].any() and not out["embed"].cpu()[dead].any() and not out["sampled_logprob"][dead].any()
    assert not out["attn_weight"].cpu().transpose(1, 2)[dead].any() and (out["seq"][dead] == R.END_IDX).all()
    # attention weights: 0 beyond a clip's frames, 1 in total at every live step
    w = out["attn_weight"].cpu()
    for i, ln in enumerate(lens.tolist()):
        assert not w[i, ln:, :].any(), f"clip {i}: weight on a masked frame"
        s = w[i].sum(0)[live[i]]
        assert float((s - 1).abs().max()) <= 2 * Tm * 2.0 ** -24, f"clip {i}: weights sum to {s.tolist()}"
    # greedy is sampling from the one best word
    top1 = model(dict(req, sample_method="top1", seed=3))
    assert torch.equal(top1["seq"], out["seq"]) and torch.equal(top1["logit"], out["logit"])
    # only the condition changes: other logits
    other = model(dict(req, condition=cond.roll(1) + 0.25))
    assert float((other["logit"][:, 0] - out["logit"][:, 0]).abs().max()) > 1e-3
    # a condition given as a device tensor or a list is the same request
    again = model(dict(req, condition=cond.to(DEV)))
    assert torch.equal(again["logit"], out["logit"]) and torch.equal(model(dict(req, condition=cond.tolist()))["seq"], out["seq"])
    for k in beams:
        b = model(dict(req, sample_method="beam", beam_size=k))
        np.testing.assert_array_equal(b["seq"].numpy(), g26[f"{key}_beam{k}_seq"])
        b64 = R.beam_search(kind, sd, mem, lens, cond, k, L, dtype=torch.float64)
        absdiff(f"{kind} {name} beam {k} attn_weight", b["attn_weight"], b64["attn_weight"], GATE)


@torch.no_grad()
@pytest.mark.parametrize("kind", R.KINDS)
def test_one_step_forward_contract(g26, kind):
    """``decoder(input_dict)``: one step from a non-zero state with the reference's keys plus ``condition``."""
    sd = decoder_state(g26, kind, "small")
    mem, lens, cond, _, _ = R.infer_inputs("small")
    dec = make_decoder(kind, "small", sd).eval()
    g = torch.Generator().manual_seed(5)
    h = torch.rand(5, dec.d_model, generator=g) * 2 - 1
    words = torch.randint(0, dec.vocab_size, (5, 1), generator=g)
    want = R.step(kind, AR.cast(sd, torch.float64), sd["word_embedding.weight"][words[:, 0]].double(), h.double(), mem.double(),
                  lens, cond)
    out = dec({"word": words, "state": h[None].to(DEV), "attn_emb": mem.to(DEV), "attn_emb_len": lens,
               "fc_emb": torch.zeros(5, 96), "condition": cond})
    assert tuple(out["logit"].shape) == (5, 1, 517) and tuple(out["state"].shape) == (1, 5, 128)
    assert tuple(out["embed"].shape) == (5, 1, 128) and tuple(out["attn_weight"].shape) == (5, 70)
    absdiff(f"{kind} step logit", out["logit"][:, 0], want[1], GATE)
    absdiff(f"{kind} step state", out["state"][0], want[0], GATE)
    absdiff(f"{kind} step attn_weight", out["attn_weight"], want[2], GATE)
    with pytest.raises(ValueError, match="condition"):
        dec({"word": words, "attn_emb": mem.to(DEV), "attn_emb_len": lens, "fc_emb": torch.zeros(5, 96)})


# ---- the metamorphic identity ---------------------------------------------------------------------------------------------
def test_conditional_decoder_is_a_catfc_decoder_on_two_columns(g26):
    """ConditionalBahAttnDecoder at condition c against a BahAttnCatFcDecoder whose fc_proj.weight holds
    condition_embedding.weight[0] and [1] in its first two columns (the other 30 zero, bias zero), fed fc_emb =
    [1 - c, c, 0, ...], F = 32: the same up to the order of a two-term f32 sum - logits of a search, and in training the
    gradients, d condition_embedding.weight being d fc_proj.weight[:, :2]^T."""
    import audiocaption_amd as A
    sd = decoder_state(g26, "cond", "small")
    mem, lens, cond, cap, cap_len = R.train_inputs("small")
    B, E, F = mem.shape[0], TR.SMALL["emb_dim"], 32
    cat_sd = {k: v for k, v in sd.items() if k != "condition_embedding.weight"}
    cat_sd["fc_proj.weight"] = torch.cat((sd["condition_embedding.weight"].T, torch.zeros(E, F - 2)), dim=1)
    cat_sd["fc_proj.bias"] = torch.zeros(E)
    fc = torch.cat((torch.stack((1 - cond, cond), dim=1), torch.zeros(B, F - 2)), dim=1)
    dec = make_decoder("cond", "small", sd).train()
    cat = A.BahAttnCatFcDecoder(dropout=0.0, **dict(TR.SMALL, fc_emb_dim=F))
    cat.load_state_dict(cat_sd, strict=True)
    cat = cat.to(DEV).train()
    with torch.no_grad():
        a = A.ConditionalSeq2SeqAttnModel(torch.nn.Identity(), dec)(
            {"mode": "inference", "attn_emb": mem.to(DEV), "fc_emb": fc.to(DEV), "attn_emb_len": lens, "max_length": 6,
             "condition": cond})
        b = A.Seq2SeqAttnModel(torch.nn.Identity(), cat)(
            {"mode": "inference", "attn_emb": mem.to(DEV), "fc_emb": fc.to(DEV), "attn_emb_len": lens, "max_length": 6})
    assert torch.equal(a["seq"], b["seq"])
    assert rel("metamorphic search logits", a["logit"], b["logit"]) < LOGIT_BAR
    use_cap = g26["cond_train_small_ss_use_cap"].tolist()
    args = (lens, cap.to(DEV), use_cap, None, R.START_IDX)
    fa = dec.train_forward(mem.to(DEV), cond, *args)
    fb = cat.train_forward(mem.to(DEV), fc.to(DEV), *args)
    assert torch.equal(fa["seq"], fb["seq"])
    assert rel("metamorphic training logits", fa["logit"], fb["logit"]) < LOGIT_BAR
    _, dlogit = _loss_and_dlogit(fb["logit"], cap, cap_len)
    ga, da, dfa = dec.train_backward(fa["saved"], dlogit)
    gb, db, _ = cat.train_backward(fb["saved"], dlogit)
    assert rel("metamorphic d condition_embedding", ga["condition_embedding.weight"], gb["fc_proj.weight"][:, :2].T) < GRAD_BAR
    for k in ga:
        if k != "condition_embedding.weight":
            assert rel(f"metamorphic d {k}", ga[k], gb[k]) < GRAD_BAR, k
    assert rel("metamorphic d attn_emb", da, db) < GRAD_BAR
    assert not dfa.any()


# ---- training: the decoder alone ------------------------------------------------------------------------------------------
def _loss_and_dlogit(logit, cap, cap_len):
    from audiocaption_amd.loss import LabelSmoothingLoss
    leaf = logit.detach().clone().requires_grad_(True)
    loss = LabelSmoothingLoss(smoothing=0.1)({"logit": leaf, "tgt": cap[:, 1:].to(DEV), "tgt_len": torch.as_tensor(cap_len - 1)})
    loss.backward()
    return float(loss.detach()), leaf.grad


def _decoder_step(dec, mem, lens, cond, cap, cap_len, use_cap, seed=0):
    out = dec.train_forward(mem.to(DEV), cond, lens, cap.to(DEV), use_cap, None, R.START_IDX, dropout_seed=seed)
    loss, dlogit = _loss_and_dlogit(out["logit"], cap, cap_len)
    grads, d_attn, d_fc = dec.train_backward(out["saved"], dlogit)
    return out, loss, grads, d_attn, d_fc


def _grads_vs_fixture(g26, prefix, idx_prefix, grads):
    bad = []
    for key, grad in grads.items():
        gn = float(g26[f"{prefix}_gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g26[f"{idx_prefix}_sample_idx/{key}"]).to(DEV)].cpu().numpy()
        d_s = float(np.abs(sample - g26[f"{prefix}_gsample/{key}"]).max()) / (float(grad.abs().max()) + 1e-12)
        print(f"[{prefix} {key}] norm {d_norm:.3e} samples {d_s:.3e}")
        if not (d_norm < GRAD_BAR and d_s < GRAD_BAR):
            bad.append((key, d_norm, d_s))
    assert not bad, f"gradients differ from the reference's: {bad}"


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name,tag", [(n, t) for n in R.TRAIN for t in ("tf", "ss")])
def test_decoder_step_vs_reference(g26, kind, name, tag):
    shape = R.TRAIN[name][0]
    case = f"{kind}_train_{name}_{tag}"
    sd = R.state(kind, shape, *R.recipe(g26, kind, shape))
    mem, lens, cond, cap, cap_len = R.train_inputs(name)
    dec = make_decoder(kind, shape, sd).train()
    out, loss, grads, d_attn, d_fc = _decoder_step(dec, mem, lens, cond, cap, cap_len, g26[f"{case}_use_cap"].tolist())
    top_val, top_idx = out["logit"].topk(8, dim=-1)
    assert rel(f"{case} logit top-8", top_val, g26[f"{case}_logit_top_val"]) < LOGIT_BAR
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g26[f"{case}_logit_top_idx"][..., 0])
    assert np.array_equal(out["seq"].cpu().numpy(), g26[f"{case}_seq"])
    if f"{case}_attn_weight" in g26:
        assert rel(f"{case} attn_weight", out["attn_weight"], g26[f"{case}_attn_weight"]) < LOGIT_BAR
    want = float(g26[f"{case}_loss"])
    print(f"[{case} loss] {abs(loss - want) / want:.3e}")
    assert abs(loss - want) < LOSS_BAR * want
    assert torch.equal(out["embed"][:, -1], out["state"][0])
    named = {"decoder." + k: v for k, v in grads.items()}
    named["attn_emb"] = d_attn
    assert set(named) == {k.split("/", 1)[1] for k in g26 if k.startswith(f"{case}_gnorm/")}
    _grads_vs_fixture(g26, case, f"{kind}_train_{name}", named)
    # the last column of the odd-pitch weight_ih_l0 (the raw condition's) has its own gradient path: all of it, in float64
    if kind == "spec":
        ref = R.decoder_step_grads(kind, sd, mem, lens, cond, cap, cap_len, g26[f"{case}_use_cap"].tolist(),
                                   dtype=torch.float64)["grads"]["model.weight_ih_l0"]
        assert rel(f"{case} d weight_ih_l0[:, -1]", grads["model.weight_ih_l0"][:, -1], ref[:, -1]) < GRAD_BAR
        assert rel(f"{case} d weight_ih_l0", grads["model.weight_ih_l0"], ref) < GRAD_BAR
    # neither decoder reads fc_emb; frames at or beyond a clip's length get exactly zero
    assert not d_fc.any() and tuple(d_fc.shape) == (mem.shape[0], R.SHAPES[shape]["fc_emb_dim"])
    for b, n in enumerate(lens.tolist()):
        assert not d_attn[b, n:].any()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("tag", ["tf", "ss"])
def test_dropout_vs_restatement(g26, kind, tag):
    """in_dropout 0.5 with the project's counter-hash masks, regenerated in the backward, against float64."""
    sd = R.state(kind, "small", *R.recipe(g26, kind, "small"))
    mem, lens, cond, cap, cap_len = R.train_inputs("small")
    use_cap = g26[f"{kind}_train_small_{tag}_use_cap"].tolist()
    seed = 77
    want = R.decoder_step_grads(kind, sd, mem, lens, cond, cap, cap_len, use_cap, p=0.5, base_seed=seed, dtype=torch.float64)
    gap = TR.fed_back_gaps(want["gap"], use_cap, False)
    assert not gap.numel() or float(gap.min()) >= GATE, f"near-tie {float(gap.min()):.1e} on a fed-back step: choose another seed"
    dec = make_decoder(kind, "small", sd, p=0.5).train()
    out, loss, grads, d_attn, d_fc = _decoder_step(dec, mem, lens, cond, cap, cap_len, use_cap, seed)
    name = f"{kind} dropout {tag}"
    assert torch.equal(out["seq"].cpu(), want["seq"])
    assert rel(f"{name} logit", out["logit"], want["logit"]) < LOGIT_BAR
    print(f"[{name} loss] {abs(loss - float(want['loss'])) / float(want['loss']):.3e}")
    assert abs(loss - float(want["loss"])) < LOSS_BAR * float(want["loss"])
    bad = []
    for key, got in list(grads.items()) + [("attn_emb", d_attn)]:
        ref = want["grads"][key] if key in want["grads"] else want["d_" + key]
        d_norm = abs(float(got.double().norm()) - float(ref.norm())) / (float(ref.norm()) + 1e-12)
        d_s = rel(f"{name} {key}", got, ref)
        if not (d_norm < GRAD_BAR and d_s < GRAD_BAR):
            bad.append((key, d_norm, d_s))
    assert not bad, bad
    assert not d_fc.any()
    args = (mem.to(DEV), cond, lens, cap.to(DEV), use_cap, None, R.START_IDX)
    assert torch.equal(dec.train_forward(*args, dropout_seed=seed)["logit"], out["logit"])
    assert not torch.equal(dec.train_forward(*args, dropout_seed=seed + 1)["logit"], out["logit"])


# ---- training: the whole model through the reference runner's surface ----------------------------------------------------
def _pub_model(kind, state):
    import audiocaption_amd as A
    cfg = A.cnn14rnn_trm_config(TR.PUB["vocab_size"])
    cfg["encoder"]["rnn"]["args"]["dropout"] = 0.0
    name = {"cond": "ConditionalBahAttnDecoder", "spec": "SpecificityBahAttnDecoder"}[kind]
    cfg["decoder"] = {"type": "captioning.models.rnn_decoder." + name, "args": dict(TR.PUB, dropout=0.0)}
    cfg["type"] = "captioning.models.attn_model.ConditionalSeq2SeqAttnModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s: None)
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.startswith("encoder.cnn.") for k in missing)   # the Cnn14 is preset: never run
    model = model.to("cuda:0").train()
    model.encoder.cnn.eval()
    return model


@pytest.mark.parametrize("kind", R.KINDS)
def test_model_step_vs_reference(g26, kind):
    """model(input_dict) + SpecificityLossWrapper(LabelSmoothingLoss(0.1), ws, "sum", 0.3) + loss.backward() +
    clip_grad_norm_ + FusedAdam against the step the reference ran; the Cnn14 features go in through ``_cnn_attn``."""
    import audiocaption_amd as A
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    case = f"{kind}_train_pub_ss"
    model = _pub_model(kind, R.pub_state(kind, *R.recipe(g26, kind, "pub")))
    attn = TR.pub_cnn_attn()
    cap, cap_len = TR.pub_caption()
    cond = R.conditions(TR.PUB_N, 2)
    B, Tq = attn.shape[:2]
    batch = {"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
             "wav_len": [320 * (32 * int(n) - 1) for n in TR.PUB_LENS], "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len,
             "ss_ratio": 0.7, "condition": cond, "_cnn_attn": attn.to(DEV)}
    with pytest.raises(ValueError, match="condition"):
        model({k: v for k, v in batch.items() if k != "condition"})
    random.seed(int(g26["coin_seed"]))
    out = model(batch)
    after = random.random()
    random.seed(int(g26["coin_seed"]))
    assert after == [random.random() for _ in range(cap.shape[1])][-1], "one coin per step, drawn from Python's stream"
    logit = out["logit"]
    assert logit.requires_grad and tuple(logit.shape) == (TR.PUB_N, TR.PUB_TC - 1, TR.PUB["vocab_size"])
    top_val, top_idx = logit.detach().topk(8, dim=-1)
    assert rel(f"{case} logit top-8", top_val, g26[f"{case}_logit_top_val"]) < LOGIT_BAR
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g26[f"{case}_logit_top_idx"][..., 0])
    assert np.array_equal(out["seq"].numpy(), g26[f"{case}_seq"])
    wrap = A.SpecificityLossWrapper(LabelSmoothingLoss(smoothing=0.1), R.word_specificity(TR.PUB["vocab_size"]), "sum", R.ALPHA)
    losses = wrap({"logit": logit, "tgt": cap[:, 1:].to(DEV), "tgt_len": torch.as_tensor(cap_len - 1), "conditions": cond})
    for k, got in zip(("loss", "word_loss", "condition_loss"), losses):
        want = float(g26[f"{case}_{k}"])
        print(f"[{case} {k}] {abs(float(got.detach()) - want) / want:.3e}")
        assert abs(float(got.detach()) - want) < LOSS_BAR * want
    losses[0].backward()
    named = dict(model.named_parameters())
    keys = [k[len(f"{kind}_train_pub_sample_idx/"):] for k in g26 if k.startswith(f"{kind}_train_pub_sample_idx/")]
    assert set(keys) == {k for k, p in named.items() if p.requires_grad}
    _grads_vs_fixture(g26, case, f"{kind}_train_pub", {k: named[k].grad for k in keys})
    params = [p for p in model.parameters() if p.requires_grad]
    before = {k: named[k].detach().clone() for k in keys}
    clip = clip_grad_norm_(params, 1.0)
    tn = float(g26[f"{case}_total_norm"])
    print(f"[{case} total norm] {abs(float(clip.total_norm) - tn) / tn:.3e}")
    assert abs(float(clip.total_norm) - tn) < NORM_BAR * tn
    # the reference's own float32 total is up to 9e-5 away from the norm of its own gradients (one tensor of 786k entries
    # carries nearly all of it); against that norm, summed in float64 from the recorded per-tensor norms:
    tn64 = float(np.sqrt(sum(float(g26[f"{case}_gnorm/{k}"]) ** 2 for k in keys)))
    print(f"[{case} total norm vs the recorded gradients'] {abs(float(clip.total_norm) - tn64) / tn64:.3e}")
    assert abs(float(clip.total_norm) - tn64) < GRAD_BAR * tn64
    FusedAdam(params, lr=5e-4, weight_decay=1e-6).step()
    worst = 0.0
    for key in keys:
        idx = torch.from_numpy(g26[f"{kind}_train_pub_sample_idx/{key}"]).to(DEV)
        delta = (named[key].detach() - before[key]).reshape(-1)[idx].cpu().numpy()
        gs = np.abs(g26[f"{case}_gsample/{key}"])
        solid = gs > 1e-4 * (gs.max() + 1e-30) + 1e-6
        d = np.abs(delta - g26[f"{case}_delta/{key}"])[solid].max(initial=0.0)
        worst = max(worst, float(d))
        assert d < DELTA_BAR, key
    print(f"[{case} Adam delta] {worst:.3e}")
    # the step after the update reads the new weights (the specificity decoder's pack of weight_ih_l0 is rebuilt)
    random.seed(int(g26["coin_seed"]))
    with torch.no_grad():
        assert not torch.equal(model(batch)["logit"], logit.detach())


# ---- the loss kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LOSS_GRID, ids=R.loss_case_name)
def test_specificity_loss_vs_float64(g26, case):
    import audiocaption_amd as A
    logit, tgt_len, conds, ws, reduce, alpha = R.loss_inputs(case)
    gate_loss, gate_grad = g26["loss_gate"].tolist()
    name = R.loss_case_name(case)
    l64 = logit.double().requires_grad_(True)
    word64 = R.stand_in_word_loss({"logit": l64})
    cl64 = R.specificity_loss(l64, ws.double(), tgt_len, conds.double(), reduce)
    (word64 + alpha * cl64).backward()
    leaf = logit.to(DEV).requires_grad_(True)
    wrap = A.SpecificityLossWrapper(R.stand_in_word_loss, ws, reduce, alpha)
    loss, word, cl = wrap({"logit": leaf, "tgt_len": tgt_len, "conditions": conds})
    for k, got, want in (("loss", loss, word64 + alpha * cl64), ("word_loss", word, word64), ("condition_loss", cl, cl64)):
        d = abs(float(got.detach()) - float(want.detach())) / (abs(float(want.detach())) + 1e-30)
        print(f"[loss {name} {k}] {d:.3e}")
        assert d < gate_loss, k
    assert np.allclose([float(loss.detach()), float(word.detach()), float(cl.detach())], g26[f"loss_{name}_losses"], rtol=gate_loss)
    loss.backward()
    assert rel(f"loss {name} d logit", leaf.grad, l64.grad) < gate_grad
    # the condition term alone: exact zeros in the rows that do not count, every row sums to 0
    alone = logit.to(DEV).requires_grad_(True)
    wrap({"logit": alone, "tgt_len": tgt_len, "conditions": conds})[2].backward()
    l64c = logit.double().requires_grad_(True)
    R.specificity_loss(l64c, ws.double(), tgt_len, conds.double(), reduce).backward()
    assert rel(f"loss {name} d logit (condition term)", alone.grad, l64c.grad) < gate_grad
    counted = torch.arange(logit.shape[1])[None, :] < (tgt_len - 1)[:, None]
    assert not alone.grad.cpu()[~counted].any()
    assert counted.any() and alone.grad.cpu()[counted].abs().sum() > 0
    rows = float(alone.grad.double().sum(-1).abs().max()) / float(alone.grad.abs().max())
    print(f"[loss {name} row sums / max] {rows:.3e}")
    assert rows < logit.shape[2] * 2.0 ** -23
