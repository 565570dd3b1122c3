"""GPU tests of the keyword-conditioned Transformer captioner: the PRO_EMBED_KW producer of csrc/decoder.hip through the new
entry points against float64, the searches / the eval-mode forward / the training step against what the REFERENCE produced
(tests/golden/g27_keyword_trm.npz), and the training step with dropout against the restatement of tests/_keyword_trm_ref.py.
Every figure a gate is held to is printed as ``[name] value`` (REPORT_keyword_trm.txt records a run's worst ones)."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch

import _keyword_trm_ref as R
from _decoder_shapes import LOGIT_BAR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 1024                    # guard floats on either side of a buffer (tests/test_gpu_attn_gru_edges.py)
SENTINEL = 0x7FA5C3E1       # a NaN with a payload no kernel produces
GATE = R.GATE


@pytest.fixture(scope="module")
def g27():
    return R.load_g27()


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f"[{name}] {d:.3e}")
    return d


def _decoder(shape, state=None, **over):
    import audiocaption_amd as A
    from audiocaption_amd import build
    build.build()
    kw = dict(R.SHAPES[shape], dropout=0.2)
    kw.update(over)
    dec = A.KeywordProbTransformerDecoder(**kw)
    if state is not None:
        dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")}, strict=True)
    return dec.eval().to(DEV)


def _guarded(n):
    """(buffer, float view of its middle n words): sentinel everywhere."""
    buf = torch.full((n + 2 * G,), SENTINEL, device=DEV, dtype=torch.int32)
    return buf, buf[G:G + n].view(torch.float32)


def _guards_intact(buf, n):
    lo, hi = buf[:G].cpu().numpy(), buf[G + n:].cpu().numpy()
    assert (lo == SENTINEL).all(), f"{int((lo != SENTINEL).sum())} words written below the buffer"
    assert (hi == SENTINEL).all(), f"{int((hi != SENTINEL).sum())} words written above the buffer"


# ---- the step producer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 256, 512])            # one, four and the maximum eight float4 per lane
@pytest.mark.parametrize("classes", [1, 30, 300])
def test_embed_producer_vs_float64(d, classes):
    """LayerNorm(E[tok] sqrt(d) + kwp[r / row_div]) + pe[t] and layer 0's QKV projection of it: 3 rows (a lone partial
    16-row block) and 17 (a full block and a partial one) at t = 0 and 5, 18 rows over 6 clips (row_div 3); a pad token among
    the inputs, one all-zero keyword row (kwp = the bias alone); guard words around xout and qkv."""
    from audiocaption_amd import _lib
    torch.manual_seed(d + classes)
    dec = _decoder("d128", emb_dim=d, nhead=max(1, d // 64), nlayers=1, dim_feedforward=64, attn_emb_dim=32, fc_emb_dim=32,
                   vocab_size=50, keyword_classes_num=classes)
    with torch.no_grad():
        dec.word_keyword_norm.weight.uniform_(0.5, 1.5)
        dec.word_keyword_norm.bias.uniform_(-0.5, 0.5)
        dec.keyword_proj.weight.normal_(0.0, 1.0)
        dec.word_embedding.weight.mul_(5.0)           # xavier rows are ~0.2 / sqrt(d): bring E sqrt(d) to the keyword term's order
    lib = _lib.load()
    w = dec.weights()
    W, b, ln_w, ln_b = dec._keyword_weights()
    sd = {k: v.detach().double().cpu() for k, v in dec.state_dict().items()}
    L0 = "model.layers.0.self_attn."
    worst = {"kwp": 0.0, "xout": 0.0, "qkv": 0.0}
    for rows, row_div in ((3, 1), (17, 1), (18, 3)):
        clips = rows // row_div
        kw = R.keywords(clips, classes, rows, zero_row=clips - 1)
        kwp = torch.empty(clips, d, device=DEV)
        dec._keyword_proj_launch(kw.to(DEV), kwp)
        kwp64 = kw.double() @ sd["keyword_proj.weight"].T + sd["keyword_proj.bias"]
        worst["kwp"] = max(worst["kwp"], float((kwp.double().cpu() - kwp64).abs().max()))
        assert torch.equal(kwp[clips - 1].cpu(), dec.keyword_proj.bias.detach().cpu())
        g = torch.Generator().manual_seed(rows)
        tok = torch.randint(3, 50, (rows, 7), generator=g, dtype=torch.int32)
        tok[1, :] = R.PAD
        tok_d = tok.to(DEV)
        for t in (0, 5):
            n = rows * d + rows * 3 * d
            buf, mid = _guarded(n)
            xout, qkv = mid[:rows * d].view(rows, d), mid[rows * d:].view(rows, 3 * d)
            key = _lib.AcTrmKeyword(kwp.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), row_div)
            rc = lib.ac_trm_kw_embed_qkv(ctypes.byref(w), ctypes.byref(key), rows, row_div, t, tok_d.data_ptr(), 7,
                                         xout.data_ptr(), qkv.data_ptr(), None)
            assert rc == 0
            torch.cuda.synchronize()
            _guards_intact(buf, n)
            x = sd["word_embedding.weight"][tok[:, t].long()] * math.sqrt(d) + kwp64.repeat_interleave(row_div, 0)
            x = torch.nn.functional.layer_norm(x, (d,), sd["word_keyword_norm.weight"], sd["word_keyword_norm.bias"])
            x = x + sd["pos_encoder.pe"][t, 0]
            q = x @ sd[L0 + "in_proj_weight"].T + sd[L0 + "in_proj_bias"]
            worst["xout"] = max(worst["xout"], float((xout.double().cpu() - x).abs().max()))
            worst["qkv"] = max(worst["qkv"], float((qkv.double().cpu() - q).abs().max()))
            assert float(x.abs().max()) > 1.0 and float(q.abs().max()) > 0.5      # the bar is not met by small numbers
    for k, v in worst.items():
        print(f"[producer d {d} classes {classes} {k}] {v:.3e}")
    assert worst["kwp"] < LOGIT_BAR and worst["xout"] < LOGIT_BAR and worst["qkv"] < LOGIT_BAR
    # operands the launches would read out of bounds or misaligned are refused before any of them
    key = _lib.AcTrmKeyword(kwp.data_ptr() + 4, ln_w.data_ptr(), ln_b.data_ptr(), 3)
    assert lib.ac_trm_kw_embed_qkv(ctypes.byref(w), ctypes.byref(key), 18, 3, 0, tok_d.data_ptr(), 7, xout.data_ptr(),
                                   qkv.data_ptr(), None) == _lib.AC_ERR_ARG
    key = _lib.AcTrmKeyword(kwp.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), 3)
    assert lib.ac_trm_kw_embed_qkv(ctypes.byref(w), ctypes.byref(key), 17, 3, 0, tok_d.data_ptr(), 7, xout.data_ptr(),
                                   qkv.data_ptr(), None) == _lib.AC_ERR_ARG          # rows % row_div
    assert lib.ac_trm_kw_embed_qkv(ctypes.byref(w), ctypes.byref(key), 18, 3, 7, tok_d.data_ptr(), 7, xout.data_ptr(),
                                   qkv.data_ptr(), None) == _lib.AC_ERR_ARG          # t beyond the token rows


# ---- the searches against the reference ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(R.SHAPES))
def searcher(request, g27):
    import audiocaption_amd as A
    shape = request.param
    dec = _decoder(shape, R.decoder_state(shape, *R.recipe(g27, shape)))
    return shape, A.KeywordCondTransformerModel(torch.nn.Identity(), dec).eval()


def _request(shape, which, **kw):
    attn, lens, key = R.infer_inputs(shape, which)
    d = {"mode": "inference", "attn_emb": attn.to(DEV), "attn_emb_len": lens, "fc_emb": torch.zeros(R.B, 4, device=DEV),
         "keyword": key, "max_length": R.MAX_LENGTH}
    d.update(kw)
    return d


def _greedy_vs_g27(g27, shape, which, out):
    want = g27[f"{shape}_k{which}_greedy_seq"]
    assert np.array_equal(out["seq"].numpy(), want), (shape, which)
    live = R.live_mask(want)
    got = out["logit"].cpu().gather(2, torch.from_numpy(g27[f"{shape}_k{which}_greedy_top_idx"]).long())
    d = float((got.double() - torch.from_numpy(g27[f"{shape}_k{which}_greedy_top_val"]).double())[live].abs().max())
    print(f"[{shape} k{which} greedy top-8 logits] {d:.3e}")
    assert d < GATE


def test_greedy_vs_g27_eager_and_replayed(searcher, g27, monkeypatch):
    shape, model = searcher
    calls = [model(_request(shape, 0)) for _ in range(3)]       # eager, captured + replayed, replayed
    st = next(iter(model.decoder._greedy_state.values()))
    assert st["graph"] is not None and st["uses"] == 3
    for out in calls:
        _greedy_vs_g27(g27, shape, 0, out)
    for out in calls[1:]:
        for k in ("seq", "logit", "embed", "sampled_logprob"):
            assert torch.equal(out[k], calls[0][k]), k
    # two keyword batches through ONE captured graph give each its own fixture; the keyword may live anywhere, in any float
    other = model(_request(shape, 1))
    _greedy_vs_g27(g27, shape, 1, other)
    back = model(_request(shape, 0, keyword=R.infer_inputs(shape, 0)[2].double().to(DEV)))
    assert len(model.decoder._greedy_state) == 1 and st["uses"] == 5
    assert torch.equal(back["logit"], calls[0]["logit"]) and torch.equal(back["seq"], calls[0]["seq"])
    zero = model(_request(shape, 0, keyword=torch.zeros_like(R.infer_inputs(shape, 0)[2])))
    moved = float((zero["logit"][:, 0] - calls[0]["logit"][:, 0]).abs().max())
    print(f"[{shape} step-0 logits moved by zeroing the keywords] {moved:.3e}")
    assert moved > 1e-3
    # the one-launch search is not built for it
    import audiocaption_amd as A
    monkeypatch.setenv("AUDIOCAPTION_GREEDY", "cluster")
    with pytest.raises(A._lib.HipLibraryError):
        model(_request(shape, 0))


@pytest.mark.parametrize("beam", R.BEAMS)
def test_beam_vs_g27(searcher, g27, beam):
    shape, model = searcher
    for rep in range(3):                                        # eager, captured, replayed
        for which in (0, 1):
            out = model(_request(shape, which, sample_method="beam", beam_size=beam))
            assert np.array_equal(out["seq"].numpy(), g27[f"{shape}_k{which}_beam{beam}_seq"]), (shape, which, beam, rep)
    for which in (0, 1):
        out = model(_request(shape, which, sample_method="beam", beam_size=beam, n_best=True, n_best_size=beam))
        assert np.array_equal(out["seq"].numpy(), g27[f"{shape}_k{which}_beam{beam}_nbest_seq"]), (shape, which, beam)
    assert any(st["graphs"] for st in model._beam_state.values())


def test_sampling_is_reproducible_and_top1_is_greedy(searcher, g27):
    shape, model = searcher
    for method in ("sample", "top5", "top0.8", "gumbel"):
        a = model(_request(shape, 0, sample_method=method, seed=11))
        b = model(_request(shape, 0, sample_method=method, seed=11))     # the replayed graph
        c = model(_request(shape, 0, sample_method=method, seed=12))
        assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["logit"], b["logit"]), method
        assert torch.equal(a["sampled_logprob"], b["sampled_logprob"]), method
        assert a["seq"].shape == c["seq"].shape == (R.B, R.MAX_LENGTH)
    top1 = model(_request(shape, 0, sample_method="top1", seed=3))
    assert np.array_equal(top1["seq"].numpy(), g27[f"{shape}_k0_greedy_seq"])
    with pytest.raises(KeyError, match="keyword"):
        d = _request(shape, 0, sample_method="sample")
        d.pop("keyword")
        model(d)


def test_eval_forward_vs_g27_inside_a_guarded_workspace(searcher, g27):
    from audiocaption_amd import _lib
    shape, model = searcher
    dec = model.decoder
    inp = R.forward_inputs(shape)
    out = dec({k: (v.to(DEV) if k in ("attn_emb", "word", "cap_padding_mask") else v) for k, v in inp.items()})
    for key in ("logit", "embed"):
        d = float((out[key].double().cpu() - torch.from_numpy(g27[f"{shape}_forward_{key}"]).double()).abs().max())
        print(f"[{shape} eval forward {key}] {d:.3e}")
        assert d < GATE
    # the same call through the entry point with the workspace between guard words
    lib = _lib.load()
    w = dec.weights()
    N, T = inp["word"].shape
    n = lib.ac_trm_workspace_floats(ctypes.byref(w), N, T)
    buf, ws = _guarded(n)
    st = dec._extra_buffers(torch.device(DEV), N)
    dec._keyword_proj_launch(inp["keyword"].to(DEV), st["kwp"])
    memkv = dec.memory(inp["attn_emb"].to(DEV))
    tokens = inp["word"].to(DEV).to(torch.int32).contiguous()
    mask = inp["cap_padding_mask"].to(DEV).to(torch.uint8).contiguous()
    lens = inp["attn_emb_len"].to(DEV).to(torch.int32)
    embed, logit = torch.empty_like(out["embed"]), torch.empty_like(out["logit"])
    assert lib.ac_trm_kw_forward_tokens(ctypes.byref(w), ctypes.byref(st["kw"]), memkv.data_ptr(), lens.data_ptr(), N,
                                        R.TM, tokens.data_ptr(), mask.data_ptr(), T, embed.data_ptr(), logit.data_ptr(),
                                        ws.data_ptr(), None) == 0
    torch.cuda.synchronize()
    _guards_intact(buf, n)
    assert torch.equal(logit, out["logit"]) and torch.equal(embed, out["embed"])


# ---- training ----------------------------------------------------------------------------------------------------------------
def _train_model(state, p_dec=0.0):
    import audiocaption_amd as A
    from audiocaption_amd import build
    build.build()
    s = R.SHAPES["d256"]
    cfg = A.cnn14rnn_keyword_trm_config(s["vocab_size"], s["keyword_classes_num"])
    cfg["encoder"]["rnn"]["args"]["dropout"] = 0.0
    cfg["decoder"]["args"].update(dim_feedforward=s["dim_feedforward"], nhead=s["nhead"], dropout=p_dec)
    model = A.init_model_from_config(cfg, print_fn=lambda s_: None)
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.startswith("encoder.cnn.") for k in missing)      # the Cnn14 is preset: never run
    model = model.to(DEV).train()
    model.encoder.cnn.eval()
    return model


def _train_batch(attn, lens, kw, cap, cap_len, ss_ratio, **extra):
    Bn, Tq = attn.shape[:2]
    d = {"mode": "train", "wav": torch.zeros(Bn, 320 * 32 * Tq, device=DEV), "wav_len": [320 * (32 * int(n) - 1) for n in lens],
         "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len, "ss_ratio": ss_ratio, "_cnn_attn": attn.to(DEV),
         "keyword": kw}
    d.update(extra)
    return d


@pytest.mark.parametrize("tag", ["tf", "ss"])
def test_training_step_vs_reference_g27(g27, tag):
    """model(input_dict) + LabelSmoothingLoss + loss.backward() + clip at p = 0 against one step the REFERENCE ran: top-8
    logits, greedy tokens, loss, every gradient (the four keyword tensors and the embedding among them), the total norm."""
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import clip_grad_norm_
    pre = f"d256_train_{tag}_"
    model = _train_model(R.model_state(*R.recipe(g27, "d256")))
    attn, lens, kw, cap, cap_len = R.train_inputs()
    random.seed(int(g27["coin_seed"]))           # the reference drew its scheduled-sampling coins from this stream
    out = model(_train_batch(attn, lens, kw, cap, cap_len, 1 if tag == "tf" else 0.5))
    logit = out["logit"]
    top_val, top_idx = logit.detach().topk(8, dim=-1)
    assert rel(f"train {tag} logit top-8", top_val, g27[pre + "logit_top_val"]) < 2e-5
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g27[pre + "logit_top_idx"][..., 0])
    if tag == "ss":
        assert np.array_equal(out["seq"].cpu().numpy(), g27[pre + "seq"])
    loss = LabelSmoothingLoss(smoothing=0.1)({"logit": logit, "tgt": cap[:, 1:].to(DEV), "tgt_len": torch.as_tensor(cap_len - 1)})
    want = float(g27[pre + "loss"])
    print(f"[train {tag} loss] {abs(float(loss.detach()) - want) / want:.3e}")
    assert abs(float(loss.detach()) - want) < 2e-5 * want
    loss.backward()
    named = dict(model.named_parameters())
    keys = [k[len("d256_sample_idx/"):] for k in g27.files if k.startswith("d256_sample_idx/")]
    assert set(keys) == {k for k, p in named.items() if p.requires_grad}
    bad, worst = [], 0.0
    for key in keys:
        grad = named[key].grad
        gn = float(g27[f"{pre}gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g27[f"d256_sample_idx/{key}"]).to(DEV)].cpu().numpy()
        d_s = float(np.abs(sample - g27[f"{pre}gsample/{key}"]).max()) / (float(grad.abs().max()) + 1e-12)
        worst = max(worst, d_norm, d_s)
        if "keyword" in key or key.endswith("word_embedding.weight"):
            print(f"[train {tag} grad {key}] norm {d_norm:.3e} samples {d_s:.3e}")
        if not (d_norm < 1e-4 and d_s < 1e-4):
            bad.append((key, d_norm, d_s))
    print(f"[train {tag} worst gradient figure] {worst:.3e}")
    assert not bad, f"gradients differ from the reference's: {bad}"
    clip = clip_grad_norm_([p for p in model.parameters() if p.requires_grad], 1.0)
    tn = float(g27[pre + "total_norm"])
    print(f"[train {tag} total norm] {abs(float(clip.total_norm) - tn) / tn:.3e}")
    assert abs(float(clip.total_norm) - tn) < 1e-4 * tn


def test_training_step_with_dropout_vs_restatement(g27):
    """Dropout 0.1 at every decoder site, scheduled sampling with the fixture's coins: the engine's forward and backward against
    the float64 restatement drawing the same counter-hash masks; the same seed gives the same bits, another seed does not."""
    from audiocaption_amd.loss import _launch
    from audiocaption_amd.train import TrainEngine
    state = R.model_state(*R.recipe(g27, "d256"))
    model = _train_model(state, p_dec=0.1)
    attn, lens, kw, cap, cap_len = R.train_inputs()
    use_cap = g27["d256_train_ss_use_cap"].tolist()
    seed = 77
    batch = _train_batch(attn, lens, kw, cap, cap_len, 0.5, _use_cap=use_cap, dropout_seed=seed)
    eng = TrainEngine(model)
    out = eng.forward(batch)
    sv = eng._saved
    ws_, R_ = sv["ws"], sv["lay"]["R"]
    N, Tq = sv["N"], sv["Tq"]
    gates = {"mem": ws_.tensor("mem_a")[:N * Tq * 256].view(N * Tq, 256).cpu(),
             "ffn": [ws_.tensor(f"hdn{l}")[:R_ * sv["F"]].view(R_, sv["F"]).cpu() for l in range(2)]}
    o = R.train_step_grads(state, attn, lens, kw, cap, cap_len, use_cap, base_seed=seed, p_dec=0.1, relu_gates=gates,
                           kink=1e-4)
    last = max(t for t in range(len(use_cap)) if not use_cap[t] and t > 0)
    top2 = o["logit"][:, :last].topk(2, -1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    assert gap >= 1e-3, f"near-tie {gap:.1e} on a fed-back step: choose another seed"
    assert torch.equal(out["seq"].cpu(), o["seq"])
    assert rel("dropout logit", out["logit"], o["logit"]) < 5e-5
    tgt_len = torch.as_tensor(cap_len - 1)
    count = float(tgt_len.sum())
    dlogit = torch.empty_like(out["logit"])
    loss, _ = _launch(out["logit"], cap[:, 1:].to(DEV), tgt_len.to(device=DEV, dtype=torch.int32), 0.1, 1.0 / count, dlogit,
                      1.0 / count, None)
    d_loss = abs(float(loss) - float(o["loss"])) / float(o["loss"])
    print(f"[dropout loss] {d_loss:.3e}")
    assert d_loss < 2e-5
    eng.backward(dlogit)
    bad = []
    for key, view in zip(eng.flat.names, eng.flat.grad_views):
        d = rel(f"dropout grad {key}", view, o["grads"][key])
        if not d < 2e-4:
            bad.append((key, d))
    assert not bad, bad
    assert eng.flat.names[-4:] == ["decoder.keyword_proj.weight", "decoder.keyword_proj.bias",
                                   "decoder.word_keyword_norm.weight", "decoder.word_keyword_norm.bias"]
    again = eng.forward(batch)["logit"]
    other = eng.forward(dict(batch, dropout_seed=seed + 1))["logit"]
    assert torch.equal(again, out["logit"]) and not torch.equal(other, out["logit"])
    # a keyword of another width is refused before anything is launched, and so are the fused step and the rollout
    with pytest.raises(ValueError, match="keyword"):
        eng.forward(dict(batch, keyword=kw[:, :-1]))
    with pytest.raises(KeyError, match="keyword"):
        eng.forward({k: v for k, v in batch.items() if k != "keyword"})
    with pytest.raises(NotImplementedError, match="keyword"):
        eng.step(batch, None)


def test_training_step_over_the_transformer_encoder_vs_restatement():
    """The same decoder half behind a Cnn14TransformerEncoder (memory = cls row + frames, 256 wide): forward and backward at
    p = 0 against the float64 restatement, scheduled sampling with two free-running passes."""
    import audiocaption_amd as A
    from audiocaption_amd.loss import _launch
    from audiocaption_amd.train import TrainEngine
    s = R.SHAPES["d256"]
    state = R.trm_model_state(41)
    cfg = A.config.cnn14trm_trm_config(s["vocab_size"])
    cfg["encoder"]["transformer"]["args"]["dropout"] = 0.0
    cfg["decoder"] = {"type": "captioning.models.transformer_decoder.KeywordProbTransformerDecoder",
                      "args": dict(s, fc_emb_dim=256, attn_emb_dim=256, dropout=0.0)}
    cfg["type"] = "captioning.models.transformer_model.KeywordCondTransformerModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s_: None)
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.startswith("encoder.cnn.") for k in missing)
    model = model.to(DEV).train()
    model.encoder.cnn.eval()
    attn, lens, kw, cap, cap_len = R.train_inputs()
    use_cap = [1, 0, 1, 1, 0]
    eng = TrainEngine(model)
    out = eng.forward(_train_batch(attn, lens, kw, cap, cap_len, 0.5, _use_cap=use_cap, dropout_seed=3))
    o = R.train_step_grads(state, attn, lens, kw, cap, cap_len, use_cap)
    top2 = o["logit"][:, :4].topk(2, -1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) >= 1e-3, "near-tie on a fed-back step: choose another seed"
    assert torch.equal(out["seq"].cpu(), o["seq"])
    assert rel("trm-encoder logit", out["logit"], o["logit"]) < 5e-5
    tgt_len = torch.as_tensor(cap_len - 1)
    count = float(tgt_len.sum())
    dlogit = torch.empty_like(out["logit"])
    loss, _ = _launch(out["logit"], cap[:, 1:].to(DEV), tgt_len.to(device=DEV, dtype=torch.int32), 0.1, 1.0 / count, dlogit,
                      1.0 / count, None)
    assert abs(float(loss) - float(o["loss"])) < 2e-5 * float(o["loss"])
    eng.backward(dlogit)
    bad = [(k, d) for k, d in ((k, rel(f"trm-encoder grad {k}", v, o["grads"][k]))
                               for k, v in zip(eng.flat.names, eng.flat.grad_views)) if not d < 2e-4]
    assert not bad, bad
