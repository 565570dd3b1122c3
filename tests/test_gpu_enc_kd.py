"""GPU tests of encoder-level knowledge distillation: the loss head ``ac_enc_kd_loss`` (csrc/enc_kd.hip) against the float64
restatement of tests/_enc_kd_ref.py, its edge cases and refusals, ``enc_kd.enc_kd_loss`` under autograd, and the path INTO the
encoders: ``fc_emb`` of the training engines' forward, its gradient through the bi-GRU / the Transformer encoder / the
attention-GRU engine against torch autograd over the existing restatements, and the wrappers in ``mode="train"``.

Bounds (the ones ``ac_label_smoothing_loss`` is held to): the loss within 2e-5 relative, every gradient within 1e-5 of its
tensor's maximum; the encoder gradients within 1e-4 of each tensor's maximum (test_training_step_vs_reference_gradients).
Measured figures: tests/golden/REPORT_enc_kd.txt."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _enc_kd_ref as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOSS_BAR, GRAD_BAR, ENC_BAR = 2e-5, 1e-5, 1e-4
SHAPES = [(1, 16), (2, 4), (5, 16), (33, 50), (64, 1024), (65, 1000), (256, 1024)]
SCALE0 = float(np.log(1 / 0.07))


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


def _draw(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=g), torch.randn(B, D, generator=g) + 0.25


def _head(s, t, scale, bits, **kw):
    from audiocaption_amd.enc_kd import head
    sc = torch.tensor([scale], device=DEV, dtype=torch.float32) if bits & E.CONTRA else None
    loss, ds, dt, dscale, _ = head(s, t, sc, bits, **kw)
    return loss, ds, dt, dscale


def _check(tag, got, want, bits, rows=None):
    """got = (loss[3], ds, dt, dscale) of the kernel, want = _enc_kd_ref.head's dict; returns the figures."""
    loss, ds, dt, dscale = got
    loss = loss.double().cpu()
    fig = {}
    for i, k in enumerate(("loss", "contra", "mse")):
        w = float(want[k])
        fig[k] = abs(float(loss[i]) - w) / abs(w) if w != 0 else abs(float(loss[i]))
    for k, g_, w in (("ds", ds, want["ds"]), ("dt", dt, want["dt"])):
        g_, w = g_.double().cpu(), w
        if rows is not None:
            g_, w = g_[rows], w[rows]
        top = float(w.abs().max())
        fig[k] = float((g_ - w).abs().max()) / top if top > 0 else float(g_.abs().max())
    if bits & E.CONTRA:
        w = float(want["dscale"])
        # d logit_scale is a sum over B*B terms of either sign: judged against the largest |gradient| a unit logit carries
        fig["dscale"] = abs(float(dscale[0]) - w) / max(abs(w), 1e-3)
    else:
        assert float(dscale[0]) == 0.0
    print(f"[{tag}] " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert torch.isfinite(loss).all() and torch.isfinite(ds).all() and torch.isfinite(dt).all()
    assert fig["loss"] <= LOSS_BAR and fig["contra"] <= LOSS_BAR and fig["mse"] <= LOSS_BAR, (tag, fig)
    assert fig["ds"] <= GRAD_BAR and fig["dt"] <= GRAD_BAR and fig.get("dscale", 0.0) <= GRAD_BAR, (tag, fig)
    return fig


@pytest.mark.parametrize("B,D", SHAPES)
def test_head_vs_float64(lib, B, D):
    """One row, ragged wave tails, the published shared width, a batch beyond one workgroup's rows - every kind."""
    s, t = _draw(B, D, 100 * B + D)
    sd, td = s.to(DEV), t.to(DEV)
    for kind, bits in E.KINDS.items():
        got = _head(sd, td, SCALE0, bits)
        want = E.head(s, t, float(np.float32(SCALE0)), bits)
        _check(f"{B}x{D} {kind}", got, want, bits)
        if B == 1 and kind == "contra":
            assert float(got[0][0]) == 0.0 and not got[1].any() and not got[2].any() and float(got[3][0]) == 0.0
        # the float32 torch expression at the same shape, for the record (REPORT_enc_kd.txt)
        a, b = sd.clone().requires_grad_(True), td.clone().requires_grad_(True)
        sc = torch.tensor(SCALE0, device=DEV, requires_grad=True)
        lt = E.torch_loss(a, b, sc, bits)
        lt.backward()
        w = float(want["loss"])
        print(f"    torch f32: loss {abs(float(lt.detach()) - w) / abs(w) if w else abs(float(lt.detach())):.2e} "
              f"ds {float((a.grad.double().cpu() - want['ds']).abs().max()) / max(float(want['ds'].abs().max()), 1e-300):.2e}")


def test_head_edge_rows_and_large_scale(lib):
    B, D = 6, 40
    s, t = _draw(B, D, 7)
    # a zero row goes through the 1e-12 clamp (gradient dy / 1e-12); judged apart from the other rows, whose gradients are
    # twelve orders of magnitude smaller
    z = s.clone()
    z[2] = 0.0
    others = [0, 1, 3, 4, 5]
    for kind, bits in E.KINDS.items():
        got = _head(z.to(DEV), t.to(DEV), SCALE0, bits)
        want = E.head(z, t, float(np.float32(SCALE0)), bits)
        _check(f"zero row {kind} (others)", got, want, bits, rows=others)
        if bits != E.MSE:
            g2, w2 = got[1][2].double().cpu(), want["ds"][2]
            assert float(w2.abs().max()) > 1e6 and float((g2 - w2).abs().max()) <= GRAD_BAR * float(w2.abs().max())
    # two identical rows (student and teacher): the two clips share their soft-max mass
    tw_s, tw_t = s.clone(), t.clone()
    tw_s[4], tw_t[4] = tw_s[1], tw_t[1]
    for kind, bits in E.KINDS.items():
        got = _head(tw_s.to(DEV), tw_t.to(DEV), SCALE0, bits)
        _check(f"twin rows {kind}", got, E.head(tw_s, tw_t, float(np.float32(SCALE0)), bits), bits)
        assert torch.equal(got[1][1], got[1][4]) and torch.equal(got[2][1], got[2][4])
    # a learnt logit_scale of 100: the soft-maxes are max-subtracted
    for B2, D2 in ((6, 40), (65, 1000)):
        s2, t2 = _draw(B2, D2, 11)
        for kind in ("contra", "contra_mse_l2"):
            got = _head(s2.to(DEV), t2.to(DEV), 100.0, E.KINDS[kind])
            _check(f"scale 100 {B2}x{D2} {kind}", got, E.head(s2, t2, 100.0, E.KINDS[kind]), E.KINDS[kind])


def test_head_strided_offset_views_repeat_and_gscale(lib):
    B, D = 33, 50
    s, t = _draw(B, D, 3)
    big_s = torch.full((B, D + 3), float("nan"), device=DEV)
    big_t = torch.full((B + 1, D + 7), float("nan"), device=DEV)
    vs, vt = big_s[:, 1:1 + D], big_t[1:, 5:5 + D]      # row pitch > D, base 4 bytes (s) / not 16-byte aligned (t)
    vs.copy_(s)
    vt.copy_(t)
    assert vs.data_ptr() % 16 == 4 and vs.stride(0) == D + 3 and vt.stride(0) == D + 7
    bits = E.KINDS["contra_mse_l2"]
    dense = _head(s.to(DEV), t.to(DEV), SCALE0, bits)
    view = _head(vs, vt, SCALE0, bits)
    again = _head(vs, vt, SCALE0, bits)
    for a, b, c in zip(dense, view, again):
        assert torch.equal(a, b) and torch.equal(b, c)      # same bits: no atomics, no dependence on alignment or pitch
    _check("views", view, E.head(s, t, float(np.float32(SCALE0)), bits), bits)
    # gscale and gscale_dev scale the three gradients, not the loss
    up = torch.tensor([3.0], device=DEV)
    scaled = _head(vs, vt, SCALE0, bits, gscale=0.5, gscale_dev=up)
    assert torch.equal(scaled[0], view[0])
    for a, b in zip(scaled[1:], view[1:]):
        assert float((a - 1.5 * b).abs().max()) <= 1e-6 * float(b.abs().max())
    # forward only
    from audiocaption_amd.enc_kd import head
    only = head(vs, vt, torch.tensor([SCALE0], device=DEV), bits, grads=False)
    assert torch.equal(only[0], view[0]) and only[1] is None


def test_head_refuses_out_of_contract_arguments(lib):
    from audiocaption_amd._lib import AC_ERR_ARG, ptr, stream
    B, D = 4, 8
    s, t = (x.to(DEV) for x in _draw(B, D, 1))
    sc = torch.tensor([SCALE0], device=DEV)
    loss = torch.full((3,), 7.0, device=DEV)
    ws = torch.empty(lib.ac_enc_kd_workspace_floats(512, 16), device=DEV)
    ds, dt, dsc = torch.empty(B, D, device=DEV), torch.empty(B, D, device=DEV), torch.empty(1, device=DEV)

    def call(**kw):
        a = dict(s=ptr(s), ld_s=D, t=ptr(t), ld_t=D, B=B, D=D, kind=3, scale=ptr(sc), loss=ptr(loss), ds=ptr(ds), dt=ptr(dt),
                 dsc=ptr(dsc), gscale=1.0, gdev=None, ws=ptr(ws))
        a.update(kw)
        return lib.ac_enc_kd_loss(a["s"], a["ld_s"], a["t"], a["ld_t"], a["B"], a["D"], a["kind"], a["scale"], a["loss"],
                                  a["ds"], a["dt"], a["dsc"], a["gscale"], a["gdev"], a["ws"], stream())

    assert call() == 0
    bad = [dict(B=0), dict(B=513), dict(B=-1), dict(D=0), dict(D=4097), dict(ld_s=D - 1), dict(ld_t=D - 1), dict(kind=0),
           dict(kind=4), dict(kind=8), dict(kind=11), dict(kind=-1), dict(s=None), dict(t=None), dict(loss=None), dict(ws=None),
           dict(scale=None), dict(scale=None, kind=7), dict(gscale=float("inf")), dict(gscale=float("nan"))]
    torch.cuda.synchronize()
    loss.fill_(7.0)
    for kw in bad:
        assert call(**kw) == AC_ERR_ARG, kw
    torch.cuda.synchronize()
    assert loss.tolist() == [7.0, 7.0, 7.0]          # refused BEFORE anything was launched
    assert call(scale=None, kind=2) == 0 and call(scale=None, kind=6) == 0      # the MSE kinds need no logit_scale
    assert call(ds=None, dt=None, dsc=None) == 0
    for b, d in ((0, 8), (513, 8), (4, 0), (4, 4097)):
        assert lib.ac_enc_kd_workspace_floats(b, d) == -1
    assert lib.ac_enc_kd_workspace_floats(512, 4096) == 2 * 512 * 4096 + 512 * 512 + 11 * 512
    # the largest accepted batch and width run (one launch set each; values against float64)
    for B2, D2 in ((512, 16), (3, 4096)):
        s2, t2 = _draw(B2, D2, 5)
        _check(f"bound {B2}x{D2}", _head(s2.to(DEV), t2.to(DEV), SCALE0, 3), E.head(s2, t2, float(np.float32(SCALE0)), 3), 3)


# ---- enc_kd_loss: the projections and the head as one autograd node -------------------------------------------------
GRADS = ["fc_emb", "stdnt_proj.weight", "stdnt_proj.bias", "tchr_proj.weight", "tchr_proj.bias", "logit_scale"]


def _heads(fc, tchr_dim, shared, seed):
    torch.manual_seed(seed)
    sp, tp = nn.Linear(fc, shared), nn.Linear(tchr_dim, shared)
    scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
    return sp.to(DEV), tp.to(DEV), scale.to(DEV).detach().requires_grad_(True)


def _ref_full(fc, tchr, sp, tp, scale, bits):
    return E.full(fc.cpu(), tchr.cpu(), sp.weight.cpu(), sp.bias.cpu(), tp.weight.cpu(), tp.bias.cpu(), float(scale), bits)


def test_enc_kd_loss_parity_with_the_reference_fixture(lib, golden_dir):
    from audiocaption_amd.enc_kd import enc_kd_loss
    g24 = dict(np.load(os.path.join(golden_dir, "g24_enc_kd.npz")))
    sp, tp, scale = _heads(24, 12, 16, 0)
    with torch.no_grad():
        for m, n in ((sp, "stdnt_proj"), (tp, "tchr_proj")):
            m.weight.copy_(torch.from_numpy(g24[n + ".weight"]))
            m.bias.copy_(torch.from_numpy(g24[n + ".bias"]))
        scale.fill_(float(g24["logit_scale"]))
    for b in ("b5", "b1"):
        for kind in E.KINDS:
            for p in (sp.weight, sp.bias, tp.weight, tp.bias, scale):
                p.grad = None
            fc = torch.from_numpy(g24[f"{b}/fc_emb"]).to(DEV).requires_grad_(True)
            loss = enc_kd_loss(fc, torch.from_numpy(g24[f"{b}/tchr_emb"]).to(DEV), sp, tp, scale if "contra" in kind else None,
                               kind.replace("_l2", ""), kind.endswith("_l2"))
            want = float(g24[f"{b}/{kind}/loss"])
            d = abs(float(loss.detach()) - want) / abs(want) if want else abs(float(loss.detach()))
            assert d <= LOSS_BAR, (b, kind, d)
            loss.backward()
            got = dict(zip(GRADS, (fc.grad, sp.weight.grad, sp.bias.grad, tp.weight.grad, tp.bias.grad, scale.grad)))
            for k in GRADS:
                key = f"{b}/{kind}/d/{k}"
                if key not in g24:
                    assert k == "logit_scale" and got[k] is None
                    continue
                ref = torch.from_numpy(g24[key])
                top = float(ref.abs().max())
                err = float((got[k].double().cpu() - ref).abs().max())
                print(f"[g24 {b} {kind} {k}] {err / top if top else err:.2e}")
                assert err <= GRAD_BAR * top, key


@pytest.mark.parametrize("B,fc,td,shared", [(5, 24, 12, 16), (33, 512, 768, 1024)])
def test_enc_kd_loss_autograd_vs_float64(lib, B, fc, td, shared):
    """Gradients for fc_emb, both projections and logit_scale, with an upstream gradient other than 1."""
    from audiocaption_amd.enc_kd import enc_kd_loss
    g = torch.Generator().manual_seed(B)
    x, tchr = torch.randn(B, fc, generator=g).to(DEV), torch.randn(B, td, generator=g).to(DEV)
    for kind in E.KINDS:
        sp, tp, scale = _heads(fc, td, shared, 3)
        xr = x.clone().requires_grad_(True)
        tr = tchr.clone().requires_grad_(True)
        loss = enc_kd_loss(xr, tr, sp, tp, scale if "contra" in kind else None, kind.replace("_l2", ""), kind.endswith("_l2"))
        (0.5 * loss).backward()
        want = _ref_full(x, tchr, sp, tp, scale.detach(), E.KINDS[kind])
        assert abs(float(loss.detach()) - float(want["loss"])) <= LOSS_BAR * abs(float(want["loss"]))
        assert tr.grad is None                                     # the teacher's embedding gets no gradient
        got = dict(zip(GRADS, (xr.grad, sp.weight.grad, sp.bias.grad, tp.weight.grad, tp.bias.grad, scale.grad)))
        for k in GRADS:
            if k == "logit_scale" and "contra" not in kind:
                assert got[k] is None
                continue
            ref = 0.5 * want[k]
            err = float((got[k].double().cpu() - ref).abs().max()) / float(ref.abs().max())
            print(f"[{B} {kind} {k}] {err:.2e}")
            assert err <= GRAD_BAR, (kind, k, err)


# ---- the engines: fc_emb out of the training forward, its gradient into the encoder ------------------------------------
N, TQ, TC, TD, SHARED = 3, 8, 6, 12, 32
LENS = [8, 5, 3]
SEED = 77


def _cap():
    g = torch.Generator().manual_seed(6)
    cap = torch.randint(4, 4981, (N, TC), generator=g)
    cap_len = np.array([6, 4, 5])
    cap[:, 0] = 1
    for i, n in enumerate(cap_len):
        cap[i, n - 1] = 2
        cap[i, n:] = 0
    return cap, cap_len


def _cnn_attn():
    g = torch.Generator().manual_seed(8)
    return torch.randn(N, TQ, 2048, generator=g).abs() * 0.5


def _batch(**extra):
    cap, cap_len = _cap()
    b = {"mode": "train", "wav": torch.zeros(N, 320 * 32 * TQ, device=DEV), "wav_len": [320 * (32 * n - 1) for n in LENS],
         "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len, "ss_ratio": 1, "dropout_seed": SEED,
         "_cnn_attn": _cnn_attn().to(DEV)}
    b.update(extra)
    return b


def _set_p(model, p_dec, p_enc):
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = p_dec
        if isinstance(m, nn.MultiheadAttention):
            m.dropout = p_dec
    enc = model.encoder
    if hasattr(enc, "rnn"):
        enc.rnn.network.dropout = p_enc
    else:
        for m in enc.trm.modules():
            if isinstance(m, nn.Dropout):
                m.p = p_enc
            if isinstance(m, nn.MultiheadAttention):
                m.dropout = p_enc
    if hasattr(model.decoder, "in_dropout"):
        model.decoder.in_dropout.p = p_dec
    enc.cnn.eval()


def _build(kind):
    """(model, its state dict on the CPU) - "rnn": TransformerModel over CrnnEncoder, "trm": over Cnn14TransformerEncoder,
    "attn": TemporalSeq2SeqAttnModel over CrnnEncoder.  The Cnn14 is never run (the ``_cnn_attn`` hook)."""
    import audiocaption_amd as A
    from audiocaption_amd import build, procedural as P
    build.build()
    if kind == "rnn":
        state = P.to_torch(P.cnn14rnn_trm_state(4981))
        model = A.init_model_from_config(A.cnn14rnn_trm_config(4981), print_fn=lambda s: None)
        model.load_state_dict(state, strict=True)
    elif kind == "trm":
        state = P.to_torch(P.cnn14trm_trm_state(4981))
        model = A.init_model_from_config(A.config.cnn14trm_trm_config(4981), print_fn=lambda s: None)
        model.load_state_dict(state, strict=True)
    else:
        import _attn_gru_train_ref as R
        state = R.pub_state(*R.load_g22()["pub_recipe"])
        cfg = A.cnn14rnn_trm_config(R.PUB["vocab_size"])
        cfg["decoder"] = {"type": "audiocaption_amd.rnn_decoder.TemporalBahAttnDecoder", "args": dict(R.PUB, dropout=0.5)}
        cfg["type"] = "audiocaption_amd.attn_model.TemporalSeq2SeqAttnModel"
        model = A.init_model_from_config(cfg, print_fn=lambda s: None)
        missing, unexpected = model.load_state_dict(state, strict=False)
        assert not unexpected and all(k.startswith("encoder.cnn.") for k in missing)
    state = {k: v for k, v in state.items() if not k.startswith("encoder.cnn.")}
    return model.to("cuda:0").train(), state


@pytest.fixture(scope="module", params=["rnn", "trm", "attn"])
def built(request):
    kind = request.param
    model, state = _build(kind)
    return kind, model, state


P_DEC, P_ENC = {"rnn": 0.2, "trm": 0.2, "attn": 0.5}, {"rnn": 0.5, "trm": 0.2, "attn": 0.5}
TAGS = [0, 1, 3]


def _extra(kind):
    return {"temporal_tag": torch.tensor(TAGS)} if kind == "attn" else {}


def _width(kind):
    return 256 if kind == "trm" else 512


def test_training_forward_fc_emb_equals_the_inference_encoder(built):
    """(a) every dropout 0: ``fc_emb`` of the training forward, in train() and in eval(), is the inference encoder's."""
    kind, model, _ = built
    _set_p(model, 0.0, 0.0)
    attn = _cnn_attn().to(DEV)
    model.eval()
    with torch.no_grad():
        sub = model.encoder.trm if kind == "trm" else model.encoder.rnn
        want = sub({"attn": attn, "attn_len": torch.tensor(LENS)})["fc_emb"].clone()
        teacher = model(_batch(**_extra(kind)))
    assert tuple(want.shape) == (N, _width(kind)) and model.encoder.fc_emb_size == _width(kind)
    assert not teacher["fc_emb"].requires_grad and not teacher["logit"].requires_grad
    model.train()
    model.encoder.cnn.eval()
    student = model(_batch(**_extra(kind)))
    assert student["fc_emb"].requires_grad and student["logit"].requires_grad
    top = float(want.abs().max())
    for tag, got in (("eval", teacher["fc_emb"]), ("train", student["fc_emb"])):
        d = float((got.detach() - want).abs().max()) / top
        print(f"[{kind} fc_emb {tag}] {d:.2e}")
        assert tuple(got.shape) == tuple(want.shape) and d <= 1e-5


def _reference(kind, state, gates, heads, tchr):
    """float64 autograd over the restatements: (fc_emb, gradients of the enc_kd term alone, of caption loss + 0.5 enc_kd,
    the head's own gradients at weight 1)."""
    from oracle import train_path as OT
    cap, cap_len = _cap()
    attn = _cnn_attn().double()
    lens = torch.tensor(LENS)
    keys = [k for k in state if not k.endswith("pos_encoder.pe")]
    st = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
    for k in keys:
        st[k] = st[k].detach().clone().requires_grad_(True)
    use_cap = [1] * (TC - 1)
    if kind == "rnn":
        # (oracle.cpu_path's GRU allocates its state in the default dtype)
        torch.set_default_dtype(torch.float64)
        try:
            emb = OT.gru_train_forward(st, attn, lens, SEED, P_ENC[kind])
        finally:
            torch.set_default_dtype(torch.float32)
        fc = emb.sum(1) / lens[:, None].double()
        out = OT.train_forward(st, emb, lens, cap, use_cap, SEED, P_DEC[kind], teacher_forcing=True,
                               relu_gates={"mem": gates["mem"].double(), "ffn": [g.double() for g in gates["dec_ffn"]]})
        cap_loss = OT.label_smoothing_loss(out["logit"], cap[:, 1:], torch.as_tensor(cap_len) - 1, 0.1)
    elif kind == "trm":
        import _trm_train_ref as TR
        emb = TR.encoder_train_forward(st, attn, lens, SEED, P_ENC[kind], relu_gates=gates)
        fc = emb[:, 0]
        out = OT.train_forward(st, emb, lens + 1, cap, use_cap, SEED, P_DEC[kind], teacher_forcing=True,
                               relu_gates={"mem": gates["mem"].double(), "ffn": [g.double() for g in gates["dec_ffn"]]})
        cap_loss = OT.label_smoothing_loss(out["logit"], cap[:, 1:], torch.as_tensor(cap_len) - 1, 0.1)
    else:
        import _attn_gru_train_ref as R
        emb, fc = R.encoder_forward(st, attn, lens, P_ENC[kind], SEED)
        dec = {k[len("decoder."):]: v for k, v in st.items() if k.startswith("decoder.")}
        out = R.decoder_forward(dec, emb, lens, fc, cap, use_cap, torch.tensor(TAGS), P_DEC[kind], SEED)
        cap_loss = R.label_smoothing_loss(out["logit"], cap[:, 1:], torch.as_tensor(cap_len) - 1, 0.1)
    sp, tp, scale = heads
    h = _ref_full(fc.detach(), tchr, sp, tp, scale.detach(), E.CONTRA)
    kd_term = (fc * h["fc_emb"]).sum()          # its gradient is d enc_kd / d fc_emb chained into the encoder
    leaves = [st[k] for k in keys]

    def grads(loss):
        gs = torch.autograd.grad(loss, leaves, allow_unused=True, retain_graph=True)
        return {k: (g if g is not None else torch.zeros_like(st[k])) for k, g in zip(keys, gs)}
    return {"fc": fc.detach(), "kd": grads(kd_term), "both": grads(cap_loss + 0.5 * kd_term), "head": h,
            "cap_loss": float(cap_loss.detach())}


def _gates(kind, model):
    """The ReLU outputs of the forward just run, consulted by the restatements at ReLU kinks only."""
    sv = model._train_engine._saved
    ws_ = sv["ws"]
    if kind == "attn":
        return None
    R_, Tm, F_ = sv["lay"]["R"], sv["Tm"], sv["F"]
    g = {"mem": ws_.tensor("mem_a")[:N * Tm * 256].view(N * Tm, 256).cpu(),
         "dec_ffn": [ws_.tensor(f"hdn{l}")[:R_ * F_].view(R_, F_).cpu() for l in range(model.decoder.nlayers)]}
    if kind == "trm":
        Fe = model.encoder.trm.dim_feedforward
        g["proj"] = ws_.tensor("enc_a")[:N * TQ * 256].view(N * TQ, 256).cpu()
        g["ffn"] = [ws_.tensor(f"enc_hdn{l}")[:N * Tm * Fe].view(N * Tm, Fe).cpu() for l in range(2)]
    return g


def _compare(tag, model, want, zero_decoder):
    named = {k: p for k, p in model.named_parameters() if p.requires_grad}
    assert set(named) <= set(want) and any(k.startswith("encoder.") for k in named), set(named) - set(want)
    bad, worst = [], 0.0
    for k, p in named.items():
        assert p.grad is not None, k
        if zero_decoder and k.startswith("decoder."):
            assert not p.grad.any(), k                       # no gradient reached logit: exactly zero
            assert not want[k].any()
            continue
        top = float(want[k].abs().max())
        d = float((p.grad.double().cpu() - want[k]).abs().max()) / top
        worst = max(worst, d)
        if not d <= ENC_BAR:
            bad.append((k, d))
    print(f"[{tag}] worst gradient difference vs the restatement: {worst:.2e}")
    assert not bad, bad


def test_enc_kd_gradient_reaches_the_encoder(built):
    """(b) loss = enc_kd_loss alone and (c) caption loss + 0.5 enc_kd_loss, dropout active, against float64 autograd over the
    restatements with the same masks."""
    from audiocaption_amd.enc_kd import enc_kd_loss
    from audiocaption_amd.loss import LabelSmoothingLoss
    kind, model, state = built
    _set_p(model, P_DEC[kind], P_ENC[kind])
    heads = _heads(_width(kind), TD, SHARED, 9)
    sp, tp, scale = heads
    tchr = torch.randn(N, TD, generator=torch.Generator().manual_seed(10)).to(DEV)
    cap, cap_len = _cap()
    want = None
    for case in ("kd", "both"):
        for p in list(model.parameters()) + [sp.weight, sp.bias, tp.weight, tp.bias, scale]:
            p.grad = None
        out = model(_batch(**_extra(kind)))
        if want is None:
            want = _reference(kind, state, _gates(kind, model), heads, tchr)
            d = float((out["fc_emb"].detach().double().cpu() - want["fc"]).abs().max()) / float(want["fc"].abs().max())
            print(f"[{kind} fc_emb vs restatement, dropout on] {d:.2e}")
            assert d <= 2e-5
        kd = enc_kd_loss(out["fc_emb"], tchr, sp, tp, scale, "contra")
        assert abs(float(kd.detach()) - float(want["head"]["loss"])) <= 1e-4 * float(want["head"]["loss"])
        if case == "kd":
            kd.backward()
        else:
            cl = LabelSmoothingLoss(smoothing=0.1)({"logit": out["logit"], "tgt": cap[:, 1:].to(DEV),
                                                    "tgt_len": torch.as_tensor(cap_len - 1)})
            assert abs(float(cl.detach()) - want["cap_loss"]) <= 2e-5 * want["cap_loss"]
            (cl + 0.5 * kd).backward()
        _compare(f"{kind} {case}", model, want[case], zero_decoder=case == "kd")
        w = 1.0 if case == "kd" else 0.5
        for k, p in (("stdnt_proj.weight", sp.weight), ("tchr_proj.weight", tp.weight), ("logit_scale", scale)):
            ref = w * want["head"][k]
            assert float((p.grad.double().cpu() - ref).abs().max()) <= ENC_BAR * float(ref.abs().max()), k
    # a plain captioning loss still takes the route it took before (no gradient arrives on fc_emb)
    for p in model.parameters():
        p.grad = None
    model(_batch(**_extra(kind)))["logit"].sum().backward()
    assert all(p.grad is not None for p in model.parameters() if p.requires_grad)


def test_wrapper_trains_encoder_heads_and_logit_scale(built):
    """(d) ContraEncoderKdWrapper in mode "train" with ``tchr_output``: ``enc_kd_loss`` and ``logit`` come back, and after
    ``backward()`` the encoder, the decoder, the heads and ``logit_scale`` all carry a gradient; the teacher's side is the
    eval-mode forward's ``fc_emb`` (run_kd.py:42-44)."""
    from audiocaption_amd.kd_wrapper import ContraEncoderKdWrapper, ContraMseEncoderKdWrapper
    from audiocaption_amd.loss import LabelSmoothingLoss
    kind, model, _ = built
    _set_p(model, P_DEC[kind], P_ENC[kind])
    cap, cap_len = _cap()
    model.eval()
    with torch.no_grad():
        teacher_emb = model(_batch(**_extra(kind)))["fc_emb"]
    model.train()
    model.encoder.cnn.eval()
    for cls in (ContraEncoderKdWrapper, ContraMseEncoderKdWrapper):
        for p in model.parameters():
            p.grad = None
        w = cls(model, SHARED, _width(kind)).to(DEV)
        out = w(_batch(tchr_output={"embedding": teacher_emb}, **_extra(kind)))
        assert out["enc_kd_loss"].requires_grad and out["logit"].requires_grad and out["enc_kd_loss"].dim() == 0
        loss = LabelSmoothingLoss(smoothing=0.1)({"logit": out["logit"], "tgt": cap[:, 1:].to(DEV),
                                                  "tgt_len": torch.as_tensor(cap_len - 1)}) + 0.5 * out["enc_kd_loss"]
        loss.backward()
        for k, p in w.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any(), k
        assert any(k.startswith("model.encoder.") for k, p in w.named_parameters() if p.requires_grad)
        assert w.logit_scale.grad is not None and w.stdnt_proj.weight.grad is not None


def test_effb2_captioner_still_refuses_encoder_kd_in_train_mode():
    """(e) no training engine differentiates the EfficientNet-B2 encoder: the refusal and its head-only wording stay."""
    from audiocaption_amd.hf_wrapper import Effb2TrmCaptioningModel, Effb2TrmConfig
    m = Effb2TrmCaptioningModel(Effb2TrmConfig())
    d = {"mode": "train", "wav": torch.zeros(2, 16000), "wav_len": [16000, 16000], "cap": torch.zeros(2, 5, dtype=torch.int64),
         "cap_len": np.array([5, 5]), "ss_ratio": 1, "tchr_output": {"embedding": torch.zeros(2, 768)}}
    with pytest.raises(NotImplementedError, match="head-only"):
        m.model(d)
