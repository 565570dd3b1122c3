"""CPU tests of the condition-controlled attention-GRU captioners and the specificity loss: the restatement of
tests/_cond_attn_gru_ref.py against what the REFERENCE computed (tests/golden/g26_cond_attn_gru.npz), the host-side checks
and refusals, the strict load of a reference-shaped state dict, the C ABI's new rows, the refusals the entry points make
before any launch, and ``caption_metrics.specificity`` (nothing here needs a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _attn_gru_ref as AR
import _attn_gru_train_ref as TR
import _cond_attn_gru_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-4                                         # tests/test_gpu_attn_gru.py
LOGIT_BAR, LOSS_BAR, GRAD_BAR = 2e-5, 2e-5, 1e-4    # tests/test_gpu_attn_gru_train.py
NEW_ENTRIES = ("ac_bah_memory_cond", "ac_bah_train_forward_cond", "ac_bah_train_backward_cond", "ac_specificity_loss",
               "ac_specificity_loss_bwd")


@pytest.fixture(scope="module")
def g26():
    return R.load_g26()


# ---- the restatement against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.INFER))
def test_inference_restatement_vs_reference(g26, kind, name):
    shape = R.INFER[name][0]
    key = R.infer_prefix(kind, name)
    sd = R.state(kind, shape, *R.recipe(g26, kind, shape)) if shape != "pub" else \
        {k[len("decoder."):]: v for k, v in R.pub_state(kind, *R.recipe(g26, kind, "pub")).items() if k.startswith("decoder.")}
    mem, lens, cond, L, beams = R.infer_inputs(name)
    res = R.greedy(kind, sd, mem, lens, cond, L)
    assert np.array_equal(res["seq"].numpy(), g26[f"{key}_greedy_seq"])
    live = AR.live_mask(res["seq"].numpy())
    tv, ti = res["logit"].topk(8, dim=2)
    assert float(np.abs(tv.numpy() - g26[f"{key}_greedy_top_val"])[live].max()) < GATE
    assert np.array_equal(ti.numpy()[..., 0][live], g26[f"{key}_greedy_top_idx"][..., 0][live])
    assert float((tv[..., 0] - tv[..., 1])[torch.from_numpy(live)].min()) >= GATE      # the draw rule
    assert float(np.abs(res["state"].numpy() - g26[f"{key}_greedy_state"]).max()) < GATE
    if f"{key}_greedy_attn_weight" in g26:
        assert float(np.abs(res["attn_weight"].numpy() - g26[f"{key}_greedy_attn_weight"]).max()) < GATE
    for k in beams:
        trace = []
        b = R.beam_search(kind, sd, mem, lens, cond, k, L, trace=trace)
        assert np.array_equal(b["seq"].numpy(), g26[f"{key}_beam{k}_seq"])
        assert min(r["margin"] for r in trace) >= GATE
        if f"{key}_beam{k}_attn_weight" in g26:
            assert float(np.abs(b["attn_weight"].numpy() - g26[f"{key}_beam{k}_attn_weight"]).max()) < GATE
    # the condition is an input: other values, other logits
    other = R.greedy(kind, sd, mem, lens, cond.roll(1) + 0.25, L)
    assert float((other["logit"][:, 0] - res["logit"][:, 0]).abs().max()) > 1e-3


def _check_step(g26, case, idx_prefix, res, grads):
    top = res["logit"].topk(8, dim=-1)
    want = g26[f"{case}_logit_top_val"]
    assert float(np.abs(top.values.numpy() - want).max()) < LOGIT_BAR * float(np.abs(want).max())
    assert np.array_equal(top.indices.numpy()[..., 0], g26[f"{case}_logit_top_idx"][..., 0])
    assert np.array_equal(res["seq"].numpy(), g26[f"{case}_seq"])
    for k in ("loss", "word_loss", "condition_loss"):
        assert abs(float(res[k]) - float(g26[f"{case}_{k}"])) <= LOSS_BAR * abs(float(g26[f"{case}_{k}"])), k
    assert set(grads) == {k.split("/", 1)[1] for k in g26 if k.startswith(f"{case}_gnorm/")}
    for key, grad in grads.items():
        gn = float(g26[f"{case}_gnorm/{key}"])
        assert abs(float(grad.double().norm()) - gn) <= GRAD_BAR * gn, key      # T = 1: the gradient of W_hh is exactly 0
        sample = grad.reshape(-1)[torch.from_numpy(g26[f"{idx_prefix}_sample_idx/{key}"])].numpy()
        assert float(np.abs(sample - g26[f"{case}_gsample/{key}"]).max()) <= GRAD_BAR * float(grad.abs().max()), key


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name,tag", [(n, t) for n in R.TRAIN for t in ("tf", "ss")])
def test_decoder_training_restatement_vs_reference(g26, kind, name, tag):
    shape = R.TRAIN[name][0]
    case = f"{kind}_train_{name}_{tag}"
    sd = R.state(kind, shape, *R.recipe(g26, kind, shape))
    mem, lens, cond, cap, cap_len = R.train_inputs(name)
    use_cap = g26[f"{case}_use_cap"].tolist()
    res = R.decoder_step_grads(kind, sd, mem, lens, cond, cap, cap_len, use_cap)
    grads = {"decoder." + k: v for k, v in res["grads"].items()}
    grads["attn_emb"] = res["d_attn_emb"]
    _check_step(g26, case, f"{kind}_train_{name}", res, grads)
    if f"{case}_attn_weight" in g26:
        assert float((res["attn_weight"] - torch.from_numpy(g26[f"{case}_attn_weight"])).abs().max()) < LOGIT_BAR
    for b, n in enumerate(lens.tolist()):
        assert not res["d_attn_emb"][b, n:].any()
    fed = TR.fed_back_gaps(res["gap"], use_cap, False)
    assert not fed.numel() or float(fed.min()) >= GATE


@pytest.mark.parametrize("kind", R.KINDS)
def test_model_training_restatement_vs_reference(g26, kind):
    """The whole model at the published widths under SpecificityLossWrapper(LabelSmoothingLoss(0.1), ws, "sum", 0.3)."""
    state = R.pub_state(kind, *R.recipe(g26, kind, "pub"))
    cap, cap_len = TR.pub_caption()
    cond = R.conditions(TR.PUB_N, 2)
    case = f"{kind}_train_pub_ss"
    use_cap = g26[f"{case}_use_cap"].tolist()
    res = R.model_step_grads(kind, state, TR.pub_cnn_attn(), torch.tensor(TR.PUB_LENS), cond, cap, cap_len, use_cap,
                             ws=R.word_specificity(TR.PUB["vocab_size"]), targets=cond, reduce="sum", alpha=R.ALPHA)
    assert float(res["condition_loss"]) > 0
    _check_step(g26, case, f"{kind}_train_pub", res, res["grads"])


@pytest.mark.parametrize("case", R.LOSS_GRID, ids=R.loss_case_name)
def test_loss_restatement_vs_reference(g26, case):
    logit, tgt_len, conds, ws, reduce, alpha = R.loss_inputs(case)
    key = "loss_" + R.loss_case_name(case)
    gate_loss, gate_grad = g26["loss_gate"].tolist()
    assert gate_loss == LOSS_BAR and gate_grad == GRAD_BAR      # the reference's float32 run stays within a quarter of both
    for dtype in (torch.float32, torch.float64):
        leaf = logit.detach().to(dtype).clone().requires_grad_(True)
        word = R.stand_in_word_loss({"logit": leaf})
        cl = R.specificity_loss(leaf, ws, tgt_len, conds, reduce)
        loss = word + alpha * cl
        loss.backward()
        want = g26[f"{key}_losses"]
        for got, w in zip((loss, word, cl), want):
            assert abs(float(got.detach()) - w) <= gate_loss * abs(w)
        gn = float(g26[f"{key}_gnorm"])
        assert abs(float(leaf.grad.double().norm()) - gn) < gate_grad * gn
        sample = leaf.grad.reshape(-1)[torch.from_numpy(g26[f"{key}_sample_idx"])].double().numpy()
        assert float(np.abs(sample - g26[f"{key}_gsample"]).max()) < gate_grad * float(leaf.grad.abs().max())


# ---- the host side -----------------------------------------------------------------------------------------------------
def _decoder(kind, shape="small", **kw):
    import audiocaption_amd as A
    cls = {"cond": A.ConditionalBahAttnDecoder, "spec": A.SpecificityBahAttnDecoder}[kind]
    return cls(**dict(dict(R.SHAPES[shape], dropout=0.5), **kw))


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_state_dict_loads_strictly(g26, kind):
    dec = _decoder(kind, "pub")
    assert set(dec.state_dict()) == set(g26[f"{kind}_state_keys"].tolist())
    state = R.pub_state(kind, 26, 3.0)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")}, strict=True)
    E, A_ = TR.PUB["emb_dim"], TR.PUB["attn_emb_dim"]
    assert dec.model.weight_ih_l0.shape[1] == (3 * E if kind == "cond" else E + A_ + 1)
    assert not hasattr(dec, "fc_proj") and hasattr(dec, "condition_embedding") == (kind == "cond")
    assert dec.attn_size == 512 and dec.d_model == 512 and dec.in_dropout.p == 0.5
    if kind == "spec":
        x = torch.ones(2)
        assert dec.ctx_proj(x) is x      # the reference's identity


@pytest.mark.parametrize("kind", R.KINDS)
def test_constructor_limits(kind):
    for bad in (dict(emb_dim=48), dict(d_model=1056), dict(attn_size=100), dict(attn_emb_dim=0), dict(vocab_size=16385),
                dict(rnn_type="LSTM"), dict(num_layers=2), dict(bidirectional=True)):
        with pytest.raises(NotImplementedError):
            _decoder(kind, **bad)
    _decoder(kind, vocab_size=16384, emb_dim=1024)


def test_check_condition():
    from audiocaption_amd.rnn_decoder import check_condition
    got = check_condition([0.0, 1.0, 0.37, -2.5, 7.5], 5)
    assert got.dtype == torch.float32 and got.tolist() == pytest.approx([0.0, 1.0, 0.37, -2.5, 7.5])
    assert check_condition(torch.tensor([[0.5], [2.0]], dtype=torch.float64), 2).shape == (2,)
    assert check_condition(np.array([0.25], dtype=np.float32), 1).tolist() == [0.25]
    for bad in (None, [0.0, 1.0], [0.0, float("nan"), 1.0], [0.0, float("inf"), 1.0], torch.tensor([0, 1, 1]),
                torch.tensor([True, False, True]), [0, 1, 2]):
        with pytest.raises(ValueError, match="condition"):
            check_condition(bad, 3)


@pytest.mark.parametrize("kind", R.KINDS)
def test_model_refusals(kind):
    import audiocaption_amd as A
    dec = _decoder(kind)
    model = A.ConditionalSeq2SeqAttnModel(torch.nn.Identity(), dec)
    assert model.compatible_decoders == (A.ConditionalBahAttnDecoder, A.SpecificityBahAttnDecoder)
    assert model.train_forward_keys[-1] == "condition" and model.inference_forward_keys[-1] == "condition"
    mem = torch.zeros(3, 7, 160)
    base = {"mode": "inference", "attn_emb": mem, "fc_emb": torch.zeros(3, 96), "attn_emb_len": [7, 7, 7]}
    for method in ("greedy", "beam", "sample"):       # a missing or malformed condition is refused on the host
        with pytest.raises(ValueError, match="condition"):
            model(dict(base, sample_method=method))
        with pytest.raises(ValueError, match="condition"):
            model(dict(base, sample_method=method, condition=[0.0, float("nan"), 1.0]))
        with pytest.raises(ValueError, match="condition"):
            model(dict(base, sample_method=method, condition=[0.0, 1.0]))
    with pytest.raises(ValueError, match="condition"):
        dec({"word": torch.ones(3, 1, dtype=torch.long), "attn_emb": mem, "attn_emb_len": [7, 7, 7], "fc_emb": base["fc_emb"]})
    with pytest.raises(NotImplementedError, match="dbs"):
        model(dict(base, sample_method="dbs", condition=[0.0, 1.0, 2.0]))
    with pytest.raises(NotImplementedError, match="forward_async"):
        model.forward_async(dict(base, condition=[0.0, 1.0, 2.0]))
    with pytest.raises(NotImplementedError, match="train"):
        model({"mode": "train", "condition": [0.0, 1.0, 2.0]})       # over another encoder than CrnnEncoder
    with pytest.raises(NotImplementedError):
        A.EnsembleModel([model, model])
    with pytest.raises(NotImplementedError, match="ConditionalSeq2SeqAttnModel"):
        A.ScstWrapper(model)
    with pytest.raises(NotImplementedError, match="rollout"):
        dec.train_rollout(mem, None, [7, 7, 7], 4, 1.0, None)
    # the plain models do not take the conditional decoders, and the conditional model takes no plain decoder
    with pytest.raises(NotImplementedError, match="ConditionalSeq2SeqAttnModel"):
        A.Seq2SeqAttnModel(torch.nn.Identity(), dec)
    with pytest.raises(AssertionError):
        A.ConditionalSeq2SeqAttnModel(torch.nn.Identity(), A.BahAttnCatFcDecoder(dropout=0.5, **TR.SMALL))


def test_scst_wrapper_refuses_the_conditional_model_over_a_crnn_encoder():
    import audiocaption_amd as A
    cfg = A.cnn14rnn_trm_config(517)
    cfg["decoder"] = {"type": "captioning.models.rnn_decoder.SpecificityBahAttnDecoder",
                      "args": dict(TR.SMALL, attn_emb_dim=512, fc_emb_dim=512, dropout=0.2)}
    cfg["type"] = "captioning.models.attn_model.ConditionalSeq2SeqAttnModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s: None)       # config.py routes the reference's names
    assert type(model) is A.ConditionalSeq2SeqAttnModel and type(model.decoder) is A.SpecificityBahAttnDecoder
    with pytest.raises(NotImplementedError, match="ConditionalSeq2SeqAttnModel"):
        A.ScstWrapper(model)


def test_routing_and_exports():
    import sys
    import audiocaption_amd as A
    from audiocaption_amd import compat, config
    for name in ("ConditionalBahAttnDecoder", "SpecificityBahAttnDecoder", "ConditionalSeq2SeqAttnModel",
                 "SpecificityLossWrapper"):
        assert name in A.__all__ and hasattr(A, name)
    for path, cls in (("captioning.models.attn_model.ConditionalSeq2SeqAttnModel", A.ConditionalSeq2SeqAttnModel),
                      ("captioning.models.rnn_decoder.ConditionalBahAttnDecoder", A.ConditionalBahAttnDecoder),
                      ("captioning.models.rnn_decoder.SpecificityBahAttnDecoder", A.SpecificityBahAttnDecoder),
                      ("captioning.losses.loss.SpecificityLossWrapper", A.SpecificityLossWrapper)):
        assert config.get_cls_from_str(path) is cls
    saved = {k: v for k, v in sys.modules.items() if k.startswith("captioning")}
    try:
        compat.install()
        import importlib
        assert importlib.import_module("captioning.models.attn_model").ConditionalSeq2SeqAttnModel is A.ConditionalSeq2SeqAttnModel
        assert importlib.import_module("captioning.models.rnn_decoder").SpecificityBahAttnDecoder is A.SpecificityBahAttnDecoder
        assert importlib.import_module("captioning.losses.loss").SpecificityLossWrapper is A.SpecificityLossWrapper
    finally:
        for k in [k for k in sys.modules if k.startswith("captioning")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_loss_wrapper_host_checks():
    import audiocaption_amd as A
    logit = torch.zeros(2, 3, 50)
    out = {"logit": logit, "tgt_len": torch.tensor([3, 1]), "conditions": torch.tensor([0.5, 1.0])}
    word = lambda o: o["logit"].sum()      # noqa: E731
    with pytest.raises(ValueError, match="word_specificity"):
        A.SpecificityLossWrapper(word, torch.zeros(49))(out)
    with pytest.raises(ValueError, match="tgt_len"):
        A.SpecificityLossWrapper(word, torch.zeros(50), sentence_reduce="mean")(out)
    with pytest.raises(ValueError, match="one value per clip"):
        A.SpecificityLossWrapper(word, torch.zeros(50))(dict(out, conditions=torch.tensor([0.5])))
    w = A.SpecificityLossWrapper(word, torch.zeros(50), "mean", 0.3)
    assert w.alpha == 0.3 and w.sentence_reduce == "mean" and w.loss_fn is word
    with pytest.raises(A._lib.HipLibraryError, match="CPU"):     # there is no CPU fallback for the condition term
        from audiocaption_amd import build
        build.build()
        A.SpecificityLossWrapper(word, torch.zeros(50))(out)


def test_specificity_metric():
    from audiocaption_amd.caption_metrics import specificity
    table = {"a": 0.5, "dog": 2.25, "barks": 3.0, "loudly": 1.25}
    preds = [{"tokens": "a dog barks"}, {"tokens": "a dog barks loudly"}, {"tokens": ""}]
    assert specificity(preds, table) == pytest.approx((5.75 + 7.0 + 0.0) / 3)
    assert specificity(["dog  dog", "a"], table) == pytest.approx((4.5 + 0.5) / 2)
    with pytest.raises(KeyError):
        specificity(["a cat barks"], table)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_abi_rows_and_build_list():
    from audiocaption_amd import _lib, build
    assert "spec_loss.hip" in build.SOURCES and _lib.ABI_VERSION == 2
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    assert "#define AC_ABI_VERSION 2" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        proto = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert proto, name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_long if proto.group(1) == "long" else ctypes.c_int)
        params = [a.strip() for a in proto.group(2).split(",")]
        assert len(params) == len(args), name
        for prm, ct in zip(params, args):      # pointers as pointers, floats as floats, 64-bit words as such
            want = ctypes.c_void_p if "*" in prm else ctypes.c_float if prm.startswith("float") else \
                ctypes.c_ulonglong if prm.startswith("unsigned long long") else ctypes.c_long if prm.startswith("long") \
                else ctypes.c_int
            assert ct is want, (name, prm)
    fields = re.search(r"typedef struct \{([^}]*)\} ac_bah_weights;", header).group(1)
    ints = [f.strip() for line in fields.split(";") if line.strip().startswith("int32_t")
            for f in line.strip()[len("int32_t"):].split(",")]
    assert ints == [n for n, t in _lib.AcBahWeights._fields_ if t is ctypes.c_int32] and ints[-1] == "variant"


def _fake_weights(variant):
    from audiocaption_amd import _lib
    keep = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(keep))      # a non-null address no accepted call ever reaches
    w = _lib.AcBahWeights()
    w.emb_dim, w.d_model, w.attn_size, w.attn_emb_dim, w.fc_emb_dim, w.vocab, w.n_tags = 64, 128, 96, 160, 96, 517, 0
    w.variant = variant
    unused = {0: ("temb",), 1: ("temb", "fc_b"), 2: ("temb", "fc_b", "ctx_w", "ctx_b")}[variant]
    for name, t in _lib.AcBahWeights._fields_:
        if t is ctypes.c_void_p and name not in unused:
            setattr(w, name, p)
    g = _lib.AcBahGrads()
    for name, _ in _lib.AcBahGrads._fields_:
        if name not in unused:
            setattr(g, name, p)
    return w, g, p, keep


@pytest.mark.parametrize("variant", [1, 2])
def test_entry_points_refuse_before_touching_the_device(variant):
    """AC_ERR_ARG / -1 for a variant mismatch, a slot the variant does not use, a bad width, Tm 4096 and null pointers
    (nothing is launched on a machine without a GPU)."""
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    w, g, p, keep = _fake_weights(variant)
    ref = ctypes.byref
    assert lib.ac_bah_workspace_floats(ref(w), 5, 15, 70, 6) > 0 and lib.ac_bah_train_workspace_floats(ref(w), 5, 70, 8) > 0
    plain = _fake_weights(0)[0]
    wrong = []
    for field in ("fc_b",) + (("ctx_w",) if variant == 2 else ()):       # a slot the variant does not use must be NULL
        x = _lib.AcBahWeights.from_buffer_copy(w)
        setattr(x, field, p)
        wrong.append(x)
    for field, value in (("attn_size", 100), ("emb_dim", 1056), ("vocab", 16385), ("n_tags", 4), ("variant", 3), ("fc_w", None)):
        x = _lib.AcBahWeights.from_buffer_copy(w)
        setattr(x, field, value)
        wrong.append(x)
    for x in wrong:
        assert lib.ac_bah_workspace_floats(ref(x), 5, 15, 70, 6) == -1
        assert lib.ac_bah_train_workspace_floats(ref(x), 5, 70, 8) == -1
    wrong.append(plain)       # the _cond entry points refuse the plain decoder ...
    mem = [ref(w), p, p, 5, 15, 70, 6, p, None]
    coins = (ctypes.c_int * 8)(*([1] * 8))
    fwd = [ref(w), p, p, p, p, 9, coins, 5, 70, 8, 1, 0.0, 0, None, p, p, p, p, p, p, p, None]
    bwd = [ref(w), ref(g), p, p, p, p, 5, 70, 8, 0.0, 0, None, p, p, p, None]
    no_w_ih = _lib.AcBahGrads.from_buffer_copy(g)
    no_w_ih.w_ih = None
    extra = _lib.AcBahGrads.from_buffer_copy(g)
    extra.fc_b = p
    for fn, good, cases in (
            (lib.ac_bah_memory_cond, mem, [(0, ref(x)) for x in wrong] + [(1, None), (2, None), (3, 0), (4, 4), (5, 4096),
                                                                            (6, 0), (7, None)]),
            (lib.ac_bah_train_forward_cond, fwd, [(0, ref(x)) for x in wrong] + [
                (1, None), (2, None), (3, None), (4, None), (5, 7), (6, None), (8, 4096), (9, 0), (11, -0.1), (11, 1.0),
                (14, None), (15, None), (18, None), (20, None)]),
            (lib.ac_bah_train_backward_cond, bwd, [(0, ref(x)) for x in wrong] + [
                (0, None), (1, None), (1, ref(no_w_ih)), (1, ref(extra)), (2, None), (3, None), (5, None), (7, 4096), (8, 0),
                (12, None), (13, None), (14, None)])):
        for i, v in cases:
            args = list(good)
            args[i] = v
            assert fn(*args) == _lib.AC_ERR_ARG, (fn.__name__, i)
    # ... and the entry points that take fc_emb refuse the conditional ones
    assert lib.ac_bah_memory(*mem) == _lib.AC_ERR_ARG
    assert lib.ac_bah_train_forward(*(fwd[:7] + [None] + fwd[7:])) == _lib.AC_ERR_ARG
    assert lib.ac_bah_train_backward(*bwd) == _lib.AC_ERR_ARG
    assert lib.ac_bah_train_rollout(ref(w), p, p, p, None, 5, 70, 8, 1, 2, 1.0, p, None, 8, 0.0, 0, None, p, p, p, p, p, p, p,
                                    p, None) == _lib.AC_ERR_ARG
    del keep


def test_loss_entry_points_refuse_before_touching_the_device():
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    keep = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(keep))
    fwd = [p, p, p, p, 2, 3, 50, 0, p, p, p, p, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (6, 0), (8, None), (9, None), (10, None), (11, None)):
        args = list(fwd)
        args[i] = v
        assert lib.ac_specificity_loss(*args) == _lib.AC_ERR_ARG, i
    bwd = [p, p, p, p, p, p, p, 2, 3, 50, 1, p, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, 0), (8, -1), (9, 0), (11, None)):
        args = list(bwd)
        args[i] = v
        assert lib.ac_specificity_loss_bwd(*args) == _lib.AC_ERR_ARG, i
    del keep
