"""Keyword-conditioned Transformer captioners without a GPU: the CPU restatement of tests/_keyword_trm_ref.py against what the
REFERENCE produced (tests/golden/g27_keyword_trm.npz), and the Python / C surface that needs no device - names and order
of the parameters, the compatibility assertions, every refusal, the keyword checks, the header / ctypes rows of the new
entry points with their argument refusals, and construction through the reference's dotted paths."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _keyword_trm_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ac_trm_kw_greedy_segments", "ac_trm_kw_sample", "ac_trm_kw_forward_tokens", "ac_trm_kw_beam_step",
               "ac_trm_kw_embed_qkv", "ac_kw_embed_fwd", "ac_kw_embed_bwd")


@pytest.fixture(scope="module")
def g27():
    return R.load_g27()


def _decoder(shape="d128", **over):
    import audiocaption_amd as A
    kw = dict(R.SHAPES[shape], dropout=0.2)
    kw.update(over)
    return A.KeywordProbTransformerDecoder(**kw).eval()


# ---- the restatement against the reference's outputs ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.SHAPES))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_restatement_searches_and_forward_vs_g27(g27, shape, dtype):
    state = R.decoder_state(shape, *R.recipe(g27, shape))
    if dtype == "float64":
        state = R.f64(state)
    for which in (0, 1):
        attn, lens, kw = R.infer_inputs(shape, which)
        out = R.greedy(state, attn, lens, kw, shape)
        want = g27[f"{shape}_k{which}_greedy_seq"]
        assert np.array_equal(out["seq"].numpy(), want)
        live = R.live_mask(want)
        idx = torch.from_numpy(g27[f"{shape}_k{which}_greedy_top_idx"]).long()
        got = out["logit"].gather(2, idx)
        d = float((got.double() - torch.from_numpy(g27[f"{shape}_k{which}_greedy_top_val"]).double())[live].abs().max())
        print(f"[{shape} k{which} greedy top-8, {dtype}] {d:.3e}")
        assert d < R.GATE
        if dtype == "float64":
            for k in R.BEAMS:
                assert np.array_equal(R.beam_search(state, attn, lens, kw, shape, k)["seq"].numpy(),
                                      g27[f"{shape}_k{which}_beam{k}_seq"])
                assert np.array_equal(R.beam_search(state, attn, lens, kw, shape, k, n_best=True, n_best_size=k)["seq"].numpy(),
                                      g27[f"{shape}_k{which}_beam{k}_nbest_seq"])
    assert not np.array_equal(g27[f"{shape}_k0_greedy_seq"], g27[f"{shape}_k1_greedy_seq"])    # the keywords steer the caption
    inp = R.forward_inputs(shape)
    out = R.forward(state, inp["word"], inp["attn_emb"], inp["attn_emb_len"], inp["keyword"], shape)
    for key in ("logit", "embed"):
        assert float((out[key].double() - torch.from_numpy(g27[f"{shape}_forward_{key}"]).double()).abs().max()) < R.GATE


@pytest.mark.parametrize("tag", ["tf", "ss"])
def test_restatement_training_step_vs_g27(g27, tag):
    state = R.model_state(*R.recipe(g27, "d256"))
    attn, lens, kw, cap, cap_len = R.train_inputs()
    use_cap = g27[f"d256_train_{tag}_use_cap"].tolist()
    assert (tag == "tf") == all(use_cap)
    o = R.train_step_grads(state, attn, lens, kw, cap, cap_len, use_cap, teacher_forcing=(tag == "tf"))
    top_val = o["logit"].gather(2, torch.from_numpy(g27[f"d256_train_{tag}_logit_top_idx"]).long())
    want = torch.from_numpy(g27[f"d256_train_{tag}_logit_top_val"]).double()
    assert float((top_val - want).abs().max()) / float(want.abs().max()) < 2e-5
    if tag == "ss":
        assert np.array_equal(o["seq"].numpy(), g27["d256_train_ss_seq"])
    loss = float(g27[f"d256_train_{tag}_loss"])
    assert abs(float(o["loss"]) - loss) < 2e-5 * loss
    keys = [k[len("d256_sample_idx/"):] for k in g27.files if k.startswith("d256_sample_idx/")]
    assert set(keys) == set(R.trainable_keys(state))
    assert {"decoder.keyword_proj.weight", "decoder.keyword_proj.bias", "decoder.word_keyword_norm.weight",
            "decoder.word_keyword_norm.bias", "decoder.word_embedding.weight"} <= set(keys)
    for key in keys:
        grad = o["grads"][key]
        gn = float(g27[f"d256_train_{tag}_gnorm/{key}"])
        assert abs(float(grad.norm()) - gn) < 1e-4 * (gn + 1e-12), key
        sample = grad.reshape(-1)[torch.from_numpy(g27[f"d256_sample_idx/{key}"])].numpy()
        assert np.abs(sample - g27[f"d256_train_{tag}_gsample/{key}"]).max() < 1e-4 * (float(grad.abs().max()) + 1e-12), key


# ---- names, order, compatibility ------------------------------------------------------------------------------------------
def test_state_dict_and_parameter_order_are_the_reference_s(g27):
    dec = _decoder("d256")
    sd = dec.state_dict()
    assert list(sd.keys()) == g27["state_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g27["state_shapes"].tolist()
    assert [k for k, _ in dec.named_parameters()] == g27["param_names"].tolist()
    assert list(sd.keys())[-4:] == ["keyword_proj.weight", "keyword_proj.bias", "word_keyword_norm.weight",
                                    "word_keyword_norm.bias"]
    # created after the base class's xavier pass, as in the reference: torch's defaults
    assert torch.equal(dec.word_keyword_norm.weight, torch.ones(256)) and not dec.word_keyword_norm.bias.any()
    bound = 1.0 / np.sqrt(dec.keyword_classes_num)
    assert float(dec.keyword_proj.weight.detach().abs().max()) <= bound
    dec.load_state_dict({k[len("decoder."):]: v for k, v in R.decoder_state("d256", *R.recipe(g27, "d256")).items()},
                        strict=True)


def test_compatible_decoders_both_ways():
    import audiocaption_amd as A
    dec = _decoder()
    model = A.KeywordCondTransformerModel(torch.nn.Identity(), dec)
    assert model.compatible_decoders == (A.KeywordProbTransformerDecoder,)
    assert model.train_forward_keys[-1] == "keyword" and model.inference_forward_keys[-1] == "keyword"
    assert isinstance(model, A.TransformerModel) and isinstance(dec, A.TransformerDecoder)
    with pytest.raises(AssertionError, match="KeywordProbTransformerDecoder is incompatible with TransformerModel"):
        A.TransformerModel(torch.nn.Identity(), dec)
    plain = A.TransformerDecoder(emb_dim=128, vocab_size=60, fc_emb_dim=64, attn_emb_dim=64, dropout=0.2, nhead=2)
    with pytest.raises(AssertionError, match="TransformerDecoder is incompatible with KeywordCondTransformerModel"):
        A.KeywordCondTransformerModel(torch.nn.Identity(), plain)
    A.TransformerModel(torch.nn.Identity(), plain)


def test_check_supported_adds_the_class_count():
    import audiocaption_amd as A
    _decoder().check_supported()
    with pytest.raises(A._lib.HipLibraryError, match="keyword_classes_num 0"):
        dec = _decoder()
        dec.keyword_classes_num = 0
        dec.check_supported()
    with pytest.raises(A._lib.HipLibraryError, match="emb_dim 96"):
        _decoder(emb_dim=96, nhead=1).check_supported()
    assert _decoder("d256").cluster_covers(3, 7, 6) is False


# ---- refusals and keyword checks, all before any launch ------------------------------------------------------------------
def test_keyword_checks():
    from audiocaption_amd.transformer_decoder import check_keyword
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        got = check_keyword(torch.ones(3, 30, dtype=dtype), 3, 30)
        assert got.dtype == torch.float32 and got.shape == (3, 30)
    assert check_keyword(np.ones((3, 30), dtype=np.float64), 3, 30).dtype == torch.float32
    with pytest.raises(KeyError, match="keyword"):
        check_keyword(None, 3, 30)
    for bad in (torch.ones(3, 29), torch.ones(2, 30), torch.ones(30), torch.ones(3, 30, 1), torch.ones(3, 30, dtype=torch.long)):
        with pytest.raises(ValueError, match="keyword"):
            check_keyword(bad, 3, 30)


def test_model_refusals():
    import audiocaption_amd as A
    dec = _decoder()
    model = A.KeywordCondTransformerModel(torch.nn.Identity(), dec).eval()
    attn, lens, kw = R.infer_inputs("d128")
    base = {"mode": "inference", "attn_emb": attn, "fc_emb": torch.zeros(R.B, 64), "attn_emb_len": lens}
    for method in ("greedy", "beam", "sample", "top5"):
        with pytest.raises(KeyError, match="keyword"):
            model(dict(base, sample_method=method))
        with pytest.raises(ValueError, match="keyword"):
            model(dict(base, sample_method=method, keyword=kw[:, :-1]))
        with pytest.raises(ValueError, match="keyword"):
            model(dict(base, sample_method=method, keyword=kw[:2]))
    with pytest.raises(KeyError, match="keyword"):
        model({"mode": "train", "attn_emb": attn})
    with pytest.raises(NotImplementedError, match="dbs"):
        model(dict(base, sample_method="dbs", keyword=kw))
    with pytest.raises(NotImplementedError, match="forward_async"):
        model.forward_async(dict(base, keyword=kw))
    with pytest.raises(NotImplementedError):
        model(dict(base, mode="train", keyword=kw))            # over another encoder than the training engine's
    with pytest.raises(NotImplementedError, match="keyword"):
        A.EnsembleModel([model, model])
    with pytest.raises(NotImplementedError, match="KeywordCondTransformerModel"):
        A.ScstWrapper(model)
    for wrapper in (A.MseEncoderKdWrapper, A.ContraEncoderKdWrapper, A.ContraMseEncoderKdWrapper):
        with pytest.raises(NotImplementedError, match="KeywordCondTransformerModel"):
            wrapper(model, 64, 64)
    with pytest.raises(NotImplementedError, match="whole-model training step"):
        dec.train()(dict(base, word=torch.ones(3, 1, dtype=torch.long), keyword=kw))
    with pytest.raises(NotImplementedError, match="one batch"):
        dec.eval().greedy([attn, attn], [lens, lens], 6, 1, 2, 0, keyword=kw)
    with pytest.raises(KeyError, match="keyword"):
        dec.greedy(attn, lens, 6, 1, 2, 0)


def test_training_engine_refusals():
    """The fused step (also with kd=) and the SCST rollout name the feature; the autograd route is the one that is built."""
    import audiocaption_amd as A
    from audiocaption_amd import build
    from audiocaption_amd.train import TrainEngine
    build.build()
    model = A.init_model_from_config(A.cnn14rnn_keyword_trm_config(61, 30), print_fn=lambda s: None).train()
    assert type(model) is A.KeywordCondTransformerModel and type(model.decoder) is A.KeywordProbTransformerDecoder
    eng = TrainEngine(model)
    assert eng.keyword
    with pytest.raises(NotImplementedError, match="keyword"):
        eng.step({}, None)
    with pytest.raises(NotImplementedError, match="keyword"):
        eng.step({}, None, kd={"tchr_logit": None, "temp": 1.0, "sup_weight": 0.5})
    with pytest.raises(NotImplementedError, match="keyword"):
        eng.rollout({})
    with pytest.raises(NotImplementedError, match="KeywordCondTransformerModel"):
        A.ScstWrapper(model)
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    assert names[-4:] == ["decoder.keyword_proj.weight", "decoder.keyword_proj.bias", "decoder.word_keyword_norm.weight",
                          "decoder.word_keyword_norm.bias"]
    from audiocaption_amd import procedural as P
    state = P.cnn14rnn_keyword_trm_state(61, 30)
    model.load_state_dict(P.to_torch(state), strict=True)      # (the mel front end's buffers are not persistent)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def _host_weights(d=128, nhead=2):
    from audiocaption_amd import _lib
    w = _lib.AcTrmWeights()
    w.d_model, w.nhead, w.nlayers, w.dim_ff, w.vocab, w.max_pos, w.attn_emb_dim = d, nhead, 2, 256, 60, 100, 64
    return w


def test_header_and_ctypes_rows_of_the_new_entry_points():
    from audiocaption_amd import _lib
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    assert re.search(r"#define AC_ABI_VERSION 2\b", header) and _lib.ABI_VERSION == 2
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ac_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body))
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in protos, name
        args = [a.strip() for a in protos[name].split(",")]
        res, want = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(want), name
        if name.startswith("ac_trm_kw_"):
            assert args[0].startswith("const ac_trm_weights*") and want[0] is _lib._WP
            assert args[1] == "const ac_trm_keyword* kw" and want[1] is ctypes.c_void_p
    m = re.search(r"typedef struct \{([^}]*)\} ac_trm_keyword;", body)
    fields = re.findall(r"(\w+);", m.group(1))
    assert fields == [f[0] for f in _lib.AcTrmKeyword._fields_] == ["kwp", "ln_w", "ln_b", "row_div"]
    assert ctypes.sizeof(_lib.AcTrmKeyword) == 32
    # ac_trm_weights keeps its layout
    assert ctypes.sizeof(_lib.AcTrmWeights) == 8 * 4 + 8 * 8 + _lib.AC_MAX_LAYERS * 18 * 8


def test_entry_points_refuse_null_and_misaligned_operands_without_a_gpu():
    """AC_ERR_ARG comes back before any launch: these calls run on a machine without a device."""
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    w = ctypes.byref(_host_weights())
    fake = 0x7f0000001000          # never dereferenced on the host
    good = _lib.AcTrmKeyword(fake, fake + 4096, fake + 8192, 1)
    cases = [None, _lib.AcTrmKeyword(0, fake, fake, 1), _lib.AcTrmKeyword(fake, 0, fake, 1), _lib.AcTrmKeyword(fake, fake, 0, 1),
             _lib.AcTrmKeyword(fake + 4, fake, fake, 1), _lib.AcTrmKeyword(fake, fake + 8, fake, 1),
             _lib.AcTrmKeyword(fake, fake, fake + 12, 1), _lib.AcTrmKeyword(fake, fake, fake, 2),
             good]                  # good: the other operands are null
    P = ctypes.c_void_p(fake)
    for kw in cases:
        k = None if kw is None else ctypes.byref(kw)
        null = kw is good
        a = None if null else P
        assert lib.ac_trm_kw_greedy_segments(w, k, a, a, 3, 1, 7, 6, 1, 2, 0, a, a, a, a, a, a, None) == _lib.AC_ERR_ARG
        assert lib.ac_trm_kw_sample(w, k, a, a, 3, 7, 6, 1, 2, 0, a, a, a, a, a, a, 0, 0, 0.0, 1.0, a, None) == _lib.AC_ERR_ARG
        assert lib.ac_trm_kw_forward_tokens(w, k, a, a, 3, 7, a, None, 6, a, a, a, None) == _lib.AC_ERR_ARG
        assert lib.ac_trm_kw_embed_qkv(w, k, 3, 1, 0, a, 7, a, a, None) == _lib.AC_ERR_ARG
    # the beam step reads row_div = beam
    assert lib.ac_trm_kw_beam_step(w, ctypes.byref(good), P, P, 3, 2, 7, 6, 0, 1.0, P, P, P, P, P, P, None) == _lib.AC_ERR_ARG
    assert lib.ac_trm_kw_beam_step(w, None, P, P, 3, 1, 7, 6, 0, 1.0, P, P, P, P, P, P, None) == _lib.AC_ERR_ARG
    assert lib.ac_trm_kw_beam_step(w, ctypes.byref(good), None, P, 3, 1, 7, 6, 0, 1.0, P, P, P, P, P, P, None) == _lib.AC_ERR_ARG
    # an unsupported decoder shape is refused as everywhere else
    bad = ctypes.byref(_host_weights(d=96, nhead=1))
    assert lib.ac_trm_kw_embed_qkv(bad, ctypes.byref(good), 3, 1, 0, P, 7, P, P, None) == _lib.AC_ERR_ARG
    # the training kernels: null operands, another width than 256, misaligned rows
    f = lambda *a: lib.ac_kw_embed_fwd(*a)      # noqa: E731
    args = [P, P, P, P, P, P, P, P, P, P, 0, 8, 256, 0.0, 21, 0.0, 22, None, 1e-5, None]
    for i in range(10):
        assert f(*(args[:i] + [None] + args[i + 1:])) == _lib.AC_ERR_ARG
    assert f(*(args[:12] + [128] + args[13:])) == _lib.AC_ERR_ARG
    assert f(*(args[:11] + [0] + args[12:])) == _lib.AC_ERR_ARG
    assert f(*([ctypes.c_void_p(fake + 4)] + args[1:])) == _lib.AC_ERR_ARG
    b = lambda *a: lib.ac_kw_embed_bwd(*a)      # noqa: E731
    args = [P, P, P, P, P, P, P, P, P, 8, 256, 0.0, 21, 0.0, 22, None, 1e-5, None]
    for i in range(9):
        assert b(*(args[:i] + [None] + args[i + 1:])) == _lib.AC_ERR_ARG
    assert b(*(args[:10] + [512] + args[11:])) == _lib.AC_ERR_ARG
    assert b(*([ctypes.c_void_p(fake + 8)] + args[1:])) == _lib.AC_ERR_ARG


# ---- construction through the reference's names ---------------------------------------------------------------------------
def test_routing_exports_and_compat_install():
    import importlib
    import sys
    import audiocaption_amd as A
    from audiocaption_amd import compat, config
    for name in ("KeywordProbTransformerDecoder", "KeywordCondTransformerModel", "cnn14rnn_keyword_trm_config"):
        assert name in A.__all__ and hasattr(A, name)
    assert compat.HOT_MODULES["captioning.models.transformer_decoder"] == "audiocaption_amd.transformer_decoder"
    assert compat.HOT_MODULES["captioning.models.transformer_model"] == "audiocaption_amd.transformer_model"
    yaml_shaped = config.cnn14rnn_keyword_trm_config(61, 30)
    assert yaml_shaped["type"] == "captioning.models.transformer_model.KeywordCondTransformerModel"
    assert yaml_shaped["decoder"]["type"] == "captioning.models.transformer_decoder.KeywordProbTransformerDecoder"
    assert yaml_shaped["decoder"]["args"]["keyword_classes_num"] == 30
    saved = {k: v for k, v in sys.modules.items() if k.startswith("captioning")}
    try:
        compat.install()
        assert importlib.import_module("captioning.models.transformer_model").KeywordCondTransformerModel \
            is A.KeywordCondTransformerModel
        assert importlib.import_module("captioning.models.transformer_decoder").KeywordProbTransformerDecoder \
            is A.KeywordProbTransformerDecoder

        def by_import(path):         # train_util.get_obj_from_str: a plain import of the dotted path, no alias table
            module, cls = path.rsplit(".", 1)
            return getattr(importlib.import_module(module), cls)
        plain_cls = config.get_cls_from_str
        config.get_cls_from_str = lambda s: by_import(s)
        try:
            model = config.init_model_from_config(yaml_shaped, print_fn=lambda s: None)
        finally:
            config.get_cls_from_str = plain_cls
    finally:
        for k in [k for k in sys.modules if k.startswith("captioning")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert type(model) is A.KeywordCondTransformerModel and type(model.decoder) is A.KeywordProbTransformerDecoder
    assert model.decoder.keyword_proj.weight.shape == (256, 30) and type(model.encoder) is A.CrnnEncoder
    assert type(config.init_model_from_config(yaml_shaped, print_fn=lambda s: None)) is A.KeywordCondTransformerModel
