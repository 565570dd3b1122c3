"""CPU tests of encoder-level knowledge distillation: the float64 restatement (tests/_enc_kd_ref.py) and the CPU route of
``enc_kd.enc_kd_loss`` against what the reference's own ``kd_wrapper`` classes computed (tests/golden/g24_enc_kd.npz), the
wrappers' constructors, state-dict keys and refusals, the routing of the reference's class paths, and the plumbing of the
new entry point (header, ctypes row, build list)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import _enc_kd_ref as E

GRADS = ["fc_emb", "stdnt_proj.weight", "stdnt_proj.bias", "tchr_proj.weight", "tchr_proj.bias", "logit_scale"]
WEIGHTS = ["stdnt_proj.weight", "stdnt_proj.bias", "tchr_proj.weight", "tchr_proj.bias"]


@pytest.fixture(scope="module")
def g24(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g24_enc_kd.npz")))


def _cases():
    return [(b, k) for b in ("b5", "b1") for k in E.KINDS]


def test_restatement_vs_reference_fixture(g24):
    w = [torch.from_numpy(g24[k]) for k in WEIGHTS]
    assert g24["b5/fc_emb"].shape == (5, 24) and g24["b5/tchr_emb"].shape == (5, 12) and g24["b1/fc_emb"].shape == (1, 24)
    assert g24["stdnt_proj.weight"].shape == (16, 24) and g24["tchr_proj.weight"].shape == (16, 12)
    assert float(g24["logit_scale"]) == float(torch.ones([]) * np.log(1 / 0.07))
    for b, kind in _cases():
        got = E.full(torch.from_numpy(g24[f"{b}/fc_emb"]), torch.from_numpy(g24[f"{b}/tchr_emb"]), *w,
                     float(g24["logit_scale"]), E.KINDS[kind])
        want = float(g24[f"{b}/{kind}/loss"])
        assert abs(float(got["loss"]) - want) <= 1e-12 * max(abs(want), 1.0), (b, kind)
        if b == "b1" and kind == "contra":
            assert want == 0.0 and float(got["loss"]) == 0.0       # one clip: nothing to contrast
        for k in GRADS:
            key = f"{b}/{kind}/d/{k}"
            assert (key in g24) == (k != "logit_scale" or "contra" in kind)
            if key in g24:
                ref = torch.from_numpy(g24[key])
                assert float((got[k] - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-300), key


def test_restatement_gradient_is_the_derivative_of_its_loss():
    """The closed form against autograd over the reference's expression, in float64 - with a row below the clamp."""
    g = torch.Generator().manual_seed(5)
    s, t = torch.randn(6, 10, generator=g).double(), torch.randn(6, 10, generator=g).double()
    s[2] = 0.0
    for kind, bits in E.KINDS.items():
        for scale in (2.5, 100.0):
            a, b = s.clone().requires_grad_(True), t.clone().requires_grad_(True)
            sc = torch.tensor(scale, dtype=torch.float64, requires_grad=True)
            loss = E.torch_loss(a, b, sc, bits)
            loss.backward()
            got = E.head(s, t, scale, bits)
            assert abs(float(got["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
            for name, x, ref in (("ds", got["ds"], a.grad), ("dt", got["dt"], b.grad)):
                assert float((x - ref).abs().max()) <= 1e-11 * float(ref.abs().max()), (kind, scale, name)
            if bits & E.CONTRA:
                assert abs(float(got["dscale"]) - float(sc.grad)) <= 1e-11 * max(abs(float(sc.grad)), 1e-3)
            assert torch.isfinite(got["ds"]).all()
            if bits != E.MSE:
                assert float(got["ds"][2].abs().max()) > 1e6     # dy / 1e-12


def _stub(fc=24):
    class Enc(nn.Module):
        fc_emb_size = fc

        def forward(self, d):
            return {"fc_emb": d["feat"], "from": "encoder"}

    class Cap(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = Enc()

        def forward(self, d):
            return {"fc_emb": d["feat"], "from": "model"}
    return Cap()


def _wrapper(kind):
    from audiocaption_amd import kd_wrapper as W
    return {"contra": lambda: W.ContraEncoderKdWrapper(_stub(), 16, 12),
            "mse": lambda: W.MseEncoderKdWrapper(_stub(), 16, 12),
            "mse_l2": lambda: W.MseEncoderKdWrapper(_stub(), 16, 12, l2_norm=True),
            "contra_mse": lambda: W.ContraMseEncoderKdWrapper(_stub(), 16, 12),
            "contra_mse_l2": lambda: W.ContraMseEncoderKdWrapper(_stub(), 16, 12, l2_norm=True)}[kind]()


def test_cpu_route_of_the_wrappers_vs_reference_fixture(g24):
    """float32 torch on the CPU against the reference's float64: 1e-5 of each tensor's maximum, 2e-5 on the loss."""
    for b, kind in _cases():
        w = _wrapper(kind)
        with torch.no_grad():
            for k in WEIGHTS:
                dict(w.named_parameters())[k].copy_(torch.from_numpy(g24[k]))
        feat = torch.from_numpy(g24[f"{b}/fc_emb"]).clone().requires_grad_(True)
        out = w({"feat": feat, "mode": "inference", "tchr_output": {"embedding": torch.from_numpy(g24[f"{b}/tchr_emb"])}})
        assert out["from"] == "model"
        want = float(g24[f"{b}/{kind}/loss"])
        assert abs(float(out["enc_kd_loss"]) - want) <= 2e-5 * max(abs(want), 1e-3), (b, kind)
        if want == 0.0:
            continue
        out["enc_kd_loss"].backward()
        got = {"fc_emb": feat.grad, **{k: p.grad for k, p in w.named_parameters()}}
        for k in GRADS:
            key = f"{b}/{kind}/d/{k}"
            if key in g24:
                ref = torch.from_numpy(g24[key])
                assert float((got[k].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), key


def test_wrapper_signatures_state_dict_keys_and_refusals():
    from audiocaption_amd import hf_wrapper, kd_wrapper as W
    assert hf_wrapper.ContraEncoderKdWrapper is W.ContraEncoderKdWrapper
    sig = {c: list(inspect.signature(getattr(W, c).__init__).parameters) for c in (
        "MseEncoderKdWrapper", "ContraEncoderKdWrapper", "ContraMseEncoderKdWrapper", "WmlEncoderKdWrapper")}
    assert sig["MseEncoderKdWrapper"] == ["self", "model", "shared_dim", "tchr_dim", "use_tchr_proj", "l2_norm"]
    assert sig["ContraMseEncoderKdWrapper"] == sig["MseEncoderKdWrapper"]
    assert sig["ContraEncoderKdWrapper"] == ["self", "model", "shared_dim", "tchr_dim"]
    assert sig["WmlEncoderKdWrapper"] == ["self", "model", "shared_dim", "tchr_layer_to_dims", "loss_type"]
    d = inspect.signature(W.MseEncoderKdWrapper.__init__).parameters
    assert d["use_tchr_proj"].default is True and d["l2_norm"].default is False
    heads = ["stdnt_proj.weight", "stdnt_proj.bias", "tchr_proj.weight", "tchr_proj.bias"]
    assert sorted(_wrapper("mse").state_dict()) == sorted(heads)
    assert sorted(_wrapper("contra").state_dict()) == sorted(heads + ["logit_scale"])
    assert sorted(_wrapper("contra_mse_l2").state_dict()) == sorted(heads + ["logit_scale"])
    w = _wrapper("contra_mse")
    assert w.stdnt_proj.weight.shape == (16, 24) and w.tchr_proj.weight.shape == (16, 12) and w.tchr_dim == 12
    assert abs(float(w.logit_scale) - np.log(1 / 0.07)) < 1e-6 and float(w.stdnt_proj.bias.abs().max()) == 0.0
    assert _wrapper("mse_l2").l2_norm is True and _wrapper("mse").l2_norm is False
    with pytest.raises(NotImplementedError, match="use_tchr_proj"):
        W.MseEncoderKdWrapper(_stub(16), 16, 16, use_tchr_proj=False)
    with pytest.raises(NotImplementedError, match="use_tchr_proj"):
        W.ContraMseEncoderKdWrapper(_stub(16), 16, 16, use_tchr_proj=False)
    with pytest.raises(NotImplementedError, match="WmlEncoderKdWrapper"):
        W.WmlEncoderKdWrapper(_stub(), 16, {"a": 12})
    # a captioner without a training engine: mode "train" is refused for every kind, unsup and inference are head-only
    feat, tchr = torch.randn(3, 24), torch.randn(3, 12)
    for kind in E.KINDS:
        w = _wrapper(kind)
        with pytest.raises(NotImplementedError, match="head-only"):
            w({"feat": feat, "mode": "train", "tchr_output": {"embedding": tchr}})
        out = w({"feat": feat, "mode": "train", "unsup": True, "tchr_output": {"embedding": tchr}})
        assert out["from"] == "encoder" and out["enc_kd_loss"].requires_grad
        assert "enc_kd_loss" not in w({"feat": feat, "mode": "inference"})


def test_enc_kd_loss_arguments():
    from audiocaption_amd.enc_kd import enc_kd_loss, kind_bits
    assert kind_bits("contra", True) == 1 and kind_bits("mse", True) == 6 and kind_bits("contra_mse") == 3
    lin_s, lin_t = nn.Linear(24, 16), nn.Linear(12, 16)
    with pytest.raises(ValueError, match="kind"):
        enc_kd_loss(torch.randn(2, 24), torch.randn(2, 12), lin_s, lin_t, None, "wml")
    with pytest.raises(ValueError, match="logit_scale"):
        enc_kd_loss(torch.randn(2, 24), torch.randn(2, 12), lin_s, lin_t, None, "contra")


def test_compat_resolves_the_reference_class_paths():
    import importlib
    from audiocaption_amd import compat, kd_wrapper as W
    assert compat.HOT_MODULES["captioning.models.kd_wrapper"] == "audiocaption_amd.kd_wrapper"
    compat.install()
    mod = importlib.import_module("captioning.models.kd_wrapper")
    for c in ("MseEncoderKdWrapper", "ContraEncoderKdWrapper", "ContraMseEncoderKdWrapper", "WmlEncoderKdWrapper"):
        assert getattr(mod, c) is getattr(W, c)


def test_header_ctypes_row_and_build_list():
    import ctypes
    from audiocaption_amd import _lib, build
    assert "enc_kd.hip" in build.SOURCES and _lib.ABI_VERSION == 2
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "audiocaption_hip.h")).read()
    assert re.search(r"#define AC_ABI_VERSION 2\b", header)
    assert re.search(r"^int ac_enc_kd_loss\(", header, re.M) and re.search(r"^long ac_enc_kd_workspace_floats\(", header, re.M)
    for name, val in (("CONTRA", 1), ("MSE", 2), ("L2NORM", 4)):
        assert re.search(rf"#define AC_ENC_KD_{name} {val}\b", header)
    res, args = _lib.SIGNATURES["ac_enc_kd_loss"]
    assert res is ctypes.c_int and len(args) == 16 and args[12] is ctypes.c_float and args[4:7] == [ctypes.c_int] * 3
    assert args[1] is ctypes.c_long and args[3] is ctypes.c_long
    assert _lib.SIGNATURES["ac_enc_kd_workspace_floats"] == (ctypes.c_long, [ctypes.c_int, ctypes.c_int])


def test_composite_encoders_carry_fc_emb_size():
    from audiocaption_amd.crnn_trm_encoder import Cnn14TransformerEncoder, CrnnEncoder
    from audiocaption_amd.rnn_encoder import RnnEncoder
    from audiocaption_amd.transformer_encoder import TransformerEncoder
    cnn = nn.Identity()
    rnn = RnnEncoder(-1, 2048, 2048, bidirectional=True, hidden_size=256, dropout=0.5, num_layers=3)
    assert CrnnEncoder(cnn, rnn).fc_emb_size == 512
    assert Cnn14TransformerEncoder(cnn, TransformerEncoder(-1, 2048, 2048, 256)).fc_emb_size == 256
