"""The reference's encoder-distillation wrappers on the MI355X path (``captioning.models.kd_wrapper``,
kd_wrapper.py:56-226; ``ContraEncoderKdWrapper`` is also hf_wrapper.py:1071-1112): a captioner plus the heads that project
its clip embedding ``fc_emb`` and a teacher's embedding into a shared space, and with ``tchr_output`` in the input dict the
loss between the two as ``enc_kd_loss`` (``enc_kd.enc_kd_loss``: one autograd node over the HIP head of csrc/enc_kd.hip).

Same constructor keywords and state-dict keys as the reference (``model.*``, ``stdnt_proj.*``, ``tchr_proj.*``, and
``logit_scale`` for the contrastive kinds).

* ``mode="train"`` distils INTO the encoder: the training forward of ``TransformerModel`` / ``Seq2SeqAttnModel`` over a
  ``CrnnEncoder`` or ``Cnn14TransformerEncoder`` returns ``fc_emb`` behind the engine's bridge node (train.py), so
  ``loss = loss_fn(output) + w * output["enc_kd_loss"]`` trains encoder, decoder, heads and ``logit_scale`` together.  A
  captioner without such an engine (the EfficientNet-B2 one, any foreign module) is refused: the loss would silently train
  nothing but the heads.
* ``mode="inference"`` or ``unsup=True``: the loss is head-only (``fc_emb`` comes out of the inference encoder detached).

``fc_emb_size`` is read from ``model.encoder`` (or ``model``), as the reference does.  This package's composite encoders
(``CrnnEncoder``, ``Cnn14TransformerEncoder``) define it - an extension: the reference's composites lack the attribute, so
its wrappers can only be constructed over encoders that define it themselves.

Not built (``NotImplementedError``): ``use_tchr_proj=False`` (it projects ``attn_emb`` as well and feeds the decoder the
projected embeddings) and ``WmlEncoderKdWrapper``.
"""
import numpy as np
import torch
import torch.nn as nn

from .enc_kd import enc_kd_loss
from .transformer_model import CaptionMetaMixin


def _trains_encoder(model):
    """Whether ``model(input_dict)`` with mode "train" returns an ``fc_emb`` that carries the encoder's gradient."""
    from .attn_model import Seq2SeqAttnModel
    from .crnn_trm_encoder import Cnn14TransformerEncoder, CrnnEncoder
    from .transformer_model import TransformerModel
    enc = getattr(model, "encoder", None)
    if isinstance(model, Seq2SeqAttnModel):
        return isinstance(enc, CrnnEncoder) and enc.freeze_cnn_bn
    if isinstance(model, TransformerModel):
        return isinstance(enc, (CrnnEncoder, Cnn14TransformerEncoder)) and enc.freeze_cnn_bn
    return False


def _ref_init(linear):
    """model_util.py:86-108 on an nn.Linear (what the reference applies to the heads)."""
    nn.init.kaiming_uniform_(linear.weight)
    nn.init.constant_(linear.bias, 0)


class _EncoderKdWrapper(nn.Module, CaptionMetaMixin):
    kind = None            # enc_kd.KINDS
    has_scale = False

    def _build(self, model, shared_dim, tchr_dim, use_tchr_proj=True, l2_norm=False, ref_init=True):
        if not use_tchr_proj:
            raise NotImplementedError(f"{type(self).__name__}: use_tchr_proj=False (the student's projection applied to "
                                      "attn_emb as well and fed to the decoder, kd_wrapper.py:91-96) is not built")
        from .transformer_model import KeywordCondTransformerModel
        if isinstance(model, KeywordCondTransformerModel):
            raise NotImplementedError(f"{type(self).__name__}: encoder knowledge distillation is not built for "
                                      "KeywordCondTransformerModel (keyword conditioning)")
        self.model = model
        self.use_tchr_proj = use_tchr_proj
        self.tchr_dim = tchr_dim
        self.l2_norm = l2_norm
        fc = model.encoder.fc_emb_size if hasattr(model, "encoder") else model.fc_emb_size
        self.stdnt_proj = nn.Linear(fc, shared_dim)
        self.tchr_proj = nn.Linear(tchr_dim, shared_dim)
        if ref_init:
            _ref_init(self.stdnt_proj)
            _ref_init(self.tchr_proj)
        if self.has_scale:
            self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))

    def forward(self, input_dict):
        unsup = input_dict.get("unsup", False)
        kd = "tchr_output" in input_dict
        if kd and input_dict.get("mode") == "train" and not unsup:
            from .cnn_encoder import Cnn14Encoder
            cnn = getattr(getattr(self.model, "encoder", None), "cnn", None)
            if cnn is not None and not isinstance(cnn, Cnn14Encoder):
                raise NotImplementedError(f"{type(self).__name__}: encoder knowledge distillation in mode='train' runs on the "
                                          f"training engines, which are built around Cnn14Encoder; training over "
                                          f"{type(cnn).__name__} is not built.  Use mode='inference' (or unsup=True) for a "
                                          f"head-only loss")
        if kd and input_dict.get("mode") == "train" and not unsup and not _trains_encoder(self.model):
            raise NotImplementedError(
                f"{type(self).__name__}: encoder knowledge distillation in mode='train' needs the gradient of enc_kd_loss "
                "with respect to the encoder (kd_wrapper.py:85-111 on top of base.py:133), which the training engines give "
                "for TransformerModel / Seq2SeqAttnModel over a CrnnEncoder or Cnn14TransformerEncoder with a frozen Cnn14; "
                f"{type(self.model).__name__} over {type(getattr(self.model, 'encoder', None)).__name__} has no such "
                "engine.  Use mode='inference' (or unsup=True) for a head-only loss")
        out = self.model.encoder(input_dict) if unsup else self.model(input_dict)
        if kd:
            out["enc_kd_loss"] = enc_kd_loss(out["fc_emb"], input_dict["tchr_output"]["embedding"], self.stdnt_proj,
                                             self.tchr_proj, self.logit_scale if self.has_scale else None, self.kind,
                                             self.l2_norm)
        return out


class MseEncoderKdWrapper(_EncoderKdWrapper):
    """kd_wrapper.py:56-111: ``F.mse_loss`` of the two projected embeddings (normalised first with ``l2_norm``)."""
    kind = "mse"

    def __init__(self, model, shared_dim, tchr_dim, use_tchr_proj=True, l2_norm=False):
        super().__init__()
        self._build(model, shared_dim, tchr_dim, use_tchr_proj, l2_norm)


class ContraEncoderKdWrapper(_EncoderKdWrapper):
    """kd_wrapper.py:114-157 / hf_wrapper.py:1071-1112: the symmetric contrastive (CLIP-style) loss between the projected clip
    embedding and the teacher's, with the learnt ``logit_scale`` (initialised to log(1 / 0.07), used as it is).  Its heads
    are in the published ``wsntxxn/effb2-trm-audio-captioning`` state dict; they keep nn.Linear's own initialisation here."""
    kind = "contra"
    has_scale = True

    def __init__(self, model, shared_dim, tchr_dim):
        super().__init__()
        self._build(model, shared_dim, tchr_dim, ref_init=False)


class ContraMseEncoderKdWrapper(_EncoderKdWrapper):
    """kd_wrapper.py:160-226: the sum of the two."""
    kind = "contra_mse"
    has_scale = True

    def __init__(self, model, shared_dim, tchr_dim, use_tchr_proj=True, l2_norm=False):
        super().__init__()
        self._build(model, shared_dim, tchr_dim, use_tchr_proj, l2_norm)


class WmlEncoderKdWrapper(nn.Module, CaptionMetaMixin):
    """kd_wrapper.py:13-53 (attention-weighted multi-layer distillation): not built."""

    def __init__(self, model, shared_dim, tchr_layer_to_dims, loss_type="mse"):
        super().__init__()
        raise NotImplementedError("WmlEncoderKdWrapper (kd_wrapper.py:13-53) is not built on the HIP path; the encoder "
                                  "distillation wrappers here are Mse / Contra / ContraMse")
