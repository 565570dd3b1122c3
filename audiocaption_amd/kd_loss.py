"""Token-level knowledge distillation on the MI355X path.  Plugin-compatible with the reference classes
``captioning.losses.kd_loss.TokenLevelKdLoss`` and ``SupKdLoss`` (kd_loss.py:8-49): same constructors, ``forward(output)``
reading ``logit`` / ``tchr_logit`` (N, T, V), ``tgt`` (N, T) and ``tgt_len`` (N,).

``TokenLevelKdLoss`` is the cross entropy of the student's ``softmax(logit / temp)`` against the frozen teacher's
``softmax(tchr_logit / temp)``, averaged over the valid target tokens (not scaled by ``temp ** 2``, as the reference);
``SupKdLoss`` weighs it against a supervised loss.  Forward and backward are the one-pass kernel of csrc/kd.hip
(``ac_kd_loss``); the pair ``SupKdLoss(LabelSmoothingLoss(reduction="mean"), TokenLevelKdLoss("kl"))`` is ONE launch each
way.  There is no PyTorch fallback; the teacher's logits get no gradient.
"""
import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, stream
from .loss import LabelSmoothingLoss


def _launch(logit, tchr_logit, tgt, tgt_len_dev, smoothing, temp, sup_weight, inv_count, dlogit, gscale, gscale_dev):
    """One ``ac_kd_loss`` call: returns (loss [3] = total, sup, kd; row_sup [N*T]; row_kd [N*T])."""
    lib = _lib.load()
    N, T, V = logit.shape
    row_sup = torch.empty(N * T, device=logit.device, dtype=torch.float32)
    row_kd = torch.empty(N * T, device=logit.device, dtype=torch.float32)
    loss = torch.empty(3, device=logit.device, dtype=torch.float32)
    check(lib.ac_kd_loss(ptr(logit), ptr(tchr_logit), ptr(tgt), tgt.stride(0), ptr(tgt_len_dev), N, T, V, float(smoothing),
                         float(temp), float(sup_weight), float(inv_count), ptr(row_sup), ptr(row_kd), ptr(loss), ptr(dlogit),
                         float(gscale), ptr(gscale_dev), stream()), "ac_kd_loss")
    return loss, row_sup, row_kd


class _KdLossFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logit, tchr_logit, tgt, tgt_len_dev, smoothing, temp, sup_weight, inv_count):
        loss, _, _ = _launch(logit, tchr_logit, tgt, tgt_len_dev, smoothing, temp, sup_weight, inv_count, None, 0.0, None)
        ctx.save_for_backward(logit, tchr_logit, tgt, tgt_len_dev)
        ctx.args = (smoothing, temp, sup_weight, inv_count)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        logit, tchr_logit, tgt, tgt_len_dev = ctx.saved_tensors
        smoothing, temp, sup_weight, inv_count = ctx.args
        dlogit = torch.empty_like(logit)
        g = grad_out.reshape(1).to(device=logit.device, dtype=torch.float32)
        _launch(logit, tchr_logit, tgt, tgt_len_dev, smoothing, temp, sup_weight, inv_count, dlogit, inv_count, g)
        return dlogit, None, None, None, None, None, None, None


def _inputs(output, logit_name="logit", target_name="tgt"):
    """``logit``, ``tchr_logit``, ``tgt``, ``tgt_len`` of ``output`` as the kernel takes them, converted as
    ``LabelSmoothingLoss`` converts its own, and 1 / (valid target tokens)."""
    logit, tchr = output[logit_name], output["tchr_logit"]
    tgt = output[target_name]
    tgt_len = torch.as_tensor(output[f"{target_name}_len"])
    if logit.dim() != 3:
        raise ValueError("logit must be (batch, length, classes)")
    if tuple(tchr.shape) != tuple(logit.shape):
        raise ValueError(f"tchr_logit {tuple(tchr.shape)} and logit {tuple(logit.shape)} differ in shape")
    if logit.dtype != torch.float32 or not logit.is_contiguous():
        logit = logit.float().contiguous()
    dev = logit.device
    tchr = tchr.detach().to(device=dev)
    if tchr.dtype != torch.float32 or not tchr.is_contiguous():
        tchr = tchr.float().contiguous()
    T = logit.shape[1]
    tgt = tgt.to(device=dev, dtype=torch.int64)
    if tgt.stride(1) != 1:
        tgt = tgt.contiguous()
    # generate_length_mask(tgt_len) (model_util.py:29-38) has max(tgt_len) columns: every row below T counts
    count = float(torch.clamp(tgt_len.cpu(), max=T).sum())
    if not count > 0:
        raise ValueError("tgt_len holds no valid target token: the mean over the valid tokens is undefined")
    return logit, tchr, tgt, tgt_len.to(device=dev, dtype=torch.int32), 1.0 / count


class TokenLevelKdLoss(nn.Module):

    def __init__(self, temp=1.0, loss_type="kl"):
        super().__init__()
        if loss_type in ("l2", "l1"):
            raise NotImplementedError(
                f"TokenLevelKdLoss (HIP path): loss_type={loss_type!r} is not built; the reference fails there too "
                "(kd_loss.py:30 reshapes the (N*T, V) element-wise loss to tgt's (N, T) shape)")
        if loss_type != "kl":
            raise ValueError(f"TokenLevelKdLoss: unknown loss_type {loss_type!r}")
        if not (math.isfinite(float(temp)) and float(temp) > 0):
            raise ValueError(f"TokenLevelKdLoss: temp must be finite and > 0, got {temp}")
        self.temp = temp
        self.loss_type = loss_type

    def forward(self, output):
        logit, tchr, tgt, tgt_len_dev, inv_count = _inputs(output)
        return _KdLossFn.apply(logit, tchr, tgt, tgt_len_dev, 0.0, float(self.temp), 0.0, inv_count)


class SupKdLoss(nn.Module):

    def __init__(self, sup_loss, kd_loss, sup_weight=0.5):
        super().__init__()
        self.sup_loss = sup_loss
        self.kd_loss = kd_loss
        self.sup_weight = sup_weight

    def fused(self):
        """True when the pair is the one ``ac_kd_loss`` covers in a single launch."""
        s, k = self.sup_loss, self.kd_loss
        return (type(s) is LabelSmoothingLoss and s.reduction == "mean" and s.logit_name == "logit" and
                s.target_name == "tgt" and type(k) is TokenLevelKdLoss and 0.0 <= float(self.sup_weight) <= 1.0)

    def forward(self, output):
        if self.fused():
            logit, tchr, tgt, tgt_len_dev, inv_count = _inputs(output)
            return _KdLossFn.apply(logit, tchr, tgt, tgt_len_dev, float(self.sup_loss.smoothing), float(self.kd_loss.temp),
                                   float(self.sup_weight), inv_count)
        # any other pair: composed as the reference composes it (kd_loss.py:45-48)
        sup_loss = self.sup_loss(output)
        kd_loss = self.kd_loss(output)
        return sup_loss * self.sup_weight + kd_loss * (1 - self.sup_weight)
