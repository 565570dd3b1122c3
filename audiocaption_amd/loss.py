"""Label-smoothing cross entropy on the MI355X path.  Plugin-compatible with the reference class
``captioning.losses.loss.LabelSmoothingLoss`` (loss.py:40-74): same constructor, ``forward(output_dict)`` reading
``logit`` (N, T, V), ``tgt`` (N, T) and ``tgt_len`` (N,), reductions "mean" / "sum" / "none".

Forward and backward are the one-pass kernel of csrc/train.hip (log-sum-exp, smoothed target term and
``softmax - q`` per row); there is no PyTorch fallback.

``SpecificityLossWrapper`` (loss.py:195-219) adds the condition term of controllable captioning to a word loss: the mean
squared error between each caption's expected specificity under softmax(logit) and the requested ``conditions``.  That
term is the forward and backward kernels of csrc/spec_loss.hip behind one ``autograd.Function``.
"""
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, stream


def _launch(logit, tgt, tgt_len_dev, smoothing, inv_count, dlogit, gscale, gscale_dev):
    lib = _lib.load()
    N, T, V = logit.shape
    row_loss = torch.empty(N * T, device=logit.device, dtype=torch.float32)
    loss = torch.empty(1, device=logit.device, dtype=torch.float32)
    check(lib.ac_label_smoothing_loss(ptr(logit), ptr(tgt), tgt.stride(0), ptr(tgt_len_dev), N, T, V, float(smoothing),
                                      float(inv_count), ptr(row_loss), ptr(loss), ptr(dlogit), float(gscale),
                                      ptr(gscale_dev), stream()), "ac_label_smoothing_loss")
    return loss, row_loss


class _LabelSmoothingFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logit, tgt, tgt_len_dev, smoothing, inv_count, reduction):
        loss, row_loss = _launch(logit, tgt, tgt_len_dev, smoothing, inv_count, None, 0.0, None)
        ctx.save_for_backward(logit, tgt, tgt_len_dev)
        ctx.args = (smoothing, inv_count, reduction)
        if reduction == "none":
            return row_loss.view(logit.shape[0], logit.shape[1])
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        logit, tgt, tgt_len_dev = ctx.saved_tensors
        smoothing, inv_count, reduction = ctx.args
        if reduction == "none":
            raise NotImplementedError("LabelSmoothingLoss (HIP path): backward of reduction='none' is not built")
        dlogit = torch.empty_like(logit)
        g = grad_out.reshape(1).to(device=logit.device, dtype=torch.float32)
        _launch(logit, tgt, tgt_len_dev, smoothing, inv_count, dlogit, inv_count, g)
        return dlogit, None, None, None, None, None


class LabelSmoothingLoss(nn.Module):

    def __init__(self, smoothing=0.0, dim=-1, reduction="mean", logit_name="logit", target_name="tgt"):
        super().__init__()
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing
        if dim not in (-1, 2):
            raise NotImplementedError("LabelSmoothingLoss (HIP path): the class axis must be the last one")
        self.dim = dim
        self.reduction = reduction
        self.logit_name = logit_name
        self.target_name = target_name

    def forward(self, output):
        logit = output[self.logit_name]
        tgt = output[self.target_name]
        tgt_len = torch.as_tensor(output[f"{self.target_name}_len"])
        if logit.dim() != 3:
            raise ValueError("logit must be (batch, length, classes)")
        if logit.dtype != torch.float32 or not logit.is_contiguous():
            logit = logit.float().contiguous()
        dev = logit.device
        T = logit.shape[1]
        tgt = tgt.to(device=dev, dtype=torch.int64)
        if tgt.stride(1) != 1:
            tgt = tgt.contiguous()
        # generate_length_mask(tgt_len) (model_util.py:29-38) has max(tgt_len) columns: every row below T counts
        count = float(torch.clamp(tgt_len.cpu(), max=T).sum())
        inv_count = {"mean": 1.0 / count, "sum": 1.0, "none": 1.0}[self.reduction]
        tgt_len_dev = tgt_len.to(device=dev, dtype=torch.int32)
        return _LabelSmoothingFn.apply(logit, tgt, tgt_len_dev, self.smoothing, inv_count, self.reduction)


class _SpecificityFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logit, word_spec, tgt_len_dev, cond, mean_reduce):
        N, T, V = logit.shape
        f32 = dict(device=logit.device, dtype=torch.float32)
        row_s, row_lse = torch.empty(N * T, **f32), torch.empty(N * T, **f32)
        diff, loss = torch.empty(N, **f32), torch.empty(1, **f32)
        check(_lib.load().ac_specificity_loss(ptr(logit), ptr(word_spec), ptr(tgt_len_dev), ptr(cond), N, T, V, mean_reduce,
                                              ptr(row_s), ptr(row_lse), ptr(diff), ptr(loss), stream()),
              "ac_specificity_loss")
        ctx.save_for_backward(logit, word_spec, tgt_len_dev, row_s, row_lse, diff)
        ctx.mean_reduce = mean_reduce
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        logit, word_spec, tgt_len_dev, row_s, row_lse, diff = ctx.saved_tensors
        N, T, V = logit.shape
        dlogit = torch.empty_like(logit)
        g = grad_out.reshape(1).to(device=logit.device, dtype=torch.float32)
        check(_lib.load().ac_specificity_loss_bwd(ptr(logit), ptr(word_spec), ptr(tgt_len_dev), ptr(row_s), ptr(row_lse),
                                                  ptr(diff), ptr(g), N, T, V, ctx.mean_reduce, ptr(dlogit), stream()),
              "ac_specificity_loss_bwd")
        return dlogit, None, None, None, None


class SpecificityLossWrapper(nn.Module):
    """``loss_fn(output) + alpha * MSE(caption specificity, output["conditions"])``; returns (loss, word_loss,
    condition_loss) as the reference does.  The caption specificity is the sum (``sentence_reduce="sum"``) or, for any other
    value, the ``mean_with_lens`` over the positions t < tgt_len - 1 of sum_v softmax(logit)_v * word_specificity[v]."""

    def __init__(self, loss_fn, word_specificity, sentence_reduce="sum", alpha=1):
        super().__init__()
        self.loss_fn = loss_fn
        self.word_specificity = word_specificity   # [vocab_size]
        self.alpha = alpha
        self.sentence_reduce = sentence_reduce

    def forward(self, output):
        word_loss = self.loss_fn(output)
        logit = output["logit"]
        if logit.dim() != 3:
            raise ValueError("logit must be (batch, length, classes)")
        if logit.dtype != torch.float32 or not logit.is_contiguous():
            logit = logit.float().contiguous()
        N, T, V = logit.shape
        dev = logit.device
        ws = torch.as_tensor(self.word_specificity)
        if ws.dim() != 1 or ws.numel() != V:
            raise ValueError(f"word_specificity holds {ws.numel()} values for a vocabulary of {V}")
        tgt_len = torch.as_tensor(output["tgt_len"]).detach().cpu().reshape(-1)
        cond = torch.as_tensor(output["conditions"]).detach()
        if tgt_len.numel() != N or cond.numel() != N:
            raise ValueError(f"tgt_len ({tgt_len.numel()}) and conditions ({cond.numel()}) must hold one value per clip ({N})")
        mean_reduce = int(self.sentence_reduce != "sum")
        if mean_reduce and int(tgt_len.min()) < 2:
            raise ValueError(f"sentence_reduce={self.sentence_reduce!r} divides by tgt_len - 1: every tgt_len must be at least "
                             f"2 (got {tgt_len.tolist()})")
        condition_loss = _SpecificityFn.apply(
            logit, ws.detach().to(device=dev, dtype=torch.float32).contiguous(), tgt_len.to(device=dev, dtype=torch.int32),
            cond.reshape(N).to(device=dev, dtype=torch.float32).contiguous(), mean_reduce)
        loss = word_loss + self.alpha * condition_loss
        return loss, word_loss, condition_loss
