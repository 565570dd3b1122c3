"""Encoder-level knowledge distillation on the MI355X path: the loss of kd_wrapper.py:56-226 (``MseEncoderKdWrapper``,
``ContraEncoderKdWrapper``, ``ContraMseEncoderKdWrapper``; hf_wrapper.py:1095-1111) between a student's clip embedding
``fc_emb`` and a teacher's embedding, as ONE autograd node.

    s = stdnt_proj(fc_emb), t = tchr_proj(tchr_emb)            two ``ac_gemm`` (exact f32), bias in the epilogue
    loss, ds, dt, d logit_scale = ac_enc_kd_loss(s, t, ...)    csrc/enc_kd.hip: four launches, forward AND backward
    backward: dW = d^T x (``ac_gemm``), db = column sums (``ac_colsum``), d fc_emb = ds W_s (``ac_gemm``)

The head's gradients are computed with the loss (the head is a handful of latency-bound launches; a second visit would
double them) and kept; the node's backward scales them by the upstream gradient and runs the projections' backward.
``fc_emb`` may come from the training engines' bridge node (train.py), which is how the loss reaches the encoder.  The
teacher's embedding gets no gradient.

On CPU tensors the same loss is the torch expression (no device, no kernel): the wrappers' head-only use in host tests.
"""
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, f32c, ptr

CONTRA, MSE, L2NORM = 1, 2, 4      # include/audiocaption_hip.h AC_ENC_KD_*
KINDS = {"contra": CONTRA, "mse": MSE, "contra_mse": CONTRA | MSE}
MAX_B, MAX_D = 512, 4096


def kind_bits(kind, l2_norm=False):
    if kind not in KINDS:
        raise ValueError(f"enc_kd_loss: kind {kind!r}; one of {sorted(KINDS)}")
    return KINDS[kind] | (L2NORM if (l2_norm and KINDS[kind] & MSE) else 0)


def torch_enc_kd_loss(s, t, logit_scale, bits):
    """The reference's expression on projected embeddings (any device or dtype torch handles)."""
    loss = None
    if bits & MSE:
        a, b = (F.normalize(s, dim=-1), F.normalize(t, dim=-1)) if bits & L2NORM else (s, t)
        loss = F.mse_loss(a, b)
    if bits & CONTRA:
        # CLIP-style loss: cosine similarities of every (student clip, teacher clip) pair, scaled, matched on the diagonal
        sim = logit_scale * (F.normalize(s, dim=-1) @ F.normalize(t, dim=-1).t())
        target = torch.arange(sim.shape[0], device=sim.device)
        contra = 0.5 * (F.cross_entropy(sim, target) + F.cross_entropy(sim.t(), target))
        loss = contra if loss is None else loss + contra
    return loss


def head(s, t, logit_scale, bits, grads=True, gscale=1.0, gscale_dev=None):
    """``ac_enc_kd_loss`` on device tensors: s (B, D) / t (B, D) f32 with unit column stride (rows may be strided),
    ``logit_scale`` a one-element f32 device tensor (None without CONTRA).  Returns (loss[3] = total, contrastive, MSE;
    ds, dt, dscale, flat) - the gradients views of the one buffer ``flat`` = ds | dt | dscale; all None unless ``grads``."""
    lib = _lib.load()
    B, D = s.shape
    if tuple(t.shape) != (B, D):
        raise ValueError(f"enc_kd head: student {tuple(s.shape)} and teacher {tuple(t.shape)} embeddings differ in shape")
    n = lib.ac_enc_kd_workspace_floats(B, D)
    if n < 0:
        raise ValueError(f"enc_kd head: batch {B} (1..{MAX_B}) / width {D} (1..{MAX_D}) out of range")
    if s.stride(1) != 1 or t.stride(1) != 1:
        raise ValueError("enc_kd head: embeddings must have unit column stride")
    f32 = dict(device=s.device, dtype=torch.float32)
    ws = torch.empty(n, **f32)
    loss = torch.empty(3, **f32)
    g = torch.empty(2 * B * D + 1, **f32) if grads else None      # ds | dt | dscale: one buffer, scaled in one go
    ds = g[:B * D].view(B, D) if grads else None
    dt = g[B * D:2 * B * D].view(B, D) if grads else None
    dscale = g[2 * B * D:] if grads else None
    check(lib.ac_enc_kd_loss(ptr(s), s.stride(0), ptr(t), t.stride(0), B, D, bits, ptr(logit_scale), ptr(loss), ptr(ds),
                             ptr(dt), ptr(dscale), float(gscale), ptr(gscale_dev), ptr(ws), _lib.stream()), "ac_enc_kd_loss")
    return loss, ds, dt, dscale, g


def _gemm(lib, s, A, sam, sak, Bm, sbk, sbn, C, M, N, K, bias=None):
    check(lib.ac_gemm(ptr(A), sam, sak, ptr(Bm), sbk, sbn, ptr(C), N, M, N, K, ptr(bias), 0, 0.0, 1, 0.0, 0, None, 0, None, 0,
                      s), "ac_gemm")


def _linear_fwd(lib, s, x, W, b):
    """y = x W^T + b; x (M, K), W (N, K), all contiguous f32."""
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    _gemm(lib, s, x, K, 1, W, 1, K, y, M, N, K, b)
    return y


def _linear_bwd(lib, s, dy, x, W, need_x, need_w, need_b):
    """(dx, dW, db) of y = x W^T + b given dy (M, N)."""
    M, K = x.shape
    N = W.shape[0]
    f32 = dict(device=x.device, dtype=torch.float32)
    dx = dW = db = None
    if need_x:
        dx = torch.empty(M, K, **f32)
        _gemm(lib, s, dy, N, 1, W, K, 1, dx, M, K, N)           # dy W
    if need_w:
        dW = torch.empty(N, K, **f32)
        _gemm(lib, s, dy, 1, N, x, K, 1, dW, N, K, M)           # dy^T x
    if need_b:
        db = torch.zeros(N, **f32)                              # ac_colsum adds
        check(lib.ac_colsum(ptr(dy), N, ptr(db), M, N, s), "ac_colsum")
    return dx, dW, db


class _EncKdLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, fc_emb, tchr_emb, ws_, bs_, wt_, bt_, logit_scale, bits):
        lib = _lib.load()
        s = _lib.stream()
        x, xt = f32c(fc_emb.detach()), f32c(tchr_emb.detach())
        Ws, bs, Wt, bt = (f32c(p.detach()) for p in (ws_, bs_, wt_, bt_))
        if x.shape[0] != xt.shape[0]:
            raise ValueError(f"enc_kd_loss: {x.shape[0]} student clips, {xt.shape[0]} teacher embeddings")
        es, et = _linear_fwd(lib, s, x, Ws, bs), _linear_fwd(lib, s, xt, Wt, bt)
        scale = f32c(logit_scale.detach()).reshape(1) if bits & CONTRA else None
        need = any(ctx.needs_input_grad)
        loss, _, _, _, flat = head(es, et, scale, bits, grads=need)
        ctx.saved = (x, xt, Ws, Wt, flat, es.shape) if need else None
        ctx.scale_shape = logit_scale.shape if logit_scale is not None else None
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        s = _lib.stream()
        x, xt, Ws, Wt, flat, (B, D) = ctx.saved
        need = ctx.needs_input_grad
        # ds | dt | dscale share one buffer: the upstream gradient (a device scalar) scales all three at once
        flat = flat * g.to(torch.float32)
        ds, dt, dscale = flat[:B * D].view(B, D), flat[B * D:2 * B * D].view(B, D), flat[2 * B * D:]
        dx, dWs, dbs = _linear_bwd(lib, s, ds, x, Ws, need[0], need[2], need[3])
        _, dWt, dbt = _linear_bwd(lib, s, dt, xt, Wt, False, need[4], need[5])
        dsc = dscale.reshape(ctx.scale_shape) if (need[6] and ctx.scale_shape is not None) else None
        return dx, None, dWs, dbs, dWt, dbt, dsc, None


def enc_kd_loss(fc_emb, tchr_emb, stdnt_proj, tchr_proj, logit_scale=None, kind="contra", l2_norm=False):
    """The encoder-distillation loss of the reference's wrappers, differentiable with respect to ``fc_emb``, both
    projections' parameters and ``logit_scale``.

    ``fc_emb`` (B, fc) student clip embedding; ``tchr_emb`` (B, tchr_dim) teacher embedding (no gradient);
    ``stdnt_proj`` / ``tchr_proj``: the two ``nn.Linear`` heads; ``logit_scale``: the contrastive temperature parameter
    (multiplies as it is), None for ``kind="mse"``; ``kind``: "contra", "mse" or "contra_mse"; ``l2_norm``: the MSE term on
    normalised embeddings.  Device tensors go through the HIP head (B <= 512, shared width <= 4096); CPU tensors through
    the same expression in torch."""
    bits = kind_bits(kind, l2_norm)
    if bits & CONTRA and logit_scale is None:
        raise ValueError("enc_kd_loss: the contrastive kinds need logit_scale")
    if not fc_emb.is_cuda:
        return torch_enc_kd_loss(stdnt_proj(fc_emb), tchr_proj(tchr_emb), logit_scale, bits)
    if stdnt_proj.bias is None or tchr_proj.bias is None:
        raise NotImplementedError("enc_kd_loss: the projections carry a bias (kd_wrapper.py:73-80)")
    tchr_emb = tchr_emb.to(fc_emb.device)
    return _EncKdLoss.apply(fc_emb, tchr_emb, stdnt_proj.weight, stdnt_proj.bias, tchr_proj.weight, tchr_proj.bias,
                            logit_scale, bits)
