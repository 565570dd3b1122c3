"""float64 restatement of token-level knowledge distillation (the reference's captioning/losses/kd_loss.py: TokenLevelKdLoss
"kl" and SupKdLoss over a LabelSmoothingLoss), independent of the product code - plain torch on the CPU.

For a valid row (n, t), t < tgt_len[n] (tgt_len clamped to T):

    kd_row  = -sum_v softmax(z_t / temp)_v * log_softmax(z_s / temp)_v          (not scaled by temp^2)
    sup_row = -sum_v q_v * log_softmax(z_s)_v,  q = 1 - smoothing on the target, smoothing / (V - 1) elsewhere
    kd = sum(kd_row) / count, sup = sum(sup_row) / count, count = sum_n min(tgt_len[n], T)
    loss = w * sup + (1 - w) * kd
    dlogit = g * [w * (softmax(z_s) - q) + (1 - w) * (softmax(z_s / temp) - softmax(z_t / temp)) / temp] / count

Masked rows contribute nothing and their teacher / student values (NaN included) are never looked at.
"""
import torch


def valid_mask(tgt_len, T):
    tgt_len = torch.as_tensor(tgt_len).to(torch.int64).clamp(max=T)
    return torch.arange(T)[None, :] < tgt_len[:, None]


def _rows(logit, tchr_logit, tgt, tgt_len, smoothing, temp):
    """(row_sup, row_kd, mask, count) in float64; masked rows are computed on zeros and then zeroed."""
    logit = torch.as_tensor(logit).double()
    tchr = torch.as_tensor(tchr_logit).double()
    N, T, V = logit.shape
    mask = valid_mask(tgt_len, T)
    zs = torch.where(mask[..., None], logit, torch.zeros_like(logit))
    zt = torch.where(mask[..., None], tchr, torch.zeros_like(tchr))
    tgt = torch.as_tensor(tgt).to(torch.int64)
    tgt = torch.where(mask, tgt, torch.zeros_like(tgt))
    lp = torch.log_softmax(zs, dim=-1)
    q = torch.full_like(lp, smoothing / (V - 1))
    q.scatter_(-1, tgt[..., None], 1.0 - smoothing)
    row_sup = -(q * lp).sum(-1)
    lpT = torch.log_softmax(zs / temp, dim=-1)
    pt = torch.softmax(zt / temp, dim=-1)
    row_kd = -(pt * lpT).sum(-1)
    m = mask.double()
    return row_sup * m, row_kd * m, mask, float(m.sum())


def row_sup(logit, tchr_logit, tgt, tgt_len, smoothing, temp):
    return _rows(logit, tchr_logit, tgt, tgt_len, smoothing, temp)[0]


def row_kd(logit, tchr_logit, tgt, tgt_len, smoothing, temp):
    return _rows(logit, tchr_logit, tgt, tgt_len, smoothing, temp)[1]


def kd_loss(logit, tchr_logit, tgt, tgt_len, smoothing, temp, sup_weight):
    """(loss, sup, kd, scale): scale = the mean of the absolute row terms that enter the loss, the size rounding errors
    are measured against."""
    rs, rk, mask, count = _rows(logit, tchr_logit, tgt, tgt_len, smoothing, temp)
    sup, kd = rs.sum() / count, rk.sum() / count
    w = float(sup_weight)
    loss = w * sup + (1.0 - w) * kd
    scale = (w * rs.abs().sum() + (1.0 - w) * rk.abs().sum()) / count
    return loss, sup, kd, scale


def kd_dlogit(logit, tchr_logit, tgt, tgt_len, smoothing, temp, sup_weight, g=1.0):
    """d(g * loss) / d(logit), written out (not autograd): exactly 0 on masked rows."""
    logit = torch.as_tensor(logit).double()
    tchr = torch.as_tensor(tchr_logit).double()
    N, T, V = logit.shape
    mask = valid_mask(tgt_len, T)
    count = float(mask.sum())
    zs = torch.where(mask[..., None], logit, torch.zeros_like(logit))
    zt = torch.where(mask[..., None], tchr, torch.zeros_like(tchr))
    tgt = torch.as_tensor(tgt).to(torch.int64)
    tgt = torch.where(mask, tgt, torch.zeros_like(tgt))
    q = torch.full_like(zs, smoothing / (V - 1))
    q.scatter_(-1, tgt[..., None], 1.0 - smoothing)
    w = float(sup_weight)
    d = w * (torch.softmax(zs, -1) - q) + (1.0 - w) * (torch.softmax(zs / temp, -1) - torch.softmax(zt / temp, -1)) / temp
    return torch.where(mask[..., None], d * (g / count), torch.zeros_like(d))
