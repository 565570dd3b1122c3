"""Float64 restatement of the encoder-distillation losses (kd_wrapper.py:56-226) and of their gradients in CLOSED FORM -
no autograd, so that it checks the fixture (the reference's own autograd, tests/golden/g24_enc_kd.npz) and the HIP head
(csrc/enc_kd.hip) independently of both.

    n(x) = x / max(||x||, 1e-12);  L = scale * n(s) n(t)^T
    contrastive = 0.5 * (mean_i CE(L_i., i) + mean_j CE(L_.j, j));  MSE = mean (a - b)^2, (a, b) = (n(s), n(t)) or (s, t)
    G = (softmax_rows(L) + softmax_cols(L) - 2 I) / (2 B);  d n(s) = scale * G n(t);  d n(t) = scale * G^T n(s)
    d scale = sum_ij G_ij cos_ij;  through n: dx = (dy - y (y . dy)) / ||x||, dy / 1e-12 below the clamp

A row is normalised once (kd_wrapper.py:216 normalises a normalised row again: the same value, and the same gradient
above the clamp).
"""
import torch

CONTRA, MSE, L2NORM = 1, 2, 4
EPS = 1e-12
KINDS = {"contra": CONTRA, "mse": MSE, "mse_l2": MSE | L2NORM, "contra_mse": CONTRA | MSE, "contra_mse_l2": CONTRA | MSE | L2NORM}


def _normalize(x):
    nrm = x.norm(dim=1, keepdim=True)
    den = nrm.clamp_min(EPS)
    return x / den, den, nrm < EPS


def _normalize_bwd(dy, y, den, clamped):
    return torch.where(clamped, dy / EPS, (dy - y * (y * dy).sum(1, keepdim=True)) / den)


def head(s, t, scale, bits):
    """s, t (B, D); scale a float.  Returns a dict of float64 tensors: loss, contra, mse, ds, dt, dscale."""
    s, t = s.detach().double(), t.detach().double()
    B, D = s.shape
    ys, den_s, cl_s = _normalize(s)
    yt, den_t, cl_t = _normalize(t)
    contra = torch.zeros((), dtype=torch.float64)
    mse = torch.zeros((), dtype=torch.float64)
    dys, dyt = torch.zeros_like(s), torch.zeros_like(t)
    ds, dt = torch.zeros_like(s), torch.zeros_like(t)
    dscale = torch.zeros((), dtype=torch.float64)
    if bits & CONTRA:
        cos = ys @ yt.t()
        L = float(scale) * cos
        lr = L - L.max(1, keepdim=True).values
        lc = L - L.max(0, keepdim=True).values
        lse_r = lr.exp().sum(1).log() + L.max(1).values
        lse_c = lc.exp().sum(0).log() + L.max(0).values
        diag = L.diagonal()
        contra = 0.5 * ((lse_r - diag).mean() + (lse_c - diag).mean())
        G = (torch.softmax(L, 1) + torch.softmax(L, 0) - 2.0 * torch.eye(B, dtype=torch.float64)) / (2.0 * B)
        dys = dys + float(scale) * (G @ yt)
        dyt = dyt + float(scale) * (G.t() @ ys)
        dscale = (G * cos).sum()
    if bits & MSE:
        a, b = (ys, yt) if bits & L2NORM else (s, t)
        mse = ((a - b) ** 2).mean()
        g = 2.0 * (a - b) / (B * D)
        if bits & L2NORM:
            dys, dyt = dys + g, dyt - g
        else:
            ds, dt = ds + g, dt - g
    if bits & CONTRA or bits & L2NORM:
        ds = ds + _normalize_bwd(dys, ys, den_s, cl_s)
        dt = dt + _normalize_bwd(dyt, yt, den_t, cl_t)
    return {"loss": contra + mse, "contra": contra, "mse": mse, "ds": ds, "dt": dt, "dscale": dscale}


def full(fc_emb, tchr_emb, ws, bs, wt, bt, scale, bits):
    """The loss behind the two projections s = fc_emb ws^T + bs, t = tchr_emb wt^T + bt, with the gradients of everything
    that gets one: fc_emb, ws, bs, wt, bt, scale."""
    x, xt, ws, bs, wt, bt = (v.detach().double() for v in (fc_emb, tchr_emb, ws, bs, wt, bt))
    h = head(x @ ws.t() + bs, xt @ wt.t() + bt, scale, bits)
    return {"loss": h["loss"], "contra": h["contra"], "mse": h["mse"],
            "fc_emb": h["ds"] @ ws, "stdnt_proj.weight": h["ds"].t() @ x, "stdnt_proj.bias": h["ds"].sum(0),
            "tchr_proj.weight": h["dt"].t() @ xt, "tchr_proj.bias": h["dt"].sum(0), "logit_scale": h["dscale"]}


def torch_loss(s, t, scale, bits):
    """The reference's expression (autograd-able, any dtype): what the float32 torch baseline of the bounds evaluates."""
    import torch.nn.functional as F
    loss = 0.0
    if bits & MSE:
        a, b = (F.normalize(s, dim=-1), F.normalize(t, dim=-1)) if bits & L2NORM else (s, t)
        loss = loss + F.mse_loss(a, b)
    if bits & CONTRA:
        sim = scale * (F.normalize(s, dim=-1) @ F.normalize(t, dim=-1).t())
        tgt = torch.arange(sim.shape[0], device=sim.device)
        loss = loss + 0.5 * (F.cross_entropy(sim, tgt) + F.cross_entropy(sim.t(), tgt))
    return loss
