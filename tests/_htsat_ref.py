"""Float64 restatement of the HTS-AT encoder's eval-mode arithmetic (reference transformer_encoder.py:119-996), one helper
per device kernel of csrc/htsat.hip so that the GPU tests can call them on small shapes.  Written from the seven steps
of the encoder's specification: bn0 per mel bin, bicubic stretch of the time axis to 1024 frames, fold into a 256 x 256
image, 4x4 patch embedding + LayerNorm, four stages of pre-norm Swin blocks (8 x 8 windows, odd blocks shifted by 4 with a
-100 region mask, relative-position bias, exact GELU), patch merging after stages 0-2, final LayerNorm, pooling.  Pinned
against the reference itself by tests/golden/g_htsat.npz (tests/test_htsat_cpu.py)."""
import math

import torch

WINDOW, FRAMES = 8, 1024
DT = torch.float64


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def bn0(state, lms, prefix="", eps=1e-5):
    """lms (B, T, 64) log-mel in dB -> BatchNorm per mel bin with the running statistics."""
    g, b = state[prefix + "bn0.weight"].to(DT), state[prefix + "bn0.bias"].to(DT)
    m, v = state[prefix + "bn0.running_mean"].to(DT), state[prefix + "bn0.running_var"].to(DT)
    return (lms.to(DT) - m) / torch.sqrt(v + eps) * g + b


def cubic_taps(t, A=-0.75):
    """Weights of the four taps at offsets -1, 0, 1, 2 for a fraction t in [0, 1): Keys' cubic convolution kernel."""
    def near(d):   # |d| <= 1
        return ((A + 2.0) * d - (A + 3.0)) * d * d + 1.0

    def far(d):    # 1 < |d| < 2
        return ((A * d - 5.0 * A) * d + 8.0 * A) * d - 4.0 * A

    return torch.stack([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)], dim=-1)


def bicubic_time(x, out_frames=FRAMES):
    """x (B, T, M) -> (B, out_frames, M): cubic convolution along time with aligned corners (output frame f sits at
    f (T - 1) / (out_frames - 1)) and tap indices clamped to the clip.  T == out_frames: unchanged."""
    B, T, M = x.shape
    if T == out_frames:
        return x.to(DT)
    f = torch.arange(out_frames, dtype=torch.int64)
    num = f * (T - 1)
    i0 = num // (out_frames - 1)
    t = (num % (out_frames - 1)).to(DT) / (out_frames - 1)
    taps = cubic_taps(t)                                                    # (F, 4)
    idx = (i0[:, None] + torch.arange(-1, 3)[None, :]).clamp(0, T - 1)      # (F, 4)
    return (x.to(DT)[:, idx, :] * taps[None, :, :, None]).sum(2)


def fold(x):
    """x (B, 1024, 64) -> image (B, 256, 256): row = chunk * 64 + mel, column = frame % 256, chunk = frame // 256."""
    B = x.shape[0]
    return x.reshape(B, 4, 256, 64).permute(0, 1, 3, 2).reshape(B, 256, 256)


def patch_embed(x, w, b, ln_w, ln_b):
    """x (B, T, 64) bn0-normalised log-mel -> tokens (B, 4096, C): stretch, fold, 4x4 / stride-4 patches times
    w (C, 1, 4, 4) + b, LayerNorm; tokens row-major over (image row / 4, image column / 4)."""
    img = fold(bicubic_time(x))
    B = img.shape[0]
    p = img.reshape(B, 64, 4, 64, 4).permute(0, 1, 3, 2, 4).reshape(B, 4096, 16)
    y = p @ w.to(DT).reshape(-1, 16).t() + b.to(DT)
    return _ln(y, ln_w.to(DT), ln_b.to(DT))


def relative_bias(table, window=WINDOW):
    """table ((2 window - 1)^2, heads) -> (heads, window^2, window^2): entry for query (h1, w1), key (h2, w2) is row
    (h1 - h2 + window - 1) (2 window - 1) + (w1 - w2 + window - 1) of the table."""
    n = window * window
    out = torch.empty(table.shape[1], n, n, dtype=table.dtype)
    for a in range(n):
        for c in range(n):
            dh, dw = a // window - c // window, a % window - c % window
            out[:, a, c] = table[(dh + window - 1) * (2 * window - 1) + dw + window - 1]
    return out


def region_ids(H, W, shift, window=WINDOW):
    """(H, W) region label of every position of the rolled image: three bands per axis - before the last window, the last
    window up to the shift, the wrapped-around rest."""
    def band(n):
        return torch.tensor([0 if i < n - window else (1 if i < n - shift else 2) for i in range(n)])

    return band(H)[:, None] * 3 + band(W)[None, :]


def window_attn(qkv, bias, H, W, heads, shift):
    """qkv (B, H*W, 3C), bias (heads, 64, 64) -> (B, H*W, C): roll by -shift, cut into 8 x 8 windows, per head
    softmax(q k^T / sqrt(24) + bias [+ -100 across regions]) v, undo the cut and the roll."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    x = qkv.to(DT).view(B, H, W, C3)
    ids = region_ids(H, W, shift) if shift else torch.zeros(H, W, dtype=torch.int64)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))

    def cut(t, last):
        return t.reshape(-1, H // WINDOW, WINDOW, W // WINDOW, WINDOW, last).permute(0, 1, 3, 2, 4, 5).reshape(
            -1, H // WINDOW, W // WINDOW, WINDOW * WINDOW, last)

    xw = cut(x, C3)                                                   # (B, nh, nw, 64, 3C)
    idw = cut(ids.view(1, H, W, 1), 1)[0, ..., 0]                     # (nh, nw, 64)
    mask = (idw[..., :, None] != idw[..., None, :]).to(DT) * -100.0   # (nh, nw, 64, 64)
    q, k, v = (xw[..., i * C:(i + 1) * C].reshape(*xw.shape[:4], heads, hd).transpose(3, 4) for i in range(3))
    s = (q * hd ** -0.5) @ k.transpose(-1, -2) + bias.to(DT) + mask[None, :, :, None]
    o = (torch.softmax(s, -1) @ v).transpose(3, 4).reshape(B, H // WINDOW, W // WINDOW, WINDOW, WINDOW, C)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(B, N, C)


def patch_merge(x, H, W, ln_w, ln_b):
    """x (B, H*W, C) -> (B, H/2*W/2, 4C): channels [x(even row, even col), x(odd row, even col), x(even row, odd col),
    x(odd row, odd col)], LayerNorm(4C); the bias-free reduction is a plain linear layer applied by the caller."""
    B, N, C = x.shape
    x = x.to(DT).view(B, H, W, C)
    y = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return _ln(y.reshape(B, N // 4, 4 * C), ln_w.to(DT), ln_b.to(DT))


def pool(x, Hh, Ww, fbins):
    """x (B, Hh*Ww, C), token row chunk * fbins + f -> attn (B, Hh/fbins * Ww, C) = mean over f, fc (B, C) = mean over
    all frames."""
    B, N, C = x.shape
    attn = x.to(DT).view(B, Hh // fbins, fbins, Ww, C).mean(2).reshape(B, -1, C)
    return attn, attn.mean(1)


def token_mean(x):
    return x.to(DT).mean(1)


def feat_len(wav_len, hop=320):
    return (torch.as_tensor(wav_len) // hop + 1) // 8 // 4


def swin_block(state, p, x, H, W, heads, shift):
    g = lambda k: state[p + k].to(DT)   # noqa: E731
    y = _ln(x, g("norm1.weight"), g("norm1.bias"))
    qkv = y @ g("attn.qkv.weight").t() + g("attn.qkv.bias")
    a = window_attn(qkv, relative_bias(g("attn.relative_position_bias_table")), H, W, heads, shift)
    x = x + a @ g("attn.proj.weight").t() + g("attn.proj.bias")
    y = _ln(x, g("norm2.weight"), g("norm2.bias"))
    h = gelu(y @ g("mlp.fc1.weight").t() + g("mlp.fc1.bias"))
    return x + h @ g("mlp.fc2.weight").t() + g("mlp.fc2.bias")


def forward(state, x, depths=(2, 2, 6, 2), prefix="", heads=(4, 8, 16, 32)):
    """x (B, T, 64) bn0-normalised log-mel -> {"attn_emb", "fc_emb", "layer_0" .. "layer_3", "tokens": [after the patch
    embedding, after every stage]}."""
    g = lambda k: state[prefix + k].to(DT)   # noqa: E731
    t = patch_embed(x, g("patch_embed.proj.weight"), g("patch_embed.proj.bias"), g("patch_embed.norm.weight"),
                    g("patch_embed.norm.bias"))
    out = {"tokens": [t]}
    H = 64
    for s, depth in enumerate(depths):
        for b in range(depth):
            shift = WINDOW // 2 if (b % 2 == 1 and H > WINDOW) else 0
            t = swin_block(state, f"{prefix}layers.{s}.blocks.{b}.", t, H, H, heads[s], shift)
        if s < len(depths) - 1:
            t = patch_merge(t, H, H, g(f"layers.{s}.downsample.norm.weight"), g(f"layers.{s}.downsample.norm.bias"))
            t = t @ g(f"layers.{s}.downsample.reduction.weight").t()
            H //= 2
            out[f"layer_{s}"] = token_mean(t)
        out["tokens"].append(t)
    t = _ln(t, g("norm.weight"), g("norm.bias"))
    out["attn_emb"], out["fc_emb"] = pool(t, H, H, H // 4)
    out[f"layer_{len(depths) - 1}"] = out["fc_emb"]
    return out
