"""F(6,3) along time - the row-SEXTET tile form of the F(4,3) conv kernel (csrc/conv3x3_wino43.hip) - as a CPU reference,
next to tests/_split_ref.py, whose matrices table ``XF``, split, products and bound it uses.  Importing this module
registers m = 6 there (``XF[6]``, ``FORM_M["wino63"]``), so ``conv_wino_f64(x, w, 6)`` and ``layer_bound(..., "wino63")``
work as for the other forms; the input / output transforms of the emulation are spelled here with the factoring of
csrc/ac_wino43.h (w6_transform, w6_outputs).

The kernel tiles the STACKED rows of a batch ([B*Hp] rows, zero rows between clips) from row 0 on, so a sextet may
straddle two clips and its transformed operands see both: ``stacked_*`` evaluate emulation and bound on that one signal,
which is the tiling the kernel has."""
import torch
import torch.nn.functional as F

import _split_ref as S

# F(6,3), points 0, +-1, +-2, +-1/2, inf (Lavin & Gray)
BT6 = torch.tensor([[1, 0, -21 / 4, 0, 21 / 4, 0, -1, 0],
                    [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0],
                    [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
                    [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0],
                    [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0],
                    [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0],
                    [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0],
                    [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]], dtype=torch.float64)
G6 = torch.tensor([[1, 0, 0], [-2 / 9, -2 / 9, -2 / 9], [-2 / 9, 2 / 9, -2 / 9], [1 / 90, 1 / 45, 2 / 45], [1 / 90, -1 / 45, 2 / 45],
                   [32 / 45, 16 / 45, 8 / 45], [32 / 45, -16 / 45, 8 / 45], [0, 0, 1]], dtype=torch.float64)
AT6 = torch.tensor([[1, 1, 1, 1, 1, 1, 1, 0],
                    [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0],
                    [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0],
                    [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 0],
                    [0, 1, 1, 16, 16, 1 / 16, 1 / 16, 0],
                    [0, 1, -1, 32, -32, 1 / 32, -1 / 32, 1]], dtype=torch.float64)
S.XF.setdefault(6, (BT6, G6, AT6))
S.FORM_M.setdefault("wino63", 6)

_fma = S._fma


def in_transform(d):
    """The rows d[0 .. 7] (f32) of a sextet -> the 8 positions in f32, factored as w6_transform (every constant is a dyadic
    rational: the plain products are exact, every fma rounds once)."""
    te1, to1 = _fma(-4.25, d[4], d[2] + d[6]), _fma(-4.25, d[3], d[1] + d[5])
    te2, to2 = _fma(0.25, d[2], _fma(-1.25, d[4], d[6])), _fma(2.0, d[5], _fma(-2.5, d[3], 0.5 * d[1]))
    te3, to3 = _fma(4.0, d[2], _fma(-5.0, d[4], d[6])), _fma(2.0, d[1], _fma(-2.5, d[3], 0.5 * d[5]))
    return [_fma(5.25, d[4] - d[2], d[0] - d[6]), te1 + to1, te1 - to1, te2 + to2, te2 - to2, te3 + to3, te3 - to3,
            _fma(5.25, d[3] - d[5], d[7] - d[1])]


def out_transform(M):
    """The 8 position sums (f32) -> the 6 output rows (f32), factored as w6_outputs."""
    s12, d12, s34, d34, s56, d56 = M[1] + M[2], M[1] - M[2], M[3] + M[4], M[3] - M[4], M[5] + M[6], M[5] - M[6]
    return [((M[0] + s12) + s34) + s56, _fma(0.5, d56, _fma(2.0, d34, d12)), _fma(0.25, s56, _fma(4.0, s34, s12)),
            _fma(0.125, d56, _fma(8.0, d34, d12)), _fma(0.0625, s56, _fma(16.0, s34, s12)),
            _fma(0.03125, d56, _fma(32.0, d34, d12)) + M[7]]


def conv_split(x, w, ar=S.FAITHFUL):
    """``_split_ref.conv_split`` for m = 6: conv3x3 (padding 1) of x (B, C, H, W) f32 in the sextet form's arithmetic, tiles
    from row 0 of every clip: (B, O, H, W) f32, no epilogue."""
    B, C, H, W = x.shape
    rows, He = S._tiles(x.float(), 6)
    v = torch.stack(in_transform(rows), 0)                                       # (8, B, C, nt, W + 2) f32
    Mp = S.split_products(S.filter_transform(w, 6), S._mel_taps(v, W), ar)       # (8, O, N)
    y = torch.stack(out_transform(list(Mp)), 0)                                  # (6, O, B * nt * W)
    nt = He // 6
    return y.reshape(6, -1, B, nt, W).permute(2, 1, 3, 0, 4).reshape(B, -1, He, W)[:, :, :H]


def layer_emul(x, w, sc, sh, mode, ar=S.FAITHFUL):
    return S._epilogue(F.relu(S._fma_bn(conv_split(x, w, ar), sc, sh)), mode)


def stack(x, Hp):
    """(B, C, H, W) -> the batch as ONE clip (1, C, B * Hp, W) with zero rows from H on in every clip: what the kernel tiles."""
    B, C, H, W = x.shape
    xs = torch.zeros(B, C, Hp, W, dtype=x.dtype)
    xs[:, :, :H] = x
    return xs.permute(1, 0, 2, 3).reshape(1, C, B * Hp, W)


def unstack(y, B, H):
    """(1, O, B * Hp, W) -> (B, O, H, W): the valid rows of every clip."""
    _, O, rows, W = y.shape
    return y.reshape(O, B, rows // B, W).permute(1, 0, 2, 3)[:, :, :H]


def stacked_bound(x, w, sc, mode, Hp):
    """``_split_ref.layer_bound`` for m = 6 on the stacked signal: 2^-15 of the transform-aware magnitude
    |A^T| ((|G| |w|) . (|B^T| |x|)) |scale| with the sextets where the kernel puts them, through the pool.  Layout of
    ``_split_ref._epilogue``: (B, H', W', O)."""
    B, _, H, _ = x.shape
    t = unstack(S.conv_wino_f64(stack(x, Hp), w, 6, absolute=True), B, H) * sc.double().abs()[None, :, None, None]
    return S.EPS_PRODUCT * S._epilogue(t, mode)


def stacked_emul(x, w, sc, sh, mode, Hp):
    """The layer in the sextet form's arithmetic with the sextets where the kernel puts them: (B, H', W', O) f32."""
    B, _, H, _ = x.shape
    y = unstack(conv_split(stack(x, Hp), w), B, H)
    return S._epilogue(F.relu(S._fma_bn(y, sc, sh)), mode)
