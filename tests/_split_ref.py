"""The split-bf16 conv tier's arithmetic as a CPU reference (torch on the CPU only: neither oracle/ nor the library), for
tests/test_split_ref_cpu.py, tests/test_gpu_split_error.py and the checker script tests/wino_split_emulation.py.

For one layer ``relu(scale * conv3x3(x, w) + shift)`` followed by the kernel's epilogue (mode 0: nothing; 1: 2x2 average pool;
2: mean over the two mel columns) ``layer()`` returns a ``Case`` with

    exact : the result in float64;
    emul  : the result in the tier's own arithmetic as the sources document it - filter transform in float64 and then split
            (kernels.pack_conv_weight_wino43_frag / pack_conv_weight_wino1d_frag; the direct form splits the f32 weight:
            pack_conv_weight_bf16x3_frag), input transform in f32 with the factoring of csrc/ac_wino43.h and then split,
            hi = RNE(x), lo = RNE(x - hi) both times, products hi*hi + hi*lo + lo*hi, f32 accumulation, output transform
            (w4_outputs) + BatchNorm + ReLU + pool in f32;
    mag   : the normaliser |scale| * conv3x3(|x|, |w|) in float64 through the same pool / mean (convex combinations: a
            componentwise bound carries over).

all three in the layout (B, H_out, W_out, Cout) of the VALID output rows (mode 2: (B, H, Cout)).  Errors are
``rho(a, b) = |a - b| / mag``: no unit, indifferent to how the data is scaled.  Forms: "direct" (conv3x3_bn_relu_bf16x3_gw,
conv3x3_bn_relu_skinny, and ``linear()`` for the one-tap linear layer), "wino1d" = F(2,3) along time, "wino43" = F(4,3) along
time, and ``block1()``: conv block 1 in one kernel (csrc/conv3x3_block1_w4.hip).

``Arith`` holds the knobs that turn the faithful arithmetic into one of the MUTANTS the acceptance criterion (``figures`` /
``verdict``: what tests/test_gpu_split_error.py asserts of a kernel) must reject, and into the faithful variants (another
order of the K sum, another rounding of the input transform) it must accept."""
import math
import os
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

# F(2,3), points 0, +-1, inf
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
# F(4,3), points 0, +-1, +-2, inf (Lavin & Gray) - the matrices csrc/ac_wino43.h spells out row by row
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                   [0, 0, 1]], dtype=torch.float64)
AT4 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)
# "F(1,3)": the direct form as a degenerate transform (three positions = the three taps)
BT1, G1, AT1 = torch.eye(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64), torch.ones(1, 3, dtype=torch.float64)
XF = {1: (BT1, G1, AT1), 2: (BT, G, AT), 4: (BT4, G4, AT4)}
FORM_M = {"direct": 1, "wino1d": 2, "wino43": 4}   # outputs per tile along time

EPS_PRODUCT = 2.0 ** -15   # componentwise bound of one split product, derived above ``layer_bound``


# ---- the operand split ------------------------------------------------------------------------------------------------
def trunc_bf16(x):
    """Round toward zero to bf16 (keep the upper half of the f32 word): the WRONG rounding of the mutants."""
    x = x.float().contiguous()
    return (x.view(torch.int32) & -65536).view(torch.float32)


def split(x, fmt="bf16", flush=False, hi_mode="rne", lo_mode="rne"):
    """x (f32 / f64) -> (hi, lo) as f32 tensors holding values representable in fmt: hi = RNE(x), lo = RNE(x - hi), the
    difference taken in x's own precision (f32 in the kernels, f64 in the weight packs of the Winograd forms)."""
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[fmt]
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()

    def rnd(t, mode):
        if mode == "rne":
            return t.to(dt).to(x.dtype)
        assert fmt == "bf16" and mode == "trunc", mode
        return trunc_bf16(t).to(x.dtype)

    hi = rnd(x, hi_mode)
    lo = rnd(x - hi, lo_mode)
    hi, lo = hi.float(), lo.float()
    if flush and fmt == "f16":
        tiny = 2.0 ** -14
        hi = torch.where(hi.abs() < tiny, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < tiny, torch.zeros_like(lo), lo)
    return hi, lo


@dataclass
class Arith:
    """The faithful arithmetic (defaults) and its variants.  Mutants: ``x_hi`` / ``x_lo`` / ``w`` = "trunc" (the split rounds
    toward zero: activations' hi, activations' lo, both planes of the weights); ``no_wlo_xhi_kstep = s``: the product
    w_lo * x_hi is missing in the 16-channel K step s; ``no_wlo_pos = p``: the weights' lo plane is lost at transform
    position p (all mel taps); ``no_xlo_kblock = b``: the activations' lo plane is lost for the 32-channel block b.
    Faithful variants: ``chunk = n``: one f32 accumulator walked over n-channel K steps (hi*lo, lo*hi, hi*hi per step, the
    order of the kernels' K loops) instead of three whole-K products; ``transform64``: input transform evaluated in float64
    and rounded once to f32."""
    x_hi: str = "rne"
    x_lo: str = "rne"
    w: str = "rne"
    no_wlo_xhi_kstep: int = None
    no_wlo_pos: int = None
    no_xlo_kblock: int = None
    chunk: int = None
    transform64: bool = False
    fmt: str = "bf16"
    flush: bool = False


FAITHFUL = Arith()


def mutants(cin):
    """name -> Arith: the table of the acceptance criterion's teeth (tests/test_split_ref_cpu.py).  K steps / blocks in the
    middle of the channel range."""
    return {
        "split by truncation, both operands": Arith(x_hi="trunc", x_lo="trunc", w="trunc"),
        "split by truncation, activations only": Arith(x_hi="trunc", x_lo="trunc"),
        "lo = trunc(x - hi), activations only": Arith(x_lo="trunc"),
        "w_lo * x_hi missing in one 16-channel K step": Arith(no_wlo_xhi_kstep=cin // 32),
        "weight lo plane lost at one position": Arith(no_wlo_pos=1),
        "input lo plane lost for one 32-channel block": Arith(no_xlo_kblock=cin // 64),
    }


def _fma(a, x, y):
    """a * x + y with ONE rounding to f32 (__builtin_fmaf): a is a small integer, so the float64 result is exact up to a
    double rounding that cannot be seen at f32."""
    return (a * x.double() + y.double()).float()


def _in_transform(m, d, t64=False):
    """The rows d[0 .. m+1] (f32) of a tile -> the m + 2 positions, in f32 with the kernels' factoring
    (csrc/ac_wino43.h w4_transform; csrc/conv3x3_wino1d.hip: one add each)."""
    if t64:
        bt = XF[m][0]
        return [sum(float(bt[p, r]) * d[r].double() for r in range(m + 2) if float(bt[p, r]) != 0.0).float() for p in range(m + 2)]
    if m == 1:
        return list(d)
    if m == 2:
        return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    t1, t2 = _fma(-4.0, d[2], d[4]), _fma(-4.0, d[1], d[3])
    t3, u = d[4] - d[2], d[3] - d[1]
    return [_fma(4.0, d[0], _fma(-5.0, d[2], d[4])), t1 + t2, t1 - t2, _fma(2.0, u, t3), _fma(-2.0, u, t3),
            _fma(4.0, d[1], _fma(-5.0, d[3], d[5]))]


def _out_transform(m, M):
    """The m + 2 position sums (f32) -> the m output rows (f32), factored as the kernels' epilogues (w4_outputs)."""
    if m == 1:
        return [(M[0] + M[1]) + M[2]]
    if m == 2:
        return [(M[0] + M[1]) + M[2], (M[1] - M[2]) - M[3]]
    s12, d12, s34, d34 = M[1] + M[2], M[1] - M[2], M[3] + M[4], M[3] - M[4]
    return [(M[0] + s12) + s34, _fma(2.0, d34, d12), _fma(4.0, s34, s12), _fma(8.0, d34, d12) + M[5]]


def filter_transform(w, m):
    """OIHW -> U[p][kx] (P, 3, O, C) in float64: G over the time taps ky, the sums spelled as the weight packs spell them."""
    g = w.double()
    gm = XF[m][1]
    return torch.stack([float(gm[p, 0]) * g[:, :, 0] + float(gm[p, 1]) * g[:, :, 1] + float(gm[p, 2]) * g[:, :, 2]
                        for p in range(m + 2)], 0).permute(0, 3, 1, 2).contiguous()   # (P, o, c, kx) -> (P, kx, o, c)


def split_products(U, V, ar=FAITHFUL):
    """sum over (tap, channel) of U[p, t, o, c] * V[p, t, c, n] with both operands split: (P, O, N) in f32.  U float64 (or
    f32: the direct form), V f32."""
    P, T, O, C = U.shape
    uh, ul = split(U, ar.fmt, ar.flush, ar.w, ar.w)
    vh, vl = split(V, ar.fmt, ar.flush, ar.x_hi, ar.x_lo)
    if ar.no_wlo_xhi_kstep is not None:
        s = ar.no_wlo_xhi_kstep
        assert 16 * s + 16 <= C
        ul = ul.clone()
        ul[:, :, :, 16 * s:16 * s + 16] = 0
    if ar.no_wlo_pos is not None:
        ul = ul.clone()
        ul[ar.no_wlo_pos] = 0
    if ar.no_xlo_kblock is not None:
        b = ar.no_xlo_kblock
        assert 32 * b + 32 <= C
        vl = vl.clone()
        vl[:, :, 32 * b:32 * b + 32] = 0
    if ar.chunk:
        acc = torch.zeros(P, O, V.shape[-1])
        for c0 in range(0, C, ar.chunk):
            c1 = min(C, c0 + ar.chunk)
            a_h, a_l = (t[..., c0:c1].permute(0, 2, 1, 3).reshape(P, O, -1) for t in (uh, ul))
            b_h, b_l = (t[:, :, c0:c1].reshape(P, -1, V.shape[-1]) for t in (vh, vl))
            acc = acc + a_h @ b_l
            acc = acc + a_l @ b_h
            acc = acc + a_h @ b_h
        return acc
    a_h, a_l = (t.permute(0, 2, 1, 3).reshape(P, O, T * C) for t in (uh, ul))
    b_h, b_l = (t.reshape(P, T * C, -1) for t in (vh, vl))
    return a_h @ b_h + (a_h @ b_l + a_l @ b_h)


def _tiles(x, m):
    """x (B, C, H, W) -> the m + 2 rows of every tile, each (B, C, nt, W + 2), zero padded; tiles start at row 0 of a clip."""
    H = x.shape[2]
    He = -(-H // m) * m
    xp = F.pad(x, (1, 1, 1, 1 + He - H))
    return [xp[:, :, r:r + He:m] for r in range(m + 2)], He


def _mel_taps(v, W):
    """v (P, B, C, nt, W + 2) -> (P, 3 kx, C, B * nt * W)"""
    P, B, C, nt, _ = v.shape
    return torch.stack([v[..., kx:kx + W].permute(0, 2, 1, 3, 4).reshape(P, C, B * nt * W) for kx in range(3)], 1)


def conv_split(x, w, form, ar=FAITHFUL):
    """conv3x3 (padding 1) of x (B, C, H, W) f32 with w OIHW in the tier's arithmetic: (B, O, H, W) f32, no epilogue."""
    m = FORM_M[form]
    B, C, H, W = x.shape
    rows, He = _tiles(x.float(), m)
    v = torch.stack(_in_transform(m, rows, ar.transform64), 0)                  # (P, B, C, nt, W + 2) f32
    U = w.float().permute(2, 3, 0, 1).contiguous() if m == 1 else filter_transform(w, m)   # direct: the f32 weight, (ky, kx, o, c)
    Mp = split_products(U, _mel_taps(v, W), ar)                                  # (P, O, N)
    y = torch.stack(_out_transform(m, list(Mp)), 0)                              # (m, O, B * nt * W)
    nt = He // m
    return y.reshape(m, -1, B, nt, W).permute(2, 1, 3, 0, 4).reshape(B, -1, He, W)[:, :, :H]


def conv_wino_f64(x, w, m, absolute=False):
    """The same Winograd pipeline in float64 without any split; ``absolute``: every matrix and operand by its absolute
    value - the transform-aware magnitude |A^T| ((|G| |w|) . (|B^T| |x|)) that a componentwise bound is taken against."""
    bt, gm, at = XF[m]
    x, w = x.double(), w.double()
    if absolute:
        bt, gm, at, x, w = bt.abs(), gm.abs(), at.abs(), x.abs(), w.abs()
    B, C, H, W = x.shape
    rows, He = _tiles(x, m)
    d = torch.stack(rows, 0)                                                     # (m + 2, B, C, nt, W + 2)
    v = torch.einsum("pr,rbctw->pbctw", bt, d)
    U = torch.einsum("pk,ockx->pxoc", gm, w)                                     # (P, kx, O, C)
    P = m + 2
    Mp = U.permute(0, 2, 1, 3).reshape(P, -1, 3 * C) @ _mel_taps(v, W).reshape(P, 3 * C, -1)
    y = torch.einsum("ap,pon->aon", at, Mp)
    nt = He // m
    return y.reshape(m, -1, B, nt, W).permute(2, 1, 3, 0, 4).reshape(B, -1, He, W)[:, :, :H]


# ---- epilogues and layouts --------------------------------------------------------------------------------------------
def _bn(y, sc, sh):
    return y * sc[None, :, None, None] + sh[None, :, None, None]


def _epilogue(y, mode):
    """(B, O, H, W) -> the valid rows in the kernels' channels-last order: (B, H', W', O), mode 2: (B, H, O)."""
    if mode == 1:
        y = F.avg_pool2d(y, 2)
    if mode == 2:
        return y.mean(dim=3).transpose(1, 2).contiguous()
    return y.permute(0, 2, 3, 1).contiguous()


def to_rows(x_nchw, Hp):
    """(B, C, H, W) -> the kernels' activation layout [B*Hp][W][C] with zero rows from H on."""
    B, C, H, W = x_nchw.shape
    out = torch.zeros(B, Hp, W, C)
    out[:, :H] = x_nchw.permute(0, 2, 3, 1)
    return out.reshape(B * Hp, W, C).contiguous()


@dataclass
class Case:
    exact: torch.Tensor
    emul: torch.Tensor
    mag: torch.Tensor
    info: dict = field(default_factory=dict)

    def clips(self, n):
        """The first n clips (clips do not interact)."""
        return Case(self.exact[:n], self.emul[:n], self.mag[:n], self.info)


def layer_exact(x, w, sc, sh, mode):
    y = F.relu(_bn(F.conv2d(x.double(), w.double(), padding=1), sc.double(), sh.double()))
    mag = F.conv2d(x.double().abs(), w.double().abs(), padding=1) * sc.double().abs()[None, :, None, None]
    return _epilogue(y, mode), _epilogue(mag, mode)


def _fma_bn(y, sc, sh):
    """fmaf(y, scale, shift) in f32 (one rounding)"""
    return (y.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]).float()


def layer_emul(x, w, sc, sh, mode, form, ar=FAITHFUL):
    y = conv_split(x, w, form, ar)
    y = F.relu(_fma_bn(y, sc, sh))
    return _epilogue(y, mode)


def layer(x, w, sc, sh, mode, form, ar=FAITHFUL):
    exact, mag = layer_exact(x, w, sc, sh, mode)
    return Case(exact, layer_emul(x, w, sc, sh, mode, form, ar), mag, dict(form=form, mode=mode, cin=x.shape[1]))


# Why 2^-15 per product.  hi = RNE_bf16(x) leaves |x - hi| <= 2^-9 |x|, lo = RNE_bf16(x - hi) leaves |x - hi - lo| <= 2^-18 |x|.
# A product of two split operands without the lo*lo term, (xh + xl)(wh + wl) - xl wl, is therefore off by at most
# |x| |w| (2^-18 + 2^-18 + 2^-18) < 2^-16 |x| |w| to first order (the two split residuals and the missing lo*lo).  The operands of the products are the TRANSFORMED
# ones, B^T x and G w, so the sum of the bounds over a dot product is 2^-16 (|G||w|) . (|B^T||x|), carried through the
# output transform by |A^T| and through BatchNorm by |scale|; ReLU is 1-Lipschitz and the pool / mean are convex
# combinations.  The factor 2 on top (2^-15) pays for what first order leaves out: the f32 roundings of the input
# transform (a few 2^-24 of |B^T||x|) and of the accumulation, which stays far below its worst case K 2^-24 (the faithful
# emulation sits at a few percent of this bound for K = 1152 ... 18432, see tests/golden/REPORT_split_error.txt).
def layer_bound(x, w, sc, mode, form):
    """Componentwise bound of |emul - exact| for one layer (derivation above)."""
    m = FORM_M[form]
    t = conv_wino_f64(x, w, m, absolute=True) * sc.double().abs()[None, :, None, None]
    return EPS_PRODUCT * _epilogue(t, mode)


# ---- conv block 1 in one kernel ---------------------------------------------------------------------------------------
def _conv1_exact(x, w1, s1, t1):
    return F.relu(_bn(F.conv2d(x.double(), w1.double(), padding=1), s1.double(), t1.double()))


def _conv1_mag(x, w1, s1, t1):
    """Magnitude of conv1's own sum (>= |conv1 output|): what conv1's rounding errors are relative to."""
    return _bn(F.conv2d(x.double().abs(), w1.double().abs(), padding=1), s1.double().abs(), t1.double().abs())


def conv1_emul(x, w1, s1, t1, form, ar=FAITHFUL):
    """conv1 of block 1 (one input channel) + BN + ReLU in f32 as csrc/conv3x3_block1_w4.hip computes it.  "mfma": a split
    product with K = 9 - taps times the BN scale (f32 product) and then split, the BN shift split as one more tap against a
    constant 1, the log-mel values split; "valu": the 9-term fmaf chain of conv_first_kernel, then fmaf(a, scale, shift)."""
    B, _, H, W = x.shape
    xp = F.pad(x.float(), (1, 1, 1, 1))[:, 0]                                    # (B, H + 2, W + 2)
    taps = [xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]   # t = 3 ky + kx, each (B, H, W)
    if form == "valu":
        a = torch.zeros(B, 64, H, W)
        wf = w1.float().reshape(64, 9)
        for t in range(9):
            a = (taps[t].double()[:, None] * wf[:, t].double()[None, :, None, None] + a.double()).float()
        return F.relu(_fma_bn(a, s1.float(), t1.float()))
    assert form == "mfma", form
    wt = (w1.float().reshape(64, 9) * s1.float()[:, None])                       # f32 product, then split
    A = torch.cat([wt, t1.float()[:, None]], 1)                                  # (64, 10): nine taps and the shift
    Bm = torch.stack(taps + [torch.ones_like(taps[0])], 0).reshape(10, -1)       # (10, B * H * W)
    y = split_products(A.reshape(1, 1, 64, 10), Bm.reshape(1, 1, 10, -1), Arith(fmt=ar.fmt))[0]
    return F.relu(y.reshape(64, B, H, W).permute(1, 0, 2, 3))


def block1_exact(x, w1, s1, t1, w2, s2, t2):
    """conv_block1 + 2x2 average pool in float64: x (B, 1, H, 64) -> (exact, mag).  ``mag`` = |s2| * conv3x3(m1, |w2|) with m1
    the magnitude of conv1's own sum: it normalises conv2's error (m1 >= |conv1 output|) and conv1's error carried through
    conv2."""
    y1 = _conv1_exact(x, w1, s1, t1)
    exact = _epilogue(F.relu(_bn(F.conv2d(y1, w2.double(), padding=1), s2.double(), t2.double())), 1)
    m1 = _conv1_mag(x, w1, s1, t1)
    return exact, _epilogue(F.conv2d(m1, w2.double().abs(), padding=1) * s2.double().abs()[None, :, None, None], 1)


def block1(x, w1, s1, t1, w2, s2, t2, conv1="mfma", ar=FAITHFUL, exact_mag=None):
    """The Case of conv block 1 in one kernel with conv1 in the form ``conv1``; ``exact_mag``: what ``block1_exact`` returned
    (shared between the two forms)."""
    exact, mag = exact_mag if exact_mag is not None else block1_exact(x, w1, s1, t1, w2, s2, t2)
    e1 = conv1_emul(x, w1, s1, t1, conv1, ar)
    return Case(exact, layer_emul(e1, w2, s2, t2, 1, "wino43", ar), mag, dict(form="block1/" + conv1, mode=1, cin=64))


def block1_bound(x, w1, s1, t1, w2, s2):
    """conv2's bound on conv1's exact output plus conv1's own bound (2^-15 of its magnitude, K = 9 and the shift) carried
    through |s2| conv3x3(., |w2|); ReLU is 1-Lipschitz."""
    y1 = _conv1_exact(x, w1, s1, t1)
    own = conv_wino_f64(y1, w2, 4, absolute=True)
    carried = F.conv2d(_conv1_mag(x, w1, s1, t1), w2.double().abs(), padding=1)
    return EPS_PRODUCT * _epilogue((own + carried) * s2.double().abs()[None, :, None, None], 1)


# ---- the one-tap linear layer -----------------------------------------------------------------------------------------
def linear(x, w, b, relu=False, ar=FAITHFUL):
    """y = act(x @ w.T + b) on the "bf16x3" path (ac_linear_bf16x3: the one-tap instance of the direct kernel, scale 1,
    shift b).  x (M, K), w (N, K); results (M, N)."""
    y = x.double() @ w.double().t() + (b.double() if b is not None else 0.0)
    mag = x.double().abs() @ w.double().abs().t()
    e = split_products(w.float().reshape(1, 1, *w.shape), x.float().t().reshape(1, 1, x.shape[1], -1), ar)[0].t()
    if b is not None:
        e = (e.double() + b.double()).float()
    if relu:
        y, e = y.relu(), e.relu()
    return Case(y, e.contiguous(), mag, dict(form="linear", mode=0, cin=x.shape[1]))


# ---- the two input families -------------------------------------------------------------------------------------------
FAMILIES = ("randn", "checkpoint-like")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bn_draw(g, family, cout):
    if family == "randn":
        return torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    sc = torch.exp(torch.rand(cout, generator=g) * math.log(4 / 0.05) + math.log(0.05))   # log-uniform in [0.05, 4]
    sc = torch.where(torch.rand(cout, generator=g) < 0.2, -sc, sc)                        # about one channel in five negative
    return sc, torch.randn(cout, generator=g) * 0.1


def _weights_draw(g, family, cout, cin, taps, gain_in=None):
    w = torch.randn(cout, cin, *taps, generator=g) * math.sqrt(2.0 / (cin * taps[0] * taps[1]))
    if family == "randn":
        return w
    go = torch.exp(torch.randn(cout, generator=g))
    gi = gain_in.clamp_min(0.2) if gain_in is not None else torch.ones(cin)
    return w * go.view(-1, 1, 1, 1) / gi.view(1, -1, 1, 1)


def draw_layer(family, B, H, W, Cin, Cout, seed):
    """x (B, Cin, H, W), w OIHW, scale, shift.  "randn": what the existing kernel tests draw (unit-variance inputs, He-normal
    weights, BN scale in [0.5, 1.5)).  "checkpoint-like": inputs relu(randn + 0.5) (non-negative with a DC part, which the
    Winograd input transform has to cancel) times a per-input-channel gain exp(N(0,1)); He-normal weights times a
    per-output-channel gain exp(N(0,1)), divided by the input gain clamped at 0.2; folded BN scale log-uniform in [0.05, 4]
    with about one channel in five NEGATIVE; shift 0.1 * randn."""
    assert family in FAMILIES, family
    g = _gen(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    gain = None
    if family == "checkpoint-like":
        gain = torch.exp(torch.randn(Cin, generator=g))
        x = F.relu(x + 0.5) * gain.view(1, -1, 1, 1)
    w = _weights_draw(g, family, Cout, Cin, (3, 3), gain)
    sc, sh = _bn_draw(g, family, Cout)
    return x, w, sc, sh


def draw_block1(family, B, H, seed):
    """x (B, 1, H, 64), w1, s1, t1, w2, s2, t2.  "randn": as tests/test_gpu_wino43.py draws block 1.  "checkpoint-like": the
    input is procedural.synthetic_logmel through a bn0-like affine map (per-mel scale and shift that bring the dB values to
    O(1)), conv1 / conv2 weights and BatchNorms as in ``draw_layer`` (conv1's output plays conv2's gained input)."""
    g = _gen(seed)
    if family == "randn":
        x = torch.randn(B, 1, H, 64, generator=g)
        w1 = torch.randn(64, 1, 3, 3, generator=g) * 0.5
        s1, t1 = _bn_draw(g, family, 64)
        w2 = _weights_draw(g, family, 64, 64, (3, 3))
        s2, t2 = _bn_draw(g, family, 64)
        return x, w1, s1, t1, w2, s2, t2
    from audiocaption_amd import procedural as P
    lm = torch.from_numpy(P.synthetic_logmel(B, H, seed=seed)).transpose(1, 2)   # (B, H, 64) dB
    a0 = (torch.rand(64, generator=g) * 0.1 + 0.05)                              # 1 / sqrt(running_var): dB spread of 7 ... 20
    x = ((lm + 25.0 + torch.randn(64, generator=g) * 3.0) * a0).unsqueeze(1).contiguous()
    w1 = _weights_draw(g, family, 64, 1, (3, 3))
    s1, t1 = _bn_draw(g, family, 64)
    w2 = _weights_draw(g, family, 64, 64, (3, 3), s1.abs())
    s2, t2 = _bn_draw(g, family, 64)
    return x, w1, s1, t1, w2, s2, t2


def draw_linear(family, M, N, K, seed):
    g = _gen(seed)
    x = torch.randn(M, K, generator=g)
    gain = None
    if family == "checkpoint-like":
        gain = torch.exp(torch.randn(K, generator=g))
        x = F.relu(x + 0.5) * gain
    w = _weights_draw(g, family, N, K, (1, 1), gain).reshape(N, K) / math.sqrt(2.0)   # 1 / sqrt(K) as the linear tests draw
    b = torch.randn(N, generator=g) * (1.0 if family == "randn" else 0.1)
    return x, w, b


# ---- the acceptance criterion -----------------------------------------------------------------------------------------
def rho(a, b, mag):
    """|a - b| / mag over every element: (rms, max).  mag must be positive everywhere (asserted, not masked)."""
    assert bool((mag > 0).all()), "mag == 0 inside the compared region: a row that sees nothing but padding"
    r = (a.double() - b.double()).abs() / mag
    return float(r.pow(2).mean().sqrt()), float(r.max())


RMS_VS_EMUL, RMS_VS_EXACT, MAX_VS_EXACT = 0.25, 1.25, 2.0


def figures(got, case):
    """The three ratios tests/test_gpu_split_error.py asserts of a kernel's output ``got`` (laid out like case.exact)."""
    ke_rms, ke_max = rho(got, case.emul, case.mag)
    kx_rms, kx_max = rho(got, case.exact, case.mag)
    ex_rms, ex_max = rho(case.emul, case.exact, case.mag)
    return dict(emul_rms=ex_rms, emul_max=ex_max, kernel_vs_emul_rms=ke_rms, kernel_rms=kx_rms, kernel_max=kx_max,
                r_emul=ke_rms / ex_rms, r_rms=kx_rms / ex_rms, r_max=kx_max / ex_max)


def verdict(fig):
    """[] if the kernel is accepted, else the assertions it misses.
    1. rho(kernel, emul) rms <= 0.25 x rho(emul, exact) rms: kernel and emulation round every operand alike and differ in
       the order of f32 operations only (0.03 - 0.10 of the split error on the CPU); the smallest mutant measures 1.35.
    2. rho(kernel, exact): rms <= 1.25 x, max <= 2 x the emulation's own: the 2^-16 grade itself."""
    out = []
    if not fig["r_emul"] <= RMS_VS_EMUL:
        out.append(f"rho(kernel, emul) rms is {fig['r_emul']:.3f} x the split error's (bar {RMS_VS_EMUL})")
    if not fig["r_rms"] <= RMS_VS_EXACT:
        out.append(f"rho(kernel, exact) rms is {fig['r_rms']:.3f} x the emulation's (bar {RMS_VS_EXACT})")
    if not fig["r_max"] <= MAX_VS_EXACT:
        out.append(f"rho(kernel, exact) max is {fig['r_max']:.3f} x the emulation's (bar {MAX_VS_EXACT})")
    return out


def fmt_figures(name, fig):
    return (f"{name}: rho(emul, exact) rms {fig['emul_rms']:.3e} max {fig['emul_max']:.3e} | kernel / emul rms "
            f"{fig['r_emul']:.3f} | kernel vs exact: rms x{fig['r_rms']:.4f} max x{fig['r_max']:.3f}")


def report(line):
    """Print a figure and, when SPLIT_ERROR_REPORT names a file, append it there (how the sections of
    tests/golden/REPORT_split_error.txt are collected)."""
    print(line, flush=True)
    path = os.environ.get("SPLIT_ERROR_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
