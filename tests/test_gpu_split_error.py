"""The split-bf16 conv kernels held to the error their arithmetic predicts (through the wrappers of kernels.py).

Every split-bf16 conv form the default tier can reach - F(4,3) (csrc/conv3x3_wino43.hip), conv block 1 in one kernel
(csrc/conv3x3_block1_w4.hip), F(2,3) with its K-sliced entry (csrc/conv3x3_wino1d.hip), the weight-streaming direct form
(csrc/conv3x3_skinny.hip), the direct "gw" kernel and its one-tap linear instance (csrc/conv3x3.hip) - on two seeded input
families (tests/_split_ref.py: "randn", what the absolute-bar tests draw, and "checkpoint-like": non-negative inputs with a
DC part, channel gains over a decade, BN scales over two decades with one channel in five NEGATIVE).  The references are
the float64 result and the CPU emulation of the tier's own arithmetic; errors are rho = |a - b| / mag with
mag = |scale| * conv3x3(|x|, |w|): no unit, indifferent to the scale of the data.  Asserted per case:

1. rho(kernel, emul) rms <= 0.25 x rho(emul, exact) rms.  Kernel and emulation round every operand alike and differ in the
   order of f32 operations only (0.03 - 0.10 of the split error between faithful variants on the CPU); the smallest mutant,
   the activations' lo part truncated instead of rounded, measures 1.35 (tests/test_split_ref_cpu.py).
2. rho(kernel, exact): rms <= 1.25 x and max <= 2 x the emulation's own - the 2^-16 grade itself, on checkpoint-like data and
   under negative BN scales too.
3. Rows at or beyond H are zeros (compared for equality); inside H nothing is masked: mag > 0 everywhere is asserted.

The ratios measured on an MI355X are recorded in tests/golden/REPORT_split_error.txt.  The float64 references are the slow
part: each is computed once per (shape, family) and shared by the tile-count / block-map variants of the launch."""
import pytest
import torch

import _split_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from audiocaption_amd import build
    build.build()
    from audiocaption_amd import kernels
    return kernels


def _seed(*dims):
    return 7 + sum(int(d) * (i + 5) for i, d in enumerate(dims)) % 100003


def _layer_case(form, family, B, H, W, Cin, Cout, mode):
    x, w, sc, sh = S.draw_layer(family, B, H, W, Cin, Cout, _seed(B, H, W, Cin, Cout, mode))
    return x, w, sc, sh, S.layer(x, w, sc, sh, mode, form)


def _hp4(H):
    return (H + 4) & ~3          # multiple of 4, at least one zero row


def _hp2(H):
    return H + 1 + ((H + 1) % 2)   # even, at least one zero row


def _out_buffer(B, Hp, H, W, Cout, mode):
    shape = {0: (B * Hp, W, Cout), 1: (B * Hp // 2, W // 2, Cout), 2: (B, H, Cout)}[mode]
    return torch.full(shape, 7.0, device="cuda")


def _valid(out, case, B):
    """The kernel's output buffer -> the valid rows, laid out like case.exact; the padding rows must be zeros."""
    got = out.cpu().reshape(B, -1, *case.exact.shape[2:])
    rows = case.exact.shape[1]
    assert got.shape[1] >= rows
    assert torch.equal(got[:, rows:], torch.zeros_like(got[:, rows:])), "rows at or beyond H are zeros"
    return got[:, :rows]


def _hold(name, got, case):
    assert got.shape == case.exact.shape, (got.shape, case.exact.shape)
    assert bool(torch.isfinite(got).all())
    fig = S.figures(got, case)              # asserts mag > 0 over every compared element
    S.report(S.fmt_figures("gpu " + name, fig))
    missed = S.verdict(fig)
    assert not missed, (name, missed)


# ---- F(4,3) -----------------------------------------------------------------------------------------------------------
W43 = [(3, 21, 32, 64, 128, 0),      # conv1 of block 2: H not a multiple of 4, four K steps (half-size workgroups by default)
       (3, 18, 16, 256, 256, 1),     # conv2 of block 3 with the pool, H % 4 == 2
       (6, 13, 4, 1024, 1024, 1),    # conv2 of block 5: a workgroup's 16 quads span four clips of Hp = 16; odd H under the pool
       (5, 10, 8, 256, 512, 0),      # conv1 of block 4: a workgroup's quads span clips
       (5, 7, 2, 1024, 2048, 0),     # block 6 (column tiles), conv1
       (5, 7, 2, 2048, 1024, 2)]     # block 6, conv2's K = 18432 with the mean over the two mel columns (half its channels)


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("B,H,W,Cin,Cout,mode", W43)
def test_wino43_split_error(K, B, H, W, Cin, Cout, mode, family):
    x, w, sc, sh, case = _layer_case("wino43", family, B, H, W, Cin, Cout, mode)
    Hp = _hp4(H)
    xr, wp, scd, shd = S.to_rows(x, Hp).cuda(), K.pack_conv_weight_wino43_frag(w.cuda()), sc.cuda(), sh.cuda()
    for tiles in ((1, 2) if W != 2 else (0,)):          # W = 2: column tiles, always two per wave
        for map_mode in (-1, 0):
            out = _out_buffer(B, Hp, H, W, Cout, mode)
            K.conv3x3_bn_relu_wino43(xr, wp, scd, shd, out, B, Hp, H, W, Cin, Cout, mode, map_mode, tiles_per_wave=tiles)
            _hold(f"wino43 x{tiles} map{map_mode} {B}x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]", _valid(out, case, B), case)


# ---- conv block 1 in one kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("B,H", [(3, 37), (1, 1001)])
def test_block1_split_error(K, B, H, family):
    """Both forms of conv1: a split-bf16 product on the matrix cores ("mfma", the default) and the f32 chain ("valu")."""
    x, w1, s1, t1, w2, s2, t2 = t = S.draw_block1(family, B, H, _seed(B, H))
    exact_mag = S.block1_exact(*t)
    Hp = (H + 8) & ~7
    x0 = torch.zeros(B, Hp, 64)
    x0[:, :H] = x[:, 0]
    x0, wp = x0.reshape(B * Hp, 64).cuda(), K.pack_conv_weight_wino43_frag(w2.cuda())
    for conv1 in ("mfma", "valu"):
        case = S.block1(*t, conv1=conv1, exact_mag=exact_mag)
        out = torch.full((B * Hp // 2, 32, 64), 7.0, device="cuda")
        K.conv3x3_block1_wino43(x0, w1.reshape(64, 9).contiguous().cuda(), s1.cuda(), t1.cuda(), wp, s2.cuda(), t2.cuda(), out, B, Hp,
                                H, conv1=conv1)
        _hold(f"block1/{conv1} {B}x{H} [{family}]", _valid(out, case, B), case)


# ---- F(2,3): blocks 4 - 6 of the 16 x 4 s default route ---------------------------------------------------------------
W1D = [(3, 50, 8, 256, 512, 0, False), (3, 50, 8, 512, 512, 1, False), (3, 25, 4, 512, 1024, 0, False),
       (3, 25, 4, 1024, 1024, 1, False), (3, 12, 2, 1024, 2048, 0, False),
       (3, 12, 2, 2048, 2048, 2, True)]       # ... and its first clip alone through the workspace= (K-sliced) entry


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("B,H,W,Cin,Cout,mode,sliced", W1D)
def test_wino1d_split_error(K, B, H, W, Cin, Cout, mode, sliced, family):
    x, w, sc, sh, case = _layer_case("wino1d", family, B, H, W, Cin, Cout, mode)
    Hp = _hp2(H)
    xr, wp, scd, shd = S.to_rows(x, Hp).cuda(), K.pack_conv_weight_wino1d_frag(w.cuda()), sc.cuda(), sh.cuda()
    out = _out_buffer(B, Hp, H, W, Cout, mode)
    K.conv3x3_bn_relu_wino1d(xr, wp, scd, shd, out, B, Hp, H, W, Cin, Cout, mode)
    _hold(f"wino1d {B}x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]", _valid(out, case, B), case)
    if sliced:
        floats = K.wino1d_splitk_floats(1, Hp, W, Cin, Cout)
        assert floats >= 2 * Hp * W * Cout, "a single clip of this layer is meant to run K-sliced"
        ws = torch.full((floats,), float("nan"), device="cuda")
        one = _out_buffer(1, Hp, H, W, Cout, mode)
        K.conv3x3_bn_relu_wino1d(xr[:Hp].contiguous(), wp, scd, shd, one, 1, Hp, H, W, Cin, Cout, mode, workspace=ws)
        _hold(f"wino1d K-sliced 1x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]", _valid(one, case.clips(1), 1), case.clips(1))


# ---- the direct forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("B,H,W,Cin,Cout,mode", [(2, 25, 4, 1024, 1024, 1), (4, 12, 2, 1024, 2048, 0), (4, 12, 2, 2048, 2048, 2)])
def test_skinny_split_error(K, B, H, W, Cin, Cout, mode, family):
    from audiocaption_amd import cnn_encoder as CE
    x, w, sc, sh, case = _layer_case("direct", family, B, H, W, Cin, Cout, mode)
    Hp = _hp4(H)
    assert B * Hp * W <= CE.SKINNY_MAX_PX
    n = K.skinny_workspace_floats(B, Hp, W, Cin, Cout)
    assert n > 0
    out = _out_buffer(B, Hp, H, W, Cout, mode)
    K.conv3x3_bn_relu_skinny(S.to_rows(x, Hp).cuda(), K.pack_conv_weight_bf16x3_frag(w.cuda()), sc.cuda(), sh.cuda(), out, B, Hp, H, W,
                             Cin, Cout, mode, torch.empty(n, device="cuda"))
    _hold(f"skinny {B}x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]", _valid(out, case, B), case)


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("B,H,W,Cin,Cout,mode", [(2, 11, 16, 128, 256, 0), (3, 6, 4, 1024, 1024, 1)])
def test_bf16x3_gw_split_error(K, B, H, W, Cin, Cout, mode, family):
    x, w, sc, sh, case = _layer_case("direct", family, B, H, W, Cin, Cout, mode)
    Hp = _hp2(H)
    out = _out_buffer(B, Hp, H, W, Cout, mode)
    K.conv3x3_bn_relu_bf16x3_gw(S.to_rows(x, Hp).cuda(), K.pack_conv_weight_bf16x3_frag(w.cuda()), sc.cuda(), sh.cuda(), out, B, Hp, H,
                                W, Cin, Cout, mode)
    _hold(f"bf16x3_gw {B}x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]", _valid(out, case, B), case)


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("M,N,K_,relu", [(1984, 1536, 2048, False),      # the GRU input projection
                                         (131, 832, 1024, True)])       # a ragged M
def test_linear_bf16x3_split_error(K, M, N, K_, relu, family):
    x, w, b = S.draw_linear(family, M, N, K_, _seed(M, N, K_))
    case = S.linear(x, w, b, relu)
    assert K.LINEAR_ALGO == "bf16x3" and N * K_ >= 1536 * 512 and K_ % 32 == 0 and N % 64 == 0, "the split path's own conditions"
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    got = K.linear(xd, wd, bd, relu=relu)
    saved, K.LINEAR_ALGO = K.LINEAR_ALGO, "f32"
    try:
        f32 = K.linear(xd, wd, bd, relu=relu)
    finally:
        K.LINEAR_ALGO = saved
    assert not torch.equal(f32, got), "the split-bf16 path ran above, not the exact-f32 GEMM"
    _hold(f"linear {M}x{N}x{K_}{' relu' if relu else ''} [{family}]", got.cpu(), case)
