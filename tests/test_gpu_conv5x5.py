"""The 5x5 conv kernels of csrc/conv5x5.hip (through the wrappers of kernels.py) against float64 and against the CPU
emulation of their own arithmetic (tests/_cnn_small_ref.py on tests/_split_ref.py).

``conv5x5_bn_relu_bf16x3``: B = 3 clips (and one B = 1), both input families of ``_split_ref``, the three layers of Cnn6's
blocks 2-4, modes 0 and 1, two H per layer with the smallest Hp the kernel takes (even, >= H + 2: the 5x5 reads two rows beyond
a clip, and H + 1 == Hp is refused - tests/test_cnn_small_cpu.py) - odd H under the pool, tiles that span clips, partial last
tiles.  Asserted per case, as tests/test_gpu_split_error.py does for the 3x3 forms:

1. rho(kernel, emul) rms <= 0.25 x rho(emul, exact) rms;
2. rho(kernel, exact): rms <= 1.25 x and max <= 2 x the emulation's own;
3. rows at or beyond H (H / 2 of a pooled output) are zeros, exactly, in a buffer pre-filled with 7.0;
4. on randn data, max |kernel - exact| <= 1e-3 * max(1, sqrt(25 * Cin / 576)): the absolute bar of tests/test_gpu_kernels.py.

The ratios measured on an MI355X are recorded in tests/golden/REPORT_cnn_small.txt."""
import pytest
import torch

import _cnn_small_ref as R
import _split_ref as S

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cout): level-2, level-3 and level-4 shapes
SHAPES = [(3, 30, 32, 64, 128), (3, 16, 32, 64, 128), (3, 15, 16, 128, 256), (3, 8, 16, 128, 256), (3, 7, 8, 256, 512),
          (3, 4, 8, 256, 512), (1, 30, 32, 64, 128)]


@pytest.fixture(scope="module")
def K():
    from audiocaption_amd import build
    build.build()
    from audiocaption_amd import kernels
    return kernels


def _hp(H):
    return (H + 3) & ~1          # even, two zero rows at least


def _seed(*dims):
    return 11 + sum(int(d) * (i + 5) for i, d in enumerate(dims)) % 100003


_CASES = {}


def _case(family, B, H, W, Cin, Cout, mode):
    """(x, w, sc, sh, Case), computed once per case and shared."""
    key = (family, B, H, W, Cin, Cout, mode)
    if key not in _CASES:
        x, w, sc, sh = R.draw_layer5(family, B, H, W, Cin, Cout, _seed(B, H, W, Cin, Cout))
        _CASES[key] = (x, w, sc, sh, R.layer5(x, w, sc, sh, mode))
    return _CASES[key]


def _run(K, x, w, sc, sh, B, Hp, H, W, Cin, Cout, mode, rows=None):
    out = torch.full((B * Hp, W, Cout) if mode == 0 else (B * Hp // 2, W // 2, Cout), 7.0, device="cuda")
    xr = (S.to_rows(x, Hp) if rows is None else rows).cuda()
    K.conv5x5_bn_relu_bf16x3(xr, K.pack_conv5x5_weight(w.cuda()), sc.cuda(), sh.cuda(), out, B, Hp, H, W, Cin, Cout, mode)
    return out.cpu()


def _valid(out, B, rows):
    """The kernel's output buffer -> the valid rows (B, rows, W', C); the padding rows must be zeros."""
    got = out.reshape(B, -1, *out.shape[1:])
    assert torch.equal(got[:, rows:], torch.zeros_like(got[:, rows:])), "rows at or beyond H are zeros"
    return got[:, :rows]


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_conv5x5_split_error(K, B, H, W, Cin, Cout, mode, family):
    x, w, sc, sh, case = _case(family, B, H, W, Cin, Cout, mode)
    Hp = _hp(H)
    got = _valid(_run(K, x, w, sc, sh, B, Hp, H, W, Cin, Cout, mode), B, case.exact.shape[1])
    assert got.shape == case.exact.shape and bool(torch.isfinite(got).all())
    fig = S.figures(got, case)              # asserts mag > 0 over every compared element
    name = f"conv5x5 {B}x{H}(Hp {Hp})x{W} {Cin}->{Cout} mode{mode} [{family}]"
    worst = float((got.double() - case.exact).abs().max())
    R.report(S.fmt_figures("gpu " + name, fig) + f" | max|kernel - exact| {worst:.3e}")
    assert S.verdict(fig) == [], (name, S.verdict(fig))
    if family == "randn":
        assert worst <= R.abs_bar(Cin), (name, worst, R.abs_bar(Cin))


@pytest.mark.parametrize("Cin,Cout", [(64, 128), (256, 512)])
def test_pack_kernel_equals_the_torch_pack_bit_for_bit(K, Cin, Cout):
    w = torch.randn(Cout, Cin, 5, 5, generator=torch.Generator().manual_seed(Cin)) * 0.05
    w[0, 0, 0, 0], w[1, 1, 2, 2] = 0.0, 1.0 + 2.0 ** -8     # an exact zero, and a tie of the hi rounding
    got = K.pack_conv5x5_weight(w.cuda()).cpu()
    want = K.pack_conv_weight_bf16x3_frag(w)
    assert got.shape == want.shape == (Cin // 32, 25, 2, Cout // 32, 2, 64, 8)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,W,Cin,Cout", [(30, 32, 64, 128), (15, 16, 128, 256), (7, 8, 256, 512)])
def test_a_clip_does_not_read_its_neighbours_rows(K, H, W, Cin, Cout, mode):
    """Clip 1 of a 3-clip batch whose clips 0 and 2 hold values 1e4 times larger equals, within the absolute bar, the same
    clip run alone: had one row of a neighbour been read, the difference would be of the order of 1e4."""
    x, w, sc, sh = R.draw_layer5("randn", 3, H, W, Cin, Cout, _seed(H, W, Cin))
    Hp = _hp(H)
    loud = x.clone()
    loud[0] *= 1e4
    loud[2] *= 1e4
    rows = H if mode == 0 else H // 2
    alone = _valid(_run(K, x[1:2], w, sc, sh, 1, Hp, H, W, Cin, Cout, mode), 1, rows)
    among = _valid(_run(K, loud, w, sc, sh, 3, Hp, H, W, Cin, Cout, mode), 3, rows)
    d = float((among[1] - alone[0]).abs().max())
    print(f"bleed {H}x{W} {Cin}->{Cout} mode{mode}: max|among - alone| {d:.3e}")
    assert d <= R.abs_bar(Cin)


@pytest.mark.parametrize("mode", [0, 1])
def test_input_padding_rows_are_not_trusted(K, mode):
    """Staging tests every row against the clip's own H: whatever the input buffer holds in its padding rows, the result is
    the bits of the run on zero padding."""
    B, H, W, Cin, Cout = 3, 15, 16, 128, 256
    x, w, sc, sh = R.draw_layer5("randn", B, H, W, Cin, Cout, 5)
    Hp = _hp(H)
    clean = S.to_rows(x, Hp)
    dirty = clean.reshape(B, Hp, W, Cin).clone()
    dirty[:, H:] = 1e4
    a = _run(K, x, w, sc, sh, B, Hp, H, W, Cin, Cout, mode, rows=clean)
    b = _run(K, x, w, sc, sh, B, Hp, H, W, Cin, Cout, mode, rows=dirty.reshape(B * Hp, W, Cin))
    assert torch.equal(a, b)


@pytest.mark.parametrize("H", [60, 33, 16])
def test_conv5x5_first(K, H):
    """Block 1 (Cin = 1, f32 FMAs, BN + ReLU + pool in one kernel) against float64, at the tolerance tests/test_gpu_kernels.py
    holds ``conv3x3_first`` to (weights drawn at 0.3 = 0.5 * 3 / 5: the same output scale over 25 taps as its 0.5 over 9)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3 + H)
    B, W = 3, 64
    x = torch.randn(B, 1, H, W, generator=g)
    w = torch.randn(64, 1, 5, 5, generator=g) * 0.3
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    sc[::5] *= -1.0                                              # ReLU before the pool
    y = F.relu(F.conv2d(x.double(), w.double(), padding=2) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None])
    want = F.avg_pool2d(y, 2).permute(0, 2, 3, 1)               # (B, H // 2, 32, 64): an odd H loses its last row
    Hp = _hp(H)
    rows = S.to_rows(x, Hp).reshape(B, Hp, W)
    rows[:, H:] = 1e4                                            # padding rows of the input are not trusted
    out = torch.full((B * Hp // 2, 32, 64), 7.0, device="cuda")
    K.conv5x5_first(rows.reshape(B * Hp, W).cuda(), w.reshape(64, 25).cuda(), sc.cuda(), sh.cuda(), out, B, Hp, H)
    got = _valid(out.cpu(), B, H // 2)
    d = float((got.double() - want).abs().max())
    print(f"conv5x5_first H={H}: max|diff| {d:.3e} (|want| max {float(want.max()):.3e})")
    assert d < 1e-5
