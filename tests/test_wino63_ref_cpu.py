"""F(6,3) along time on the CPU: the matrices that tests/_wino63_ref.py registers next to ``_split_ref.XF`` reproduce conv2d,
and the split-operand emulation of the row-sextet form of the F(4,3) conv kernel stays inside the componentwise bound
``_split_ref.layer_bound`` gives for m = 6 (no GPU, no library)."""
import pytest
import torch
import torch.nn.functional as F

import _split_ref as S
import _wino63_ref as R6


def test_f63_is_registered_next_to_the_other_forms():
    assert S.FORM_M["wino63"] == 6 and tuple(S.XF[6][0].shape) == (8, 8) and tuple(S.XF[6][1].shape) == (8, 3) \
        and tuple(S.XF[6][2].shape) == (6, 8)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 13, 8, 16, 8), (1, 6, 4, 8, 8), (3, 7, 5, 4, 4)])
def test_f63_matrices_reproduce_conv2d_in_f64(B, H, W, Cin, Cout):
    """A^T ((G g) . (B^T d)) = conv: exact in exact arithmetic, so in float64 the difference is rounding - a few 2^-53 of
    the transform-aware magnitude (the sum of the absolute terms), which is what it is held to."""
    g = torch.Generator().manual_seed(B + H + W)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    got = S.conv_wino_f64(x, w, 6)
    want = F.conv2d(x, w, padding=1)
    mag = S.conv_wino_f64(x, w, 6, absolute=True)
    r = float(((got - want).abs() / mag).max())
    print(f"F(6,3) vs conv2d in f64: max |diff| {float((got - want).abs().max()):.3e}, {r / 2.0 ** -53:.1f} x 2^-53 of the magnitude")
    assert r < 64 * 2.0 ** -53      # 3 * Cin terms per position, 8 positions, three matrix products: far below it
    # the factored f32 transforms of the kernel are the same matrices
    d = [torch.randn(5, generator=g) for _ in range(8)]
    v = torch.stack(R6.in_transform(d), 0).double()
    assert torch.allclose(v, torch.einsum("pr,rn->pn", R6.BT6, torch.stack(d, 0).double()), rtol=0, atol=1e-5)
    M = [torch.randn(5, generator=g) for _ in range(8)]
    y = torch.stack(R6.out_transform(M), 0).double()
    assert torch.allclose(y, torch.einsum("ap,pn->an", R6.AT6, torch.stack(M, 0).double()), rtol=0, atol=1e-4)


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("mode", [0, 1])
def test_f63_emulation_is_inside_the_bound_for_m6(family, mode):
    """One layer, Cin 32 -> Cout 128 (two K steps of the kernel), H not a multiple of 6: |emul - exact| <= the bound of
    ``_split_ref.layer_bound`` for m = 6, componentwise; and, for scale, its rms error against F(4,3)'s on the same data."""
    B, H, W, Cin, Cout = 2, 13, 8, 32, 128
    x, w, sc, sh = S.draw_layer(family, B, H, W, Cin, Cout, 63 + mode)
    exact, mag = S.layer_exact(x, w, sc, sh, mode)
    emul = R6.layer_emul(x, w, sc, sh, mode)
    bound = S.layer_bound(x, w, sc, mode, "wino63")
    err = (emul.double() - exact).abs()
    worst = float((err / bound).max())
    e6 = S.rho(emul, exact, mag)
    e4 = S.rho(S.layer_emul(x, w, sc, sh, mode, "wino43"), exact, mag)
    print(f"[{family}, mode {mode}] F(6,3) emulation: max |err| / bound {worst:.3f}; rho rms {e6[0]:.3e} max {e6[1]:.3e} "
          f"(F(4,3): rms {e4[0]:.3e} max {e4[1]:.3e})")
    assert bool((err <= bound).all()), worst
    # the same on the stacked signal (sextets straddling the clips of Hp = 16: the kernel's own tiling)
    Hp = 16
    err_s = (R6.stacked_emul(x, w, sc, sh, mode, Hp).double() - exact).abs()
    assert bool((err_s <= R6.stacked_bound(x, w, sc, mode, Hp)).all())
