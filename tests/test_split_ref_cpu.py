"""CPU checks of tests/_split_ref.py, the restatement of the split-bf16 conv tier's arithmetic that
tests/test_gpu_split_error.py holds the HIP kernels to.

* The emulation against float64, both input families, every form: rho = |emul - exact| / mag is printed (rms and max: the
  record in tests/golden/REPORT_split_error.txt that the GPU ratios are read against) and its max is held under the
  first-order componentwise bound of three-product split arithmetic (2^-15 per product, derived in _split_ref.py) - a sanity
  floor, not the sharp test.
* The acceptance criterion of the GPU tests has teeth: every mutant of the arithmetic, put in the kernel's place, is rejected
  on both families, and the faithful variants (another order of the K sum, another rounding of the input transform) pass."""
import pytest
import torch

import _split_ref as S

LAYERS = [   # form, B, H, W, Cin, Cout, mode
    ("direct", 2, 11, 16, 128, 256, 0), ("direct", 2, 13, 4, 512, 1024, 1), ("direct", 2, 7, 2, 2048, 2048, 2),
    ("wino1d", 2, 25, 8, 256, 512, 1), ("wino1d", 2, 12, 2, 2048, 2048, 2), ("wino1d", 2, 13, 4, 512, 1024, 0),
    ("wino43", 2, 21, 16, 128, 256, 0), ("wino43", 2, 13, 4, 512, 1024, 1), ("wino43", 2, 7, 2, 2048, 2048, 2),
    ("wino43", 3, 22, 32, 64, 128, 1)]


def _seed(*dims):
    return sum(int(d) * (i + 3) for i, d in enumerate(dims)) % 100003


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("form,B,H,W,Cin,Cout,mode", LAYERS)
def test_emulation_stays_under_the_componentwise_bound(form, B, H, W, Cin, Cout, mode, family):
    x, w, sc, sh = S.draw_layer(family, B, H, W, Cin, Cout, _seed(B, H, W, Cin, Cout, mode))
    case = S.layer(x, w, sc, sh, mode, form)
    assert case.exact.shape == case.emul.shape == case.mag.shape == \
        {0: (B, H, W, Cout), 1: (B, H // 2, W // 2, Cout), 2: (B, H, Cout)}[mode]
    rms, mx = S.rho(case.emul, case.exact, case.mag)
    bound = S.layer_bound(x, w, sc, mode, form)
    frac = float(((case.emul.double() - case.exact).abs() / bound).max())
    S.report(f"cpu {form} {B}x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]: rho(emul, exact) rms {rms:.3e} max {mx:.3e}; "
             f"max |emul - exact| / bound {frac:.4f}; bound / (2^-15 mag) up to {float((bound / case.mag).max() / S.EPS_PRODUCT):.2f}")
    assert frac < 1.0
    if form == "direct":
        assert mx < S.EPS_PRODUCT      # the direct form's bound IS 2^-15 mag


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("conv1", ["mfma", "valu"])
def test_block1_emulation_stays_under_the_componentwise_bound(conv1, family):
    B, H = 2, 37
    x, w1, s1, t1, w2, s2, t2 = S.draw_block1(family, B, H, 41)
    case = S.block1(x, w1, s1, t1, w2, s2, t2, conv1)
    assert case.exact.shape == (B, H // 2, 32, 64)
    rms, mx = S.rho(case.emul, case.exact, case.mag)
    frac = float(((case.emul.double() - case.exact).abs() / S.block1_bound(x, w1, s1, t1, w2, s2)).max())
    S.report(f"cpu block1/{conv1} {B}x{H} [{family}]: rho(emul, exact) rms {rms:.3e} max {mx:.3e}; max |emul - exact| / bound {frac:.4f}")
    assert frac < 1.0


def test_block1_valu_conv1_is_the_f32_chain():
    """conv1 as the fmaf chain is f32-grade: far inside the split grade of the mfma form, and not equal to it."""
    x, w1, s1, t1, *_ = S.draw_block1("randn", 1, 13, 5)
    exact = S._conv1_exact(x, w1, s1, t1)
    valu, mfma = S.conv1_emul(x, w1, s1, t1, "valu"), S.conv1_emul(x, w1, s1, t1, "mfma")
    mag = S._conv1_mag(x, w1, s1, t1)
    ev, em = float(((valu - exact).abs() / mag).max()), float(((mfma - exact).abs() / mag).max())
    print(f"conv1 max rho: valu {ev:.2e} mfma {em:.2e}")
    assert ev < 9 * 2.0 ** -24 and ev < em < S.EPS_PRODUCT


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("M,N,K,relu", [(130, 832, 1024, True), (64, 1536, 2048, False)])
def test_linear_emulation_stays_under_the_componentwise_bound(M, N, K, relu, family):
    x, w, b = S.draw_linear(family, M, N, K, _seed(M, N, K))
    case = S.linear(x, w, b, relu)
    rms, mx = S.rho(case.emul, case.exact, case.mag)
    S.report(f"cpu linear {M}x{N}x{K} [{family}]: rho(emul, exact) rms {rms:.3e} max {mx:.3e}")
    assert mx < S.EPS_PRODUCT


def test_split_follows_the_weight_packs_and_the_kernels_rounding():
    """hi / lo of the emulation are, bit for bit, what kernels.pack_conv_weight_wino43_frag stores for the filter transform
    (restated here: float64 transform, RNE twice), and RNE differs from truncation where it should."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(32, 16, 3, 3, generator=g)
    U = S.filter_transform(w, 4)                                           # (6, kx, o, c)
    hi, lo = S.split(U)
    gd = w.double()
    for p in range(6):
        u = float(S.G4[p, 0]) * gd[:, :, 0] + float(S.G4[p, 1]) * gd[:, :, 1] + float(S.G4[p, 2]) * gd[:, :, 2]   # (o, c, kx)
        h = u.to(torch.bfloat16)
        l = (u - h.double()).to(torch.bfloat16)
        assert torch.equal(hi[p], h.float().permute(2, 0, 1)) and torch.equal(lo[p], l.float().permute(2, 0, 1))
    assert float(((hi.double() + lo.double() - U).abs() / U.abs().clamp_min(1e-30)).max()) <= 2.0 ** -17
    x = torch.randn(4096, generator=g)
    th, tl = S.split(x, hi_mode="trunc", lo_mode="trunc")
    assert bool((th.abs() <= x.abs()).all()) and bool(((x - th) * x >= 0).all()) and not torch.equal(th, S.split(x)[0])
    assert float(((th + tl - x).abs() / x.abs()).max()) <= 2.0 ** -15


TEETH = [("wino43", 2, 21, 16, 128, 256, 0), ("wino43", 2, 13, 4, 512, 1024, 1), ("wino1d", 2, 21, 16, 128, 256, 1),
         ("direct", 2, 21, 16, 128, 256, 0)]


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("form,B,H,W,Cin,Cout,mode", TEETH)
def test_the_acceptance_criterion_has_teeth(form, B, H, W, Cin, Cout, mode, family):
    """Every mutant in the kernel's place is rejected by what tests/test_gpu_split_error.py asserts; the faithful variants
    are accepted with the margins the criterion was sized for."""
    x, w, sc, sh = S.draw_layer(family, B, H, W, Cin, Cout, _seed(B, H, W, Cin, Cout, mode) + 1)
    case = S.layer(x, w, sc, sh, mode, form)
    name = f"{form} {B}x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]"
    variants = {"K sum in 16-channel steps": S.Arith(chunk=16)}
    if form == "wino43":
        variants["input transform in float64, K sum in 16-channel steps"] = S.Arith(chunk=16, transform64=True)
    for vname, ar in variants.items():
        fig = S.figures(S.layer_emul(x, w, sc, sh, mode, form, ar), case)
        S.report(S.fmt_figures(f"teeth {name} faithful, {vname}", fig))
        assert S.verdict(fig) == [], (vname, fig)
        assert fig["r_emul"] <= 0.5 * S.RMS_VS_EMUL      # at most half of the bar: the other half is the kernels' margin
    accepted = []
    for mname, ar in S.mutants(Cin).items():
        fig = S.figures(S.layer_emul(x, w, sc, sh, mode, form, ar), case)
        missed = S.verdict(fig)
        S.report(S.fmt_figures(f"teeth {name} MUTANT {mname}", fig) + f" -> {'rejected' if missed else 'ACCEPTED'}")
        if not missed:
            accepted.append(mname)
    assert not accepted, accepted
