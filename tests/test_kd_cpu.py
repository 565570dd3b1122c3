"""CPU tests of token-level knowledge distillation: the float64 restatement (tests/_kd_ref.py) against what the reference's
own ``SupKdLoss(LabelSmoothingLoss(0.1), TokenLevelKdLoss(temp), w)`` computed (tests/golden/g18_kd.npz), the routing of
the reference's class paths, and the refusals that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

import _kd_ref as K


@pytest.fixture(scope="module")
def g18(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g18_kd.npz")))


def test_restatement_vs_reference_fixture(g18):
    logit, tchr = torch.from_numpy(g18["logit"]), torch.from_numpy(g18["tchr_logit"])
    tgt, tgt_len = torch.from_numpy(g18["tgt"]), torch.from_numpy(g18["tgt_len"])
    assert tuple(logit.shape) == (3, 5, 257) and tgt_len.tolist() == [5, 3, 1]
    assert g18["temps"].tolist() == [0.5, 1.0, 2.0] and g18["weights"].tolist() == [0.0, 0.5, 1.0]
    smoothing = float(g18["smoothing"])
    mask = K.valid_mask(tgt_len, 5)
    for temp in g18["temps"]:
        for w in g18["weights"]:
            want, dwant = float(g18[f"loss/{temp:g}/{w:g}"]), torch.from_numpy(g18[f"dlogit/{temp:g}/{w:g}"]).double()
            loss, sup, kd, _ = K.kd_loss(logit, tchr, tgt, tgt_len, smoothing, float(temp), float(w))
            d = K.kd_dlogit(logit, tchr, tgt, tgt_len, smoothing, float(temp), float(w))
            dv = abs(float(loss) - want) / abs(want)
            dg = float((d - dwant).abs().max()) / float(dwant.abs().max())
            print(f"temp {temp:g} w {w:g}: value {dv:.2e} gradient {dg:.2e}")
            assert dv <= 1e-6 and dg <= 1e-6
            assert float(d[~mask].abs().max()) == 0.0 and float(dwant[~mask].abs().max()) == 0.0
            assert abs(float(loss) - (w * float(sup) + (1 - w) * float(kd))) <= 1e-12 * abs(float(loss))
            # the written-out gradient is the derivative of the written-out loss
            z = logit.double().requires_grad_(True)
            (K.kd_loss(z, tchr, tgt, tgt_len, smoothing, float(temp), float(w))[0] * 3.0).backward()
            d3 = K.kd_dlogit(logit, tchr, tgt, tgt_len, smoothing, float(temp), float(w), g=3.0)
            assert float((z.grad - d3).abs().max()) <= 1e-12 * float(d3.abs().max())


def test_restatement_ignores_masked_positions(g18):
    logit, tchr = torch.from_numpy(g18["logit"]).clone(), torch.from_numpy(g18["tchr_logit"]).clone()
    tgt, tgt_len = torch.from_numpy(g18["tgt"]), torch.from_numpy(g18["tgt_len"])
    a = K.kd_loss(logit, tchr, tgt, tgt_len, 0.1, 2.0, 0.5)
    mask = K.valid_mask(tgt_len, 5)
    tchr[~mask] = float("nan")
    logit[~mask] = float("inf")
    b = K.kd_loss(logit, tchr, tgt, tgt_len, 0.1, 2.0, 0.5)
    assert all(float(x) == float(y) for x, y in zip(a, b))
    assert bool(torch.isfinite(K.kd_dlogit(logit, tchr, tgt, tgt_len, 0.1, 2.0, 0.5)).all())
    # tgt_len beyond T is clamped
    c = K.kd_loss(logit, tchr, tgt, torch.tensor([9, 3, 1]), 0.1, 2.0, 0.5)
    assert float(c[0]) == float(a[0])


def test_compat_routes_the_kd_losses():
    import audiocaption_amd.kd_loss as own
    from audiocaption_amd import compat
    saved = {k: v for k, v in sys.modules.items() if k == "captioning" or k.startswith("captioning.")}
    try:
        compat.install()
        import importlib
        mod = importlib.import_module("captioning.losses.kd_loss")
        assert mod.TokenLevelKdLoss is own.TokenLevelKdLoss and mod.SupKdLoss is own.SupKdLoss
        assert compat.HOT_CLASSES["captioning.losses.kd_loss"] == ("audiocaption_amd.kd_loss", ["TokenLevelKdLoss", "SupKdLoss"])
        # the reference's YAML ``loss:`` block resolves through the dotted paths
        from captioning.losses.loss import LabelSmoothingLoss
        fn = mod.SupKdLoss(LabelSmoothingLoss(0.1), mod.TokenLevelKdLoss(temp=2.0), sup_weight=0.3)
        assert fn.fused() and fn.kd_loss.temp == 2.0 and fn.sup_weight == 0.3
        assert not mod.SupKdLoss(LabelSmoothingLoss(0.1, reduction="sum"), mod.TokenLevelKdLoss()).fused()
    finally:
        for k in [k for k in sys.modules if k == "captioning" or k.startswith("captioning.")]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize("loss_type", ["l2", "l1"])
def test_l2_and_l1_are_refused(loss_type):
    from audiocaption_amd.kd_loss import TokenLevelKdLoss
    with pytest.raises(NotImplementedError, match="reference fails there too"):
        TokenLevelKdLoss(loss_type=loss_type)


def test_shape_mismatch_is_refused():
    from audiocaption_amd.kd_loss import SupKdLoss, TokenLevelKdLoss
    from audiocaption_amd.loss import LabelSmoothingLoss
    out = {"logit": torch.zeros(2, 3, 10), "tchr_logit": torch.zeros(2, 3, 11), "tgt": torch.zeros(2, 3, dtype=torch.int64),
           "tgt_len": torch.tensor([3, 2])}
    with pytest.raises(ValueError, match="shape"):
        TokenLevelKdLoss()(out)
    with pytest.raises(ValueError, match="shape"):
        SupKdLoss(LabelSmoothingLoss(0.1), TokenLevelKdLoss(), 0.5)(out)
    out.update(tchr_logit=torch.zeros(2, 3, 10), tgt_len=torch.tensor([0, 0]))
    with pytest.raises(ValueError, match="no valid target token"):
        TokenLevelKdLoss()(out)


def test_ctypes_row_and_build_list():
    import ctypes
    from audiocaption_amd import _lib, build
    assert "kd.hip" in build.SOURCES and _lib.ABI_VERSION == 2
    args = _lib.SIGNATURES["ac_kd_loss"][1]
    assert len(args) == 19 and args[8:12] == [ctypes.c_float] * 4 and args[16] is ctypes.c_float
