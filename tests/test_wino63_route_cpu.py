"""Which launches of the "wino43" tier take the row-sextet form (no GPU, no library: the kernel entry points are replaced by
recorders).  The inference forward of a large uniform batch does; the forward of a training step never does, with or without
dropout - ``sextet_route`` depends on the launch's size, and a training step's gradient has to stay linear in the batch
(tests/test_gpu_fullsize.py::test_training_gradient_is_linear_in_the_batch), so a clip's features may not change form between
a batch and its halves."""
import pytest

from audiocaption_amd import cnn_encoder as C


@pytest.fixture
def calls(monkeypatch):
    seen = []
    monkeypatch.setattr(C.K, "wino43_workgroups", lambda B, Hp, W, Cout: B * (Hp // 4) * (Cout // 128))
    for name in ("conv3x3_bn_relu_wino63", "conv3x3_bn_relu_wino43", "conv3x3_bn_relu_wino1d"):
        monkeypatch.setattr(C.K, name, lambda *a, _n=name, **k: seen.append(_n))
    monkeypatch.setattr(C.K, "wino1d_splitk_floats", lambda *a: 0)
    return seen


def _launch(layer, B, **offer):
    W, Cin, Cout = layer
    pack = C.Wino43Pack("f23", "f43", None, "f63")
    C._conv_wino43(None, pack, None, None, None, B, 1024, 1001, W, Cin, Cout, 1 if Cin == Cout else 0, **offer)


@pytest.mark.parametrize("layer", sorted(C.SEXTET_LAYERS))
def test_sextets_are_for_the_inference_forward_only(calls, layer):
    big = 2 * C.SEXTET_MIN_WORKGROUPS      # workgroups of the recorder's count: well above the threshold, and its half too
    _launch(layer, big)
    _launch(layer, big, train=True)
    _launch(layer, big, train=True, dropout=(0.2, 40, 0))
    _launch(layer, big, need=(None, 32, 60))
    _launch(layer, 1)                      # a single clip: far below the threshold
    assert calls == ["conv3x3_bn_relu_wino63"] + ["conv3x3_bn_relu_wino43"] * 4


def test_a_layer_outside_the_list_stays_on_quads(calls):
    assert (8, 512, 512) not in C.SEXTET_LAYERS
    _launch((8, 512, 512), 4096)
    assert calls == ["conv3x3_bn_relu_wino43"]
