"""CPU checks of the Cnn6 / Cnn10 encoders and of the references their GPU tests use (tests/_cnn_small_ref.py).

* The float64 restatement of both forwards equals the reference's outputs in tests/golden/g28_cnn_small.npz.
* The split-bf16 emulation of the 5x5 layer stays at the 2^-16 operand grade against float64 on both input families, and the
  acceptance criterion of tests/test_gpu_conv5x5.py tells the smallest mutant apart.
* Geometry (chosen rule: ``geometry`` guarantees Hp_k >= H_k + 2 at every conv level of BOTH encoders, and the entry points of
  csrc/conv5x5.hip refuse less), constructor keys, ``load_pretrained``, refusals, compat paths, the C ABI rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _cnn_small_ref as R
import _split_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("cnn6", "cnn10")
NEW_SYMBOLS = ("ac_conv5x5_first", "ac_conv5x5_bn_relu_bf16x3", "ac_pack_conv5x5_weight_bf16x3")
LAYERS5 = [(32, 64, 128), (16, 128, 256), (8, 256, 512)]   # (W, Cin, Cout) of blocks 2-4


@pytest.fixture(scope="module")
def g28():
    return dict(np.load(R.FIXTURE))


def _cls(kind):
    import audiocaption_amd as A
    return {"cnn6": A.Cnn6Encoder, "cnn10": A.Cnn10Encoder}[kind]


def _config(kind, vocab=R.VOCAB):
    import audiocaption_amd as A
    return {"cnn6": A.cnn6rnn_trm_config, "cnn10": A.cnn10rnn_trm_config}[kind](vocab)


# ---- the restatement against the reference's outputs ----------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_float64_restatement_equals_the_fixture(g28, kind, case):
    sr, T, frames = R.CASES[case]
    lens = R.feat_len(R.wav_lens(case), sr)
    assert lens == g28[f"{kind}/{case}/attn_emb_len"].tolist()
    out = R.forward_f64(kind, R.fixture_state(kind), R.logmel(case), lens)
    assert out["attn_emb"].shape == (len(frames), T // 16, 512) and out["fc_emb"].shape == (len(frames), 512)
    # attn_emb is stored as f32 (values up to ~6: half an ulp is 2.4e-7), fc_emb as f64
    assert float((out["attn_emb"] - torch.from_numpy(g28[f"{kind}/{case}/attn_emb"]).double()).abs().max()) < 5e-7
    assert float((out["fc_emb"] - torch.from_numpy(g28[f"{kind}/{case}/fc_emb"])).abs().max()) < 1e-9
    if case == "a":
        for b in range(4):
            for k, v in R.block_digest(out["blocks"][b]).items():
                want = g28[f"{kind}/a/block{b + 1}_{k}"]
                np.testing.assert_allclose(v, want, rtol=1e-9 if want.dtype == np.float64 else 0, atol=1e-9)


def test_fixture_weights_show_the_relu_pool_order(g28):
    """One BN channel in five is negative, so pooling BEFORE the ReLU gives visibly different block outputs."""
    import torch.nn.functional as F
    st = {k: torch.as_tensor(v).double() for k, v in R.fixture_state("cnn6").items()}
    assert bool((st["conv_block2.bn1.weight"][::5] < 0).all()) and bool((st["conv_block2.bn1.weight"][1::5] > 0).all())
    right = R.forward_f64("cnn6", R.fixture_state("cnn6"), R.logmel("a"), [3, 2, 1])["blocks"]

    def bn(x, p):
        sc = st[p + ".weight"] / torch.sqrt(st[p + ".running_var"] + 1e-5)
        return x * sc[None, :, None, None] + (st[p + ".bias"] - st[p + ".running_mean"] * sc)[None, :, None, None]

    wrong = F.relu(F.avg_pool2d(bn(F.conv2d(right[0], st["conv_block2.conv1.weight"], padding=2), "conv_block2.bn1"), 2))
    assert float((wrong - right[1]).abs().max()) > 1e-2


# ---- the emulation of the 5x5 layer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("W,Cin,Cout", LAYERS5)
@pytest.mark.parametrize("mode", [0, 1])
def test_conv5x5_emulation_is_at_the_split_grade_and_the_criterion_has_teeth(W, Cin, Cout, mode, family):
    B, H = 2, {32: 9, 16: 7, 8: 5}[W]
    x, w, sc, sh = R.draw_layer5(family, B, H, W, Cin, Cout, 7 * W + mode)
    case = R.layer5(x, w, sc, sh, mode)
    assert case.exact.shape == case.emul.shape == case.mag.shape == ((B, H, W, Cout) if mode == 0 else (B, H // 2, W // 2, Cout))
    rms, mx = S.rho(case.emul, case.exact, case.mag)
    print(f"cpu conv5x5 {B}x{H}x{W} {Cin}->{Cout} mode{mode} [{family}]: rho(emul, exact) rms {rms:.3e} max {mx:.3e}")
    assert mx < S.EPS_PRODUCT                       # the direct form's componentwise bound: 2^-15 mag (see _split_ref.py)
    assert rms < 2.0 ** -18                         # ... and typically a few percent of it
    # the kernel's order of the K sum (16-channel steps, hi*lo, lo*hi, hi*hi per step) is accepted ...
    fig = S.figures(F_relu_bn(R.conv5_split(x, w, S.Arith(chunk=16)), sc, sh, mode), case)
    assert S.verdict(fig) == [] and fig["r_emul"] <= 0.5 * S.RMS_VS_EMUL, fig
    # ... and the smallest mutant (activations' lo part truncated) is not
    fig = S.figures(F_relu_bn(R.conv5_split(x, w, R.SMALLEST_MUTANT), sc, sh, mode), case)
    print(S.fmt_figures("  mutant lo = trunc(x - hi)", fig))
    assert S.verdict(fig) != [], fig


def F_relu_bn(y, sc, sh, mode):
    return S._epilogue(torch.relu(S._fma_bn(y, sc, sh)), mode)


def test_conv5x5_pack_layout_is_the_fragment_order_with_25_taps():
    """``kernels.pack_conv5x5_weight`` (a device kernel) documents the layout ``pack_conv_weight_bf16x3_frag`` gives a
    5x5 weight; pin that layout on the CPU: element [c][tap][ks][nt][plane][lane][e] is w[nt*32 + lane%32][c*32 + ks*16 +
    (lane//32)*8 + e][tap], hi / lo = RNE twice."""
    from audiocaption_amd.kernels import pack_conv_weight_bf16x3_frag
    w = torch.randn(64, 64, 5, 5, generator=torch.Generator().manual_seed(1))
    pk = pack_conv_weight_bf16x3_frag(w)
    assert pk.shape == (2, 25, 2, 2, 2, 64, 8) and pk.dtype == torch.bfloat16
    hi, lo = S.split(w)
    for (c, tap, ks, nt, lane, e) in [(0, 0, 0, 0, 0, 0), (1, 24, 1, 1, 63, 7), (0, 7, 1, 0, 37, 3), (1, 13, 0, 1, 5, 6)]:
        o, i = nt * 32 + lane % 32, c * 32 + ks * 16 + (lane // 32) * 8 + e
        assert float(pk[c, tap, ks, nt, 0, lane, e]) == float(hi[o, i, tap // 5, tap % 5])
        assert float(pk[c, tap, ks, nt, 1, lane, e]) == float(lo[o, i, tap // 5, tap % 5])


# ---- geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_geometry_keeps_two_zero_rows_and_pooling_pairs_inside_a_clip(kind):
    enc = _cls(kind)()
    for T in range(16, 261):
        t, H, Hp = enc.geometry(enc.hop_length * (T - 1))
        assert t == T and H == [T >> k for k in range(5)] and len(Hp) == 5
        for k in range(4):
            assert Hp[k] == 2 * Hp[k + 1]
            assert Hp[k] >= H[k] + 2, (T, k)            # a 5x5 conv's two rows beyond a clip are the clip's own zero rows
            assert Hp[k] % 4 == 0                        # a row quad of the F(4,3) tiers never straddles clips (Cnn10)
        assert Hp[4] >= H[4] + 1 and Hp[0] % 8 == 0
    assert enc.geometry(320 * 1000)[2] == [1024, 512, 256, 128, 64]   # ten seconds: nothing wasted on the rule


# ---- constructor, checkpoints ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_constructor_keys_and_shapes_equal_the_references(g28, kind):
    for sr in (32000, 16000):
        enc = _cls(kind)(sample_rate=sr)
        sd = enc.state_dict()
        # the generator's stand-in mel front end registers no buffers; torchaudio's registers these two, as this package does
        mel = [k for k in sd if k.startswith("melspec_extractor.")]
        assert mel == ["melspec_extractor.spectrogram.window", "melspec_extractor.mel_scale.fb"]
        sd = {k: v for k, v in sd.items() if k not in mel}
        assert list(sd.keys()) == g28[f"{kind}/keys"].tolist()
        assert [",".join(str(n) for n in v.shape) for v in sd.values()] == g28[f"{kind}/shapes"].tolist()
        assert enc.downsample_ratio == 16 and enc.fc_emb_size == 512 and enc.hop_length == sr // 100 and enc.freeze is False
    with pytest.raises(KeyError):
        _cls(kind)(sample_rate=44100)
    assert sum(p.numel() for n, p in _cls(kind)().named_parameters() if ".conv" in n) == {"cnn6": 4302400, "cnn10": 4682304}[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_load_pretrained_merges_by_key_and_shape_and_freezes_what_it_loaded(kind, tmp_path):
    from audiocaption_amd import procedural as P
    state = P.to_torch(R.fixture_state(kind))
    del state["fc1.bias"]
    state["conv_block4.bn1.weight"] = torch.zeros(7)          # wrong shape: reported, not loaded
    state["not_a_key"] = torch.zeros(1)
    path = str(tmp_path / "ckpt.pth")
    torch.save({"model": state}, path)
    said = []
    for freeze in (False, True):
        enc = _cls(kind)(freeze=freeze)
        before = enc.conv_block4.bn1.weight.detach().clone()
        enc.load_pretrained(path, said.append)
        assert torch.equal(enc.conv_block2.conv1.weight, state["conv_block2.conv1.weight"])
        assert torch.equal(enc.conv_block4.bn1.weight, before)
        grads = {n: p.requires_grad for n, p in enc.named_parameters()}
        if freeze:
            assert not grads["conv_block1.conv1.weight"] and not grads["fc1.weight"]
            assert grads["fc1.bias"] and grads["conv_block4.bn1.weight"]
        else:
            assert all(grads.values())
    assert "not_a_key" in said[0] and "conv_block4.bn1.weight" in said[0]
    torch.save({"state_dict": state}, path)
    with pytest.raises(Exception, match="checkpoint format"):
        _cls(kind)().load_pretrained(path, said.append)


def test_procedural_states_are_seeded_by_name_and_fit_the_configs():
    import audiocaption_amd as A
    from audiocaption_amd import procedural as P
    a, b = P.cnn6_state(), P.cnn6_state("encoder.cnn.")
    assert all(np.array_equal(a[k], P.cnn6_state()[k]) for k in a)
    assert not np.array_equal(a["conv_block2.conv1.weight"], b["encoder.cnn.conv_block2.conv1.weight"])
    assert P.cnn10_state()["conv_block3.conv2.weight"].shape == (256, 256, 3, 3) and a["conv_block3.conv1.weight"].shape == (256, 128, 5, 5)
    for kind in KINDS:
        model = A.init_model_from_config(_config(kind), print_fn=lambda s: None)
        model.load_state_dict(P.to_torch(R.fixture_model_state(kind, P.BASE_SEED)), strict=True)
        assert type(model.encoder.cnn) is _cls(kind) and model.encoder.rnn.embed_dim == 512


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_encoder_refusals_come_before_any_launch(kind):
    enc = _cls(kind)()
    wav = torch.zeros(2, 320 * 59)
    with pytest.raises(NotImplementedError, match=f"{_cls(kind).__name__} \\(HIP path\\)"):
        enc({"wav": wav, "wav_len": [320 * 59] * 2})            # a fresh module is in train mode
    enc.eval()
    with pytest.raises(ValueError, match="shorter than one"):
        enc({"wav": torch.zeros(1, 320 * 14), "wav_len": [320 * 14]})   # 15 frames
    with pytest.raises(ValueError, match="shorter than one"):
        enc.geometry(320 * 14)
    assert enc.geometry(320 * 15)[1][4] == 1
    if kind == "cnn6":
        for algo in ("wino43", "bf16x3", "direct"):
            with pytest.raises(ValueError, match="5x5"):
                enc({"wav": wav, "wav_len": [320 * 59] * 2, "conv_algo": algo})
        assert enc.effective_algo(None) == enc.effective_algo("conv5x5") == "conv5x5"
    else:
        with pytest.raises(ValueError, match="unknown conv_algo"):
            enc({"wav": wav, "wav_len": [320 * 59] * 2, "conv_algo": "conv5x5"})
        assert enc.effective_algo("f16x2") == "bf16x3" and enc.effective_algo("wino1d") == "wino1d"


@pytest.mark.parametrize("kind", KINDS)
def test_the_training_entry_points_name_the_encoder_they_refuse(kind):
    import audiocaption_amd as A
    from audiocaption_amd import kd_wrapper as W
    from audiocaption_amd.train import TrainEngine
    from audiocaption_amd.train_attn_gru import AttnGruTrainEngine
    import _attn_gru_train_ref as G
    name = _cls(kind).__name__
    model = A.init_model_from_config(_config(kind), print_fn=lambda s: None)
    assert model.encoder.freeze_cnn_bn                          # the recipe the engine would otherwise accept
    with pytest.raises(NotImplementedError, match=name):
        TrainEngine(model)
    with pytest.raises(NotImplementedError, match=name):
        model({"mode": "train", "wav": torch.zeros(1, 320 * 59), "wav_len": [320 * 59], "cap": torch.zeros(1, 4).long(),
               "cap_len": [4], "ss_ratio": 1.0})
    amodel = A.Seq2SeqAttnModel(model.encoder, A.rnn_decoder.BahAttnCatFcDecoder(dropout=0.0, **G.PUB))
    with pytest.raises(NotImplementedError, match=name):
        AttnGruTrainEngine(amodel)
    wrapper = W.ContraEncoderKdWrapper(model, 16, 12)
    with pytest.raises(NotImplementedError, match=name):
        wrapper({"mode": "train", "tchr_output": {"embedding": torch.zeros(1, 12)}})


# ---- plugin paths and the C ABI ------------------------------------------------------------------------------------------------
def test_compat_install_resolves_the_reference_paths_of_both_encoders():
    import importlib
    import sys
    import audiocaption_amd as A
    from audiocaption_amd import compat, config
    saved = {k: v for k, v in sys.modules.items() if k.startswith("captioning")}
    try:
        compat.install()
        mod = importlib.import_module("captioning.models.cnn_encoder")
        assert mod.Cnn6Encoder is A.Cnn6Encoder and mod.Cnn10Encoder is A.Cnn10Encoder and mod.Cnn14Encoder is A.Cnn14Encoder
    finally:
        for k in [k for k in sys.modules if k.startswith("captioning")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert config.get_cls_from_str("captioning.models.cnn_encoder.Cnn6Encoder") is A.Cnn6Encoder
    assert config.get_cls_from_str("captioning.models.cnn_encoder.Cnn10Encoder") is A.Cnn10Encoder


def test_header_ctypes_rows_and_build_list_of_the_new_entry_points():
    from audiocaption_amd import _lib, build
    assert "conv5x5.hip" in build.SOURCES
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ac_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body))
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in protos, name
        res, want = _lib.SIGNATURES[name]
        args = [a.strip() for a in protos[name].split(",")]
        assert res is ctypes.c_int and len(args) == len(want), name
        for a, t in zip(args, want):
            assert t is (ctypes.c_void_p if "*" in a else ctype[a.split()[0]]), (name, a)


def test_entry_points_refuse_bad_geometry_without_a_gpu():
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ok5 = dict(B=1, Hp=8, H=6, W=16, Cin=64, Cout=128, mode=1)

    def conv(**kw):
        a = dict(ok5, **kw)
        return lib.ac_conv5x5_bn_relu_bf16x3(one, one, one, one, one, a["B"], a["Hp"], a["H"], a["W"], a["Cin"], a["Cout"],
                                             a["mode"], None)

    assert lib.ac_conv5x5_bn_relu_bf16x3(None, one, one, one, one, 1, 8, 6, 16, 64, 128, 1, None) == _lib.AC_ERR_ARG
    for bad in (dict(Hp=7, H=5), dict(H=7), dict(Hp=6, H=5), dict(W=4), dict(W=64), dict(Cin=48), dict(Cout=64), dict(mode=2),
                dict(B=0), dict(H=0)):
        assert conv(**bad) == _lib.AC_ERR_ARG, bad               # H + 1 == Hp is refused: the 5x5 needs two zero rows
    assert lib.ac_conv5x5_first(one, one, one, one, one, 1, 7, 5, None) == _lib.AC_ERR_ARG
    assert lib.ac_conv5x5_first(one, one, one, one, one, 1, 6, 5, None) == _lib.AC_ERR_ARG
    assert lib.ac_conv5x5_first(one, None, one, one, one, 1, 8, 5, None) == _lib.AC_ERR_ARG
    assert lib.ac_pack_conv5x5_weight_bf16x3(one, one, 48, 128, None) == _lib.AC_ERR_ARG
    assert lib.ac_pack_conv5x5_weight_bf16x3(one, None, 64, 128, None) == _lib.AC_ERR_ARG
