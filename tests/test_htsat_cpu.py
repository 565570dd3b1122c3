"""CPU tests of the HTS-AT encoder (audiocaption_amd.htsat.Htsat): the float64 restatement tests/_htsat_ref.py against the
reference's own float64 run (tests/golden/g_htsat.npz, made by tests/golden/make_golden_htsat.py), the bicubic helper
against torch, and the plugin surface of the class - state-dict keys, construction from the reference's dotted path,
refused arguments, the checkpoint hook - none of which needs a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _htsat_ref as R  # noqa: E402

import audiocaption_amd as A  # noqa: E402
from audiocaption_amd import _lib, build, compat, config, procedural as P  # noqa: E402
from audiocaption_amd.htsat import Htsat, htsat_feat_len, relative_position_index, shifted_window_mask  # noqa: E402

CASES = {"t1001": (2, 1001), "t1024": (1, 1024)}
OUTPUTS = ["attn_emb", "fc_emb", "layer_0", "layer_1", "layer_2", "layer_3"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g_htsat.npz"))


@pytest.fixture(scope="module")
def restated():
    """The restatement's forward of both golden cases, computed once."""
    state = P.to_torch(P.htsat_state())
    out = {}
    for case, (B, T) in CASES.items():
        lms = torch.from_numpy(P.synthetic_logmel(B, T)).transpose(1, 2).contiguous()
        x = R.bn0(state, lms)
        out[case] = dict(R.forward(state, x), image=R.fold(R.bicubic_time(x)))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_vs_reference_float64(golden, restated, case):
    """The reference ran in float64 (see the generator), so every stored array is held to 1e-9 of its maximum."""
    got = restated[case]
    arrays = {k: got[k] for k in OUTPUTS}
    arrays["corner"], arrays["corner_fold"] = got["image"][:, :8, :8], got["image"][:, 62:66, 252:256]
    for k, tok in enumerate(got["tokens"]):
        idx = golden[f"{case}/tok{k}_idx"].astype(np.int64)
        arrays[f"tok{k}_val"] = tok[idx[:, 0], idx[:, 1], idx[:, 2]]
    assert len(got["tokens"]) == 5
    for name, mine in arrays.items():
        want = torch.from_numpy(golden[f"{case}/{name}"])
        assert mine.shape == want.shape, name
        d = float((mine - want).abs().max() / want.abs().max())
        print(f"{case} {name}: {d:.2e}")
        assert d < 1e-9, (case, name, d)


@pytest.mark.parametrize("T", [33, 1001, 1023])
def test_bicubic_helper_vs_torch(T):
    x = torch.from_numpy(P.synthetic_logmel(2, T, seed=5)).double().transpose(1, 2).contiguous()    # (B, T, 64)
    want = torch.nn.functional.interpolate(x[:, None], (1024, 64), mode="bicubic", align_corners=True)[:, 0]
    got = R.bicubic_time(x)
    assert got.shape == (2, 1024, 64)
    assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    taps = R.cubic_taps(torch.linspace(0, 1, 17, dtype=torch.float64)[:-1])
    assert float((taps.sum(-1) - 1).abs().max()) < 1e-14     # the four weights of any fraction sum to one
    assert torch.equal(R.bicubic_time(x[:, :1].expand(2, 1024, 64)), x[:, :1].expand(2, 1024, 64))


def test_state_dict_keys_and_shapes_are_the_references(golden):
    own = {k: ",".join(map(str, v.shape)) for k, v in Htsat().state_dict().items()}
    mel = {k for k in own if k.startswith("melspec_extractor.")}
    # torchaudio's MelSpectrogram registers these two; the generator's stand-in for it registers none
    assert mel == {"melspec_extractor.spectrogram.window", "melspec_extractor.mel_scale.fb"}
    ref = dict(zip(golden["state_keys"].tolist(), golden["state_shapes"].tolist()))
    assert [k for k in own if k not in mel] == list(ref)
    assert {k: v for k, v in own.items() if k not in mel} == ref
    assert own["layers.0.blocks.1.attn_mask"] == "64,64,64" and "layers.3.blocks.1.attn_mask" not in own
    assert set(P.htsat_state()) == {k for k in ref if not k.endswith(("attn_mask", "relative_position_index"))}


def test_constructor_buffers_vs_restatement():
    """``relative_position_index`` and ``attn_mask`` against the restatement's own index arithmetic."""
    table = torch.arange(225 * 2, dtype=torch.float64).view(225, 2)
    got = table[relative_position_index().reshape(-1)].view(64, 64, 2).permute(2, 0, 1)
    assert torch.equal(got, R.relative_bias(table))
    for H in (16, 64):
        ids = R.region_ids(H, H, 4).view(H // 8, 8, H // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
        want = (ids[:, :, None] != ids[:, None, :]).float() * -100.0
        assert torch.equal(shifted_window_mask(H, H), want)
    assert int((shifted_window_mask(16, 16) != 0).sum()) > 0 and len(set(R.region_ids(16, 16, 4).reshape(-1).tolist())) == 9


def test_builds_from_the_references_dotted_path():
    compat.install()
    enc = config.init_obj_from_dict({"type": "captioning.models.transformer_encoder.Htsat", "args": {"sample_rate": 16000}})
    assert type(enc) is Htsat and enc.hop_length == 160 and enc.fc_emb_size == 768
    import importlib
    assert importlib.import_module("captioning.models.transformer_encoder").Htsat is Htsat
    model = A.init_model_from_config(A.htsat_trm_config(100, depths=(1, 1, 1, 1)), print_fn=lambda s: None)
    assert type(model.encoder) is Htsat and type(model).__name__ == "TransformerModel"
    state = P.to_torch(P.htsat_trm_state(100, depths=(1, 1, 1, 1)))
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith(("attn_mask", "relative_position_index", "spectrogram.window", "mel_scale.fb"))
                                  for k in missing)


REFUSED = {"sample_rate": 44100, "spec_size": 224, "patch_size": 8, "patch_stride": (2, 2), "in_chans": 3, "embed_dim": 128,
           "depths": [2, 2, 6], "num_heads": [3, 6, 12, 24], "window_size": 7, "mlp_ratio": 2.0, "qkv_bias": False,
           "qk_scale": 0.5, "norm_layer": torch.nn.Identity, "ape": True, "patch_norm": False, "norm_before_mlp": "bn"}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_argument_raises_with_its_name(name):
    with pytest.raises(NotImplementedError, match=name):
        Htsat(**{name: REFUSED[name]})


def test_accepted_arguments():
    enc = Htsat(depths=[1, 2, 1, 1], freeze=True, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.3, use_checkpoint=True)
    assert [len(l.blocks) for l in enc.layers] == [1, 2, 1, 1] and not any(p.requires_grad for p in enc.parameters())
    assert [b.shift_size for l in Htsat().layers for b in l.blocks] == [0, 4, 0, 4, 0, 4, 0, 4, 0, 4, 0, 0]


def test_train_mode_and_frame_limits_raise():
    enc = Htsat(depths=[1, 1, 1, 1])
    wav = torch.zeros(1, 320 * 100)
    with pytest.raises(NotImplementedError, match="inference only"):
        enc.train()({"wav": wav, "wav_len": [wav.shape[1]], "specaug": False})
    enc.eval()
    with pytest.raises(ValueError, match="1025 frames"):
        enc({"wav": torch.zeros(1, 320 * 1024), "wav_len": [320 * 1024], "specaug": False})
    with pytest.raises(ValueError, match="shorter than one output frame"):
        enc({"wav": torch.zeros(1, 320 * 30), "wav_len": [320 * 30], "specaug": False})
    with pytest.raises(_lib.HipLibraryError):     # a valid length on the CPU: no fallback
        enc({"wav": wav, "wav_len": [wav.shape[1]], "specaug": False})


def test_feat_len():
    assert htsat_feat_len([320000, 256000, 176000], 320).tolist() == [31, 25, 17]
    assert R.feat_len([320000, 256000, 176000]).tolist() == [31, 25, 17]
    got = htsat_feat_len(torch.tensor([327360, 10240]), 320)
    assert got.tolist() == [32, 1] and got.dtype == torch.int64 and got.device.type == "cpu"


def test_load_pretrained_wavcaps_layout(tmp_path):
    depths = (1, 1, 1, 1)
    state = P.to_torch(P.htsat_state(depths=depths))
    del state["norm.weight"]
    ckpt = {"model": {"encoder.audio_enc." + k: v for k, v in state.items()}}
    ckpt["model"]["text_encoder.w"] = torch.zeros(3)
    ckpt["model"]["encoder.audio_enc.patch_embed.proj.bias"] = torch.zeros(7)      # wrong shape: reported, not loaded
    path = str(tmp_path / "wavcaps.pt")
    torch.save(ckpt, path)
    enc = Htsat(depths=list(depths))
    before = enc.patch_embed.proj.bias.detach().clone()
    said = []
    enc.load_pretrained(path, said.append)
    assert torch.equal(enc.layers[2].blocks[0].mlp.fc1.weight, state["layers.2.blocks.0.mlp.fc1.weight"])
    assert torch.equal(enc.patch_embed.proj.bias, before) and "patch_embed.proj.bias" in said[0]
    grads = {n: p.requires_grad for n, p in enc.named_parameters()}
    assert grads["norm.weight"] and grads["patch_embed.proj.bias"] and not grads["norm.bias"]
    assert sum(grads.values()) == 2
    for bad in ({"state_dict": {}}, {"model": {"audio_encoder.x": torch.zeros(1)}}, {"model": {}}):
        torch.save(bad, path)
        with pytest.raises(ValueError, match="WavCaps"):
            enc.load_pretrained(path, said.append)


def test_new_entry_points_refuse_what_they_do_not_cover():
    """Rejected before any HIP call, so this runs without a GPU: null pointers and geometries outside the kernels."""
    build.build()
    lib = _lib.load()
    p = 4096     # any non-null, 16-byte aligned address: nothing is dereferenced on these paths
    E = _lib.AC_ERR_ARG
    assert lib.ac_htsat_patch_embed(None, 1, 64, p, p, p, p, p, 96, None) == E
    assert lib.ac_htsat_patch_embed(p, 1, 1025, p, p, p, p, p, 96, None) == E      # more than 1024 frames
    assert lib.ac_htsat_patch_embed(p, 1, 0, p, p, p, p, p, 96, None) == E
    assert lib.ac_htsat_patch_embed(p, 1, 64, p, p, p, p, p, 320, None) == E         # more channels than a wave holds
    assert lib.ac_swin_window_attn(p, p, None, 1, 16, 16, 48, 2, 0, None) == E
    assert lib.ac_swin_window_attn(p, p, p, 1, 16, 16, 64, 2, 0, None) == E                   # head width 32
    assert lib.ac_swin_window_attn(p, p, p, 1, 12, 16, 48, 2, 0, None) == E                   # H not a multiple of the window
    assert lib.ac_swin_window_attn(p, p, p, 1, 16, 20, 48, 2, 0, None) == E
    assert lib.ac_swin_window_attn(p, p, p, 1, 16, 16, 48, 2, 8, None) == E                   # shift outside the window
    assert lib.ac_swin_window_attn(p, p, p, 1, 8, 8, 48, 2, 4, None) == E                     # one window cannot be shifted
    assert lib.ac_swin_patch_merge(p, None, p, p, 1, 16, 16, 48, None) == E
    assert lib.ac_swin_patch_merge(p, p, p, p, 1, 15, 16, 48, None) == E
    assert lib.ac_swin_patch_merge(p, p, p, p, 1, 16, 16, 768, None) == E
    assert lib.ac_htsat_pool(p, p, None, 1, 8, 8, 768, 2, None) == E
    assert lib.ac_htsat_pool(p, p, p, 1, 8, 8, 768, 3, None) == E
    assert lib.ac_htsat_token_mean(None, p, 1, 64, 192, None) == E
    assert lib.ac_gelu(p, None, 16, None) == E and lib.ac_gelu(p, p, 0, None) == E
