"""Cnn6Encoder / Cnn10Encoder and the captioners over them against the reference's outputs (tests/golden/g28_cnn_small.npz,
made by tests/golden/make_golden_cnn_small.py in float64; cases of tests/_cnn_small_ref.py).

The fixture starts at the log-mel, so the encoders are fed ``input_dict["_logmel"]`` (bn0 applied with torch): per-block
outputs and ``attn_emb`` are held to what tests/test_gpu_model.py holds Cnn14Encoder to against g1_cnn14.npz on the same tier
(1e-4 on a block, 2e-4 on attn_emb, 2e-5 relative on the channel sums), ``attn_emb_len`` exactly.  Cnn10 runs on the tiers
"wino43" (its F(4,3) and one-kernel block 1 forced onto these few-clip batches, as there), "wino1d", "bf16x3" and "direct";
Cnn6 on its own 5x5 kernels."""
import contextlib

import numpy as np
import pytest
import torch

import _cnn_small_ref as R

pytestmark = pytest.mark.gpu

BLOCK_TOL, ATTN_TOL, BLOCK_SUM_RTOL = 1e-4, 2e-4, 2e-5    # tests/test_gpu_model.py _F32_GRADE: "block", "attn_golden", "block_sum_rtol"
# fc_emb = relu(fc1(max over frames + mean over frames)) sits behind a max, where a near-tie between two frames can flip: its
# tolerance is 2 x the largest error measured over all cases and tiers on an MI355X (tests/golden/REPORT_cnn_small.txt)
FC_TOL = 2 * 4.671e-5     # the largest: cnn10 / bf16x3, case (b)
RUNS = [("cnn6", None), ("cnn10", "wino43"), ("cnn10", "wino1d"), ("cnn10", "bf16x3"), ("cnn10", "direct")]


@pytest.fixture(scope="module")
def g28():
    from audiocaption_amd import build
    build.build()
    return dict(np.load(R.FIXTURE))


@contextlib.contextmanager
def _forced_f43(algo):
    from audiocaption_amd import cnn_encoder as CE
    saved = CE.W43_MIN_WORKGROUPS
    if algo == "wino43":
        CE.W43_MIN_WORKGROUPS = 1
    try:
        yield
    finally:
        CE.W43_MIN_WORKGROUPS = saved


_ENCODERS = {}


def _encoder(kind, sr):
    import audiocaption_amd as A
    from audiocaption_amd import procedural as P
    if (kind, sr) not in _ENCODERS:
        enc = {"cnn6": A.Cnn6Encoder, "cnn10": A.Cnn10Encoder}[kind](sample_rate=sr)
        enc.load_state_dict(P.to_torch(R.fixture_state(kind)), strict=False)   # (the mel buffers keep their own values)
        _ENCODERS[(kind, sr)] = enc.eval().to("cuda:0")
    return _ENCODERS[(kind, sr)]


def _inputs(enc, case, algo):
    sr, T, frames = R.CASES[case]
    L = R.hop(sr) * (T - 1)
    pk = enc._pack(torch.device("cuda:0"), algo)
    x0 = R.x0_rows(R.logmel(case).cuda(), pk["bn0"][0], pk["bn0"][1], enc.geometry(L)[2][0])
    d = {"wav": torch.zeros(len(frames), L, device="cuda"), "wav_len": R.wav_lens(case), "_logmel": x0}
    if algo is not None:
        d["conv_algo"] = algo
    return d


def _maxdiff(name, got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    d = float((got - want).abs().max())
    R.report(f"[{name}] max|diff| {d:.3e} (|want| max {float(want.abs().max()):.3e})")
    return d


@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("kind,algo", RUNS)
def test_encoder_vs_reference_golden(g28, kind, algo, case):
    sr, T, frames = R.CASES[case]
    enc = _encoder(kind, sr)
    tag = f"{kind}/{algo or 'conv5x5'} ({case})"
    with _forced_f43(algo):
        inp = _inputs(enc, case, algo)
        out = enc(inp)
        blocks = []
        if case == "a":
            attn2 = enc.encode(inp["wav"], algo=algo, x0=inp["_logmel"], blocks=blocks)
            assert torch.equal(attn2, out["attn_emb"])
    assert out["attn_emb"].shape == (len(frames), T // 16, 512) and out["fc_emb"].shape == (len(frames), 512)
    assert out["attn_emb_len"].tolist() == g28[f"{kind}/{case}/attn_emb_len"].tolist()
    for b, blk in enumerate(blocks):
        got = R.block_digest(blk.cpu())
        assert _maxdiff(f"{tag} block{b + 1}", got["sub"], g28[f"{kind}/a/block{b + 1}_sub"]) < BLOCK_TOL
        np.testing.assert_allclose(got["sum"], g28[f"{kind}/a/block{b + 1}_sum"], rtol=BLOCK_SUM_RTOL, atol=5e-2)
    assert _maxdiff(f"{tag} attn_emb", out["attn_emb"], g28[f"{kind}/{case}/attn_emb"]) < ATTN_TOL
    assert _maxdiff(f"{tag} fc_emb", out["fc_emb"], g28[f"{kind}/{case}/fc_emb"]) < FC_TOL


def test_skip_fc_and_half_precision_tier_hand_over(g28):
    """``skip_fc`` (what CrnnEncoder asks for) leaves ``fc_emb`` out; on Cnn10 a tier with fp16 activations runs its declared
    fallback: the bits of "bf16x3"."""
    enc = _encoder("cnn10", 32000)
    inp = _inputs(enc, "a", "bf16x3")
    want = enc(inp)
    got = enc(dict(inp, conv_algo="f16x2"), skip_fc=True)
    assert "fc_emb" not in got and torch.equal(got["attn_emb"], want["attn_emb"])


# ---- the captioners ------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(kind, g28):
    import audiocaption_amd as A
    from audiocaption_amd import procedural as P
    if kind not in _MODELS:
        cfg = {"cnn6": A.cnn6rnn_trm_config, "cnn10": A.cnn10rnn_trm_config}[kind](R.VOCAB)
        model = A.init_model_from_config(cfg, print_fn=lambda s: None)
        state = P.to_torch(R.fixture_model_state(kind, int(g28[f"{kind}/d/seed"])))
        missing, unexpected = model.load_state_dict(state, strict=False)
        assert not unexpected and all("melspec_extractor" in k for k in missing), (missing, unexpected)
        _MODELS[kind] = model.eval().to("cuda:0")
    return _MODELS[kind]


@pytest.mark.parametrize("kind", ["cnn6", "cnn10"])
def test_greedy_and_beam_ids_equal_the_references(g28, kind):
    model = _model(kind, g28)
    inp = dict(_inputs(model.encoder.cnn, "a", None), mode="inference", specaug=False, max_length=R.MAX_LENGTH)
    greedy = model(dict(inp, sample_method="greedy"))
    assert greedy["seq"].cpu().tolist() == g28[f"{kind}/d/greedy_seq"].tolist()
    assert greedy["attn_emb"].shape == (3, 3, 512) and greedy["attn_emb_len"].tolist() == [3, 2, 1]
    beam = model(dict(inp, sample_method="beam", beam_size=R.BEAM))
    assert beam["seq"].cpu().tolist() == g28[f"{kind}/d/beam_seq"].tolist()


@pytest.mark.parametrize("kind", ["cnn6", "cnn10"])
def test_forward_async_and_group_beam_run_over_the_small_encoders(g28, kind):
    """From the waveform (the encoders' own mel front, ``logmel_front`` on its stream): ``forward_async`` returns the
    blocking call's ids, and group beam search runs."""
    from audiocaption_amd import procedural as P
    model = _model(kind, g28)
    wav = torch.from_numpy(P.synthetic_wav(3, 320 * 99, varied=True)).cuda()
    inp = {"mode": "inference", "wav": wav, "wav_len": [320 * 99, 320 * 70, 320 * 40], "specaug": False,
           "sample_method": "greedy", "max_length": R.MAX_LENGTH}
    want = model(dict(inp))
    got = model.forward_async(dict(inp)).result()
    assert torch.equal(want["seq"], got["seq"]) and want["attn_emb_len"].tolist() == [6, 4, 2]
    out = model(dict(inp, sample_method="beam", beam_size=4, group_size=2))
    assert out["seq"].shape == (3, 4, R.MAX_LENGTH)

