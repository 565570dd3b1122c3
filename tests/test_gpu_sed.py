"""The sound-event tagger on the GPU (csrc/sed.hip, audiocaption_amd/sed_model.py, hf_wrapper.Cnn14RnnTempAttnGruModel)
against the reference's recorded outputs (tests/golden/g21_sed.npz) and the CPU restatement tests/_sed_ref.py.

Gates.  ac_pool_avgmax: within 4 * 2^-24 * (mean|x| + max|x|) over the window of the float64 result (the rounding of a
4-term f32 sum plus one add; the window of the fused mean form is the row's 8 mel columns), rows at or beyond H_out exactly
0.  Tags: identical to the recorded ones.  fc_audioset's pre-activation: within 1e-4 absolute of the fixture (the project's
f32 parity gate) on every logit - at T = 1001 the fixture keeps every second class column; the
others are held to the CPU restatement with the gate narrowed by its recorded deviation from the reference.  Every figure is printed before it is asserted; tests/golden/REPORT_sed.txt keeps a
run.
"""
import os

import numpy as np
import pytest
import torch

import _sed_ref as R

pytestmark = pytest.mark.gpu

GATE = 1e-4
ULPS = 8 * 2.0 ** -24   # sigmoid in f32 against float64: expf (2 ulp), the add, the division and the final rounding, at p <= 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def g21():
    if "g21" not in _CACHE:
        _CACHE["g21"] = np.load(os.path.join(GOLDEN, "g21_sed.npz"))
    return _CACHE["g21"]


def tagger():
    """The tagger with the fixture's weights on the GPU (built once per module)."""
    if "model" not in _CACHE:
        import audiocaption_amd as A
        from audiocaption_amd import build, procedural as P
        build.build()
        seed, head_seed, scale = g21()["recipe"]
        model = A.Cnn8rnnSedModel(447)
        model.load_state_dict(P.to_torch(P.sed_state(seed=int(seed), head_seed=int(head_seed), head_scale=float(scale))),
                              strict=True)
        _CACHE["model"] = model.cuda().eval()
    return _CACHE["model"]


# ---- ac_pool_avgmax -------------------------------------------------------------------------------------------------------
def _pool_case(B, H, Hp, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hp, W, C, generator=g) * 3.0        # signed
    x[:, H:] = float("nan")                                 # padding rows: never read for a row below H_out
    return x


def _pool_ref(x, H, ph):
    """float64 avg + max over (ph, 2) windows of the rows below H, and the bound's mean|x| + max|x| per window."""
    B, _, W, C = x.shape
    v = x[:, :(H // ph) * ph].double().reshape(B, H // ph, ph, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // ph, W // 2, C, -1)
    return v.mean(-1) + v.amax(-1), v.abs().mean(-1) + v.abs().amax(-1)


@pytest.mark.parametrize("ph,B,H,Hp,W,C", [(2, 3, 37, 40, 8, 128), (1, 3, 9, 12, 8, 256)])
def test_pool_avgmax(ph, B, H, Hp, W, C):
    from audiocaption_amd import kernels as K
    x = _pool_case(B, H, Hp, W, C, 5 + ph)
    Hp_out = Hp // ph
    out = torch.full((B, Hp_out, W // 2, C), 7.0, device="cuda")
    K.pool_avgmax(x.cuda().reshape(-1), out, B, Hp, H, W, C, ph, Hp_out=Hp_out)
    out = out.cpu()
    want, scale = _pool_ref(x, H, ph)
    err = ((out[:, :H // ph].double() - want).abs() / scale).max().item() / 2.0 ** -24
    print(f"pool ({ph},2) B {B} H {H} W {W} C {C}: worst error {err:.3f} x 2^-24 (mean|x| + max|x|), gate 4")
    assert err <= 4.0
    assert H // ph < Hp_out and bool((out[:, H // ph:] == 0).all()), "rows at or beyond H_out must be exactly 0"


def test_pool_avgmax_mean_over_mel():
    from audiocaption_amd import kernels as K
    B, H, Hp, W, C = 3, 9, 12, 8, 256
    x = _pool_case(B, H, Hp, W, C, 11)
    out = torch.empty(B, H, C, device="cuda")
    K.pool_avgmax(x.cuda().reshape(-1), out, B, Hp, H, W, C, 1, mean_w=True)
    pooled, _ = _pool_ref(x, H, 1)                                     # (B, H, W / 2, C)
    rows = x[:, :H].double().abs()
    scale = rows.mean(2) + rows.amax(2)                                 # over the row's 8 mel columns
    err = ((out.cpu().double() - pooled.mean(2)).abs() / scale).max().item() / 2.0 ** -24
    print(f"pool (1,2) + mean over mel B {B} H {H} W {W} C {C}: worst error {err:.3f} x 2^-24 (mean|x| + max|x|), gate 4")
    assert err <= 4.0


# ---- ac_sed_temporal_tag --------------------------------------------------------------------------------------------------
def test_temporal_tag_on_the_handbuilt_set():
    from audiocaption_amd import kernels as K
    ws = None
    for name, prob, frames, ratio in [c + (R.RATIO,) for c in R.handbuilt_cases()] + [R.handbuilt_ratio1()]:
        tags, ws = K.sed_temporal_tag(torch.from_numpy(prob).cuda(), frames, ratio, workspace=ws)
        got, want = tags.tolist(), g21()[f"hand_{name}_tags"].tolist()
        print(f"{name}: B {prob.shape[0]} tags {got} recorded {want}")
        assert got == want, name


def test_sed_head():
    from audiocaption_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    x, b = torch.randn(37, 447, generator=g) * 12.0, torch.randn(447, generator=g)
    pre = torch.empty(37, 447, device="cuda")
    prob = K.sed_head(x.cuda(), b.cuda(), pre=pre).cpu()
    want = torch.sigmoid(x.double() + b.double()).clamp(1e-7, 1.0)
    d = float((prob.double() - want).abs().max())
    print(f"sed head: |prob - float64| {d:.2e}; min {float(prob.min()):.1e} max {float(prob.max()):.1e}")
    assert torch.equal(pre.cpu(), x + b) and d < ULPS and float(prob.min()) >= 1e-7 and float(prob.max()) <= 1.0


# ---- the assembled tagger --------------------------------------------------------------------------------------------------
def restatement(B, T):
    """The CPU restatement's pre-activation of a fixture case (computed once per module)."""
    if ("cpu", B, T) not in _CACHE:
        from audiocaption_amd import procedural as P
        seed, head_seed, scale = g21()["recipe"]
        state = P.to_torch(P.sed_state(seed=int(seed), head_seed=int(head_seed), head_scale=float(scale)))
        with torch.no_grad():
            _CACHE[("cpu", B, T)] = R.stack(state, torch.from_numpy(P.synthetic_logmel(B, T)))
    return _CACHE[("cpu", B, T)]


def check_preactivation(pre, B, T, what):
    """fc_audioset's pre-activation (B, T // 4, 447) of a fixture case against the fixture, 1e-4 on every logit: the
    recorded columns against the reference's values; at T = 1001, where the fixture holds every second column, the others
    against the CPU restatement with the gate narrowed by the restatement's recorded deviation from the reference (over all
    columns), and the sums over all classes against the reference's."""
    key = f"b{B}_t{T}"
    if key + "_pre" in g21().files:
        d = float((pre - torch.from_numpy(g21()[key + "_pre"])).abs().max())
    else:
        d = float((pre[:, :, ::2] - torch.from_numpy(g21()[key + "_pre_cols"])).abs().max())
        dev = float(g21()[key + "_restatement_dev"])
        do = float((pre[:, :, 1::2] - restatement(B, T)[:, :, 1::2]).abs().max())
        ds = float((pre.double().sum(2) - torch.from_numpy(g21()[key + "_pre_rowsum"])).abs().max())
        print(f"{what}: unrecorded columns vs the restatement {do:.2e} (gate {GATE:.0e} - {dev:.2e}); sums over all classes "
              f"differ by {ds:.2e} (gate {GATE * pre.shape[2]:.2e})")
        assert do < GATE - dev and ds < GATE * pre.shape[2]
    print(f"{what}: |pre-activation - fixture| {d:.2e} (gate {GATE:.0e})")
    assert d < GATE


@pytest.mark.parametrize("B,T", [(2, 37), (3, 64), (2, 1001)])
def test_tagger_matches_the_reference(B, T):
    from audiocaption_amd import procedural as P
    assert [B, T] in g21()["cases"].tolist()
    model = tagger()
    lms = torch.from_numpy(P.synthetic_logmel(B, T)).cuda()
    with torch.no_grad():
        out = model.forward_prob(lms)
        pre = model.last_preact.cpu()
        tags = model(lms)
    key = f"b{B}_t{T}"
    check_preactivation(pre, B, T, f"B {B} T {T}")
    print(f"B {B} T {T}: tags {tags} recorded {g21()[key + '_tags'].tolist()}")
    seg, frame = out["segmentwise_output"].cpu(), out["framewise_output"].cpu()
    assert seg.shape == (B, T // 4, 447) and frame.shape == (B, T, 447)
    dp = float((seg.double() - torch.sigmoid(pre.double()).clamp(1e-7, 1.0)).abs().max())
    print(f"B {B} T {T}: |segmentwise - sigmoid(pre-activation)| {dp:.2e}")
    assert dp < ULPS
    assert np.array_equal(R.framewise(seg.numpy(), T), frame.numpy())
    assert tags == g21()[key + "_tags"].tolist()
    assert isinstance(tags, list) and all(isinstance(t, int) for t in tags)


def test_tagger_on_the_full_chip_route():
    """Eight 10 s clips (the fixture's two, four times): every layer of blocks 2-4 launches enough workgroups for the F(4,3)
    kernel - the route of the 64-clip product call; the fixture's batches of 2 and 3 clips take the K-sliced F(2,3) form."""
    from audiocaption_amd import cnn_encoder as C, kernels as K, procedural as P
    model = tagger()
    B, T, REPS = 2, 1001, 4
    assert model.effective_algo() == "wino43"
    Hp = model.geometry(T)[1]
    groups = [K.wino43_workgroups(REPS * B, Hp[lvl], W, cout) for lvl, W, cout in ((1, 32, 128), (2, 16, 256), (2, 8, 512))]
    small = [K.wino43_workgroups(B, Hp[lvl], W, cout) for lvl, W, cout in ((1, 32, 128), (2, 16, 256), (2, 8, 512))]
    print(f"F(4,3) workgroups per block at {REPS * B} clips {groups}, at 2 clips {small}, threshold {C.W43_MIN_WORKGROUPS}")
    assert min(groups) >= C.W43_MIN_WORKGROUPS > max(small)
    lms = torch.from_numpy(P.synthetic_logmel(B, T)).cuda().repeat(REPS, 1, 1)
    with torch.no_grad():
        tags = model(lms)
        pre = model.last_preact.cpu()
    for r in range(REPS):
        check_preactivation(pre[r * B:(r + 1) * B], B, T, f"{REPS * B} clips, F(4,3) route, clips {r * B}..{r * B + 1}")
    assert tags == g21()[f"b{B}_t{T}_tags"].tolist() * REPS


def test_temporal_tag_tie_sweep():
    """4096 segment pairs on the 4-frame grid, three quarters of them exact ties in integer frames, through the tag kernel:
    equal to the reference's pair rule on every one (durations with the product fused into the subtraction get 1021 of
    them wrong, the integer form 1746: tests/test_sed_cpu.py)."""
    from audiocaption_amd import kernels as K
    pairs = R.tie_sweep()
    want = g21()["sweep_tags"].tolist()
    tags, _ = K.sed_temporal_tag(torch.from_numpy(R.sweep_probabilities(pairs)).cuda(), 4 * R.SWEEP_S)
    got = tags.tolist()
    wrong = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    print(f"tie sweep: {len(pairs)} pairs, {len(wrong)} differ from the reference's rule" +
          "".join(f"; {pairs[i]} kernel {got[i]} reference {want[i]}" for i in wrong[:4]))
    assert not wrong


def test_forward_wav_matches_forward_on_its_logmel():
    from audiocaption_amd import kernels as K, procedural as P
    from audiocaption_amd.mel import MelTables
    model = tagger()
    wav = torch.from_numpy(P.synthetic_wav(2, 32000, varied=True)).cuda()      # 1 s: 101 frames, 25 segments
    tables = MelTables(32000, 1024, 320, 50.0, 14000.0, 64, "slaney", "slaney", wav.device)
    with torch.no_grad():
        tags_wav = model.forward_wav(wav)
        pre_wav = model.last_preact.cpu()
        lms = K.logmel(wav, tables, channels_last=False)                       # (B, 64, T), no BN fold
        tags_lms = model(lms)
        pre_lms = model.last_preact.cpu()
    d = float((pre_wav - pre_lms).abs().max())
    print(f"forward_wav vs forward(logmel): |pre-activation| {d:.2e} (gate {GATE:.0e}); tags {tags_wav.tolist()} / {tags_lms}")
    assert tags_wav.dtype == torch.int32 and tags_wav.is_cuda
    assert d < GATE and tags_wav.tolist() == tags_lms


# ---- the HF model ----------------------------------------------------------------------------------------------------------
def test_hf_model(state4981):
    from audiocaption_amd import hf_wrapper as H, procedural as P
    small = dict(emb_dim=64, d_model=128, attn_size=128)
    cfg = H.Cnn14RnnTempAttnGruConfig(vocab_size=517, decoder_emb_dim=64, decoder_d_model=128)
    sd = {"cap_model." + k: v for k, v in state4981.items() if k.startswith("encoder.")}
    sd.update(P.to_torch(P.bah_decoder_state("cap_model.decoder.", vocab_size=517, temporal=True, **small)))
    sd.update(P.to_torch(P.sed_state("sed_model.", active=40)))
    model = H.Cnn14RnnTempAttnGruModel(cfg)
    model.load_checkpoint(sd, strict=True)
    model = model.cuda().eval()
    wav = torch.from_numpy(P.synthetic_wav(2, 64000, varied=True))              # two clips of 2 s
    lens = [64000, 48000]
    wav[1, 48000:] = 0
    tags = model.temporal_tags(wav.cuda())
    print(f"HF model: the tagger's tags {tags.tolist()}")
    assert tags.dtype == torch.int64 and not tags.is_cuda and int(tags.min()) >= 0 and int(tags.max()) <= 3
    # the same tags without the wrapper's own mel tables and BN fold: the tagger on a log-mel computed here, and on the
    # waveform with its default tables
    from audiocaption_amd import kernels as K
    from audiocaption_amd.mel import MelTables
    with torch.no_grad():
        lms = K.logmel(wav.cuda(), MelTables(32000, 1024, 320, 50.0, 14000.0, 64, "slaney", "slaney", torch.device("cuda:0")),
                       channels_last=False)
        assert model.sed_model(lms) == tags.tolist()
        assert model.sed_model.forward_wav(wav.cuda()).tolist() == tags.tolist()
    for method in ("beam", "greedy"):
        seq = model(wav, lens, sample_method=method, max_length=8)
        by_hand = model.cap_model({"mode": "inference", "wav": wav.cuda(), "wav_len": lens, "specaug": False,
                                   "sample_method": method, "beam_size": 3, "max_length": 8, "temp": 1.0,
                                   "temporal_tag": tags})["seq"]
        assert seq.shape == (2, 8) and seq.dtype == torch.long and not seq.is_cuda
        assert torch.equal(seq, by_hand), method
    # a caller's tag is combined with the tagger's by element-wise minimum: zeros force tag 0
    assert model.temporal_tags(wav.cuda(), [3, 1]).tolist() == [min(3, int(tags[0])), min(1, int(tags[1]))]
    forced = model(wav, lens, temporal_tag=[0, 0], sample_method="greedy", max_length=8)
    zeros = model.cap_model({"mode": "inference", "wav": wav.cuda(), "wav_len": lens, "specaug": False,
                             "sample_method": "greedy", "max_length": 8, "temp": 1.0,
                             "temporal_tag": torch.zeros(2, dtype=torch.long)})["seq"]
    assert torch.equal(forced, zeros)
    # strict round trip
    again = H.Cnn14RnnTempAttnGruModel(cfg)
    again.load_state_dict(model.state_dict(), strict=True)
    assert all(torch.equal(v.cpu(), again.state_dict()[k]) for k, v in model.state_dict().items())
