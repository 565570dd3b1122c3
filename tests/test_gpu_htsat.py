"""GPU tests of the HTS-AT encoder: every kernel of csrc/htsat.hip through the C ABI against the float64 restatement
tests/_htsat_ref.py (itself pinned to the reference's float64 run by tests/test_htsat_cpu.py), the whole encoder against
tests/golden/g_htsat.npz, wav -> encoder -> captions against the restatement + oracle/cpu_path.py's decoder.

``rel`` = max |diff| / max |want|.  Bars: 1e-5 for a kernel on exact-f32 products (every kernel here), 2e-4 for the whole
encoder (12 blocks deep, linear layers on split-bf16 operands), 1e-4 absolute on logits (the package's logit gate)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _htsat_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL_BAR, ENCODER_BAR, LOGIT_BAR = 1e-5, 2e-4, 1e-4
V, MAXLEN = 4368, 12
OUTPUTS = ["attn_emb", "fc_emb", "layer_0", "layer_1", "layer_2", "layer_3"]
CLIP_LENS = [320000, 256000, 176000]     # 10 s, 8 s, 5.5 s


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    sc = float(want.abs().max())
    d = float((got - want).abs().max()) / (sc + 1e-30)
    print(f"[{name}] max|diff| / max|want| = {d:.3e} (max|want| {sc:.3e})")
    return d


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def state():
    from audiocaption_amd import procedural as Pr
    return Pr.to_torch(Pr.htsat_trm_state(V))


@pytest.fixture(scope="module")
def model(lib, state):
    import audiocaption_amd as A
    m = A.init_model_from_config(A.htsat_trm_config(V), print_fn=lambda s: None)
    m.load_state_dict(dict(m.state_dict(), **state), strict=True)
    return m.eval().to("cuda:0")


@pytest.fixture(scope="module")
def golden_encoder(lib):
    """The encoder alone with the weights the golden was made with (``htsat_state`` without a key prefix: a tensor's
    values are a function of its key)."""
    import audiocaption_amd as A
    from audiocaption_amd import procedural as Pr
    enc = A.Htsat().eval()
    enc.load_state_dict(dict(enc.state_dict(), **Pr.to_torch(Pr.htsat_state())), strict=True)
    return enc.to("cuda:0")


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_KEEP = []


@pytest.fixture(autouse=True)
def _drop_kept_tensors():
    _KEEP.clear()
    yield
    _KEEP.clear()


def P(t):
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def canary(*shape):
    return torch.full(shape, float("nan"), device="cuda")


# ---- kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1024, 1001, 33, 32, 513, 1023, 1])
def test_patch_embed(lib, state, T):
    """Identity (1024), a mild stretch (1001) and a 31-times stretch with clamped borders (33); the shortest clip the encoder
    takes (32), a stretch by almost two (513), by 1023 / 1022 (every fraction occurs once) and a single frame (all four taps
    clamped onto it)."""
    B, C = 2, 96
    x = randn(B, T, 64, seed=T, scale=1.5)
    w, b, lw, lb = (state["encoder.patch_embed." + k] for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"))
    out = canary(B, 4096, C)
    rc = lib.ac_htsat_patch_embed(P(x.cuda()), B, T, P(w.reshape(C, 16).contiguous().cuda()), P(b.cuda()), P(lw.cuda()),
                                  P(lb.cuda()), P(out), C, S())
    assert rc == 0
    assert rel(f"patch embed T={T}", out, R.patch_embed(x, w, b, lw, lb)) < KERNEL_BAR


@pytest.mark.parametrize("B,H,heads,shift", [(2, 16, 2, 4), (2, 16, 2, 0), (2, 8, 2, 0), (1, 64, 4, 4)])
def test_window_attention(lib, B, H, heads, shift):
    """Four windows with all nine regions and the wrap-around; the same unshifted; a single window; the real first stage."""
    C = heads * 24
    qkv = randn(B, H * H, 3 * C, seed=H + shift)
    table = randn(225, heads, seed=3)          # distinct entries: a transposed or mis-indexed bias fails
    bias = R.relative_bias(table)
    assert not torch.equal(bias, bias.transpose(1, 2)) and len(set(table.reshape(-1).tolist())) == 225 * heads
    out = canary(B, H * H, C)
    rc = lib.ac_swin_window_attn(P(qkv.cuda()), P(bias.contiguous().cuda()), P(out), B, H, H, C, heads, shift, S())
    assert rc == 0
    want = R.window_attn(qkv, bias, H, H, heads, shift)
    if shift:
        assert float((want - R.window_attn(qkv, bias, H, H, heads, 0)).abs().max()) > 0.1
    assert rel(f"window attention {B}x{H}x{H}x{C} shift {shift}", out, want) < KERNEL_BAR


def test_patch_merge(lib):
    B, H, C = 2, 16, 48
    x = randn(B, H, H, C, seed=11)
    x[:, 0::2, 0::2] += 1.0            # a value per quadrant: a swapped channel order fails
    x[:, 1::2, 0::2] -= 2.0
    x[:, 0::2, 1::2] += 3.0
    x = x.reshape(B, H * H, C)
    lw, lb = 1.0 + 0.2 * randn(4 * C, seed=12), 0.1 * randn(4 * C, seed=13)
    out = canary(B, H * H // 4, 4 * C)
    assert lib.ac_swin_patch_merge(P(x.cuda()), P(lw.cuda()), P(lb.cuda()), P(out), B, H, H, C, S()) == 0
    assert rel("patch merge", out, R.patch_merge(x, H, H, lw, lb)) < KERNEL_BAR


def test_pool_token_mean_and_gelu(lib):
    B, C = 2, 768
    x = randn(B, 64, C, seed=21)
    attn, fc, mean = canary(B, 32, C), canary(B, C), canary(B, C)
    assert lib.ac_htsat_pool(P(x.cuda()), P(attn), P(fc), B, 8, 8, C, 2, S()) == 0
    want_attn, want_fc = R.pool(x, 8, 8, 2)
    assert rel("pool attn_emb", attn, want_attn) < KERNEL_BAR and rel("pool fc_emb", fc, want_fc) < KERNEL_BAR
    assert lib.ac_htsat_token_mean(P(x.cuda()), P(mean), B, 64, C, S()) == 0
    assert rel("token mean 64 x 768", mean, R.token_mean(x)) < KERNEL_BAR
    y = randn(B, 1024, 192, seed=22) + 0.3      # the first stage's output: 1024 tokens
    mean = canary(B, 192)
    assert lib.ac_htsat_token_mean(P(y.cuda()), P(mean), B, 1024, 192, S()) == 0
    assert rel("token mean 1024 x 192", mean, R.token_mean(y)) < KERNEL_BAR
    z = torch.cat([randn(70001, seed=23, scale=3.0), torch.tensor([0.0, -0.0, 10.0, -10.0])])    # 274 blocks with a partly empty
    # last one: ONE pass of the grid-stride loop (the grid is capped at 65 536 blocks; test_gelu_in_place_beyond_one_grid_pass)
    g = canary(z.numel())
    assert lib.ac_gelu(P(z.cuda()), P(g), z.numel(), S()) == 0
    assert rel("gelu", g, R.gelu(z.double())) < KERNEL_BAR


@pytest.mark.parametrize("B,H,W,heads,shift", [(2, 32, 32, 8, 0), (2, 32, 32, 8, 4), (2, 16, 16, 16, 0), (2, 16, 16, 16, 4),
                                               (2, 8, 8, 32, 0), (2, 16, 24, 2, 0), (2, 16, 24, 2, 4), (2, 24, 16, 2, 0),
                                               (2, 24, 16, 2, 4)])
def test_window_attention_encoder_stages_and_rectangles(lib, B, H, W, heads, shift):
    """The head counts and image sides of the encoder's stages 1 - 3 (8, 16 and 32 heads: the head offset into a 3C-wide row
    reaches 3 * 768 floats), and images with H != W (six windows: the window index splits into (row, column) by W / 8, the
    roll and the region bands take H and W separately)."""
    C = heads * 24
    qkv = randn(B, H * W, 3 * C, seed=H * 100 + W + shift + heads)
    bias = R.relative_bias(randn(225, heads, seed=5))
    out = canary(B, H * W, C)
    rc = lib.ac_swin_window_attn(P(qkv.cuda()), P(bias.contiguous().cuda()), P(out), B, H, W, C, heads, shift, S())
    assert rc == 0
    want = R.window_attn(qkv, bias, H, W, heads, shift)
    if shift:
        assert float((want - R.window_attn(qkv, bias, H, W, heads, 0)).abs().max()) > 0.1
    if H != W:      # the transposed image is another problem: a swapped H and W fails
        assert float((want - R.window_attn(qkv, bias, W, H, heads, shift)).abs().max()) > 0.1
    assert rel(f"window attention {B}x{H}x{W}x{C} heads {heads} shift {shift}", out, want) < KERNEL_BAR


@pytest.mark.parametrize("B,H,W,C", [(2, 16, 16, 96), (2, 16, 8, 192), (1, 6, 10, 384), (2, 8, 8, 384)])
def test_patch_merge_encoder_widths(lib, B, H, W, C):
    """The encoder's widths (4C = 1536 is the kernel's register bound, 64 lanes x 24), a rectangular image, and 15 merged
    tokens: a last workgroup with one idle wave."""
    x = randn(B, H, W, C, seed=H + W + C)
    x[:, 0::2, 0::2] += 1.0
    x[:, 1::2, 0::2] -= 2.0
    x[:, 0::2, 1::2] += 3.0
    x = x.reshape(B, H * W, C)
    lw, lb = 1.0 + 0.2 * randn(4 * C, seed=12), 0.1 * randn(4 * C, seed=13)
    out = canary(B, H * W // 4, 4 * C)
    assert lib.ac_swin_patch_merge(P(x.cuda()), P(lw.cuda()), P(lb.cuda()), P(out), B, H, W, C, S()) == 0
    assert rel(f"patch merge {B}x{H}x{W}x{C}", out, R.patch_merge(x, H, W, lw, lb)) < KERNEL_BAR


def test_patch_merge_refuses_a_width_beyond_its_registers(lib):
    from audiocaption_amd import _lib
    buf = torch.zeros(2 * 2 * 4 * 385, device="cuda")
    assert lib.ac_swin_patch_merge(P(buf), P(buf), P(buf), P(buf), 1, 2, 2, 385, S()) == _lib.AC_ERR_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0      # nothing was launched


@pytest.mark.parametrize("B,N,C", [(2, 1, 96), (2, 3, 96), (3, 1023, 96), (2, 1023, 192)])
def test_token_mean_token_counts(lib, B, N, C):
    """Fewer tokens than waves (1, 3), a count that is no multiple of the four waves (1023), and C = 96: the second channel
    block is half empty."""
    x = randn(B, N, C, seed=N + C) + 0.3
    mean = canary(B, C)
    assert lib.ac_htsat_token_mean(P(x.cuda()), P(mean), B, N, C, S()) == 0
    assert rel(f"token mean {N} x {C}", mean, R.token_mean(x)) < KERNEL_BAR


@pytest.mark.parametrize("B,Hh,Ww,C,fbins", [(2, 8, 8, 768, 1), (2, 8, 8, 768, 4), (3, 4, 6, 96, 2), (2, 6, 4, 300, 3)])
def test_pool_bins_and_rectangles(lib, B, Hh, Ww, C, fbins):
    """One bin per frame (the pool is a copy), four, and token grids with Hh != Ww; C = 300: a second, partly empty block."""
    x = randn(B, Hh * Ww, C, seed=Hh * 10 + Ww + fbins) + 0.2
    attn, fc = canary(B, Hh // fbins * Ww, C), canary(B, C)
    assert lib.ac_htsat_pool(P(x.cuda()), P(attn), P(fc), B, Hh, Ww, C, fbins, S()) == 0
    want_attn, want_fc = R.pool(x, Hh, Ww, fbins)
    assert rel(f"pool attn_emb {Hh}x{Ww} / {fbins}", attn, want_attn) < KERNEL_BAR
    assert rel(f"pool fc_emb {Hh}x{Ww} / {fbins}", fc, want_fc) < KERNEL_BAR


def test_gelu_in_place_beyond_one_grid_pass(lib):
    """As the encoder calls it: in place, on more elements than the capped grid (65 536 blocks of 256) covers in one pass."""
    n = 65536 * 256 + 1000
    z = randn(n, seed=24, scale=3.0)
    zd = z.cuda()
    assert lib.ac_gelu(P(zd), P(zd), n, S()) == 0
    want = R.gelu(z.double())
    assert rel("gelu in place, first pass", zd[:65536 * 256], want[:65536 * 256]) < KERNEL_BAR
    assert rel("gelu in place, second pass", zd[65536 * 256:], want[65536 * 256:]) < KERNEL_BAR


# ---- the whole encoder -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B,T", [("t1001", 2, 1001), ("t1024", 1, 1024)])
def test_encoder_vs_reference_golden(golden_encoder, golden_dir, case, B, T):
    """From the log-mel hook against the reference's float64 run.  Measured (MI355X, linear layers on split-bf16 operands):
    see tests/golden/REPORT_htsat.txt."""
    from audiocaption_amd import procedural as Pr
    g = np.load(os.path.join(golden_dir, "g_htsat.npz"))
    lms = torch.from_numpy(Pr.synthetic_logmel(B, T)).transpose(1, 2).contiguous().cuda()
    tokens = []
    got = golden_encoder.features_from_logmel(lms, stage_tokens=tokens)
    worst = {}
    for k in OUTPUTS:
        assert tuple(got[k].shape) == g[f"{case}/{k}"].shape
        worst[k] = rel(f"{case} {k}", got[k], g[f"{case}/{k}"])
    assert len(tokens) == 5
    for k, tok in enumerate(tokens):
        idx = torch.from_numpy(g[f"{case}/tok{k}_idx"].astype(np.int64))
        worst[f"tok{k}"] = rel(f"{case} tokens after " + ("the patch embedding" if k == 0 else f"stage {k - 1}"),
                               tok.cpu()[idx[:, 0], idx[:, 1], idx[:, 2]], g[f"{case}/tok{k}_val"])
    assert max(worst.values()) < ENCODER_BAR, worst


@pytest.fixture(scope="module")
def clips(model, state):
    """Three clips of uneven length, the product's outputs for them and the restatement fed with the HIP log-mel."""
    from audiocaption_amd import kernels as K, procedural as Pr
    L = CLIP_LENS[0]
    wav = Pr.synthetic_wav(3, L, varied=True)
    for i, n in enumerate(CLIP_LENS):
        wav[i, n:] = 0.0
    wav = torch.from_numpy(wav).cuda()
    enc = model.encoder
    inp = {"wav": wav, "wav_len": list(CLIP_LENS), "specaug": False}
    got = enc(inp)
    T = L // enc.hop_length + 1
    lms = K.logmel(wav, enc._tables, rows_per_clip=T, channels_last=True).view(3, T, 64).cpu()      # dB, before bn0
    want = R.forward(state, R.bn0(state, lms, "encoder."), prefix="encoder.")
    return {"wav": wav, "inp": inp, "got": got, "want": want}


def test_wav_to_encoder(model, clips):
    got, want = clips["got"], clips["want"]
    assert got["attn_emb_len"].tolist() == [31, 25, 17] and got["attn_emb_len"].dtype == torch.int64
    assert got["attn_emb_len"].device.type == "cpu" and tuple(got["attn_emb"].shape) == (3, 32, 768)
    assert got["layer_3"] is got["fc_emb"] or torch.equal(got["layer_3"], got["fc_emb"])
    for k in OUTPUTS:
        assert rel(f"wav -> {k}", got[k], want[k]) < ENCODER_BAR
    again = model.encoder(clips["inp"])           # cached buffers and packs: no stale state
    for k in OUTPUTS:
        assert torch.equal(again[k], got[k]), k
    one = model.encoder({"wav": clips["wav"][:1], "wav_len": CLIP_LENS[:1], "specaug": False})      # the same stretch: 1001 frames
    for k in OUTPUTS:
        assert rel(f"B = 1 vs row 0 of the batch: {k}", one[k], got[k][:1]) < ENCODER_BAR
    assert torch.equal(model.encoder(clips["inp"])["attn_emb"], got["attn_emb"])        # and back to B = 3


class _RecordingLib:
    """Forwards every call to the library and records (M, N, K, has_bias, beta) of the ``ac_gemm_bf16x3`` calls (the proxy of
    tools/launch_trace.py, cut down to one symbol)."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "ac_gemm_bf16x3":
            return fn

        def call(*a):
            self._calls.append((a[8], a[9], a[10], a[11] is not None, float(a[13])))
            return fn(*a)

        return call


def _encode_recording(encoder, inp):
    from audiocaption_amd import _lib
    calls, real = [], _lib.load
    proxy = _RecordingLib(real(), calls)
    _lib.load = lambda: proxy
    try:
        out = encoder(inp)
        torch.cuda.synchronize()
    finally:
        _lib.load = real
    return out, calls


def test_encoder_at_eight_clips_and_its_gemm_calls(model, clips):
    """Eight clips are where the linear layers of stage 0 first take the 128 x 128 split-bf16 tile and those of stage 1 all
    leave the exact kernels (tests/_gemm_routes.py): the fixture's three clips tiled to eight rows, every row against the
    restatement's row for the same clip, and the issued ``ac_gemm_bf16x3`` calls against ``htsat_linear_calls`` - the list
    whose routes tests/test_gemm_routes_cpu.py pins.  The same for one clip (stage 0's proj on the exact nt<1> kernel)."""
    import _gemm_routes as G
    rows = [0, 1, 2, 0, 1, 2, 0, 1]
    inp = {"wav": clips["wav"][rows].contiguous(), "wav_len": [CLIP_LENS[r] for r in rows], "specaug": False}
    got, calls = _encode_recording(model.encoder, inp)
    assert calls == [c[1:] for c in G.htsat_linear_calls(8)]
    assert got["attn_emb_len"].tolist() == [[31, 25, 17][r] for r in rows]
    want = clips["want"]
    for k in OUTPUTS:
        assert tuple(got[k].shape) == (8,) + tuple(want[k].shape[1:])
        for i, r in enumerate(rows):
            assert rel(f"B = 8, row {i} (clip {r}): {k}", got[k][i], want[k][r]) < ENCODER_BAR
    one, calls = _encode_recording(model.encoder, {"wav": clips["wav"][:1], "wav_len": CLIP_LENS[:1], "specaug": False})
    assert calls == [c[1:] for c in G.htsat_linear_calls(1)]
    for k in OUTPUTS:
        assert rel(f"B = 1: {k}", one[k][0], want[k][0]) < ENCODER_BAR


def test_repack_after_load_state_dict(model, state, clips):
    enc = model.encoder
    before = enc._packed
    key = "layers.3.blocks.1.mlp.fc2.bias"
    sd = enc.state_dict()
    try:
        # (a ramp: a constant added to every channel would be removed by the final LayerNorm)
        enc.load_state_dict(dict(sd, **{key: sd[key] + torch.linspace(-1.0, 1.0, 768, device=sd[key].device)}))
        moved = enc(clips["inp"])["fc_emb"]
        assert enc._packed[0] != before[0] and float((moved - clips["got"]["fc_emb"]).abs().max()) > 1e-3
    finally:
        enc.load_state_dict(dict(sd, **{key: state["encoder." + key].cuda()}))
    assert torch.equal(enc(clips["inp"])["fc_emb"], clips["got"]["fc_emb"])


def test_captioner_vs_oracle_decoder(model, state, clips):
    from oracle import cpu_path as O
    s64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
    attn, lens = clips["want"]["attn_emb"], R.feat_len(CLIP_LENS)
    want = O.greedy_decode(s64, attn, lens, max_length=MAXLEN)
    st = want["steps"]
    top2 = want["logit"][:, :st].topk(2, -1).values
    margin = float((top2[..., 0] - top2[..., 1]).min())
    print(f"greedy top-two margin {margin:.3e} over {st} steps")
    assert margin > 1e-3            # every step of every clip: the ids below are decided by more than the logit gate
    req = dict(clips["inp"], mode="inference", max_length=MAXLEN)
    got = model(dict(req, sample_method="greedy"))
    d = float((got["logit"][:, :st].double().cpu() - want["logit"][:, :st]).abs().max())
    print(f"greedy logits: max |diff| {d:.3e}")
    assert d < LOGIT_BAR
    assert torch.equal(got["seq"].cpu(), want["seq"])
    pend = model.forward_async(dict(req, sample_method="greedy"))        # the generic-encoder path of the throughput mode
    assert torch.equal(pend.result()["seq"].cpu(), want["seq"])
    trace = []
    want_b = O.beam_search(s64, attn, lens, beam_size=3, max_length=MAXLEN, trace=trace)
    bmargin = min(r["margin"] for r in trace)
    print(f"beam margin {bmargin:.3e}")
    assert bmargin > 1e-3
    got_b = model(dict(req, sample_method="beam", beam_size=3))
    assert torch.equal(got_b["seq"].cpu(), want_b["seq"])
    out = model(dict(req, sample_method="sample", n_samples=3, seed=7))
    assert tuple(out["seq"].shape) == (3, 3, MAXLEN)
    out = model(dict(req, sample_method="beam", beam_size=4, group_size=2))
    assert tuple(out["seq"].shape) == (3, 4, MAXLEN)


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_abi(lib):
    from audiocaption_amd import _lib
    names = ["ac_htsat_patch_embed", "ac_swin_window_attn", "ac_swin_patch_merge", "ac_htsat_pool", "ac_htsat_token_mean",
             "ac_gelu"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "audiocaption_hip.h")).read()
    for n in names:
        assert re.search(rf"\bint\s+{n}\s*\(", header) and n in _lib.SIGNATURES and hasattr(lib, n)
    buf = torch.zeros(1 << 16, device="cuda")
    p, E = P(buf), _lib.AC_ERR_ARG
    assert lib.ac_swin_window_attn(p, p, p, 1, 16, 16, 64, 2, 0, S()) == E          # head width 32
    assert lib.ac_swin_window_attn(p, p, p, 1, 12, 16, 48, 2, 0, S()) == E          # H not a multiple of the window
    assert lib.ac_swin_window_attn(p, p, p, 1, 16, 12, 48, 2, 0, S()) == E
    assert lib.ac_swin_window_attn(p, None, p, 1, 16, 16, 48, 2, 0, S()) == E
    assert lib.ac_htsat_patch_embed(p, 1, 2000, p, p, p, p, p, 96, S()) == E
    assert lib.ac_htsat_patch_embed(p, 1, 64, p, None, p, p, p, 96, S()) == E
    assert lib.ac_swin_patch_merge(p, p, p, p, 1, 16, 15, 48, S()) == E and lib.ac_swin_patch_merge(None, p, p, p, 1, 16, 16, 48, S()) == E
    assert lib.ac_htsat_pool(p, p, p, 1, 8, 8, 96, 3, S()) == E and lib.ac_htsat_pool(p, None, p, 1, 8, 8, 96, 2, S()) == E
    assert lib.ac_htsat_token_mean(p, None, 1, 64, 96, S()) == E and lib.ac_gelu(None, p, 16, S()) == E
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0      # nothing was launched
