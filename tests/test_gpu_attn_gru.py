"""The attention-GRU caption decoder on the GPU (csrc/attn_gru.hip, audiocaption_amd/rnn_decoder.py, attn_model.py), encoder
outputs fed directly, against the reference's recorded outputs (tests/golden/g19_attn_gru.npz) and the CPU restatement
tests/_attn_gru_ref.py.

Gates.  Ids: identical to the fixture.  Logits and log-probabilities: within 1e-4 absolute of the fixture (the project's
f32 parity gate).  attn_weight, state, embed: n = the largest deviation of the restatement in f32
from the restatement in float64 on the same case, gate 8 * n against the float64 values (8: the other summation order over
dots of up to 1536 terms).  Every figure is printed before it is asserted; tests/golden/REPORT_attn_gru.txt keeps a run.
"""
import ctypes

import numpy as np
import pytest
import torch

import _attn_gru_ref as R
import _sampling_ref as SR

pytestmark = pytest.mark.gpu

GATE = 1e-4
L = 20
_CACHE = {}


def g19():
    if "g19" not in _CACHE:
        _CACHE["g19"] = R.load_g19()
    return _CACHE["g19"]


def build(case, sd):
    import audiocaption_amd as A
    shape, kind = case.split("_")
    dcls, mcls = ((A.TemporalBahAttnDecoder, A.TemporalSeq2SeqAttnModel) if kind == "t" else
                  (A.BahAttnCatFcDecoder, A.Seq2SeqAttnModel))
    dec = dcls(dropout=0.5, **R.SHAPES[shape])
    dec.load_state_dict(sd, strict=True)
    return mcls(torch.nn.Identity(), dec).cuda().eval()


def case(name):
    """Model, inputs and the restatement's f32 / float64 greedy runs of a fixture case (computed once per module)."""
    if name not in _CACHE:
        sd, mem, lens, fc, tags = R.case_inputs(g19(), name)
        c = {"sd": sd, "mem": mem, "lens": lens, "fc": fc, "tags": tags, "model": build(name, sd)}
        with torch.no_grad():
            c["ref32"] = R.greedy(sd, mem, lens, fc, tags, L)
            c["ref64"] = R.greedy(sd, mem, lens, fc, tags, L, dtype=torch.float64)
        assert torch.equal(c["ref32"]["seq"], c["ref64"]["seq"])
        c["live"] = R.live_mask(c["ref32"]["seq"].numpy())
        c["n"] = R.error_budget(c["ref32"], c["ref64"], c["live"])
        _CACHE[name] = c
    return _CACHE[name]


def request(c, rows=None, **kw):
    sel = slice(None) if rows is None else rows
    d = {"mode": "inference", "attn_emb": c["mem"][sel].cuda(), "fc_emb": c["fc"][sel].cuda(),
         "attn_emb_len": c["lens"][sel], "max_length": L}
    if c["tags"] is not None:
        d["temporal_tag"] = c["tags"][sel]
    d.update(kw)
    return d


def check(name, got, want, gate):
    d = float((torch.as_tensor(got).double().cpu() - torch.as_tensor(want).double()).abs().max())
    print(f"{name}: max |gpu - reference| {d:.3e} (gate {gate:.3e})")
    assert d <= gate, name
    return d


# ---- (a), (b), (e), (g): greedy against the fixture, published and small shape, both model classes ----------------------
@torch.no_grad()
@pytest.mark.parametrize("name", R.CASES)
def test_greedy_matches_the_fixture(name):
    c, g = case(name), g19()
    out = c["model"](request(c))
    live = torch.from_numpy(c["live"])
    assert out["seq"].dtype == torch.int64 and not out["seq"].is_cuda and not out["sampled_logprob"].is_cuda
    np.testing.assert_array_equal(out["seq"].numpy(), g[name + "_greedy_seq"])
    logit = out["logit"].cpu()
    tv, ti = logit.topk(8, dim=2)
    np.testing.assert_array_equal(ti.numpy() * c["live"][..., None], g[name + "_greedy_top_idx"])
    check(f"{name} top-8 logits", tv * live[..., None], g[name + "_greedy_top_val"], GATE)
    check(f"{name} logit columns", logit[:, :, g["logit_cols"].tolist()], g[name + "_greedy_logit_cols"], GATE)
    check(f"{name} logits (restatement, every column)", logit, c["ref32"]["logit"], GATE)
    check(f"{name} sampled_logprob", out["sampled_logprob"], g[name + "_greedy_value"], GATE)
    n = c["n"]
    print(f"{name} n (f32 vs float64 restatement): {n}")
    check(f"{name} attn_weight", out["attn_weight"], c["ref64"]["attn_weight"], 8 * n["attn_weight"])
    check(f"{name} state", out["state"], c["ref64"]["state"], 8 * n["state"])
    check(f"{name} embed", out["embed"], c["ref64"]["embed"], 8 * n["embed"])
    assert tuple(out["attn_weight"].shape) == (c["mem"].shape[0], c["mem"].shape[1], L)
    assert tuple(out["state"].shape) == (1, c["mem"].shape[0], c["model"].decoder.d_model)
    # finished-row contract: after a row's first <end> everything reads <end> / 0
    dead = ~live
    assert not logit[dead].any() and not out["embed"].cpu()[dead].any() and not out["sampled_logprob"][dead].any()
    assert not out["attn_weight"].cpu().transpose(1, 2)[dead].any()
    assert (out["seq"][dead] == 2).all()
    np.testing.assert_array_equal(out["unfinished_cnt"].cpu().numpy(), c["ref32"]["unfinished_cnt"].numpy())
    # (g) masked frames weigh exactly 0 and the weights of a live step sum to 1 within f32 rounding
    w = out["attn_weight"].cpu()
    Tm = w.shape[1]
    for i, ln in enumerate(c["lens"].tolist()):
        assert not w[i, ln:, :].any(), f"clip {i}: weight on a masked frame"
        s = w[i].sum(0)[live[i]]
        assert float((s - 1).abs().max()) <= 2 * Tm * 2.0 ** -24, f"clip {i}: weights sum to {s.tolist()}"


@torch.no_grad()
def test_early_stop_keeps_the_initial_columns():
    """(e) pub_t: every row has ended after step 3 of 20 - later columns keep <end> / 0, the counts stop at 0 and the state
    is the one the last executed step left."""
    c = case("pub_t")
    steps = c["ref32"]["steps"]
    assert steps < L
    out = c["model"](request(c))
    cnt = out["unfinished_cnt"].cpu().numpy()
    assert cnt[steps - 1] == 0 and not cnt[steps:].any() and cnt[0] > 0
    assert (out["seq"][:, steps:] == 2).all() and not out["sampled_logprob"][:, steps:].any()
    assert not out["logit"][:, steps:].any() and not out["embed"][:, steps:].any() and not out["attn_weight"][:, :, steps:].any()
    check("pub_t state after the early stop", out["state"], c["ref64"]["state"], 8 * c["n"]["state"])


# ---- (a), (b): beam 3 / 4 and n_best against the fixture ----------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("name", R.CASES)
def test_beam_matches_the_fixture(name, k):
    c, g = case(name), g19()
    out = c["model"](request(c, sample_method="beam", beam_size=k))
    np.testing.assert_array_equal(out["seq"].numpy(), g[f"{name}_beam{k}_seq"])
    nb = c["model"](request(c, sample_method="beam", beam_size=k, n_best=True, n_best_size=k))
    np.testing.assert_array_equal(nb["seq"].numpy(), g[f"{name}_beam{k}_nbest"])
    args = (c["sd"], c["mem"], c["lens"], c["fc"], c["tags"], k, L)
    r32, r64 = R.beam_search(*args), R.beam_search(*args, dtype=torch.float64)
    assert torch.equal(r32["seq"], r64["seq"])
    n = float((r32["attn_weight"].double() - r64["attn_weight"]).abs().max())
    print(f"{name} beam {k} n (attn_weight, f32 vs float64 restatement): {n:.3e}")
    check(f"{name} beam {k} attn_weight", out["attn_weight"], r64["attn_weight"], 8 * n)
    check(f"{name} beam {k} attn_weight (n-best run)", nb["attn_weight"], r64["attn_weight"], 8 * n)
    for i, steps in enumerate(g[f"{name}_beam{k}_steps"].tolist()):   # columns the clip's search never reached
        assert not out["attn_weight"][i, :, steps:].any()


# ---- (c): row counts off the 64-row tile; every clip equals the same clip decoded alone -----------------------------------
@torch.no_grad()
def test_row_counts_off_the_tile_and_clips_alone():
    """15 rows (5 clips x beam 3) and 120 rows (40 clips x beam 3) of the small shape: ids equal to the restatement's, and
    every clip of the 40 equals the same clip decoded alone (beam and greedy)."""
    c = case("small_t")
    model = c["model"]
    reps = 8
    mem = torch.cat([torch.roll(c["mem"], 7 * j, dims=2) for j in range(reps)])
    fc = torch.cat([torch.roll(c["fc"], 7 * j, dims=1) for j in range(reps)])
    lens = torch.cat([torch.clamp(c["lens"] - 3 * j, min=1) for j in range(reps)])
    tags = torch.cat([(c["tags"] + j) % 4 for j in range(reps)])
    big = {"mem": mem, "fc": fc, "lens": lens, "tags": tags}
    want = R.beam_search(c["sd"], mem, lens, fc, tags, 3, L)
    out = model(request(big, sample_method="beam", beam_size=3))
    assert out["seq"].shape == (40, L)
    np.testing.assert_array_equal(out["seq"].numpy(), want["seq"].numpy())
    r64 = R.beam_search(c["sd"], mem, lens, fc, tags, 3, L, dtype=torch.float64)
    n = float((want["attn_weight"].double() - r64["attn_weight"]).abs().max())
    check("40 clips x beam 3 attn_weight", out["attn_weight"], r64["attn_weight"], 8 * n)
    greedy = model(request(big))
    for i in range(40):
        alone = model(request(big, rows=slice(i, i + 1), sample_method="beam", beam_size=3))
        assert torch.equal(alone["seq"][0], out["seq"][i]), f"clip {i} (beam)"
        d = float((alone["attn_weight"][0].double().cpu() - r64["attn_weight"][i]).abs().max())
        assert d <= 8 * n, f"clip {i} alone (beam attn_weight): {d:.3e} > {8 * n:.3e}"
        alone = model(request(big, rows=slice(i, i + 1)))
        assert torch.equal(alone["seq"][0], greedy["seq"][i]), f"clip {i} (greedy)"
    five = model(request(c, sample_method="beam", beam_size=3))
    np.testing.assert_array_equal(five["seq"].numpy(), out["seq"][:5].numpy())


# ---- (d): the decoder step alone through the C ABI --------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("t", [0, 5])
def test_step_logits_alone(t):
    """ac_bah_step_logits over 15 rows (5 clips x 3 rows each) at t = 0 with the tags and at t > 0 with word ids and a
    non-zero state, against the restatement's step."""
    c = case("small_t")
    dec, sd = c["model"].decoder, c["sd"]
    B, Tm, _ = c["mem"].shape
    div, R_ = 3, 15
    g = torch.Generator().manual_seed(19 + t)
    h = torch.zeros(R_, dec.d_model) if t == 0 else torch.rand(R_, dec.d_model, generator=g) * 2 - 1
    words = torch.randint(0, dec.vocab_size, (R_,), generator=g)
    tags = c["tags"] if t == 0 else None
    rep = lambda x: x.repeat_interleave(div, 0)   # noqa: E731
    emb = R.input_embed(sd, words, None if tags is None else rep(tags), t)
    want = R.step(sd, emb, h, rep(c["mem"]), rep(c["lens"]), rep(c["fc"]))
    sd64 = R.cast(sd, torch.float64)
    want64 = R.step(sd64, emb.double(), h.double(), rep(c["mem"]).double(), rep(c["lens"]), rep(c["fc"]).double())
    mem = dec.memory(c["mem"].cuda(), c["fc"].cuda(), c["lens"], div, L)
    f32 = dict(device="cuda", dtype=torch.float32)
    V, ldl = dec.vocab_size, dec.vocab_size + 3
    state_out, logit = torch.empty(R_, dec.d_model, **f32), torch.zeros(R_, ldl, **f32)
    embed, attn = torch.empty(R_, dec.d_model, **f32), torch.empty(R_, Tm, **f32)
    wbuf = torch.full((R_, 4), -1, device="cuda", dtype=torch.int32)   # word ids at a stride of 4
    wbuf[:, 0] = words.cuda().int()
    dec.step(mem, h.cuda(), state_out, words=wbuf, word_stride=4, tags=None if tags is None else tags.cuda().int(),
             logit=logit, ldl=ldl, embed=embed, attn_weight=attn, attn_strides=(Tm, 1))
    check(f"step t={t} logits", logit[:, :V], want[1], GATE)
    assert not logit[:, V:].any()                       # the pitch beyond V is left alone
    for nm, got, a32, a64 in (("state", state_out, want[0], want64[0]), ("attn_weight", attn, want[2], want64[2])):
        n = float((a32.double() - a64).abs().max())
        check(f"step t={t} {nm} (n {n:.3e})", got, a64, 8 * n)
    assert torch.equal(embed, state_out)
    # the reference's dict contract on the same step (hf_wrapper.py:1513-1554), one row per clip
    res = dec({"word": words[::div].reshape(B, 1).cuda(), "state": h[::div].reshape(1, B, -1).cuda(), "fc_emb": c["fc"].cuda(),
               "attn_emb": c["mem"].cuda(), "attn_emb_len": c["lens"], "temporal_tag": c["tags"], "t": t})
    assert tuple(res["logit"].shape) == (B, 1, V) and tuple(res["embed"].shape) == (B, 1, dec.d_model)
    assert tuple(res["state"].shape) == (1, B, dec.d_model) and tuple(res["attn_weight"].shape) == (B, Tm)
    check(f"forward t={t} logits", res["logit"][:, 0], want[1][::div], GATE)
    n = float((want[2].double() - want64[2]).abs().max())
    check(f"forward t={t} attn_weight", res["attn_weight"], want64[2][::div], 8 * n)


@torch.no_grad()
def test_abi_refuses_before_launching():
    from audiocaption_amd import _lib
    c = case("small_t")
    dec = c["model"].decoder
    lib = _lib.load()
    w = dec.weights()
    assert lib.ac_bah_workspace_floats(ctypes.byref(w), 5, 5, 4096, L) == -1          # more frames than the kernel holds
    bad = _lib.AcBahWeights.from_buffer_copy(w)
    bad.d_model = 100
    assert lib.ac_bah_workspace_floats(ctypes.byref(bad), 5, 5, 70, L) == -1
    mem = dec.memory(c["mem"].cuda(), c["fc"].cuda(), c["lens"], 1, L)
    h = torch.zeros(5, dec.d_model, device="cuda")
    with pytest.raises(_lib.HipLibraryError, match="AC_ERR_ARG"):                     # state_in == state_out
        dec.step(mem, h, h, words=torch.ones(5, device="cuda", dtype=torch.int32),
                 logit=torch.empty(5, dec.vocab_size, device="cuda"))


# ---- (f): sampling ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("method,temp", [("sample", 0.7), ("top5", 0.7), ("top0.9", 1.0), ("gumbel", 1.0)])
def test_sampling(method, temp):
    c = case("small_t")
    model = c["model"]
    a = model(request(c, sample_method=method, temp=temp, seed=1234))
    b = model(request(c, sample_method=method, temp=temp, seed=1234))
    assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["sampled_logprob"], b["sampled_logprob"])
    assert torch.equal(a["logit"], b["logit"])
    other = model(request(c, sample_method=method, temp=temp, seed=99))
    assert not torch.equal(a["seq"], other["seq"])
    # every live step: the word is what the sampler's rule draws from the returned logits, the value what it stores
    code, k, p = R.parse_method(method)
    seq, logit, lp = a["seq"].numpy(), a["logit"].cpu().numpy(), a["sampled_logprob"].numpy()
    live = R.live_mask(seq)
    worst = 0.0
    for t in range(L):
        rows = np.flatnonzero(live[:, t])
        if rows.size == 0:
            continue
        _, _, oks, _ = SR.sample_rows(logit[rows, t], code, k, p, temp, 1234, t, rows=rows)
        for r, ok in zip(rows, oks):
            assert int(seq[r, t]) in ok, (t, r, int(seq[r, t]), ok)
            stored = SR.distribution(logit[r, t], code, k, p, temp)[1][int(seq[r, t])]
            worst = max(worst, abs(stored - lp[r, t]))
    print(f"{method}: max |stored value - rule on the returned logits| {worst:.3e} (gate {GATE:.0e})")
    assert worst <= GATE
    assert not lp[~live].any() and (seq[~live] == 2).all() and not logit[~live].any()
    # the logits are the decoder's on the drawn words: replay them through the restatement
    words = a["seq"]
    replay = R.greedy(c["sd"], c["mem"], c["lens"], c["fc"], c["tags"], L,
                      pick=lambda t, lg: (words[:, t], torch.from_numpy(lp[:, t])))
    assert torch.equal(replay["seq"], words)
    check(f"{method} logits on the drawn words", a["logit"], replay["logit"], GATE)
