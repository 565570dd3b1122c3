"""The attention-GRU caption decoder (csrc/attn_gru.hip, rnn_decoder.py, attn_model.py) at its declared bounds and on every
route of ac_gemm (csrc/train.hip): the cases of tests/_attn_gru_edges.py - S < 64, 301 and 2048 frames, every dim 1024
with V 16384, lengths 0 / above Tm / below 0, beam 1, 2 and 8, a beam temperature, max_length 1 and 23, the key projection
and the classifier on the nt kernels - against the CPU restatement tests/_attn_gru_ref.py (held to the reference's recorded
steps at the length edges by tests/test_attn_gru_edges_cpu.py).

Gates, the ones tests/test_gpu_attn_gru.py uses.  Ids: identical to the restatement's.  Logits and log-probabilities: within
1e-4 absolute of the f32 restatement.  attn_weight, state, embed: n = the largest deviation of the restatement in f32 from
the restatement in float64 on the same case, gate 8 * n against the float64 values.  ac_gemm alone: max|diff| / max|want|
< 1e-5 against float64.  Every figure is printed before it is asserted; tests/golden/REPORT_attn_gru_edges.txt keeps a run.
"""
import ctypes

import numpy as np
import pytest
import torch

import _attn_gru_edges as E
import _attn_gru_ref as R
import _sampling_ref as SR
from test_gpu_attn_gru import GATE, check, request

pytestmark = pytest.mark.gpu

_CACHE = {}
G = 1024                    # guard floats on either side of a workspace
SENTINEL = 0x7FA5C3E1       # a NaN with a payload no kernel produces


def base(name, kind="t", seed=None):
    """Model and inputs of a case (built once per module)."""
    seed = E.CASES[name]["seed"] if seed is None else seed
    key = ("base", name, kind, seed)
    if key not in _CACHE:
        sd, mem, lens, fc, tags = E.case_inputs(name, kind == "t", seed)
        _CACHE[key] = {"sd": sd, "mem": mem, "lens": lens, "fc": fc, "tags": tags,
                       "model": E.build_model(E.CASES[name]["shape"], kind == "t", sd)}
    return _CACHE[key]


def case(name, kind="t", L=None):
    """``base`` plus the restatement's f32 / float64 greedy runs at max_length L and the error budget n."""
    L = E.CASES[name]["L"] if L is None else L
    key = ("greedy", name, kind, L)
    if key not in _CACHE:
        c = dict(base(name, kind), L=L)
        c["ref32"], c["ref64"], c["live"] = E.greedy_pair(c["sd"], c["mem"], c["lens"], c["fc"], c["tags"], L)
        assert torch.equal(c["ref32"]["seq"], c["ref64"]["seq"])
        gap = float(c["ref32"]["gap"][torch.from_numpy(c["live"])].min())
        assert gap >= GATE, f"{name}: top-1 / top-2 gap {gap:.2e} of the restatement"
        c["n"] = R.error_budget(c["ref32"], c["ref64"], c["live"])
        _CACHE[key] = c
    return _CACHE[key]


def check_greedy(label, c, out):
    L, r32, r64 = c["L"], c["ref32"], c["ref64"]
    live = torch.from_numpy(c["live"])
    B, Tm, _ = c["mem"].shape
    d_model = c["model"].decoder.d_model
    assert out["seq"].dtype == torch.int64 and not out["seq"].is_cuda and not out["sampled_logprob"].is_cuda
    np.testing.assert_array_equal(out["seq"].numpy(), r32["seq"].numpy())
    logit = out["logit"].cpu()
    check(f"{label} logits (every column)", logit, r32["logit"], GATE)
    check(f"{label} sampled_logprob", out["sampled_logprob"], r32["sampled_logprob"], GATE)
    n = c["n"]
    print(f"{label} n (f32 vs float64 restatement): {n}")
    check(f"{label} attn_weight", out["attn_weight"], r64["attn_weight"], 8 * n["attn_weight"])
    check(f"{label} state", out["state"], r64["state"], 8 * n["state"])
    check(f"{label} embed", out["embed"], r64["embed"], 8 * n["embed"])
    assert tuple(out["attn_weight"].shape) == (B, Tm, L) and tuple(out["state"].shape) == (1, B, d_model)
    assert tuple(logit.shape) == (B, L, c["model"].decoder.vocab_size)
    # finished-row contract: after a row's first <end> everything reads <end> / 0
    dead = ~live
    assert not logit[dead].any() and not out["embed"].cpu()[dead].any() and not out["sampled_logprob"][dead].any()
    assert not out["attn_weight"].cpu().transpose(1, 2)[dead].any()
    assert (out["seq"][dead] == 2).all()
    np.testing.assert_array_equal(out["unfinished_cnt"].cpu().numpy(), r32["unfinished_cnt"].numpy())
    # masked frames weigh exactly 0, live columns sum to 1, a clip without a frame weighs every frame 1 / Tm
    w = out["attn_weight"].cpu()
    worst_sum, worst_uniform = 0.0, 0.0
    for i, ln in enumerate(c["lens"].tolist()):
        ln = min(max(ln, 0), Tm)
        if ln > 0:
            assert not w[i, ln:, :].any(), f"clip {i}: weight on a masked frame"
        cols = w[i][:, live[i]].double()
        worst_sum = max(worst_sum, float((cols.sum(0) - 1).abs().max()))
        if ln == 0:
            worst_uniform = max(worst_uniform, float((cols - 1.0 / Tm).abs().max()))
    empty = sum(1 for ln in c["lens"].tolist() if ln <= 0)
    print(f"{label} max |sum of a live column - 1| {worst_sum:.3e} (gate {2 * Tm * 2.0 ** -24:.3e}); "
          f"{empty} clips of length 0: max |weight - 1/Tm| {worst_uniform:.3e} "
          f"(gate {float(np.spacing(np.float32(1.0 / Tm))):.3e})")
    assert worst_sum <= 2 * Tm * 2.0 ** -24
    assert worst_uniform <= float(np.spacing(np.float32(1.0 / Tm)))


# ---- greedy, every case -----------------------------------------------------------------------------------------------------
GREEDY = [("narrow", "t"), ("narrow", "p"), ("long", "t"), ("long", "p"), ("full", "t"), ("wide", "t"), ("routes-1", "t"),
          ("routes-2", "t")]


def test_case_table_reaches_every_gemm_route():
    reached = E.assert_route_coverage()
    for rt, who in sorted(reached.items()):
        print(f"{rt}: {len(who)} decoder GEMMs, e.g. {who[0]}")


@torch.no_grad()
@pytest.mark.parametrize("name,kind", GREEDY)
def test_greedy(name, kind):
    c = case(name, kind)
    out = c["model"](request(c, max_length=c["L"]))
    check_greedy(f"{name}_{kind}", c, out)


# ---- lengths above Tm and below 0 ----------------------------------------------------------------------------------------------
def run_step(dec, mem, fc, lens, tags, t, h, words, div, L=20, handle=None):
    """One ac_bah_step_logits over div rows per clip: (state, logit with a pitch of V + 3, embed, attn_weight)."""
    B, Tm, _ = mem.shape
    rows, V = B * div, dec.vocab_size
    handle = dec.memory(mem.cuda(), fc.cuda(), lens, div, L) if handle is None else handle
    f32 = dict(device="cuda", dtype=torch.float32)
    state_out, logit = torch.empty(rows, dec.d_model, **f32), torch.zeros(rows, V + 3, **f32)
    embed, attn = torch.empty(rows, dec.d_model, **f32), torch.empty(rows, Tm, **f32)
    wbuf = torch.full((rows, 4), -1, device="cuda", dtype=torch.int32)   # word ids at a stride of 4
    wbuf[:, 0] = words.cuda().int()
    dec.step(handle, h.cuda(), state_out, words=wbuf, word_stride=4, tags=tags.cuda().int() if t == 0 else None,
             logit=logit, ldl=V + 3, embed=embed, attn_weight=attn, attn_strides=(Tm, 1))
    return state_out, logit, embed, attn


def step_inputs(c, t, div, seed):
    dec = c["model"].decoder
    rows = c["mem"].shape[0] * div
    g = torch.Generator().manual_seed(seed + t)
    h = torch.zeros(rows, dec.d_model) if t == 0 else torch.rand(rows, dec.d_model, generator=g) * 2 - 1
    return h, torch.randint(0, dec.vocab_size, (rows,), generator=g)


@torch.no_grad()
def test_lengths_outside_the_memory():
    """len = Tm + 5 reads as len = Tm and len = -3 as len = 0, bit for bit (the kernel clamps to [0, Tm])."""
    c = case("long", "t")
    B, Tm, _ = c["mem"].shape
    assert c["lens"].tolist()[0] == Tm and c["lens"].tolist()[3] == 0
    above, below = c["lens"].clone(), c["lens"].clone()
    above[0], below[3] = Tm + 5, -3
    want = c["model"](request(c, max_length=c["L"]))
    got = c["model"](request(dict(c, lens=above), max_length=c["L"]))
    for k in ("seq", "logit", "sampled_logprob", "embed", "attn_weight", "state", "unfinished_cnt"):
        assert torch.equal(got[k], want[k]), f"greedy with len = Tm + 5: {k} differs from len = Tm"
    dec = c["model"].decoder
    for t in (0, 3):
        h, words = step_inputs(c, t, 3, 41)
        ref = run_step(dec, c["mem"], c["fc"], c["lens"], c["tags"], t, h, words, 3)
        for what, lens in (("Tm + 5", above), ("-3", below)):
            res = run_step(dec, c["mem"], c["fc"], lens, c["tags"], t, h, words, 3)
            for nm, a, b in zip(("state", "logit", "embed", "attn_weight"), res, ref):
                assert torch.equal(a, b), f"step t={t} with len = {what}: {nm} differs"
        w = ref[3][9:12].double().cpu()   # the rows of the length-0 clip
        assert float((w - 1.0 / Tm).abs().max()) <= float(np.spacing(np.float32(1.0 / Tm)))


# ---- the decoder step alone ------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("t", [0, 3])
@pytest.mark.parametrize("name", ["narrow", "long", "g20"])
def test_step_alone(name, t):
    """ac_bah_step_logits over 3 rows per clip, t = 0 with the tags and t = 3 with a state in (-1, 1), against the
    restatement's step; "g20": the inputs of tests/golden/g20_attn_gru_edges.npz, against the reference's recorded step."""
    div = 3
    rep = lambda x: x.repeat_interleave(div, 0)   # noqa: E731
    if name == "g20":
        if "g20" not in _CACHE:
            sd, mem, lens, fc, tags = E.g20_inputs()
            _CACHE["g20"] = {"sd": sd, "mem": mem, "lens": lens, "fc": fc, "tags": tags,
                             "model": E.build_model(E.G20_SHAPE, True, sd)}
        c = _CACHE["g20"]
        h, words = (rep(x) for x in E.g20_step_inputs(c["sd"], t))
    else:
        c = base(name)
        h, words = step_inputs(c, t, div, 43)
    sd, dec = c["sd"], c["model"].decoder
    V = dec.vocab_size
    emb = R.input_embed(sd, words, rep(c["tags"]), t)
    want = R.step(sd, emb, h, rep(c["mem"]), rep(c["lens"]), rep(c["fc"]))
    want64 = R.step(R.cast(sd, torch.float64), emb.double(), h.double(), rep(c["mem"]).double(), rep(c["lens"]),
                    rep(c["fc"]).double())
    state, logit, embed, attn = run_step(dec, c["mem"], c["fc"], c["lens"], c["tags"], t, h, words, div)
    check(f"{name} step t={t} logits", logit[:, :V], want[1], GATE)
    assert not logit[:, V:].any()                       # the pitch beyond V is left alone
    for nm, got, a32, a64 in (("state", state, want[0], want64[0]), ("attn_weight", attn, want[2], want64[2])):
        n = float((a32.double() - a64).abs().max())
        check(f"{name} step t={t} {nm} (n {n:.3e})", got, a64, 8 * n)
    assert torch.equal(embed, state)
    if name == "g20":
        g = E.load_g20()
        tv, ti = logit[:, :V].cpu().topk(8, dim=1)
        np.testing.assert_array_equal(ti.numpy(), np.repeat(g[f"t{t}_top_idx"], div, 0))
        check(f"g20 step t={t} top-8 logits (fixture)", tv, np.repeat(g[f"t{t}_top_val"], div, 0), GATE)
        check(f"g20 step t={t} state (fixture)", state, np.repeat(g[f"t{t}_state"], div, 0), GATE)
        check(f"g20 step t={t} attn_weight (fixture)", attn, np.repeat(g[f"t{t}_attn_weight"], div, 0), GATE)
        assert torch.equal(attn[12:15], attn[0:3])      # length 306 over 301 frames: the length-301 rows of the same memory


# ---- beam -------------------------------------------------------------------------------------------------------------------------
def check_beam(name, k, temp, L, seed):
    c = base(name, "t", seed)
    key = ("beam", name, k, temp, L, seed)
    if key not in _CACHE:
        _CACHE[key] = E.beam_pair(c["sd"], c["mem"], c["lens"], c["fc"], c["tags"], k, L, temp)
    r32, r64, nb32, nb64, margin, steps = _CACHE[key]
    label = f"{name} beam {k} temp {temp} L {L}"
    print(f"{label}: smallest margin at the cut {margin:.3e}, steps per clip {steps[:8]}")
    assert margin >= GATE and torch.equal(r32["seq"], r64["seq"]) and torch.equal(nb32["seq"], nb64["seq"])
    out = c["model"](request(c, sample_method="beam", beam_size=k, temp=temp, max_length=L))
    np.testing.assert_array_equal(out["seq"].numpy(), r32["seq"].numpy())
    nb = c["model"](request(c, sample_method="beam", beam_size=k, temp=temp, max_length=L, n_best=True, n_best_size=k))
    np.testing.assert_array_equal(nb["seq"].numpy(), nb32["seq"].numpy())
    n = float((r32["attn_weight"].double() - r64["attn_weight"]).abs().max())
    print(f"{label} n (attn_weight, f32 vs float64 restatement): {n:.3e}")
    check(f"{label} attn_weight", out["attn_weight"], r64["attn_weight"], 8 * n)
    check(f"{label} attn_weight (n-best run)", nb["attn_weight"], r64["attn_weight"], 8 * n)
    assert tuple(out["attn_weight"].shape) == (c["mem"].shape[0], c["mem"].shape[1], L)
    for i, st in enumerate(steps):   # columns the clip's search never reached
        assert not out["attn_weight"][i, :, st:].any()


BEAMS = [(name, k, temp) for name in ("narrow", "long", "routes-1") for (k, temp) in E.CASES[name]["beam_seed"]]


@torch.no_grad()
@pytest.mark.parametrize("name,k,temp", BEAMS)
def test_beam(name, k, temp):
    c0 = E.CASES[name]
    assert k <= c0["shape"]["vocab_size"]
    check_beam(name, k, temp, c0.get("beam_L", c0["L"]), c0["beam_seed"][(k, temp)])


def test_beam_cases_cover_the_declared_range():
    assert set(BEAMS) == {("narrow", 1, 1.0), ("narrow", 2, 1.0), ("narrow", 8, 1.0), ("long", 1, 1.0), ("long", 2, 1.0),
                          ("long", 8, 1.0), ("long", 3, 0.7), ("long", 3, 1.0), ("routes-1", 4, 1.0)}


# ---- sampling ---------------------------------------------------------------------------------------------------------------------
def check_sampling(name, method, temp, L, seed=1234):
    """test_gpu_attn_gru.test_sampling's three checks: the same seed draws the same words; every live word is one the
    sampler's rule draws from the returned logits and the stored value is the rule's; the logits are the decoder's on the
    drawn words (replayed through the restatement)."""
    c = base(name)
    model = c["model"]
    a = model(request(c, sample_method=method, temp=temp, seed=seed, max_length=L))
    b = model(request(c, sample_method=method, temp=temp, seed=seed, max_length=L))
    assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["sampled_logprob"], b["sampled_logprob"])
    assert torch.equal(a["logit"], b["logit"]) and torch.equal(a["attn_weight"], b["attn_weight"])
    code, k, p = R.parse_method(method)
    seq, logit, lp = a["seq"].numpy(), a["logit"].cpu().numpy(), a["sampled_logprob"].numpy()
    live = R.live_mask(seq)
    worst = 0.0
    for t in range(L):
        rows = np.flatnonzero(live[:, t])
        if rows.size == 0:
            continue
        _, _, oks, _ = SR.sample_rows(logit[rows, t], code, k, p, temp, seed, t, rows=rows)
        for r, ok in zip(rows, oks):
            assert int(seq[r, t]) in ok, (t, r, int(seq[r, t]), ok)
            stored = SR.distribution(logit[r, t], code, k, p, temp)[1][int(seq[r, t])]
            worst = max(worst, abs(stored - lp[r, t]))
    print(f"{name} {method} L {L}: max |stored value - rule on the returned logits| {worst:.3e} (gate {GATE:.0e}); "
          f"lengths {live.sum(1).tolist()}")
    assert worst <= GATE
    assert not lp[~live].any() and (seq[~live] == 2).all() and not logit[~live].any()
    words = a["seq"]
    replay = R.greedy(c["sd"], c["mem"], c["lens"], c["fc"], c["tags"], L,
                      pick=lambda t, lg: (words[:, t], torch.from_numpy(lp[:, t])))
    assert torch.equal(replay["seq"], words)
    check(f"{name} {method} L {L} logits on the drawn words", a["logit"], replay["logit"], GATE)


@torch.no_grad()
@pytest.mark.parametrize("name,method,temp", [("wide", "top0.9", 1.0), ("narrow", "top5", 0.7)])
def test_sampling_at_the_vocabulary_bounds(name, method, temp):
    check_sampling(name, method, temp, E.CASES[name]["L"])


# ---- max_length 1 and 23 ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("L", E.MAX_LENGTHS)
def test_max_length(L):
    """max_length 1: no step has a ``stop`` word.  23: above 16, so the host's polls of the beam search at t = 8 / 12 / 16
    are not the last thing before the loop ends; and odd - with "narrow"'s odd V (33) the row pitch max_length * V of the
    logits is odd and the pick and sampling kernels never take 16-byte loads ("long"'s V 516 keeps them on every step)."""
    for kind in ("t", "p"):
        c = case("long", kind, L)
        check_greedy(f"long_{kind} max_length {L}", c, c["model"](request(c, max_length=L)))
    check_beam("long", 3, 1.0, L, E.CASES["long"]["beam_seed"][(3, 1.0)])
    if L > 1:
        check_sampling("long", "top5", 0.7, L)
        assert (L * E.CASES["narrow"]["shape"]["vocab_size"]) % 2 == 1
        for kind in ("t", "p"):
            c = case("narrow", kind, L)
            check_greedy(f"narrow_{kind} max_length {L}", c, c["model"](request(c, max_length=L)))
        check_sampling("narrow", "top5", 0.7, L)


# ---- workspace guard ------------------------------------------------------------------------------------------------------------------
def guarded_memory(dec, c, div, L):
    """``dec.memory`` with the workspace in the middle of a sentinel-filled buffer: (handle, buffer, workspace floats)."""
    from audiocaption_amd import _lib, kernels as K
    lib, w = _lib.load(), dec.weights()
    B, Tm, _ = c["mem"].shape
    n = lib.ac_bah_workspace_floats(ctypes.byref(w), B, B * div, Tm, L)
    assert n > 0
    buf = torch.full((n + 2 * G,), SENTINEL, device="cuda", dtype=torch.int32)
    ws = buf.view(torch.float32)[G:G + n]
    attn_emb, fc = c["mem"].cuda(), c["fc"].cuda()
    handle = {"attn_emb": attn_emb, "len": K.upload(c["lens"], attn_emb.device, torch.int32), "B": B, "R": B * div, "Tm": Tm,
              "max_length": L, "row_div": div, "ws": ws, "fc": fc}
    _lib.check(lib.ac_bah_memory(ctypes.byref(w), _lib.ptr(attn_emb), _lib.ptr(fc), B, B * div, Tm, L, _lib.ptr(ws),
                                 _lib.stream()), "ac_bah_memory")
    return handle, buf, n


def guards_intact(buf, n):
    torch.cuda.synchronize()
    lo, hi = buf[:G].cpu().numpy(), buf[G + n:].cpu().numpy()
    assert hi.size == G
    assert (lo == SENTINEL).all(), f"{int((lo != SENTINEL).sum())} words written below the workspace"
    assert (hi == SENTINEL).all(), f"{int((hi != SENTINEL).sum())} words written above the workspace (first at +{int(np.flatnonzero(hi != SENTINEL)[0])})"
    assert (buf[G:G + n] != SENTINEL).any()


@torch.no_grad()
@pytest.mark.parametrize("L", [7, 6])
def test_workspace_guard_greedy(L):
    """narrow, R = B = 3.  max_length 6: R * (max_len + 1) = 21 is not a multiple of 4 - the int array is rounded up and the
    byte mask ends mid-word; max_length 7 (24 ints, 24 bytes) fills its words exactly."""
    c = base("narrow")
    dec = c["model"].decoder
    tags = c["tags"].cuda().int()
    handle, buf, n = guarded_memory(dec, c, 1, L)
    got = dec.greedy(handle, tags, 1, 2, 0)
    guards_intact(buf, n)
    want = dec.greedy(dec.memory(c["mem"].cuda(), c["fc"].cuda(), c["lens"], 1, L), tags, 1, 2, 0)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    ref = case("narrow", "t", L)
    np.testing.assert_array_equal(got["seq"].cpu().numpy(), ref["ref32"]["seq"].numpy())


@torch.no_grad()
def test_workspace_guard_step():
    """long, R = 12 (3 rows per clip): ac_bah_memory and one ac_bah_step_logits inside the guarded workspace."""
    c = base("long")
    dec = c["model"].decoder
    h, words = step_inputs(c, 3, 3, 47)
    handle, buf, n = guarded_memory(dec, c, 3, 20)
    got = run_step(dec, c["mem"], c["fc"], c["lens"], c["tags"], 3, h, words, 3, handle=handle)
    guards_intact(buf, n)
    want = run_step(dec, c["mem"], c["fc"], c["lens"], c["tags"], 3, h, words, 3)
    for nm, a, b in zip(("state", "logit", "embed", "attn_weight"), got, want):
        assert torch.equal(a, b), nm


# ---- ac_gemm alone at the decoder's operand layouts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("route,name,which,beam", [("kk", "long", "gi", 3), ("general", "long", "ek", 1),
                                                   ("nt<1>", "routes-1", "ek", 1), ("nt<1>", "routes-1", "classifier", 1),
                                                   ("nt<2>", "routes-2", "ek", 1)])
def test_gemm_at_the_decoder_layouts(route, name, which, beam):
    """One product per route with (M, N, K) of a decoder GEMM of the case table: the weight d floats into a [N][d + K]
    matrix, the output one float into its buffer with a pitch of N + 3, a bias; against float64 with the exact-f32 gate of
    test_gpu_train.test_general_gemm_all_layouts.  The pad columns and the float before the base keep their sentinel."""
    from audiocaption_amd import _lib
    lib = _lib.load()
    M, N, K, rt = E.case_routes(name, beam)[which]
    d = E.CASES[name]["shape"]["d_model"]
    assert rt == route == E.gemm_route(M, N, K, aligned=d % 4 == 0, pitches_mod4=(d + K) % 4 == 0 and K % 4 == 0)
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, d + K, generator=g), torch.randn(N, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    sentinel = 1.25e30
    buf = torch.full((1 + M * (N + 3),), sentinel, device="cuda")
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + 4 * off)   # noqa: E731
    rc = lib.ac_gemm(at(xd, 0), K, 1, at(wd, d), 1, d + K, at(buf, 1), N + 3, M, N, K, at(bd, 0), 0, 0.0, 1, 0.0, 0, None, 0,
                     None, 0, _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out = buf[1:].view(M, N + 3).cpu()
    want = x.double() @ w[:, d:].double().t() + b.double()
    diff = (out[:, :N].double() - want).abs()
    rel = float(diff.max()) / float(want.abs().max())
    print(f"ac_gemm {route} {which} of {name} ({M} x {N} x {K}): max|diff| / max|want| = {rel:.3e} (gate 1e-5); "
          f"worst row {int(diff.max(1).values.argmax())}, worst column {int(diff.max(0).values.argmax())}")
    assert rel < 1e-5
    assert (out[:, N:] == sentinel).all(), "a pad column was written"
    assert bool((buf[:1].cpu() == sentinel).all()), "the float before the output base was written"
