"""Repetition and word constraints on the GPU (csrc/logit_rules.hip, ac_trm_search_rules, ac_trm_beam_step_rules,
TransformerModel with the four keys): the kernel alone against the numpy restatement (tests/_logit_rules_ref.py), and the
constrained greedy / beam / sampled searches end to end against the reference searches over the oracle on the four
``g4_greedy`` memories.  tests/test_logit_rules_cpu.py asserts that those inputs are at least 1e-3 away from every tie, so
the ids must agree exactly."""
import ctypes

import numpy as np
import pytest
import torch

import _logit_rules_ref as R
import _sampling_ref as S
from audiocaption_amd import _lib
from audiocaption_amd import sampling as SM

pytestmark = pytest.mark.gpu

END, START = R.END, R.START
TOL = 1e-6           # test_gpu_sampling's ambiguity rule


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import build
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
def _struct(rules, bad_dev, end_idx=END):
    bad = rules.get("bad_words", ())
    return _lib.AcLogitRules(float(rules.get("repetition_penalty", 1.0)), int(rules.get("no_repeat_ngram_size", 0)),
                             int(rules.get("min_length", 0)), end_idx, len(bad), bad_dev.data_ptr() if len(bad) else None)


def _apply(lib, z, tokens, t, rules, ld_in, ld_out):
    """ac_logit_rules_apply on z (R, V) laid out with the two strides; returns the output rows and checks that the input
    plane (padding included) is unchanged."""
    Rn, V = z.shape
    src = torch.full((Rn, ld_in), 7.25, device="cuda:0", dtype=torch.float32)
    src[:, :V] = torch.from_numpy(z).cuda()
    before = src.clone()
    dst = torch.full((Rn, ld_out), -3.5, device="cuda:0", dtype=torch.float32)
    tok = torch.from_numpy(tokens.astype(np.int32)).cuda().contiguous()
    bad = torch.tensor(list(rules.get("bad_words", ())) or [0], device="cuda:0", dtype=torch.int32)
    st = _struct(rules, bad)
    rc = lib.ac_logit_rules_apply(_lib.ptr(src), ld_in, _lib.ptr(dst), ld_out, Rn, V, _lib.ptr(tok), tok.shape[1], t,
                                  ctypes.byref(st), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the input plane was modified"
    assert bool((dst[:, V:] == -3.5).all()), "the output plane's padding was written"
    return dst[:, :V].cpu().numpy()


def _prefixes(gen, rows, V, L=20):
    """Token rows (rows, L + 1): hand-made prefixes first (the CPU test's), then rows over a small pool of words (many
    repeats), then rows over the whole vocabulary."""
    tok = np.empty((rows, L + 1), dtype=np.int64)
    tok[:, 0] = START
    hand = [[5, 7, 9, 5, 7], [3, 3, 3, 3], [9, 9, 9, 9, 9, 1, 4], [5, 7, 5, 9, 5], [5, 7, 9, 7, 5], [END, END, 5, END]]
    for r in range(rows):
        if r < len(hand):
            body = (hand[r] * L)[:L]
        elif r % 2:
            body = gen.integers(3, 9, L).tolist()
        else:
            body = gen.integers(0, V, L).tolist()
        tok[r, 1:] = body
    return tok


KERNEL_RULES = [
    {"repetition_penalty": 1.5, "no_repeat_ngram_size": 3, "bad_words": [3, 8, 41, 77, 99], "min_length": 2},   # all four
    {"repetition_penalty": 1.5}, {"repetition_penalty": 0.75},
    {"no_repeat_ngram_size": 1}, {"no_repeat_ngram_size": 2}, {"no_repeat_ngram_size": 3},
    {"bad_words": [3, 8, 41, 77, 99]}, {"min_length": 2}, {"min_length": 20},
]


@pytest.mark.parametrize("V,ld_in,ld_out", [(100, 100, 100), (4981, 4984, 4984), (16384, 16384, 16384),
                                            (4981, 4981, 4984), (4981, 4984, 4981), (101, 101, 101)])
def test_kernel_against_the_restatement(lib, V, ld_in, ld_out):
    """37 rows (more than one workgroup, not a multiple of anything); every t at which a rule starts to act: 0, 1, n - 2,
    n - 1 (n = 3 in the combined set: 1 and 2) and the last step 19.  Strides: rows that stay 16-byte aligned (the 16-byte
    path) and rows that do not (the scalar path), on either side."""
    gen = np.random.default_rng(V + ld_in)
    rows = 37
    z = gen.normal(0, 3, (rows, V)).astype(np.float32)
    z[:, 4] = 0.0                                              # a zero logit among the penalised words
    tok = _prefixes(gen, rows, V)
    for rules in KERNEL_RULES:
        for t in (0, 1, 2, 19):
            got = _apply(lib, z, tok, t, rules, ld_in, ld_out)
            want = R.apply_rows(z, tok, t, rules)
            banned = np.isneginf(want)
            assert np.array_equal(np.isneginf(got), banned), (rules, t)
            assert np.isfinite(got[~banned]).all()
            same = (want.view(np.int32) == z.view(np.int32))
            assert np.array_equal(got.view(np.int32)[same], z.view(np.int32)[same]), (rules, t)      # untouched: bit-identical
            pen = ~banned & ~same
            assert (np.abs(got[pen] - want[pen]) <= np.spacing(np.abs(want[pen]))).all(), (rules, t)  # within 1 ulp
            if "repetition_penalty" in rules and t == 19:
                assert pen.any()
            if set(rules) - {"repetition_penalty"} and t == 19 and rules.get("min_length", 0) != 2:
                assert banned.any()


def test_kernel_refusals_launch_nothing(lib):
    z = torch.randn(4, 100, device="cuda:0")
    out = torch.full((4, 100), -3.5, device="cuda:0")
    tok = torch.full((4, 21), 5, device="cuda:0", dtype=torch.int32)
    bad = torch.tensor([7], device="cuda:0", dtype=torch.int32)

    def call(st, V=100, t=3, ld_tok=21):
        return lib.ac_logit_rules_apply(_lib.ptr(z), 100, _lib.ptr(out), 100, 4, V, _lib.ptr(tok), ld_tok, t, ctypes.byref(st),
                                        _lib.stream())
    ok = {"repetition_penalty": 1.5, "no_repeat_ngram_size": 1}
    assert call(_struct(ok, bad), V=16385) == _lib.AC_ERR_ARG
    assert call(_struct(ok, bad), t=-1) == _lib.AC_ERR_ARG and call(_struct(ok, bad), t=21) == _lib.AC_ERR_ARG
    st = _struct(ok, bad)
    st.n_bad, st.bad_words = 257, bad.data_ptr()
    assert call(st) == _lib.AC_ERR_ARG
    for rho in (0.0, -2.0, float("inf"), float("nan")):
        assert call(_struct({"repetition_penalty": rho}, bad)) == _lib.AC_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -3.5).all())
    assert call(_struct(ok, bad), t=20) == 0                  # the last column of the token row
    torch.cuda.synchronize()
    assert bool(torch.isneginf(out[:, 5]).all())


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the four memories
# ---------------------------------------------------------------------------------------------------------------------
def _decode(model, method, emb, lens, rules=None, max_length=20, **more):
    d = {"mode": "inference", "sample_method": method, "temp": 1.0, "max_length": max_length}
    d.update(rules or {})
    d.update(more)
    out = model.forward_decoder(d, {"attn_emb": emb.cuda(), "attn_emb_len": lens})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", R.CASES)
def test_greedy_equals_the_reference(diverse_models, name):
    model = diverse_models["greedy"]
    ref, _, (emb, lens) = R.reference("greedy", name)
    out = _decode(model, "greedy", emb, lens, R.case(name, "greedy"))
    seq, lp, logit = out["seq"], out["sampled_logprob"], out["logit"]
    assert seq.dtype == torch.int64 and seq.device.type == "cpu" and seq.shape == (4, 20)
    assert lp.dtype == torch.float32 and lp.device.type == "cpu" and lp.shape == (4, 20)
    assert logit.shape == (4, 20, 4981) and logit.is_cuda and out["embed"].shape == (4, 20, 256)
    assert np.array_equal(seq.numpy(), ref["seq"]), f"{name}:\n{seq.numpy()}\nreference\n{ref['seq']}"
    steps = ref["steps"]
    logit = logit.cpu().numpy()
    assert np.isfinite(logit).all(), "logit holds the RAW logits: no -inf"
    delta = float(np.abs(logit[:, :steps] - ref["logit"][:, :steps]).max())
    print(f"greedy {name}: logits within {delta:.2e} of the oracle, "
          f"logprob within {float(np.abs(lp.numpy() - ref['sampled_logprob']).max()):.2e}")
    assert delta < 1e-4
    assert np.abs(lp.numpy() - ref["sampled_logprob"]).max() < 1e-4
    # the columns of the steps after every row has ended: 0 / end_idx / 0, as the unconstrained chain leaves them
    assert (logit[:, steps:] == 0).all() and (seq[:, steps:] == END).all() and (lp[:, steps:] == 0).all()
    assert bool((out["embed"][:, steps:] == 0).all())
    cnt = out["unfinished_cnt"].cpu().numpy()
    assert cnt.shape == (20,) and (cnt[:steps - 1] > 0).all() and (cnt[steps:] == 0).all()
    assert steps == 20 or cnt[steps - 1] == 0
    assert all(R.holds(c, R.case(name, "greedy")) for c in seq.numpy())


@pytest.mark.parametrize("beam", [2, 3])
@pytest.mark.parametrize("name", R.CASES)
def test_beam_equals_the_reference(diverse_models, name, beam):
    model = diverse_models["greedy"]
    method = f"beam{beam}"
    ref, _, (emb, lens) = R.reference(method, name)
    rules = R.case(name, method)
    out = _decode(model, "beam", emb, lens, rules, beam_size=beam, n_best=True)
    seq = out["seq"].numpy()
    assert seq.shape == (4, beam, 20)
    assert np.array_equal(seq, ref["seq"]), f"{method} {name}:\n{seq}\nreference\n{ref['seq']}"
    best = _decode(model, "beam", emb, lens, rules, beam_size=beam)["seq"].numpy()
    assert np.array_equal(best, ref["seq"][:, 0])
    assert all(R.holds(c, rules) for c in seq.reshape(-1, 20))


def test_banned_and_repeated_words_never_appear(diverse_models):
    """With every clip's unconstrained first word banned and n = 1, no caption holds a banned or a repeated word.  (Before the
    rules were built the keys were ignored: the captions started with the banned words and repeated themselves.)"""
    model = diverse_models["greedy"]
    emb, lens = R.clips(0)
    rules = R.case("bad_n1", "greedy")
    off = _decode(model, "greedy", emb, lens)["seq"].numpy()
    assert sorted(set(off[:, 0].tolist())) == rules["bad_words"]
    got = _decode(model, "greedy", emb, lens, rules)["seq"].numpy()
    for c in got:
        words = c.tolist()
        words = words[:words.index(END)] if END in words else words
        assert not set(words) & set(rules["bad_words"]), c
        assert len(set(words)) == len(words), c
    assert np.array_equal(got, R.search("greedy", "bad_n1", 0)["seq"])
    for beam in (2, 3):
        b = _decode(model, "beam", emb, lens, rules, beam_size=beam, n_best=True)["seq"].numpy()
        assert all(R.holds(c, rules) for c in b.reshape(-1, 20))


def test_wide_beams_take_the_rules_too(diverse_models):
    """Beam sizes above 8 score through the two-kernel form of the beam step (in place, on the constrained plane)."""
    model = diverse_models["greedy"]
    emb, lens = R.clips(0)
    rules = R.case("all", "greedy")
    runs = [_decode(model, "beam", emb, lens, rules, beam_size=10, n_best=True)["seq"] for _ in range(3)]   # eager, capture, replay
    assert runs[0].shape == (4, 10, 20)
    assert torch.equal(runs[1], runs[0]) and torch.equal(runs[2], runs[0])
    assert all(R.holds(c, rules) for c in runs[0].numpy().reshape(-1, 20))
    free = _decode(model, "beam", emb, lens, beam_size=10, n_best=True)["seq"]
    assert not all(R.holds(c, rules) for c in free.numpy().reshape(-1, 20))


@pytest.mark.parametrize("method", ["top5", "top0.9"])
def test_sampling_draws_from_the_constrained_rows(diverse_models, method):
    """test_gpu_sampling.test_end_to_end_vs_oracle with the rules between the oracle's logits and the restated sampler."""
    from oracle import cpu_path as O
    model = diverse_models["greedy"]
    emb, lens = R.clips(0)
    rules = R.case("all", "greedy")
    seed = 0x5eed0002
    out = _decode(model, method, emb, lens, rules, seed=seed)
    seq, lp = out["seq"], out["sampled_logprob"]
    B, L = seq.shape
    code, k, p, t = SM.parse_sample_method(method, 4981, 1.0)
    word = torch.cat([torch.full((B, 1), START, dtype=torch.int64), seq], 1)
    ref = O.decoder_forward(R.state(), word[:, :L], emb, lens.numpy())["logit"]
    got_logit = out["logit"].cpu()
    assert bool(torch.isfinite(got_logit).all())
    cnt = out["unfinished_cnt"].cpu().numpy()
    tokens = word.numpy()
    amb = checked = 0
    unfinished = np.ones(B, dtype=bool)
    for s in range(L):
        if s > 0 and cnt[s - 1] == 0:
            assert torch.all(seq[:, s:] == END) and torch.all(lp[:, s:] == 0)
            break
        delta = float((got_logit[:, s] - ref[:, s]).abs().max())
        assert delta < 1e-4, f"step {s}: logits differ from the oracle by {delta}"
        x_got = R.apply_rows(got_logit[:, s].numpy(), tokens, s, rules)
        x_ref = R.apply_rows(ref[:, s].numpy(), tokens, s, rules)
        rw, rlp, oks, ramb = S.sample_rows(x_got, code, k, p, t, seed, s, tol=TOL)
        ow, olp, ooks, oamb = S.sample_rows(x_ref, code, k, p, t, seed, s, tol=TOL + 4 * delta / min(t, 1.0))
        for b in range(B):
            drawn = int(seq[b, s]) if unfinished[b] else None
            if drawn is not None:
                assert np.isfinite(x_ref[b, drawn]), f"step {s} clip {b}: {drawn} is banned"
                assert drawn in oks[b], f"step {s} clip {b}: {drawn} vs {sorted(oks[b])[:4]}"
                assert drawn in ooks[b], f"step {s} clip {b}: {drawn} vs oracle {sorted(ooks[b])[:4]}"
                amb += int(oamb[b])
                checked += 1
            else:
                assert int(seq[b, s]) == END
            if not ramb[b] and (drawn is None or drawn == rw[b]):
                assert abs(float(lp[b, s]) - rlp[b]) < 1e-5
                if not oamb[b]:
                    assert abs(float(lp[b, s]) - olp[b]) < 1e-4
            if drawn is not None and drawn == END:
                unfinished[b] = False
        assert cnt[s] == int(unfinished.sum())
    assert checked > 0
    assert all(R.holds(c, rules) for c in seq.numpy())
    if code != SM.TOPP:
        assert amb <= max(2, 0.2 * checked), f"{amb} of {checked} draws ambiguous against the oracle"


def test_n_samples_with_rules(diverse_models):
    model = diverse_models["greedy"]
    emb, lens = R.clips(0)
    rules = R.case("all", "greedy")
    out = _decode(model, "top0.9", emb, lens, rules, seed=11, n_samples=3)
    assert out["seq"].shape == (4, 3, 20) and out["seq"].dtype == torch.int64 and out["seq"].device.type == "cpu"
    assert out["sampled_logprob"].shape == (4, 3, 20) and out["logit"].shape == (4, 3, 20, 4981)
    assert out["embed"].shape == (4, 3, 20, 256)
    assert bool(torch.isfinite(out["logit"]).all())
    caps = out["seq"].numpy().reshape(-1, 20)
    assert all(R.holds(c, rules) for c in caps)
    assert len({tuple(c) for c in caps}) > 4                    # the samples of a clip differ
    again = _decode(model, "top0.9", emb, lens, rules, seed=11, n_samples=3)
    assert torch.equal(again["seq"], out["seq"])
    free = _decode(model, "top0.9", emb, lens, seed=11, n_samples=3)["seq"]
    assert not torch.equal(free, out["seq"])


NEUTRAL = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "bad_words": [], "min_length": 0}


def test_neutral_keys_take_the_unconstrained_path(diverse_models):
    model = diverse_models["greedy"]
    dec = model.decoder
    emb, lens = R.clips(0)
    for method, more, states in (("greedy", {}, "_greedy_state"), ("top5", {"seed": 5}, "_sample_state"),
                                 ("beam", {"beam_size": 3}, None)):
        plain = _decode(model, method, emb, lens, **more)
        table = getattr(dec, states) if states else model._beam_state
        keys = list(table)
        uses = table[keys[-1]]["uses"]
        same = _decode(model, method, emb, lens, NEUTRAL, **more)
        assert list(table) == keys and table[keys[-1]]["uses"] == uses + 1          # the same state, used once more
        for k in ("seq", "logit", "sampled_logprob"):
            if method == "beam" and k == "logit":
                continue                                                             # torch.empty in a beam search
            assert torch.equal(plain[k], same[k]), (method, k)
        ruled = _decode(model, method, emb, lens, R.case("all"), **more)
        assert len(table) == len(keys) + 1 or list(table) != keys                   # the rules have a state of their own
        assert not torch.equal(ruled["seq"], plain["seq"])


def test_graphs(diverse_models, monkeypatch):
    model = diverse_models["greedy"]
    emb, lens = R.clips(0)
    cases = [("greedy", R.case("n1"), {}), ("greedy", R.case("n2"), {}), ("greedy", R.case("rho"), {}),
             ("greedy", {"repetition_penalty": 1.25}, {}), ("greedy", R.case("bad"), {}), ("greedy", {"bad_words": [2125]}, {}),
             ("greedy", R.case("min6"), {}), ("greedy", {"min_length": 5}, {}), ("greedy", {}, {}),
             ("beam", R.case("n1"), {"beam_size": 3}), ("beam", R.case("min6"), {"beam_size": 3}), ("beam", {}, {"beam_size": 3}),
             ("top5", R.case("n1"), {"seed": 9}), ("top5", R.case("all"), {"seed": 9})]
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "0")
    want = [_decode(model, m, emb, lens, r, **more) for m, r, more in cases]
    monkeypatch.delenv("AUDIOCAPTION_DECODE_GRAPH")
    assert len({tuple(w["seq"].numpy().reshape(-1)) for w in want[:9]}) >= 6      # the requests really differ
    for _ in range(3):                   # eager, capture, replay of every request, interleaved
        for (m, r, more), w in zip(cases, want):
            got = _decode(model, m, emb, lens, r, **more)
            assert torch.equal(got["seq"], w["seq"]), (m, r)
            assert torch.equal(got["sampled_logprob"], w["sampled_logprob"]), (m, r)
            if m != "beam":
                assert torch.equal(got["logit"], w["logit"]), (m, r)


def test_effb2_and_hf_wrapper_surfaces(state_effb2, hip_model):
    import audiocaption_amd as A
    from audiocaption_amd import procedural as P
    from audiocaption_amd.hf_wrapper import CaptioningModel
    wav = torch.from_numpy(P.synthetic_wav(2, 64000, varied=True))
    model = A.init_model_from_config(A.effb2_trm_config(4981), print_fn=lambda s: None)
    model.load_state_dict(state_effb2, strict=True)
    model = model.eval().to("cuda:0")
    req = {"mode": "inference", "wav": wav.cuda(), "wav_len": [64000, 48000], "specaug": False, "sample_method": "greedy",
           "max_length": 12}
    off = model(dict(req))["seq"]
    bad = sorted({int(w) for w in off[:, 0]} - {END, START})
    rules = {"no_repeat_ngram_size": 2, "bad_words": bad}
    out = model(dict(req, **rules))
    assert out["seq"].shape == (2, 12) and out["seq"].dtype == torch.int64 and out["logit"].shape == (2, 12, 4981)
    assert int(out["seq"].min()) >= 0 and int(out["seq"].max()) < 4981
    assert all(R.holds(c, rules) for c in out["seq"].numpy())
    hf = CaptioningModel(hip_model)
    for method in ("greedy", "beam"):
        free = hf(wav, [64000, 48000], sample_method=method, max_length=10)
        bad = sorted({int(w) for w in free[:, 0]} - {END, START})
        seq = hf(wav, [64000, 48000], sample_method=method, max_length=10, no_repeat_ngram_size=2, bad_words=bad)
        assert seq.shape == (2, 10) and seq.dtype == torch.int64 and seq.device.type == "cpu"
        assert int(seq.min()) >= 0 and int(seq.max()) < 4981
        assert all(R.holds(c, {"no_repeat_ngram_size": 2, "bad_words": bad}) for c in seq.numpy())
