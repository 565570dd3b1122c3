"""On-device caption sampling (csrc/sample.hip, ac_sample_rows / ac_trm_sample, TransformerModel.sample_search) against the
numpy restatement of base.py:214-252 (tests/_sampling_ref.py) fed the same Philox stream, and end to end against the oracle.

Ambiguity: a draw whose u * total lies within TOL * total of a CDF boundary (or a top-p row whose cumulative mass lies within
TOL of p at the cut) may take the neighbouring word; everything else must match exactly.  TOL = 1e-6 for the kernel on its
own inputs (f32 prefix sums and expf are good to a few 1e-7 of the total); stricter than 1e-5, which at V = 4981 would call
~10 % of flat-row draws ambiguous."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _sampling_ref as S
from audiocaption_amd import _lib
from audiocaption_amd import sampling as SM

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TOL = 1e-6
END = 2


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import build
    build.build()
    return _lib.load()


def _rows(lib, logits, method, k, p, temp, seed, step):
    """ac_sample_rows on a (R, V) f32 tensor -> (words, logprobs) on the host."""
    x = logits.to("cuda:0", torch.float32).contiguous()
    R, V = x.shape
    word = torch.empty(R, device="cuda:0", dtype=torch.int32)
    lp = torch.empty(R, device="cuda:0", dtype=torch.float32)
    sd = torch.tensor([SM.seed_word(seed)], device="cuda:0", dtype=torch.int64)
    _lib.check(lib.ac_sample_rows(_lib.ptr(x), V, R, V, method, k, float(p), float(temp), _lib.ptr(sd), step,
                                  _lib.ptr(word), _lib.ptr(lp), _lib.stream()), "ac_sample_rows")
    torch.cuda.synchronize()
    return word.cpu().numpy(), lp.cpu().numpy()


def _compare(words, lps, logits, method, k, p, temp, seed, step, where, lp_tol=1e-5):
    """Exact words (ambiguity rule), logprob within lp_tol; returns the number of ambiguous draws."""
    rw, rlp, oks, amb = S.sample_rows(logits, method, k, p, temp, seed, step, tol=TOL)
    for r in range(len(words)):
        assert int(words[r]) in oks[r], f"{where} row {r}: word {int(words[r])}, restatement {sorted(oks[r])[:5]}"
        if int(words[r]) == rw[r] and not amb[r]:
            assert abs(float(lps[r]) - rlp[r]) <= lp_tol, f"{where} row {r}: logprob {lps[r]} vs {rlp[r]}"
    return int(amb.sum())


METHODS = [("sample", 0.7), ("sample", 1.3), ("top5", 0.7), ("top50", 1.0), ("top1", 1.0), ("top0.5", 1.0),
           ("top0.9", 1.0), ("gumbel", 1.0)]


def test_kernel_on_golden_rows(lib):
    g = np.load(os.path.join(GOLDEN, "g14_sampling.npz"))
    x = g["logits"]
    for method, temp in METHODS:
        code, k, p, t = SM.parse_sample_method(method, x.shape[1], temp)
        for seed in (0, 1, 0xfedcba9876543210):
            for step in (0, 5, 19):
                w, lp = _rows(lib, torch.from_numpy(x), code, k, p, t, seed, step)
                _compare(w, lp, x, code, k, p, t, seed, step, f"g14 {method} seed {seed} step {step}")


@pytest.mark.parametrize("V", [4981, 100, 2048, 8000, 16384])
def test_kernel_on_random_rows(lib, V):
    """4096 rows (at V = 4981; 512 at the other widths: every register-tile size) over several (seed, step) pairs."""
    gen = np.random.default_rng(V)
    n_rows = 4096 if V == 4981 else 512
    per = 512
    total = amb = 0
    for method, temp in METHODS:
        code, k, p, t = SM.parse_sample_method(method, V, temp)
        for j in range(n_rows // per):
            x = (gen.normal(0, gen.uniform(1, 4), (per, V))).astype(np.float32)
            if j % 2:                                   # exact ties at the head of every row
                x[:, 7] = x[:, 3] = x.max(1)
            seed, step = int(gen.integers(0, 2 ** 63)), int(gen.integers(0, 30))
            w, lp = _rows(lib, torch.from_numpy(x), code, k, p, t, seed, step)
            amb += _compare(w, lp, x, code, k, p, t, seed, step, f"V {V} {method} block {j}")
            total += per
    # ~2 * TOL boundaries' worth of the CDF per kept word: the ambiguous share grows with V (1 % at the AudioCaps vocabulary)
    assert amb <= 0.01 * max(1.0, V / 4981) * total, f"{amb} of {total} draws ambiguous"


def _chi2_sf(stat, df):
    return float(torch.special.gammaincc(torch.tensor(df / 2.0, dtype=torch.float64),
                                         torch.tensor(stat / 2.0, dtype=torch.float64)))


@pytest.mark.parametrize("method,temp", [("sample", 0.8), ("top20", 1.2), ("top0.8", 1.0), ("gumbel", 2.0), ("top1", 0.5)])
def test_draws_follow_the_distribution(lib, method, temp):
    V = 4981
    x = np.random.default_rng(7).normal(0, 2.5, V).astype(np.float32)
    code, k, p, t = SM.parse_sample_method(method, V, temp)
    rows = torch.from_numpy(np.repeat(x[None], 4096, 0))
    # 2^16 draws.  The kernel's draws equal the restatement's for the same stream (tests above), so for this fixed seed the
    # statistic is deterministic; its p-values over other seeds are uniform
    draws = np.concatenate([_rows(lib, rows, code, k, p, t, 2024, step)[0] for step in range(16)])
    w, _, _ = S.distribution(x, code, k, p, t)
    prob = w / w.sum()
    support = set(np.flatnonzero(prob > 0).tolist())
    assert set(np.unique(draws).tolist()) <= support
    if method == "top1":
        assert np.all(draws == int(np.argmax(x)))
        return
    counts = np.bincount(draws, minlength=V).astype(np.float64)
    expect = prob * draws.shape[0]
    big = expect >= 5
    obs = np.concatenate([counts[big], [counts[~big].sum()]])
    exp = np.concatenate([expect[big], [expect[~big].sum()]])
    if exp[-1] < 5:
        obs, exp = obs[:-1], exp[:-1]
    stat = float(((obs - exp) ** 2 / exp).sum())
    pval = _chi2_sf(stat, len(obs) - 1)
    assert pval > 1e-3, f"{method}: chi2 {stat:.1f} over {len(obs) - 1} dof, p = {pval:.2e}"


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g4():
    g = np.load(os.path.join(GOLDEN, "g4_greedy.npz"))
    return torch.from_numpy(g["attn_emb"]), torch.from_numpy(g["attn_emb_len"])


def _clips(n=8):
    emb, lens = _g4()
    e = torch.cat([torch.roll(emb[i % 4:i % 4 + 1], i // 4, dims=1) for i in range(n)]).contiguous()
    return e, torch.cat([lens[i % 4:i % 4 + 1] for i in range(n)])


def _decode(model, method, temp=1.0, max_length=20, seed=None, emb=None, lens=None):
    if emb is None:
        emb, lens = _clips()
    d = {"mode": "inference", "sample_method": method, "temp": temp, "max_length": max_length}
    if seed is not None:
        d["seed"] = seed
    out = model.forward_decoder(d, {"attn_emb": emb.cuda(), "attn_emb_len": lens})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("method,temp", [("top10", 1.0), ("top0.9", 1.0), ("sample", 1.3)])
def test_end_to_end_vs_oracle(diverse_models, state4981, method, temp):
    from audiocaption_amd import procedural as P
    from oracle import cpu_path as O
    model = diverse_models["greedy"]
    st = dict(state4981)
    st.update(P.to_torch(P.decoder_state_diverse("greedy", vocab_size=4981)))
    emb, lens = _clips()
    seed = 0x5eed0001
    out = _decode(model, method, temp, seed=seed, emb=emb, lens=lens)
    seq, lp = out["seq"], out["sampled_logprob"]
    B, L = seq.shape
    assert seq.dtype == torch.int64 and lp.dtype == torch.float32 and seq.device.type == "cpu"
    code, k, p, t = SM.parse_sample_method(method, 4981, temp)
    # teacher-force the sampled words through the oracle
    word = torch.cat([torch.full((B, 1), 1, dtype=torch.int64), seq], 1)
    ref = O.decoder_forward(st, word[:, :L], emb, lens.numpy())["logit"]
    got_logit = out["logit"].cpu()
    cnt = out["unfinished_cnt"].cpu().numpy()
    amb = checked = 0
    unfinished = np.ones(B, dtype=bool)
    for s in range(L):
        if s > 0 and cnt[s - 1] == 0:       # the reference loop stopped: columns keep end_idx / 0
            assert torch.all(seq[:, s:] == END) and torch.all(lp[:, s:] == 0)
            break
        x_ref = ref[:, s].numpy()
        delta = float((got_logit[:, s] - ref[:, s]).abs().max())
        assert delta < 1e-4, f"step {s}: logits differ from the oracle by {delta}"
        # the kernel on its own logits: exact up to TOL; on the oracle's: up to what the logit difference allows
        rw, rlp, oks, ramb = S.sample_rows(got_logit[:, s].numpy(), code, k, p, t, seed, s, tol=TOL)
        ow, olp, ooks, oamb = S.sample_rows(x_ref, code, k, p, t, seed, s, tol=TOL + 4 * delta / min(t, 1.0))
        for b in range(B):
            drawn = int(seq[b, s]) if unfinished[b] else None
            if drawn is not None:
                assert drawn in oks[b], f"step {s} clip {b}: {drawn} vs {sorted(oks[b])[:4]}"
                assert drawn in ooks[b], f"step {s} clip {b}: {drawn} vs oracle {sorted(ooks[b])[:4]}"
                amb += int(oamb[b])
                checked += 1
            else:
                assert int(seq[b, s]) == END                   # finished rows emit end_idx
            if not ramb[b] and (drawn is None or drawn == rw[b]):
                assert abs(float(lp[b, s]) - rlp[b]) < 1e-5
                if not oamb[b]:
                    assert abs(float(lp[b, s]) - olp[b]) < 1e-4
            if drawn is not None and drawn == END:
                unfinished[b] = False
        assert cnt[s] == int(unfinished.sum())
    assert checked > 0
    if code != SM.TOPP:   # top-p on a high-entropy row: the cut almost always lies within the logit difference of p
        assert amb <= max(2, 0.2 * checked), f"{amb} of {checked} draws ambiguous against the oracle"


def test_seed_reproducibility_and_graph_replay(diverse_models, monkeypatch):
    model = diverse_models["greedy"]
    runs = [_decode(model, "top0.9", seed=42) for _ in range(3)]      # eager, capture, replay
    for r in runs[1:]:
        assert torch.equal(r["seq"], runs[0]["seq"]) and torch.equal(r["sampled_logprob"], runs[0]["sampled_logprob"])
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "0")
    eager = _decode(model, "top0.9", seed=42)
    monkeypatch.delenv("AUDIOCAPTION_DECODE_GRAPH")
    assert torch.equal(eager["seq"], runs[0]["seq"])
    other = [_decode(model, "top0.9", seed=s)["seq"] for s in (43, 44)]   # the same replayed graph, new seeds
    assert not torch.equal(other[0], runs[0]["seq"]) and not torch.equal(other[1], other[0])
    again = _decode(model, "top0.9", seed=42)
    assert torch.equal(again["seq"], runs[0]["seq"])


def test_torch_manual_seed_reproduces_without_a_seed(diverse_models):
    model = diverse_models["greedy"]
    torch.manual_seed(11)
    a = _decode(model, "sample", 1.2)["seq"]
    torch.manual_seed(11)
    b = _decode(model, "sample", 1.2)["seq"]
    torch.manual_seed(12)
    c = _decode(model, "sample", 1.2)["seq"]
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_method_changes_never_replay_the_wrong_graph(diverse_models, monkeypatch):
    model = diverse_models["greedy"]
    cases = [("top5", 1.0), ("top0.9", 1.0), ("sample", 0.7), ("sample", 1.5), ("gumbel", 1.0), ("top1", 1.0)]
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "0")
    want = {c: _decode(model, c[0], c[1], seed=9)["seq"] for c in cases}
    monkeypatch.delenv("AUDIOCAPTION_DECODE_GRAPH")
    for _ in range(3):                   # eager, capture, replay for every case, interleaved
        for c in cases:
            assert torch.equal(_decode(model, c[0], c[1], seed=9)["seq"], want[c]), c


def test_top1_and_cold_sampling_reduce_to_greedy(diverse_models, hip_model, monkeypatch):
    model = diverse_models["greedy"]
    monkeypatch.setenv("AUDIOCAPTION_GREEDY", "chain")      # the launch chain: the same kernels as the sampled search
    greedy = _decode(model, "greedy")
    monkeypatch.delenv("AUDIOCAPTION_GREEDY")
    for temp in (0.3, 1.0, 2.5):
        t1 = _decode(model, "top1", temp, seed=5)
        assert torch.equal(t1["seq"], greedy["seq"])
        assert torch.equal(t1["logit"], greedy["logit"])
    emb, lens = _g4()
    g = _decode(hip_model, "greedy", emb=emb, lens=lens)
    cold = _decode(hip_model, "sample", 1e-4, seed=77, emb=emb, lens=lens)
    assert torch.equal(cold["seq"], g["seq"])


def test_effb2_and_hf_wrapper_surfaces(state_effb2, hip_model):
    import audiocaption_amd as A
    from audiocaption_amd import procedural as P
    from audiocaption_amd.hf_wrapper import CaptioningModel
    wav = torch.from_numpy(P.synthetic_wav(2, 64000, varied=True))
    model = A.init_model_from_config(A.effb2_trm_config(4981), print_fn=lambda s: None)
    model.load_state_dict(state_effb2, strict=True)
    model = model.eval().to("cuda:0")
    out = model({"mode": "inference", "wav": wav.cuda(), "wav_len": [64000, 48000], "specaug": False,
                 "sample_method": "top0.9", "max_length": 12, "seed": 3})
    assert out["seq"].shape == (2, 12) and out["seq"].dtype == torch.int64
    assert out["sampled_logprob"].shape == (2, 12) and out["logit"].shape == (2, 12, 4981)
    assert int(out["seq"].min()) >= 0 and int(out["seq"].max()) < 4981
    hf = CaptioningModel(hip_model)
    torch.manual_seed(0)
    seq = hf(wav, [64000, 48000], sample_method="top0.9", max_length=10)
    assert seq.shape == (2, 10) and seq.dtype == torch.int64 and seq.device.type == "cpu"
    assert int(seq.min()) >= 0 and int(seq.max()) < 4981
