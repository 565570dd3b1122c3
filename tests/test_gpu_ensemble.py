"""Ensemble decoding on the GPU (csrc/ensemble.hip, ac_trm_step_logits, ac_trm_beam_update_all, EnsembleModel): the pick
kernels against float64, the never-retiring bookkeeping against a restatement of ensemble.py:222-251, ``decode()`` against
the reference's recorded outputs (tests/golden/g16_ensemble.npz) and, from waveforms, against tests/_ensemble_ref.py.

The gate throughout is the project's fp32 parity gate: identical token ids, values within 1e-4.
Captions are compared up to and including each row's first <end>: the reference keeps writing words after it, the product
writes <end> (audiocaption_amd/ensemble.py).

Measured on an MI355X (worst deviations are in tests/golden/REPORT_ensemble.txt)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _ensemble_ref as E
import _sampling_ref as S
from test_ensemble_oracle import assert_prefix_equal, load_members, sample_planes

from audiocaption_amd import _lib
from audiocaption_amd import sampling as SM

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
END, PAD, START = 2, 0, 1
GATE = 1e-4


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g16():
    return dict(np.load(os.path.join(GOLDEN, "g16_ensemble.npz")))


def _planes_arg(planes):
    """(device tensors [rows][ld] per member) -> the ABI's host array of device pointers."""
    return (ctypes.c_void_p * len(planes))(*[p.data_ptr() for p in planes])


def _upload(logits, ld):
    """logits (M, rows, V) numpy -> M device planes of leading dimension ld (columns beyond V hold garbage on purpose)."""
    M, R, V = logits.shape
    out = []
    for n in range(M):
        t = torch.full((R, ld), 1e30, device=DEV, dtype=torch.float32)   # a kernel that read past V would pick these
        t[:, :V] = torch.from_numpy(logits[n]).to(DEV)
        out.append(t)
    return out


def _mean64(logits):
    """m = mean_n log_softmax(logit_n) in float64: (rows, V)."""
    x = logits.astype(np.float64)
    mx = x.max(-1, keepdims=True)
    lp = x - mx - np.log(np.exp(x - mx).sum(-1, keepdims=True))
    return lp.mean(0)


def _seeded_logits(M, R, V, seed, min_gap=1e-3):
    """Seeded member logits whose mean has a decisive top-1 / top-2 gap of at least ``min_gap`` on every row, with one
    peaked member on row 0 and, from three rows on, exact ties at the top of rows 1 and 2 (identical columns in every member)."""
    g = np.random.default_rng(seed)
    x = g.normal(0.0, 2.0, (M, R, V)).astype(np.float32)
    x[M - 1, 0, 77] += 60.0                       # one member all but certain of word 77
    for _ in range(50):
        m = _mean64(x)
        top = np.sort(m, -1)[:, -2:]
        bad = np.flatnonzero(top[:, 1] - top[:, 0] < min_gap)
        if bad.size == 0:
            break
        x[:, bad, m[bad].argmax(-1)] += np.float32(0.05)
    else:
        raise AssertionError("could not open the top-1 / top-2 gap")
    ties = {}
    if R >= 3:
        for r, (a, b) in ((1, (40, 3000)), (2, (V - 1, 5))):
            m = _mean64(x)
            x[:, r, a] = x[:, r, m[r].argmax()]       # two columns equal to the winner's, member by member; the winner's
            x[:, r, b] = x[:, r, a]                   # own index may be lower than both
            ties[r] = min(a, b, int(m[r].argmax()))
    return x, ties


def _greedy_pick(lib, planes, ld, R, V, t=0, L=4, unfinished=None, cnt=None):
    seq = torch.full((R, L), END, device=DEV, dtype=torch.int64)
    lp = torch.zeros(R, L, device=DEV)
    tok = torch.full((R, L + 1), END, device=DEV, dtype=torch.int32)
    mask = torch.zeros(R, L + 1, device=DEV, dtype=torch.uint8)
    unf = torch.ones(R, device=DEV, dtype=torch.int32) if unfinished is None else unfinished
    cnt = torch.zeros(L, device=DEV, dtype=torch.int32) if cnt is None else cnt
    rc = lib.ac_ens_greedy_pick(_planes_arg(planes), len(planes), ld, R, V, t, L, END, PAD, _lib.ptr(seq), _lib.ptr(lp),
                                _lib.ptr(tok), _lib.ptr(mask), _lib.ptr(unf), _lib.ptr(cnt), _lib.stream())
    torch.cuda.synchronize()
    return rc, seq.cpu().numpy(), lp.cpu().numpy(), tok.cpu().numpy(), mask.cpu().numpy(), unf.cpu().numpy(), cnt.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# pick kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4368, 4981, 9000])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("R", [1, 64, 192])
def test_greedy_pick_vs_float64(lib, M, V, R):
    x, ties = _seeded_logits(M, R, V, seed=1000 * M + R + V)
    m = _mean64(x)
    want = m.argmax(-1)
    for r, first in ties.items():
        want[r] = first
    worst = 0.0
    for ld in (V, (V + 3) // 4 * 4 + 8):          # the scalar path (odd rows are not 16-byte aligned) and the 16-byte one
        rc, seq, lp, tok, mask, unf, cnt = _greedy_pick(lib, _upload(x, ld), ld, R, V)
        assert rc == 0
        np.testing.assert_array_equal(seq[:, 0], want)
        worst = max(worst, float(np.abs(lp[:, 0] - m[np.arange(R), want]).max()))
        np.testing.assert_array_equal(tok[:, 1], want)
        np.testing.assert_array_equal(unf, (want != END).astype(np.int32))
        assert cnt[0] == int((want != END).sum())
        np.testing.assert_array_equal(mask[:, 1], (want == PAD).astype(np.uint8))   # a picked pad word is masked as a key
    print(f"greedy pick M={M} V={V} R={R}: max |m[word] - float64| {worst:.3e}")
    assert worst < GATE
    assert want[0] == 77                       # the peaked member decides row 0


def test_greedy_pick_bookkeeping_and_limits(lib):
    V, R, M = 4981, 6, 3
    x, _ = _seeded_logits(M, R, V, seed=5)
    x[:, 3, END] += 40.0                           # row 3 picks <end>
    x[:, 4, PAD] += 40.0                           # row 4 picks the pad word: masked as a key from the next step on
    ld = 4984
    planes = _upload(x, ld)
    unf = torch.tensor([1, 0, 1, 1, 1, 1], device=DEV, dtype=torch.int32)   # row 1 finished earlier
    cnt = torch.tensor([5, 0, 0, 0], device=DEV, dtype=torch.int32)
    rc, seq, lp, tok, mask, unf, cnt = _greedy_pick(lib, planes, ld, R, V, t=1, unfinished=unf, cnt=cnt)
    assert rc == 0
    want = _mean64(x).argmax(-1)
    assert seq[1, 1] == END and lp[1, 1] == 0.0 and tok[1, 2] == END        # a finished row emits <end>, stores nothing
    assert seq[3, 1] == END and unf[3] == 0 and abs(lp[3, 1] - _mean64(x)[3, END]) < GATE
    assert seq[4, 1] == PAD and mask[4, 2] == 1 and unf[4] == 1
    np.testing.assert_array_equal(seq[[0, 2, 5], 1], want[[0, 2, 5]])
    assert cnt[1] == 4                                                        # rows 0, 2, 4, 5
    # the search is over once no row was left unfinished: nothing is written
    rc, seq, lp, tok, *_ = _greedy_pick(lib, planes, ld, R, V, t=2, cnt=torch.zeros(4, device=DEV, dtype=torch.int32))
    assert rc == 0 and (seq == END).all() and (lp == 0).all()
    # more members than AC_ENS_MAX, a vocabulary beyond the registers, a leading dimension below V
    nine = _upload(np.zeros((9, 1, 64), np.float32), 64)
    assert _greedy_pick(lib, nine, 64, 1, 64)[0] == _lib.AC_ERR_ARG
    assert _greedy_pick(lib, nine[:8], 64, 1, 64)[0] == 0
    assert _greedy_pick(lib, nine[:2], 64, 1, 16385)[0] == _lib.AC_ERR_ARG
    assert _greedy_pick(lib, nine[:2], 32, 1, 64)[0] == _lib.AC_ERR_ARG
    sd = torch.zeros(1, device=DEV, dtype=torch.int64)
    w = torch.zeros(1, device=DEV, dtype=torch.int32)
    lpw = torch.zeros(1, device=DEV)
    assert lib.ac_ens_sample_pick(_planes_arg(nine), 9, 64, 1, 64, SM.PLAIN, 0, 0.0, 1.0, _lib.ptr(sd), 0, 4, END, PAD, None,
                                  _lib.ptr(lpw), None, None, None, None, _lib.ptr(w), _lib.stream()) == _lib.AC_ERR_ARG
    tv, ti = torch.zeros(1, 3, device=DEV), torch.zeros(1, 3, device=DEV, dtype=torch.int32)
    assert lib.ac_ens_beam_step_select(_planes_arg(nine), 9, 64, 1, 3, 64, 0, 1.0, _lib.ptr(lpw), _lib.ptr(tv), _lib.ptr(ti),
                                       _lib.ptr(torch.zeros(64, device=DEV)), _lib.stream()) == _lib.AC_ERR_ARG


def test_greedy_pick_strided_vocabulary(lib):
    """Beyond 8192 words (64 values per thread), up to the sampler's limit."""
    for V in (12000, 16384):
        x, ties = _seeded_logits(3, 5, V, seed=V)
        m = _mean64(x)
        want = m.argmax(-1)
        for r, first in ties.items():
            want[r] = first
        rc, seq, lp, *_ = _greedy_pick(lib, _upload(x, V), V, 5, V)
        assert rc == 0
        np.testing.assert_array_equal(seq[:, 0], want)
        assert float(np.abs(lp[:, 0] - m[np.arange(5), want]).max()) < GATE


# ---------------------------------------------------------------------------------------------------------------------
# beam select and the never-retiring bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [3, 4, 8])
@pytest.mark.parametrize("temp", [1.0, 0.7])
def test_beam_select_vs_float64(lib, beam, temp):
    M, B, V = 3, 5, 4981
    R = B * beam
    g = np.random.default_rng(100 + beam)
    x = g.normal(0.0, 2.0, (M, R, V)).astype(np.float32)
    cum = g.normal(-3.0, 1.0, R).astype(np.float32)
    cum[1::beam] -= 1000.0                          # a finished beam's row (the -1000 of ensemble.py:251)
    z = _mean64(x) / temp
    zx = z.max(-1, keepdims=True)
    score = z - zx - np.log(np.exp(z - zx).sum(-1, keepdims=True)) + cum.astype(np.float64)[:, None]
    ld = 4984
    planes = _upload(x, ld)
    d_cum = torch.from_numpy(cum).to(DEV)
    worst = 0.0
    for t in (0, 3):
        tv = torch.zeros(B, beam, device=DEV)
        ti = torch.zeros(B, beam, device=DEV, dtype=torch.int32)
        scratch = torch.zeros(2 * R * beam, device=DEV)
        rc = lib.ac_ens_beam_step_select(_planes_arg(planes), M, ld, B, beam, V, t, temp, _lib.ptr(d_cum),
                                         _lib.ptr(tv), _lib.ptr(ti), _lib.ptr(scratch), _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0
        for c in range(B):
            flat = score[c * beam:(c + 1) * beam].reshape(-1) if t > 0 else score[c * beam]
            order = np.argsort(-flat, kind="stable")[:beam + 1]
            assert float(np.min(flat[order[:-1]] - flat[order[1:]])) > GATE, "test input: candidate margin too small"
            np.testing.assert_array_equal(ti[c].cpu().numpy(), order[:beam])
            worst = max(worst, float(np.abs(tv[c].cpu().numpy() - flat[order[:beam]]).max()))
    print(f"beam select beam={beam} temp={temp}: max |score - float64| {worst:.3e}")
    assert worst < GATE


def _update_restatement(top_val, top_idx, seqs, cum, done, t, beam, V, L):
    """ensemble.py:229-251 for one clip: seqs (list of token lists), cum (beam,), done (list of (seq, score))."""
    prev = [int(i) // V for i in top_idx]
    word = [int(i) % V for i in top_idx]
    seqs = [[word[k]] if t == 0 else seqs[prev[k]] + [word[k]] for k in range(beam)]
    cum = [float(v) for v in top_val]
    for k in range(beam):
        if word[k] == END or t == L - 1:
            done.append((list(seqs[k]), cum[k] / (t + 1)))
            cum[k] -= 1000.0
    return seqs, cum, prev


def test_beam_update_never_retires(lib):
    """ac_trm_beam_update_all over a whole search with synthetic selections: many beams end (more than `beam` finished
    beams per clip, the -1000 path), the clip stays active, and everything ends at the last step."""
    B, beam, V, L = 3, 3, 50, 6
    R, ld, cap = B * beam, L + 1, beam * L
    g = np.random.default_rng(7)
    i32 = dict(device=DEV, dtype=torch.int32)
    tok = [torch.full((R, ld), END, **i32) for _ in range(2)]
    tok[0][:, 0] = START
    mask = torch.zeros(R, ld, device=DEV, dtype=torch.uint8)
    cum = torch.zeros(R, device=DEV)
    active, done_cnt = torch.ones(B, **i32), torch.zeros(B, **i32)
    done_seq, done_score = torch.zeros(B, cap, L, **i32), torch.zeros(B, cap, device=DEV)
    src_row, n_active = torch.zeros(R, **i32), torch.full((1,), B, **i32)
    ref = [{"seqs": None, "cum": [0.0] * beam, "done": []} for _ in range(B)]
    for t in range(L):
        words = g.integers(3, V, (B, beam))
        words[g.random((B, beam)) < 0.45] = END            # nearly half of the kept candidates end
        parents = g.integers(0, beam, (B, beam)) if t > 0 else np.zeros((B, beam), np.int64)
        top_idx = (parents * V + words).astype(np.int32)
        top_val = np.sort(g.normal(-2.0 * (t + 1), 1.0, (B, beam)).astype(np.float32))[:, ::-1].copy()
        d_val, d_idx = torch.from_numpy(top_val).to(DEV), torch.from_numpy(top_idx).to(DEV)   # kept alive over the launch
        rc = lib.ac_trm_beam_update_all(_lib.ptr(d_val), _lib.ptr(d_idx),
                                        _lib.ptr(tok[t & 1]), _lib.ptr(tok[(t + 1) & 1]), _lib.ptr(mask), _lib.ptr(cum),
                                        _lib.ptr(active), _lib.ptr(done_cnt), _lib.ptr(done_seq), _lib.ptr(done_score),
                                        _lib.ptr(src_row), _lib.ptr(n_active), B, beam, V, L, t, END, PAD, cap, _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0
        got_tok, got_cum, got_src = tok[(t + 1) & 1].cpu().numpy(), cum.cpu().numpy(), src_row.cpu().numpy()
        for c in range(B):
            r = ref[c]
            r["seqs"], r["cum"], prev = _update_restatement(top_val[c], top_idx[c], r["seqs"], r["cum"], r["done"], t, beam, V, L)
            for k in range(beam):
                assert got_tok[c * beam + k, 1:t + 2].tolist() == r["seqs"][k]
                assert got_tok[c * beam + k, 0] == START
                assert got_src[c * beam + k] == c * beam + prev[k]
            np.testing.assert_allclose(got_cum[c * beam:(c + 1) * beam], r["cum"], rtol=0, atol=1e-4)
        assert active.cpu().tolist() == [1] * B and int(n_active.item()) == B
    counts = done_cnt.cpu().numpy()
    assert counts.max() > beam                              # a retiring search would have stopped these clips
    for c in range(B):
        assert counts[c] == len(ref[c]["done"]) <= cap
        for j, (s, sc) in enumerate(ref[c]["done"]):
            assert done_seq[c, j].cpu().tolist() == s + [END] * (L - len(s))
            assert abs(float(done_score[c, j]) - sc) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# decode() against the reference's recorded outputs
# ---------------------------------------------------------------------------------------------------------------------
def _gpu_member(state):
    import audiocaption_amd as A
    dec = A.TransformerDecoder(emb_dim=256, vocab_size=4981, fc_emb_dim=512, attn_emb_dim=512, dropout=0.2)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items()}, strict=True)
    return A.TransformerModel(nn.Identity(), dec).eval().to(DEV)


@pytest.fixture(scope="module")
def g16_ensemble(lib, g16):
    from audiocaption_amd.ensemble import EnsembleModel
    out = {}
    for short in (False, True):
        members = load_members(g16, short)
        models = {}
        for mb in members:
            if mb["draw"] not in models:
                models[mb["draw"]] = _gpu_member(mb["state"])
        encs = [{"attn_emb": mb["attn_emb"].to(DEV), "attn_emb_len": mb["attn_emb_len"]} for mb in members]
        out[short] = (EnsembleModel([models[mb["draw"]] for mb in members]), encs, members)
    return out


@pytest.mark.parametrize("short", [False, True])
def test_decode_greedy_vs_reference(g16_ensemble, g16, short):
    ens, encs, _ = g16_ensemble[short]
    key = "short_greedy" if short else "greedy"
    for use in range(3):                                     # eager, capture, replay
        out = ens.decode(encs, sample_method="greedy", max_length=20)
        assert out["seq"].dtype == torch.int64 and out["seq"].device.type == "cpu" and tuple(out["seq"].shape) == (4, 20)
        np.testing.assert_array_equal(out["seq"].numpy(), g16[key + "_seq"])   # <end> after the first <end>, as the fixture's
        d = float(np.abs(out["sampled_logprob"].numpy() - g16[key + "_value"]).max())
        print(f"decode {key} use {use}: max |sampled_logprob - reference m[word]| {d:.3e}")
        assert d < GATE
    assert out["encoder_outputs"] is not None and len(out["encoder_outputs"]) == len(encs)


@pytest.mark.parametrize("k", [3, 4])
def test_decode_beam_vs_reference(g16_ensemble, g16, k):
    ens, encs, _ = g16_ensemble[False]
    for use in range(3):
        out = ens.decode(encs, sample_method="beam", beam_size=k, max_length=20)
        np.testing.assert_array_equal(out["seq"].numpy(), g16[f"beam{k}_seq"])
        assert not out["sampled_logprob"].any() and tuple(out["sampled_logprob"].shape) == (4, 20)
    nb = ens.decode(encs, sample_method="beam", beam_size=k, max_length=20, n_best=True, n_best_size=k)
    assert tuple(nb["seq"].shape) == (4, k, 20)
    np.testing.assert_array_equal(nb["seq"].numpy(), g16[f"beam{k}_nbest"])
    d = float(np.abs(nb["score"].numpy() - g16[f"beam{k}_nbest_score"]).max())
    print(f"decode beam {k}: max |n-best score - reference| {d:.3e}")
    assert d < GATE
    # the recorded clips on which a retiring search would answer otherwise are answered as the reference answers them
    assert len(g16[f"beam{k}_retiring_differs"]) > 0


def test_decode_beam_short_memory_member(g16_ensemble, g16):
    ens, encs, _ = g16_ensemble[True]
    assert encs[int(g16["short_member"])]["attn_emb"].shape[1] == int(g16["short_tm"]) != encs[0]["attn_emb"].shape[1]
    out = ens.decode(encs, sample_method="beam", beam_size=3, max_length=20)
    np.testing.assert_array_equal(out["seq"].numpy(), g16["short_beam3_seq"])


# ---------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------
def _sample_pick(lib, planes, ld, R, V, code, k, p, temp, seed, step):
    word = torch.empty(R, device=DEV, dtype=torch.int32)
    lp = torch.empty(R, device=DEV)
    sd = torch.tensor([SM.seed_word(seed)], device=DEV, dtype=torch.int64)
    rc = lib.ac_ens_sample_pick(_planes_arg(planes), len(planes), ld, R, V, code, k, float(p), float(temp), _lib.ptr(sd), step,
                                1, END, PAD, None, _lib.ptr(lp), None, None, None, None, _lib.ptr(word), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return word.cpu().numpy(), lp.cpu().numpy()


def test_sample_pick_vs_reference_distributions(lib, g16):
    """Every rule's kept distribution as the reference handed it to Categorical: the kernel's draw is the inverse CDF over
    it at the Philox uniform of (seed, step, row), and the value it stores is the reference's for that word.  A draw
    forced onto the reference's own recorded word (a seed whose uniform falls inside that word's CDF interval) returns the
    recorded word and value."""
    x = sample_planes(g16)
    M, R, V = x.shape
    ld = 4984
    planes = _upload(x, ld)
    m64 = _mean64(x)
    worst = 0.0
    for mi, method in enumerate(g16["sample_methods"].tolist()):
        for ti, temp in enumerate(g16["sample_temps"].tolist()):
            code, k, p, _ = SM.parse_sample_method(method, V, temp)
            dist = g16["sample_dist"][mi, ti].astype(np.float64)
            w = np.exp(dist - dist.max(-1, keepdims=True))           # exp(-inf) = 0 outside the kept set
            stored = m64 if method == "gumbel" else dist            # ensemble.py:425 gathers m, :446 the kept logits
            cases = [(seed, step) for seed in (0, 1, 0xfedcba9876543210) for step in (0, 7)]
            forced = {}
            for r in range(R):                                       # a seed that forces the recorded word on row r
                cdf = np.cumsum(w[r]) / w[r].sum()
                rec = int(g16["sample_word"][mi, ti, r])
                lo, hi = (cdf[rec - 1] if rec else 0.0), cdf[rec]
                for seed in range(100, 20000):
                    u = float(S.uniform(seed, 3, [r])[0])
                    if lo + 0.05 * (hi - lo) < u < hi - 0.05 * (hi - lo):
                        forced[r] = seed
                        break
                assert r in forced, f"{method}: no seed below 20000 forces word {rec}"
                cases.append((forced[r], 3))
            for seed, step in cases:
                got_w, got_lp = _sample_pick(lib, planes, ld, R, V, code, k, p, temp, seed, step)
                us = S.uniform(seed, step, np.arange(R))
                for r in range(R):
                    want, ok = S.draw(w[r], us[r], 1e-5)
                    assert int(got_w[r]) in ok, f"{method} temp {temp} seed {seed} step {step} row {r}: {got_w[r]} vs {want}"
                    d = abs(float(got_lp[r]) - float(stored[r, int(got_w[r])]))
                    worst = max(worst, d)
                    assert d < GATE, f"{method} temp {temp} row {r}: stored {got_lp[r]} vs {stored[r, int(got_w[r])]}"
                    if step == 3 and forced.get(r) == seed:
                        assert int(got_w[r]) == int(g16["sample_word"][mi, ti, r])
                        assert abs(float(got_lp[r]) - float(g16["sample_value"][mi, ti, r])) < GATE
    print(f"sample pick: max |stored value - reference| {worst:.3e}")


def test_sampled_decode_is_reproducible(g16_ensemble):
    ens, encs, _ = g16_ensemble[False]
    big = [{"attn_emb": e["attn_emb"].repeat(4, 1, 1), "attn_emb_len": torch.as_tensor(e["attn_emb_len"]).repeat(4)} for e in encs]
    for method, temp in (("sample", 1.3), ("top20", 1.0), ("top0.9", 0.8), ("gumbel", 1.0)):
        a = ens.decode(big, sample_method=method, temp=temp, max_length=20, seed=1234)
        b = ens.decode(big, sample_method=method, temp=temp, max_length=20, seed=1234)
        c = ens.decode(big, sample_method=method, temp=temp, max_length=20, seed=99)
        assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["sampled_logprob"], b["sampled_logprob"]), method
        assert not torch.equal(a["seq"], c["seq"]), method
        for row, lp in zip(a["seq"].tolist(), a["sampled_logprob"].tolist()):   # <end> and 0 after the first <end>
            n = E.first_end(row)
            assert all(t == END for t in row[n:]) and all(v == 0 for v in lp[n:])


# ---------------------------------------------------------------------------------------------------------------------
# consistency
# ---------------------------------------------------------------------------------------------------------------------
def test_one_member_twice_and_permuted(g16_ensemble, g16):
    from audiocaption_amd.ensemble import EnsembleModel
    ens, encs, members = g16_ensemble[False]
    m0, e0 = ens.models[0], encs[0]
    own = m0.forward_decoder({"mode": "inference", "sample_method": "greedy", "max_length": 20},
                             {"attn_emb": e0["attn_emb"], "attn_emb_len": e0["attn_emb_len"]})
    one = EnsembleModel([m0]).decode([e0], sample_method="greedy", max_length=20)
    np.testing.assert_array_equal(one["seq"].numpy(), own["seq"].numpy())
    for i, row in enumerate(own["seq"].tolist()):            # for one member m[word] is that log-softmax value
        n = E.first_end(row)
        assert float((one["sampled_logprob"][i, :n] - own["sampled_logprob"][i, :n]).abs().max()) < GATE
    twice = EnsembleModel([m0, m0]).decode([e0, e0], sample_method="greedy", max_length=20)
    np.testing.assert_array_equal(twice["seq"].numpy(), one["seq"].numpy())
    # members in another order: the same mean up to rounding, the same ids (the fixture's gaps are >= 4e-3)
    swapped = EnsembleModel(list(ens.models)[::-1]).decode(encs[::-1], sample_method="greedy", max_length=20)
    np.testing.assert_array_equal(swapped["seq"].numpy(), g16["greedy_seq"])
    swapped_b = EnsembleModel(list(ens.models)[::-1]).decode(encs[::-1], sample_method="beam", beam_size=3, max_length=20)
    np.testing.assert_array_equal(swapped_b["seq"].numpy(), g16["beam3_seq"])


def test_old_entry_points_are_untouched_by_an_ensemble_call(diverse_models, g16_ensemble, golden_dir):
    """One g4b case through the existing entry points before and after ensemble calls on the same decoder: identical
    outputs (the workspaces are the ensemble's own, the parametrised sampler passes the old rules at the old call sites)."""
    from audiocaption_amd.ensemble import EnsembleModel
    g4 = dict(np.load(os.path.join(golden_dir, "g4_greedy.npz")))
    gb = dict(np.load(os.path.join(golden_dir, "g4b_greedy.npz")))
    model = diverse_models["greedy"]
    enc = {"attn_emb": torch.from_numpy(g4["attn_emb"]).cuda(), "attn_emb_len": torch.from_numpy(g4["attn_emb_len"])}

    def old_path():
        g = model.forward_decoder({"mode": "inference", "sample_method": "greedy", "max_length": 20}, enc)
        s = model.forward_decoder({"mode": "inference", "sample_method": "top0.9", "max_length": 20, "seed": 5}, enc)
        b = model.forward_decoder({"mode": "inference", "sample_method": "beam", "beam_size": 3, "max_length": 20}, enc)
        return [g["seq"], g["sampled_logprob"], s["seq"], s["sampled_logprob"], b["seq"]]

    before = old_path()
    np.testing.assert_array_equal(before[0].numpy(), gb["seq"])
    ens = EnsembleModel([model, model])
    for method in ("greedy", "top0.9", "beam"):
        ens.decode([enc, enc], sample_method=method, max_length=20, seed=5)
    after = old_path()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# wav to tokens: two different captioners as one ensemble
# ---------------------------------------------------------------------------------------------------------------------
def test_wav_to_tokens_two_architectures(lib):
    """A CrnnEncoder captioner and a Cnn14TransformerEncoder captioner decode the reference's ragged smoke batch together;
    checked against tests/_ensemble_ref.py over the oracle's encoders.  A clip whose CPU margins fall under the 1e-4 gate
    is named and left out (at most one of the four) - decided from the restatement alone, before the GPU result is read."""
    import audiocaption_amd as A
    from audiocaption_amd import config as C
    from audiocaption_amd import procedural as P
    from audiocaption_amd.ensemble import EnsembleModel
    from oracle import cpu_path as O
    V = 4981
    wav_len = [320000, 280000, 160000, 300000]
    wav = P.synthetic_wav(4, 320000, varied=True)
    for i, n in enumerate(wav_len):
        wav[i, n:] = 0.0
    wav = torch.from_numpy(wav)
    # Decoder draws that do not answer <end> at step 0 on these encoders: the high-entropy "beam" draw of procedural.DIVERSE
    # (for the second member at its own memory width, 256) with half its <end> row.  On the CPU this gives four captions of
    # 20 words, greedy gaps >= 4.9e-3 and beam-3 margins >= 4.6e-4.
    c = P.DIVERSE["beam"]

    def diverse(attn_emb_dim):
        d = P.decoder_state("decoder.", V, 256, attn_emb_dim, 2, 1024, seed=c["seed"])
        d["decoder.word_embedding.weight"] = d["decoder.word_embedding.weight"] * np.float32(c["emb_scale"])
        d["decoder.pos_encoder.pe"] = d["decoder.pos_encoder.pe"] * np.float32(c["pe_scale"])
        b3 = d["decoder.model.layers.1.norm3.bias"]
        cw = d["decoder.classifier.weight"].copy()
        cw[END] = ((0.5 * c["end_beta"] / float(np.dot(b3, b3))) * b3).astype(np.float32)
        d["decoder.classifier.weight"] = cw
        return P.to_torch(d)

    st_a = P.to_torch(P.cnn14rnn_trm_state(V))
    st_a.update(diverse(512))
    st_b = P.to_torch(P.cnn14trm_trm_state(V))
    st_b.update(diverse(256))
    models = []
    for cfg, st in ((A.cnn14rnn_trm_config(V), st_a), (C.cnn14trm_trm_config(V), st_b)):
        m = A.init_model_from_config(cfg, print_fn=lambda s: None)
        m.load_state_dict(st, strict=True)
        models.append(m.eval().to(DEV))
    ens = EnsembleModel(models)

    with torch.no_grad():
        cnn = O.cnn14_forward(st_a, wav, wav_len)                              # both members carry the same Cnn14 draw
        assert all(torch.equal(st_a[k], st_b[k]) for k in st_a if k.startswith("encoder.cnn."))
        enc_a = O.gru_forward(st_a, cnn["attn_emb"], cnn["attn_emb_len"])
        enc_b = O.transformer_encoder_forward(st_b, cnn["attn_emb"], cnn["attn_emb_len"], prefix="encoder.trm.")
        members = [{"state": st_a, "attn_emb": enc_a["attn_emb"], "attn_emb_len": enc_a["attn_emb_len"]},
                   {"state": st_b, "attn_emb": enc_b["attn_emb"], "attn_emb_len": enc_b["attn_emb_len"]}]
        want_g = E.greedy(members, 20)
        trace = []
        want_b = E.beam_search(members, 3, 20, trace=trace)
    thin_g = {i for i in range(4) if float(want_g["gap"][i].min()) < GATE}
    thin_b = {r["clip"] for r in trace if r["margin"] < GATE}
    for r in trace:
        if r["margin"] < GATE:
            print(f"beam 3: clip {r['clip']} step {r['t']} margin {r['margin']:.2e} under the gate: clip left out")
    for i in thin_g:
        t = int(want_g["gap"][i].argmin())
        print(f"greedy: clip {i} step {t} gap {float(want_g['gap'][i].min()):.2e} under the gate: clip left out")
    assert len(thin_g) <= 1 and len(thin_b) <= 1, "more than one clip under the gate: not a usable input"

    req = {"mode": "inference", "wav": wav.to(DEV), "wav_len": wav_len, "specaug": False, "max_length": 20}
    got_g = ens(dict(req, sample_method="greedy"))
    got_b = ens(dict(req, sample_method="beam", beam_size=3))
    assert len(got_g["encoder_outputs"]) == 2
    assert got_g["encoder_outputs"][1]["attn_emb"].shape[1] == got_g["encoder_outputs"][0]["attn_emb"].shape[1] + 1   # the cls frame
    print("greedy", got_g["seq"].tolist(), "\nbeam 3", got_b["seq"].tolist())
    for i in range(4):
        if i not in thin_g:
            assert got_g["seq"][i].tolist() == want_g["seq"][i].tolist(), f"greedy clip {i}"
        if i not in thin_b:
            assert got_b["seq"][i].tolist() == want_b["seq"][i].tolist(), f"beam 3 clip {i}"
