"""GPU tests of the built-in BLEU and ROUGE-L scorers (audiocaption_amd/caption_metrics.py, csrc/capmetrics.hip) against
the float64 restatement (tests/_metrics_ref.py): every batch through the id route and the string route and both hypothesis
sets, the closed forms, repeatability, the NaN of a bad word id, the refusals, and one decoded batch through
``eval_prediction`` with all three built-in scorers.

Every integer (``stats``, ``lcs``) must equal the restatement's; every float must lie within 1e-12 + 1e-9 |reference| of it:
the kernels evaluate a few dozen float64 operations (one pow, one exp, a few divisions) on exact integers, each within an
ulp or two of 1.1e-16 relative, and the one sum over keys adds K values below 1 with K * 1.1e-16 absolute.  Measured maxima
are printed and recorded in tests/golden/REPORT_metrics.txt."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _cider_ref as R
import _metrics_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gate(want):
    return 1e-12 + 1e-9 * np.abs(want)


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _case(name):
    return M.make_case(name)


@functools.lru_cache(maxsize=None)
def _want(name, which, n=4):
    return M.host_results(_case(name), which, n)


def _score_ids(scorer, case, device=DEV, which=(0, 1)):
    words = [torch.from_numpy(case["words"][w]).to(device) for w in which]
    return scorer.score_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"], words, R.START, R.END)


def _worst(got, want):
    """max of |got - want| / gate(want): at most 1 passes."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and not np.isnan(got).any()
    return float((np.abs(got - want) / gate(want)).max()), float(np.abs(got - want).max())


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if k != "keys")


@pytest.mark.parametrize("name", M.CASES)
def test_batches_vs_float64(lib, name):
    from audiocaption_amd.caption_metrics import Bleu, Rouge
    case = _case(name)
    want = [_want(name, which) for which in range(2)]
    N, K, M_ = len(case["keys"]), len(want[0]["references"]), len(want[0]["lcs"])
    bleu, rouge = Bleu(4), Rouge()
    b, r = _score_ids(bleu, case), _score_ids(rouge, case)
    assert b["keys"] == r["keys"] == list(want[0]["references"])
    assert b["stats"].dtype == r["lcs"].dtype == torch.int32 and tuple(b["stats"].shape) == (2, K, 10)
    assert tuple(r["lcs"].shape) == (2, M_)
    assert all(t.is_cuda and t.dtype == torch.float64 for t in (b["scores"], b["corpus"], r["scores"], r["mean"]))
    assert tuple(b["scores"].shape) == (2, 4, N) and tuple(b["corpus"].shape) == (2, 4)
    assert tuple(r["scores"].shape) == (2, N) and tuple(r["mean"].shape) == (2,)
    worst = {}
    for which in range(2):
        w = want[which]
        assert np.array_equal(b["stats"][which].cpu().numpy(), w["stats"]), "BLEU stats differ"
        assert np.array_equal(r["lcs"][which].cpu().numpy(), w["lcs"]), "LCS lengths differ"
        for what, got, ref in (("bleu", b["scores"][which], w["bleu"]), ("corpus", b["corpus"][which], w["corpus"]),
                               ("rouge", r["scores"][which], w["rouge"]), ("mean", r["mean"][which], w["mean"])):
            rel, ab = _worst(got.cpu().numpy(), ref)
            worst[what] = max(worst.get(what, (0.0, 0.0)), (rel, ab))
    print(f"[{name}] N {N} K {K} sentences {M_}: max |got - float64| / gate (absolute) " +
          ", ".join(f"{k} {v[0]:.3e} ({v[1]:.3e})" for k, v in worst.items()))
    assert all(v[0] <= 1.0 for v in worst.values()), worst
    # a second call (references now cached) and hypothesis words that live on the host: the same bits
    assert _same(_score_ids(bleu, case), b) and _same(_score_ids(rouge, case), r)
    hb, hr = _score_ids(Bleu(4), case, device="cpu"), _score_ids(Rouge(), case, device="cpu")
    assert hb["scores"].is_cuda and hr["scores"].is_cuda and _same(hb, b) and _same(hr, r)
    # the string route on the same sentences: the same bits per key, totals over the same keys
    for which in range(2):
        w = want[which]
        rows = [case["keys"].index(k) for k in w["references"]]
        corpus, per_key = Bleu(4).compute_score(w["references"], w["hypothesis"])
        assert isinstance(corpus, list) and len(corpus) == 4 and all(isinstance(v, float) for v in corpus)
        assert len(per_key) == 4 and all(isinstance(p, list) and len(p) == K for p in per_key)
        assert np.array_equal(np.array(per_key), b["scores"][which].cpu().numpy()[:, rows]), "string and id routes differ"
        assert corpus == b["corpus"][which].cpu().tolist()
        mean, per_key = Rouge().compute_score(w["references"], w["hypothesis"])
        assert isinstance(mean, float) and per_key.dtype == np.float64 and per_key.shape == (K,)
        assert np.array_equal(per_key, r["scores"][which].cpu().numpy()[rows]) and mean == float(r["mean"][which])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_other_orders_and_a_single_set(lib, n):
    from audiocaption_amd.caption_metrics import Bleu
    for name in ("edge", "repeated-keys"):
        case = _case(name)
        w = _want(name, 1, n)
        out = _score_ids(Bleu(n), case, which=(1,))
        assert tuple(out["stats"].shape) == (1, len(w["references"]), 2 + 2 * n) and tuple(out["corpus"].shape) == (1, n)
        assert np.array_equal(out["stats"][0].cpu().numpy(), w["stats"])
        assert _worst(out["scores"][0].cpu().numpy(), w["bleu"])[0] <= 1.0
        assert _worst(out["corpus"][0].cpu().numpy(), w["corpus"])[0] <= 1.0
        # the lower orders do not depend on how many are asked for
        assert np.array_equal(out["stats"][0, :, :2 + n].cpu().numpy(), _want(name, 1)["stats"][:, :2 + n])


def test_closed_form_answers_on_the_device(lib):
    from audiocaption_amd.caption_metrics import Bleu, Rouge
    refs = {i: item[1] for i, item in enumerate(M.BLEU_CLOSED)}
    hyps = {i: [item[0]] for i, item in enumerate(M.BLEU_CLOSED)}
    corpus, per_key = Bleu(4).compute_score(refs, hyps)
    for i, (_, _, _, want) in enumerate(M.BLEU_CLOSED):
        for k, w in enumerate(want):
            assert w is None or M.close(per_key[k][i], w), (i, k, per_key[k][i], w)
    assert per_key[0][2] == per_key[3][2] == 0.0                         # the empty hypothesis: exactly 0
    assert all(M.close(g, w) for g, w in zip(corpus, M.BLEU_CLOSED_CORPUS[2])), corpus
    out = _score_ids(Bleu(4), _case("closed"))
    for i, (_, _, stats, _) in enumerate(M.BLEU_CLOSED):
        assert out["stats"][0, i].tolist() == [stats[0], stats[1]] + stats[2] + stats[3]
    refs = {i: item[1] for i, item in enumerate(M.ROUGE_CLOSED)}
    hyps = {i: [item[0]] for i, item in enumerate(M.ROUGE_CLOSED)}
    mean, per_key = Rouge().compute_score(refs, hyps)
    for i, (_, _, want) in enumerate(M.ROUGE_CLOSED):
        assert M.close(per_key[i], want), (i, per_key[i], want)
    assert per_key[3] == 0.0 and per_key[4] == 0.0 and M.close(mean, (0.628865979 + 0.75 + 0.5) / 5)


def test_bad_word_id_is_nan_for_its_key_alone(lib):
    from audiocaption_amd.caption_metrics import Bleu, Rouge
    case = _case("edge")
    V = case["vocab_size"]
    bad = case["words"][0].copy()
    bad[4, 2] = V                                    # key d, before its <end>: never read as an index
    late = case["words"][1].copy()
    late[0, 5] = V + 7                               # key a, after its <end>: not part of the sentence
    words = [torch.from_numpy(bad).to(DEV), torch.from_numpy(late).to(DEV)]
    for scorer in (Bleu(4), Rouge()):
        with pytest.raises(ValueError):              # on the host the id can be seen
            scorer.score_ids(case["key2refs"], case["vocabulary"], V, case["keys"], [torch.from_numpy(bad)], R.START, R.END)
        out = scorer.score_ids(case["key2refs"], case["vocabulary"], V, case["keys"], words, R.START, R.END)
        good = _score_ids(scorer, case)
        s, g = out["scores"], good["scores"]
        assert torch.isnan(s[0][..., 4]).all() and not torch.isnan(s[0][..., [0, 1, 2, 3, 5]]).any()
        assert torch.equal(s[0][..., [0, 1, 2, 3, 5]], g[0][..., [0, 1, 2, 3, 5]]) and torch.equal(s[1], g[1])
        total = out["corpus" if "corpus" in out else "mean"]
        assert torch.isnan(total[0]).all() and torch.equal(total[1], good["corpus" if "corpus" in good else "mean"][1])
        ints = out["stats" if "stats" in out else "lcs"]
        if "stats" in out:
            assert (ints[0, 3] == -1).all() and torch.equal(ints[0, [0, 1, 2, 4]], good["stats"][0, [0, 1, 2, 4]])
        else:
            assert (ints[0, 10:13] == -1).all() and torch.equal(ints[0, :10], good["lcs"][0, :10])
        assert torch.equal(ints[1], good["stats" if "stats" in good else "lcs"][1])


def test_refusals_launch_nothing(lib):
    from audiocaption_amd import _lib
    from audiocaption_amd.caption_metrics import Bleu, Rouge
    from audiocaption_amd.cider import MAX_HYP_WORDS, MAX_REF_WORDS, MAX_SETS
    case = _case("edge")
    V, keys = case["vocab_size"], case["keys"]
    words = [torch.from_numpy(w).to(DEV) for w in case["words"]]
    for scorer in (Bleu(4), Rouge()):
        args = (case["vocabulary"], V, keys)
        with pytest.raises(ValueError):       # a reference beyond the kernels' word limit
            scorer.score_ids(dict(case["key2refs"], d=[" ".join(["w5"] * (MAX_REF_WORDS + 1))]), *args, words, R.START, R.END)
        with pytest.raises(ValueError):       # hypotheses beyond the LDS budget
            scorer.score_ids(case["key2refs"], *args, [torch.full((6, MAX_HYP_WORDS + 1), 5, device=DEV, dtype=torch.int32)],
                             R.START, R.END)
        with pytest.raises(ValueError):       # more sets than the kernels take
            scorer.score_ids(case["key2refs"], *args, [words[0]] * (MAX_SETS + 1), R.START, R.END)
        with pytest.raises(ValueError):       # five keys for six rows
            scorer.score_ids(case["key2refs"], case["vocabulary"], V, keys[:5], words, R.START, R.END)
        with pytest.raises(ValueError):       # a reference without words
            scorer.score_ids(dict(case["key2refs"], d=["w5", ""]), *args, words, R.START, R.END)
        exact = dict(case["key2refs"], d=[" ".join(["w5"] * MAX_REF_WORDS)])       # the limits themselves are served
        out = scorer.score_ids(exact, *args, [torch.full((6, MAX_HYP_WORDS), 5, device=DEV, dtype=torch.int32)], R.START, R.END)
        assert not torch.isnan(out["scores"]).any()
        assert abs(float(out["scores"][0][..., 4].max()) - 1.0) < 1e-9          # key d: 1024 times w5 on both sides
    # the entry points themselves on real device buffers: a workspace one byte short, a hypothesis one word too long
    bleu = Bleu(4)
    batch, canon = bleu.pack_ids(case["key2refs"], case["vocabulary"], V, keys)
    P = _lib.ptr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    canon_dev = dev(canon)
    b_words, b_sent, b_key, b_row, b_first = (dev(a) for a in (batch.words, batch.sent_off, batch.key_off, batch.row_key,
                                                               batch.first_row))
    W, M_, K, N = b_words.numel(), b_sent.numel() - 1, b_first.numel(), b_row.numel()
    need = lib.ac_capmetrics_workspace_bytes(K, 2)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    hyp = (ctypes.c_void_p * 2)(words[0].data_ptr(), words[1].data_ptr())
    stats = torch.full((2, K, 10), -7, device=DEV, dtype=torch.int32)
    lcs = torch.full((2, M_), -7, device=DEV, dtype=torch.int32)
    scores = torch.full((2, 4, N), -7.0, device=DEV, dtype=torch.float64)
    total = torch.full((2, 4), -7.0, device=DEV, dtype=torch.float64)

    def call(fn, ints, ws_bytes, T=words[0].shape[1], order=()):
        return fn(ctypes.cast(hyp, ctypes.c_void_p), 2, max(T, words[0].stride(0)), N, T, R.START, R.END, P(canon_dev), V,
                  P(b_words), W, P(b_sent), M_, batch.max_ref_words, P(b_key), K, P(b_row), P(b_first), *order, P(ws), ws_bytes,
                  P(ints), P(scores), P(total), _lib.stream())

    for fn, ints, order in ((lib.ac_bleu_scores, stats, (4,)), (lib.ac_rouge_l_scores, lcs, ())):
        assert call(fn, ints, need - 1, order=order) == _lib.AC_ERR_ARG
        assert call(fn, ints, need, T=MAX_HYP_WORDS + 1, order=order) == _lib.AC_ERR_ARG
        torch.cuda.synchronize()
        assert int(ints.max()) == -7 and float(scores.max()) == -7.0 and float(total.max()) == -7.0     # nothing was launched
    _lib.check(call(lib.ac_bleu_scores, stats, need, order=(4,)), "ac_bleu_scores")
    assert torch.equal(stats, _score_ids(bleu, case)["stats"])
    _lib.check(call(lib.ac_rouge_l_scores, lcs, need), "ac_rouge_l_scores")
    assert torch.equal(lcs, _score_ids(Rouge(), case)["lcs"])


def test_decoded_batch_through_eval_prediction(lib, hip_model):
    """Four clips decoded by the product model, ids -> text through text.py, then ``eval_prediction`` with the three
    built-in scorers against the restatements on the same strings."""
    from audiocaption_amd import Cider, procedural as Pr
    from audiocaption_amd.caption_metrics import Bleu, Rouge, eval_prediction
    from audiocaption_amd.text import DictTokenizer
    tokenizer = DictTokenizer()
    for i in range(4, 4981):
        tokenizer.add_word(f"w{i}")
    B, L = 4, 96000
    with torch.no_grad():
        out = hip_model({"mode": "inference", "wav": torch.from_numpy(Pr.synthetic_wav(B, L, seed=5)).to(DEV),
                         "wav_len": [L, L - 20000, L // 2, L - 5000], "specaug": False, "sample_method": "greedy",
                         "max_length": 12})
    texts = tokenizer.decode(out["seq"].cpu().numpy())
    keys = [f"clip{i}" for i in range(B)]
    key2pred = {k: [t] for k, t in zip(keys, texts)}
    assert sum(len(t.split()) for t in texts) >= B, texts          # there is something to score
    # references around what was decoded: the caption with words dropped and replaced, twice, and a foreign sentence
    rng = np.random.default_rng(3)
    key2refs = {}
    for k, t in zip(reversed(keys), reversed(texts)):                    # (another order than the predictions')
        words = t.split() or ["w5"]
        refs = [[f"w{int(rng.integers(4, 4981))}" if rng.random() < swap else w for w in words if rng.random() > 0.15] + ["w5"]
                for swap in (0.2, 0.5)]
        key2refs[k] = [" ".join(r) for r in refs] + [" ".join(f"w{int(w)}" for w in rng.integers(4, 4981, 9))]
    got = eval_prediction(key2refs, key2pred, [Bleu(4), Rouge(), Cider()], per_audio=True)
    want = eval_prediction(key2refs, key2pred, [M.BleuScorer(4), M.RougeScorer(), R.Scorer()], per_audio=True)
    assert list(got) == list(want) == ["per_audio", "Bleu", "Rouge", "CIDEr"]
    assert isinstance(got["Bleu"], list) and len(got["Bleu"]) == 4 and isinstance(got["Rouge"], float)
    print("predictions", texts, "\nscores", {k: got[k] for k in ("Bleu", "Rouge", "CIDEr")})
    assert _worst(got["Bleu"], want["Bleu"])[0] <= 1.0 and _worst(got["Rouge"], want["Rouge"])[0] <= 1.0
    assert abs(got["CIDEr"] - want["CIDEr"]) <= 1e-4                 # (the fp32 gate of the CIDEr scorer's own tests)
    for name in ("Bleu", "Rouge", "CIDEr"):
        assert list(got["per_audio"][name]) == list(key2refs) == list(want["per_audio"][name])
        g = [got["per_audio"][name][k] for k in key2refs]
        w = [want["per_audio"][name][k] for k in key2refs]
        if name == "CIDEr":
            assert np.abs(np.array(g) - np.array(w)).max() <= 1e-4
        else:
            assert _worst(g, w)[0] <= 1.0
    assert got["Bleu"][0] > 0.1 and got["Rouge"] > 0.1                   # worth comparing
