"""GPU tests of the built-in CIDEr-D scorer (audiocaption_amd/cider.py, csrc/cider.hip) against the float64 restatement
(tests/_cider_ref.py): the edge batch and the random batches of tests/test_cider_cpu.py through the id route and the string
route, the refusals, and ScstWrapper with ``Cider()`` against the same iteration with the restatement on the host route.

The gate is the project's fp32 parity gate, 1e-4 absolute on scores in [0, 10]; measured maxima are printed and recorded
in tests/golden/REPORT_cider.txt."""
import ctypes

import numpy as np
import pytest
import torch

import _cider_ref as R
import _scst_ref as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE = 1e-4
V = 4981


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


def _case(name):
    return R.edge_case() if name == "edge" else R.random_case(*R.RANDOM_CASES[name])


def _score_ids(scorer, case, device=DEV):
    words = [torch.from_numpy(w).to(device) for w in case["words"]]
    return scorer.score_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"], words, R.START, R.END)


@pytest.mark.parametrize("name", ["edge"] + sorted(R.RANDOM_CASES))
def test_scores_and_reward_vs_float64(lib, name):
    from audiocaption_amd.cider import Cider
    case = _case(name)
    scorer = Cider()
    out = _score_ids(scorer, case)
    scores, reward = out["scores"], out["reward"]
    N = len(case["keys"])
    assert scores.is_cuda and reward.is_cuda and scores.dtype == reward.dtype == torch.float32
    assert tuple(scores.shape) == (2, N) and tuple(reward.shape) == (N,)
    got = scores.cpu().numpy().astype(np.float64)
    want = np.stack([R.host_scores(case, which)[0] for which in range(2)])
    err = np.abs(got - want).max()
    err_r = np.abs(reward.cpu().numpy().astype(np.float64) - (want[0] - want[1])).max()
    print(f"[{name}] max |score - float64| {err:.3e}, reward {err_r:.3e}; scores {want.min():.4f} .. {want.max():.4f}")
    assert not np.isnan(got).any()
    assert err <= GATE and err_r <= GATE
    assert got.min() >= 0.0 and got.max() <= 10.0
    assert np.array_equal(reward.cpu().numpy(), (scores[0] - scores[1]).cpu().numpy())
    # a second call (references now cached, the table claimed in another order): the same bits
    again = _score_ids(scorer, case)
    assert torch.equal(again["scores"], scores) and torch.equal(again["reward"], reward)
    # hypothesis words that live on the host are uploaded: the same bits again
    host = _score_ids(Cider(), case, device="cpu")
    assert host["scores"].is_cuda and torch.equal(host["scores"], scores)
    # the string route on the same sentences
    for which in range(2):
        _, references, hypothesis = R.host_scores(case, which)
        mean, per_key = Cider().compute_score(references, hypothesis)
        assert isinstance(mean, float) and per_key.dtype == np.float64 and per_key.shape == (len(references),)
        by_key = dict(zip(references.keys(), per_key))
        assert np.array_equal(np.array([by_key[k] for k in case["keys"]]), got[which]), "string and id routes differ"
        assert mean == float(per_key.mean())


def test_sentences_at_the_length_limit(lib):
    """Hypotheses of exactly MAX_HYP_WORDS words (every LDS array of cider_hyp_kernel full, the staging of the row
    included) and a reference of exactly MAX_REF_WORDS words, among ordinary keys."""
    from audiocaption_amd.cider import Cider, MAX_HYP_WORDS, MAX_REF_WORDS
    case = R.limit_case(MAX_HYP_WORDS, MAX_REF_WORDS)
    assert all(w.shape == (4, MAX_HYP_WORDS) for w in case["words"])
    assert [len(r.split()) for r in case["key2refs"]["full"]] == [MAX_REF_WORDS, 12]
    assert all(len(R.row_sentence(case["words"][s][row], case["vocabulary"].idx2word).split()) == MAX_HYP_WORDS
               for s, row in ((0, 0), (0, 1), (1, 1), (1, 2)))
    out = _score_ids(Cider(), case)
    got = out["scores"].cpu().numpy().astype(np.float64)
    want = np.stack([R.host_scores(case, which)[0] for which in range(2)])
    err = np.abs(got - want).max()
    err_r = np.abs(out["reward"].cpu().numpy().astype(np.float64) - (want[0] - want[1])).max()
    print(f"[limit] max |score - float64| {err:.3e}, reward {err_r:.3e}; scores {want.tolist()}")
    assert want[0, 1] > 1.0 and want[0, 2] > 1.0                 # worth comparing: the long pair and an ordinary one
    assert not np.isnan(got).any()
    assert err <= GATE and err_r <= GATE
    assert got.min() >= 0.0 and got.max() <= 10.0
    assert np.array_equal(got[:, 3], got[:, 1])                  # the second row of the key: the score of its first


def test_closed_form_answers_on_the_device(lib):
    from audiocaption_amd.cider import Cider
    refs = {"a": ["w1 w2 w3 w4 w5"], "b": ["w6 w7"], "c": ["w8 w9 w10 w11"]}
    _, s = Cider().compute_score(refs, {"a": ["w1 w2 w3 w4 w5"], "b": ["w6 w7"], "c": [""]})
    assert np.abs(s - [10.0, 5.0, 0.0]).max() <= 1e-5 and s.max() <= 10.0
    _, s = Cider().compute_score(refs, {"a": [""], "b": ["w6"], "c": [""]})
    assert abs(s[1] - 1.7433843) <= 1e-5 and s[0] == 0.0 and s[2] == 0.0
    mean, s = Cider().compute_score({"a": refs["a"]}, {"a": refs["a"]})
    assert s.tolist() == [0.0] and mean == 0.0


def test_single_set_and_other_orders(lib):
    """One hypothesis set gives no reward; n = 2 agrees with the restatement at n = 2."""
    from audiocaption_amd.cider import Cider
    case = _case("small")
    words = [torch.from_numpy(case["words"][0]).to(DEV)]
    out = Cider(n=2, sigma=3.0).score_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"], words,
                                          R.START, R.END)
    assert out["reward"] is None and tuple(out["scores"].shape) == (1, len(case["keys"]))
    _, references, hypothesis = R.host_scores(case, 0)
    _, want = R.compute_score(references, hypothesis, n=2, sigma=3.0)
    by_key = dict(zip(references.keys(), want))
    want = np.array([by_key[k] for k in case["keys"]])
    assert np.abs(out["scores"][0].cpu().numpy() - want).max() <= GATE


def test_refusals(lib):
    from audiocaption_amd import _lib
    from audiocaption_amd.cider import Cider, MAX_HYP_WORDS, MAX_REF_WORDS
    case = _case("edge")
    scorer = Cider()
    # a reference beyond the kernel's word limit, a hypothesis beyond the LDS budget
    long_refs = dict(case["key2refs"], d=[" ".join(["w5"] * (MAX_REF_WORDS + 1))])
    with pytest.raises(ValueError):
        scorer.score_ids(long_refs, case["vocabulary"], case["vocab_size"], case["keys"],
                         [torch.from_numpy(w).to(DEV) for w in case["words"]], R.START, R.END)
    with pytest.raises(ValueError):
        scorer.score_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"],
                         [torch.full((5, MAX_HYP_WORDS + 1), 5, device=DEV, dtype=torch.int32)] * 2, R.START, R.END)
    with pytest.raises(ValueError):       # four keys for five rows
        scorer.score_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"][:4],
                         [torch.from_numpy(w).to(DEV) for w in case["words"]], R.START, R.END)
    # a reference word id at vocab_size + the words outside the vocabulary
    batch, canon = scorer.pack_ids(case["key2refs"], case["vocabulary"], case["vocab_size"], case["keys"])
    canon_dev = torch.from_numpy(canon).to(DEV)
    words = [torch.from_numpy(w).to(DEV) for w in case["words"]]
    assert batch.n_words == case["vocab_size"] + 1
    batch.words = batch.words.copy()
    batch.words[3] = batch.n_words
    with pytest.raises(ValueError):
        scorer.score_packed(batch, words, R.START, R.END, canon_dev, case["vocab_size"])
    batch.words[3] = batch.n_words - 1        # the largest id that is one
    scores_ok, _ = scorer.score_packed(batch, words, R.START, R.END, canon_dev, case["vocab_size"])
    assert not torch.isnan(scores_ok).any()
    # a hypothesis word id at vocab_size: refused on the host when it can be seen there, NaN (never a read) on the device
    bad = case["words"][0].copy()
    bad[4, 2] = case["vocab_size"]
    with pytest.raises(ValueError):
        scorer.score_packed(batch, [torch.from_numpy(bad), words[1]], R.START, R.END, canon_dev, case["vocab_size"])
    scores, _ = scorer.score_packed(batch, [torch.from_numpy(bad).to(DEV), words[1]], R.START, R.END, canon_dev,
                                    case["vocab_size"])
    assert torch.isnan(scores[0, 4]) and not torch.isnan(scores[0, :4]).any() and not torch.isnan(scores[1]).any()
    # a workspace that is too small: the entry point itself, on real device buffers
    P = _lib.ptr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    b_words, b_sent, b_key, b_row, b_first = (dev(a) for a in (batch.words, batch.sent_off, batch.key_off, batch.row_key,
                                                               batch.first_row))
    W, M, K, N = b_words.numel(), b_sent.numel() - 1, b_first.numel(), b_row.numel()
    need = lib.ac_cider_workspace_bytes(W, M, K, 2)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    out_s, out_r = torch.full((2, N), -1.0, device=DEV), torch.full((N,), -1.0, device=DEV)
    hyp = (ctypes.c_void_p * 2)(words[0].data_ptr(), words[1].data_ptr())

    def call(ws_bytes):
        return lib.ac_cider_scores(ctypes.cast(hyp, ctypes.c_void_p), 2, words[0].stride(0), N, words[0].shape[1], R.START, R.END,
                                   P(canon_dev), case["vocab_size"], batch.n_words, P(b_words), W, P(b_sent), M,
                                   batch.max_ref_words, P(b_key), K, P(b_row), P(b_first), 4, 6.0, P(ws), ws_bytes, P(out_s),
                                   P(out_r), _lib.stream())

    with pytest.raises(_lib.HipLibraryError):
        _lib.check(call(need - 1), "ac_cider_scores")
    assert float(out_s.max()) == -1.0 and float(out_r.max()) == -1.0          # nothing was launched
    _lib.check(call(need), "ac_cider_scores")
    assert torch.equal(out_s, scores_ok)


# ---- ScstWrapper ---------------------------------------------------------------------------------------------------------
def _sentence_words(row):
    return [int(w) for w in R.row_sentence(row, _Ids()).split()]


class _Ids:
    def __getitem__(self, i):
        return str(int(i))


def _refs_from(sampled, greedy, keys, rng):
    """References of real length in the stub vocabulary's words, close enough to what the model emits that rewards are
    not zero: per key, the sampled and (more heavily) the greedy sentence of its first row with words replaced or dropped, and 1 - 3
    sentences of 5 - 15 random words; every key's first reference ends with the same word (df == keys)."""
    key2refs = {}
    for row, key in enumerate(keys):
        if key in key2refs:
            continue
        refs = []
        for sent, swap in ((_sentence_words(sampled[row]), 0.2), (_sentence_words(greedy[row]), 0.6)):
            kept = [int(rng.integers(4, V)) if rng.random() < swap else w for w in sent if rng.random() > 0.1]
            refs.append(kept + [5])
        for _ in range(int(rng.integers(1, 4))):
            refs.append(rng.integers(4, V, int(rng.integers(5, 16))).tolist())
        key2refs[key] = [" ".join(f"w{w}" for w in r) for r in refs]
    return key2refs


def test_wrapper_with_the_builtin_scorer_vs_the_host_route(lib, state4981):
    import audiocaption_amd as A
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.cider import Cider
    from audiocaption_amd.rl_model import scst_loss
    from audiocaption_amd.train import _TrainBridge
    from test_gpu_scst import _rnn_model
    model = _rnn_model(state4981)
    wrapper = A.ScstWrapper(model)
    params = [p for p in wrapper.parameters() if p.requires_grad]
    B, L, T, temp = 4, 96000, 8, 0.9
    keys = ["a", "b", "a", "c"]
    batch = {"mode": "train", "wav": torch.from_numpy(Pr.synthetic_wav(B, L, seed=5)).to(DEV),
             "wav_len": [L, L - 20000, L // 2, L - 5000], "specaug": False, "max_length": T, "temp": temp, "keys": keys,
             "vocabulary": SC.StubVocabulary(), "seed": 77, "dropout_seed": 1}
    # the words this iteration draws do not depend on the scorer: take them once to build references around them
    probe = wrapper(dict(batch, key2refs={k: ["w5"] for k in keys}, scorer=SC.ConstantScorer()))
    model._train_engine._saved = None
    batch["key2refs"] = _refs_from(probe["sampled_seqs"].numpy(), probe["greedy_seqs"].numpy(), keys,
                                   np.random.default_rng(9))
    assert max(len(r.split()) for refs in batch["key2refs"].values() for r in refs) <= 16

    def iteration(scorer):
        wrapper.zero_grad(set_to_none=True)
        out = wrapper(dict(batch, scorer=scorer))
        eng = model._train_engine
        lp = eng._saved["ws"].tensor("scst_logprob")[:B * T].view(B, T).cpu().double()
        out["loss"].backward()
        return out, lp, [p.grad.detach().clone() for p in params]

    a, lp_a, grad_a = iteration(R.Scorer())
    _, _, grad_a2 = iteration(R.Scorer())                       # the same iteration again: what the backward's atomics move
    b, lp_b, grad_b = iteration(Cider())
    assert model.training
    assert set(a) == set(b) == {"greedy_seqs", "sampled_seqs", "reward", "score", "loss"}
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].device == b[k].device and a[k].shape == b[k].shape, k
    assert all(not b[k].is_cuda for k in ("greedy_seqs", "sampled_seqs", "reward", "score")) and b["loss"].is_cuda
    assert torch.equal(a["sampled_seqs"], b["sampled_seqs"]) and torch.equal(a["greedy_seqs"], b["greedy_seqs"])
    assert torch.equal(a["sampled_seqs"], probe["sampled_seqs"]) and torch.equal(lp_a, lp_b)
    d_reward = float((a["reward"] - b["reward"]).abs().max())
    d_score = float((a["score"] - b["score"]).abs().max())
    print(f"reward {a['reward'].tolist()}, score {a['score'].tolist()}: max difference {d_reward:.3e} / {d_score:.3e}")
    assert float(a["reward"].abs().max()) > 0.01 and float(a["score"].max()) > 0.01        # worth comparing
    assert a["reward"][0] == a["reward"][2] and b["reward"][0] == b["reward"][2]            # the repeated key
    assert d_reward <= GATE and d_score <= GATE
    # loss = mean_n sum_t -(logprob * mask) * reward[n]: linear in the reward
    mask = SC.mask_of(a["sampled_seqs"]).double()
    per_clip = (lp_a * mask).abs().sum(1)
    scale = float((per_clip * a["reward"].abs()).mean())
    rounding = 2 * B * T * 2.0 ** -24 * scale         # two fp32 sums of B * T terms, each within (terms) ulps of its scale
    d_loss = abs(float(a["loss"]) - float(b["loss"]))
    print(f"loss {float(a['loss']):.6f} vs {float(b['loss']):.6f}: {d_loss:.3e}, bound "
          f"{d_reward * float(per_clip.mean()) + rounding:.3e}")
    assert d_loss <= d_reward * float(per_clip.mean()) + rounding
    # the gradient is linear in the reward as well: grad = sum_n reward[n] * G_n, G_n the gradient under reward e_n
    eng = model._train_engine
    unit = []
    for n in range(B):
        wrapper.zero_grad(set_to_none=True)
        ro = eng.rollout(dict(batch, max_length=T, temp=temp))
        assert torch.equal(ro["seq"].cpu(), a["sampled_seqs"])
        logit = _TrainBridge.apply(eng, ro["logit"], *eng.flat.params)
        e_n = torch.zeros(B)
        e_n[n] = 1.0
        scst_loss(logit, ro["seq_i32"], e_n, temp, model.end_idx).backward()
        unit.append([float(p.grad.abs().max()) for p in params])
    unit = np.asarray(unit)                                     # (clip, parameter) max |G_n|
    r_abs = a["reward"].abs().numpy()
    worst, worst_repeat = 0.0, 0.0
    for i, (ga, gb) in enumerate(zip(grad_a, grad_b)):
        own = float((unit[:, i] * r_abs).sum())                 # the scale of this gradient: sum_n |reward[n]| max |G_n|
        repeat = float((ga - grad_a2[i]).abs().max())           # same rewards, bit for bit: the order of atomic additions
        # Beside the reward term: twice the repeat-to-repeat difference measured above, and 32 ulps (2^-19) of the scale
        # for the rounding of two fp32 chains of ~1000 accumulations each on slightly different inputs (sqrt(1000) ulps)
        bound = d_reward * float(unit[:, i].sum()) + 2 * repeat + 2.0 ** -19 * own
        d = float((ga - gb).abs().max())
        worst, worst_repeat = max(worst, d / (own + 1e-30)), max(worst_repeat, repeat / (own + 1e-30))
        assert d <= bound, (i, d, bound, repeat, own)
    print(f"worst gradient difference relative to its scale: {worst:.3e} (repeat to repeat {worst_repeat:.3e}, reward term "
          f"{d_reward / (float(r_abs.max()) + 1e-30):.3e})")
