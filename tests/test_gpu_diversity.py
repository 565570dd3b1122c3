"""GPU tests of the built-in diversity scorer (audiocaption_amd/diversity.py, csrc/diversity.hip) against the float64
restatement (tests/_diversity_ref.py), which scores every sentence against all the others directly and knows nothing of
the device's table: the closed-form corpora through both routes, an edge batch with one row per branch, a crowded table, a
table at its minimum size, sentences up to the limit of 1024 words, pooling, repeatability, the NaN of a bad word id, and
one sampled batch of the product model end to end.

Every integer (``stats``, ``sent_distinct``, ``totals``) must equal the restatement's; every float must lie within
1e-12 + 1e-9 |reference| of it, the gate of tests/test_gpu_caption_metrics.py: a score is four logarithms, two
exponentials and a few divisions in float64 on exact integers, each within an ulp or two of 1.1e-16 relative; a richness
term sums at most 1024 logarithms below 20 and a mean at most a few hundred values, N * 1.1e-16 relative."""
import numpy as np
import pytest
import torch

import _diversity_ref as D
from _metrics_ref import close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INTS = ("stats", "sent_distinct", "totals")
FLOATS = ("self_bleu", "summary")


def gate(want):
    return 1e-12 + 1e-9 * np.abs(want)


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


def _score(scorer, case, device=DEV, words=None):
    words = case["words"] if words is None else words
    words = [torch.from_numpy(w).to(device) for w in words] if isinstance(words, list) else torch.from_numpy(words).to(device)
    return scorer.score_ids(case["vocabulary"], case["vocab_size"], words, D.START, D.END)


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in INTS + FLOATS)     # bits, NaN included


def _check(out, want, name):
    """Shapes, types, integers exactly, floats at the gate; prints the worst float."""
    N = len(want["self_bleu"])
    assert {k: tuple(out[k].shape) for k in out} == {"self_bleu": (N,), "stats": (N, 10), "sent_distinct": (N, 4),
                                                      "totals": (5,), "summary": (6,)}
    assert all(out[k].is_cuda and out[k].dtype == torch.int32 for k in INTS)
    assert all(out[k].is_cuda and out[k].dtype == torch.float64 for k in FLOATS)
    for k in INTS:
        got = out[k].cpu().numpy()
        assert np.array_equal(got, want[k]), (name, k, np.argwhere(got != want[k])[:5].tolist())
    worst = {}
    for k in FLOATS:
        got, ref = out[k].cpu().numpy(), want[k]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (name, k, got, ref)
        ok = ~np.isnan(ref)
        worst[k] = float((np.abs(got[ok] - ref[ok]) / gate(ref[ok])).max())
    print(f"[{name}] N {N}: max |got - float64| / gate " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (name, worst)


@pytest.mark.parametrize("name", list(D.CLOSED))
def test_closed_forms_through_both_routes(lib, name):
    from audiocaption_amd.diversity import Diversity
    case, want = D.make_case(name), D.want(name)
    sentences, answers = D.CLOSED[name]
    scorer = Diversity()
    out = _score(scorer, case)
    _check(out, want, name)
    for g, w in zip(out["self_bleu"].cpu().tolist(), answers):
        assert close(g, w), (name, g, w)
    strings = scorer._score_strings(sentences)
    assert _same(strings, out), "string and id routes differ"
    numbers = scorer.compute_score({"clip": sentences[:2], "other": sentences[2:]}, train_captions=[sentences[0], "snow"],
                                   instance=name != "captions")
    ref = D.corpus_numbers([s.split() for s in sentences])
    assert numbers.pop("novel") == (len(sentences) - 1) / len(sentences)
    assert set(numbers) == set(ref) and all(type(v) in (int, float) for v in numbers.values())
    assert numbers["vocabulary"] == ref["vocabulary"] and numbers["distinct_1"] == ref["distinct_1"]
    assert numbers["distinct_2"] == ref["distinct_2"]
    assert numbers["self_bleu"] == float(out["summary"][0]) and numbers["richness"] == float(out["summary"][5])
    for k in ("distinct_1_instance", "distinct_2_instance"):
        assert k not in ref or abs(numbers[k] - ref[k]) < 1e-15
    if name == "captions":
        assert close(numbers["self_bleu"], D.CLOSED_CAPTIONS["mean"]) and close(numbers["richness"], D.CLOSED_CAPTIONS["overall"])
        assert out["totals"].tolist()[:3] == D.CLOSED_CAPTIONS["totals"] and float(out["self_bleu"][3]) == 0.0
        with pytest.raises(ValueError, match="rain"):                   # the instance means: "rain" has no bigram
            scorer.compute_score(sentences)
        assert "novel" not in scorer.compute_score(sentences, instance=False)


@pytest.mark.parametrize("name", ["edge", "crowded", "minimum", "long"])
def test_corpora_vs_float64(lib, name):
    from audiocaption_amd.diversity import Diversity
    case, want = D.make_case(name), D.want(name)
    scorer = Diversity()
    out = _score(scorer, case)
    _check(out, want, name)
    # a second call, another scorer object, and words held on the host: the same bits
    assert _same(_score(scorer, case), out) and _same(_score(Diversity(), case), out)
    host = _score(Diversity(), case, device="cpu")
    assert host["self_bleu"].is_cuda and _same(host, out)


def test_a_list_of_planes_is_one_corpus(lib):
    from audiocaption_amd.diversity import Diversity
    case = D.make_case("crowded")
    rows = case["words"]
    whole = _score(Diversity(), case)
    parts = _score(Diversity(), case, words=[rows[:100], rows[100:101], rows[101:]])
    assert _same(parts, whole)
    # planes of different lengths: the shorter rows end where they end
    edge = D.make_case("edge")
    short = np.ascontiguousarray(edge["words"][:3, :3])               # rows 0 .. 2 have their <end> within three columns
    mixed = _score(Diversity(), edge, words=[short, edge["words"][3:]])
    assert _same(mixed, _score(Diversity(), edge))
    # a view with a stride: the plane is read through its leading dimension
    wide = torch.from_numpy(np.concatenate((rows, rows[:, ::-1]), axis=1)).to(DEV)
    view = Diversity().score_ids(case["vocabulary"], case["vocab_size"], wide[:, :rows.shape[1]], D.START, D.END)
    assert _same(view, whole)


@pytest.mark.parametrize("bad", ["vocab_size", -1])
def test_bad_word_id_is_nan_for_the_whole_call(lib, bad):
    from audiocaption_amd.diversity import Diversity
    case = D.make_case("edge")
    scorer = Diversity()
    good = _score(scorer, case)
    words = case["words"].copy()
    words[7, 2] = case["vocab_size"] if bad == "vocab_size" else -1           # before the row's <end>: never an index
    out = _score(scorer, case, words=words)
    assert all(bool((out[k] == -1).all()) for k in INTS) and all(bool(torch.isnan(out[k]).all()) for k in FLOATS)
    late = case["words"].copy()
    late[6, 9] = case["vocab_size"] + 5 if bad == "vocab_size" else -1        # after the row's <end>: not part of the sentence
    assert _same(_score(scorer, case, words=late), good)
    assert _same(_score(scorer, case), good)                                  # the next call on clean input is right again
    _check(good, D.want("edge"), "edge after a bad call")


def test_refusals_launch_nothing(lib):
    from audiocaption_amd import _lib
    from audiocaption_amd.cider import MAX_HYP_WORDS
    from audiocaption_amd.diversity import Diversity
    case = D.make_case("edge")
    rows = torch.from_numpy(case["words"]).to(DEV)
    scorer = Diversity()
    with pytest.raises(ValueError):
        scorer.score_ids(case["vocabulary"], case["vocab_size"], rows[:1], D.START, D.END)
    with pytest.raises(ValueError):
        scorer.score_ids(case["vocabulary"], case["vocab_size"], torch.full((3, MAX_HYP_WORDS + 1), 5, device=DEV), D.START, D.END)
    # the entry point itself on real device buffers: a workspace one byte short, one sentence, a row one word too long
    N, T = rows.shape
    canon = torch.arange(case["vocab_size"], device=DEV, dtype=torch.int32)
    need = lib.ac_diversity_workspace_bytes(N, T)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    stats = torch.full((N, 10), -7, device=DEV, dtype=torch.int32)
    sent = torch.full((N, 4), -7, device=DEV, dtype=torch.int32)
    totals = torch.full((5,), -7, device=DEV, dtype=torch.int32)
    bleu = torch.full((N,), -7.0, device=DEV, dtype=torch.float64)
    summary = torch.full((6,), -7.0, device=DEV, dtype=torch.float64)
    P = _lib.ptr

    def call(ws_bytes=need, N_=N, T_=T):
        return lib.ac_diversity_scores(P(rows), max(T_, rows.stride(0)), N_, T_, D.START, D.END, P(canon), case["vocab_size"],
                                       P(ws), ws_bytes, P(stats), P(sent), P(totals), P(bleu), P(summary), _lib.stream())

    assert call(ws_bytes=need - 1) == _lib.AC_ERR_ARG and call(N_=1) == _lib.AC_ERR_ARG
    assert call(T_=MAX_HYP_WORDS + 1) == _lib.AC_ERR_ARG and call(T_=0) == _lib.AC_ERR_ARG
    torch.cuda.synchronize()
    assert all(int(t.max()) == -7 and int(t.min()) == -7 for t in (stats, sent, totals))      # nothing was launched
    assert float(bleu.max()) == -7.0 and float(summary.max()) == -7.0
    _lib.check(call(), "ac_diversity_scores")
    names = list(case["vocabulary"].idx2word)
    names[9] = "w9"                                                   # (canon was the identity in the call above)
    want = scorer.score_ids(D.ListVocabulary(names), case["vocab_size"], rows, D.START, D.END)
    assert _same({"stats": stats, "sent_distinct": sent, "totals": totals, "self_bleu": bleu, "summary": summary}, want)
    # sentences at the limit itself are served: 1024 times one word in both rows, every n-gram matched
    full = scorer.score_ids(case["vocabulary"], case["vocab_size"], torch.full((2, MAX_HYP_WORDS), 5, device=DEV), D.START, D.END)
    assert full["self_bleu"].tolist() == [1.0, 1.0] and full["totals"].tolist() == [2 * MAX_HYP_WORDS, 1, 1, 1, 1]
    assert full["summary"].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_sampled_batch_end_to_end(lib, hip_model):
    """Eight clips decoded twice by the product model with ``sample_method="sample"`` and two fixed seeds: the two ``seq``
    go through ``Diversity.score_ids`` as they come, pooled into one corpus of sixteen captions, and the result must
    equal the restatement on the same ids."""
    from audiocaption_amd import Diversity, procedural as Pr
    B, L = 8, 64000
    batch = {"mode": "inference", "wav": torch.from_numpy(Pr.synthetic_wav(B, L, seed=5)).to(DEV),
             "wav_len": [L, L - 20000, L // 2, L - 5000, L, L - 1000, L // 2, L - 7000], "specaug": False,
             "sample_method": "sample", "temp": 0.5, "max_length": 12}
    with torch.no_grad():
        seqs = [hip_model(dict(batch, seed=seed))["seq"] for seed in (0x5eed0025, 0x5eed0026)]
    V = 4981
    vocabulary = D.ListVocabulary(D.word_list(V))
    got = Diversity().score_ids(vocabulary, V, seqs, D.START, D.END)
    sentences = [D.row_sentence(r, vocabulary.idx2word).split() for seq in seqs for r in seq.cpu().numpy()]
    print("sampled", [" ".join(s) for s in sentences], "\nsummary", got["summary"].tolist(), got["totals"].tolist())
    assert len(sentences) == 2 * B and sum(len(s) for s in sentences) >= 2 * B          # there is something to score
    assert not torch.equal(seqs[0], seqs[1]) and int(got["stats"][:, 6].sum()) > 0      # two draws, and words in common
    _check(got, D.host_results(sentences), "sampled")
