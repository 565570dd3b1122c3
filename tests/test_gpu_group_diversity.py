"""GPU tests of diversity WITHIN groups (``Diversity.score_groups`` / ``compute_group_score``, csrc/diversity.hip
``ac_diversity_group_scores``) against the grouped CPU reference (tests/_group_diversity_ref.py: the pooled float64
restatement applied inside each group, which knows nothing of the device's one table).

Every integer (``stats``, ``sent_distinct``, ``group_totals``) must equal the reference's; every float64 (``self_bleu``,
``mbleu``, ``group_mean``, ``summary``) must lie within 1e-12 + 1e-9 |reference| of it, the gate of the pooled scorer
(tests/test_gpu_diversity.py): a score is at most four logarithms, two exponentials and a few divisions in float64 on
exact integers, a mean sums at most a few hundred of them."""
import functools
import os

import numpy as np
import pytest
import torch

import _diversity_ref as D
import _group_diversity_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INTS = ("stats", "sent_distinct", "group_totals")
FLOATS = ("self_bleu", "mbleu", "group_mean", "summary")


def gate(want):
    return 1e-12 + 1e-9 * np.abs(want)


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


def _score(scorer, case, off, words=None, device=DEV):
    words = torch.from_numpy(case["words"] if words is None else words).to(device)
    return scorer.score_groups(case["vocabulary"], case["vocab_size"], words, D.START, D.END, group_off=off)


def _bits(a, b, keys=INTS + FLOATS):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)     # bits, NaN included


def _check(out, want, name):
    """Shapes, types, integers exactly, floats at the gate; prints the worst float."""
    N, Gn = len(want["self_bleu"]), len(want["group_mean"])
    assert {k: tuple(out[k].shape) for k in out} == {"self_bleu": (N,), "mbleu": (N, 4), "stats": (N, 10), "sent_distinct": (N, 4),
                                                      "group_totals": (Gn, 5), "group_mean": (Gn, 5), "summary": (5,)}
    assert all(out[k].is_cuda and out[k].dtype == torch.int32 for k in INTS)
    assert all(out[k].is_cuda and out[k].dtype == torch.float64 for k in FLOATS)
    for k in INTS:
        got = out[k].cpu().numpy()
        assert np.array_equal(got, want[k]), (name, k, np.argwhere(got != want[k])[:5].tolist())
    assert torch.equal(out["mbleu"][:, 3], out["self_bleu"])
    worst = {}
    for k in FLOATS:
        got, ref = out[k].cpu().numpy(), want[k]
        assert not np.isnan(got).any() and not np.isnan(ref).any(), (name, k)
        worst[k] = float((np.abs(got - ref) / gate(ref)).max())
    print(f"[{name}] N {N} G {Gn}: max |got - float64| / gate " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (name, worst)


def _case_of(sentences, T, V=12, names=None):
    """Word-id sentences as a case of tests/_diversity_ref.py: rows of T columns, <end> after the words unless they fill it."""
    rng = np.random.default_rng(T)
    return D._case(V, [D._row(list(s), T, rng, V) for s in sentences], names)


@functools.lru_cache(maxsize=None)
def _one_group_want(name):
    sentences = D.make_case(name)["sentences"]
    return G.group_results(sentences, [0, len(sentences)])


# ---- G = 1: the pooled call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.CASES)
def test_one_group_is_the_pooled_call(lib, name):
    from audiocaption_amd.diversity import Diversity
    case = D.make_case(name)
    N = len(case["sentences"])
    scorer = Diversity()
    out = _score(scorer, case, [0, N])
    _check(out, _one_group_want(name), name)
    pooled = scorer.score_ids(case["vocabulary"], case["vocab_size"], torch.from_numpy(case["words"]).to(DEV), D.START, D.END)
    assert _bits(out, pooled, ("stats", "sent_distinct"))
    # per sentence the same closed formula on the same integers; the mean sums the same rows in the same order
    assert _bits(out, pooled, ("self_bleu",))
    assert torch.equal(out["group_totals"][0], pooled["totals"])
    assert torch.equal(out["group_mean"][0, 4].view(torch.int64), pooled["summary"][0].view(torch.int64))
    assert torch.equal(out["summary"].view(torch.int64), out["group_mean"][0].view(torch.int64))
    # the (1, N, T) form is the same call
    three = scorer.score_groups(case["vocabulary"], case["vocab_size"], torch.from_numpy(case["words"]).to(DEV)[None], D.START,
                                D.END)
    assert _bits(three, out)


# ---- the same words in two groups: one table, two slots ----------------------------------------------------------------------
def test_the_same_sentences_in_two_groups_do_not_see_each_other(lib):
    from audiocaption_amd.diversity import Diversity
    a, b, c, d, e, f = range(D.FIRST_WORD, D.FIRST_WORD + 6)
    first = [[a, b, c], [a, b, c, d], [a, e, f], [d]]
    third = [[a, b, e, e], [f, a, b], [c, c, a, b, a, b]]        # shares the bigram "a b" (and its words) with the others only
    sentences = first + first + third
    off = [0, 4, 8, 11]
    case = _case_of(sentences, 7)
    scorer = Diversity()
    out = _score(scorer, case, off)
    _check(out, G.group_results(case["sentences"], off), "two equal groups")
    for g, (lo, hi) in enumerate(zip(off[:-1], off[1:])):         # every group as if scored alone
        alone = _score(scorer, case, [0, hi - lo], words=case["words"][lo:hi])
        for k in ("stats", "sent_distinct", "self_bleu", "mbleu"):
            assert torch.equal(out[k][lo:hi].view(torch.int32), alone[k].view(torch.int32)), (g, k)
        assert torch.equal(out["group_totals"][g], alone["group_totals"][0])
        assert torch.equal(out["group_mean"][g].view(torch.int64), alone["group_mean"][0].view(torch.int64))
    assert torch.equal(out["stats"][:4], out["stats"][4:8]) and torch.equal(out["group_totals"][0], out["group_totals"][1])
    # pooled, the copies match each other completely: every n-gram of the first eight sentences is found (num == its count)
    pooled = scorer.score_ids(case["vocabulary"], case["vocab_size"], torch.from_numpy(case["words"]).to(DEV), D.START, D.END)
    L = pooled["stats"][:8, :1]
    assert torch.equal(pooled["stats"][:8, 6:], (L - torch.arange(4, device=DEV)).clamp(min=0).to(torch.int32))
    assert int(out["stats"][:8, 6].sum()) < int(pooled["stats"][:8, 6].sum())


# ---- group sizes -------------------------------------------------------------------------------------------------------------
def test_ragged_groups_identical_captions_and_short_sentences(lib):
    from audiocaption_amd.diversity import Diversity
    rng = np.random.default_rng(253)
    w = lambda n: rng.integers(D.FIRST_WORD, 12, n).tolist()      # noqa: E731
    same = w(6)
    sentences = [[], [5]] + [w(int(n)) for n in rng.integers(0, 10, 5)] + [same, same, same]      # sizes 2, 5, 3
    off = [0, 2, 7, 10]
    case = _case_of(sentences, 9)
    out = _score(Diversity(), case, off)
    want = G.group_results(case["sentences"], off)
    _check(out, want, "ragged")
    # identical captions: every n-gram of a sentence is matched by the others
    assert out["self_bleu"][7:].tolist() == [1.0] * 3 and out["mbleu"][7:].tolist() == [[1.0] * 4] * 3
    assert out["group_mean"][2].tolist() == [1.0] * 5 and out["group_totals"][2].tolist() == [18] + want["group_totals"][2, 1:].tolist()
    assert out["group_totals"][2, 1].item() == len(set(same))
    # the empty sentence and the one-word sentence: nothing in common, lengths 0 and 1 are each other's reference length
    assert out["stats"][0].tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0, 0] and out["stats"][1].tolist() == [1, 0, 1, 1, 1, 1, 0, 0, 0, 0]
    assert out["self_bleu"][:2].tolist() == [0.0, 0.0] and out["group_totals"][0].tolist() == [1, 1, 0, 0, 0]
    # the explicit offsets of equal groups are the (B, S, T) form
    eq = D.random_case(12, 8, 10, 12)
    scorer = Diversity()
    by_off = _score(scorer, eq, [0, 3, 6, 9, 12])
    by_shape = scorer.score_groups(eq["vocabulary"], eq["vocab_size"], torch.from_numpy(eq["words"]).to(DEV).view(4, 3, -1),
                                   D.START, D.END)
    assert _bits(by_off, by_shape)
    _check(by_off, G.group_results(eq["sentences"], [0, 3, 6, 9, 12]), "four groups of three")
    host = scorer.score_groups(eq["vocabulary"], eq["vocab_size"], torch.from_numpy(eq["words"]).view(4, 3, -1), D.START, D.END)
    assert host["summary"].is_cuda and _bits(host, by_off)


def test_random_ids_collide_in_nine_groups(lib):
    """Captions of 0 to 20 words over 12 words, T = 21 (no multiple of a wave or of the workgroup): the 41 sentences repeat
    each other's n-grams within and ACROSS the groups of 2 to 7 rows."""
    from audiocaption_amd.diversity import Diversity
    sizes = [2, 7, 3, 5, 2, 6, 4, 3, 9]
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    case = D.random_case(sum(sizes), 20, 12, 2041, T=21)
    out = _score(Diversity(), case, off)
    _check(out, G.group_results(case["sentences"], off), "random")
    assert int(out["stats"][:, 7].sum()) > 0 and int(out["stats"][:, 8].sum()) > 0      # bigrams and trigrams do repeat in a group


# ---- bad input, repeatability ----------------------------------------------------------------------------------------------------
def test_bad_word_id_is_nan_and_calls_repeat_bitwise(lib):
    from audiocaption_amd import _lib
    from audiocaption_amd.diversity import Diversity
    case = D.make_case("edge")
    off = [0, 4, 9]
    scorer = Diversity()
    good = _score(scorer, case, off)
    _check(good, G.group_results(case["sentences"], off), "edge in two groups")
    assert _bits(_score(scorer, case, off), good) and _bits(_score(Diversity(), case, off), good)
    for bad in (case["vocab_size"], -1, 1 << 30):
        words = case["words"].copy()
        words[7, 2] = bad                                          # before the row's <end>: never an index
        out = _score(scorer, case, off, words=words)
        assert all(bool((out[k] == -1).all()) for k in INTS) and all(bool(torch.isnan(out[k]).all()) for k in FLOATS)
        late = case["words"].copy()
        late[6, 9] = bad                                           # after the row's <end>: not part of the sentence
        assert _bits(_score(scorer, case, off, words=late), good)
    assert _bits(_score(scorer, case, off), good)                  # the next call on clean input is right again
    # the entry point itself with offsets the Python layer would have refused: checked on the device, nothing outside a
    # group is read, NaN / -1 come back
    rows = torch.from_numpy(case["words"]).to(DEV)
    N, T = rows.shape
    canon = scorer._canon(case["vocabulary"], case["vocab_size"], torch.device(DEV))      # ids 4 and 9 spell one word
    ws = torch.empty(lib.ac_diversity_group_workspace_bytes(N, T, 3), device=DEV, dtype=torch.uint8)
    P = _lib.ptr

    def call(offsets):
        o = {"stats": torch.full((N, 10), -7, device=DEV, dtype=torch.int32), "sent_distinct": torch.full((N, 4), -7, device=DEV, dtype=torch.int32),
             "self_bleu": torch.full((N,), -7.0, device=DEV, dtype=torch.float64), "mbleu": torch.full((N, 4), -7.0, device=DEV, dtype=torch.float64),
             "group_totals": torch.full((3, 5), -7, device=DEV, dtype=torch.int32), "group_mean": torch.full((3, 5), -7.0, device=DEV, dtype=torch.float64),
             "summary": torch.full((5,), -7.0, device=DEV, dtype=torch.float64)}
        go = torch.tensor(offsets, device=DEV, dtype=torch.int32)
        _lib.check(lib.ac_diversity_group_scores(P(rows), rows.stride(0), N, T, D.START, D.END, P(canon), case["vocab_size"], P(go), 3,
                                                 P(ws), ws.numel(), P(o["stats"]), P(o["sent_distinct"]), P(o["self_bleu"]), P(o["mbleu"]),
                                                 P(o["group_totals"]), P(o["group_mean"]), P(o["summary"]), _lib.stream()),
                   "ac_diversity_group_scores")
        torch.cuda.synchronize()
        return o
    for offsets in ([0, 4, 3, 9], [0, 4, 12, 9], [1, 4, 6, 9], [0, 4, 6, 8], [-3, 4, 6, 9], [0, 4, 1 << 30, 9]):
        o = call(offsets)
        assert all(bool((o[k] == -1).all()) for k in INTS) and all(bool(torch.isnan(o[k]).all()) for k in FLOATS), offsets
    one = call([0, 4, 5, 9])                                       # a group of one row: NaN / -1 for it alone (and the summary)
    want = G.group_results(case["sentences"][:4] + case["sentences"][5:], [0, 4, 8])
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    assert np.array_equal(one["stats"].cpu().numpy()[keep], want["stats"]) and one["stats"][4].tolist() == [-1] * 10
    assert np.array_equal(one["group_totals"].cpu().numpy()[[0, 2]], want["group_totals"]) and one["group_totals"][1].tolist() == [-1] * 5
    assert bool(torch.isnan(one["self_bleu"][4])) and bool(torch.isnan(one["mbleu"][4]).all()) and bool(torch.isnan(one["group_mean"][1]).all())
    assert np.all(np.abs(one["self_bleu"].cpu().numpy()[keep] - want["self_bleu"]) <= gate(want["self_bleu"]))
    assert bool(torch.isnan(one["summary"]).all())


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_sampled_captions_of_three_clips_end_to_end(lib, diverse_models):
    """``n_samples=4`` on three clips, the device ``seq_dev`` straight into ``score_groups``: the numbers must be those of
    ``compute_group_score`` on the decoded strings (another numbering of the words, the same integers, the same formulas)
    and of the CPU reference."""
    from audiocaption_amd import Diversity
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g4_greedy.npz"))
    emb, lens = torch.from_numpy(g["attn_emb"])[:3].contiguous(), torch.from_numpy(g["attn_emb_len"])[:3]
    model = diverse_models["greedy"]
    with torch.no_grad():
        out = model.forward_decoder({"mode": "inference", "sample_method": "sample", "temp": 0.5, "max_length": 12,
                                     "seed": 0x5eed0040, "n_samples": 4, "_seq_on_device": True},
                                    {"attn_emb": emb.to(DEV), "attn_emb_len": lens})
    seq_dev = out["seq_dev"]
    assert seq_dev.is_cuda and tuple(seq_dev.shape) == (3, 4, 12) and torch.equal(seq_dev.cpu(), out["seq"])
    V = 4981
    vocabulary = D.ListVocabulary(D.word_list(V))
    scorer = Diversity()
    got = scorer.score_groups(vocabulary, V, seq_dev, D.START, D.END)
    strings = {f"clip{b}": [D.row_sentence(r, vocabulary.idx2word) for r in clip] for b, clip in enumerate(out["seq"].numpy())}
    numbers = scorer.compute_group_score(strings)
    print("sampled", strings, "\n", {k: v for k, v in numbers.items() if k != "per_key"})
    assert sum(len(s.split()) for c in strings.values() for s in c) >= 12
    assert [numbers[k] for k in ("mbleu_1", "mbleu_2", "mbleu_3", "mbleu_4", "self_bleu")] == got["summary"].tolist()
    totals = got["group_totals"].cpu().tolist()
    for b, (key, per) in enumerate(numbers["per_key"].items()):
        assert [per[k] for k in ("mbleu_1", "mbleu_2", "mbleu_3", "mbleu_4", "self_bleu")] == got["group_mean"][b].tolist()
        assert per["div_1"] == totals[b][1] / totals[b][0] and per["div_2"] == totals[b][2] / totals[b][0]
    assert numbers["div_1"] == sum(numbers["per_key"][k]["div_1"] for k in strings) / 3
    sentences = [s.split() for c in strings.values() for s in c]
    _check(got, G.group_results(sentences, [0, 4, 8, 12]), "sampled")
    ref = G.group_numbers(strings)
    assert all(abs(numbers[k] - ref[k]) <= gate(ref[k]) for k in ref if k != "per_key")
