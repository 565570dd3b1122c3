"""The launch chain of the on-device search (csrc/decoder.hip trm_search) stops per SEGMENT - the rows of one batch inside a
shared chain - as the reference's loop stops per batch (base.py:167, :206-211): every kernel of a step skips the rows of
segments that have ended, and the columns of the steps a segment did not run read 0 / <end> / 0.

Inputs: the g4 encoder fixture decoded with the ``procedural.DIVERSE`` greedy draw, whose four clips emit <end> at
positions 3 / 10 / 19 / 10 (tests/golden/g4b_greedy.npz), so segments built from different clips stop at different steps."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAXLEN = 20
END = 2   # the <end> id of the fixtures (TransformerModel.end_idx)

# name -> the segments of one chain, each a list of g4 clip indices (equal lengths: forward_async groups equal shapes).
# Five rows or more per segment: the memory projection of ac_trm_memory (ac_linear over rows x 31 frames) takes its skinny
# kernel up to 128 rows and the tiled one beyond, which sum in different orders - a grouped chain and its segments alone
# can only agree to the bit when both sides are on the same one (5 x 31 = 155 rows: tiled).
CASES = {
    # 5 rows per segment: the one 16-row tile of every projection holds rows of all three segments
    "3x5_one_straddling_tile": [[0] * 5, [1, 3, 1, 3, 1], [2, 0, 1, 3, 0]],
    # 17 rows per segment: tile 0 lies in the segment that ends first, tile 1 straddles the boundary, tile 2 stays live
    "2x17_tile_boundary_inside": [[0] * 17, [2] + [0] * 16],
    # 16 rows per segment: every tile belongs to one segment
    "4x16_whole_tiles": [[0] * 16, [1] * 16, [2] * 16, [3] * 16],
    # clip 2 in both segments: nothing ends before max_length
    "2x5_none_dead": [[2, 0, 0, 1, 3], [1, 2, 3, 0, 0]],
}


def _end_pos():
    """Position of the first <end> of each g4 clip in the reference's greedy ids (MAXLEN: never)."""
    seq = np.load(os.path.join(GOLDEN, "g4b_greedy.npz"))["seq"]
    assert seq.shape == (4, MAXLEN)
    return [int(np.argmax(row == END)) if (row == END).any() else MAXLEN for row in seq]


def _want_cnt(rows, end_pos):
    """unfinished_cnt of a segment: rows still unfinished after step t."""
    return np.array([sum(end_pos[r] > t for r in rows) for t in range(MAXLEN)], dtype=np.int32)


def _ran(cnt):
    """Step t ran iff t == 0 or rows were unfinished after step t - 1."""
    ran = np.ones(len(cnt), dtype=bool)
    ran[1:] = cnt[:-1] > 0
    return ran


def test_cases_hold_live_and_dead_segments_at_every_step():
    """From the golden stop steps alone (no GPU): at every step each case has at least one live segment, and either no dead
    segment at all or at least one; the cases with dead segments have them from step 4 on; the straddling cases really put
    rows of a live and of a dead segment into one 16-row tile."""
    end_pos = _end_pos()
    assert end_pos == [3, 10, 19, 10]
    for name, segs in CASES.items():
        assert len({len(s_) for s_ in segs}) == 1, name
        ran = np.stack([_ran(_want_cnt(s_, end_pos)) for s_ in segs])   # [segment][step]
        live, dead = ran.sum(0), (~ran).sum(0)
        assert (live >= 1).all(), f"{name}: a step at which every segment is dead"
        if name.endswith("none_dead"):
            assert (dead == 0).all(), name
            continue
        assert (dead[:4] == 0).all() and (dead[4:] >= 1).all(), f"{name}: dead segments per step {dead}"
        n = len(segs[0])
        if n % 16:
            tiles = {(r // 16) for r in range(len(segs) * n)}
            mixed = [t for t in tiles
                     if len({bool(ran[min(r // n, len(segs) - 1), 5]) for r in range(16 * t, min(16 * t + 16, len(segs) * n))}) == 2]
            assert mixed, f"{name}: no tile with live and dead rows at step 5"


def _fixture():
    g4 = dict(np.load(os.path.join(GOLDEN, "g4_greedy.npz")))
    return torch.from_numpy(g4["attn_emb"]), torch.from_numpy(g4["attn_emb_len"])


def _args(model):
    assert model.end_idx == END
    return (MAXLEN, model.start_idx, model.end_idx, model.pad_idx)


def _sync(out):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check_not_run_columns(out, cnt, what):
    ran = torch.from_numpy(_ran(np.asarray(cnt)))
    assert torch.all(out["logit"][:, ~ran] == 0), f"{what}: logit of steps not run"
    assert torch.all(out["embed"][:, ~ran] == 0), f"{what}: embed of steps not run"
    assert torch.all(out["seq"][:, ~ran] == END), f"{what}: seq of steps not run"
    assert torch.all(out["sampled_logprob"][:, ~ran] == 0), f"{what}: log-probability of steps not run"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_grouped_chain_equals_single_segment_chains(diverse_models, case):
    """A chain of k segments equals the k single-segment chains bit for bit - ids, log-probabilities, counts, and the WHOLE
    logit and embed tensors - eager (first use), captured (second) and replayed (third); the counts and ids are the golden
    ones."""
    model = diverse_models["greedy"]
    dec = model.decoder
    attn, alen = _fixture()
    end_pos = _end_pos()
    gold = np.load(os.path.join(GOLDEN, "g4b_greedy.npz"))["seq"]
    segs = CASES[case]
    n = len(segs[0])
    parts = [attn[s_].cuda() for s_ in segs]
    lens = [alen[s_] for s_ in segs]
    singles = []
    for p_, l_ in zip(parts, lens):
        for _ in range(3):
            one = _sync(dec.greedy(p_, l_, *_args(model), mode="chain"))
        singles.append(one)
    for i, (s_, one) in enumerate(zip(segs, singles)):
        assert one["unfinished_cnt"].shape == (MAXLEN,)
        np.testing.assert_array_equal(one["unfinished_cnt"].numpy(), _want_cnt(s_, end_pos))
        np.testing.assert_array_equal(one["seq"].numpy(), gold[s_])
        _check_not_run_columns(one, one["unfinished_cnt"].numpy(), f"{case} single {i}")
    for it in ("eager", "captured", "replayed"):
        got = _sync(dec.greedy(parts, lens, *_args(model), mode="chain"))
        assert got["unfinished_cnt"].shape == (len(segs), MAXLEN)
        for i, one in enumerate(singles):
            rows = slice(i * n, (i + 1) * n)
            what = f"{case} {it} segment {i}"
            ran = _ran(one["unfinished_cnt"].numpy())
            d = float((got["logit"][rows][:, ran] - one["logit"][:, ran]).abs().max())
            print(f"{what}: {int(ran.sum())} steps ran, max|dlogit| over them {d:.2e}")
            assert torch.equal(got["unfinished_cnt"][i], one["unfinished_cnt"]), what
            assert torch.equal(got["seq"][rows], one["seq"]), what
            assert torch.equal(got["sampled_logprob"][rows], one["sampled_logprob"]), what
            assert torch.equal(got["logit"][rows], one["logit"]), what
            assert torch.equal(got["embed"][rows], one["embed"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("segments", [1, 2])
def test_steps_not_run_hold_no_stale_values(diverse_models, segments):
    """The same shape - the same static buffers and, from the second use on, the same captured graph - searched long
    (clip 2: all 20 steps), then short (clip 0: 4 steps), three times over: the short search's columns 4 .. 19 are exactly 0 /
    <end> / 0, not what the long one left there."""
    model = diverse_models["greedy"]
    dec = model.decoder
    attn, alen = _fixture()
    long_rows, short_rows = [2, 0, 1, 3, 0], [0] * 5
    end_pos = _end_pos()

    def run(rows_per_segment):
        parts = [attn[r_].cuda() for r_ in rows_per_segment]
        lens = [alen[r_] for r_ in rows_per_segment]
        if segments == 1:
            return _sync(dec.greedy(parts[0], lens[0], *_args(model), mode="chain"))
        return _sync(dec.greedy(parts, lens, *_args(model), mode="chain"))

    for rnd in range(3):
        out_long = run([long_rows] * segments)
        assert bool((out_long["logit"][:5, 4:] != 0).any(-1).all())   # the long search did fill the later columns
        out = run([short_rows] + [long_rows] * (segments - 1))   # segment 0 stops early (beside a long one when grouped)
        cnt = out["unfinished_cnt"].reshape(segments, MAXLEN)[0].numpy()
        np.testing.assert_array_equal(cnt, _want_cnt(short_rows, end_pos))
        first = {k: v[:5] for k, v in out.items() if k != "unfinished_cnt"}
        assert float(first["logit"][:, :4].abs().max()) > 0
        _check_not_run_columns(first, cnt, f"round {rnd}, {segments} segment(s)")


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["top1", "top0.9"])
def test_sampled_search_stops_with_its_segment(diverse_models, method):
    """ac_trm_sample is the same chain over one segment.  "top1" keeps one word, so it must reproduce the golden greedy ids
    and counts of clips that stop early; any method: counts consistent with the ids, steps not run 0 / <end> / 0 on buffers
    a 20-step search has just used, and the logits of the steps that ran equal to the bits of a teacher-forced replay of
    the drawn words through the same step kernels (ac_trm_forward_tokens, where every row is always live)."""
    from audiocaption_amd import sampling as SM
    model = diverse_models["greedy"]
    dec = model.decoder
    attn, alen = _fixture()
    end_pos = _end_pos()
    gold = np.load(os.path.join(GOLDEN, "g4b_greedy.npz"))["seq"]
    code, k, p, temp = SM.parse_sample_method(method, model.vocab_size, 1.0)
    for rnd in range(3):   # eager, captured, replayed - each after a search that ran every step on the same buffers
        for rows in ([2, 0, 1], [0, 3, 1]):
            a, l = attn[rows].cuda(), alen[rows]
            out = _sync(dec.sample(a, l, *_args(model), code, k, p, temp, 0x5eed0002))
            seq, cnt = out["seq"], out["unfinished_cnt"].numpy()
            assert cnt.shape == (MAXLEN,)
            unfinished = np.cumprod((seq.numpy() != END), axis=1)   # a finished row emits <end> from then on
            np.testing.assert_array_equal(cnt, unfinished.sum(0))
            if method == "top1":
                np.testing.assert_array_equal(seq.numpy(), gold[rows])
                np.testing.assert_array_equal(cnt, _want_cnt(rows, end_pos))
            ran = _ran(cnt)
            print(f"{method} round {rnd} rows {rows}: {int(ran.sum())} steps ran")
            _check_not_run_columns(out, cnt, f"{method} rows {rows}")
            word = torch.cat([torch.full((len(rows), 1), model.start_idx, dtype=torch.int64), seq[:, :-1]], 1)
            ref = dec({"word": word, "attn_emb": a, "attn_emb_len": l, "cap_padding_mask": word == model.pad_idx})
            torch.cuda.synchronize()
            d = float((ref["logit"].cpu()[:, ran] - out["logit"][:, ran]).abs().max())
            print(f"  max|logit - teacher-forced replay| over the steps run {d:.2e}")
            assert torch.equal(ref["logit"].cpu()[:, ran], out["logit"][:, ran])
            assert torch.equal(ref["embed"].cpu()[:, ran], out["embed"][:, ran])
