"""audiocaption_amd/search_state.py on the host: the state cache and the eager side of the capture rule over dict states and
a stub launch, and the ranking of finished beams over hand-written ``done_*`` arrays."""
import pytest
import torch

from audiocaption_amd import search_state as S


def _builder(log, name):
    def build():
        log.append(name)
        return {"name": name, "graph": None}
    return build


def test_lookup_builds_once_per_key_and_counts_uses():
    states, log = {}, []
    a = S.lookup(states, "a", _builder(log, "a"), 3)
    assert a["uses"] == 1 and a["graph"] is None
    assert S.lookup(states, "a", _builder(log, "a"), 3) is a and a["uses"] == 2
    b = S.lookup(states, "b", _builder(log, "b"), 3)
    assert S.lookup(states, "a", _builder(log, "a"), 3) is a
    assert log == ["a", "b"] and (a["uses"], b["uses"]) == (3, 1)


def test_lookup_orders_by_recency_and_evicts_exactly_beyond_keep():
    states, log = {}, []
    for k in "abc":
        S.lookup(states, k, _builder(log, k), 3)
    assert list(states) == ["a", "b", "c"]           # keep = 3 entries: nothing leaves
    S.lookup(states, "a", _builder(log, "a"), 3)
    assert list(states) == ["b", "c", "a"]           # a hit moves to most recently used
    S.lookup(states, "d", _builder(log, "d"), 3)
    assert list(states) == ["c", "a", "d"]           # the fourth entry evicts the oldest, and only it
    b = S.lookup(states, "b", _builder(log, "b"), 3)
    assert list(states) == ["a", "d", "b"] and b["uses"] == 1 and log == ["a", "b", "c", "d", "b"]   # evicted: built afresh
    S.lookup(states, "e", _builder(log, "e"), 1)
    assert list(states) == ["e"]                     # a smaller keep drops every older entry


def test_lookup_build_that_raises_leaves_the_cache_unchanged():
    states, log = {}, []
    a = S.lookup(states, "a", _builder(log, "a"), 2)
    b = S.lookup(states, "b", _builder(log, "b"), 2)

    def build():
        raise RuntimeError("no buffers")
    with pytest.raises(RuntimeError, match="no buffers"):
        S.lookup(states, "c", build, 2)
    assert list(states) == ["a", "b"] and states["a"] is a and states["b"] is b and (a["uses"], b["uses"]) == (1, 1)


def test_run_is_eager_on_first_use_and_with_graphs_disabled(monkeypatch):
    states, calls = {}, []
    monkeypatch.delenv("AUDIOCAPTION_DECODE_GRAPH", raising=False)
    st = S.lookup(states, "k", lambda: {"graph": None}, 2)
    assert not S.captures(st)                        # first use: eager whatever the variable says
    S.run(st, "cpu", lambda: calls.append(1))
    assert calls == [1] and st["graph"] is None
    st = S.lookup(states, "k", lambda: {"graph": None}, 2)
    assert S.captures(st)                            # second use: a graph, unless disabled - read per call
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "0")
    assert not S.captures(st)
    for n in (2, 3):
        S.run(st, "cpu", lambda: calls.append(n))
    assert calls == [1, 2, 3] and st["graph"] is None and st["uses"] == 2


def _book(done_cnt, done_score, done_seq):
    return {"done_cnt": torch.tensor(done_cnt, dtype=torch.int32), "done_score": torch.tensor(done_score, dtype=torch.float32),
            "done_seq": torch.tensor(done_seq, dtype=torch.int32)}


END, L, CAP = 9, 3, 4


def _rows(*firsts):
    """Finished beams (CAP slots) told apart by their first word."""
    return [[f, f + 10, END] for f in firsts]


def test_beam_rank_tie_none_finished_short_and_over_cap():
    ninf = float("-inf")
    st = _book([3, 0, 2, 7],
               [[-1.0, -0.5, -0.5, 5.0],       # a tie between slots 1 and 2: slot 1 finished first; slot 3 is beyond the count
                [9.0, 9.0, 9.0, 9.0],          # no finished beam: whatever the slots hold is ignored
                [-2.0, -3.0, 0.0, 0.0],        # fewer finished beams than n_best_size
                [-4.0, -1.0, -3.0, -2.0]],     # a count above cap: the cap slots are ranked
               [_rows(1, 2, 3, 4), _rows(5, 5, 5, 5), _rows(6, 7, 8, 8), _rows(1, 2, 3, 4)])
    seq, score = S.beam_rank(st, 4, CAP, L, END, True, 3)
    assert seq.dtype == torch.int64 and tuple(seq.shape) == (4, 3, L) and tuple(score.shape) == (4, 3)
    assert seq[:, :, 0].tolist() == [[2, 3, 1], [END, END, END], [6, 7, END], [2, 4, 3]]
    assert seq[0, 0].tolist() == [2, 12, END] and seq[1].eq(END).all() and seq[2, 2].eq(END).all()
    assert score.tolist() == [[-0.5, -0.5, -1.0], [ninf, ninf, ninf], [-2.0, -3.0, ninf], [-1.0, -2.0, -3.0]]
    best, best_score = S.beam_rank(st, 4, CAP, L, END, False, 3)
    assert tuple(best.shape) == (4, L) and best.is_contiguous() and torch.equal(best, seq[:, 0])
    assert best_score.tolist() == [-0.5, ninf, -2.0, -1.0]
