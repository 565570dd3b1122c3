"""What every on-device search shares on the host: the cache of static-buffer states, the capture-or-replay rule of a
fixed launch sequence, and the book of a batched beam search.  Plain functions over plain dicts - tests and tools read
these dicts (``st["uses"]``, ``st["graph"]``, ``st["graphs"]``, ``st["tok"]``).

A search keeps its inputs, workspace and outputs in static buffers per shape (``lookup``).  Its launch sequence runs
eagerly on the first use of a state (also the warm-up a capture needs; a shape that never comes back is never captured)
and is captured into a HIP graph on the second and replayed from then on (``run``; AUDIOCAPTION_DECODE_GRAPH=0: always
eager).  A beam search is the buffers of base.py:290-323's per-clip bookkeeping (``beam_buffers``), their reset to the start
of a search (``beam_reset``), the device-side update of every step (``beam_update``) and the host-side ranking of the
finished beams (``beam_rank``).  A group beam search keeps one such book per group: the order of its steps
(``group_steps``), the earlier groups' planes a selection reads (``group_prev_planes``) and its result (``group_rank``)."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream


# ---- static-buffer states ----------------------------------------------------------------------------------------------
def lookup(states, key, build, keep):
    """The state of ``key`` in the dict ``states``, built by ``build()`` on a miss (a ``build`` that raises leaves the cache
    as it was), moved to most recently used (last); the oldest entries beyond ``keep`` are dropped.  Counts the use."""
    st = states.pop(key, None)
    if st is None:
        st = build()
        st["uses"] = 0
    states[key] = st
    while len(states) > keep:
        states.pop(next(iter(states)))
    st["uses"] += 1
    return st


def captures(st):
    """This use of the state replays a graph: not its first use, and AUDIOCAPTION_DECODE_GRAPH (read per call) is not 0."""
    return os.environ.get("AUDIOCAPTION_DECODE_GRAPH", "1") != "0" and st["uses"] >= 2


def replay(graphs, name, dev, launch):
    """Replay ``graphs[name]``, captured from ``launch()`` (fixed launches over static buffers) when it is not there yet."""
    graph = graphs.get(name)
    if graph is None:
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch()
        graphs[name] = graph
    graph.replay()


def run(st, dev, launch):
    """The whole launch sequence of a search: eager, or replayed from ``st["graph"]``."""
    if captures(st):
        replay(st, "graph", dev, launch)
    else:
        launch()


# ---- the beam book -----------------------------------------------------------------------------------------------------
def beam_buffers(dev, B, beam, max_length, start, end, pad):
    """Buffers of a beam search over B clips: two token planes (read / written in turn), the key-padding mask, cumulative
    scores, the per-clip bookkeeping (up to ``beam * max_length`` finished beams per clip), and ``tok0`` / ``mask0``, what
    plane 0 and the mask hold when a search starts."""
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    R, cap = B * beam, beam * max_length
    tok0 = torch.full((R, max_length + 1), end, **i32)
    tok0[:, 0] = start
    return {"tok0": tok0, "mask0": (tok0 == pad).to(torch.uint8), "end_idx": end,
            "tok": [torch.empty_like(tok0) for _ in range(2)], "mask": torch.empty(R, max_length + 1, device=dev, dtype=torch.uint8),
            "cum": torch.empty(R, **f32), "active": torch.empty(B, **i32), "done_cnt": torch.empty(B, **i32),
            "done_seq": torch.empty(B, cap, max_length, **i32), "done_score": torch.empty(B, cap, **f32),
            "src_row": torch.empty(R, **i32), "n_active": torch.empty(1, **i32),
            "top_val": torch.empty(B, beam, **f32), "top_idx": torch.empty(B, beam, **i32)}


def beam_reset(st, B):
    """The start of a search on the current stream (capturable)."""
    st["tok"][0].copy_(st["tok0"])
    st["tok"][1].fill_(st["end_idx"])
    st["mask"].copy_(st["mask0"])
    st["cum"].zero_()
    st["active"].fill_(1)
    st["done_cnt"].zero_()
    st["n_active"].fill_(B)


def beam_update(st, t, B, beam, V, max_length, end_idx, pad_idx, cap, all_rows=False):
    """Step t's bookkeeping from ``top_val`` / ``top_idx``: plane ``(t + 1) & 1``, mask, scores, finished beams and
    ``src_row`` (where each row's history comes from).  ``all_rows``: no clip is ever retired (the ensemble's search)."""
    name = "ac_trm_beam_update_all" if all_rows else "ac_trm_beam_update"
    tok = st["tok"]
    check(getattr(_lib.load(), name)(ptr(st["top_val"]), ptr(st["top_idx"]), ptr(tok[t & 1]), ptr(tok[(t + 1) & 1]),
                                     ptr(st["mask"]), ptr(st["cum"]), ptr(st["active"]), ptr(st["done_cnt"]),
                                     ptr(st["done_seq"]), ptr(st["done_score"]), ptr(st["src_row"]), ptr(st["n_active"]), B,
                                     beam, V, max_length, t, end_idx, pad_idx, cap, stream()), name)


def beam_rank(st, B, cap, max_length, end_idx, n_best, n_best_size):
    """The finished beams of every clip, best score first (stable: ties keep the order the beams finished in), on the host:
    ``seq`` (B, max_length) int64 and ``score`` (B,), or (B, n_best_size, max_length) and (B, n_best_size) with ``n_best``.
    Where a clip has fewer finished beams (or none) ``seq`` stays ``end_idx`` and ``score`` -inf."""
    counts, seqs, scores = st["done_cnt"].cpu().numpy(), st["done_seq"].cpu().numpy(), st["done_score"].cpu().numpy()
    width = n_best_size if n_best else 1
    seq = np.full((B, width, max_length), end_idx, dtype=np.int64)
    score = np.full((B, width), -np.inf, dtype=np.float32)
    for i in range(B):
        n = min(int(counts[i]), cap)
        order = sorted(range(n), key=lambda j: -scores[i, j])
        for j, o in enumerate(order[:width]):
            seq[i, j] = seqs[i, o]
            score[i, j] = scores[i, o]
    seq, score = torch.from_numpy(seq), torch.from_numpy(score)
    return (seq, score) if n_best else (seq[:, 0], score[:, 0])


# ---- group beam search: G beam books staggered in time (base.py:413-417) --------------------------------------------------
def group_steps(G, max_length):
    """``(g, lt)`` of every group step in launch order: at global step t = 0 .. max_length + G - 2 the groups g = 0 .. G - 1 whose
    local position lt = t - g lies in 0 .. max_length - 1."""
    return [(g, t - g) for t in range(max_length + G - 1) for g in range(G) if 0 <= t - g < max_length]


def group_prev_planes(books, g, lt, max_length):
    """What ``ac_group_beam_select`` takes as ``prev_tok`` when group g stands at lt: the CURRENT token planes of the books
    of groups 0 .. g - 1 as a ctypes array (None for group 0).  Group q has by then finished its step at
    min(lt + g - q, max_length - 1), whose update wrote plane ``(step + 1) & 1``."""
    if g == 0:
        return None
    planes = [books[q]["tok"][(min(lt + g - q, max_length - 1) + 1) & 1] for q in range(g)]
    return (ctypes.c_void_p * g)(*[p.data_ptr() for p in planes])


def group_rank(books, B, bdash, max_length, end_idx, beam_size, group_nbest):
    """base.py:463-469: per group its ``bdash`` best finished beams (``beam_rank``); ``seq`` (B, beam_size, max_length) int64 on
    the host with group 0's captions first (rows beyond G * bdash stay ``end_idx``), or (B, G, max_length), the best of each
    group, without ``group_nbest``."""
    G = len(books)
    seq = torch.full((B, beam_size if group_nbest else G, max_length), end_idx, dtype=torch.int64)
    for g, book in enumerate(books):
        best, _ = beam_rank(book, B, bdash * max_length, max_length, end_idx, True, bdash)
        if group_nbest:
            seq[:, g * bdash:(g + 1) * bdash] = best
        else:
            seq[:, g] = best[:, 0]
    return seq
