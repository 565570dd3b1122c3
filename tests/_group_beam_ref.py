"""Group (diverse) beam search restated in plain torch (base.py:363-471 diverse_beam_search), over a step function - what
tests/golden/make_golden_group_beam.py holds against the reference's own run, and what the CPU and GPU tests of
``TransformerModel.group_beam_search`` compare with.

G groups of bdash = beam_size // G beams per clip.  At global step t = 0 .. L + G - 2 the groups g = 0 .. G - 1 with
0 <= lt = t - g <= L - 1 make one beam step each, in that order: lp = log_softmax(log_softmax(z) / temp), minus
count[w] * lambda with count[w] the rows of groups 0 .. g - 1 whose CURRENT beams hold w at position lt, plus the row's
cumulative score; the top bdash of the flattened bdash * V (row 0 alone at lt == 0); finished beams (``<end>``, or every
beam at lt == L - 1) are recorded with score / (lt + 1) and go on at -1000.  Per group the bdash best finished beams, stable.

The models are the decoder-only procedural draws of tests/test_gpu_decode_select.py over the encoder memory of
tests/golden/g4_greedy.npz; a clip is (k, length) as there."""
import functools
import os

import numpy as np
import torch

from oracle import cpu_path as O

END, PAD, START = O.END_IDX, O.PAD_IDX, O.START_IDX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "g_group_beam.npz")

MARGIN = 1e-3        # test_gpu_decode_select.py: a gap in the scores below which the kept ids are no meaningful comparison
SCORE_GAP = 2e-4     # finished-beam scores closer than this could sort either way in float32

# (id, G, bdash, beam_size, lambda, temp, max_length, V): the cases of the end-to-end comparison
CASES = [
    ("G3-b2-L20-V100", 3, 2, 6, 0.5, 1.0, 20, 100),
    ("G2-b1-t1.7-L2-V5121", 2, 1, 2, 0.5, 1.7, 2, 5121),
    ("G3-b1-L1-V100", 3, 1, 3, 1.0, 1.0, 1, 100),            # L < G
    ("G8-b8-t0.5-L4-V100", 8, 8, 64, 0.5, 0.5, 4, 100),      # 64 rows per clip
    ("G1-b3-L20-V100", 1, 3, 3, 0.5, 1.0, 20, 100),
    ("G3-b2-beam7-L20-V100", 3, 2, 7, 0.5, 1.0, 20, 100),    # beam_size % G != 0: the seventh row stays end_idx
]
CASE_IDS = [c[0] for c in CASES]
OTHER_LAMBDA = 2.0   # case 0 under another penalty (the cached-state test): other captions, the same guards (CPU test)
# candidate clips in the order the generator tries them (memory lengths include 1); it keeps the first CLIPS_PER_CASE that
# pass the tie guards on the reference's own run, at least one of them of length 1
CANDIDATE_CLIPS = [(2, 1), (0, 31), (3, 1), (1, 27), (6, 15), (5, 5), (5, 1), (2, 15), (3, 29), (7, 5), (4, 1), (0, 5), (7, 29),
                   (3, 5), (0, 1), (1, 1)] + [(k, 1) for k in range(6, 64)]
CLIPS_PER_CASE = 3


@functools.lru_cache(maxsize=None)
def golden_memory():
    g = np.load(os.path.join(GOLDEN, "g4_greedy.npz"))
    return torch.from_numpy(g["attn_emb"]), g["attn_emb_len"]


def clips(spec):
    """(k, length) pairs -> attn_emb (B, Tm, A) and attn_emb_len (B,): golden clip k % 4 with its frames rolled by k // 4."""
    emb, _ = golden_memory()
    e = torch.cat([torch.roll(emb[k % 4:k % 4 + 1], k // 4, dims=1) for k, _ in spec])
    return e.contiguous(), torch.tensor([ln for _, ln in spec], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def state(V):
    from audiocaption_amd import procedural as P
    return P.to_torch(P.decoder_state_diverse("beam", vocab_size=V))


def decoder_step(st, attn_emb, attn_emb_len):
    """step(clip, words): words (n, lt) int64, the rows' words so far -> (n, V) raw logits of position lt, the decoder run
    on start token + words with the key-padding mask ``== PAD`` as oracle.cpu_path.beam_search runs it."""
    lens = torch.as_tensor(attn_emb_len)

    def step(clip, words):
        n = words.shape[0]
        word = torch.cat([torch.full((n, 1), START, dtype=torch.long), words], dim=1)
        out = O.decoder_forward(st, word, attn_emb[clip:clip + 1].repeat(n, 1, 1), lens[clip:clip + 1].repeat(n), word == PAD)
        return out["logit"][:, -1]
    return step


def group_beam_search(step, B, V, beam_size, group_size, max_length, temp=1.0, diversity_lambda=0.5, group_nbest=True,
                      end_idx=END, trace=None):
    """``seq`` (B, beam_size, max_length) int64 (or (B, group_size, max_length) without ``group_nbest``) filled with
    ``end_idx``.  ``trace`` (a list) receives one record per (clip, group, lt): the kept scores (``kept``) and the first
    cut (``first_cut``), the smallest gap among them (``margin``) and the gap at the cut (``cut``), the kept words and their
    parents, and the scores of the beams that finished."""
    G, L = group_size, max_length
    bdash = beam_size // G
    seq_out = torch.full((B, beam_size if group_nbest else G, L), end_idx, dtype=torch.long)
    for i in range(B):
        seqs = [torch.zeros(bdash, 0, dtype=torch.long) for _ in range(G)]
        cum = [None] * G
        done = [[] for _ in range(G)]
        for t in range(L + G - 1):
            for g in range(G):
                lt = t - g
                if not 0 <= lt <= L - 1:
                    continue
                z = step(i, seqs[g])
                if cum[g] is None:
                    cum[g] = torch.zeros(bdash, dtype=z.dtype)
                lp = torch.log_softmax(torch.log_softmax(z, dim=1) / temp, dim=1)
                if g > 0:
                    change = torch.zeros(V, dtype=torch.float32)
                    for q in range(g):
                        change.scatter_add_(0, seqs[q][:, lt], torch.ones(bdash))
                    lp = lp - change.to(lp.dtype)[None] * diversity_lambda
                cand = cum[g][:, None] + lp
                flat = cand[0] if lt == 0 else cand.reshape(-1)
                top_val, top_idx = flat.topk(bdash, 0, True, True)
                prev, word = torch.div(top_idx, V, rounding_mode="trunc"), top_idx % V
                seqs[g] = torch.cat([seqs[g][prev], word[:, None]], dim=1)
                is_end = word == end_idx
                if lt == L - 1:
                    is_end = torch.ones_like(is_end)
                ends = [top_val[b].item() / (lt + 1) for b in range(bdash) if is_end[b]]
                for b in range(bdash):
                    if is_end[b]:
                        done[g].append({"seq": seqs[g][b].clone(), "score": top_val[b].item() / (lt + 1)})
                cum[g] = top_val.clone()
                cum[g][is_end] -= 1000
                if trace is not None:
                    c = flat.topk(min(bdash + 1, flat.numel())).values.double()
                    gaps = c[:-1] - c[1:]
                    trace.append({"clip": i, "g": g, "lt": lt, "margin": float(gaps.min()) if len(gaps) else float("inf"),
                                  "cut": float(gaps[-1]) if len(c) > bdash else float("inf"), "kept": c[:bdash].tolist(),
                                  "first_cut": float(c[bdash]) if len(c) > bdash else float("-inf"), "words": word.tolist(),
                                  "prev": prev.tolist(), "end_scores": ends})
        best = [sorted(d, key=lambda x: -x["score"])[:bdash] for d in done]
        rows = sum(best, []) if group_nbest else [b[0] for b in best]
        for j, d in enumerate(rows):
            seq_out[i, j, :len(d["seq"])] = d["seq"]
    return {"seq": seq_out}


def guards(trace, bdash):
    """(smallest margin over every step, smallest gap among the finished scores that decide a group's top bdash)."""
    margin = min(r["margin"] for r in trace)
    score_gap = float("inf")
    for key in sorted({(r["clip"], r["g"]) for r in trace}):
        sc = sorted((s for r in trace if (r["clip"], r["g"]) == key for s in r["end_scores"]), reverse=True)[:bdash + 1]
        for a, b in zip(sc[:-1], sc[1:]):
            score_gap = min(score_gap, a - b)
    return margin, score_gap


def run_case(case, spec, group_nbest=True, trace=None, dtype=torch.float32, **over):
    """The restatement on one case of ``CASES`` over the clips ``spec``; ``over``: parameters to replace."""
    _, G, bdash, beam, lam, temp, L, V = case
    p = dict(beam_size=beam, group_size=G, max_length=L, temp=temp, diversity_lambda=lam)
    p.update(over)
    st = state(V)
    if dtype != torch.float32:
        st = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}
    emb, lens = clips(spec)
    return group_beam_search(decoder_step(st, emb.to(dtype), lens), len(spec), V, group_nbest=group_nbest, trace=trace, **p)


@functools.lru_cache(maxsize=None)
def fixture():
    """g_group_beam.npz: per case ``<id>/clips`` (n, 2), ``<id>/seq`` (group_nbest), ``<id>/seq_best`` (without) - the
    reference's own results - and ``<id>/gaps`` = (margin, score gap) found on the reference's run."""
    f = np.load(FIXTURE)
    return {k: f[k] for k in f.files}


def case_clips(case_id):
    return [tuple(int(v) for v in row) for row in fixture()[f"{case_id}/clips"]]
