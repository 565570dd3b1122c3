"""CPU restatement of ensemble decoding (reference python_scripts/train_eval/ensemble.py: stepwise_forward :94-151,
beam_search :154-276, sample_next_word_with_logprob :412-449) on the decoder of ``oracle/cpu_path.py``.

A member is a dict {"state", "attn_emb", "attn_emb_len"} (+ optional "prefix", default "decoder."): its own weights and its
own audio memory of its own length.  Members share the prefix tokens and the vocabulary.  ``tests/test_ensemble_oracle.py``
holds these functions to the reference's recorded outputs (tests/golden/g16_ensemble.npz); the wav-to-tokens GPU test uses
them over the oracle's encoders, for whole models no fixture can carry.
"""
import torch

from oracle import cpu_path as O

START_IDX, END_IDX, PAD_IDX = O.START_IDX, O.END_IDX, O.PAD_IDX


def mean_logprob(members, word, rows=None, repeat=1):
    """m = mean_n log_softmax(logit_n) of the last position of ``word`` (N, T), f32, not renormalised (:133-136, :212-216).
    ``rows`` selects clips of every member's memory, ``repeat`` repeats each of them (beam rows)."""
    lps = []
    for mb in members:
        mem, lens = mb["attn_emb"], torch.as_tensor(mb["attn_emb_len"])
        if rows is not None:
            mem, lens = mem[rows], lens[rows]
        if repeat > 1:
            mem, lens = mem.repeat_interleave(repeat, 0), lens.repeat_interleave(repeat, 0)
        logit = O.decoder_forward(mb["state"], word, mem, lens, word == PAD_IDX, mb.get("prefix", "decoder."))["logit"][:, -1]
        lps.append(torch.log_softmax(logit, -1))
    return torch.stack(lps).mean(dim=0)


def greedy(members, max_length=20, stop=True):
    """argmax m per step; the stored value is m[word].  ``stop`` (the product's contract): a row's columns after its first
    <end> are <end> with value 0 and the loop ends when every row has.  stop=False is the reference (:111-150): all
    max_length steps, words kept after <end>.  Also returns per executed step the whole m's top-8 and top-1 / top-2 gap."""
    B = members[0]["attn_emb"].shape[0]
    seq = torch.full((B, max_length), END_IDX, dtype=torch.long)
    value = torch.zeros(B, max_length)
    gap = torch.full((B, max_length), float("inf"))
    top_val = torch.zeros(B, max_length, 8)
    top_idx = torch.zeros(B, max_length, 8, dtype=torch.long)
    unfinished = torch.ones(B, dtype=torch.bool)
    steps = 0
    for t in range(max_length):
        word = torch.cat([torch.full((B, 1), START_IDX, dtype=torch.long), seq[:, :t]], dim=1)
        m = mean_logprob(members, word)
        v, w = torch.max(m, 1)
        tv, ti = m.topk(8, dim=1)
        steps += 1
        live = unfinished.clone() if stop else torch.ones(B, dtype=torch.bool)
        top_val[live, t], top_idx[live, t] = tv[live], ti[live]
        gap[live, t] = (tv[:, 0] - tv[:, 1])[live]
        seq[live, t] = w[live]
        value[live, t] = v[live]
        unfinished = unfinished & (w != END_IDX)
        if stop and not unfinished.any():
            break
    return {"seq": seq, "sampled_logprob": value, "gap": gap, "top_val": top_val, "top_idx": top_idx, "steps": steps}


def beam_search(members, beam_size=3, max_length=20, temp=1.0, n_best=False, n_best_size=None, retire=False, trace=None):
    """:154-276.  score = log_softmax(m / temp) + topk_logprob; finished beams get score / (t + 1) and -1000; the search
    NEVER retires a clip (no ``len(done) == beam_size`` break as base.py has: ``retire=True`` adds it back, to show what a
    retiring implementation would return).  Returns the best caption (or the n_best list) and, always, "nbest_score"."""
    B = members[0]["attn_emb"].shape[0]
    V = members[0]["state"][members[0].get("prefix", "decoder.") + "classifier.weight"].shape[0]
    n_best_size = beam_size if n_best_size is None else n_best_size
    out_seq = torch.full((B, max_length), END_IDX, dtype=torch.long)
    nbest_seq = torch.full((B, n_best_size, max_length), END_IDX, dtype=torch.long)
    nbest_score = torch.full((B, n_best_size), float("-inf"))
    for i in range(B):
        topk_logprob = torch.zeros(beam_size)
        seq = None
        done = []
        for t in range(max_length):
            start = torch.full((beam_size, 1), START_IDX, dtype=torch.long)
            word = start if t == 0 else torch.cat([start, seq], dim=1)
            m = mean_logprob(members, word, rows=slice(i, i + 1), repeat=beam_size)
            lp = torch.log_softmax(m / temp, dim=1)
            lp = topk_logprob.unsqueeze(1) + lp
            flat = lp[0] if t == 0 else lp.view(-1)
            topk_logprob, topk_words = flat.topk(beam_size, 0, True, True)
            prev_beam = torch.div(topk_words, V, rounding_mode="trunc")
            next_word = topk_words % V
            seq = next_word.unsqueeze(1) if t == 0 else torch.cat([seq[prev_beam], next_word.unsqueeze(1)], dim=1)
            is_end = next_word == END_IDX
            if t == max_length - 1:
                is_end = torch.ones_like(is_end)
            if trace is not None:
                cand = flat.topk(beam_size + 1).values
                trace.append({"clip": i, "t": t, "margin": float((cand[:-1] - cand[1:]).min()),
                              "ended": is_end.tolist(), "prev_beam": prev_beam.tolist()})
            for b in range(beam_size):
                if is_end[b]:
                    done.append({"seq": seq[b].clone(), "score": topk_logprob[b].item() / (t + 1)})
            topk_logprob = topk_logprob.clone()
            topk_logprob[is_end] -= 1000
            if retire and len(done) == beam_size:
                break
        done = sorted(done, key=lambda x: -x["score"])   # stable: ties keep the order the beams finished in
        out_seq[i, :len(done[0]["seq"])] = done[0]["seq"]
        for j, d in enumerate(done[:n_best_size]):
            nbest_seq[i, j, :len(d["seq"])] = d["seq"]
            nbest_score[i, j] = d["score"]
    return {"seq": nbest_seq if n_best else out_seq, "nbest_score": nbest_score}


def sample_distribution(m, method, temp):
    """The (unnormalised) logits ensemble.py:426-445 hands to Categorical for rows m (N, V), and the value it stores for
    every word (N, V).  "gumbel": argmax(m + Gumbel) is a draw from softmax(m) and the stored value is m (:423-425)."""
    m = m.clone()
    if method == "gumbel":
        return m, m
    lp = m / temp
    if method.startswith("top"):
        num = float(method[3:])
        if 0 < num < 1:
            probs = torch.softmax(lp, dim=1)
            sp, si = torch.sort(probs, descending=True, dim=1)
            mask = sp.cumsum(1) < num
            mask = torch.cat([torch.ones_like(mask[:, :1]), mask[:, :-1]], 1)
            sp = sp * mask.to(sp)
            sp = sp / sp.sum(1, keepdim=True)
            lp = lp.scatter(1, si, sp.log())
        else:
            tmp = torch.full_like(lp, float("-inf"))
            tv, ti = torch.topk(lp, int(num), dim=1)
            lp = tmp.scatter(1, ti, tv)
    return lp, lp


def first_end(row, end_idx=END_IDX):
    """Columns of a caption up to and including its first <end> (the whole row when it has none)."""
    row = list(row)
    return row.index(end_idx) + 1 if end_idx in row else len(row)
