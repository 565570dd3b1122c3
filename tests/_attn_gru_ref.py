"""CPU restatement in torch of the attention-GRU caption decoder and its searches (reference hf_wrapper.py:1377-1554
Seq2SeqAttention / BahAttnCatFcDecoder / TemporalBahAttnDecoder, :1557-1788 the two models, base.py greedy / beam search).

``sd`` is the decoder's state dict (torch tensors, no prefix); ``tags`` (B,) selects the temporal decoder's first input,
None the plain decoder's <start>.  ``dtype`` switches the arithmetic (torch.float64 for the error budget of the GPU
tests).  tests/test_attn_gru_oracle.py holds these functions to the reference's recorded outputs
(tests/golden/g19_attn_gru.npz).
"""
import os

import numpy as np
import torch

import _sampling_ref as SR
from audiocaption_amd import procedural as P

START_IDX, END_IDX, PAD_IDX = 1, 2, 0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = {
    "pub": dict(emb_dim=512, d_model=512, attn_size=512, attn_emb_dim=512, fc_emb_dim=512, vocab_size=4981),
    "small": dict(emb_dim=64, d_model=128, attn_size=96, attn_emb_dim=160, fc_emb_dim=96, vocab_size=517),
}
CASES = ["pub_t", "pub_p", "small_t", "small_p"]


def load_g19():
    return dict(np.load(os.path.join(GOLDEN, "g19_attn_gru.npz")))


def case_inputs(g, case):
    """(state dict, attn_emb, lens, fc_emb, tags or None) of a fixture case from its recipe (CPU tensors)."""
    shape, kind = case.split("_")
    temporal = kind == "t"
    seed, scale = g[case + "_recipe"].tolist()
    sd = P.to_torch(P.bah_decoder_state(temporal=temporal, seed=int(seed), end_scale=scale, **SHAPES[shape]))
    if shape == "pub":
        g3 = np.load(os.path.join(GOLDEN, "g3_decoder.npz"))
        mem, lens, tags = g3["attn_emb"], g3["attn_emb_len"].astype(np.int64), [0, 1, 2, 3]
    else:
        mem = np.random.default_rng(int(g["small_seed"])).normal(0.0, 0.25, (5, 70, 160)).astype(np.float32)
        lens, tags = g["small_lens"].astype(np.int64), [0, 1, 2, 3, 0]
    mem_t, lens_t = torch.from_numpy(mem), torch.from_numpy(lens)
    valid = (torch.arange(mem_t.shape[1])[None, :] < lens_t[:, None]).float()
    fc = ((mem_t * valid[:, :, None]).sum(1) / lens_t[:, None].float())[:, :SHAPES[shape]["fc_emb_dim"]].contiguous()
    return sd, mem_t, lens_t, fc, (torch.tensor(tags) if temporal else None)



def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def step(sd, embed, h, attn_emb, lens, fc_emb):
    """One decoder step (hf_wrapper.py:1390-1414,1533-1554): input embedding (N, E), state (N, d), memory (N, Tm, A) with
    lengths, fc_emb (N, F) -> (new state, logit (N, V), attention weights (N, Tm)); the GRU output equals the new state."""
    N, Tm, _ = attn_emb.shape
    d = h.shape[1]
    attn_in = torch.cat((h.unsqueeze(1).expand(N, Tm, d), attn_emb), dim=-1)
    attn_out = torch.tanh(attn_in @ sd["attn.h2attn.weight"].T + sd["attn.h2attn.bias"])
    score = attn_out @ sd["attn.v"]
    mask = torch.arange(Tm).unsqueeze(0) < torch.as_tensor(lens).view(-1, 1)
    score = score.masked_fill(~mask, -1e10)
    w = torch.softmax(score, dim=-1)
    ctx = torch.bmm(w.unsqueeze(1), attn_emb).squeeze(1)
    p_fc = fc_emb @ sd["fc_proj.weight"].T + sd["fc_proj.bias"]
    p_ctx = ctx @ sd["ctx_proj.weight"].T + sd["ctx_proj.bias"]
    x = torch.cat((embed, p_ctx, p_fc), dim=-1)
    gi = x @ sd["model.weight_ih_l0"].T + sd["model.bias_ih_l0"]
    gh = h @ sd["model.weight_hh_l0"].T + sd["model.bias_hh_l0"]
    i_r, i_z, i_n = gi.chunk(3, 1)
    h_r, h_z, h_n = gh.chunk(3, 1)
    r = torch.sigmoid(i_r + h_r)
    z = torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    hn = (1 - z) * n + z * h
    return hn, hn @ sd["classifier.weight"].T + sd["classifier.bias"], w


def input_embed(sd, words, tags, t):
    if t == 0 and tags is not None:
        return sd["temporal_embedding.weight"][torch.as_tensor(tags).long()]
    return sd["word_embedding.weight"][words]


def greedy(sd, attn_emb, lens, fc_emb, tags=None, max_length=20, stop=True, dtype=torch.float32, pick=None):
    """argmax of log_softmax(logit) per step.  ``stop`` (the product's contract): after a row's first <end> its seq columns
    are <end> and its value, logit, embed and attention columns 0, and the loop ends when every row has ended.  stop=False
    is the reference's bookkeeping (base.py:152-170): every row is written at every executed step.  Either way the state
    of every row advances at every executed step (with <end> as input once a row has ended), as in the reference.
    ``pick(t, logit) -> (word, value)`` replaces the argmax (sampling)."""
    sd = cast(sd, dtype)
    attn_emb, fc_emb = attn_emb.to(dtype), fc_emb.to(dtype)
    B, Tm, _ = attn_emb.shape
    V, d = sd["classifier.weight"].shape
    seq = torch.full((B, max_length), END_IDX, dtype=torch.long)
    out = {"sampled_logprob": torch.zeros(B, max_length, dtype=dtype), "logit": torch.zeros(B, max_length, V, dtype=dtype),
           "embed": torch.zeros(B, max_length, d, dtype=dtype), "attn_weight": torch.zeros(B, Tm, max_length, dtype=dtype),
           "gap": torch.full((B, max_length), float("inf"), dtype=dtype), "top_val": torch.zeros(B, max_length, 8, dtype=dtype),
           "top_idx": torch.zeros(B, max_length, 8, dtype=torch.long),
           "unfinished_cnt": torch.zeros(max_length, dtype=torch.int32)}
    h = torch.zeros(B, d, dtype=dtype)
    unfinished = torch.ones(B, dtype=torch.bool)
    steps = 0
    for t in range(max_length):
        words = torch.full((B,), START_IDX, dtype=torch.long) if t == 0 else seq[:, t - 1]
        h, logit, w = step(sd, input_embed(sd, words, tags, t), h, attn_emb, lens, fc_emb)
        lp = torch.log_softmax(logit, dim=1)
        if pick is None:
            v, word = torch.max(lp, 1)
        else:
            word, v = pick(t, logit)
        tv, ti = lp.topk(8, dim=1)
        steps += 1
        live = unfinished.clone() if stop else torch.ones(B, dtype=torch.bool)
        out["top_val"][live, t], out["top_idx"][live, t] = tv[live], ti[live]
        out["gap"][live, t] = (tv[:, 0] - tv[:, 1])[live]
        out["sampled_logprob"][live, t] = v[live].to(dtype)
        out["logit"][live, t], out["embed"][live, t] = logit[live], h[live]
        out["attn_weight"][live, :, t] = w[live]
        seq[live, t] = word[live]
        unfinished = unfinished & (word != END_IDX)
        seq[~unfinished, t] = END_IDX
        out["unfinished_cnt"][t] = int(unfinished.sum())
        if not unfinished.any():
            break
    out.update(seq=seq, state=h.unsqueeze(0), steps=steps)
    return out


def beam_search(sd, attn_emb, lens, fc_emb, tags=None, beam_size=3, max_length=20, temp=1.0, n_best=False, n_best_size=None,
                dtype=torch.float32, trace=None):
    """base.py:254-361 clip by clip with the attention bookkeeping of hf_wrapper.py:1612-1674: the weights of step t go to
    column t of every beam row BEFORE the rows are re-gathered by the step's parent beams; a clip's ``attn_weight`` is that
    of beam row 0 after the last reorder; the clip exits when its finished count EQUALS beam_size.  Columns never written
    are 0 (the reference: torch.empty)."""
    sd = cast(sd, dtype)
    attn_emb, fc_emb = attn_emb.to(dtype), fc_emb.to(dtype)
    B, Tm, _ = attn_emb.shape
    V, d = sd["classifier.weight"].shape
    n_best_size = beam_size if n_best_size is None else n_best_size
    out_seq = torch.full((B, max_length), END_IDX, dtype=torch.long)
    nbest_seq = torch.full((B, n_best_size, max_length), END_IDX, dtype=torch.long)
    attn_weight = torch.zeros(B, Tm, max_length, dtype=dtype)
    for i in range(B):
        mem, ln = attn_emb[i:i + 1].expand(beam_size, Tm, -1), torch.as_tensor(lens)[i:i + 1].expand(beam_size)
        fc = fc_emb[i:i + 1].expand(beam_size, -1)
        tg = None if tags is None else torch.as_tensor(tags)[i:i + 1].expand(beam_size)
        topk_logprob = torch.zeros(beam_size, dtype=dtype)
        h = torch.zeros(beam_size, d, dtype=dtype)
        aw = torch.zeros(beam_size, Tm, max_length, dtype=dtype)
        seq, next_word, done = None, None, []
        for t in range(max_length):
            words = torch.full((beam_size,), START_IDX, dtype=torch.long) if t == 0 else next_word
            h_in = h if t == 0 else h[prev_beam]
            h, logit, w = step(sd, input_embed(sd, words, tg, t), h_in, mem, ln, fc)
            lp = torch.log_softmax(torch.log_softmax(logit, dim=1) / temp, dim=1)
            lp = topk_logprob.unsqueeze(1) + lp
            flat = lp[0] if t == 0 else lp.reshape(-1)
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
                              "prev_beam": prev_beam.tolist()})
            for b in range(beam_size):
                if is_end[b]:
                    done.append({"seq": seq[b].clone(), "score": topk_logprob[b].item() / (t + 1)})
            topk_logprob = topk_logprob.clone()
            topk_logprob[is_end] -= 1000
            aw[..., t] = w
            aw = aw[prev_beam]
            if len(done) == beam_size:
                break
        done = sorted(done, key=lambda x: -x["score"])   # stable: ties keep the order the beams finished in
        out_seq[i, :len(done[0]["seq"])] = done[0]["seq"]
        for j, dn in enumerate(done[:n_best_size]):
            nbest_seq[i, j, :len(dn["seq"])] = dn["seq"]
        attn_weight[i] = aw[0]
    return {"seq": nbest_seq if n_best else out_seq, "attn_weight": attn_weight}


METHOD_CODES = {"sample": SR.PLAIN, "gumbel": SR.GUMBEL}


def parse_method(method):
    """(code, k, p) of a sample_method name as base.py:217-233 reads it."""
    if method.startswith("top"):
        num = float(method[3:])
        return (SR.TOPP, 0, num) if 0 < num < 1 else (SR.TOPK, int(num), 0.0)
    return METHOD_CODES.get(method, SR.PLAIN), 0, 0.0


def sample_pick(method, temp, seed):
    """A ``pick`` for ``greedy``: the word the on-device sampler draws for (seed, step, row) and the value it stores."""
    code, k, p = parse_method(method)

    def pick(t, logit):
        words, stored, _, _ = SR.sample_rows(logit.double().numpy(), code, k, p, temp, seed, t)
        return torch.from_numpy(words).long(), torch.from_numpy(stored)

    return pick


def first_end(row, end_idx=END_IDX):
    """Columns of a caption up to and including its first <end> (the whole row when it has none)."""
    row = list(row)
    return row.index(end_idx) + 1 if end_idx in row else len(row)


def live_mask(seq):
    """(B, L) bool: positions up to and including each row's first <end>."""
    seq = np.asarray(seq)
    m = np.zeros(seq.shape, dtype=bool)
    for i, row in enumerate(seq.tolist()):
        m[i, :first_end(row)] = True
    return m


def error_budget(ref32, ref64, live, keys=("attn_weight", "state", "embed")):
    """n per quantity: the largest deviation of the f32 restatement from the float64 one (over live positions)."""
    n = {}
    for k in keys:
        a, b = ref32[k].double(), ref64[k]
        if k == "attn_weight" and live is not None:
            m = torch.from_numpy(live)[:, None, :].expand_as(a)
        elif k == "embed" and live is not None:
            m = torch.from_numpy(live)[:, :, None].expand_as(a)
        else:
            m = torch.ones_like(a, dtype=torch.bool)
        n[k] = float((a - b)[m].abs().max())
    return n
