"""Keyword-conditioned Transformer captioners (audiocaption_amd.KeywordCondTransformerModel over a
KeywordProbTransformerDecoder): shapes, seeded procedural weights and inputs, and the CPU restatement shared by
tests/golden/make_golden_keyword_trm.py (against the reference), tests/test_keyword_trm_cpu.py and
tests/test_gpu_keyword_trm.py.  A helper module, not a conftest.

The restatement is the reference's arithmetic (transformer_decoder.py:186-214) in the dtype of the state it is handed
(float32 or float64): ``decoder_pass`` is oracle.train_path.decoder_pass with the embedding row

    x = LayerNorm(dropA(E[word]) * sqrt(d) + keyword_proj(keyword)[clip]; word_keyword_norm) + pe[pos], then dropB

in the place of ``dropA(E[word]) * sqrt(d) + pe``; with p = 0 it is the eval-mode forward.  The searches are
oracle.cpu_path's greedy_decode / beam_search run over that forward."""
import contextlib
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_path as O
from oracle import train_path as OT

import _attn_gru_train_ref as AT
import _trm_train_ref as ET

END, PAD, START = O.END_IDX, O.PAD_IDX, O.START_IDX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATE = 1e-4                     # logits against the reference, absolute; also the draw rule's smallest gap
COIN_SEED = 3                   # random.seed before every reference training forward: ss_ratio 0.5 draws the coins 1 0 1 0 0

# constructor arguments of the decoder per shape.  d128: two heads of 64 on the general launch sequence; d256: four heads
# of 64, the fused per-row kernels, and the width the training engine is built for (attn_emb_dim 512 = the bi-GRU's)
SHAPES = {
    "d128": dict(emb_dim=128, vocab_size=60, fc_emb_dim=64, attn_emb_dim=64, nhead=2, nlayers=2, dim_feedforward=256,
                 keyword_classes_num=30),
    "d256": dict(emb_dim=256, vocab_size=61, fc_emb_dim=512, attn_emb_dim=512, nhead=4, nlayers=2, dim_feedforward=512,
                 keyword_classes_num=30),
}
B, TM, LENS, MAX_LENGTH = 3, 7, (7, 4, 1), 6          # the searches: ragged attn_emb_len
BEAMS = (2, 3)
TRAIN_N, TRAIN_TQ, TRAIN_LENS, TRAIN_TC, TRAIN_CAP_LEN = 3, 7, (7, 4, 1), 6, (6, 4, 5)     # training: T = 5
# candidate draws, tried in order by the fixture maker: (seed, end_beta)
CANDIDATES = [(seed, beta) for seed in range(27, 39) for beta in (2.0, 3.0, 1.5)]


def oracle_kw(shape):
    return {"nlayers": SHAPES[shape]["nlayers"], "nhead": SHAPES[shape]["nhead"]}


def f64(state):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def decoder_state(shape, seed, end_beta):
    """``procedural.keyword_decoder_state`` at the shape under ``decoder.``, with the high-entropy scales of
    tests/_decoder_shapes.diverse_state (embedding and word_keyword_norm.weight x 3, positional encoding x 4, <end> aligned
    with the last norm3.bias at ``end_beta``): float32 torch tensors.  Left unchanged by its readers."""
    from audiocaption_amd import procedural as P
    s = SHAPES[shape]
    st = P.keyword_decoder_state("decoder.", s["vocab_size"], s["keyword_classes_num"], s["emb_dim"], s["attn_emb_dim"],
                                 s["nlayers"], s["dim_feedforward"], seed=int(seed))
    st["decoder.word_embedding.weight"] = st["decoder.word_embedding.weight"] * np.float32(3.0)
    st["decoder.pos_encoder.pe"] = st["decoder.pos_encoder.pe"] * np.float32(4.0)
    # word_keyword_norm brings the embedding rows back to unit variance: its gain restores the embedding's scale of 3
    st["decoder.word_keyword_norm.weight"] = st["decoder.word_keyword_norm.weight"] * np.float32(3.0)
    b3 = st[f"decoder.model.layers.{s['nlayers'] - 1}.norm3.bias"]
    cw = st["decoder.classifier.weight"].copy()
    cw[END] = ((float(end_beta) / float(np.dot(b3, b3))) * b3).astype(np.float32)
    st["decoder.classifier.weight"] = cw
    return P.to_torch(st)


@functools.lru_cache(maxsize=None)
def model_state(seed, end_beta):
    """The trainable tensors of the whole d256 model for the training cases: ``decoder_state("d256")`` plus the bi-GRU of
    ``procedural.gru_state`` under ``encoder.rnn.`` (the Cnn14 is preset and never run)."""
    from audiocaption_amd import procedural as P
    st = dict(P.to_torch(P.gru_state("encoder.rnn.", 2048, 256, 3, int(seed))))
    st.update(decoder_state("d256", seed, end_beta))
    return st


@functools.lru_cache(maxsize=None)
def trm_model_state(seed):
    """The trainable tensors of the keyword captioner over a Cnn14TransformerEncoder (config.cnn14trm_trm_config with the
    keyword pair: decoder memory 256 wide), plain procedural draws."""
    from audiocaption_amd import procedural as P
    s = SHAPES["d256"]
    st = dict(P.trm_encoder_state("encoder.trm.", 2048, 256, 2, 1024, int(seed)))
    st.update(P.keyword_decoder_state("decoder.", s["vocab_size"], s["keyword_classes_num"], 256, 256, 2, s["dim_feedforward"],
                                      seed=int(seed)))
    return P.to_torch(st)


def keywords(rows, classes, seed, zero_row=None):
    """(rows, classes) float32: row 0 multi-hot (three classes), the others probabilities; ``zero_row`` all zero."""
    g = torch.Generator().manual_seed(1000 + seed)
    kw = torch.rand(rows, classes, generator=g) * (torch.rand(rows, classes, generator=g) < 0.2)
    kw[0] = 0.0
    kw[0, torch.randperm(classes, generator=g)[:min(3, classes)]] = 1.0
    if zero_row is not None:
        kw[zero_row] = 0.0
    return kw


def infer_inputs(shape, which=0):
    """(attn_emb (B, TM, A), attn_emb_len, keyword (B, C)) of the searches; ``which`` 1: the second keyword batch."""
    g = torch.Generator().manual_seed(271)
    attn = torch.randn(B, TM, SHAPES[shape]["attn_emb_dim"], generator=g)
    return attn, torch.tensor(LENS), keywords(B, SHAPES[shape]["keyword_classes_num"], 7 + which)


def forward_inputs(shape):
    """Teacher-forced eval call: words behind <start>, row 1 padded from position 3 on."""
    attn, lens, kw = infer_inputs(shape)
    g = torch.Generator().manual_seed(272)
    word = torch.randint(3, SHAPES[shape]["vocab_size"], (B, MAX_LENGTH), generator=g)
    word[:, 0] = START
    word[1, 3:] = PAD
    return {"word": word, "cap_padding_mask": word == PAD, "attn_emb": attn, "attn_emb_len": lens, "keyword": kw}


def train_inputs():
    """(cnn_attn (N, T', 2048), lens, keyword, cap (N, Tc), cap_len) of the training cases."""
    g = torch.Generator().manual_seed(273)
    attn = torch.randn(TRAIN_N, TRAIN_TQ, 2048, generator=g).abs() * 0.5
    cap = torch.randint(4, SHAPES["d256"]["vocab_size"], (TRAIN_N, TRAIN_TC), generator=g)
    cap[:, 0] = START
    for i, n in enumerate(TRAIN_CAP_LEN):
        cap[i, n - 1] = END
        cap[i, n:] = PAD
    return attn, torch.tensor(TRAIN_LENS), keywords(TRAIN_N, SHAPES["d256"]["keyword_classes_num"], 9), cap, \
        np.array(TRAIN_CAP_LEN)


# ---- the restatement ------------------------------------------------------------------------------------------------
def embed_rows(state, word, keyword, p=0.0, base_seed=0, row0=0, prefix="decoder."):
    """The decoder's input rows (N, L, d) for tokens ``word`` (N, L) and ``keyword`` (N, C)."""
    E = state[prefix + "word_embedding.weight"]
    d, dt = E.shape[1], E.dtype
    N, L = word.shape
    kwp = F.linear(keyword.to(dt), state[prefix + "keyword_proj.weight"], state[prefix + "keyword_proj.bias"])
    x = E[word] * OT._mask_t(OT.op_seed(base_seed, OT.OP_EMB_A), row0 * d, (N, L, d), p).to(dt)
    x = F.layer_norm(x * math.sqrt(d) + kwp[:, None, :], (d,), state[prefix + "word_keyword_norm.weight"],
                     state[prefix + "word_keyword_norm.bias"])
    x = x + state[prefix + "pos_encoder.pe"][:L, 0][None]
    return x * OT._mask_t(OT.op_seed(base_seed, OT.OP_EMB_B), row0 * d, (N, L, d), p).to(dt)


def decoder_pass(state, word, attn_emb, attn_emb_len, keyword, nlayers, nhead, p=0.0, base_seed=0, row0=0, mrow0=0, seq0=0,
                 pl=None, relu_gates=None, kink=OT.KINK, prefix="decoder."):
    """oracle.train_path.decoder_pass with ``embed_rows``; p = 0: the eval-mode forward.  Returns (N, L, d)."""
    d = state[prefix + "word_embedding.weight"].shape[1]
    dt = state[prefix + "word_embedding.weight"].dtype
    N, L = word.shape
    pl = L if pl is None else pl
    Tm = attn_emb.shape[1]
    a = OT._relu_at_kinks(F.linear(attn_emb.to(dt), state[prefix + "attn_proj.0.weight"], state[prefix + "attn_proj.0.bias"]),
                          relu_gates["mem"] if relu_gates else None, kink)
    a = a * OT._mask_t(OT.op_seed(base_seed, OT.OP_MEM), mrow0 * d, (N, Tm, d), p).to(dt)
    mem = F.layer_norm(a, (d,), state[prefix + "attn_proj.3.weight"], state[prefix + "attn_proj.3.bias"])
    x = embed_rows(state, word, keyword, p, base_seed, row0, prefix)
    neg = float("-inf")
    causal = torch.zeros(L, L, dtype=dt).masked_fill(torch.triu(torch.ones(L, L, dtype=torch.bool), 1), neg)
    self_mask = causal[None, None] + torch.zeros(N, 1, 1, L, dtype=dt).masked_fill((word == PAD)[:, None, None, :], neg)
    lens = torch.as_tensor(attn_emb_len)
    mem_mask = torch.zeros(N, 1, 1, Tm, dtype=dt).masked_fill(~(torch.arange(Tm)[None, :] < lens[:, None])[:, None, None, :],
                                                              neg)

    def rowmask(op, width=d):
        return OT._mask_t(OT.op_seed(base_seed, op), row0 * width, (N, L, width), p).to(dt)

    def pmask(op, ptk, tk):
        return OT._mask_t(OT.op_seed(base_seed, op), seq0 * nhead * pl * ptk, (N, nhead, pl, ptk), p)[:, :, :L, :tk].to(dt)

    for l in range(nlayers):
        lp = f"{prefix}model.layers.{l}."
        op = OT.OP_LAYER + 10 * l
        sa = OT._mha_train(x, x, x, state[lp + "self_attn.in_proj_weight"], state[lp + "self_attn.in_proj_bias"],
                           state[lp + "self_attn.out_proj.weight"], state[lp + "self_attn.out_proj.bias"], nhead,
                           self_mask, pmask(op + 0, pl, L))
        x = F.layer_norm(x + sa * rowmask(op + 1), (d,), state[lp + "norm1.weight"], state[lp + "norm1.bias"])
        ca = OT._mha_train(x, mem, mem, state[lp + "multihead_attn.in_proj_weight"],
                           state[lp + "multihead_attn.in_proj_bias"], state[lp + "multihead_attn.out_proj.weight"],
                           state[lp + "multihead_attn.out_proj.bias"], nhead, mem_mask, pmask(op + 2, Tm, Tm))
        x = F.layer_norm(x + ca * rowmask(op + 3), (d,), state[lp + "norm2.weight"], state[lp + "norm2.bias"])
        pre = F.linear(x, state[lp + "linear1.weight"], state[lp + "linear1.bias"])
        dm = rowmask(op + 4, pre.shape[-1])
        theirs = None
        if relu_gates:
            theirs = relu_gates["ffn"][l][row0:row0 + N * L].reshape(pre.shape).to(dt)
            theirs = torch.where(dm > 0, theirs, pre.detach())
        hdn = OT._relu_at_kinks(pre, theirs, kink) * dm
        ff = F.linear(hdn, state[lp + "linear2.weight"], state[lp + "linear2.bias"])
        x = F.layer_norm(x + ff * rowmask(op + 5), (d,), state[lp + "norm3.weight"], state[lp + "norm3.bias"])
    return x


def forward(state, word, attn_emb, attn_emb_len, keyword, shape):
    """The eval-mode full-sequence call -> {"embed", "logit"} (pads of ``word`` are the masked keys)."""
    x = decoder_pass(state, word, attn_emb, attn_emb_len, keyword, **oracle_kw(shape))
    return {"embed": x, "logit": F.linear(x, state["decoder.classifier.weight"])}


@contextlib.contextmanager
def _oracle_over(keyword):
    """oracle.cpu_path's searches call its module-level ``decoder_forward``: for the duration, the keyword forward with
    ``keyword`` (one row per decoder row, or one row repeated over the beams of a clip)."""
    plain = O.decoder_forward

    def fwd(state, word, attn_emb, attn_emb_len, cap_padding_mask=None, prefix="decoder.", nlayers=2, nhead=4):
        kw = keyword if keyword.shape[0] == word.shape[0] else keyword.expand(word.shape[0], -1)
        x = decoder_pass(state, word, attn_emb, attn_emb_len, kw, nlayers, nhead, prefix=prefix)
        return {"embed": x, "logit": F.linear(x, state[prefix + "classifier.weight"])}
    O.decoder_forward = fwd
    try:
        yield
    finally:
        O.decoder_forward = plain


def greedy(state, attn_emb, attn_emb_len, keyword, shape, max_length=MAX_LENGTH):
    dt = state["decoder.classifier.weight"].dtype
    with _oracle_over(keyword):
        return O.greedy_decode(state, attn_emb.to(dt), attn_emb_len, max_length, **oracle_kw(shape))


def beam_search(state, attn_emb, attn_emb_len, keyword, shape, beam, max_length=MAX_LENGTH, n_best=False, n_best_size=None,
                trace=None):
    """base.py:254-361 clip by clip (the reference repeats a clip's keyword row over its beams, transformer_model.py:255-264)."""
    dt = state["decoder.classifier.weight"].dtype
    lens = torch.as_tensor(attn_emb_len)
    seqs = []
    for i in range(attn_emb.shape[0]):
        with _oracle_over(keyword[i:i + 1]):
            out = O.beam_search(state, attn_emb[i:i + 1].to(dt), lens[i:i + 1], beam, max_length, 1.0, n_best=n_best,
                                n_best_size=n_best_size, trace=trace, **oracle_kw(shape))
        seqs.append(out["seq"])
    return {"seq": torch.cat(seqs, 0)}


def live_mask(seq):
    """(B, L) bool: the positions a greedy search ran while the row had not ended (its <end> included), up to the step
    after which no row of the batch was left."""
    seq = torch.as_tensor(seq)
    ended = (seq == END).long().cumsum(1) > 0
    live = torch.ones_like(ended)
    live[:, 1:] = ~ended[:, :-1]
    steps = int((~ended).any(0).long().sum()) + 1
    live[:, min(steps, seq.shape[1]):] = False
    return live


def train_forward(state, attn_emb, attn_emb_len, keyword, cap, use_cap, base_seed=0, p_dec=0.0, teacher_forcing=False,
                  relu_gates=None, kink=OT.KINK):
    """oracle.train_path.train_forward over ``decoder_pass``: logit (N, T, V), seq (N, T)."""
    N, Tc = cap.shape
    T = Tc - 1
    Tm = attn_emb.shape[1]
    cls = state["decoder.classifier.weight"]
    kw = dict(nlayers=2, nhead=4, p=p_dec, base_seed=base_seed, relu_gates=relu_gates, kink=kink)
    if teacher_forcing:
        x = decoder_pass(state, cap[:, :-1], attn_emb, attn_emb_len, keyword, pl=T, **kw)
        logit = F.linear(x, cls)
        return {"logit": logit, "seq": logit.argmax(-1)}
    seq = torch.zeros(N, T, dtype=torch.long)
    logits, row0 = [], 0
    for t in range(T):
        L = t + 1
        word = cap[:, :L] if use_cap[t] else torch.cat([torch.full((N, 1), START, dtype=torch.long), seq[:, :t]], dim=1)
        x = decoder_pass(state, word, attn_emb, attn_emb_len, keyword, row0=row0, mrow0=t * N * Tm, seq0=t * N, pl=T, **kw)
        logit_t = F.linear(x[:, -1], cls)
        seq[:, t] = logit_t.detach().argmax(-1)
        logits.append(logit_t)
        row0 += N * L
    return {"logit": torch.stack(logits, dim=1), "seq": seq}


def trainable_keys(state):
    return [k for k in state if k.startswith(("encoder.rnn.", "encoder.trm.", "decoder.")) and not k.endswith("pos_encoder.pe")]


def train_step_grads(state, cnn_attn, attn_len, keyword, cap, cap_len, use_cap, base_seed=0, p_dec=0.0, p_rnn=0.0,
                     smoothing=0.1, teacher_forcing=False, relu_gates=None, kink=OT.KINK, dtype=torch.float64):
    """Loss, logits, greedy tokens and the gradient of every trainable tensor for one batch, given the frozen Cnn14's
    output: the bi-GRU of tests/_attn_gru_train_ref.py (or, for a state with ``encoder.trm.`` tensors, the Transformer encoder of
    tests/_trm_train_ref.py without dropout), ``train_forward``, LabelSmoothingLoss; gradients by autograd."""
    keys = trainable_keys(state)
    st = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()}
    for k in keys:
        st[k] = st[k].detach().clone().requires_grad_(True)
    mem_len = torch.as_tensor(attn_len).long()
    if "encoder.trm.cls_token" in st:     # Cnn14TransformerEncoder: the cls row leads every clip's memory
        attn_emb = ET.encoder_train_forward(st, cnn_attn.to(dtype), attn_len, base_seed, 0.0)
        mem_len = mem_len + 1
    else:
        attn_emb, _ = AT.encoder_forward(st, cnn_attn.to(dtype), attn_len, p_rnn, base_seed)     # (dtype-generic bi-GRU)
    gates = None
    if relu_gates:
        gates = {"mem": relu_gates["mem"].to(dtype), "ffn": [g.to(dtype) for g in relu_gates["ffn"]]}
    out = train_forward(st, attn_emb, mem_len, keyword, cap, use_cap, base_seed, p_dec, teacher_forcing, gates, kink)
    loss = OT.label_smoothing_loss(out["logit"], cap[:, 1:], torch.as_tensor(cap_len) - 1, smoothing)
    grads = torch.autograd.grad(loss, [st[k] for k in keys], allow_unused=True)
    g = {k: (gr if gr is not None else torch.zeros_like(st[k])) for k, gr in zip(keys, grads)}
    return {"loss": loss.detach(), "logit": out["logit"].detach(), "seq": out["seq"], "grads": g}


def load_g27():
    return np.load(os.path.join(GOLDEN, "g27_keyword_trm.npz"))


def recipe(g27, name):
    seed, beta = g27[f"{name}_recipe"].tolist()
    return int(seed), float(beta)
