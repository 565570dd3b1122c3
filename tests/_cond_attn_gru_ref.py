"""CPU restatement in torch of the condition-controlled attention-GRU decoders (reference rnn_decoder.py:276-336
ConditionalBahAttnDecoder, :519-575 SpecificityBahAttnDecoder, attn_model.py:191-223 ConditionalSeq2SeqAttnModel) and of the
specificity loss (losses/loss.py:195-219), in float32 or float64, with autograd for the training step.

Both decoders are restated as what they are: a ``BahAttnCatFcDecoder`` with another third input.  ``as_catfc`` rewrites a
state dict and the clips' conditions into the tensors of that decoder, with torch operations, so that gradients flow back
to the real parameters, and the step, the searches and the training forward are those of tests/_attn_gru_ref.py and
tests/_attn_gru_train_ref.py:

  "cond"   fc_proj.weight = condition_embedding.weight^T (E, 2), fc_proj.bias = 0, fc_emb = [1 - c, c]:
           fc_proj(fc_emb) = (1 - c) W[0] + c W[1] = torch.matmul([[1 - c, c]], W), the reference's line 311-312
  "spec"   ctx_proj = the identity (A, A) with a zero bias (the reference's ``lambda x: x``; a product with the identity
           and a sum with zeros are exact in every float format), fc_proj.weight = [[1]], fc_emb = [c]: the GRU input is
           cat(embed, context, c), E + A + 1 wide

tests/test_cond_attn_gru_cpu.py holds all of it to what the reference's own classes computed
(tests/golden/g26_cond_attn_gru.npz, written by tests/golden/make_golden_cond_attn_gru.py).  The inputs of every fixture
case are rebuilt here from seeds; the fixture stores outputs only.
"""
import os

import numpy as np
import torch

import _attn_gru_ref as AR
import _attn_gru_train_ref as TR
from audiocaption_amd import procedural as P

START_IDX, END_IDX, PAD_IDX = TR.START_IDX, TR.END_IDX, TR.PAD_IDX
GOLDEN = TR.GOLDEN
KINDS = ("cond", "spec")
SHAPES = {
    # the specificity input is 97 wide: odd pitch, below one 64-column tile
    "tiny": dict(emb_dim=32, d_model=32, attn_size=32, attn_emb_dim=64, fc_emb_dim=32, vocab_size=61),
    "small": TR.SMALL,     # 225 wide, V no multiple of 4
    "pub": TR.PUB,         # 1025 wide
}
CONDS = [0.0, 1.0, 0.37, -2.5, 7.5]
RAGGED7 = [7, 5, 4, 2, 1]
# inference cases: name -> (shape, clips, frames, lengths, max_length, beam sizes)
INFER = {
    "tiny": ("tiny", 5, 7, RAGGED7, 6, (2, 3)),
    "small": ("small", 5, 70, TR.SMALL_LENS, 6, (3,)),
    "small65": ("small", 65, 7, [RAGGED7[i % 5] for i in range(65)], 6, ()),        # crosses the 64-row GEMM tile
    "small22": ("small", 22, 7, [RAGGED7[i % 5] for i in range(22)], 6, (3,)),      # beam 3: 66 rows
    "small1": ("small", 1, 7, [7], 1, (2,)),                                        # one clip, one step
    "pub": ("pub", 5, 7, RAGGED7, 6, (2,)),
}
# training cases of the decoder alone: name -> (shape, clips, frames, lengths, caption columns, cap_len)
TRAIN = {
    "tiny": ("tiny", 5, 7, RAGGED7, 7, [7, 5, 6, 3, 7]),
    "small": ("small", 5, 70, TR.SMALL_LENS, TR.SMALL_TC, TR.SMALL_CAP_LEN),
    "small65": ("small", 65, 7, [RAGGED7[i % 5] for i in range(65)], 2, [2] * 65),  # T = 1, 65 rows
}
ALPHA = 0.3     # the whole-model step's weight of the condition term


def conditions(n, shift=0):
    return torch.tensor([CONDS[(i + shift) % len(CONDS)] for i in range(n)], dtype=torch.float32)


def memory(name, B, Tm, A):
    seed = 1000 + sum(ord(c) for c in name)
    return torch.from_numpy(np.random.default_rng(seed).normal(0.0, 0.25, (B, Tm, A)).astype(np.float32))


def infer_inputs(name):
    shape, B, Tm, lens, L, beams = INFER[name]
    return memory(name, B, Tm, SHAPES[shape]["attn_emb_dim"]), torch.tensor(lens), conditions(B), L, beams


def train_inputs(name):
    shape, B, Tm, lens, tc, cap_len = TRAIN[name]
    cap, cap_len = TR.caption(B, tc, cap_len, SHAPES[shape]["vocab_size"], 12)
    return memory("train" + name, B, Tm, SHAPES[shape]["attn_emb_dim"]), torch.tensor(lens), conditions(B, 2), cap, cap_len


def state(kind, shape, seed, end_scale, prefix=""):
    return P.to_torch(P.cond_decoder_state(kind, prefix, seed=int(seed), end_scale=float(end_scale), **SHAPES[shape]))


def pub_state(kind, seed, end_scale):
    """encoder.rnn.* (3-layer bi-GRU, hidden 256) and decoder.* of the whole-model case."""
    sd = P.gru_state("encoder.rnn.", 2048, 256, 3, int(seed))
    sd.update(P.cond_decoder_state(kind, "decoder.", seed=int(seed), end_scale=float(end_scale), **TR.PUB))
    return P.to_torch(sd)


def word_specificity(V, seed=31):
    """Word specificities like the reference's table: non-negative, a few words far above the rest."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(V, generator=g) ** 4 * 3.0).float()


def load_g26():
    return dict(np.load(os.path.join(GOLDEN, "g26_cond_attn_gru.npz")))


# ---- the decoders as a BahAttnCatFcDecoder ---------------------------------------------------------------------------
def as_catfc(kind, sd, cond, dtype=None):
    """(state dict of the equivalent BahAttnCatFcDecoder, its fc_emb).  ``cond`` (N,) float32 values; ``dtype``: the
    arithmetic's (default: that of the state dict)."""
    dtype = dtype or sd["classifier.weight"].dtype
    out = {k: v.to(dtype) for k, v in sd.items() if k != "condition_embedding.weight"}
    c = torch.as_tensor(cond, dtype=torch.float32).to(dtype)
    E = sd["word_embedding.weight"].shape[1]
    if kind == "cond":
        out["fc_proj.weight"] = sd["condition_embedding.weight"].to(dtype).T
        out["fc_proj.bias"] = torch.zeros(E, dtype=dtype)
        return out, torch.stack((1 - c, c), dim=1)
    A = sd["attn.h2attn.weight"].shape[1] - sd["model.weight_hh_l0"].shape[1]
    out["ctx_proj.weight"], out["ctx_proj.bias"] = torch.eye(A, dtype=dtype), torch.zeros(A, dtype=dtype)
    out["fc_proj.weight"], out["fc_proj.bias"] = torch.ones(1, 1, dtype=dtype), torch.zeros(1, dtype=dtype)
    return out, c[:, None]


def step(kind, sd, embed, h, attn_emb, lens, cond):
    """One decoder step: (new state, logit, attention weights)."""
    cat, fc = as_catfc(kind, sd, cond, h.dtype)
    return AR.step(cat, embed, h, attn_emb, lens, fc)


def greedy(kind, sd, attn_emb, lens, cond, max_length, dtype=torch.float32, **kw):
    cat, fc = as_catfc(kind, sd, cond, dtype)
    return AR.greedy(cat, attn_emb, lens, fc, None, max_length, dtype=dtype, **kw)


def beam_search(kind, sd, attn_emb, lens, cond, beam_size, max_length, dtype=torch.float32, **kw):
    cat, fc = as_catfc(kind, sd, cond, dtype)
    return AR.beam_search(cat, attn_emb, lens, fc, None, beam_size, max_length, dtype=dtype, **kw)


# ---- the specificity loss ------------------------------------------------------------------------------------------------
def specificity_loss(logit, ws, tgt_len, conds, reduce="sum"):
    """The condition term of SpecificityLossWrapper (loss.py:207-217): MSE between the caption specificity - the sum, or
    the mean_with_lens, over t < tgt_len - 1 of softmax(logit) . ws - and ``conds``."""
    s = torch.softmax(logit, dim=-1) @ ws.to(logit.dtype)
    n = (torch.as_tensor(tgt_len) - 1).to(logit.device)
    mask = (torch.arange(logit.shape[1], device=logit.device)[None, :] < n[:, None]).to(logit.dtype)
    c = (s * mask).sum(1)
    if reduce != "sum":
        c = c / n.to(logit.dtype)
    return ((c - torch.as_tensor(conds).to(logit.dtype)) ** 2).mean()


def loss_terms(logit, cap, cap_len, ws=None, targets=None, reduce="sum", alpha=1.0, smoothing=0.1):
    """(loss, word_loss, condition_loss) of LabelSmoothingLoss(0.1), wrapped in SpecificityLossWrapper when ``ws`` is given."""
    tgt_len = torch.as_tensor(cap_len) - 1
    word = TR.label_smoothing_loss(logit, cap[:, 1:], tgt_len, smoothing)
    if ws is None:
        return word, word, torch.zeros((), dtype=logit.dtype)
    cl = specificity_loss(logit, ws, tgt_len, targets, reduce)
    return word + alpha * cl, word, cl


# ---- training ----------------------------------------------------------------------------------------------------------
def decoder_step_grads(kind, sd, attn_emb, lens, cond, cap, cap_len, use_cap, p=0.0, base_seed=0, dtype=torch.float32,
                       **loss_kw):
    """Loss and gradients of the decoder alone: every decoder tensor and attn_emb.  ``cond`` is data: no gradient."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    a = attn_emb.detach().to(dtype).clone().requires_grad_(True)
    cat, fc = as_catfc(kind, leaves, cond, dtype)
    out = TR.decoder_forward(cat, a, lens, fc, cap, use_cap, None, p, base_seed)
    loss, word, cl = loss_terms(out["logit"], cap, cap_len, **loss_kw)
    keys = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in keys] + [a])
    res = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    res.update(loss=loss.detach(), word_loss=word.detach(), condition_loss=cl.detach(), grads=dict(zip(keys, grads[:-1])),
               d_attn_emb=grads[-1])
    return res


def model_step_grads(kind, state_, cnn_attn, lens, cond, cap, cap_len, use_cap, dtype=torch.float32, **loss_kw):
    """Loss and gradients of the whole model: every encoder.rnn.* and decoder.* tensor."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state_.items()}
    attn_emb, _ = TR.encoder_forward(leaves, cnn_attn.to(dtype), lens)
    dec = {k[len("decoder."):]: v for k, v in leaves.items() if k.startswith("decoder.")}
    cat, fc = as_catfc(kind, dec, cond, dtype)
    out = TR.decoder_forward(cat, attn_emb, lens, fc, cap, use_cap, None)
    loss, word, cl = loss_terms(out["logit"], cap, cap_len, **loss_kw)
    keys = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in keys])
    res = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    res.update(loss=loss.detach(), word_loss=word.detach(), condition_loss=cl.detach(), grads=dict(zip(keys, grads)))
    return res


# ---- the loss alone: SpecificityLossWrapper over a stand-in word loss --------------------------------------------------
# (V, T, N, sentence_reduce, alpha): V 50 is below one wave; tgt_len - 1 reaches 0 ("sum" only), T and values in between
LOSS_GRID = [(V, T, N, reduce, (1.0, 0.3)[(i + j + k + m) % 2])
             for i, V in enumerate((50, 517, 4981)) for j, T in enumerate((1, 7)) for k, N in enumerate((1, 5))
             for m, reduce in enumerate(("sum", "mean"))]
_TGT_LEN = {(1, 1): [2], (1, 7): [8], (5, 1): [2, 1, 2, 2, 1], (5, 7): [8, 1, 4, 2, 6]}


def loss_case_name(case):
    V, T, N, reduce, alpha = case
    return f"V{V}_T{T}_N{N}_{reduce}"


def stand_in_word_loss(output):
    """A plain differentiable word loss for the loss-alone cases (LabelSmoothingLoss cannot take tgt_len = T + 1)."""
    return output["logit"].square().mean()


def loss_inputs(case):
    """(logit (N, T, V), tgt_len, conditions, word_specificity, sentence_reduce, alpha) of a LOSS_GRID case."""
    V, T, N, reduce, alpha = case
    g = torch.Generator().manual_seed(V + 10 * T + N)
    logit = torch.randn(N, T, V, generator=g) * 3.0
    tgt_len = torch.tensor(_TGT_LEN[(N, T)])
    if reduce != "sum":
        tgt_len = tgt_len.clamp(min=2)     # the mean divides by tgt_len - 1
    return logit, tgt_len, conditions(N, 1), word_specificity(V), reduce, alpha


# ---- fixture keys ----------------------------------------------------------------------------------------------------------
def infer_prefix(kind, name):
    shape = INFER[name][0]
    return f"{kind}_{shape}" if name == shape else f"{kind}_{shape}_{name}"


def recipe(g, kind, shape):
    return g[f"{kind}_{shape}_recipe"].tolist()
