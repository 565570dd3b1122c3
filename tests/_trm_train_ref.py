"""CPU restatement of the training step of the Cnn14-TransformerEncoder captioner (audiocaption_amd.train.TrainEngine
with ``model.encoder`` a Cnn14TransformerEncoder): the encoder in train mode in torch-CPU (float64 by default) with the
counter-hash dropout masks of csrc/train.hip, chained into oracle.train_path's decoder and loss; gradients by autograd.

What it restates (reference transformer_encoder.py:95-116, nn.TransformerEncoderLayer post-LN, ReLU):
  attn_proj: Linear -> ReLU -> dropout (OP_ENC_PROJ, indexed over the N*T' frame rows) -> LayerNorm;
  cls_token prepended to every clip (never dropped), key padding from attn_len + 1;
  per layer l, op = OP_ENC_LAYER + 10 l: self-attention with dropout on P (op + 0, P index ((n*nhead + h)*L + i)*L + j),
  dropout1 (op + 1) + add + norm1, linear1 -> ReLU -> dropout (op + 2) -> linear2, dropout2 (op + 3) + add + norm2.
The output is the decoder memory: Tm = T' + 1 rows per clip, attn_emb_len = attn_len + 1."""
import torch
import torch.nn.functional as F

from oracle import train_path as OT

OP_ENC_PROJ = 100
OP_ENC_LAYER = 110
PREFIX = "encoder.trm."


def encoder_train_forward(state, attn, attn_len, base_seed, p, nlayers=2, nhead=4, relu_gates=None, kink=OT.KINK,
                          prefix=PREFIX):
    """attn (N, T', 2048) -> (N, T' + 1, d).  relu_gates: optional {"proj": (N*T', d) ReLU outputs before dropout,
    "ffn": [per layer (N*(T'+1), F) after dropout]} of the implementation under test, consulted at ReLU kinks only
    (oracle.train_path._relu_at_kinks)."""
    N, Tq, _ = attn.shape
    cls = state[prefix + "cls_token"]
    d = cls.shape[0]
    L = Tq + 1
    dt = attn.dtype
    a = F.linear(attn, state[prefix + "attn_proj.0.weight"], state[prefix + "attn_proj.0.bias"])
    a = OT._relu_at_kinks(a, relu_gates["proj"] if relu_gates else None, kink)
    a = a * OT._mask_t(OT.op_seed(base_seed, OP_ENC_PROJ), 0, (N, Tq, d), p).to(dt)
    x = F.layer_norm(a, (d,), state[prefix + "attn_proj.3.weight"], state[prefix + "attn_proj.3.bias"])
    x = torch.cat([cls.reshape(1, 1, d).expand(N, 1, d), x], dim=1)
    lens = torch.as_tensor(attn_len).long() + 1
    mask_add = torch.zeros(N, 1, 1, L, dtype=dt).masked_fill((torch.arange(L)[None, :] >= lens[:, None])[:, None, None, :],
                                                             float("-inf"))

    def rowmask(op, width):
        return OT._mask_t(OT.op_seed(base_seed, op), 0, (N, L, width), p).to(dt)

    for l in range(nlayers):
        lp = f"{prefix}model.layers.{l}."
        op = OP_ENC_LAYER + 10 * l
        pm = OT._mask_t(OT.op_seed(base_seed, op), 0, (N, nhead, L, L), p).to(dt)
        sa = OT._mha_train(x, x, x, state[lp + "self_attn.in_proj_weight"], state[lp + "self_attn.in_proj_bias"],
                           state[lp + "self_attn.out_proj.weight"], state[lp + "self_attn.out_proj.bias"], nhead, mask_add,
                           pm)
        x = F.layer_norm(x + sa * rowmask(op + 1, d), (d,), state[lp + "norm1.weight"], state[lp + "norm1.bias"])
        pre = F.linear(x, state[lp + "linear1.weight"], state[lp + "linear1.bias"])
        dm = rowmask(op + 2, pre.shape[-1])
        theirs = None
        if relu_gates:
            theirs = relu_gates["ffn"][l].reshape(pre.shape).to(dt)
            theirs = torch.where(dm > 0, theirs, pre.detach())
        hdn = OT._relu_at_kinks(pre, theirs, kink) * dm
        ff = F.linear(hdn, state[lp + "linear2.weight"], state[lp + "linear2.bias"])
        x = F.layer_norm(x + ff * rowmask(op + 3, d), (d,), state[lp + "norm2.weight"], state[lp + "norm2.bias"])
    return x


def trainable_keys(state):
    return [k for k in state if k.startswith((PREFIX, "decoder.")) and not k.endswith("pos_encoder.pe")]


def train_step_grads(state, cnn_attn, attn_len, cap, cap_len, use_cap, base_seed=0, p_dec=0.2, p_enc=0.2,
                     smoothing=0.1, teacher_forcing=False, relu_gates=None, kink=OT.KINK, dtype=torch.float64):
    """Loss, logits, greedy tokens and gradients of one batch given the frozen Cnn14's output ``cnn_attn``
    (N, T', 2048).  relu_gates: {"proj", "ffn"} of the encoder (see ``encoder_train_forward``) and {"mem", "dec_ffn"}
    of the decoder (oracle.train_path.decoder_pass's "mem" / "ffn")."""
    keys = trainable_keys(state)
    st = {k: v.to(dtype) if v.is_floating_point() else v for k, v in state.items()}
    for k in keys:
        st[k] = st[k].detach().clone().requires_grad_(True)
    emb = encoder_train_forward(st, cnn_attn.to(dtype), attn_len, base_seed, p_enc, relu_gates=relu_gates, kink=kink)
    mem_len = torch.as_tensor(attn_len).long() + 1
    dec_gates = None
    if relu_gates:
        dec_gates = {"mem": relu_gates["mem"].to(dtype), "ffn": [g.to(dtype) for g in relu_gates["dec_ffn"]]}
    out = OT.train_forward(st, emb, mem_len, cap, use_cap, base_seed, p_dec, teacher_forcing=teacher_forcing,
                           relu_gates=dec_gates, kink=kink)
    loss = OT.label_smoothing_loss(out["logit"], cap[:, 1:], torch.as_tensor(cap_len) - 1, smoothing)
    grads = torch.autograd.grad(loss, [st[k] for k in keys], allow_unused=True)
    g = {k: (gr if gr is not None else torch.zeros_like(st[k])) for k, gr in zip(keys, grads)}
    return {"loss": loss.detach(), "logit": out["logit"].detach(), "seq": out["seq"], "grads": g,
            "attn_emb": emb.detach()}


# the step cases of the Transformer encoder: (clips, Cnn14 frames T', caption tokens, dropout seed); L = T' + 1
STEP_CASES = {
    "bench_10s": (32, 31, 22, 311),      # L 32
    "clotho_30s": (8, 94, 30, 317),      # L 95: beyond ac_attn_seq_bwd's LDS limit (L <= 91)
}


def step_batch(name):
    """(cnn_attn, attn_len, cap, cap_len, use_cap, seed) of a step case, drawn like tests/_train_ref.step_batch."""
    B, Tq, Tc, seed = STEP_CASES[name]
    g = torch.Generator().manual_seed(seed)
    cnn_attn = torch.randn(B, Tq, 2048, generator=g).abs() * 0.5
    attn_len = torch.randint(Tq // 2, Tq + 1, (B,), generator=g)
    attn_len[0], attn_len[1], attn_len[2] = Tq, 1, Tq - 1
    cap = torch.randint(4, 4981, (B, Tc), generator=g)
    cap_len = torch.randint(8, Tc + 1, (B,), generator=g)
    cap_len[0] = Tc
    cap[:, 0] = 1
    for i, n in enumerate(cap_len.tolist()):
        cap[i, n - 1] = 2
        cap[i, n:] = 0
    T = Tc - 1
    use_cap = [1] * T
    for t in (2, T // 2, T // 2 + 1, T - 1):
        use_cap[t] = 0
    return cnn_attn, attn_len, cap, cap_len.numpy(), use_cap, seed
