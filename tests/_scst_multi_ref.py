"""CPU restatement of multi-rollout self-critical sequence training (ScstWrapper(model, n_rollouts=K, baseline=...),
TrainEngine.rollout(input_dict, n_rollouts=K)), built on tests/_scst_ref.py: the rollout is that file's on a decoder batch of
J = K*N clips over the train-mode encoder output of the N clips repeated K times (row j = k*N + n), so the decoder's row
space, its dropout-mask element indices and the sampler's counters are those of a batch of J clips while the encoder sites
keep the indices of a batch of N; the rewards of a clip's K rollouts are computed in float64."""
import numpy as np
import torch
import torch.nn.functional as F

import _sampling_ref as SR
import _scst_ref as SC
from oracle import train_path as OT


def rows_of(words):
    """(N, K, T) -> (K*N, T), row j = k*N + n."""
    words = torch.as_tensor(words)
    N, K, T = words.shape
    return words.permute(1, 0, 2).reshape(K * N, T)


def clips_of(rows, K):
    """(K*N, ...) with row j = k*N + n -> (N, K, ...)."""
    rows = torch.as_tensor(rows)
    return rows.reshape((K, rows.shape[0] // K) + tuple(rows.shape[1:])).transpose(0, 1)


def group_reward(scores, mode, greedy=None):
    """float64 rewards (K, N) of ``scores`` (K, N): "greedy" s[k, n] - g[n]; "mean" s[k, n] - (sum_j s[j, n] - s[k, n]) /
    (K - 1), the leave-one-out mean of the clip's other rollouts."""
    s = np.asarray(scores, dtype=np.float64)
    K = s.shape[0]
    if mode == "greedy":
        return s - np.asarray(greedy, dtype=np.float64)[None, :]
    assert mode == "mean" and K >= 2
    return s - (s.sum(0, keepdims=True) - s) / (K - 1)


def group_reward_f32(scores, mode, greedy=None):
    """The same in float32 arithmetic with the sum taken once in the order j = 0 .. K-1: what the kernel is specified to
    evaluate (tests allow it 1 ulp)."""
    s = np.asarray(scores, dtype=np.float32)
    K = s.shape[0]
    if mode == "greedy":
        return s - np.asarray(greedy, dtype=np.float32)[None, :]
    total = np.zeros(s.shape[1], dtype=np.float32)
    for j in range(K):
        total = total + s[j]
    return s - (total[None, :] - s) / np.float32(K - 1)


def rollout(state, cnn_attn, attn_len, T, K, temp=1.0, sample_seed=0, base_seed=0, p_dec=0.0, p_enc=0.0, words=None,
            enc_kind="rnn", relu_gates=None, kink=OT.KINK, tol=1e-6):
    """_scst_ref.rollout with the decoder on J = K*N rows.  ``words`` (N, K, T) forced words; ``relu_gates["mem"]`` is the
    implementation's (N*Tm, d) activation (shared by a clip's rollouts).  Returns logit (J, T, V), seq (J, T), ok (the
    sampler's admissible words per step and row j), and the state / keys the logits are differentiable in; the encoder's
    tensors receive the sum of the K rollouts' gradients through the repeat."""
    keys = SC._trainable(state, enc_kind)
    st = dict(state)
    for k in keys:
        st[k] = state[k].detach().clone().requires_grad_(True)
    dec_gates = None
    if relu_gates:
        dec_gates = {"mem": torch.as_tensor(relu_gates["mem"]).repeat(K, 1),
                     "ffn": relu_gates["dec_ffn" if enc_kind == "trm" else "ffn"]}
    emb, mem_len = SC._encode(st, cnn_attn, attn_len, base_seed, p_enc, enc_kind, relu_gates, kink)
    N, Tm = emb.shape[:2]
    J = K * N
    emb, mem_len = emb.repeat(K, 1, 1), mem_len.repeat(K)
    if words is not None:
        seq = SC.finished_rule(rows_of(words))
        cap = torch.cat([torch.full((J, 1), SC.START, dtype=torch.long), seq.long()], 1)
        out = OT.train_forward(st, emb, mem_len, cap, [1] * T, base_seed, p_dec, relu_gates=dec_gates, kink=kink)
        return {"logit": out["logit"], "seq": seq, "ok": None, "state": st, "keys": keys}
    seq = torch.full((J, T), SC.END, dtype=torch.long)
    oks, logits, row0 = [], [], 0
    done = torch.zeros(J, dtype=torch.bool)
    cls = st["decoder.classifier.weight"]
    for t in range(T):
        L = t + 1
        word = torch.cat([torch.full((J, 1), SC.START, dtype=torch.long), seq[:, :t]], 1)
        x = OT.decoder_pass(st, word, emb, mem_len, SC.PAD, base_seed, p_dec, row0, t * J * Tm, t * J, T, "decoder.",
                            relu_gates=dec_gates, kink=kink)
        logit_t = F.linear(x[:, -1], cls)
        w, _, ok, _ = SR.sample_rows(logit_t.detach().numpy(), SR.PLAIN, temp=temp, seed=sample_seed, step=t,
                                     rows=np.arange(J), tol=tol)
        w = torch.from_numpy(w).long()
        oks.append(ok)
        seq[:, t] = torch.where(done, torch.full_like(w, SC.END), w)
        done |= seq[:, t] == SC.END
        logits.append(logit_t)
        row0 += J * L
    return {"logit": torch.stack(logits, 1), "seq": seq, "ok": oks, "state": st, "keys": keys}


def scst_grads(ro, reward, temp):
    """Loss (the mean over the J rows), its scale and every trainable tensor's gradient; ``reward`` (J,)."""
    return SC.scst_grads(ro, reward, temp)
