"""Self-critical sequence training (SCST) on the MI355X path.  Plugin-compatible with the reference class
``captioning.models.rl_model.ScstWrapper`` (rl_model.py:11-85) as its runner drives it (run.py:35-41,67-72,118-119: the
wrapper gets ``keys``, ``key2refs``, ``vocabulary`` and ``scorer`` and returns the loss itself).

The reference file is stale: it reads ``"seqs"``, ``"sampled_logprobs"`` and ``"raw_feats"``, which its ``CaptionModel`` no
longer produces (base.py:122-128 has ``"seq"`` and ``"sampled_logprob"``).  What it computes is restated here with the
current keys.  For ``mode == "train"``:

1. baseline: ``model.eval()``, no gradients, ``sample_method="greedy"`` - the inference path as it is - -> ``greedy_seqs``;
2. rollout: ``model.train()``, ``sample_method="sample"``: the train-mode encoder and ``max_length`` decoder passes on the
   words drawn so far (``TrainEngine.rollout``; for the attention-GRU models ``max_length`` steps of the GRU decoder, each
   on the word the step before drew, ``AttnGruTrainEngine.rollout``); a clip that has drawn ``<end>`` keeps emitting ``<end>``;
   ``sampled_logprob[n, t] = log_softmax(logit[n, t])[w] / temp``;
3. reward: ``score(sampled) - score(greedy)`` per clip.  With the built-in ``audiocaption_amd.Cider`` as ``scorer`` it is
   computed on the device from the word ids, both sets read where the decoders left them (cider.py ``score_ids``,
   csrc/cider.hip; its one upload is the batch's packed references), and feeds the loss kernel directly;
   any other scorer object goes through ``compute_batch_score`` on the host
   (``scorer.compute_score(references, hypothesis) -> (mean, per-key list)``) and one upload;
4. ``mask[n, 0] = 1``, ``mask[n, t] = (seq[n, t-1] != end_idx)``; ``loss = mean_n sum_t -(sampled_logprob * reward[n] *
   mask)`` - one kernel (csrc/scst.hip ac_scst_loss), whose backward hands d(loss)/d(logit) to the training engine's
   bridge node, so ``loss.backward()`` fills ``.grad`` of every trainable parameter;
5. output ``{"greedy_seqs", "sampled_seqs", "reward", "score", "loss"}``; the model is left in ``train()`` mode.

``ScstWrapper(model, n_rollouts=K, baseline="greedy" | "mean")`` (K in 1..8; the defaults are the recipe above, launch for
launch) is the multi-rollout form (Luo 2020, "A Better Variant of Self-Critical Sequence Training"), for ``TransformerModel``:

* K rollouts per clip from ONE train-mode encoder pass: the decoder runs over J = K*N rollout rows, row j = k*N + n on clip
  n's audio memory (``TrainEngine.rollout(input_dict, n_rollouts=K)``);
* ``baseline="mean"``: the baseline of a rollout is the mean score of the clip's other K - 1 rollouts - no greedy decode, no
  ``eval()`` switch, no ``greedy_seqs``; ``baseline="greedy"``: step 1 above, one greedy caption per clip;
* scores: the built-in ``Cider`` reads the K row blocks of the rollout's words (and the greedy words) on the device, at most
  ``cider.MAX_SETS`` hypothesis sets per ``score_ids`` call; any other scorer gets one ``compute_batch_score`` per set on
  the host (clips sharing a key are scored once within a set, never across rollouts) and one upload of all the scores;
* reward on the device (csrc/scst.hip ac_scst_group_reward), f32, sums in the order j = 0..K-1:
  greedy ``r[k, n] = s[k, n] - g[n]``, mean ``r[k, n] = s[k, n] - (sum_j s[j, n] - s[k, n]) / (K - 1)``;
* the loss kernel over the J rows with ``reward`` (J,): ``loss = mean_j sum_t -(sampled_logprob * reward * mask)``; the
  backward sums the K rollouts' gradients into clip n's audio memory;
* output ``sampled_seqs`` (N, K, T), ``reward`` and ``score`` (N, K), ``loss``, and ``greedy_seqs`` (N, T) with the greedy
  baseline only.

The wrapped model is a ``TransformerModel``, or a ``Seq2SeqAttnModel`` / ``TemporalSeq2SeqAttnModel`` over a ``CrnnEncoder``
(``temporal_tag`` then goes to both the baseline and the rollout).  Any other mode is forwarded to the wrapped model.
The caller's ``input_dict`` is not modified (the reference overwrites its ``mode`` and ``sample_method``).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import logit_rules
from ._lib import check, ptr, stream
from .cider import Cider
from .transformer_model import CaptionMetaMixin, KeywordCondTransformerModel, TransformerModel


def compute_batch_score(decode_res, key2refs, keys, start_idx, end_idx, vocabulary, scorer):
    """Per-clip scores (N,) of the decoded words ``decode_res`` (N, max_length) - model_util.py:117-164.  A clip's
    sentence is its words up to the first ``end_idx`` (``start_idx`` skipped) joined through ``vocabulary.idx2word``; clips
    that share a key are scored once, with the first one's sentence."""
    if scorer is None:
        raise ValueError("compute_batch_score: a scorer is required (no CIDEr scorer is built in)")
    decode_res = np.asarray(decode_res)
    hypothesis, references = {}, {}
    for row, key in zip(decode_res, keys):
        if key in hypothesis:
            continue
        words = []
        for w in row.tolist():
            if w == end_idx:
                break
            if w != start_idx:
                words.append(vocabulary.idx2word[w])
        hypothesis[key] = [" ".join(words)]
        references[key] = key2refs[key]
    _, per_key = scorer.compute_score(references, hypothesis)
    by_key = dict(zip(references.keys(), per_key))
    return np.array([by_key[key] for key in keys[:decode_res.shape[0]]], dtype=np.float64)


def _launch(logit, seq, reward, temp, end_idx, dlogit, gscale_dev):
    N, T, V = logit.shape
    row_loss = torch.empty(N * T, device=logit.device, dtype=torch.float32)
    loss = torch.empty(1, device=logit.device, dtype=torch.float32)
    check(_lib.load().ac_scst_loss(ptr(logit), ptr(seq), seq.stride(0), ptr(reward), float(temp), int(end_idx), N, T, V,
                                   ptr(row_loss), ptr(loss), ptr(dlogit), ptr(gscale_dev), stream()), "ac_scst_loss")
    return loss, row_loss


class _ScstLossFn(torch.autograd.Function):
    """loss = mean_n sum_t -(log_softmax(logit)[seq] / temp * reward[n] * mask) and its gradient, both by ac_scst_loss."""

    @staticmethod
    def forward(ctx, logit, seq, reward, temp, end_idx):
        loss, _ = _launch(logit, seq, reward, temp, end_idx, None, None)
        ctx.save_for_backward(logit, seq, reward)
        ctx.args = (temp, end_idx)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        logit, seq, reward = ctx.saved_tensors
        dlogit = torch.empty_like(logit)
        g = grad_out.reshape(1).to(device=logit.device, dtype=torch.float32)
        _launch(logit, seq, reward, *ctx.args, dlogit, g)
        return dlogit, None, None, None, None


def scst_loss(logit, seq, reward, temp, end_idx):
    """The SCST loss of sampled words ``seq`` (N, T) int32 under ``logit`` (N, T, V) and per-clip ``reward`` (N,)."""
    if logit.dim() != 3:
        raise ValueError("logit must be (batch, length, classes)")
    if logit.dtype != torch.float32 or not logit.is_contiguous():
        logit = logit.float().contiguous()
    seq = seq.to(device=logit.device, dtype=torch.int32)
    if seq.stride(1) != 1:
        seq = seq.contiguous()
    reward = torch.as_tensor(reward).to(device=logit.device, dtype=torch.float32).contiguous()
    return _ScstLossFn.apply(logit, seq, reward, float(temp), int(end_idx))


MAX_ROLLOUTS = 8       # include/audiocaption_hip.h AC_SCST_MAX_ROLLOUTS
BASELINES = ("greedy", "mean")      # AC_SCST_BASELINE_GREEDY, AC_SCST_BASELINE_MEAN


def group_reward(scores, mode, greedy_scores=None):
    """``reward`` (K*N,) f32 on the device of ``scores`` (K, N) f32: csrc/scst.hip ac_scst_group_reward."""
    K, N = scores.shape
    scores = scores.float().contiguous()
    if greedy_scores is not None:
        greedy_scores = greedy_scores.to(device=scores.device, dtype=torch.float32).contiguous()
    reward = torch.empty(K * N, device=scores.device, dtype=torch.float32)
    check(_lib.load().ac_scst_group_reward(ptr(scores), K, N, BASELINES.index(mode), ptr(greedy_scores), ptr(reward),
                                           stream()), "ac_scst_group_reward")
    return reward


class ScstWrapper(nn.Module, CaptionMetaMixin):

    def __init__(self, model, n_rollouts=1, baseline="greedy"):
        super().__init__()
        if isinstance(n_rollouts, bool) or not isinstance(n_rollouts, int) or not 1 <= n_rollouts <= MAX_ROLLOUTS:
            raise ValueError(f"ScstWrapper: n_rollouts must be an int in 1..{MAX_ROLLOUTS}, got {n_rollouts!r}")
        if baseline not in BASELINES:
            raise ValueError(f"ScstWrapper: baseline must be 'greedy' or 'mean', got {baseline!r}")
        if baseline == "mean" and n_rollouts < 2:
            raise ValueError("ScstWrapper: baseline='mean' is the mean score of a clip's OTHER rollouts; it needs n_rollouts >= 2")
        from .attn_model import ConditionalSeq2SeqAttnModel, Seq2SeqAttnModel
        from .crnn_trm_encoder import CrnnEncoder
        if isinstance(model, ConditionalSeq2SeqAttnModel):
            raise NotImplementedError("ScstWrapper: self-critical training is not built for ConditionalSeq2SeqAttnModel (the "
                                      "condition-controlled decoders have no sampled rollout)")
        if isinstance(model, KeywordCondTransformerModel):
            raise NotImplementedError("ScstWrapper: self-critical training is not built for KeywordCondTransformerModel (the "
                                      "keyword-conditioned decoder has no sampled rollout)")
        self._attn_gru = isinstance(model, Seq2SeqAttnModel) and isinstance(model.encoder, CrnnEncoder)
        if not (isinstance(model, TransformerModel) or self._attn_gru):
            over = f" over {model.encoder.__class__.__name__}" if isinstance(model, Seq2SeqAttnModel) else ""
            raise NotImplementedError(f"ScstWrapper: the wrapped model must be a TransformerModel, or a Seq2SeqAttnModel / "
                                      f"TemporalSeq2SeqAttnModel over a CrnnEncoder (the HIP training engines' rollouts), "
                                      f"got {model.__class__.__name__}{over}")
        if self._attn_gru and (n_rollouts > 1 or baseline == "mean"):
            raise NotImplementedError("ScstWrapper: n_rollouts > 1 and baseline='mean' (several rollouts per clip from one "
                                      "encoder pass) are built for TransformerModel; the attention-GRU engines draw one "
                                      "rollout per clip against the greedy baseline")
        self.model = model
        self.n_rollouts, self.baseline = n_rollouts, baseline

    def forward(self, input_dict):
        if input_dict["mode"] == "train":
            return self.scst(input_dict)
        return self.model(input_dict)

    def _baseline(self, input_dict, max_length):
        """The greedy baseline: the inference path in eval mode without gradients.  Returns its words as the inference
        path hands them out (CPU, int64) and the decoder's device copy of them as int32."""
        model = self.model
        # (the rollout and the baseline stay unconstrained: the repetition and word constraints are not part of the policy)
        d = {k: v for k, v in input_dict.items()
             if k not in ("seed", "dropout_seed", "_scst_words", "_cnn_attn") + logit_rules.KEYS}
        d.update(mode="inference", sample_method="greedy", max_length=max_length, _seq_on_device=True)
        model.eval()
        with torch.no_grad():
            hook = input_dict.get("_cnn_attn")
            if hook is None:
                res = model(d)
            else:
                # parity hook (see TrainEngine._prepare): start downstream of the mel front-end and the Cnn14
                from .cnn_encoder import cnn14_feat_len
                enc = model.encoder
                lens = cnn14_feat_len(input_dict["wav_len"], enc.cnn.hop_length, enc.cnn.downsample_ratio)
                back = enc.rnn if hasattr(enc, "rnn") else enc.trm
                res = model.forward_decoder(d, back({"attn": hook, "attn_len": lens}))
            return res["seq"], res["seq_dev"].to(torch.int32)      # (a copy: the decoder reuses its buffer)

    def scst(self, input_dict):
        from .train import _TrainBridge
        model = self.model
        if input_dict.get("n_samples") is not None:
            from .transformer_model import N_SAMPLES
            raise NotImplementedError(f"ScstWrapper: {N_SAMPLES} is not built for the SCST rollout; several rollouts per "
                                      "clip at training time are the constructor argument n_rollouts")
        for k in ("keys", "key2refs", "vocabulary", "scorer"):
            if input_dict.get(k) is None:
                raise ValueError(f"ScstWrapper: input_dict[{k!r}] is required for mode 'train' (run.py:35-41)")
        temp = float(input_dict.get("temp", 1.0))
        if not (math.isfinite(temp) and temp > 0):
            raise ValueError(f"ScstWrapper: temp must be finite and > 0, got {temp}")
        method = input_dict.get("sample_method", "sample")
        if method != "sample":
            raise NotImplementedError(f"ScstWrapper: the rollout draws with plain sampling ('sample'), not {method!r}")
        max_length = int(input_dict.get("max_length", model.max_length))
        engine = getattr(model, "_train_engine", None)
        if engine is None:     # (raises for an encoder the engine is not built for)
            if self._attn_gru:
                from .train_attn_gru import AttnGruTrainEngine
                engine = model._train_engine = AttnGruTrainEngine(model)
            else:
                from .train import TrainEngine
                engine = model._train_engine = TrainEngine(model)
        keys = list(input_dict["keys"])
        if self.n_rollouts > 1 or self.baseline == "mean":
            return self._scst_multi(input_dict, engine, keys, max_length, temp)

        greedy, greedy_i32 = self._baseline(input_dict, max_length)
        model.train()
        out = engine.rollout(dict(input_dict, max_length=max_length, temp=temp))

        if isinstance(input_dict["scorer"], Cider):
            # the built-in scorer reads both sets of words where they are, on the device; the packed references of the
            # batch are its one upload.  Reward and loss are launched back to back, the downloads follow.
            res = input_dict["scorer"].score_ids(input_dict["key2refs"], input_dict["vocabulary"], model.vocab_size, keys,
                                                 (out["seq_i32"], greedy_i32), model.start_idx, model.end_idx)
            logit = out["logit"]
            if torch.is_grad_enabled():
                logit = _TrainBridge.apply(engine, logit, *engine.flat.params)
            loss = scst_loss(logit, out["seq_i32"], res["reward"], temp, model.end_idx)
            return {"greedy_seqs": torch.as_tensor(greedy).cpu(), "sampled_seqs": out["seq"].cpu(),
                    "reward": res["reward"].cpu().double(), "score": res["scores"][0].cpu().double(), "loss": loss}

        sampled = out["seq"].cpu()
        greedy = torch.as_tensor(greedy).cpu()

        score = {}
        for name, seqs in (("sampled", sampled), ("greedy", greedy)):
            score[name] = compute_batch_score(seqs.numpy(), input_dict["key2refs"], keys, model.start_idx, model.end_idx,
                                              input_dict["vocabulary"], input_dict["scorer"])
        reward = score["sampled"] - score["greedy"]
        reward_dev = torch.from_numpy(reward.astype(np.float32)).to(out["logit"].device)     # the one upload

        logit = out["logit"]
        if torch.is_grad_enabled():
            logit = _TrainBridge.apply(engine, logit, *engine.flat.params)
        loss = scst_loss(logit, out["seq_i32"], reward_dev, temp, model.end_idx)
        return {"greedy_seqs": greedy, "sampled_seqs": sampled, "reward": torch.as_tensor(reward),
                "score": torch.as_tensor(score["sampled"]), "loss": loss}

    def _scst_multi(self, input_dict, engine, keys, max_length, temp):
        """K rollouts per clip from one encoder pass, against the greedy caption or the mean of the clip's other rollouts
        (the module's docstring)."""
        from .cider import MAX_SETS
        from .train import _TrainBridge
        model, K, mean = self.model, self.n_rollouts, self.baseline == "mean"
        N = len(keys)
        greedy = greedy_i32 = None
        if not mean:
            greedy, greedy_i32 = self._baseline(input_dict, max_length)
        model.train()
        out = engine.rollout(dict(input_dict, max_length=max_length, temp=temp), n_rollouts=K)
        seq_i32 = out["seq_i32"]                      # (J, T), row j = k*N + n
        if seq_i32.shape[0] != K * N:
            raise ValueError(f"ScstWrapper: {N} keys for a batch of {seq_i32.shape[0] // K} clips")
        T = seq_i32.shape[1]
        sets = [seq_i32[k * N:(k + 1) * N] for k in range(K)] + ([] if mean else [greedy_i32])
        if isinstance(input_dict["scorer"], Cider):
            # on the device, where the decoders left the words: at most MAX_SETS hypothesis sets per call (each call's one
            # upload is the batch's packed references); nothing is downloaded before the loss is launched
            rows = []
            for i in range(0, len(sets), MAX_SETS):
                res = input_dict["scorer"].score_ids(input_dict["key2refs"], input_dict["vocabulary"], model.vocab_size, keys,
                                                     tuple(sets[i:i + MAX_SETS]), model.start_idx, model.end_idx)
                rows.append(res["scores"])
            all_scores = rows[0] if len(rows) == 1 else torch.cat(rows, 0)
        else:
            host = np.stack([compute_batch_score(w.cpu().numpy(), input_dict["key2refs"], keys, model.start_idx, model.end_idx,
                                                 input_dict["vocabulary"], input_dict["scorer"]) for w in sets])
            all_scores = torch.from_numpy(host.astype(np.float32)).to(seq_i32.device)          # the one upload
        scores = all_scores[:K]
        reward = group_reward(scores, self.baseline, None if mean else all_scores[K])
        logit = out["logit"]
        if torch.is_grad_enabled():
            logit = _TrainBridge.apply(engine, logit, *engine.flat.params)
        loss = scst_loss(logit, seq_i32, reward, temp, model.end_idx)
        res = {"sampled_seqs": out["seq"].view(K, N, T).transpose(0, 1).contiguous().cpu(),
               "reward": reward.view(K, N).t().contiguous().cpu().double(),
               "score": scores.t().contiguous().cpu().double(), "loss": loss}
        if not mean:
            res["greedy_seqs"] = torch.as_tensor(greedy).cpu()
        return res
