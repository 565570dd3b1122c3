"""Attention-GRU captioning models, MI355X path.  Plugin-compatible with the reference classes ``Seq2SeqAttnModel``
(captioning/models/attn_model.py:10-190) and ``TemporalSeq2SeqAttnModel`` (hf_wrapper.py:1557-1788) for
``mode="inference"``: the same input keys and the outputs ``seq`` (int64, CPU), ``logit``, ``sampled_logprob`` (CPU),
``embed``, ``attn_weight`` (B, Tm, max_length), ``state`` (1, B, d_model; greedy and sampled search) plus the encoder's.

Greedy and sampled search run in one C call on the device.  Beam search batches ALL clips and beams into one decoder
step per step (the reference loops over clips, base.py:266) with the per-clip bookkeeping on the device.

Finished rows follow this package's contract: after a row's first <end> its ``seq`` columns are <end> and its
``sampled_logprob``, ``logit``, ``embed`` and ``attn_weight`` columns are 0; the search stops once every row has ended.  The
reference leaves ``torch.empty`` garbage in the ``attn_weight`` columns it never writes; here they are 0.

Two quirks of the reference's beam search are kept:

* a clip's ``attn_weight`` is that of beam row 0 after the last reorder (``beamsearch_process``, hf_wrapper.py:1671-1674),
  not that of the best-scoring finished beam;
* a clip exits early when its finished count EQUALS ``beam_size`` (base.py:318-323) - a clip that finishes two beams in the
  step that takes it past ``beam_size`` searches on to ``max_length``.

``mode="train"`` over a ``CrnnEncoder`` (``freeze_cnn=True``, ``freeze_cnn_bn=True``, GRU hidden 256) runs the reference's
scheduled-sampling forward (base.py:131-208 with attn_model.py:34-65; one ``random.random()`` per step, every step run,
``seq`` the arg-max of every step) through ``train_attn_gru.AttnGruTrainEngine`` and returns ``seq`` and
``sampled_logprob`` (CPU), ``logit`` (N, T, V) attached to autograd by one bridge node, ``embed``, ``attn_weight``
(N, Tm, T), ``state`` and the encoder's ``attn_emb_len``; in ``eval()`` or under ``no_grad`` the logits are plain tensors.

Self-critical sequence training: ``rl_model.ScstWrapper`` wraps these models over a ``CrnnEncoder``.  Its greedy baseline is
this file's greedy search (with ``_seq_on_device`` the result also carries ``seq_dev``, the decoder's device copy of the
words); its sampled rollout is ``AttnGruTrainEngine.rollout``.

``ConditionalSeq2SeqAttnModel`` (attn_model.py:191-223) over a ``ConditionalBahAttnDecoder`` or a
``SpecificityBahAttnDecoder``: ``input_dict["condition"]`` holds one float per clip (required; any finite value) and goes
once per batch into the decoder's ``memory`` - the beam rows of a clip share it.  Greedy, sampled and beam search and
``mode="train"`` as above; ``ScstWrapper``, ``EnsembleModel`` membership, ``dbs`` and ``forward_async`` are refused.

Not on this path (NotImplementedError): ``sample_method="dbs"`` (the reference's own diverse beam search raises for both
attention models), ``mode="train"`` and SCST over any other encoder, ``forward_async``, the fused ``TrainEngine.step`` and
knowledge distillation for these models; ``EnsembleModel`` takes ``TransformerModel`` members only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import search_state
from ._lib import check, ptr, stream
from .rnn_decoder import (BahAttnCatFcDecoder, ConditionalBahAttnDecoder, SpecificityBahAttnDecoder, TemporalBahAttnDecoder,
                          check_condition, check_temporal_tag)
from .transformer_model import CaptionModel
from . import kernels as K


class Seq2SeqAttnModel(CaptionModel):

    compatible_decoders = (BahAttnCatFcDecoder,)

    def __init__(self, encoder, decoder, **kwargs):
        super().__init__(encoder, decoder, **kwargs)
        if decoder.n_tags and not isinstance(self, TemporalSeq2SeqAttnModel):
            raise NotImplementedError("a TemporalBahAttnDecoder needs temporal_tag: wrap it in TemporalSeq2SeqAttnModel")
        if decoder.variant and not isinstance(self, ConditionalSeq2SeqAttnModel):
            raise NotImplementedError(f"a {type(decoder).__name__} needs condition: wrap it in ConditionalSeq2SeqAttnModel")

    def forward(self, input_dict):
        if input_dict["mode"] == "train":
            # the whole training forward (frozen Cnn14, bi-GRU, scheduled-sampling decoder) is one engine call; ``logit``
            # comes back attached to autograd by a single bridge node (audiocaption_amd/train_attn_gru.py)
            from .train_attn_gru import train_forward
            return train_forward(self, input_dict)
        return super().forward(input_dict)

    def forward_async(self, input_dict, pair=None):
        raise NotImplementedError(f"{type(self).__name__}: forward_async covers TransformerModel only; use model(input_dict)")

    def _inference_dict(self, input_dict, encoder_output_dict):
        forward_dict = {"mode": "inference", "sample_method": input_dict.get("sample_method", "greedy"),
                        "max_length": input_dict.get("max_length", self.max_length), "temp": input_dict.get("temp", 1.0)}
        if forward_dict["sample_method"] == "beam":
            forward_dict["beam_size"] = input_dict.get("beam_size", 3)
            forward_dict["n_best"] = input_dict.get("n_best", False)
            forward_dict["n_best_size"] = input_dict.get("n_best_size", forward_dict["beam_size"])
        if input_dict.get("seed") is not None:
            forward_dict["seed"] = input_dict["seed"]
        if input_dict.get("_seq_on_device"):      # ScstWrapper's baseline: the device copy of the words as well ("seq_dev")
            forward_dict["_seq_on_device"] = True
        forward_dict.update(encoder_output_dict)
        return forward_dict

    def inference_forward(self, input_dict):
        if input_dict["sample_method"] == "dbs":
            raise NotImplementedError("sample_method='dbs': diverse beam search is not on the HIP path (the reference's own "
                                      "dbs_process_step drops the attention weights, hf_wrapper.py:1730-1733)")
        return super().inference_forward(input_dict)

    def _tags(self, input_dict, B):
        """The clips' temporal tags, validated, on the host (None: the decoder takes none)."""
        return None

    def _side(self, input_dict):
        """What the decoder's ``memory`` takes next to the audio memory."""
        return input_dict["fc_emb"]

    # ---- greedy / sampling (base.py:152-218 with attn_model.py:60-92) -----------------------------------------
    def _stepwise(self, input_dict, sampler=None):
        dec = self.decoder
        attn_emb = input_dict["attn_emb"]
        tags = self._tags(input_dict, attn_emb.shape[0])
        mem = dec.memory(attn_emb, self._side(input_dict), input_dict["attn_emb_len"], 1, int(input_dict["max_length"]))
        if tags is not None:
            tags = K.upload(tags, attn_emb.device, torch.int32)
        if sampler is None:
            res = dec.greedy(mem, tags, self.start_idx, self.end_idx, self.pad_idx)
        else:
            res = dec.sample(mem, tags, self.start_idx, self.end_idx, self.pad_idx, *sampler)
        if input_dict.get("_seq_on_device"):
            res["seq_dev"] = res["seq"]                          # the words where the decoder left them (int64)
        res["seq"] = res["seq"].cpu()                            # the reference keeps seq on the CPU (base.py:122)
        res["sampled_logprob"] = res["sampled_logprob"].cpu()    # CPU as in base.py:126
        return res

    def greedy_search(self, input_dict):
        return self._stepwise(input_dict)

    def sample_search(self, input_dict):
        """Temperature / top-k / top-p / Gumbel sampling with ``TransformerModel.sample_search``'s rules and ``seed``."""
        from .sampling import draw_seed, parse_sample_method
        method, k, top_p, temp = parse_sample_method(input_dict["sample_method"], self.vocab_size, input_dict.get("temp", 1.0))
        seed = input_dict.get("seed")
        seed = draw_seed() if seed is None else int(seed)
        return self._stepwise(input_dict, (method, k, top_p, temp, seed))

    # ---- beam search (base.py:254-361 with attn_model.py:94-150), all clips batched ---------------------------
    def beam_search(self, input_dict):
        dec = self.decoder
        lib = _lib.load()
        attn_emb = input_dict["attn_emb"]
        dev = attn_emb.device
        B, Tm, _ = attn_emb.shape
        beam, L, temp = int(input_dict["beam_size"]), int(input_dict["max_length"]), float(input_dict["temp"])
        n_best, n_best_size = bool(input_dict.get("n_best", False)), int(input_dict.get("n_best_size", beam))
        if not 1 <= beam <= 8:
            raise ValueError(f"beam search covers beam sizes 1..8 (got {beam})")
        if not (temp > 0 and np.isfinite(temp)):
            raise ValueError(f"beam search needs a finite temp > 0 (got {temp})")
        V, d, R, ld, cap = self.vocab_size, dec.d_model, B * beam, L + 1, beam * L
        tags = self._tags(input_dict, B)
        mem = dec.memory(attn_emb, self._side(input_dict), input_dict["attn_emb_len"], beam, L)
        if tags is not None:
            tags = K.upload(tags, dev, torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        Vp = (V + 3) // 4 * 4
        st = search_state.beam_buffers(dev, B, beam, L, self.start_idx, self.end_idx, self.pad_idx)
        search_state.beam_reset(st, B)
        tok, cum, active, n_active, top_val, top_idx = (st[k] for k in ("tok", "cum", "active", "n_active", "top_val", "top_idx"))
        active_before = torch.empty_like(active)
        scratch = torch.empty(2 * R * beam, **f32)
        logit, step_w = torch.empty(R, Vp, **f32), torch.empty(R, Tm, **f32)
        state, state_new = torch.zeros(R, d, **f32), torch.empty(R, d, **f32)
        hist = [torch.zeros(R, L, Tm, **f32) for _ in range(2)]
        planes = (ctypes.c_void_p * 1)(logit.data_ptr())
        for t in range(L):
            # the host asks now and then whether any clip is still searching (TransformerModel.beam_search's schedule)
            if t in (8, 12, 16) and int(n_active.item()) == 0:
                break
            cur = tok[t & 1]
            dec.step(mem, state, state_new, words=cur[:, t:], word_stride=ld, tags=tags if t == 0 else None, logit=logit,
                     ldl=Vp, attn_weight=step_w, attn_strides=(Tm, 1))
            active_before.copy_(active)
            check(lib.ac_ens_beam_step_select(planes, 1, Vp, B, beam, V, t, temp, ptr(cum), ptr(top_val), ptr(top_idx),
                                              ptr(scratch), stream()), "ac_ens_beam_step_select")
            search_state.beam_update(st, t, B, beam, V, L, self.end_idx, self.pad_idx, cap)
            check(lib.ac_bah_beam_gather(ptr(st["src_row"]), ptr(active_before), ptr(state_new), ptr(state), ptr(step_w),
                                         ptr(hist[t & 1]), ptr(hist[(t + 1) & 1]), B, beam, d, Tm, L, t, stream()),
                  "ac_bah_beam_gather")
            last = hist[(t + 1) & 1]
        seq, _ = search_state.beam_rank(st, B, cap, L, self.end_idx, n_best, n_best_size)
        # logit / embed / sampled_logprob are not filled by the reference's beam search either (base.py:124-127)
        return {"seq": seq, "logit": torch.empty(B, L, V, device=dev), "sampled_logprob": torch.zeros(B, L),
                "embed": torch.empty(B, L, d, device=dev),
                "attn_weight": last.view(B, beam, L, Tm)[:, 0].transpose(1, 2).contiguous()}


class TemporalSeq2SeqAttnModel(Seq2SeqAttnModel):
    """``Seq2SeqAttnModel`` over a ``TemporalBahAttnDecoder``: ``input_dict["temporal_tag"]`` holds one integer in 0..3 per
    clip, embedded instead of <start> at step 0 (hf_wrapper.py:1521-1523)."""

    compatible_decoders = (TemporalBahAttnDecoder,)

    def __init__(self, encoder, decoder, **kwargs):
        super().__init__(encoder, decoder, **kwargs)
        self.train_forward_keys = ["cap", "cap_len", "ss_ratio", "temporal_tag"]
        self.inference_forward_keys = ["sample_method", "max_length", "temp", "temporal_tag"]

    def _inference_dict(self, input_dict, encoder_output_dict):
        forward_dict = super()._inference_dict(input_dict, encoder_output_dict)
        forward_dict["temporal_tag"] = input_dict.get("temporal_tag")
        return forward_dict

    def _tags(self, input_dict, B):
        return check_temporal_tag(input_dict.get("temporal_tag"), B)


class ConditionalSeq2SeqAttnModel(Seq2SeqAttnModel):
    """``Seq2SeqAttnModel`` over a condition-controlled decoder: ``input_dict["condition"]`` holds one float per clip, fed to
    every decoder step (attn_model.py:191-223)."""

    compatible_decoders = (ConditionalBahAttnDecoder, SpecificityBahAttnDecoder)

    def __init__(self, encoder, decoder, **kwargs):
        super().__init__(encoder, decoder, **kwargs)
        self.train_forward_keys.append("condition")
        self.inference_forward_keys.append("condition")

    def _inference_dict(self, input_dict, encoder_output_dict):
        forward_dict = super()._inference_dict(input_dict, encoder_output_dict)
        forward_dict["condition"] = input_dict.get("condition")
        return forward_dict

    def _side(self, input_dict):
        return check_condition(input_dict.get("condition"), input_dict["attn_emb"].shape[0])
