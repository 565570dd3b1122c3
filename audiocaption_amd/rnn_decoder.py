"""Bahdanau-attention GRU caption decoders, MI355X path.  Plugin-compatible with the reference classes ``RnnDecoder``,
``BahAttnCatFcDecoder`` (captioning/models/rnn_decoder.py:10-36,159-216), ``Seq2SeqAttention`` (utils/model_util.py, as
restated at hf_wrapper.py:1377-1414) and ``TemporalBahAttnDecoder`` (hf_wrapper.py:1502-1554): same constructor keywords,
attributes and ``state_dict()`` keys, so a reference checkpoint loads with ``strict=True``.

The nn modules own the parameters only; the arithmetic runs in csrc/attn_gru.hip.  ``forward`` is one decoder step
(``ac_bah_step_logits``) with the reference's dict contract; the searches of ``attn_model.py`` call ``memory`` once per batch
and then ``greedy`` / ``sample`` (one C call each) or ``step`` (beam search).

Training (csrc/attn_gru_train.hip): ``train_forward`` runs the scheduled-sampling forward of the reference's
``stepwise_forward`` for ``mode="train"`` (base.py:152-208, attn_model.py:34-65) in one C call and keeps what
``train_backward`` - the backward through time, one C call - needs.  The constructor's ``dropout`` (``in_dropout`` on the
step's input embedding) takes effect when ``self.training`` is set: counter-hash masks at site ``train.OP_BAH_IN``,
regenerated in the backward.  ``train_rollout`` is the sampled rollout of self-critical sequence training
(``ac_bah_train_rollout``): the same chain with no caption, each step on the word the step before drew, and the same kept
state.  The models of ``attn_model.py`` reach all three through ``train_attn_gru.AttnGruTrainEngine``.

``ConditionalBahAttnDecoder`` (rnn_decoder.py:276-336) and ``SpecificityBahAttnDecoder`` (rnn_decoder.py:519-575) are the
condition-controlled decoders: one float per clip, ``condition``, takes ``fc_emb``'s place in ``memory``, ``train_forward``
and ``forward`` (``ac_bah_memory_cond``, ``ac_bah_train_forward_cond`` / ``ac_bah_train_backward_cond``); the searches
and the step are the same C calls.  Neither reads ``fc_emb``.  ``train_rollout`` (SCST) is not built for them.

Built: ``rnn_type="GRU"``, ``num_layers=1``, unidirectional; emb_dim, d_model, attn_size, attn_emb_dim, fc_emb_dim each a
multiple of 32 up to 1024; vocab_size <= 16384.  Anything else raises NotImplementedError in the constructor.
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from ._lib import check, f32c, ptr, stream
from .transformer_decoder import BaseDecoder

MAX_DIM, MAX_VOCAB, MAX_FRAMES = 1024, 16384, 2048


class Seq2SeqAttention(nn.Module):
    """Parameters of the additive attention: ``h2attn`` takes cat(decoder state, encoder frame) - the first ``hs_dec`` input
    columns belong to the decoder state (hf_wrapper.py:1401) - and ``v`` scores tanh(h2attn(.))."""

    def __init__(self, hs_enc, hs_dec, attn_size):
        super().__init__()
        self.h2attn = nn.Linear(hs_enc + hs_dec, attn_size)
        self.v = nn.Parameter(torch.randn(attn_size))

    def forward(self, h_dec, h_enc, src_lens):
        raise NotImplementedError("Seq2SeqAttention runs inside the decoder step (csrc/attn_gru.hip), not on its own")


class RnnDecoder(BaseDecoder):

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs):
        super().__init__(emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout)
        self.d_model = d_model
        self.num_layers = kwargs.get("num_layers", 1)
        self.bidirectional = kwargs.get("bidirectional", False)
        self.rnn_type = kwargs.get("rnn_type", "GRU")
        if self.rnn_type != "GRU":
            raise NotImplementedError(f"rnn_type={self.rnn_type!r}: the HIP decoder runs a GRU only")
        if self.num_layers != 1:
            raise NotImplementedError(f"num_layers={self.num_layers}: the HIP decoder runs one GRU layer")
        if self.bidirectional:
            raise NotImplementedError("bidirectional=True: the HIP decoder is unidirectional")
        self.classifier = nn.Linear(self.d_model, vocab_size)

    def forward(self, x):
        raise NotImplementedError

    def init_hidden(self, bs, device):
        return torch.zeros(1, bs, self.d_model, device=device)


class BahAttnCatFcDecoder(RnnDecoder):
    """GRU over cat(word embedding, ctx_proj(attention context), fc_proj(fc_emb)) (rnn_decoder.py:159-216)."""

    n_tags = 0
    variant = 0        # ac_bah_weights.variant
    ENTRY = {"memory": "ac_bah_memory", "train_forward": "ac_bah_train_forward", "train_backward": "ac_bah_train_backward"}

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs):
        super().__init__(emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs)
        attn_size = kwargs.get("attn_size", self.d_model)
        for name, v in (("emb_dim", emb_dim), ("d_model", d_model), ("attn_size", attn_size),
                        ("attn_emb_dim", attn_emb_dim), ("fc_emb_dim", fc_emb_dim)):
            if v < 32 or v % 32 or v > MAX_DIM:
                raise NotImplementedError(f"{name}={v}: the HIP decoder needs a multiple of 32 up to {MAX_DIM}")
        if not 1 <= vocab_size <= MAX_VOCAB:
            raise NotImplementedError(f"vocab_size={vocab_size}: the pick and sampling kernels hold at most {MAX_VOCAB} words")
        self.attn_size = attn_size
        self.model = nn.GRU(input_size=self.emb_dim * 3, hidden_size=self.d_model, batch_first=True, num_layers=1,
                            bidirectional=False)
        self.attn = Seq2SeqAttention(self.attn_emb_dim, self.d_model, attn_size)
        self.fc_proj = nn.Linear(self.fc_emb_dim, self.emb_dim)
        self.ctx_proj = nn.Linear(self.attn_emb_dim, self.emb_dim)
        self._w = self._w_key = self._w_keep = None

    # ------------------------------------------------------------------------------------------
    def weights(self):
        """ac_bah_weights struct of device pointers (rebuilt when a parameter changes)."""
        key = tuple((t.data_ptr(), t._version, t.dtype) for t in self.parameters()) + (_lib.param_generation(),)
        if self._w is not None and key == self._w_key:
            return self._w
        keep = []

        def P(t):
            t = f32c(t.detach())
            keep.append(t)
            return ctypes.c_void_p(ptr(t).value)

        w = _lib.AcBahWeights()
        w.emb_dim, w.d_model, w.attn_size = self.emb_dim, self.d_model, self.attn_size
        w.attn_emb_dim, w.fc_emb_dim, w.vocab, w.n_tags = self.attn_emb_dim, self.fc_emb_dim, self.vocab_size, self.n_tags
        w.variant = self.variant
        w.emb = P(self.word_embedding.weight)
        if self.n_tags:
            w.temb = P(self.temporal_embedding.weight)
        w.w_hh = P(self.model.weight_hh_l0)
        w.b_ih, w.b_hh = P(self.model.bias_ih_l0), P(self.model.bias_hh_l0)
        w.attn_w, w.attn_b, w.attn_v = P(self.attn.h2attn.weight), P(self.attn.h2attn.bias), P(self.attn.v)
        self._input_weights(w, P)
        w.cls_w, w.cls_b = P(self.classifier.weight), P(self.classifier.bias)
        self._w, self._w_key, self._w_keep = w, key, keep
        return w

    def _input_weights(self, w, P):
        """The slots that depend on what the GRU input is made of (``ac_bah_weights.variant``)."""
        w.w_ih = P(self.model.weight_ih_l0)
        w.fc_w, w.fc_b = P(self.fc_proj.weight), P(self.fc_proj.bias)
        w.ctx_w, w.ctx_b = P(self.ctx_proj.weight), P(self.ctx_proj.bias)

    def _side(self, side, attn_emb):
        """The once-per-batch input next to the audio memory, checked, on the device: ``fc_emb`` (N, F)."""
        fc_emb = f32c(side)
        ptr(fc_emb)
        if attn_emb.dim() != 3 or attn_emb.shape[2] != self.attn_emb_dim or fc_emb.shape != (attn_emb.shape[0], self.fc_emb_dim):
            raise ValueError(f"attn_emb {tuple(attn_emb.shape)} / fc_emb {tuple(fc_emb.shape)} do not fit attn_emb_dim "
                             f"{self.attn_emb_dim} / fc_emb_dim {self.fc_emb_dim}")
        return fc_emb

    def memory(self, attn_emb, fc_emb, attn_emb_len, rows_per_clip=1, max_length=20):
        """Once per batch: the workspace with the key projection and the fc part of the input gates (``ac_bah_memory``).
        Returns the handle ``step`` / ``greedy`` / ``sample`` take."""
        lib = _lib.load()
        w = self.weights()
        attn_emb = f32c(attn_emb)
        ptr(attn_emb)                # a CPU tensor is refused here, before anything is uploaded
        fc_emb = self._side(fc_emb, attn_emb)
        B, Tm, _ = attn_emb.shape
        if Tm > MAX_FRAMES:
            raise NotImplementedError(f"{Tm} frames of audio memory: the attention kernel holds at most {MAX_FRAMES}")
        dev = attn_emb.device
        R = B * int(rows_per_clip)
        n = lib.ac_bah_workspace_floats(ctypes.byref(w), B, R, Tm, int(max_length))
        if n <= 0:
            raise _lib.HipLibraryError("ac_bah_workspace_floats rejected the decoder configuration")
        mem = {"attn_emb": attn_emb, "len": K.upload(attn_emb_len, dev, torch.int32), "B": B, "R": R, "Tm": Tm,
               "max_length": int(max_length), "row_div": int(rows_per_clip),
               "ws": torch.empty(n, device=dev, dtype=torch.float32)}
        check(getattr(lib, self.ENTRY["memory"])(ctypes.byref(w), ptr(attn_emb), ptr(fc_emb), B, R, Tm, int(max_length),
                                                 ptr(mem["ws"]), stream()), self.ENTRY["memory"])
        mem["side"] = fc_emb
        return mem

    def step(self, mem, state_in, state_out, words=None, word_stride=1, tags=None, logit=None, ldl=None, embed=None,
             attn_weight=None, attn_strides=(0, 0)):
        """One decoder step over the rows of ``mem`` into caller-owned buffers (``ac_bah_step_logits``)."""
        ldl = self.vocab_size if ldl is None else ldl
        check(_lib.load().ac_bah_step_logits(
            ctypes.byref(self.weights()), ptr(mem["attn_emb"]), ptr(mem["len"]), mem["B"], mem["R"], mem["row_div"], mem["Tm"],
            mem["max_length"], ptr(state_in), ptr(words), word_stride, ptr(tags), ptr(state_out), ptr(embed), self.d_model,
            ptr(logit), ldl, ptr(attn_weight), attn_strides[0], attn_strides[1], ptr(mem["ws"]), stream()),
            "ac_bah_step_logits")

    def _search(self, mem, tags, start_idx, end_idx, pad_idx, sampler=None):
        lib = _lib.load()
        B, Tm, L, dev = mem["B"], mem["Tm"], mem["max_length"], mem["attn_emb"].device
        f32 = dict(device=dev, dtype=torch.float32)
        out = {"seq": torch.empty(B, L, device=dev, dtype=torch.int64), "logit": torch.empty(B, L, self.vocab_size, **f32),
               "sampled_logprob": torch.empty(B, L, **f32), "embed": torch.empty(B, L, self.d_model, **f32),
               "attn_weight": torch.empty(B, Tm, L, **f32), "state": torch.empty(1, B, self.d_model, **f32),
               "unfinished_cnt": torch.empty(L, device=dev, dtype=torch.int32)}
        args = [ctypes.byref(self.weights()), ptr(mem["attn_emb"]), ptr(mem["len"]), ptr(tags), B, Tm, L, start_idx, end_idx,
                pad_idx, ptr(out["seq"]), ptr(out["logit"]), ptr(out["sampled_logprob"]), ptr(out["embed"]),
                ptr(out["attn_weight"]), ptr(out["state"]), ptr(out["unfinished_cnt"]), ptr(mem["ws"])]
        if sampler is None:
            check(lib.ac_bah_greedy(*args, stream()), "ac_bah_greedy")
        else:
            method, k, top_p, temp, seed = sampler
            from .sampling import seed_word
            mem["seed"] = torch.full((1,), seed_word(seed), device=dev, dtype=torch.int64)
            check(lib.ac_bah_sample(*args, method, k, float(top_p), float(temp), ptr(mem["seed"]), stream()), "ac_bah_sample")
        return out

    def greedy(self, mem, tags, start_idx, end_idx, pad_idx):
        """The whole greedy search in one C call (``ac_bah_greedy``); ``mem`` from ``memory(..., rows_per_clip=1)``."""
        return self._search(mem, tags, start_idx, end_idx, pad_idx)

    def sample(self, mem, tags, start_idx, end_idx, pad_idx, method, k, top_p, temp, seed):
        """The whole sampled search in one C call (``ac_bah_sample``): the sampler and Philox counters of ``ac_trm_sample``."""
        return self._search(mem, tags, start_idx, end_idx, pad_idx, (method, k, top_p, temp, seed))

    # ---- training ------------------------------------------------------------------------------------------
    GRAD_FIELDS = (("emb", "word_embedding.weight"), ("temb", "temporal_embedding.weight"), ("w_ih", "model.weight_ih_l0"),
                   ("w_hh", "model.weight_hh_l0"), ("b_ih", "model.bias_ih_l0"), ("b_hh", "model.bias_hh_l0"),
                   ("attn_w", "attn.h2attn.weight"), ("attn_b", "attn.h2attn.bias"), ("attn_v", "attn.v"),
                   ("fc_w", "fc_proj.weight"), ("fc_b", "fc_proj.bias"), ("ctx_w", "ctx_proj.weight"),
                   ("ctx_b", "ctx_proj.bias"), ("cls_w", "classifier.weight"), ("cls_b", "classifier.bias"))

    def grad_struct(self, address_of):
        """ac_bah_grads whose fields are ``address_of(parameter name)`` (an int): where ``train_backward`` adds."""
        g = _lib.AcBahGrads()
        for field, name in self.GRAD_FIELDS:
            if field != "temb" or self.n_tags:
                setattr(g, field, ctypes.c_void_p(address_of(name)))
        return g

    def train_forward(self, attn_emb, fc_emb, attn_emb_len, cap, use_cap, tags=None, start_idx=1, dropout_seed=0,
                      seed_dev=None):
        """The training forward over T = cap.size(1) - 1 steps (``ac_bah_train_forward``; no host synchronisation).
        ``attn_emb`` (N, Tm, A), ``fc_emb`` (N, F) and ``cap`` (N, T + 1, int64) on the device; ``attn_emb_len``: host values
        or an int32 device tensor; ``use_cap``: the T scheduled-sampling coins, drawn by the caller (1: the step takes
        ``cap[:, t]``; 0: <start> at t == 0, else the arg-max of step t - 1); ``tags``: int32 (N,) on the device for a temporal
        decoder.  ``in_dropout`` is active when ``self.training``: the mask of site ``train.OP_BAH_IN`` for the base seed
        ``dropout_seed`` - or, with ``seed_dev`` (the address of a device word holding the base seed), for that word.
        Returns seq (int64), logit (N, T, V), sampled_logprob, embed (N, T, d), attn_weight (N, Tm, T), state (1, N, d) on
        the device, and under "saved" what ``train_backward`` takes."""
        from .train import OP_BAH_IN
        lib = _lib.load()
        w = self.weights()
        attn_emb = f32c(attn_emb)
        ptr(attn_emb), ptr(cap)
        fc_emb = self._side(fc_emb, attn_emb)
        B, Tm, _ = attn_emb.shape
        if Tm > MAX_FRAMES:
            raise NotImplementedError(f"{Tm} frames of audio memory: the attention kernels hold at most {MAX_FRAMES}")
        if cap.dtype != torch.int64 or cap.dim() != 2 or cap.shape[0] != B or cap.shape[1] < 2 or not cap.is_contiguous():
            raise ValueError(f"cap must be a contiguous int64 ({B}, T + 1) tensor with T >= 1")
        T = cap.shape[1] - 1
        use_cap = [int(bool(u)) for u in use_cap]
        if len(use_cap) != T:
            raise ValueError(f"use_cap holds {len(use_cap)} coins for {T} steps")
        if (tags is None) != (self.n_tags == 0):
            raise ValueError("tags: required by a temporal decoder, refused by a plain one")
        dev = attn_emb.device
        lens = attn_emb_len if (torch.is_tensor(attn_emb_len) and attn_emb_len.is_cuda and attn_emb_len.dtype == torch.int32) \
            else K.upload(attn_emb_len, dev, torch.int32)
        n = lib.ac_bah_train_workspace_floats(ctypes.byref(w), B, Tm, T)
        if n <= 0:
            raise _lib.HipLibraryError("ac_bah_train_workspace_floats rejected the decoder configuration")
        f32 = dict(device=dev, dtype=torch.float32)
        p = float(self.in_dropout.p) if self.training else 0.0
        if seed_dev is None:       # the kernels' effective seed is drop_seed + (*seed_dev << 16)
            seed = ((int(dropout_seed) << 16) + OP_BAH_IN) & 0xFFFFFFFFFFFFFFFF
        else:
            seed = OP_BAH_IN
        out = {"seq": torch.empty(B, T, device=dev, dtype=torch.int64), "logit": torch.empty(B, T, self.vocab_size, **f32),
               "sampled_logprob": torch.empty(B, T, **f32), "embed": torch.empty(B, T, self.d_model, **f32),
               "attn_weight": torch.empty(B, Tm, T, **f32), "state": torch.empty(1, B, self.d_model, **f32)}
        saved = {"w": w, "attn_emb": attn_emb, "fc_emb": fc_emb, "len": lens, "B": B, "Tm": Tm, "T": T, "p": p, "seed": seed,
                 "seed_dev": seed_dev, "ws": torch.empty(n, **f32)}
        args = [ctypes.byref(w), ptr(attn_emb), ptr(fc_emb), ptr(lens), ptr(cap), cap.shape[1], (ctypes.c_int * T)(*use_cap)]
        if not self.variant:       # the conditional entry point takes no tags
            args.append(ptr(tags))
        check(getattr(lib, self.ENTRY["train_forward"])(
            *args, B, Tm, T, int(start_idx), p, seed, seed_dev, ptr(out["seq"]), ptr(out["logit"]),
            ptr(out["sampled_logprob"]), ptr(out["embed"]), ptr(out["attn_weight"]), ptr(out["state"]), ptr(saved["ws"]),
            stream()), self.ENTRY["train_forward"])
        out["saved"] = saved
        return out

    def train_rollout(self, attn_emb, fc_emb, attn_emb_len, max_length, temp, sample_seed, tags=None, forced=None,
                      start_idx=1, end_idx=2, dropout_seed=0, seed_dev=None):
        """The sampled rollout of self-critical sequence training over ``max_length`` steps (``ac_bah_train_rollout``; no
        host synchronisation): ``train_forward`` with no caption, step t > 0 on the word step t - 1 stored.  The word of
        step t is drawn from softmax(log_softmax(logit_t) / temp) by the plain sampler at Philox counter (t, clip) under
        ``sample_seed`` (one int64 device word, see ``sampling.seed_word``) - or is ``forced[:, t]`` (int32 (N, T) on the
        device, the parity hook); a clip that has stored ``end_idx`` keeps storing it, and every step runs.  The other
        arguments are ``train_forward``'s.  Returns what ``train_forward`` returns with ``seq_i32`` (the stored words where
        the decoder left them) next to ``seq`` (int64) and ``sampled_logprob`` = log_softmax(logit)[word] / temp; "saved"
        feeds ``train_backward`` unchanged."""
        from .train import OP_BAH_IN
        lib = _lib.load()
        w = self.weights()
        attn_emb, fc_emb = f32c(attn_emb), f32c(fc_emb)
        ptr(attn_emb), ptr(fc_emb)
        if attn_emb.dim() != 3 or attn_emb.shape[2] != self.attn_emb_dim or fc_emb.shape != (attn_emb.shape[0], self.fc_emb_dim):
            raise ValueError(f"attn_emb {tuple(attn_emb.shape)} / fc_emb {tuple(fc_emb.shape)} do not fit attn_emb_dim "
                             f"{self.attn_emb_dim} / fc_emb_dim {self.fc_emb_dim}")
        B, Tm, _ = attn_emb.shape
        if Tm > MAX_FRAMES:
            raise NotImplementedError(f"{Tm} frames of audio memory: the attention kernels hold at most {MAX_FRAMES}")
        T, temp = int(max_length), float(temp)
        if T < 1:
            raise ValueError("train_rollout: max_length must be at least 1")
        if not (math.isfinite(temp) and temp > 0):
            raise ValueError(f"train_rollout: temp must be finite and > 0, got {temp}")
        if (tags is None) != (self.n_tags == 0):
            raise ValueError("tags: required by a temporal decoder, refused by a plain one")
        dev = attn_emb.device
        if forced is not None and (forced.dtype != torch.int32 or tuple(forced.shape) != (B, T) or not forced.is_contiguous()
                                   or forced.device != dev):
            raise ValueError(f"forced must be a contiguous int32 ({B}, {T}) tensor on the device")
        if sample_seed.dtype != torch.int64 or sample_seed.device != dev:
            raise ValueError("sample_seed must be one int64 word on the device")
        lens = attn_emb_len if (torch.is_tensor(attn_emb_len) and attn_emb_len.is_cuda and attn_emb_len.dtype == torch.int32) \
            else K.upload(attn_emb_len, dev, torch.int32)
        n = lib.ac_bah_train_workspace_floats(ctypes.byref(w), B, Tm, T)
        if n <= 0:
            raise _lib.HipLibraryError("ac_bah_train_workspace_floats rejected the decoder configuration")
        f32 = dict(device=dev, dtype=torch.float32)
        p = float(self.in_dropout.p) if self.training else 0.0
        seed = ((int(dropout_seed) << 16) + OP_BAH_IN) & 0xFFFFFFFFFFFFFFFF if seed_dev is None else OP_BAH_IN
        out = {"seq_i32": torch.empty(B, T, device=dev, dtype=torch.int32), "logit": torch.empty(B, T, self.vocab_size, **f32),
               "sampled_logprob": torch.empty(B, T, **f32), "embed": torch.empty(B, T, self.d_model, **f32),
               "attn_weight": torch.empty(B, Tm, T, **f32), "state": torch.empty(1, B, self.d_model, **f32)}
        saved = {"w": w, "attn_emb": attn_emb, "fc_emb": fc_emb, "len": lens, "B": B, "Tm": Tm, "T": T, "p": p, "seed": seed,
                 "seed_dev": seed_dev, "ws": torch.empty(n, **f32), "sample_seed": sample_seed, "forced": forced}
        scratch = torch.empty(2 * B, device=dev, dtype=torch.int32)
        check(lib.ac_bah_train_rollout(
            ctypes.byref(w), ptr(attn_emb), ptr(fc_emb), ptr(lens), ptr(tags), B, Tm, T, int(start_idx), int(end_idx), temp,
            ptr(sample_seed), ptr(forced), T, p, seed, seed_dev, ptr(out["seq_i32"]), ptr(scratch), ptr(out["logit"]),
            ptr(out["sampled_logprob"]), ptr(out["embed"]), ptr(out["attn_weight"]), ptr(out["state"]), ptr(saved["ws"]),
            stream()), "ac_bah_train_rollout")
        out["seq"] = out["seq_i32"].to(torch.int64)
        out["saved"] = saved
        return out

    def train_backward(self, saved, dlogit, grads=None, d_attn_emb=None, d_fc_emb=None):
        """Backward through time of the ``train_forward`` that returned ``saved`` (``ac_bah_train_backward``), given
        ``dlogit`` (N, T, V; a tensor or a device address).  ``grads``: an ``ac_bah_grads`` (``grad_struct``) the gradients
        are ADDED to; None: fresh zeroed tensors, returned by parameter name.  ``d_attn_emb`` (N, Tm, A) / ``d_fc_emb``
        (N, F): tensors or device addresses that are WRITTEN; None: fresh tensors.
        Returns (grads by name or None, d_attn_emb, d_fc_emb)."""
        lib = _lib.load()
        B, Tm, T = saved["B"], saved["Tm"], saved["T"]
        dev = saved["attn_emb"].device
        named = None
        if grads is None:
            params = dict(self.named_parameters())
            named = {name: torch.zeros_like(params[name], dtype=torch.float32).contiguous()
                     for field, name in self.GRAD_FIELDS if field != "temb" or self.n_tags}
            grads = self.grad_struct(lambda name: named[name].data_ptr())
        if torch.is_tensor(dlogit):
            dlogit = f32c(dlogit)
            if tuple(dlogit.shape) != (B, T, self.vocab_size):
                raise ValueError(f"dlogit {tuple(dlogit.shape)}: expected {(B, T, self.vocab_size)}")
        if d_attn_emb is None:
            d_attn_emb = torch.empty(B, Tm, self.attn_emb_dim, device=dev, dtype=torch.float32)
        if d_fc_emb is None:
            d_fc_emb = torch.empty(B, self.fc_emb_dim, device=dev, dtype=torch.float32)

        def P(x):
            return ptr(x) if torch.is_tensor(x) else ctypes.c_void_p(x)

        check(getattr(lib, self.ENTRY["train_backward"])(
            ctypes.byref(saved["w"]), ctypes.byref(grads), ptr(saved["attn_emb"]), ptr(saved["fc_emb"]), ptr(saved["len"]),
            P(dlogit), B, Tm, T, saved["p"], saved["seed"], saved["seed_dev"], P(d_attn_emb), P(d_fc_emb), ptr(saved["ws"]),
            stream()), self.ENTRY["train_backward"])
        return named, d_attn_emb, d_fc_emb

    def _tags(self, input_dict, n):
        return None

    def forward(self, input_dict):
        """One step with the reference's contract (rnn_decoder.py:183-216): ``word`` (N, 1), optional ``state``
        (1, N, d_model), ``fc_emb``, ``attn_emb``, ``attn_emb_len`` -> ``state``, ``embed`` (N, 1, d_model), ``logit``
        (N, 1, V), ``attn_weight`` (N, Tm).  The memory side is recomputed on every call, as in the reference."""
        attn_emb = input_dict["attn_emb"]
        dev = attn_emb.device
        N, Tm = attn_emb.shape[0], attn_emb.shape[1]
        side = check_condition(input_dict.get("condition"), N) if self.variant else input_dict["fc_emb"]
        mem = self.memory(attn_emb, side, input_dict["attn_emb_len"], 1, 1)
        state = input_dict.get("state")
        state_in = f32c(state).reshape(N, self.d_model) if state is not None else torch.zeros(N, self.d_model, device=dev)
        word = input_dict["word"]
        if word.dim() != 2 or word.shape != (N, 1):
            raise NotImplementedError(f"word of shape {tuple(word.shape)}: the HIP decoder step takes word ids (N, 1)")
        tags = self._tags(input_dict, N)
        if tags is not None:
            tags = K.upload(tags, dev, torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        out = {"state": torch.empty(1, N, self.d_model, **f32), "embed": torch.empty(N, 1, self.d_model, **f32),
               "logit": torch.empty(N, 1, self.vocab_size, **f32), "attn_weight": torch.empty(N, Tm, **f32)}
        self.step(mem, state_in, out["state"], words=K.upload(word.reshape(N), dev, torch.int32), tags=tags,
                  logit=out["logit"], embed=out["embed"], attn_weight=out["attn_weight"], attn_strides=(Tm, 1))
        return out


def check_temporal_tag(tag, n):
    """``temporal_tag`` as int64 (n,) on the host; raises ValueError unless it holds n integers in 0..3."""
    if tag is None:
        raise ValueError("temporal_tag is required: one integer in 0..3 per clip")
    tag = torch.as_tensor(tag).detach().cpu()
    if tag.dtype.is_floating_point or tag.dtype == torch.bool or tag.numel() != n:
        raise ValueError(f"temporal_tag must hold {n} integers in 0..3 (got dtype {tag.dtype}, {tag.numel()} values)")
    tag = tag.reshape(n).to(torch.int64)
    if n and (int(tag.min()) < 0 or int(tag.max()) > 3):
        raise ValueError(f"temporal_tag must be in 0..3 (got {tag.tolist()})")
    return tag


class TemporalBahAttnDecoder(BahAttnCatFcDecoder):
    """``BahAttnCatFcDecoder`` whose first input is the embedding of the clip's temporal tag instead of <start>
    (hf_wrapper.py:1502-1554)."""

    n_tags = 4

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs):
        super().__init__(emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs)
        self.temporal_embedding = nn.Embedding(4, emb_dim)

    def _tags(self, input_dict, n):
        return check_temporal_tag(input_dict.get("temporal_tag"), n) if input_dict["t"] == 0 else None


def check_condition(condition, n):
    """``condition`` as float32 (n,) on the host; raises ValueError unless it holds n finite floating-point values (any
    finite value: a specificity is a sentence sum, not confined to 0..1)."""
    if condition is None:
        raise ValueError("condition is required: one float per clip")
    condition = torch.as_tensor(condition).detach().cpu()
    if not condition.dtype.is_floating_point or condition.numel() != n:
        raise ValueError(f"condition must hold {n} floats (got dtype {condition.dtype}, {condition.numel()} values)")
    condition = condition.reshape(n).to(torch.float32)
    if n and not bool(torch.isfinite(condition).all()):
        raise ValueError(f"condition must be finite (got {condition.tolist()})")
    return condition


def _identity(x):
    return x


class ConditionalBahAttnDecoder(BahAttnCatFcDecoder):
    """GRU over cat(word embedding, ctx_proj(attention context), cond_emb) with cond_emb = (1 - condition) *
    condition_embedding.weight[0] + condition * condition_embedding.weight[1] (rnn_decoder.py:276-336).  There is no
    ``fc_proj``; ``fc_emb`` is not read.  Where ``BahAttnCatFcDecoder``'s methods take ``fc_emb`` this one takes
    ``condition``: n floats, host values or a tensor (``check_condition``)."""

    variant = 1
    ENTRY = {"memory": "ac_bah_memory_cond", "train_forward": "ac_bah_train_forward_cond",
             "train_backward": "ac_bah_train_backward_cond"}
    GRAD_FIELDS = tuple((f, "condition_embedding.weight" if f == "fc_w" else n) for f, n in BahAttnCatFcDecoder.GRAD_FIELDS
                        if f not in ("temb", "fc_b"))

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs):
        super().__init__(emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs)
        del self.fc_proj
        self.condition_embedding = nn.Embedding(2, emb_dim)

    def _input_weights(self, w, P):
        w.w_ih = P(self.model.weight_ih_l0)
        w.fc_w = P(self.condition_embedding.weight)
        w.ctx_w, w.ctx_b = P(self.ctx_proj.weight), P(self.ctx_proj.bias)

    def _side(self, side, attn_emb):
        if attn_emb.dim() != 3 or attn_emb.shape[2] != self.attn_emb_dim:
            raise ValueError(f"attn_emb {tuple(attn_emb.shape)} does not fit attn_emb_dim {self.attn_emb_dim}")
        return check_condition(side, attn_emb.shape[0]).to(attn_emb.device)

    def train_rollout(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}: the SCST rollout is not built for the condition-controlled decoders")


class SpecificityBahAttnDecoder(ConditionalBahAttnDecoder):
    """GRU over cat(word embedding, attention context, condition): E + A + 1 input columns, the context at its full width
    and the condition as one raw column (rnn_decoder.py:519-575).  No ``fc_proj``, no ``ctx_proj`` (the reference's
    identity), no ``condition_embedding``.

    ``weight_ih_l0`` has the odd row pitch E + A + 1.  ``weights()`` repacks it whenever it rebuilds the struct: the first
    E + A columns as an aligned (3d, E + A) block for the input-gate product, the last column on its own; the gradient is
    written into the parameter's own layout (``grad_struct``)."""

    variant = 2
    GRAD_FIELDS = tuple((f, n) for f, n in BahAttnCatFcDecoder.GRAD_FIELDS if f not in ("temb", "fc_w", "fc_b", "ctx_w", "ctx_b"))

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs):
        super().__init__(emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, d_model, **kwargs)
        del self.ctx_proj, self.condition_embedding
        self.ctx_proj = _identity
        self.model = nn.GRU(input_size=self.emb_dim + self.attn_emb_dim + 1, hidden_size=self.d_model, batch_first=True,
                            num_layers=1, bidirectional=False)

    def _input_weights(self, w, P):
        xw = self.emb_dim + self.attn_emb_dim
        w.w_ih = P(self.model.weight_ih_l0[:, :xw])     # P copies a strided slice into a contiguous block
        w.fc_w = P(self.model.weight_ih_l0[:, xw])

    def grad_struct(self, address_of):
        g = super().grad_struct(address_of)
        g.fc_w = ctypes.c_void_p(address_of("model.weight_ih_l0") + 4 * (self.emb_dim + self.attn_emb_dim))
        return g
