"""Transformer caption decoder, MI355X path.  Plugin-compatible with the reference class
``captioning.models.transformer_decoder.TransformerDecoder`` (transformer_decoder.py:11-103) and its
base ``captioning.models.BaseDecoder`` (models/__init__.py:64-92): same constructor, attributes
(``vocab_size``, ``d_model``, ``emb_dim``, ``fc_emb_dim``, ``attn_emb_dim``), ``state_dict()`` keys and
``forward({"word", "attn_emb", "attn_emb_len", "cap_padding_mask"}) -> {"embed", "logit"}``.

The nn modules own the parameters only.  All arithmetic runs in csrc/decoder.hip + csrc/gemm.hip:
``memory()`` projects the audio features once, ``forward`` / ``greedy`` / ``beam_*`` run the per-position
decoder step against a self-attention KV cache.
"""
import ctypes
import math
import os

import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from . import search_state
from ._lib import check, f32c, ptr, stream


class PositionalEncoding(nn.Module):
    """Sinusoid table kept as a frozen Parameter named ``pe`` so that it appears in checkpoints exactly
    like the reference's (model_util.py:167-186)."""

    def __init__(self, d_model, dropout=0.1, max_len=100):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_parameter("pe", nn.Parameter(pe.unsqueeze(1), requires_grad=False))


class BaseDecoder(nn.Module):

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout=0.2, tie_weights=False):
        super().__init__()
        self.emb_dim = emb_dim
        self.vocab_size = vocab_size
        self.fc_emb_dim = fc_emb_dim
        self.attn_emb_dim = attn_emb_dim
        self.tie_weights = tie_weights
        self.word_embedding = nn.Embedding(vocab_size, emb_dim)
        self.in_dropout = nn.Dropout(dropout)


class TransformerDecoder(BaseDecoder):

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, freeze=False,
                 tie_weights=False, **kwargs):
        super().__init__(emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout=dropout, tie_weights=tie_weights)
        self.d_model = emb_dim
        self.nhead = kwargs.get("nhead", self.d_model // 64)
        self.nlayers = kwargs.get("nlayers", 2)
        self.dim_feedforward = kwargs.get("dim_feedforward", self.d_model * 4)
        self.pos_encoder = PositionalEncoding(self.d_model, dropout)
        layer = nn.TransformerDecoderLayer(d_model=self.d_model, nhead=self.nhead,
                                           dim_feedforward=self.dim_feedforward, dropout=dropout)
        self.model = nn.TransformerDecoder(layer, self.nlayers)
        self.classifier = nn.Linear(self.d_model, vocab_size, bias=False)
        if tie_weights:
            self.classifier.weight = self.word_embedding.weight
        self.attn_proj = nn.Sequential(nn.Linear(self.attn_emb_dim, self.d_model), nn.ReLU(),
                                       nn.Dropout(dropout), nn.LayerNorm(self.d_model))
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.freeze = freeze
        if freeze:
            for p in self.parameters():
                p.requires_grad = False
        self._w = None
        self._w_key = None
        self._w_keep = None
        self._ws = {}
        self._greedy_state = None

    def load_pretrained(self, pretrained, output_fn=print):
        """Reference transformer_decoder.py:56-72: take the ``decoder.*`` entries of a model checkpoint."""
        checkpoint = torch.load(pretrained, map_location="cpu")
        if "model" in checkpoint:
            checkpoint = checkpoint["model"]
        sd = {k[8:]: v for k, v in checkpoint.items() if k.startswith("decoder.")} or checkpoint
        own = self.state_dict()
        loaded = {k: v for k, v in sd.items() if k in own and own[k].shape == v.shape}
        own.update(loaded)
        self.load_state_dict(own, strict=True)
        if self.freeze:
            for name, param in self.named_parameters():
                param.requires_grad = name not in loaded

    # ------------------------------------------------------------------------------------------
    def _weights_key(self):
        return tuple((t.data_ptr(), t._version, t.dtype) for t in self.parameters()) + (_lib.param_generation(),)

    # What the decode step runs (csrc/decoder.hip step_shape_ok / check_weights; INTEGRATION.md "Decoder shapes")
    SUPPORTED = ("emb_dim a multiple of 64 up to 512; head width emb_dim / nhead at most 64; dim_feedforward a multiple of 64 "
                 "up to 512, or a multiple of 512; attn_emb_dim a multiple of 32; 1 to %d layers" % _lib.AC_MAX_LAYERS)

    def check_supported(self):
        """Raise HipLibraryError, naming the limit, for a shape the HIP decoder does not run.  Host arithmetic only: asked by
        ``weights()`` before a device pointer is taken, so a refusal precedes every buffer, projection and capture."""
        d, h, ff, A_, n = self.d_model, self.nhead, self.dim_feedforward, self.attn_emb_dim, self.nlayers
        why = None
        if d < 64 or d % 64:
            why = f"emb_dim {d} is not a multiple of 64"
        elif d > 512:
            why = f"emb_dim {d} exceeds 512"
        elif h < 1 or d % h:
            why = f"emb_dim {d} does not divide into nhead {h} heads"
        elif d // h > 64:
            why = f"head width emb_dim / nhead = {d // h} exceeds 64"
        elif ff < 64 or ff % 64:
            why = f"dim_feedforward {ff} is not a multiple of 64"
        elif ff > 512 and ff % 512:
            why = f"dim_feedforward {ff} is above 512 and not a multiple of 512"
        elif A_ < 32 or A_ % 32:
            why = f"attn_emb_dim {A_} is not a multiple of 32"
        elif n < 1 or n > _lib.AC_MAX_LAYERS:
            why = f"nlayers {n} is outside 1..{_lib.AC_MAX_LAYERS}"
        if why is not None:
            raise _lib.HipLibraryError(f"TransformerDecoder (HIP path): {why}.  Supported: {self.SUPPORTED}")

    def weights(self):
        """ac_trm_weights struct of device pointers (rebuilt when a parameter changes)."""
        key = self._weights_key()
        if self._w is not None and key == self._w_key:
            return self._w
        keep = []

        def P(t):
            t = f32c(t.detach())
            keep.append(t)
            return ctypes.c_void_p(ptr(t).value)

        self.check_supported()
        w = _lib.AcTrmWeights()
        w.d_model, w.nhead, w.nlayers, w.dim_ff = self.d_model, self.nhead, self.nlayers, self.dim_feedforward
        w.vocab, w.max_pos, w.attn_emb_dim = self.vocab_size, self.pos_encoder.pe.shape[0], self.attn_emb_dim
        w.emb, w.pe, w.cls_w = P(self.word_embedding.weight), P(self.pos_encoder.pe), P(self.classifier.weight)
        w.proj_w, w.proj_b = P(self.attn_proj[0].weight), P(self.attn_proj[0].bias)
        w.proj_ln_w, w.proj_ln_b = P(self.attn_proj[3].weight), P(self.attn_proj[3].bias)
        for i, L in enumerate(self.model.layers):
            wl = w.layer[i]
            wl.sa_in_w, wl.sa_in_b = P(L.self_attn.in_proj_weight), P(L.self_attn.in_proj_bias)
            wl.sa_out_w, wl.sa_out_b = P(L.self_attn.out_proj.weight), P(L.self_attn.out_proj.bias)
            wl.ca_in_w, wl.ca_in_b = P(L.multihead_attn.in_proj_weight), P(L.multihead_attn.in_proj_bias)
            wl.ca_out_w, wl.ca_out_b = P(L.multihead_attn.out_proj.weight), P(L.multihead_attn.out_proj.bias)
            wl.l1_w, wl.l1_b, wl.l2_w, wl.l2_b = P(L.linear1.weight), P(L.linear1.bias), P(L.linear2.weight), P(L.linear2.bias)
            wl.n1_w, wl.n1_b = P(L.norm1.weight), P(L.norm1.bias)
            wl.n2_w, wl.n2_b = P(L.norm2.weight), P(L.norm2.bias)
            wl.n3_w, wl.n3_b = P(L.norm3.weight), P(L.norm3.bias)
        # fragment-packed copy of the step projections (read by every decode position)
        lib = _lib.load()
        n = lib.ac_trm_step_pack_floats(ctypes.byref(w))
        if n <= 0:
            raise _lib.HipLibraryError("ac_trm_step_pack_floats rejected the decoder configuration")
        pk = torch.empty(n, device=self.word_embedding.weight.device, dtype=torch.float32)
        check(lib.ac_trm_pack_step_weights(ctypes.byref(w), ptr(pk), stream()), "ac_trm_pack_step_weights")
        keep.append(pk)
        w.step_pk = ctypes.c_void_p(pk.data_ptr())
        self._cluster_pk = None   # per-part blobs of the one-launch greedy search, packed on first use (cluster_pack)
        self._w, self._w_key, self._w_keep = w, key, keep
        return w

    def cluster_pack(self):
        """Weights in the layout of the one-launch greedy search (csrc/decoder_cluster.hip: per part, per layer, row-major
        [k][column] slices), or None when the decoder's shape is not the one that kernel covers.  Cached with ``weights()``."""
        w = self.weights()
        if getattr(self, "_cluster_pk", None) is None:
            lib = _lib.load()
            n = lib.ac_trm_cluster_pack_floats(ctypes.byref(w))
            if n <= 0:
                self._cluster_pk = False
            else:
                pk = torch.empty(n, device=self.word_embedding.weight.device, dtype=torch.float32)
                check(lib.ac_trm_cluster_pack(ctypes.byref(w), ptr(pk), stream()), "ac_trm_cluster_pack")
                self._cluster_pk = pk
        return self._cluster_pk if self._cluster_pk is not False else None

    def cluster_covers(self, rows, Tm, max_length, device=None):
        """The one-launch greedy search takes this problem: shape covered, the row's keys and values fit the LDS, and the
        clusters are resident together - one workgroup per CU, four per row: rows <= compute units // 4 of ``device`` (64 on
        a whole MI355X; a CU-masked or partitioned device has fewer and would run the clusters in rounds, slower than the
        launch chain).  AUDIOCAPTION_CLUSTER_MAX_ROWS overrides the bound."""
        if self.d_model != 256 or self.nhead != 4 or self.dim_feedforward != 1024 or max_length > 32:
            return False
        vq = (self.vocab_size + 3) // 4
        if 3 * vq >= self.vocab_size:     # a vocabulary quarter without a column (csrc/decoder_cluster.hip cluster_shape_ok)
            return False
        nlc = (vq + 63) // 64 * 64
        lds = 4 * (256 + 192 + 64 + 256 + 5 * 256 + ((max(Tm, 32) + 3) & ~3) + 256 + 16 + 1024 + nlc
                   + 2 * self.nlayers * (max_length + Tm) * 64) + 64
        env = os.environ.get("AUDIOCAPTION_CLUSTER_MAX_ROWS")
        if env is not None:
            max_rows = int(env)
        else:
            dev = device if device is not None else self.word_embedding.weight.device
            max_rows = torch.cuda.get_device_properties(dev).multi_processor_count // 4 if dev.type == "cuda" else 0
        return lds <= 159 * 1024 and rows <= max_rows

    def workspace(self, rows, max_len, device):
        lib = _lib.load()
        n = lib.ac_trm_workspace_floats(ctypes.byref(self.weights()), rows, max_len)
        if n <= 0:
            raise _lib.HipLibraryError("ac_trm_workspace_floats rejected the decoder configuration")
        ws = self._ws.get(device)
        if ws is None or ws.numel() < n:
            ws = torch.empty(n, device=device, dtype=torch.float32)
            self._ws[device] = ws
        return ws

    def memory(self, attn_emb):
        """attn_emb (R, Tm, attn_emb_dim) -> memkv (nlayers, R*Tm, 2*d): attn_proj + cross-attn K/V."""
        lib = _lib.load()
        w = self.weights()   # first: an unsupported shape is refused before any buffer exists
        attn_emb = f32c(attn_emb)
        R, Tm, _ = attn_emb.shape
        memkv = torch.empty(self.nlayers, R * Tm, 2 * self.d_model, device=attn_emb.device, dtype=torch.float32)
        tmp = torch.empty(R * Tm, self.d_model, device=attn_emb.device, dtype=torch.float32)
        check(lib.ac_trm_memory(ctypes.byref(w), ptr(attn_emb), R, Tm, ptr(memkv), ptr(tmp), stream()), "ac_trm_memory")
        return memkv

    def forward(self, input_dict):
        """The eval-mode full-sequence call: {"word", "attn_emb", "attn_emb_len", "cap_padding_mask"} (and what a conditioned
        decoder takes beside them) -> {"embed", "logit"}."""
        if self.training:
            raise NotImplementedError(
                f"{type(self).__name__} (HIP path): in train mode the decoder only runs inside the whole-model training "
                "step (audiocaption_amd.train.TrainEngine / the model's forward with mode='train')")
        self.weights()       # first: an unsupported shape is refused before any buffer exists
        attn_emb = input_dict["attn_emb"]
        dev = attn_emb.device
        word = input_dict["word"].to(dev)
        N, T = word.shape
        Tm = attn_emb.shape[1]
        extra = self._forward_extra(input_dict, dev, N)
        mem_len = K.upload(input_dict["attn_emb_len"], dev, torch.int32)
        mask = input_dict.get("cap_padding_mask")
        mask_u8 = None if mask is None else mask.to(dev).to(torch.uint8).contiguous()
        st = {**extra, "attn_emb": f32c(attn_emb),
              "memkv": torch.empty(self.nlayers, N * Tm, 2 * self.d_model, device=dev, dtype=torch.float32),
              "tmp": torch.empty(N * Tm, self.d_model, device=dev, dtype=torch.float32)}
        self._memory_launch(st)
        tokens = word.to(torch.int32).contiguous()
        embed = torch.empty(N, T, self.d_model, device=dev, dtype=torch.float32)
        logit = torch.empty(N, T, self.vocab_size, device=dev, dtype=torch.float32)
        ws = self.workspace(N, T, dev)
        self._trm("forward_tokens", st.get("kw"), ptr(st["memkv"]), ptr(mem_len), N, Tm, ptr(tokens), ptr(mask_u8), T, ptr(embed),
                  ptr(logit), ptr(ws))
        return {"embed": embed, "logit": logit}

    def _trm(self, name, kw, *args):
        """``ac_trm_<name>(weights, *args, stream)`` - with the keyword struct ``kw`` of a conditioned decoder,
        ``ac_trm_kw_<name>(weights, &kw, *args, stream)``: the one place that chooses between the two entry points."""
        lib, w = _lib.load(), ctypes.byref(self.weights())
        if kw is None:
            check(getattr(lib, "ac_trm_" + name)(w, *args, stream()), "ac_trm_" + name)
        else:
            check(getattr(lib, "ac_trm_kw_" + name)(w, ctypes.byref(kw), *args, stream()), "ac_trm_kw_" + name)

    # ---- what a conditioned decoder adds to a search (KeywordProbTransformerDecoder overrides these) -------------------------
    def _keyword_struct(self, kwp, row_div):
        """The keyword struct over projected keywords ``kwp``, ``row_div`` decoder rows per clip (None: the plain entry
        points)."""
        if kwp is not None:
            raise TypeError(f"{self.__class__.__name__} takes no conditioning input")
        return None

    def _forward_extra(self, input_dict, dev, N):
        """``_extra_buffers`` of a ``forward`` over N rows with this call's inputs in them, checked before any launch."""
        return {}

    def _extra_key(self, extra):
        """The part of a search state's cache key that names the extra per-clip inputs (none here)."""
        if extra is not None:
            raise TypeError(f"{self.__class__.__name__} takes no conditioning input")
        return ()

    def _extra_buffers(self, dev, B, row_div=1):
        """Static buffers of those inputs inside a search state over B clips (``row_div`` decoder rows per clip)."""
        return {}

    def _stage_extra(self, st, extra):
        """Copy the inputs of this call into the state's static buffers (before a launch or a replay)."""

    def _memory_launch(self, st):
        """The once-per-batch part of a search's launch sequence over its static buffers, on the current stream (capturable):
        the audio memory and the cross-attention K / V of every layer."""
        B, Tm, _ = st["attn_emb"].shape
        check(_lib.load().ac_trm_memory(ctypes.byref(self.weights()), ptr(st["attn_emb"]), B, Tm, ptr(st["memkv"]),
                                        ptr(st["tmp"]), stream()), "ac_trm_memory")

    def _greedy_launch(self, st, max_length, start_idx, end_idx, pad_idx):
        """Memory preparation + the whole on-device greedy loop on the current stream (capturable)."""
        B, Tm, _ = st["attn_emb"].shape
        self._memory_launch(st)
        if st.get("cluster_ws") is not None:
            self._trm("greedy_cluster", None, ptr(st["cluster_pk"]), ptr(st["memkv"]), ptr(st["mem_len"]), B, Tm, max_length,
                      start_idx, end_idx, pad_idx, ptr(st["seq"]), ptr(st["logit"]), ptr(st["sampled_logprob"]),
                      ptr(st["embed"]), ptr(st["unfinished_cnt"]), ptr(st["cluster_ws"]), int(st["early_stop"]))
            return
        if st.get("rules") is not None:
            self._rules_search_launch(st, B, 1, max_length, start_idx, end_idx, pad_idx, None)
            return
        self._trm("greedy_segments", st.get("kw"), ptr(st["memkv"]), ptr(st["mem_len"]), B, st["segments"], Tm, max_length,
                  start_idx, end_idx, pad_idx, ptr(st["seq"]), ptr(st["logit"]), ptr(st["sampled_logprob"]), ptr(st["embed"]),
                  ptr(st["unfinished_cnt"]), ptr(st["ws"]))

    def _rules_search_launch(self, st, B, row_div, max_length, start_idx, end_idx, pad_idx, params):
        """The greedy (``params`` None) or sampled search over B * row_div rows with the state's logit rules between every
        step's logits and its pick (``ac_trm_search_rules``): always the launch chain, ``logit`` keeps the raw logits."""
        Tm = st["attn_emb"].shape[1]
        method, k, top_p, temp = (-1, 0, 0.0, 1.0) if params is None else params   # -1: AC_SEARCH_GREEDY
        self._trm("search_rules", None, ptr(st["memkv"]), ptr(st["mem_len"]), B * row_div, int(row_div), Tm, max_length,
                  start_idx, end_idx, pad_idx, ptr(st["seq"]), ptr(st["logit"]), ptr(st["sampled_logprob"]), ptr(st["embed"]),
                  ptr(st["unfinished_cnt"]), ptr(st["ws"]), int(method), int(k), float(top_p), float(temp), ptr(st.get("seed")),
                  ctypes.byref(st["rules"]), ptr(st["rules_plane"]), st["ld_plane"])

    def _rules_key(self, rules, extra):
        """The part of a search state's key that names the logit rules (none: the key of the unconstrained search)."""
        if rules is None:
            return ()
        if extra is not None:
            raise NotImplementedError(f"{type(self).__name__}: repetition and word constraints are not built for a "
                                      "conditioned decoder")
        return (("rules", rules.key()),)

    def _search_buffers(self, key, dev, B, Tm, A, max_length, segments=1, samples_per_clip=1):
        """Static buffers of an on-device search (greedy or sampled) over B clips: inputs, workspace, outputs.  ``segments``
        batches share the chain: one row of unfinished counts each (one segment: the plain ``(max_length,)`` vector).
        ``samples_per_clip`` decoder rows per clip: the inputs and the memory keep B rows, the workspace and every per-row
        output have B * samples_per_clip, clip-major."""
        f32 = dict(device=dev, dtype=torch.float32)
        R = B * samples_per_clip
        ws_n = _lib.load().ac_trm_workspace_floats(ctypes.byref(self.weights()), R, max_length)
        if ws_n <= 0:
            raise _lib.HipLibraryError(f"ac_trm_workspace_floats rejected {R} rows of {max_length} positions")
        return {
            **self._extra_buffers(dev, B),
            "key": key, "graph": None, "uses": 0, "segments": segments,
            "attn_emb": torch.empty(B, Tm, A, **f32), "mem_len": torch.empty(B, device=dev, dtype=torch.int32),
            "memkv": torch.empty(self.nlayers, B * Tm, 2 * self.d_model, **f32),
            "tmp": torch.empty(B * Tm, self.d_model, **f32), "ws": torch.empty(ws_n, **f32),
            "seq": torch.empty(R, max_length, device=dev, dtype=torch.int64),
            "logit": torch.empty(R, max_length, self.vocab_size, **f32),
            "sampled_logprob": torch.empty(R, max_length, **f32),
            "embed": torch.empty(R, max_length, self.d_model, **f32),
            "unfinished_cnt": torch.empty((segments, max_length) if segments > 1 else (max_length,), device=dev,
                                          dtype=torch.int32),
        }

    def greedy(self, attn_emb, attn_emb_len, max_length, start_idx, end_idx, pad_idx, alone=False, mode=None, extra=None,
               rules=None):
        """On-device greedy search.  Returns device tensors seq (int64), logit, logprob, embed, cnt.  ``attn_emb`` /
        ``attn_emb_len``: one batch, or lists of batches of the same (frames, width) decoded as one chain.  Batches of one
        row count are the chain's segments: each stops when ITS rows have all emitted <end>, as the reference's loop over
        that batch does (from then on the chain's launches skip its rows), and ``unfinished_cnt`` comes back per batch,
        ``(batches, max_length)``.  Batches of different row counts are searched as one segment.  The logit / embed columns
        of the steps a segment did not run are 0.  A batch decoded inside a shared chain gives the bits it gives alone as
        long as the memory projection (``ac_linear`` over rows x frames) takes the same kernel on both sides: its skinny
        kernel up to 128 rows, the tiled one beyond, which sum in different orders (~3e-6 on the logits) - e.g. 3 rows x 31
        frames alone (93) against 6 rows grouped (186) do not; from 5 rows x 31 frames per batch on both sides are tiled.

        Two forms of the same search.  "chain": ten launches per step (csrc/decoder.hip) - ~90 us per step whatever the row
        count, the form that shares the GPU with the next batch's encoder (``forward_async``).  "cluster": ONE persistent
        launch, a cluster of four workgroups per row (csrc/decoder_cluster.hip) - about half the time per step when
        nothing else runs on the GPU and the rows fit (``cluster_covers``).  ``mode`` (default: AUDIOCAPTION_GREEDY =
        "auto"): "auto" takes the cluster form when the caller says the decode runs ``alone`` (the blocking ``model()``
        call) and the problem is covered.  The returned dict then carries "cluster_error" (device int32 word, non-zero:
        a workgroup's partners never started - rerun with mode="chain").

        The ~370 short launches of a decode are latency-bound, so the fixed launch sequence (memory
        preparation + max_length decoder steps) is captured once per shape (on its second use) into a HIP graph over
        static buffers and replayed; inputs are copied in, outputs are cloned out (fresh tensors per call, as the
        reference returns).  Set AUDIOCAPTION_DECODE_GRAPH=0 to launch eagerly.

        ``rules`` (a non-neutral ``logit_rules.LogitRules``; None: the search above, with its key and graphs): the
        constrained search - always the launch chain, one launch more per step (csrc/logit_rules.hip between the classifier
        and the pick); ``logit`` keeps the raw logits.  The rules are part of the state key."""
        parts = list(attn_emb) if isinstance(attn_emb, (list, tuple)) else [attn_emb]   # several batches, one chain: each is
        dev = parts[0].device                                                           # copied into its rows of the static buffer
        B, Tm = sum(p_.shape[0] for p_ in parts), parts[0].shape[1]
        segments = len(parts) if len({p_.shape[0] for p_ in parts}) == 1 else 1
        mode = mode or os.environ.get("AUDIOCAPTION_GREEDY", "auto")
        if mode not in ("auto", "chain", "cluster"):
            raise ValueError(f"AUDIOCAPTION_GREEDY={mode!r}: 'auto', 'chain' or 'cluster'")
        if rules is not None and mode == "auto":
            mode = "chain"                                         # the one-launch form picks from the raw logits
        wanted = mode == "cluster" or (mode == "auto" and alone)   # the weights are repacked for it only when it can be chosen
        covered = wanted and self.cluster_covers(B, Tm, max_length, dev) and self.cluster_pack() is not None
        if mode == "cluster" and (not covered or rules is not None):
            raise _lib.HipLibraryError("the one-launch greedy search does not cover this decoder shape / row count" if
                                       rules is None else "the one-launch greedy search applies no logit rules")
        cluster = wanted and covered
        if cluster or rules is not None:
            segments = 1   # the one-launch form (and the constrained search) stops on the whole row set
        # AUDIOCAPTION_CLUSTER_EARLY_STOP=0: the one-launch form runs all max_length steps like the launch chain (benchmarks that
        # compare the two at equal work; the outputs are the same either way)
        early = os.environ.get("AUDIOCAPTION_CLUSTER_EARLY_STOP", "1") != "0"
        key = (dev, B, Tm, max_length, start_idx, end_idx, pad_idx, cluster, early, self._weights_key(), segments) + \
            self._extra_key(extra) + self._rules_key(rules, extra)
        if self._greedy_state is None:
            self._greedy_state = {}

        def more():
            if rules is not None:
                return rules.buffers(dev, B, self.vocab_size, end_idx)
            if not cluster:
                return {}
            nb = _lib.load().ac_trm_cluster_workspace_bytes(B)
            return {"cluster_ws": torch.zeros((nb + 7) // 8, device=dev, dtype=torch.int64),   # (the error word is reset by every call)
                    "cluster_pk": self.cluster_pack(), "early_stop": early}
        if isinstance(attn_emb_len, (list, tuple)):
            attn_emb_len = torch.cat([torch.as_tensor(l_).cpu().reshape(-1) for l_ in attn_emb_len])   # host side
        return self._search(self._greedy_state, key, parts, attn_emb_len, max_length, segments, more, extra,
                            lambda st: self._greedy_launch(st, max_length, start_idx, end_idx, pad_idx))

    def _search(self, states, key, parts, attn_emb_len, max_length, segments, more, extra, launch, seed=None,
                samples_per_clip=1):
        """The body of ``greedy`` and ``sample``: the state of ``key`` (``_search_buffers`` and what ``more()`` adds; batches of
        changing length keep 8 shapes), every batch of ``parts`` copied into its rows of the static input, ``launch(st)`` run or
        replayed (``search_state.run``), the outputs cloned out."""
        dev = parts[0].device

        def build():
            B, (Tm, A) = sum(p_.shape[0] for p_ in parts), parts[0].shape[1:]
            return {**self._search_buffers(key, dev, B, Tm, A, max_length, segments, samples_per_clip), **more()}
        st = search_state.lookup(states, key, build, 8)
        r0 = 0
        for p_ in parts:
            st["attn_emb"][r0:r0 + p_.shape[0]].copy_(p_)
            r0 += p_.shape[0]
        st["mem_len"].copy_(K.upload(attn_emb_len, dev, torch.int32))
        if seed is not None:
            st["seed"].fill_(seed)
        self._stage_extra(st, extra)
        search_state.run(st, dev, lambda: launch(st))
        out = {k: st[k].clone() for k in ("seq", "logit", "sampled_logprob", "embed", "unfinished_cnt")}
        if st.get("cluster_ws") is not None:
            out["cluster_error"] = st["cluster_ws"][:1].clone()
        return out

    def _sample_launch(self, st, max_length, start_idx, end_idx, pad_idx, params, samples_per_clip=1):
        """Memory preparation + the whole sampled search on the current stream (capturable; the seed is read on the device)."""
        B, Tm, _ = st["attn_emb"].shape
        method, k, top_p, temp = params
        self._memory_launch(st)
        if st.get("rules") is not None:
            self._rules_search_launch(st, B, samples_per_clip, max_length, start_idx, end_idx, pad_idx, params)
            return
        if samples_per_clip != 1:      # the memory of the B clips once; samples_per_clip rows per clip read it
            self._trm("sample_multi", None, ptr(st["memkv"]), ptr(st["mem_len"]), B, int(samples_per_clip), Tm, max_length,
                      start_idx, end_idx, pad_idx, ptr(st["seq"]), ptr(st["logit"]), ptr(st["sampled_logprob"]),
                      ptr(st["embed"]), ptr(st["unfinished_cnt"]), ptr(st["ws"]), int(method), int(k), float(top_p),
                      float(temp), ptr(st["seed"]))
            return
        self._trm("sample", st.get("kw"), ptr(st["memkv"]), ptr(st["mem_len"]), B, Tm, max_length, start_idx, end_idx, pad_idx,
                  ptr(st["seq"]), ptr(st["logit"]), ptr(st["sampled_logprob"]), ptr(st["embed"]), ptr(st["unfinished_cnt"]),
                  ptr(st["ws"]), int(method), int(k), float(top_p), float(temp), ptr(st["seed"]))

    def sample(self, attn_emb, attn_emb_len, max_length, start_idx, end_idx, pad_idx, method, k, top_p, temp, seed, extra=None,
               samples_per_clip=1, rules=None):
        """On-device sampled search (base.py:152-170 with a sampling ``sample_method``; csrc/sample.hip).  ``method``, ``k``,
        ``top_p``, ``temp``: ``sampling.parse_sample_method``; ``seed``: 64-bit Philox key - row b of step t draws from
        counter (t, b), so a caption depends on (seed, row, step) only.  Returns what ``greedy`` returns.

        Always the launch chain (the one-launch cluster form picks the argmax only).  Like ``greedy``, the launch sequence
        is captured per shape AND sampling parameters (second use) into a HIP graph over static buffers and replayed; the
        seed lives in a device word that is written before every launch or replay, so one graph serves every seed.
        AUDIOCAPTION_DECODE_GRAPH=0 launches eagerly.

        ``samples_per_clip`` = S > 1: S captions per clip from ONE memory projection (``ac_trm_sample_multi``).  The outputs
        have B * S rows, clip-major (row r is caption r % S of clip r // S), and row r of step t draws from counter (t, r):
        the result of this call on ``attn_emb.repeat_interleave(S, 0)`` with the same seed, without projecting a clip's
        memory S times.  S is part of the state key: a graph captured for one S is never replayed for another; S = 1 is
        the call above, with its key and graph.

        ``rules``: as in ``greedy`` - the draw is from the constrained row, ``sampled_logprob`` its value there."""
        from .sampling import seed_word
        dev, (B, Tm, _) = attn_emb.device, attn_emb.shape
        params = (int(method), int(k), float(top_p), float(temp))
        if isinstance(samples_per_clip, bool) or not isinstance(samples_per_clip, int) or samples_per_clip < 1:
            raise ValueError(f"samples_per_clip must be an int >= 1, got {samples_per_clip!r}")
        key = (dev, B, Tm, max_length, start_idx, end_idx, pad_idx, params, self._weights_key()) + self._extra_key(extra) + \
            self._rules_key(rules, extra)
        if samples_per_clip != 1:
            if extra is not None:
                raise NotImplementedError(f"{type(self).__name__}: samples_per_clip (several sampled captions per clip) is "
                                          "not built for a conditioned decoder")
            if B * samples_per_clip * (max_length + 1) >= 2 ** 31:
                raise ValueError(f"samples_per_clip: {B} clips x {samples_per_clip} captions x {max_length} positions exceed "
                                 "the search's row index")
            key += (("samples_per_clip", samples_per_clip),)
        if getattr(self, "_sample_state", None) is None:
            self._sample_state = {}
        return self._search(self._sample_state, key, [attn_emb], attn_emb_len, max_length, 1,
                            lambda: {"seed": torch.zeros(1, device=dev, dtype=torch.int64),
                                     **({} if rules is None else
                                        rules.buffers(dev, B * samples_per_clip, self.vocab_size, end_idx))}, extra,
                            lambda st: self._sample_launch(st, max_length, start_idx, end_idx, pad_idx, params, samples_per_clip),
                            seed=seed_word(seed), samples_per_clip=samples_per_clip)

    def beam_step(self, memkv, mem_len, B, beam, Tm, max_length, t, temp, tokens, mask, cum, ws, kwp=None):
        """One beam-search step outside a search state.  ``kwp`` (B, d): the clips' projected keywords, for a decoder that
        takes them."""
        kw = self._keyword_struct(kwp, beam)
        dev = memkv.device
        top_val = torch.empty(B, beam, device=dev, dtype=torch.float32)
        top_idx = torch.empty(B, beam, device=dev, dtype=torch.int32)
        self._trm("beam_step", kw, ptr(memkv), ptr(mem_len), B, beam, Tm, max_length, t, float(temp), ptr(tokens), ptr(mask),
                  ptr(cum), ptr(top_val), ptr(top_idx), ptr(ws))
        return top_val, top_idx

    def _beam_step_launch(self, st, B, beam, Tm, max_length, t, temp, tokens):
        """Step t of a beam search over the static buffers of its state (``TransformerModel._beam_begin``; capturable).  A
        state with logit rules scores the constrained rows (``ac_trm_beam_step_rules``)."""
        if st.get("rules") is not None:
            self._trm("beam_step_rules", None, ptr(st["memkv"]), ptr(st["mem_len"]), B, beam, Tm, max_length, t, float(temp),
                      ptr(tokens), ptr(st["mask"]), ptr(st["cum"]), ptr(st["top_val"]), ptr(st["top_idx"]), ptr(st["ws"]),
                      ctypes.byref(st["rules"]), ptr(st["rules_plane"]))
            return
        self._trm("beam_step", st.get("kw"), ptr(st["memkv"]), ptr(st["mem_len"]), B, beam, Tm, max_length, t, float(temp),
                  ptr(tokens), ptr(st["mask"]), ptr(st["cum"]), ptr(st["top_val"]), ptr(st["top_idx"]), ptr(st["ws"]))

    def beam_reorder(self, R, max_length, t, src_row, ws):
        lib = _lib.load()
        check(lib.ac_trm_beam_reorder(ctypes.byref(self.weights()), R, max_length, t, ptr(src_row), ptr(ws),
                                      stream()), "ac_trm_beam_reorder")


def check_keyword(keyword, rows, classes):
    """``input_dict["keyword"]`` of a keyword-conditioned captioner: (rows, classes) multi-hot or probabilities, a CPU or
    device tensor (or array) of any float dtype.  KeyError when it is missing, ValueError for another shape - both before
    anything is launched.  Returns it as a float32 tensor (device unchanged)."""
    if keyword is None:
        raise KeyError("keyword: a KeywordProbTransformerDecoder needs input_dict['keyword'] of shape "
                       f"(batch, {classes})")
    keyword = torch.as_tensor(keyword)
    if keyword.dim() != 2 or keyword.shape[0] != rows or keyword.shape[1] != classes:
        raise ValueError(f"keyword must be ({rows}, {classes}) = (batch, keyword_classes_num), got {tuple(keyword.shape)}")
    if keyword.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"keyword must be a float tensor (multi-hot or probabilities), got {keyword.dtype}")
    return keyword.detach().to(torch.float32)


class KeywordProbTransformerDecoder(TransformerDecoder):
    """The reference's ``KeywordProbTransformerDecoder`` (transformer_decoder.py:177-214): a ``TransformerDecoder`` whose
    input rows are ``word_keyword_norm(embedding * sqrt(d) + keyword_proj(keyword)) + pe`` - a per-clip keyword vector
    (multi-hot or probabilities over ``keyword_classes_num`` classes) steers every decoding position.  Same constructor,
    parameters in the reference's order (``keyword_proj``, ``word_keyword_norm`` are created after the base class has run
    its xavier initialisation, so they keep torch's default initialisation as in the reference).

    ``keyword_proj(keyword)`` runs once per batch (``ac_gemm``, inside the captured launch sequence, right after the audio
    memory); the decode step embeds through the PRO_EMBED_KW producer of csrc/decoder.hip.  Always the launch chain on the
    general / per-row routes: the one-launch cluster search and the wide routes are not built for it."""

    def __init__(self, emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, keyword_classes_num, **kwargs):
        super().__init__(emb_dim, vocab_size, fc_emb_dim, attn_emb_dim, dropout, **kwargs)
        self.keyword_classes_num = int(keyword_classes_num)
        self.keyword_proj = nn.Linear(self.keyword_classes_num, self.d_model)
        self.word_keyword_norm = nn.LayerNorm(self.d_model)
        self._kw_keep = self._kw_key = None

    def check_supported(self):
        super().check_supported()
        if self.keyword_classes_num < 1:
            raise _lib.HipLibraryError(f"KeywordProbTransformerDecoder (HIP path): keyword_classes_num "
                                       f"{self.keyword_classes_num} is below 1")

    def cluster_covers(self, rows, Tm, max_length, device=None):
        return False      # csrc/decoder_cluster.hip embeds without keywords

    def _keyword_weights(self):
        """(keyword_proj.weight, keyword_proj.bias, word_keyword_norm.weight, word_keyword_norm.bias) as contiguous f32
        device tensors on 16-byte boundaries (the producer reads the norm with 16-byte loads), cached with ``weights()``."""
        self.weights()
        if self._kw_key != self._w_key:
            def P(t):
                t = f32c(t.detach())
                return t if t.data_ptr() % 16 == 0 else t.clone()
            self._kw_keep = tuple(P(t) for t in (self.keyword_proj.weight, self.keyword_proj.bias,
                                                 self.word_keyword_norm.weight, self.word_keyword_norm.bias))
            self._kw_key = self._w_key
        return self._kw_keep

    # ---- the keyword batch inside a search state --------------------------------------------------------------------------
    def _extra_key(self, extra):
        if extra is None:
            raise KeyError("keyword: a KeywordProbTransformerDecoder needs the keyword batch")
        return ("keyword", tuple(extra.shape))

    def _keyword_struct(self, kwp, row_div):
        if kwp is None:
            raise KeyError("keyword: KeywordProbTransformerDecoder.beam_step needs kwp, the projected keyword batch")
        _, _, ln_w, ln_b = self._keyword_weights()
        return _lib.AcTrmKeyword(kwp.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), int(row_div))

    def _extra_buffers(self, dev, B, row_div=1):
        f32 = dict(device=dev, dtype=torch.float32)
        kwp = torch.empty(B, self.d_model, **f32)
        return {"keyword": torch.empty(B, self.keyword_classes_num, **f32), "kwp": kwp,
                "kw": self._keyword_struct(kwp, row_div), "kw_hold": self._keyword_weights()[2:]}

    def _stage_extra(self, st, extra):
        st["keyword"].copy_(check_keyword(extra, *st["keyword"].shape))

    def _forward_extra(self, input_dict, dev, N):
        keyword = check_keyword(input_dict.get("keyword"), N, self.keyword_classes_num).to(dev).contiguous()
        return {**self._extra_buffers(dev, N), "keyword": keyword}   # projected where it lies: no copy into the buffer

    def _keyword_proj_launch(self, keyword, kwp):
        """kwp (B, d) = keyword (B, classes) keyword_proj.weight^T + bias on the current stream (any class count)."""
        W, b, _, _ = self._keyword_weights()
        B, C = keyword.shape
        check(_lib.load().ac_gemm(ptr(keyword), C, 1, ptr(W), 1, C, ptr(kwp), self.d_model, B, self.d_model, C, ptr(b), 0, 0.0,
                                  1, 0.0, 0, None, 0, None, 0, stream()), "ac_gemm(keyword_proj)")

    def _memory_launch(self, st):
        super()._memory_launch(st)
        self._keyword_proj_launch(st["keyword"], st["kwp"])

    def greedy(self, attn_emb, attn_emb_len, max_length, start_idx, end_idx, pad_idx, keyword=None, alone=False, mode=None):
        """``TransformerDecoder.greedy`` with the keyword batch (B, keyword_classes_num); one batch per call.  ``mode``
        "cluster" (or AUDIOCAPTION_GREEDY=cluster) raises HipLibraryError: the one-launch search has no keyword producer."""
        if isinstance(attn_emb, (list, tuple)):
            raise NotImplementedError("KeywordProbTransformerDecoder: one batch per greedy chain (shared chains are not built "
                                      "for keyword conditioning)")
        keyword = check_keyword(keyword, attn_emb.shape[0], self.keyword_classes_num)
        return super().greedy(attn_emb, attn_emb_len, max_length, start_idx, end_idx, pad_idx, alone=alone, mode=mode,
                              extra=keyword)

    def sample(self, attn_emb, attn_emb_len, max_length, start_idx, end_idx, pad_idx, method, k, top_p, temp, seed,
               keyword=None):
        keyword = check_keyword(keyword, attn_emb.shape[0], self.keyword_classes_num)
        return super().sample(attn_emb, attn_emb_len, max_length, start_idx, end_idx, pad_idx, method, k, top_p, temp, seed,
                              extra=keyword)
