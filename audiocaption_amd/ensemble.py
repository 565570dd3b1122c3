"""Ensemble decoding over several captioners, MI355X path.  The counterpart of the reference's
``python_scripts/train_eval/ensemble.py`` (``EnsembleRunner.stepwise_forward`` :94-151, ``beam_search`` :154-276):
several trained captioners decode one batch together - at every step each member's decoder runs on the shared prefix,
the members' ``log_softmax`` outputs are averaged (f32, not renormalised) and one word is chosen for all of them.

``EnsembleModel(models)(input_dict)["seq"]`` is what ``TransformerModel`` returns, so ``hf_wrapper.CaptioningModel`` takes
an ensemble as it takes a single captioner.  ``ensemble.py`` is the specification, and it departs from the single-model
search (base.py) in ways that change the output:

* greedy stores ``m[word]`` (the mean itself), not a log-softmax value; for one member the two coincide;
* beam search NEVER retires a clip: there is no "as many finished beams as the beam size" break, every clip searches to
  ``max_length`` and the best length-normalised score among ALL finished beams wins.  ``EnsembleModel([m])`` with
  ``sample_method="beam"`` is therefore deliberately NOT ``m`` with ``sample_method="beam"``;
* sampling divides the mean by ``temp`` before top-p as well, and stores ``m[w] / temp`` (plain, top-k), the log of the
  renormalised kept probability (top-p) or ``m[w]`` (gumbel; made to work for any batch size);
* the reference keeps writing words after a row's ``<end>``; here, as in the single-model search, a row's columns after
  its first ``end_idx`` are ``end_idx`` with ``sampled_logprob`` 0.  Up to and including the first ``<end>`` they agree.

Members share the prefix (one token / key-mask / unfinished buffer), the vocabulary and the start / end / pad indices;
each keeps its own encoder, its own audio memory of its own length, its own ``attn_emb_len`` and its own KV cache.

Schedule: the members' encoders run one after the other on the current stream (they are matrix-bound).  Per decode step
the members' step chains (``ac_trm_step_logits``) run back to back on that stream, followed by ONE pick kernel of
csrc/ensemble.hip over all members' logit planes; the whole search is a fixed launch sequence over static buffers, captured
per shape into a HIP graph on its second use and replayed (AUDIOCAPTION_DECODE_GRAPH=0: always launch eagerly).
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from . import logit_rules
from . import search_state
from ._lib import check, ptr, stream
from .transformer_decoder import KeywordProbTransformerDecoder, TransformerDecoder
from .transformer_model import CaptionModel, _device_flags


class _EncoderRerun:
    """What ``CaptionModel._check_flags`` needs of a model, with ``forward`` = the member's ENCODER alone: a raised device
    status word re-runs the encoder on the tier / kernel that cannot raise it, not the member's own decode."""
    _check_flags = CaptionModel._check_flags
    _rerun_wide = CaptionModel._rerun_wide

    def __init__(self, model):
        self.encoder = model.encoder

    def forward(self, input_dict):
        return self.encoder(input_dict)


class EnsembleModel(nn.Module):

    def __init__(self, models):
        super().__init__()
        models = list(models)
        if not models:
            raise ValueError("EnsembleModel needs at least one member")
        if len(models) > _lib.AC_ENS_MAX:
            raise ValueError(f"EnsembleModel takes at most {_lib.AC_ENS_MAX} members (AC_ENS_MAX), got {len(models)}")
        for m in models:
            if not isinstance(getattr(m, "decoder", None), TransformerDecoder):
                raise NotImplementedError(f"EnsembleModel: the step kernels cover TransformerDecoder members only "
                                          f"(got {type(getattr(m, 'decoder', m)).__name__})")
            if isinstance(m.decoder, KeywordProbTransformerDecoder):
                raise NotImplementedError("EnsembleModel: keyword conditioning is not built for ensemble decoding (a "
                                          "KeywordProbTransformerDecoder member needs its keyword batch at every step)")
        first = models[0]
        for m in models[1:]:
            if m.vocab_size != first.vocab_size:
                raise ValueError(f"members disagree on vocab_size ({first.vocab_size} vs {m.vocab_size}); the reference "
                                 "would need a vocabulary mapping as well")
            if (m.start_idx, m.end_idx, m.pad_idx) != (first.start_idx, first.end_idx, first.pad_idx):
                raise ValueError("members disagree on start_idx / end_idx / pad_idx")
            if m.max_length != first.max_length:
                raise ValueError(f"members disagree on max_length ({first.max_length} vs {m.max_length})")
        self.models = nn.ModuleList(models)
        self.vocab_size = first.vocab_size
        self.start_idx, self.end_idx, self.pad_idx = first.start_idx, first.end_idx, first.pad_idx
        self.max_length = first.max_length
        self._state = {}

    # ---- the call surface of TransformerModel --------------------------------------------------------
    def forward(self, input_dict):
        if input_dict.get("mode") != "inference":
            raise NotImplementedError("EnsembleModel decodes only (mode='inference'); train the members one by one")
        if input_dict.get("n_samples") is not None:
            from .transformer_model import N_SAMPLES
            raise NotImplementedError(f"EnsembleModel: {N_SAMPLES} is not built for ensembles")
        logit_rules.refuse(input_dict, "EnsembleModel", "a single TransformerModel's blocking model(input_dict)")
        if input_dict.get("group_size") is not None:
            from .transformer_model import GROUP_BEAM
            raise NotImplementedError(f"EnsembleModel: {GROUP_BEAM} is not built for ensembles")
        encs = [m.encoder(input_dict) for m in self.models]   # one after the other on the current stream
        args = {k: input_dict[k] for k in ("sample_method", "max_length", "temp", "beam_size", "n_best", "n_best_size", "seed")
                if input_dict.get(k) is not None}
        out = self.decode(encs, **args)
        # The encoders' device status words, read with the results (as TransformerModel.forward does): a member whose
        # encoder raised one (fp16 range left in the conv tier, a split-GRU partner that never started) gets its ENCODER run
        # again as TransformerModel would run it again, and the ensemble is decoded once more from the new memories.
        redone = False
        for n, (m, enc) in enumerate(zip(self.models, encs)):
            flags = _device_flags(enc)
            if flags is None:
                continue
            redo = _EncoderRerun(m)._check_flags(flags.cpu(), input_dict)
            if redo is not None:
                encs[n] = redo
                redone = True
        if redone:
            out = self.decode(encs, **args)
        return out

    def decode(self, encoder_outputs, sample_method="greedy", max_length=None, temp=1.0, beam_size=3, n_best=False,
               n_best_size=None, seed=None):
        """The search from given per-member ``{"attn_emb", "attn_emb_len"}`` dicts (one per member, in member order; the
        batch size is shared, frames and feature width are each member's own).  ``temp`` is the reference's
        ``sample_word_temp`` for sampling and its ``beam_temp`` for beam search.  Returns ``seq`` (int64, CPU, (B, max_length)
        or (B, n_best_size, max_length) with ``n_best``), ``sampled_logprob`` (CPU, (B, max_length); zeros for beam search),
        ``encoder_outputs`` (the list passed in) and, for beam search, ``score`` ((B,) or (B, n_best_size))."""
        encs = list(encoder_outputs)
        if len(encs) != len(self.models):
            raise ValueError(f"{len(encs)} encoder outputs for {len(self.models)} members")
        B = encs[0]["attn_emb"].shape[0]
        if any(e["attn_emb"].shape[0] != B for e in encs):
            raise ValueError("members disagree on the batch size")
        max_length = int(self.max_length if max_length is None else max_length)
        if sample_method == "dbs":
            raise NotImplementedError("sample_method='dbs': diverse beam search is not on the accelerated path")
        if sample_method == "beam":
            res = self._beam(encs, int(beam_size), max_length, float(temp), bool(n_best),
                             int(beam_size if n_best_size is None else n_best_size))
        else:
            res = self._stepwise(encs, sample_method, max_length, float(temp), seed)
        res["encoder_outputs"] = encs
        return res

    # ---- shared plumbing -------------------------------------------------------------------------------
    def _member_buffers(self, encs, rows, row_div, max_length, dev):
        """Static per-member buffers: inputs, audio memory, workspace (its own KV cache) and the logit plane."""
        f32 = dict(device=dev, dtype=torch.float32)
        lib = _lib.load()
        ldl = (self.vocab_size + 3) // 4 * 4      # rows of a plane start 16-byte aligned: the picks load 16 bytes per lane
        out = []
        for m, e in zip(self.models, encs):
            dec = m.decoder
            Bn, Tm, A = e["attn_emb"].shape
            ws_n = lib.ac_trm_workspace_floats(ctypes.byref(dec.weights()), rows, max_length)
            if ws_n <= 0:
                raise _lib.HipLibraryError("ac_trm_workspace_floats rejected a member's decoder configuration")
            out.append({"attn_emb": torch.empty(Bn, Tm, A, **f32), "mem_len": torch.empty(Bn, device=dev, dtype=torch.int32),
                        "memkv": torch.empty(dec.nlayers, Bn * Tm, 2 * dec.d_model, **f32),
                        "tmp": torch.empty(Bn * Tm, dec.d_model, **f32), "ws": torch.empty(ws_n, **f32),
                        "logit": torch.empty(rows, ldl, **f32), "Tm": Tm, "row_div": row_div})
        planes = (ctypes.c_void_p * len(out))(*[b["logit"].data_ptr() for b in out])
        return out, planes, ldl

    def _state_for(self, kind, encs, params, build):
        dev = encs[0]["attn_emb"].device
        key = (kind, dev, params, tuple(tuple(e["attn_emb"].shape) for e in encs),
               tuple(m.decoder._weights_key() for m in self.models), self.start_idx, self.end_idx, self.pad_idx)
        st = search_state.lookup(self._state, key, lambda: dict(build(dev), graph=None), 6)
        for b, e in zip(st["members"], encs):
            b["attn_emb"].copy_(K.f32c(e["attn_emb"]))
            b["mem_len"].copy_(K.upload(e["attn_emb_len"], dev, torch.int32))
        return st, dev

    def _memory(self, st):
        lib = _lib.load()
        for m, b in zip(self.models, st["members"]):
            Bn = b["attn_emb"].shape[0]
            check(lib.ac_trm_memory(ctypes.byref(m.decoder.weights()), ptr(b["attn_emb"]), Bn, b["Tm"], ptr(b["memkv"]),
                                    ptr(b["tmp"]), stream()), "ac_trm_memory")

    def _steps(self, st, rows, max_length, t, tok, mask, cache_set):
        """Every member's decoder step for position t on the shared prefix: logits into the member's plane."""
        lib = _lib.load()
        for m, b in zip(self.models, st["members"]):
            check(lib.ac_trm_step_logits(ctypes.byref(m.decoder.weights()), ptr(b["memkv"]), ptr(b["mem_len"]), rows,
                                         b["row_div"], b["Tm"], max_length, t, ptr(tok), ptr(mask), cache_set, ptr(b["logit"]),
                                         st["ldl"], None, 0, ptr(b["ws"]), stream()), "ac_trm_step_logits")

    # ---- greedy and sampling (ensemble.py:94-151, :412-449) ------------------------------------------------
    def _stepwise(self, encs, sample_method, max_length, temp, seed):
        from .sampling import draw_seed, parse_sample_method, seed_word, GUMBEL
        B, V, M = encs[0]["attn_emb"].shape[0], self.vocab_size, len(self.models)
        if sample_method == "greedy":
            rule = None
        else:
            # ensemble.py:427 divides by temp under every rule but gumbel (whose argmax temp does not move)
            code, k, top_p, _ = parse_sample_method(sample_method, V, temp)
            if code != GUMBEL and not (temp > 0 and np.isfinite(temp)):
                raise ValueError(f"sample_method={sample_method!r} needs a finite temp > 0 (got {temp})")
            rule = (code, k, top_p, 1.0 if code == GUMBEL else temp)
            seed = draw_seed() if seed is None else int(seed)

        def build(dev):
            i32 = dict(device=dev, dtype=torch.int32)
            members, planes, ldl = self._member_buffers(encs, B, 1, max_length, dev)
            tok0 = torch.full((B, max_length + 1), self.end_idx, **i32)
            tok0[:, 0] = self.start_idx
            mask0 = torch.zeros(B, max_length + 1, device=dev, dtype=torch.uint8)
            mask0[:, 0] = int(self.start_idx == self.pad_idx)
            return {"members": members, "planes": planes, "ldl": ldl, "tok0": tok0, "mask0": mask0,
                    "tok": torch.empty_like(tok0), "mask": torch.empty_like(mask0), "unfinished": torch.empty(B, **i32),
                    "cnt": torch.empty(max_length, **i32), "seq": torch.empty(B, max_length, device=dev, dtype=torch.int64),
                    "logprob": torch.empty(B, max_length, device=dev, dtype=torch.float32),
                    "seed": torch.zeros(1, device=dev, dtype=torch.int64)}

        st, dev = self._state_for("step", encs, (B, max_length, rule), build)
        if rule is not None:
            st["seed"].fill_(seed_word(seed))     # read on the device: one graph serves every seed
        lib = _lib.load()

        def launch():
            st["tok"].copy_(st["tok0"])
            st["mask"].copy_(st["mask0"])
            st["unfinished"].fill_(1)
            st["cnt"].zero_()
            st["seq"].fill_(self.end_idx)
            st["logprob"].zero_()
            self._memory(st)
            for t in range(max_length):
                self._steps(st, B, max_length, t, st["tok"], st["mask"], 0)
                if rule is None:
                    check(lib.ac_ens_greedy_pick(st["planes"], M, st["ldl"], B, V, t, max_length, self.end_idx, self.pad_idx,
                                                 ptr(st["seq"]), ptr(st["logprob"]), ptr(st["tok"]), ptr(st["mask"]),
                                                 ptr(st["unfinished"]), ptr(st["cnt"]), stream()), "ac_ens_greedy_pick")
                else:
                    check(lib.ac_ens_sample_pick(st["planes"], M, st["ldl"], B, V, rule[0], rule[1], rule[2], rule[3],
                                                 ptr(st["seed"]), t, max_length, self.end_idx, self.pad_idx, ptr(st["seq"]),
                                                 ptr(st["logprob"]), ptr(st["tok"]), ptr(st["mask"]), ptr(st["unfinished"]),
                                                 ptr(st["cnt"]), None, stream()), "ac_ens_sample_pick")

        search_state.run(st, dev, launch)
        return {"seq": st["seq"].cpu(), "sampled_logprob": st["logprob"].cpu()}

    # ---- beam search (ensemble.py:154-276), all clips batched ---------------------------------------------
    def _beam(self, encs, beam, max_length, temp, n_best, n_best_size):
        B, V, M = encs[0]["attn_emb"].shape[0], self.vocab_size, len(self.models)
        if not 1 <= beam <= 8:
            raise ValueError(f"ensemble beam search covers beam sizes 1..8 (got {beam})")
        if not (temp > 0 and np.isfinite(temp)):
            raise ValueError(f"beam search needs a finite temp > 0 (got {temp})")
        R, cap = B * beam, beam * max_length   # cap: every beam of every step may finish

        def build(dev):
            members, planes, ldl = self._member_buffers(encs, R, beam, max_length, dev)
            return {"members": members, "planes": planes, "ldl": ldl,
                    **search_state.beam_buffers(dev, B, beam, max_length, self.start_idx, self.end_idx, self.pad_idx),
                    "scratch": torch.empty(2 * R * beam, device=dev, dtype=torch.float32)}

        st, dev = self._state_for("beam", encs, (B, beam, max_length, temp), build)
        lib = _lib.load()
        tok = st["tok"]

        def launch():
            search_state.beam_reset(st, B)
            self._memory(st)
            for t in range(max_length):
                self._steps(st, R, max_length, t, tok[t & 1], st["mask"], t & 1)
                check(lib.ac_ens_beam_step_select(st["planes"], M, st["ldl"], B, beam, V, t, temp, ptr(st["cum"]),
                                                  ptr(st["top_val"]), ptr(st["top_idx"]), ptr(st["scratch"]), stream()),
                      "ac_ens_beam_step_select")
                search_state.beam_update(st, t, B, beam, V, max_length, self.end_idx, self.pad_idx, cap, all_rows=True)
                if t + 1 < max_length:
                    for m, b in zip(self.models, st["members"]):   # every member re-gathers its own KV cache
                        check(lib.ac_trm_beam_reorder(ctypes.byref(m.decoder.weights()), R, max_length, t, ptr(st["src_row"]),
                                                      ptr(b["ws"]), stream()), "ac_trm_beam_reorder")

        search_state.run(st, dev, launch)
        seq, score = search_state.beam_rank(st, B, cap, max_length, self.end_idx, n_best, n_best_size)
        return {"seq": seq, "sampled_logprob": torch.zeros(B, max_length), "score": score}
