"""Training of the attention-GRU captioners (``Seq2SeqAttnModel`` / ``TemporalSeq2SeqAttnModel`` over ``CrnnEncoder``) on
the MI355X path: ``TrainEngine`` with the decoder half replaced.

The encoder half is the engine's own - the frozen Cnn14 forward, the 3-layer bi-GRU forward with saved gates
(``_launch_forward_gru``) and its backward through time from ``gru_dout`` (``_launch_backward_gru``), ``FlatParams``, the
``_cnn_attn`` test hook - under the engine's own limits: ``freeze_cnn=True``, ``freeze_cnn_bn=True``, GRU hidden 256.
Between the two sits the decoder of csrc/attn_gru_train.hip (``rnn_decoder.BahAttnCatFcDecoder.train_forward`` /
``train_backward``): ``fc_emb`` is the mean of the GRU output over each clip's valid frames (``ac_mean_with_lens``), and in
the backward the decoder's ``d fc_emb`` goes back into every valid frame (``ac_bah_mean_lens_bwd``) on top of its
``d attn_emb``; the total lands in ``gru_dout``.  ``forward`` returns that ``fc_emb`` as well, and a gradient arriving on
it from outside the decoder (encoder-level distillation, enc_kd.py) is added to the decoder's ``d fc_emb`` first.

``model(input_dict)`` with ``mode="train"`` (``train_forward`` below) returns ``logit`` attached to autograd by one
bridge node, so the reference runner's ``loss.backward()``, ``clip_grad_norm_`` and any torch optimiser - or
``optim.FusedAdam`` - work unchanged.  The scheduled-sampling coins follow the reference (attn_model.py:44): one
``random.random()`` per step in step order, at ``ss_ratio == 1`` as well, all drawn on the host before anything is launched.

``AttnGruTrainEngine.rollout`` is the sampled rollout of self-critical sequence training with ``TrainEngine.rollout``'s
contract (``rl_model.ScstWrapper`` drives it): the same train-mode encoder, then ``max_length`` decoder steps with no
caption, each on the word the step before drew (``BahAttnCatFcDecoder.train_rollout``, ``ac_bah_train_rollout``).  It keeps
the state of a ``forward``, so ``backward`` and the bridge node work after it; it draws no scheduled-sampling coins.

``ConditionalSeq2SeqAttnModel`` trains the same way: its decoders take ``input_dict["condition"]`` (one float per clip,
checked in ``_prepare``) where the others take ``fc_emb``; they read no ``fc_emb``, so their ``d fc_emb`` is exactly zero.
``rollout`` is refused for it.

Not built for these models: the fused ``step`` (device-side loss, clip, Adam, graph capture, the split all-reduce), graph
capture or an early exit of the rollout, and the Cnn14 look-ahead.
"""
import math
import random

import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .rnn_decoder import check_condition, check_temporal_tag
from .train import H, OP_CNN_BLOCK, TrainEngine, _TrainBridgeFc


class AttnGruTrainEngine(TrainEngine):

    def _check_widths(self, model):
        from .attn_model import Seq2SeqAttnModel
        if not isinstance(model, Seq2SeqAttnModel):
            raise NotImplementedError("AttnGruTrainEngine trains Seq2SeqAttnModel / TemporalSeq2SeqAttnModel")
        dec = model.decoder
        if self.enc_kind != "rnn" or model.encoder.rnn.hidden_size != H:
            raise NotImplementedError("AttnGruTrainEngine: mode='train' needs a CrnnEncoder with freeze_cnn=True, "
                                      "freeze_cnn_bn=True and GRU hidden 256")
        if dec.attn_emb_dim != 2 * H or dec.fc_emb_dim != 2 * H:
            raise NotImplementedError(f"AttnGruTrainEngine: attn_emb_dim {dec.attn_emb_dim} / fc_emb_dim {dec.fc_emb_dim} do "
                                      f"not fit the bi-GRU's {2 * H} features")
        return 2 * H

    def _prepare(self, input_dict, rollout=False):
        T = input_dict["cap"].shape[1] - 1
        tags = None
        if self.model.decoder.n_tags:
            tags = check_temporal_tag(input_dict.get("temporal_tag"), input_dict["cap"].shape[0])
        # one coin per step, in step order, whatever ss_ratio is: the engine draws them unless ss_ratio == 1, where the
        # reference's attention model still consumes the stream (attn_model.py:44) and every coin comes out 1
        # (the SCST rollout takes no caption and draws no coins: ``rollout`` hands them over as ``_use_cap``)
        if input_dict["ss_ratio"] == 1 and not rollout:
            for _ in range(T):
                random.random()
        cond = None
        if self.model.decoder.variant:
            if rollout:
                raise NotImplementedError("AttnGruTrainEngine: the SCST rollout is not built for the condition-controlled "
                                          "decoders")
            cond = check_condition(input_dict.get("condition"), input_dict["cap"].shape[0])
        st = super()._prepare(input_dict, rollout)     # st["use_cap"]: the T coins
        st["cond"] = cond
        st["tags"] = None if tags is None else K.upload(tags, st["cap"].device, torch.int32)
        return st

    def _launch_forward(self, st, free=True):
        model, lib = self.model, self.lib
        enc, dec = model.encoder, model.decoder
        s = _lib.stream()
        self._phase = "forward"
        ws = st["ws"]
        N, Tq, p_cnn = st["N"], st["Tq"], st["p_cnn"]
        small = st["small"]
        self._seed_ptr = small.data_ptr()
        self._pw_pack_all(s)
        if st["cnn_attn_in"] is not None:
            cnn_attn = st["cnn_attn_in"]
        else:
            cnn_attn = enc.cnn.encode(st["wav"], dropout=(p_cnn, OP_CNN_BLOCK, self._seed_ptr) if p_cnn > 0 else None,
                                      specaug=st["specaug"], train=True)
        st["cnn_attn"] = cnn_attn
        st["gru"], _ = self._launch_forward_gru(st, cnn_attn)
        A = self.enc_width
        # the last GRU layer's output is the audio memory (no dropout behind the last layer); all T' frames are kept, the
        # frames beyond a clip's length are zero and masked
        attn_emb = ws.tensor(f"gru_out{enc.rnn.num_layers - 1}")[:N * Tq * A].view(N, Tq, A)
        lens = small[2:2 + N]
        ws.f("bah_fc", N, A)
        fc_emb = ws.tensor("bah_fc")[:N * A].view(N, A)
        check(lib.ac_mean_with_lens(attn_emb.data_ptr(), lens.data_ptr(), fc_emb.data_ptr(), N, Tq, A, 0, s),
              "ac_mean_with_lens")
        was = dec.training
        dec.training = not st["eval"]     # a model in eval(): every dropout probability 0, as TrainEngine does
        ro = st.get("rollout")
        try:
            if ro is None:
                st["bah"] = dec.train_forward(attn_emb, st["cond"] if dec.variant else fc_emb, lens, st["cap"],
                                              st["use_cap"], st.get("tags"),
                                              model.start_idx, seed_dev=self._seed_ptr)
            else:
                st["bah"] = dec.train_rollout(attn_emb, fc_emb, lens, st["T"], ro["temp"], ro["seed"], st.get("tags"),
                                              ro["forced"], model.start_idx, model.end_idx, seed_dev=self._seed_ptr)
        finally:
            dec.training = was

    def _outputs(self, st):
        out = {k: v for k, v in st["bah"].items() if k != "saved"}
        out["attn_emb_len"] = st["lens_host"]
        # the reference's memory is as long as the longest clip (pad_packed_sequence)
        out["attn_weight"] = out["attn_weight"][:, :int(st["lens_host"].max())]
        return out

    def _launch_fc_emb(self, st):
        N, A = st["N"], self.enc_width
        return st["ws"].tensor("bah_fc")[:N * A].view(N, A)     # the decoder's own input (``_launch_forward``)

    def _launch_backward(self, sv, dl, part="all", dfc=None):
        """``dfc`` (address, optional): d(loss)/d(fc_emb) from outside the decoder (encoder-level distillation), added to
        the decoder's own ``bah_dfc`` before it is spread over the frames; ``dl`` None: no gradient on ``logit`` - the
        decoder's backward is skipped, its gradients stay exactly zero."""
        if part != "all":
            raise NotImplementedError("AttnGruTrainEngine: the backward runs in one piece")
        lib, fp, dec = self.lib, self.flat, self.model.decoder
        s = _lib.stream()
        self._phase = "backward"
        ws = sv["ws"]
        N, Tq, A = sv["N"], sv["Tq"], self.enc_width
        fp.grad.zero_()
        self._seed_ptr = sv["small"].data_ptr()
        dout = ws.f("gru_dout", N * Tq, A)        # where _launch_backward_gru reads d(loss)/d(GRU output)
        d_fc = ws.f("bah_dfc", N, A)
        saved = sv.pop("bah")["saved"]
        if dl is not None:
            dec.train_backward(saved, dl, dec.grad_struct(lambda name: fp.g("decoder." + name)), dout, d_fc)
        else:
            ws.tensor("gru_dout")[:N * Tq * A].zero_()
            ws.tensor("bah_dfc")[:N * A].zero_()
        if dfc is not None:
            check(lib.ac_scatter_add_rows(dfc, self._clip_rows(sv), d_fc, N, A, s), "ac_scatter_add_rows(dfc_emb)")
        check(lib.ac_bah_mean_lens_bwd(d_fc, saved["len"].data_ptr(), dout, N, Tq, A, A, s), "ac_bah_mean_lens_bwd")
        self._launch_backward_gru(sv)

    def _clip_rows(self, sv):
        """0 .. N-1 on the device (the identity row table of the ``dfc_emb`` add), built once per batch shape."""
        if sv.get("clip_rows") is None:
            sv["clip_rows"] = torch.arange(sv["N"], dtype=torch.int32, device=sv["cap"].device)
        return sv["clip_rows"].data_ptr()

    def _launch_backward_fc(self, sv, dl, dfc):
        self._launch_backward(sv, dl, dfc=dfc)

    def rollout(self, input_dict):
        """The sampled rollout of self-critical sequence training, ``TrainEngine.rollout``'s contract: the train-mode encoder
        (frozen Cnn14 with its dropout and SpecAugment, the bi-GRU with saved gates; ``_cnn_attn`` honoured), ``fc_emb`` by
        ``ac_mean_with_lens``, then ``max_length`` decoder steps with no caption (``train_rollout``).  All steps always run.

        ``input_dict``: wav / wav_len / specaug as for mode "train", ``temporal_tag`` for the temporal model; ``max_length``
        (default the model's), ``temp`` (1.0); ``dropout_seed`` as in ``forward``; ``seed``: the sampler's 64-bit seed
        (default: the dropout seed of this call); ``_scst_words`` (parity hook, int64 N x T): these words instead of the
        draws, the finished-row rule still applies.  No ``cap`` is needed and no scheduled-sampling coin is drawn.
        Returns ``logit`` (N, T, V), ``seq`` (int64), ``seq_i32`` and ``sampled_logprob`` (N, T) on the device, and
        ``embed``, ``attn_weight``, ``state``, ``attn_emb_len`` as ``forward`` does; ``backward`` works as after ``forward``."""
        model = self.model
        if input_dict.get("n_samples") is not None:
            from .transformer_model import N_SAMPLES
            raise NotImplementedError(f"AttnGruTrainEngine.rollout: {N_SAMPLES} is not built for the SCST rollout")
        T = int(input_dict.get("max_length", model.max_length))
        temp = float(input_dict.get("temp", 1.0))
        if T < 1:
            raise ValueError("rollout: max_length must be at least 1")
        if not (math.isfinite(temp) and temp > 0):
            raise ValueError(f"rollout: temp must be finite and > 0, got {temp}")
        wav = input_dict["wav"]
        if not wav.is_cuda:
            raise _lib.HipLibraryError("the training step needs tensors on a ROCm device; there is no CPU fallback")
        N = wav.shape[0]
        cap = torch.zeros(N, T + 1, device=wav.device, dtype=torch.int64)    # never read: no step takes a caption word
        d = {k: v for k, v in input_dict.items() if k != "cap_len"}
        d.update(cap=cap, ss_ratio=0.0, _use_cap=[0] * T)
        base_seed = int(input_dict.get("dropout_seed", self.seed))
        state = random.getstate()     # TrainEngine._prepare draws a coin per step before it looks at _use_cap
        try:
            st = self._prepare(d, rollout=True)
        finally:
            random.setstate(state)
        seed = int(input_dict["seed"]) if input_dict.get("seed") is not None else base_seed
        forced = input_dict.get("_scst_words")
        if forced is not None:
            forced = torch.as_tensor(forced).to(device=wav.device, dtype=torch.int32).contiguous()
            if tuple(forced.shape) != (N, T):
                raise ValueError(f"_scst_words must be ({N}, {T})")
        ro = st.get("rollout")
        if ro is None:
            ro = st["rollout"] = {"seed": torch.zeros(1, device=wav.device, dtype=torch.int64)}
        from .sampling import seed_word
        ro["seed"].copy_(torch.tensor([seed_word(seed & 0xFFFFFFFFFFFFFFFF)], dtype=torch.int64))   # read on the device
        ro.update(temp=temp, forced=forced)
        self._launch_forward(st)
        self._saved = st
        return self._outputs(st)

    def step(self, *args, **kwargs):
        raise NotImplementedError("AttnGruTrainEngine: the fused step (device-side loss, clip, Adam, graph capture) covers "
                                  "TransformerModel only; use model(input_dict) with loss.backward() and an optimiser")

    def prefetch_cnn(self, input_dict, seed):
        raise NotImplementedError("AttnGruTrainEngine: the Cnn14 look-ahead belongs to the fused step")


def train_forward(model, input_dict):
    """``Seq2SeqAttnModel.forward`` for ``mode == "train"``."""
    from .crnn_trm_encoder import CrnnEncoder
    if not isinstance(model.encoder, CrnnEncoder):
        raise NotImplementedError(f"{type(model).__name__}: mode='train' is on the HIP path over a CrnnEncoder only (frozen "
                                  f"Cnn14 + bi-GRU), not over {type(model.encoder).__name__}")
    engine = getattr(model, "_train_engine", None)
    if engine is None:
        engine = model._train_engine = AttnGruTrainEngine(model)
    out = engine.forward(input_dict)
    out["seq"] = out["seq"].cpu()                            # the reference keeps seq and sampled_logprob on the CPU
    out["sampled_logprob"] = out["sampled_logprob"].cpu()
    # a model in eval() or under no_grad: plain logits, no bridge node
    if model.training and torch.is_grad_enabled():
        out["logit"], out["fc_emb"] = _TrainBridgeFc.apply(engine, out["logit"], out["fc_emb"], *engine.flat.params)
    return out
