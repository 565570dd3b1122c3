"""Cnn8-RNN sound-event tagger, MI355X path.  Plugin-compatible with the reference class ``Cnn8rnnSedModel``
(captioning/models/hf_wrapper.py:1791-1859) in eval mode: the same constructor, the same sub-module names (a reference
``state_dict`` loads with ``strict=True``), ``forward_prob(lms)`` -> ``segmentwise_output`` / ``framewise_output`` and
``forward(lms)`` -> a list of temporal tags 0..3, one per clip - what ``TemporalBahAttnDecoder`` embeds at step 0.

The torch.nn sub-modules only OWN the parameters.  The forward pass is

    bn0 -> 4 x (conv3x3 + BN + ReLU, conv3x3 + BN + ReLU, avg + max pool)   the Cnn14 conv kernels in mode 0 + ac_pool_avgmax
        -> mean over mel -> fc1 + ReLU -> bi-GRU -> fc_audioset             K.linear, ac_gru_layer
        -> clamp(sigmoid)                                                   ac_sed_head
        -> double threshold + segment pair rule                             ac_sed_temporal_tag (no host post-processing)

on the row-padded channels-last layout of ``Cnn14Encoder`` with two time halvings instead of five: blocks 1 and 2 pool
(2, 2), blocks 3 and 4 pool (1, 2) and stay at T // 4 rows.  ``forward_wav`` is the product path: log-mel with this model's
bn0 folded in (``K.logmel``), then the same stack, tags left on the device.
"""
import os

import torch
import torch.nn as nn

from . import kernels as K
from .cnn_encoder import ConvBlock, conv_tier
from .mel import MelTables

SED_CHANNELS = [1, 64, 128, 256, 512]
POOL_TIME = [2, 2, 1, 1]   # time factor of each block's (ph, 2) pool


class Cnn8rnnSedModel(nn.Module):

    def __init__(self, classes_num, sample_rate=32000):
        super().__init__()
        self.time_resolution = 0.01
        self.interpolate_ratio = 4     # the two (2, 2) pools
        self.classes_num = classes_num
        self.bn0 = nn.BatchNorm2d(64)
        for b in range(4):
            setattr(self, f"conv_block{b + 1}", ConvBlock(SED_CHANNELS[b], SED_CHANNELS[b + 1]))
        self.fc1 = nn.Linear(512, 512, bias=True)
        self.rnn = nn.GRU(512, 256, bidirectional=True, batch_first=True)
        self.fc_audioset = nn.Linear(512, classes_num, bias=True)
        # the mel front-end of ``forward_wav`` (the reference computes the log-mel outside this class, hf_wrapper.py:1951-1954)
        self.sample_rate = sample_rate
        self.n_fft, self.hop_length = 32 * sample_rate // 1000, 10 * sample_rate // 1000
        self.f_min, self.f_max = 50.0, float({32000: 14000, 16000: 8000}[sample_rate])
        self.conv_algo = os.environ.get("AUDIOCAPTION_CONV_ALGO", "wino43")   # a name of ``cnn_encoder.TIERS``
        self.high_thres, self.low_thres, self.n_connect = 0.75, 0.25, 1       # hf_wrapper.py:1813-1814
        self._packed = {}
        self._bufs = {}
        self._tables = None
        self._tag_ws = None
        self.last_preact = None   # fc_audioset's output before the sigmoid, (B, T // 4, classes) - kept for the tests

    # ---- geometry ----------------------------------------------------------------------------------------------------
    def geometry(self, frames):
        """Valid (H) and physical (Hp) row counts of the 3 time resolutions T, T // 2, T // 4 (``Cnn14Encoder.geometry``
        with two halvings): the last level is a multiple of 4 and exceeds its H, so no row quad of F(4,3) and no pooling pair
        straddles two clips."""
        H = [frames >> k for k in range(3)]
        if H[2] < 1:
            raise ValueError(f"clips of {frames} frames are shorter than one tagger segment (4 frames)")
        hp2 = (H[2] + 4) & ~3
        return H, [hp2 << (2 - k) for k in range(3)]

    def effective_algo(self, algo=None):
        """The conv tier a call runs on: the pooling kernel reads f32, so a tier with half-precision activations hands over
        to its declared fallback."""
        algo = algo or self.conv_algo
        tier = conv_tier(algo)
        if tier.act != torch.float32:
            if tier.fallback is None:
                raise ValueError(f"conv tier {algo!r} keeps no f32 activations and declares no fallback")
            return tier.fallback
        return algo

    # ---- packed weights (cached; invalidated by in-place updates, checkpoint loads and .to()) --------------------------
    def _pack(self, algo):
        tier = conv_tier(algo)
        layers = [(b, conv, bn) for b, blk in enumerate(getattr(self, f"conv_block{b + 1}") for b in range(4))
                  for conv, bn in ((blk.conv1, blk.bn1), (blk.conv2, blk.bn2))]
        tensors = [self.bn0.weight, self.bn0.bias, self.bn0.running_mean, self.bn0.running_var]
        for _, conv, bn in layers:
            tensors += [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        tensors += list(self.rnn.parameters())
        key = tuple((t.data_ptr(), t._version, K._lib.tensor_generation(t)) for t in tensors) + (algo,)
        hit = self._packed.get(algo)
        if hit is not None and hit[0] == key:
            return hit[1]

        def fold(bn):
            return K.fold_bn(bn.weight.float(), bn.bias.float(), bn.running_mean.float(), bn.running_var.float(), bn.eps)

        with torch.no_grad():
            pk = {"bn0": fold(self.bn0), "convs": []}
            for i, (b, conv, bn) in enumerate(layers):
                w = conv.weight.detach().float()
                if i == 0:   # one input channel: the 64 x 9 array ``K.conv3x3_first`` reads
                    wp, inv = w.reshape(64, 9).contiguous(), None
                else:
                    wp, inv = tier.pack(w, b, conv.weight)
                sc, sh = fold(bn)
                if inv is not None:
                    sc = (sc * inv).contiguous()
                pk["convs"].append((wp, sc, sh))
            ps = dict(self.rnn.named_parameters())
            whh = torch.stack([ps["weight_hh_l0"], ps["weight_hh_l0_reverse"]], 0).float().contiguous()
            pk["gru"] = ([ps["weight_ih_l0"].float().contiguous(), ps["weight_ih_l0_reverse"].float().contiguous()],
                         [ps["bias_ih_l0"].float().contiguous(), ps["bias_ih_l0_reverse"].float().contiguous()],
                         K.gru_pack_whh(whh, 256),
                         torch.stack([ps["bias_hh_l0"], ps["bias_hh_l0_reverse"]], 0).float().contiguous())
        self._packed[algo] = (key, pk)
        return pk

    def _buf(self, name, numel, device):
        b = self._bufs.get(name)
        if b is None or b.numel() < numel or b.device != device:
            b = torch.empty(numel, device=device, dtype=torch.float32)
            self._bufs[name] = b
        return b

    # ---- the stack -----------------------------------------------------------------------------------------------------
    def conv_stack(self, x0, B, H, Hp, pk, algo, blocks=None):
        """bn0-normalised log-mel x0 [B*Hp[0]][64] (rows >= H[0] zero) -> (B, H[2], 512): the mean over mel of block 4.
        ``blocks``: a list that receives a float32 (B, C, H, W) copy of every pooled block output (tests)."""
        dev = x0.device
        tier = conv_tier(algo)
        a = self._buf("conv1", B * Hp[0] * 64 * 64, dev)        # conv1 outputs (largest: block 1)
        c = self._buf("conv2", B * Hp[0] * 64 * 64, dev)        # conv2 outputs
        pooled = [self._buf("pool_a", B * Hp[1] * 32 * 64, dev), self._buf("pool_b", B * Hp[2] * 16 * 128, dev)]
        offer = {"workspace": lambda n: self._buf("w1_splitk", n, dev)}
        W, lvl, src = 64, 0, x0
        for b in range(4):
            cin, cout = SED_CHANNELS[b], SED_CHANNELS[b + 1]
            w1, s1, t1 = pk["convs"][2 * b]
            w2, s2, t2 = pk["convs"][2 * b + 1]
            if b == 0:
                K.conv3x3_first(src, w1, s1, t1, a, B, Hp[0], H[0], W)
            else:
                tier.launch(src, w1, s1, t1, a, B, Hp[lvl], H[lvl], W, cin, cout, 0, **offer)
            tier.launch(a, w2, s2, t2, c, B, Hp[lvl], H[lvl], W, cout, cout, 0, **offer)
            ph = POOL_TIME[b]
            if b == 3:
                feat = torch.empty(B, H[lvl], cout, device=dev, dtype=torch.float32)
                K.pool_avgmax(c, feat, B, Hp[lvl], H[lvl], W, cout, 1, mean_w=True)
                if blocks is not None:
                    blocks.append(feat.clone())
                return feat
            nxt = lvl + (ph == 2)
            dst = pooled[b & 1]
            K.pool_avgmax(c, dst, B, Hp[lvl], H[lvl], W, cout, ph, Hp_out=Hp[nxt])
            W //= 2
            if blocks is not None:
                blk = dst[:B * Hp[nxt] * W * cout].reshape(B, Hp[nxt], W, cout)[:, :H[nxt]]
                blocks.append(blk.permute(0, 3, 1, 2).clone())
            src, lvl = dst, nxt

    def _head(self, feat, pk):
        """(B, S, 512) -> segment-wise probabilities (B, S, classes): fc1 + ReLU, the bi-GRU over all S steps of every clip
        (the reference passes no lengths), fc_audioset, clamp(sigmoid)."""
        B, S, _ = feat.shape
        dev = feat.device
        h = K.linear(feat.reshape(B * S, 512), self.fc1.weight.float(), self.fc1.bias.float(), relu=True)
        w_ih, b_ih, whhT, bhh = pk["gru"]
        # (B*S, 2 x 3 x 256): all steps; one product per direction - a 768 x 512 layer stays on the exact-f32 GEMM
        # (``K.linear`` picks the arithmetic by the layer's size), which the 1e-4 gate on the class logits wants: the head
        # multiplies what the recurrence carries by class rows several units long
        gx = torch.empty(B * S, 1536, device=dev, dtype=torch.float32)
        for d in range(2):
            K.linear(h, w_ih[d], b_ih[d], out=gx[:, d * 768:(d + 1) * 768])
        lens = torch.full((B,), S, device=dev, dtype=torch.int32)
        h = K.gru_layer(gx, whhT, bhh, lens, B, S, 256).reshape(B * S, 512)
        x = K.linear(h, self.fc_audioset.weight.float())     # the bias is added by the head kernel
        pre = torch.empty_like(x)
        prob = K.sed_head(x, self.fc_audioset.bias.float(), pre=pre)
        self.last_preact = pre.reshape(B, S, -1)
        return prob.reshape(B, S, -1)

    def _check_mode(self):
        if self.training:
            raise NotImplementedError("Cnn8rnnSedModel (HIP path): inference only - call .eval(); the tagger's train-mode "
                                      "forward (dropout, batch statistics) and its backward are not built")

    def _segmentwise(self, x0, B, frames, algo=None, blocks=None):
        algo = self.effective_algo(algo)
        H, Hp = self.geometry(frames)
        pk = self._pack(algo)
        return self._head(self.conv_stack(x0, B, H, Hp, pk, algo, blocks=blocks), pk)

    def _x0_from_lms(self, lms, algo=None):
        if lms.dim() != 3 or lms.shape[1] != 64:
            raise ValueError("lms must be (batch, 64 mel bins, frames)")
        K._dev(lms)
        B, _, T = lms.shape
        Hp0 = self.geometry(T)[1][0]
        scale, shift = self._pack(self.effective_algo(algo))["bn0"]
        x0 = torch.zeros(B, Hp0, 64, device=lms.device, dtype=torch.float32)
        x0[:, :T] = lms.float().transpose(1, 2) * scale + shift     # bn0 over the mel axis (hf_wrapper.py:1830-1832)
        return x0.reshape(B * Hp0, 64)

    def forward_prob(self, lms, algo=None, blocks=None):
        """lms (B, 64, T) on the device -> {"segmentwise_output": (B, T // 4, C), "framewise_output": (B, T, C)}."""
        self._check_mode()
        B, _, T = lms.shape
        seg = self._segmentwise(self._x0_from_lms(lms, algo), B, T, algo, blocks)
        frame = seg.repeat_interleave(self.interpolate_ratio, dim=1)              # interpolate, hf_wrapper.py:54-68
        if frame.shape[1] < T:                                                     # pad_framewise_output, :70-87
            frame = torch.cat([frame, seg[:, -1:].expand(B, T - frame.shape[1], seg.shape[2])], dim=1)
        return {"segmentwise_output": seg, "framewise_output": frame}

    def tags_of(self, segmentwise, frames):
        """Segment-wise probabilities (B, S, C) -> int32 device tensor (B,) of temporal tags."""
        tags, self._tag_ws = K.sed_temporal_tag(segmentwise, frames, self.interpolate_ratio, self.high_thres, self.low_thres,
                                                self.n_connect, self.time_resolution, 0.5, workspace=self._tag_ws)
        return tags

    def forward(self, lms):
        """lms (B, 64, T) -> list of B ints (the reference's return value, hf_wrapper.py:1810-1818)."""
        self._check_mode()
        B, _, T = lms.shape
        seg = self._segmentwise(self._x0_from_lms(lms), B, T)
        return self.tags_of(seg, T).tolist()

    def forward_wav(self, wav, tables=None):
        """wav (B, L) on the device -> int32 device tensor (B,) of temporal tags.  ``tables``: the ``MelTables`` of the
        caller's mel front-end (default: this model's sample rate, torchaudio's window and slaney filterbank)."""
        self._check_mode()
        if wav.dim() != 2:
            raise ValueError("wav must be (batch, samples)")
        dev = wav.device
        if tables is None:
            if self._tables is None or self._tables.window.device != dev:
                self._tables = MelTables(self.sample_rate, self.n_fft, self.hop_length, self.f_min, self.f_max, 64, "slaney",
                                         "slaney", dev)
            tables = self._tables
        B, L = wav.shape
        T = L // tables.hop + 1
        Hp0 = self.geometry(T)[1][0]
        scale, shift = self._pack(self.effective_algo())["bn0"]
        x0 = K.logmel(wav, tables, scale, shift, rows_per_clip=Hp0, channels_last=True)
        return self.tags_of(self._segmentwise(x0, B, T), T)
