"""HTS-AT audio encoder, MI355X path.  Plugin-compatible with the reference class
``captioning.models.transformer_encoder.Htsat`` (transformer_encoder.py:679-996): same constructor, same
``forward(input_dict) -> {"fc_emb", "attn_emb", "attn_emb_len", "layer_0" .. "layer_3"}`` contract, same ``state_dict()``
keys (``patch_embed.*``, ``layers.S.blocks.K.*`` with the ``relative_position_index`` / ``attn_mask`` buffers,
``layers.S.downsample.*``, ``norm.*``, ``bn0.*``, ``melspec_extractor.*``), same ``load_pretrained`` hook (WavCaps layout).

Inference (``eval()``) only.  The torch.nn sub-modules below only OWN the parameters and buffers; the forward never calls
them: log-mel + bn0 (csrc/logmel.hip) -> bicubic stretch + fold + patch embedding -> four stages of Swin blocks ((shifted-)
window attention, exact-GELU MLP) with patch merging between them -> final LayerNorm -> frequency / time pooling, in the
kernels of csrc/htsat.hip with the linear layers on ``ac_gemm_bf16x3``, and fails loudly if the library is
unavailable.

Supported: the constructor defaults with any four ``depths`` and ``sample_rate`` 32000 or 16000; the dropout / drop-path
rates, ``use_checkpoint`` and ``freeze`` are accepted as they are (identity, or without effect, in eval mode).  Any other
value raises ``NotImplementedError`` naming the argument.
"""
import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from ._lib import check, f32c, ptr, stream
from .mel import MelSpectrogramBuffers, MelTables

WINDOW = 8
HEAD_DIM = 24
FRAMES = 1024          # time frames of the folded image (spec_size * freq_ratio)
GRID = 64              # tokens per image side
MIN_FRAMES = 32        # one output frame: 8 (patch stride x three mergings along the folded axis) x 4 chunks


def relative_position_index(window=WINDOW):
    """(window^2, window^2) int64: row of the bias table for every (query, key) pair of a window
    (transformer_encoder.py:390-401): (dh + window - 1) * (2 window - 1) + dw + window - 1."""
    r = torch.arange(window)
    hh, ww = r.repeat_interleave(window), r.repeat(window)
    dh = hh[:, None] - hh[None, :] + window - 1
    dw = ww[:, None] - ww[None, :] + window - 1
    return dh * (2 * window - 1) + dw


def shifted_window_mask(H, W, window=WINDOW, shift=WINDOW // 2):
    """(windows, window^2, window^2) float32: 0 between tokens of the same region of the rolled image, -100 otherwise
    (transformer_encoder.py:500-519)."""
    def region(n):
        i = torch.arange(n)
        return (i >= n - window).long() + (i >= n - shift).long()

    ids = region(H)[:, None] * 3 + region(W)[None, :]
    ids = ids.view(H // window, window, W // window, window).permute(0, 2, 1, 3).reshape(-1, window * window)
    return (ids[:, None, :] != ids[:, :, None]).float() * -100.0


class PatchEmbed(nn.Module):
    def __init__(self, embed_dim):
        super().__init__()
        self.proj = nn.Conv2d(1, embed_dim, kernel_size=4, stride=4)
        self.norm = nn.LayerNorm(embed_dim)


class WindowAttention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * WINDOW - 1) ** 2, num_heads))
        self.register_buffer("relative_position_index", relative_position_index())
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, resolution, num_heads, shift):
        super().__init__()
        self.dim, self.input_resolution, self.num_heads = dim, resolution, num_heads
        # a stage no larger than the window is one unshifted window (transformer_encoder.py:479-482)
        self.shift_size = 0 if min(resolution) <= WINDOW else shift
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, num_heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, dim * 4)
        self.register_buffer("attn_mask", shifted_window_mask(*resolution, shift=self.shift_size) if self.shift_size else None)


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)


class BasicLayer(nn.Module):
    def __init__(self, dim, resolution, depth, num_heads, downsample):
        super().__init__()
        self.dim, self.input_resolution, self.depth = dim, resolution, depth
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, resolution, num_heads, 0 if i % 2 == 0 else WINDOW // 2)
                                     for i in range(depth)])
        self.downsample = PatchMerging(dim) if downsample else None


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class Htsat(nn.Module):

    def __init__(self, sample_rate=32000, freeze=False, spec_size=256, patch_size=4, patch_stride=(4, 4), in_chans=1,
                 embed_dim=96, depths=[2, 2, 6, 2], num_heads=[4, 8, 16, 32], window_size=8, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False,
                 patch_norm=True, use_checkpoint=False, norm_before_mlp="ln"):
        super().__init__()
        refused = [("sample_rate", sample_rate in (32000, 16000)), ("spec_size", _pair(spec_size) == (256, 256)),
                   ("patch_size", _pair(patch_size) == (4, 4)), ("patch_stride", _pair(patch_stride) == (4, 4)),
                   ("in_chans", in_chans == 1), ("embed_dim", embed_dim == 96), ("depths", len(depths) == 4 and min(depths) >= 1),
                   ("num_heads", list(num_heads) == [4, 8, 16, 32]), ("window_size", window_size == WINDOW),
                   ("mlp_ratio", float(mlp_ratio) == 4.0), ("qkv_bias", bool(qkv_bias)), ("qk_scale", qk_scale is None),
                   ("norm_layer", norm_layer is nn.LayerNorm), ("ape", not ape), ("patch_norm", bool(patch_norm)),
                   ("norm_before_mlp", norm_before_mlp == "ln")]
        for name, ok in refused:
            if not ok:
                raise NotImplementedError(
                    f"Htsat (HIP path): {name} = {locals()[name]!r} is not built; supported are the reference's defaults "
                    "(spec_size 256, patch 4 / stride (4, 4), in_chans 1, embed_dim 96, heads (4, 8, 16, 32), window 8, "
                    "mlp_ratio 4, qkv_bias, LayerNorm, ape=False, patch_norm=True, norm_before_mlp='ln') with any four depths "
                    "and sample_rate 32000 or 16000")
        self.sample_rate = sample_rate
        self.embed_dim, self.depths, self.num_heads = embed_dim, list(depths), list(num_heads)
        self.num_features = embed_dim * 8
        self.fc_emb_size = self.num_features
        self.freq_ratio = 4
        self.n_fft = 32 * sample_rate // 1000
        self.hop_length = 10 * sample_rate // 1000
        self.f_min, self.f_max = 50.0, float({32000: 14000, 16000: 8000}[sample_rate])
        self.melspec_extractor = MelSpectrogramBuffers(sample_rate, self.n_fft, self.f_min, self.f_max, 64, "slaney", "slaney")
        self.bn0 = nn.BatchNorm2d(64)
        self.patch_embed = PatchEmbed(embed_dim)
        self.layers = nn.ModuleList([BasicLayer(embed_dim << i, (GRID >> i, GRID >> i), self.depths[i], self.num_heads[i], i < 3)
                                     for i in range(4)])
        self.norm = nn.LayerNorm(self.num_features)
        for m in self.modules():   # transformer_encoder.py:835-842
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        if freeze:
            for p in self.parameters():
                p.requires_grad = False
        self._tables, self._tables_key = None, None
        self._packed = None     # (key of the tensors it was packed from, pack)
        self._bufs = {}

    # ---- checkpoint hook (transformer_encoder.py:844-860: the WavCaps HTS-AT layout) ----------------------------------
    def load_pretrained(self, pretrained, output_fn=print):
        from .config import merge_load_state_dict
        checkpoint = pretrained if isinstance(pretrained, dict) else torch.load(pretrained, map_location="cpu")
        prefix = "encoder.audio_enc."
        sd = checkpoint.get("model") if isinstance(checkpoint, dict) else None
        if not isinstance(sd, dict) or not sd or not next(iter(sd)).startswith(prefix):
            raise ValueError("Htsat.load_pretrained: unknown checkpoint layout; expected the WavCaps layout, a 'model' dict "
                             f"whose keys start with '{prefix}'")
        loaded = set(merge_load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, self,
                                           output_fn))
        for name, param in self.named_parameters():
            param.requires_grad = name not in loaded

    # ---- cached packs and buffers ------------------------------------------------------------------------------------
    def _pack(self):
        tensors = list(self.parameters()) + list(self.buffers())
        key = tuple((t.data_ptr(), t._version, _lib.tensor_generation(t)) for t in tensors)
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]

        def f(t):
            return t.detach().float().contiguous()

        with torch.no_grad():
            pe = self.patch_embed
            pk = {"bn0": K.fold_bn(f(self.bn0.weight), f(self.bn0.bias), f(self.bn0.running_mean), f(self.bn0.running_var),
                                   self.bn0.eps),
                  "embed": (f(pe.proj.weight).reshape(-1, 16).contiguous(), f(pe.proj.bias), f(pe.norm.weight), f(pe.norm.bias)),
                  "norm": (f(self.norm.weight), f(self.norm.bias)), "stages": []}
            for layer in self.layers:
                blocks = []
                for blk in layer.blocks:
                    a = blk.attn
                    # [heads][64][64], gathered from the table once per pack (transformer_encoder.py:424-427)
                    bias = f(a.relative_position_bias_table)[a.relative_position_index.reshape(-1)]
                    bias = bias.view(WINDOW * WINDOW, WINDOW * WINDOW, -1).permute(2, 0, 1).contiguous()
                    blocks.append({"shift": blk.shift_size, "bias": bias,
                                   "norm1": (f(blk.norm1.weight), f(blk.norm1.bias)), "norm2": (f(blk.norm2.weight), f(blk.norm2.bias)),
                                   "qkv": (f(a.qkv.weight), f(a.qkv.bias)), "proj": (f(a.proj.weight), f(a.proj.bias)),
                                   "fc1": (f(blk.mlp.fc1.weight), f(blk.mlp.fc1.bias)),
                                   "fc2": (f(blk.mlp.fc2.weight), f(blk.mlp.fc2.bias))})
                ds = layer.downsample
                merge = None if ds is None else (f(ds.norm.weight), f(ds.norm.bias), f(ds.reduction.weight))
                pk["stages"].append({"blocks": blocks, "merge": merge})
        self._packed = (key, pk)
        return pk

    def _buf(self, name, numel, device):
        b = self._bufs.get(name)
        if b is None or b.numel() < numel or b.device != device:
            b = torch.empty(numel, device=device, dtype=torch.float32)
            self._bufs[name] = b
        return b

    def _ensure_tables(self, dev):
        mkey = self.melspec_extractor.key()
        if self._tables is None or self._tables.window.device != dev or self._tables_key != mkey:
            self._tables = MelTables(self.sample_rate, self.n_fft, self.hop_length, self.f_min, self.f_max, 64, "slaney",
                                     "slaney", dev, window=self.melspec_extractor.spectrogram.window,
                                     fb=self.melspec_extractor.mel_scale.fb)
            self._tables_key = mkey

    def _linear(self, x, w, b, y, M, beta=0.0):
        """y[M][N] = x[M][K] w[N][K]^T + b (+ beta * y: the residual) on split-bf16 operands (2^-16 operand error, f32
        accumulation; the library forwards small products to the exact kernels): within 3.5e-6 of the reference at every
        stage against 8e-7 on the exact-f32 GEMM, which took 13.3 instead of 10.5 ms per 64 clips."""
        N, Kd = w.shape
        check(_lib.load().ac_gemm_bf16x3(ptr(x), Kd, 1, ptr(w), 1, Kd, ptr(y), N, M, N, Kd, ptr(b), 0, beta, 1, 0.0, 0, None, 0,
                                         None, 0, stream()), "ac_gemm_bf16x3")

    @staticmethod
    def _check_frames(T):
        if T > FRAMES:
            raise ValueError(f"Htsat: {T} frames exceed the {FRAMES} the folded image holds (the reference asserts, "
                             "transformer_encoder.py:937)")
        if T < MIN_FRAMES:
            raise ValueError(f"Htsat: clips of {T} frames are shorter than one output frame ({MIN_FRAMES} frames)")

    # ---- the network on bn0-normalised log-mel rows ----------------------------------------------------------------
    def features(self, x0, B, T, stage_tokens=None):
        """x0: bn0-normalised log-mel rows [B][T][64] f32 (``K.logmel``'s rows layout), T <= 1024 frames of the padded batch
        -> {"attn_emb" (B, 32, 768), "fc_emb" (B, 768), "layer_0" .. "layer_3"}.  ``stage_tokens`` (tests): a list that
        receives a copy of the tokens after the patch embedding and after every stage."""
        self._check_frames(T)
        lib = _lib.load()
        dev, s = x0.device, stream()
        pk = self._pack()
        C, H = self.embed_dim, GRID
        n0 = B * GRID * GRID * C                   # the residual stream at its largest: a merge quarters the tokens, doubles the width
        x = self._buf("x", n0, dev)
        y = self._buf("y", n0, dev)
        ctx = self._buf("ctx", n0, dev)
        wide = self._buf("wide", 4 * n0, dev)      # qkv (3C) and the MLP's hidden layer (4C)
        w, b, lw, lb = pk["embed"]
        check(lib.ac_htsat_patch_embed(ptr(x0), B, T, ptr(w), ptr(b), ptr(lw), ptr(lb), ptr(x), C, s), "ac_htsat_patch_embed")
        if stage_tokens is not None:
            stage_tokens.append(x[:B * H * H * C].view(B, H * H, C).clone())
        out = {}
        for i, stage in enumerate(pk["stages"]):
            rows = B * H * H
            for blk in stage["blocks"]:
                K.add_layernorm(x[:rows * C].view(rows, C), None, *blk["norm1"], out=y[:rows * C].view(rows, C))
                self._linear(y, *blk["qkv"], wide, rows)
                check(lib.ac_swin_window_attn(ptr(wide), ptr(blk["bias"]), ptr(ctx), B, H, H, C, C // HEAD_DIM, blk["shift"], s),
                      "ac_swin_window_attn")
                self._linear(ctx, *blk["proj"], x, rows, beta=1.0)
                K.add_layernorm(x[:rows * C].view(rows, C), None, *blk["norm2"], out=y[:rows * C].view(rows, C))
                self._linear(y, *blk["fc1"], wide, rows)
                check(lib.ac_gelu(ptr(wide), ptr(wide), rows * 4 * C, s), "ac_gelu")
                self._linear(wide, *blk["fc2"], x, rows, beta=1.0)
            if stage["merge"] is not None:
                lw, lb, red = stage["merge"]
                check(lib.ac_swin_patch_merge(ptr(x), ptr(lw), ptr(lb), ptr(wide), B, H, H, C, s), "ac_swin_patch_merge")
                H //= 2
                rows = B * H * H
                self._linear(wide, red, None, x, rows)
                C *= 2
                emb = torch.empty(B, C, device=dev, dtype=torch.float32)
                check(lib.ac_htsat_token_mean(ptr(x), ptr(emb), B, H * H, C, s), "ac_htsat_token_mean")
                out[f"layer_{i}"] = emb
            if stage_tokens is not None:
                stage_tokens.append(x[:B * H * H * C].view(B, H * H, C).clone())
        rows = B * H * H
        K.add_layernorm(x[:rows * C].view(rows, C), None, *pk["norm"], out=y[:rows * C].view(rows, C))
        fbins = H // self.freq_ratio
        attn = torch.empty(B, (H // fbins) * H, C, device=dev, dtype=torch.float32)
        fc = torch.empty(B, C, device=dev, dtype=torch.float32)
        check(lib.ac_htsat_pool(ptr(y), ptr(attn), ptr(fc), B, H, H, C, fbins, s), "ac_htsat_pool")
        out["layer_3"] = fc
        return dict({"fc_emb": fc, "attn_emb": attn}, **out)

    def features_from_logmel(self, lms, stage_tokens=None):
        """Test hook: a log-mel (B, T, 64) in dB in place of the waveform (the golden starts downstream of the mel front
        end, which is pinned elsewhere); bn0 is applied here with torch."""
        if not lms.is_cuda:
            raise _lib.HipLibraryError("the HIP path needs tensors on a ROCm device; there is no CPU fallback")
        pk = self._pack()
        B, T, _ = lms.shape
        x0 = (lms.float() * pk["bn0"][0] + pk["bn0"][1]).contiguous()
        return self.features(x0, B, T, stage_tokens=stage_tokens)

    def forward(self, input_dict):
        if self.training:
            raise NotImplementedError(
                "Htsat (HIP path): inference only; train mode (SpecAugment, dropout, drop-path and the backward through the "
                "Swin blocks) is not built - call eval()")
        wav = input_dict["wav"]
        if wav.dim() != 2:
            raise ValueError("wav must be (batch, samples)")
        B, L = wav.shape
        T = L // self.hop_length + 1
        self._check_frames(T)
        if not wav.is_cuda:
            raise _lib.HipLibraryError("the HIP path needs tensors on a ROCm device; there is no CPU fallback")
        wav = f32c(wav)
        self._ensure_tables(wav.device)
        pk = self._pack()
        x0 = K.logmel(wav, self._tables, pk["bn0"][0], pk["bn0"][1], rows_per_clip=T, channels_last=True)
        out = self.features(x0, B, T)
        out["attn_emb_len"] = htsat_feat_len(input_dict["wav_len"], self.hop_length)
        return out


def htsat_feat_len(wav_len, hop):
    """attn_emb_len = (floor(L / hop) + 1) // 8 // 4 as a CPU int64 tensor (transformer_encoder.py:991-995)."""
    wav_len = torch.as_tensor(wav_len).cpu()
    n = torch.div(wav_len, hop, rounding_mode="floor") + 1
    return torch.div(torch.div(n, 8, rounding_mode="floor"), 4, rounding_mode="floor").long()
